// GPU half of the baseline-JPEG decoder (include/mmrca_jpeg.h; the host half is jpeg_entropy.cpp): a batch of int16 coefficient
// blocks -> uint8 HWC RGB in the staging layout of preprocess.hip.  Integer arithmetic of libjpeg throughout (jidctint.c "islow",
// jdsample.c "fancy" upsampling, jdcolor.c), so the bytes equal libjpeg-turbo's; tests/jpeg_ref.py is the int64 NumPy mirror.
//
//   jpeg_idct_k   8 lanes per 8x8 block, 32 blocks per workgroup.  Lane j loads coefficient row j (one 16-byte load, consecutive
//                 lanes -> consecutive addresses), dequantises it, and the block goes through LDS twice: columns (descale 11), then
//                 rows (descale 18, +128, clamp).  Lane j stores sample row j (8 bytes) over the first half of the block's own
//                 coefficients: no plane buffer, and the second kernel reads 64-byte blocks that the first left in L2.
//   jpeg_rgb_k    16 pixels = 48 bytes = three aligned 16-byte stores per thread, pixels numbered across rows so that every store
//                 but an image's last is full; the tail is stored byte by byte and the alignment gap after it is not touched.
// Both are bound by bytes (2 B read per coefficient, 3 B written per pixel), not by the few dozen integer operations per sample.
#include "common.h"
#include "../../include/mmrca_jpeg.h"

static_assert(sizeof(MmrcaJpegDesc) == 464, "MmrcaJpegDesc layout (jpeg.py::DESC_DTYPE mirrors it)");

namespace {

constexpr int JPEG_THREADS = 256;
constexpr int BLOCKS_PER_WG = JPEG_THREADS / 8;

// One 1-D pass of jidctint.c (13-bit constants), descaled by n bits.
__device__ __forceinline__ void idct_1d(const int (&v)[8], int (&o)[8], int n) {
  int z1 = (v[2] + v[6]) * 4433;
  int t2 = z1 - v[6] * 15137;
  int t3 = z1 + v[2] * 6270;
  int t0 = (v[0] + v[4]) << 13;
  int t1 = (v[0] - v[4]) << 13;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = v[7];
  t1 = v[5];
  t2 = v[3];
  t3 = v[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446;
  t1 *= 16819;
  t2 *= 25172;
  t3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  const int r = 1 << (n - 1);
  o[0] = (t10 + t3 + r) >> n;
  o[7] = (t10 - t3 + r) >> n;
  o[1] = (t11 + t2 + r) >> n;
  o[6] = (t11 - t2 + r) >> n;
  o[2] = (t12 + t1 + r) >> n;
  o[5] = (t12 - t1 + r) >> n;
  o[3] = (t13 + t0 + r) >> n;
  o[4] = (t13 - t0 + r) >> n;
}

__device__ __forceinline__ int clamp255(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

__device__ __forceinline__ int total_blocks(const MmrcaJpegDesc& d) {
  const int last = d.ncomp - 1;
  return d.blk_off[last] + d.bpr[last] * d.bpc[last];
}

// grid (x, B): workgroup x of image blockIdx.y takes blocks [32x, 32x + 32), then strides by 32 gridDim.x
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_idct_k(int16_t* __restrict__ coef, const MmrcaJpegDesc* __restrict__ desc) {
  __shared__ int ws[BLOCKS_PER_WG][8][9];          // (9: the column reads of eight lanes hit eight banks)
  const MmrcaJpegDesc& d = desc[blockIdx.y];
  const int total = total_blocks(d);
  const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
  int16_t* base = coef + d.coef_offset;
  for (int g0 = blockIdx.x * BLOCKS_PER_WG; g0 < total; g0 += gridDim.x * BLOCKS_PER_WG) {     // (uniform per workgroup)
    const int g = g0 + lb;
    const bool on = g < total;
    int v[8], o[8];
    if (on) {
      const int c = (d.ncomp == 3 && g >= d.blk_off[2]) ? 2 : ((d.ncomp == 3 && g >= d.blk_off[1]) ? 1 : 0);
      const uint4 raw = *reinterpret_cast<const uint4*>(base + (int64_t)g * 64 + j * 8);
      const uint4 q = *reinterpret_cast<const uint4*>(d.qt + c * 64 + j * 8);
      const unsigned rw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ws[lb][j][2 * i] = (int)(int16_t)(rw[i] & 0xFFFF) * (int)(qw[i] & 0xFFFF);
        ws[lb][j][2 * i + 1] = (int)(int16_t)(rw[i] >> 16) * (int)(qw[i] >> 16);
      }
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = ws[lb][i][j];            // column j
      idct_1d(v, o, 11);
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (int i = 0; i < 8; ++i) ws[lb][i][j] = o[i];
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = ws[lb][j][i];            // row j
      idct_1d(v, o, 18);
      uint2 px;
      px.x = clamp255(o[0] + 128) | clamp255(o[1] + 128) << 8 | clamp255(o[2] + 128) << 16 | clamp255(o[3] + 128) << 24;
      px.y = clamp255(o[4] + 128) | clamp255(o[5] + 128) << 8 | clamp255(o[6] + 128) << 16 | clamp255(o[7] + 128) << 24;
      *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(base + (int64_t)g * 64) + j * 8) = px;
    }
    __syncthreads();
  }
}

// Sample (y, x) of a component whose blocks start at block `blk0`: jpeg_idct_k left each block's 64 samples in the first half of
// its 128 bytes.
__device__ __forceinline__ int sample(const uint8_t* __restrict__ img, int blk0, int bpr, int y, int x) {
  return img[(int64_t)(blk0 + (y >> 3) * bpr + (x >> 3)) * 128 + (y & 7) * 8 + (x & 7)];
}

// jdsample.c h2v1_fancy_upsample / h2v2_fancy_upsample at output pixel (y, x) of a dh x dw chroma plane; replicating the edge
// sample reproduces the first- and last-column rules ((4p + 1) >> 2 == (4p + 2) >> 2 == p).
__device__ __forceinline__ int chroma(const uint8_t* __restrict__ img, int blk0, int bpr, int hmax, int vmax, int dh, int dw, int y, int x) {
  if (hmax == 1) return sample(img, blk0, bpr, y, x);
  const int i = x >> 1;
  const int ni = (x & 1) ? (i + 1 < dw ? i + 1 : i) : (i > 0 ? i - 1 : i);
  if (vmax == 1) {
    const int p = sample(img, blk0, bpr, y, i), nb = sample(img, blk0, bpr, y, ni);
    return (3 * p + nb + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int r = y >> 1;
  const int nr = (y & 1) ? (r + 1 < dh ? r + 1 : r) : (r > 0 ? r - 1 : r);
  const int s = 3 * sample(img, blk0, bpr, r, i) + sample(img, blk0, bpr, nr, i);
  const int sn = 3 * sample(img, blk0, bpr, r, ni) + sample(img, blk0, bpr, nr, ni);
  return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
}

// grid (x, B): thread t of image blockIdx.y takes pixels [16t, 16t + 16) in row-major numbering
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_rgb_k(const int16_t* __restrict__ coef, const MmrcaJpegDesc* __restrict__ desc,
                                                          uint8_t* __restrict__ out) {
  const MmrcaJpegDesc& d = desc[blockIdx.y];
  const int W = d.width, H = d.height, hmax = d.hmax, vmax = d.vmax;
  const bool colour = d.ncomp == 3;
  const int dw = (W + hmax - 1) / hmax, dh = (H + vmax - 1) / vmax;
  const int npix = W * H;                                  // <= 2^28
  const int groups = (npix + 15) / 16;
  const uint8_t* img = reinterpret_cast<const uint8_t*>(coef + d.coef_offset);
  uint8_t* dst = out + d.out_offset;
  const int bpr0 = d.bpr[0], bpr1 = d.bpr[1], bpr2 = d.bpr[2], off1 = d.blk_off[1], off2 = d.blk_off[2];
  for (int t = blockIdx.x * JPEG_THREADS + threadIdx.x; t < groups; t += gridDim.x * JPEG_THREADS) {
    const int p0 = t * 16;
    int y = p0 / W, x = p0 - y * W;
    unsigned w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (p0 + i < npix) {
        const int Y = sample(img, 0, bpr0, y, x);
        int R = Y, G = Y, B = Y;
        if (colour) {
          const int cb = chroma(img, off1, bpr1, hmax, vmax, dh, dw, y, x) - 128;
          const int cr = chroma(img, off2, bpr2, hmax, vmax, dh, dw, y, x) - 128;
          R = clamp255(Y + ((91881 * cr + 32768) >> 16));
          B = clamp255(Y + ((116130 * cb + 32768) >> 16));
          G = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        }
        w[(3 * i) >> 2] |= (unsigned)R << (8 * ((3 * i) & 3));
        w[(3 * i + 1) >> 2] |= (unsigned)G << (8 * ((3 * i + 1) & 3));
        w[(3 * i + 2) >> 2] |= (unsigned)B << (8 * ((3 * i + 2) & 3));
        if (++x == W) {
          x = 0;
          ++y;
        }
      }
    }
    uint8_t* o = dst + (int64_t)p0 * 3;
    if (p0 + 16 <= npix) {
      uint4* o4 = reinterpret_cast<uint4*>(o);             // out_offset and 48 t are multiples of 16
      o4[0] = make_uint4(w[0], w[1], w[2], w[3]);
      o4[1] = make_uint4(w[4], w[5], w[6], w[7]);
      o4[2] = make_uint4(w[8], w[9], w[10], w[11]);
    } else {
      const int nbytes = (npix - p0) * 3;
#pragma unroll
      for (int b = 0; b < 48; ++b)
        if (b < nbytes) o[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
  }
}

}  // namespace

extern "C" int mmrca_jpeg_idct_rgb(void* coef, const MmrcaJpegDesc* desc, int B, void* out, void* stream) {
  MMRCA_REQUIRE(coef && desc && out, "jpeg_idct_rgb: null pointer");
  MMRCA_REQUIRE(B > 0 && B <= 65535, "jpeg_idct_rgb: bad batch size %d", B);
  MMRCA_REQUIRE(((uintptr_t)coef & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)desc & 15) == 0,
                "jpeg_idct_rgb: coef, desc and out must be 16-byte aligned");
  // enough workgroups per image to fill the device at any batch size; both kernels stride over what is left
  int gx = 8192 / B;
  gx = gx < 16 ? 16 : (gx > 1024 ? 1024 : gx);
  hipLaunchKernelGGL(jpeg_idct_k, dim3((unsigned)gx, (unsigned)B), dim3(JPEG_THREADS), 0, (hipStream_t)stream, (int16_t*)coef, desc);
  MMRCA_CHECK_LAUNCH("jpeg_idct_rgb (idct)");
  hipLaunchKernelGGL(jpeg_rgb_k, dim3((unsigned)gx, (unsigned)B), dim3(JPEG_THREADS), 0, (hipStream_t)stream, (const int16_t*)coef, desc,
                     (uint8_t*)out);
  MMRCA_CHECK_LAUNCH("jpeg_idct_rgb (rgb)");
  return 0;
}
