// K7 (the step BEFORE the hot path): the reference's validation image pipeline on the GPU.
//   PadToMaintainAR (keep_aspect_ratio.py:18-53)  ->  A.Resize(W, H, cv2.INTER_LINEAR)  ->  (V/H flip)  ->
//   A.Normalize(ImageNet mean/std)  ->  ToTensorV2                                         (main_both.py:407-440)
// One launch for a whole batch of decoded uint8 HWC images of DIFFERENT sizes: they sit back to back in one staging buffer
// (one pinned H2D copy), a descriptor per image says where and how it is padded; a thread produces one output pixel (3
// channels) from 4 taps.  The padded image is never materialised (taps that fall into the padding read 0).  HBM-bound:
// 3 B read per source pixel (gathered, mostly L2-resident after first touch) and 12 B written per output pixel.
// Resize arithmetic = float32 INTER_LINEAR with half-pixel centres and a replicated border, rounded to uint8 (what cv2
// returns for a uint8 image; cv2 itself uses 11-bit fixed-point weights, i.e. single pixels may differ by one step).
#include "common.h"

static_assert(sizeof(MmrcaImageDesc) == 40, "MmrcaImageDesc layout (preprocess.py::DESC_DTYPE mirrors it)");

// The resized uint8 pixel (y, x) of image `d` (coordinates AFTER the flips are undone), 3 channels as floats holding integers
// 0..255.  The one copy of the sampling arithmetic: image_preprocess_k and image_stats_k both call it, so the statistics are
// those of exactly the image the resize writes.  Every multiply-add is spelled out as the fused / unfused form the compiler
// picks for image_preprocess_k under its default contraction (top = fma(1-fx, t00, fx*t01) etc.): left to the compiler, the same
// expression inlined into two kernels may be contracted differently (it was: a packed unfused multiply-add in one channel of the
// statistics kernel), and one x.5 tap sum then rounds to the other uint8 step.
__device__ __forceinline__ void resized_pixel_u8(const uint8_t* __restrict__ staging, const MmrcaImageDesc& d, int y, int x, int out_h, int out_w,
                                                 float v[3]) {
  const float sx = __fmaf_rn((float)x + 0.5f, (float)d.pw / (float)out_w, -0.5f);
  const float sy = __fmaf_rn((float)y + 0.5f, (float)d.ph / (float)out_h, -0.5f);
  const float x0f = floorf(sx), y0f = floorf(sy);
  const float fx = sx - x0f, fy = sy - y0f;
  int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
  x0 = min(max(x0, 0), d.pw - 1); x1 = min(max(x1, 0), d.pw - 1);
  y0 = min(max(y0, 0), d.ph - 1); y1 = min(max(y1, 0), d.ph - 1);
  const uint8_t* src = staging + d.offset;
  auto tap = [&](int py, int px, int c) -> float {
    const int sy_ = py - d.pad_top, sx_ = px - d.pad_left;
    if (sy_ < 0 || sy_ >= d.h || sx_ < 0 || sx_ >= d.w) return 0.f;
    return (float)src[((int64_t)sy_ * d.w + sx_) * 3 + c];
  };
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = __fmaf_rn(tap(y0, x0, c), 1.f - fx, __fmul_rn(tap(y0, x1, c), fx));
    const float bot = __fmaf_rn(tap(y1, x0, c), 1.f - fx, __fmul_rn(tap(y1, x1, c), fx));
    const float val = __fmaf_rn(top, 1.f - fy, __fmul_rn(bot, fy));
    v[c] = fminf(fmaxf(floorf(val + 0.5f), 0.f), 255.f);          // uint8 rounding of the resized image
  }
}

template <bool U8>          // U8: uint8 [B,H,W,3] output for the augmentation stages (augment.hip), no normalisation
__global__ void __launch_bounds__(256)
image_preprocess_k(const uint8_t* __restrict__ staging, const MmrcaImageDesc* __restrict__ desc, float* __restrict__ out, uint8_t* __restrict__ out_u8,
                   int out_h, int out_w, float m0, float m1, float m2, float is0, float is1, float is2) {
  const MmrcaImageDesc d = desc[blockIdx.y];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= out_h * out_w) return;
  int y = idx / out_w, x = idx % out_w;
  const int oy = y, ox = x;
  if (d.flip_v) y = out_h - 1 - y;
  if (d.flip_h) x = out_w - 1 - x;
  float v[3];
  resized_pixel_u8(staging, d, y, x, out_h, out_w, v);
  if (U8) {
    uint8_t* q = out_u8 + ((int64_t)blockIdx.y * out_h * out_w + (int64_t)oy * out_w + ox) * 3;
    q[0] = (uint8_t)v[0]; q[1] = (uint8_t)v[1]; q[2] = (uint8_t)v[2];
    return;
  }
  const int64_t plane = (int64_t)out_h * out_w;
  float* o = out + (int64_t)blockIdx.y * 3 * plane + (int64_t)oy * out_w + ox;
  o[0] = (v[0] / 255.0f - m0) * is0;
  o[plane] = (v[1] / 255.0f - m1) * is1;
  o[2 * plane] = (v[2] / 255.0f - m2) * is2;
}

extern "C" int mmrca_image_preprocess(const void* staging, const void* desc, float* out, int B, int out_h, int out_w,
                                      const float* mean3, const float* std3, void* stream) {
  MMRCA_REQUIRE(staging && desc && out && mean3 && std3, "image_preprocess: null pointer");
  MMRCA_REQUIRE(B > 0 && out_h > 0 && out_w > 0 && B <= 65535, "image_preprocess: bad shape B=%d %dx%d", B, out_h, out_w);
  MMRCA_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "image_preprocess: zero std");
  dim3 grid((unsigned)((out_h * out_w + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(image_preprocess_k<false>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)staging,
                     (const MmrcaImageDesc*)desc, out, (uint8_t*)nullptr, out_h, out_w, mean3[0], mean3[1], mean3[2], 1.f / std3[0], 1.f / std3[1],
                     1.f / std3[2]);
  MMRCA_CHECK_LAUNCH("image_preprocess");
  return 0;
}

extern "C" int mmrca_image_resize_u8(const void* staging, const void* desc, void* out_u8, int B, int out_h, int out_w, void* stream) {
  MMRCA_REQUIRE(staging && desc && out_u8, "image_resize_u8: null pointer");
  MMRCA_REQUIRE(B > 0 && out_h > 0 && out_w > 0 && B <= 65535, "image_resize_u8: bad shape B=%d %dx%d", B, out_h, out_w);
  dim3 grid((unsigned)((out_h * out_w + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(image_preprocess_k<true>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)staging,
                     (const MmrcaImageDesc*)desc, (float*)nullptr, (uint8_t*)out_u8, out_h, out_w, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
  MMRCA_CHECK_LAUNCH("image_resize_u8");
  return 0;
}

// Dataset statistics (main_image.py:212-235): per image and channel {sum v, sum v*v} of the uint8 image that image_resize_u8
// would write, without writing it.  Pixels are integers 0..255, so every sum is an integer and integer addition is associative:
// the result is exact and does not depend on the grid shape or on the order in which blocks arrive (a float accumulator would).
//   thread: 6 uint32 accumulators over a grid-stride loop inside one image.  v*v <= 65025, so a thread may take at most
//           STATS_MAX_PIX_PER_THREAD = floor((2^32 - 1) / 65025) = 66051 pixels (the host entry point requires it);
//   wave:   widened to uint64, 64-lane shuffle tree;   block: 4 waves through LDS;   grid: one 64-bit atomicAdd per block and quantity.
// The flips permute pixels and leave the sums unchanged, so the descriptor's flip fields are not read.
constexpr int STATS_MAX_BLOCKS = 64;                        // blocks per image: 16384 threads cover 224x224 in ~3 pixels each
constexpr int64_t STATS_MAX_PIX_PER_THREAD = 0xFFFFFFFFll / 65025;

__global__ void __launch_bounds__(256)
image_stats_k(const uint8_t* __restrict__ staging, const MmrcaImageDesc* __restrict__ desc, unsigned long long* __restrict__ sums, int out_h, int out_w) {
  __shared__ unsigned long long part[4][6];
  const MmrcaImageDesc d = desc[blockIdx.y];
  const int npix = out_h * out_w;
  uint32_t acc[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < npix; idx += gridDim.x * 256) {
    float v[3];
    resized_pixel_u8(staging, d, idx / out_w, idx % out_w, out_h, out_w, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t q = (uint32_t)v[c];
      acc[2 * c] += q;
      acc[2 * c + 1] += q * q;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    unsigned long long t = acc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if (lane == 0) part[wave][i] = t;
  }
  __syncthreads();
  if (threadIdx.x < 6)
    atomicAdd(sums + (int64_t)blockIdx.y * 6 + threadIdx.x,
              part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}

extern "C" int mmrca_image_stats_u8(const void* staging, const void* desc, void* sums, int B, int out_h, int out_w, void* stream) {
  MMRCA_REQUIRE(staging && desc && sums, "image_stats_u8: null pointer");
  MMRCA_REQUIRE(B > 0 && out_h > 0 && out_w > 0 && B <= 65535, "image_stats_u8: bad shape B=%d %dx%d", B, out_h, out_w);
  const int64_t npix = (int64_t)out_h * out_w;
  MMRCA_REQUIRE(npix <= 0x7FFFFFFFll - STATS_MAX_BLOCKS * 256, "image_stats_u8: %dx%d pixels do not fit a 32-bit index", out_h, out_w);
  const int64_t blocks = (npix + 255) / 256 < STATS_MAX_BLOCKS ? (npix + 255) / 256 : STATS_MAX_BLOCKS;
  const int64_t per_thread = (npix + blocks * 256 - 1) / (blocks * 256);
  MMRCA_REQUIRE(per_thread <= STATS_MAX_PIX_PER_THREAD, "image_stats_u8: %lld pixels per thread overflow the 32-bit accumulators (limit %lld)",
                (long long)per_thread, (long long)STATS_MAX_PIX_PER_THREAD);
  const hipError_t e = hipMemsetAsync(sums, 0, (size_t)B * 6 * sizeof(unsigned long long), (hipStream_t)stream);
  MMRCA_REQUIRE(e == hipSuccess, "image_stats_u8: clearing the sums failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(image_stats_k, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)staging,
                     (const MmrcaImageDesc*)desc, (unsigned long long*)sums, out_h, out_w);
  MMRCA_CHECK_LAUNCH("image_stats_u8");
  return 0;
}
