// Head of the hierarchical late-fusion model (multimodal_model.Hierarchical; the reference's Hierarchical.forward,
// CVPR_code/multimodal_model.py:729-818): window average pools of two stage maps, six L2-normalised vectors concatenated into
// xi [B, 5888] | xt [B, 2304], dropout on each, two wide Linear + ReLU layers (5888 -> 512, 2304 -> 512).  The last Linear
// (1024 -> n_classes) is mmrca_linear_cls_fwd / _bwd (classifier.hip).
//
// Everything here is fp32 arithmetic with fp32 outputs; only the stage maps (and the stage gradients the pool backward adds into)
// are in the conv backbone's compute dtype.  No atomics: every sum over the batch or over the contraction runs in a fixed order, so
// two runs of the same inputs give the same bits.
#include "common.h"
#include <algorithm>

// ---------------------------------------------------------------------------------------------------------------------------
// 1. window average pool on the NHWC row layout [B*H*W, C]: AvgPool2d(k, k) with floor windows (oh = H / k, ow = W / k; the rows and
//    columns behind the last whole window are not read), written in NCHW order -- out[b*ld + c*oh*ow + i*ow + j] -- as fp32.
//    One thread per (sample, window, 4 channels): consecutive lanes read consecutive channels of the same pixel.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
hier_pool_fwd_k(const T* __restrict__ x, float* __restrict__ out, int ld, int B, int H, int W, int C, int k, int oh, int ow) {
  const int c4n = C >> 2;
  const int64_t total = (int64_t)B * oh * ow * c4n;
  const float scale = 1.f / (float)(k * k);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(t % c4n) * 4;
    int64_t r = t / c4n;
    const int j = (int)(r % ow); r /= ow;
    const int i = (int)(r % oh);
    const int b = (int)(r / oh);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int di = 0; di < k; ++di) {
      const T* row = x + (((int64_t)b * H + (i * k + di)) * W + j * k) * C + c;
      for (int dj = 0; dj < k; ++dj) {
        const Vec4<T> v = Vec4<T>::load(row + (int64_t)dj * C);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += v.v[e];
      }
    }
    float* o = out + (int64_t)b * ld + (int64_t)c * oh * ow + i * ow + j;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[(int64_t)e * oh * ow] = s[e] * scale;
  }
}

// backward: dx[b, i, j, c] += d[b*ld + c*oh*ow + (i/k)*ow + j/k] / k^2 for the covered pixels (i < oh*k, j < ow*k); every other pixel
// of dx is left as it is.  It ADDS: the stage output also feeds the next stage, whose backward wrote dx.
template <typename T>
__global__ void __launch_bounds__(256)
hier_pool_bwd_k(const float* __restrict__ d, int ld, T* __restrict__ dx, int B, int H, int W, int C, int k, int oh, int ow) {
  const int c4n = C >> 2, ch = oh * k, cw = ow * k;
  const int64_t total = (int64_t)B * ch * cw * c4n;
  const float scale = 1.f / (float)(k * k);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(t % c4n) * 4;
    int64_t r = t / c4n;
    const int j = (int)(r % cw); r /= cw;
    const int i = (int)(r % ch);
    const int b = (int)(r / ch);
    const float* g = d + (int64_t)b * ld + (int64_t)c * oh * ow + (i / k) * ow + (j / k);
    T* p = dx + (((int64_t)b * H + i) * W + j) * C + c;
    Vec4<T> v = Vec4<T>::load(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v.v[e] = fmaf(g[(int64_t)e * oh * ow], scale, v.v[e]);
    v.store(p);
  }
}

static int pool_check(const char* name, const void* x, const void* f, int ld, int B, int H, int W, int C, int k, int dtype) {
  MMRCA_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "%s: bad shape B=%d H=%d W=%d C=%d (C %% 4 == 0)", name, B, H, W, C);
  MMRCA_REQUIRE(k >= 1 && k <= H && k <= W, "%s: window %d does not fit a %d x %d map", name, k, H, W);
  MMRCA_REQUIRE((int64_t)ld >= (int64_t)C * (H / k) * (W / k), "%s: ld %d is smaller than the pooled vector (%lld)", name, ld,
                (long long)C * (H / k) * (W / k));
  MMRCA_REQUIRE(x && f && (uintptr_t)x % (dtype == MMRCA_BF16 ? 8 : 16) == 0 && (uintptr_t)f % 4 == 0, "%s: null or misaligned pointer", name);
  return 0;
}

static inline int ew_grid(int64_t total) { return (int)std::min<int64_t>((total + 255) / 256, 2048); }

extern "C" int mmrca_hier_pool_fwd(const void* x, float* out, int ld_out, int B, int H, int W, int C, int k, int dtype, void* stream) {
  if (int rc = pool_check("hier_pool_fwd", x, out, ld_out, B, H, W, C, k, dtype)) return rc;
  const int oh = H / k, ow = W / k;
  MMRCA_DISPATCH_DTYPE(dtype, "hier_pool_fwd", {
    hipLaunchKernelGGL((hier_pool_fwd_k<T>), dim3(ew_grid((int64_t)B * oh * ow * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                       (const T*)x, out, ld_out, B, H, W, C, k, oh, ow);
    MMRCA_CHECK_LAUNCH("hier_pool_fwd");
    return 0;
  })
}

extern "C" int mmrca_hier_pool_bwd(const float* d, int ld_d, void* dx, int B, int H, int W, int C, int k, int dtype, void* stream) {
  if (int rc = pool_check("hier_pool_bwd", dx, d, ld_d, B, H, W, C, k, dtype)) return rc;
  const int oh = H / k, ow = W / k;
  MMRCA_DISPATCH_DTYPE(dtype, "hier_pool_bwd", {
    hipLaunchKernelGGL((hier_pool_bwd_k<T>), dim3(ew_grid((int64_t)B * oh * k * ow * k * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                       d, ld_d, (T*)dx, B, H, W, C, k, oh, ow);
    MMRCA_CHECK_LAUNCH("hier_pool_bwd");
    return 0;
  })
}

// ---------------------------------------------------------------------------------------------------------------------------
// 2. normalise + concatenate + dropout.  raw [B, ld] holds nseg segments back to back (columns off[s] .. off[s+1]); each is divided
//    by its own L2 norm (no epsilon, as the reference); the first nseg_a segments form group a (the image vector xi), the rest
//    group b (xt), and each group draws its own dropout mask: keep = hash(seed_group, b * width_group + column in group) >= p.
//    One workgroup per (segment, sample).
// ---------------------------------------------------------------------------------------------------------------------------
#define HIER_MAX_SEG 8
struct HierSegs { int off[HIER_MAX_SEG + 1]; int nseg, nseg_a; };

__device__ __forceinline__ float block_sum_256(float v, float* red) {      // fixed order: lanes by butterfly, the four waves in order
  const float s = wave_sum(v);
  __syncthreads();                             // (red may still be read from a previous call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float hier_keep(const HierSegs& sg, int seg, int b, int col, float p, float inv_keep, uint64_t seed_a, uint64_t seed_b) {
  if (p <= 0.f) return 1.f;
  const bool a = seg < sg.nseg_a;
  const int g0 = a ? sg.off[0] : sg.off[sg.nseg_a], g1 = a ? sg.off[sg.nseg_a] : sg.off[sg.nseg];
  return mmrca_uniform(a ? seed_a : seed_b, (uint64_t)b * (uint64_t)(g1 - g0) + (uint64_t)(col - g0)) >= p ? inv_keep : 0.f;
}

__global__ void __launch_bounds__(256)
hier_norm_fwd_k(const float* __restrict__ raw, float* __restrict__ x, float* __restrict__ inv, int ld, HierSegs sg, float p,
                uint64_t seed_a, uint64_t seed_b) {
  __shared__ float red[4];
  const int seg = blockIdx.x, b = blockIdx.y, lo = sg.off[seg], hi = sg.off[seg + 1];
  const float* v = raw + (int64_t)b * ld;
  float ss = 0.f;
  for (int i = lo + threadIdx.x; i < hi; i += 256) ss = fmaf(v[i], v[i], ss);
  ss = block_sum_256(ss, red);
  const float r = 1.f / sqrtf(ss);            // a zero vector: r = inf, outputs 0 * inf = NaN, as the reference's 0 / 0
  if (threadIdx.x == 0) inv[(int64_t)b * sg.nseg + seg] = r;
  const float ik = p > 0.f ? 1.f / (1.f - p) : 1.f;
  for (int i = lo + threadIdx.x; i < hi; i += 256)
    x[(int64_t)b * ld + i] = v[i] * r * hier_keep(sg, seg, b, i, p, ik, seed_a, seed_b);
}

// y = v / |v|,  g = dx * keep:   dv = (g - y (g . y)) / |v|
__global__ void __launch_bounds__(256)
hier_norm_bwd_k(const float* __restrict__ dx, const float* __restrict__ raw, const float* __restrict__ inv, float* __restrict__ draw,
                int ld, HierSegs sg, float p, uint64_t seed_a, uint64_t seed_b) {
  __shared__ float red[4];
  const int seg = blockIdx.x, b = blockIdx.y, lo = sg.off[seg], hi = sg.off[seg + 1];
  const float* v = raw + (int64_t)b * ld;
  const float* g = dx + (int64_t)b * ld;
  const float r = inv[(int64_t)b * sg.nseg + seg];
  const float ik = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float dot = 0.f;
  for (int i = lo + threadIdx.x; i < hi; i += 256)
    dot = fmaf(g[i] * hier_keep(sg, seg, b, i, p, ik, seed_a, seed_b), v[i] * r, dot);
  dot = block_sum_256(dot, red);
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const float gi = g[i] * hier_keep(sg, seg, b, i, p, ik, seed_a, seed_b);
    draw[(int64_t)b * ld + i] = (gi - v[i] * r * dot) * r;
  }
}

static int norm_segs(const char* name, HierSegs* sg, const int* seg_off, int nseg, int nseg_a, int B, int ld, float p) {
  MMRCA_REQUIRE(seg_off && nseg >= 1 && nseg <= HIER_MAX_SEG && nseg_a >= 0 && nseg_a <= nseg, "%s: bad segment table (nseg=%d nseg_a=%d, at most %d)",
                name, nseg, nseg_a, HIER_MAX_SEG);
  MMRCA_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d outside [1, 65535]", name, B);
  MMRCA_REQUIRE(p >= 0.f && p < 1.f, "%s: drop_p %f outside [0, 1)", name, (double)p);
  for (int s = 0; s <= nseg; ++s) {
    MMRCA_REQUIRE(seg_off[s] >= 0 && seg_off[s] <= ld && (s == 0 || seg_off[s] > seg_off[s - 1]), "%s: segment offsets must increase inside [0, ld=%d]", name, ld);
    sg->off[s] = seg_off[s];
  }
  sg->nseg = nseg;
  sg->nseg_a = nseg_a;
  return 0;
}

extern "C" int mmrca_hier_norm_fwd(const float* raw, float* x, float* inv, int B, int ld, const int* seg_off, int nseg, int nseg_a,
                                   float drop_p, uint64_t seed_a, uint64_t seed_b, void* stream) {
  HierSegs sg;
  if (int rc = norm_segs("hier_norm_fwd", &sg, seg_off, nseg, nseg_a, B, ld, drop_p)) return rc;
  MMRCA_REQUIRE(raw && x && inv, "hier_norm_fwd: null pointer");
  hipLaunchKernelGGL(hier_norm_fwd_k, dim3(nseg, B), dim3(256), 0, (hipStream_t)stream, raw, x, inv, ld, sg, drop_p, seed_a, seed_b);
  MMRCA_CHECK_LAUNCH("hier_norm_fwd");
  return 0;
}

extern "C" int mmrca_hier_norm_bwd(const float* dx, const float* raw, const float* inv, float* draw, int B, int ld, const int* seg_off,
                                   int nseg, int nseg_a, float drop_p, uint64_t seed_a, uint64_t seed_b, void* stream) {
  HierSegs sg;
  if (int rc = norm_segs("hier_norm_bwd", &sg, seg_off, nseg, nseg_a, B, ld, drop_p)) return rc;
  MMRCA_REQUIRE(dx && raw && inv && draw, "hier_norm_bwd: null pointer");
  hipLaunchKernelGGL(hier_norm_bwd_k, dim3(nseg, B), dim3(256), 0, (hipStream_t)stream, dx, raw, inv, draw, ld, sg, drop_p, seed_a, seed_b);
  MMRCA_CHECK_LAUNCH("hier_norm_bwd");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// 3. Y = relu(X W^T + b), X [B, K] (row pitch ldx), W [N, K], for a batch far smaller than K: the layer is a weight stream (12 MB at
//    5888 x 512), so the contraction is split over the whole chip.  Workgroup (n tile of 64, k chunk of 128) stages its 32 KB piece of
//    W once -- every load instruction of a wave reads 512 contiguous bytes of one weight row -- and walks the batch 16 samples at a
//    time: lane = output column, wave = 4 samples, X broadcast from LDS.  Partial sums go to ws[k chunk][B][N]; a second launch adds
//    them in chunk order, adds the bias and applies the ReLU.
// ---------------------------------------------------------------------------------------------------------------------------
#define HL_NT 64
#define HL_KC 128
#define HL_BT 16
#define HL_WLD (HL_KC + 4)      // one 16-byte access of padding per row: the lane = row reads of ds_read_b128 do not collide

__global__ void __launch_bounds__(256)
hier_linear_part_k(const float* __restrict__ X, int ldx, const float* __restrict__ W, float* __restrict__ ws, int B, int N, int K) {
  __shared__ __attribute__((aligned(16))) float Ws[HL_NT * HL_WLD];
  __shared__ __attribute__((aligned(16))) float Xs[HL_BT * HL_KC];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n0 = blockIdx.x * HL_NT, k0 = blockIdx.y * HL_KC;
  // W tile: 64 rows x 128 floats = 2048 float4; thread t reads float4 (t & 31) of rows (t >> 5) + 8 i
  for (int i = 0; i < 8; ++i) {
    const int r = (t >> 5) + 8 * i, c = (t & 31) * 4;
    const float4 w = *reinterpret_cast<const float4*>(W + (int64_t)(n0 + r) * K + k0 + c);
    *reinterpret_cast<float4*>(&Ws[r * HL_WLD + c]) = w;
  }
  for (int b0 = 0; b0 < B; b0 += HL_BT) {
    __syncthreads();                           // (the previous chunk's readers are done; the first pass: orders nothing yet)
    for (int i = t; i < HL_BT * HL_KC / 4; i += 256) {
      const int r = i / (HL_KC / 4), c = (i % (HL_KC / 4)) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (b0 + r < B) v = *reinterpret_cast<const float4*>(X + (int64_t)(b0 + r) * ldx + k0 + c);
      *reinterpret_cast<float4*>(&Xs[r * HL_KC + c]) = v;
    }
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* wr = &Ws[lane * HL_WLD];
    const float* xr = &Xs[wave * 4 * HL_KC];
#pragma unroll 4
    for (int c = 0; c < HL_KC; c += 4) {
      const float4 w = *reinterpret_cast<const float4*>(wr + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 xv = *reinterpret_cast<const float4*>(xr + j * HL_KC + c);
        acc[j] = fmaf(xv.x, w.x, fmaf(xv.y, w.y, fmaf(xv.z, w.z, fmaf(xv.w, w.w, acc[j]))));
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = b0 + wave * 4 + j;
      if (b < B) ws[((int64_t)blockIdx.y * B + b) * N + n0 + lane] = acc[j];
    }
  }
}

__global__ void __launch_bounds__(256)
hier_linear_reduce_k(const float* __restrict__ ws, const float* __restrict__ bias, float* __restrict__ Y, int ldy, int B, int N, int KS) {
  const int64_t total = (int64_t)B * N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int n = (int)(i % N), b = (int)(i / N);
    float s = bias[n];
    for (int c = 0; c < KS; ++c) s += ws[(int64_t)c * total + i];
    Y[(int64_t)b * ldy + n] = fmaxf(s, 0.f);
  }
}

// backward, dZ = dY * (Y > 0):
//   dW[n, k] += sum_b dZ[b, n] X[b, k]  and  db[n] += sum_b dZ[b, n]   (samples in order, every element owned by one thread)
//   dX[b, k]  = sum_n dZ[b, n] W[n, k]                                   (N / 64 partial sums through ws, added in order; skipped when dX is null)
// In both kernels a lane owns 4 consecutive k: the 12 MB read-modify-write of dW and the reads of W are 1 KiB contiguous per wave
// instruction.
#define HL_BW_NT 32           // weight-gradient tile: 32 rows of dW (8 per wave) x 256 columns
#define HL_BW_BC 64           // samples of dZ staged at a time

__global__ void __launch_bounds__(256)
hier_linear_wgrad_k(const float* __restrict__ dY, int lddy, const float* __restrict__ Y, int ldy, const float* __restrict__ X, int ldx,
                    float* __restrict__ dW, float* __restrict__ db, int B, int N, int K) {
  __shared__ __attribute__((aligned(16))) float dz[HL_BW_BC * HL_BW_NT];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int k = blockIdx.x * 256 + lane * 4, n0 = blockIdx.y * HL_BW_NT;
  float acc[8][4];
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = 0.f;
  float bsum = 0.f;                            // (threads t < 32 of the first k tile: the bias gradient of column n0 + t)
  for (int b0 = 0; b0 < B; b0 += HL_BW_BC) {
    const int nb = min(HL_BW_BC, B - b0);
    __syncthreads();
    for (int i = t; i < nb * HL_BW_NT; i += 256) {
      const int bb = i / HL_BW_NT, n = i % HL_BW_NT;
      const int64_t b = b0 + bb;
      dz[i] = Y[b * ldy + n0 + n] > 0.f ? dY[b * lddy + n0 + n] : 0.f;
    }
    __syncthreads();
    for (int bb = 0; bb < nb; ++bb) {
      const float4 xv = *reinterpret_cast<const float4*>(X + (int64_t)(b0 + bb) * ldx + k);
      const float4 d0 = *reinterpret_cast<const float4*>(&dz[bb * HL_BW_NT + wave * 8]);
      const float4 d1 = *reinterpret_cast<const float4*>(&dz[bb * HL_BW_NT + wave * 8 + 4]);
      const float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        acc[r][0] = fmaf(d[r], xv.x, acc[r][0]);
        acc[r][1] = fmaf(d[r], xv.y, acc[r][1]);
        acc[r][2] = fmaf(d[r], xv.z, acc[r][2]);
        acc[r][3] = fmaf(d[r], xv.w, acc[r][3]);
      }
    }
    if (blockIdx.x == 0 && t < HL_BW_NT)
      for (int bb = 0; bb < nb; ++bb) bsum += dz[bb * HL_BW_NT + t];
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    float* p = dW + (int64_t)(n0 + wave * 8 + r) * K + k;
    float4 g = *reinterpret_cast<float4*>(p);
    g.x += acc[r][0]; g.y += acc[r][1]; g.z += acc[r][2]; g.w += acc[r][3];
    *reinterpret_cast<float4*>(p) = g;
  }
  if (blockIdx.x == 0 && t < HL_BW_NT) db[n0 + t] += bsum;
}

#define HL_DX_BT 32           // samples per workgroup of the input gradient (8 per wave)
#define HL_DX_NT 64           // columns n of dZ per workgroup: the sum over n is split N / 64 ways over the chip, like the forward's over k
#define HL_DX_LD 36           // row pitch of the transposed dZ tile (16-byte aligned; 36 instead of 32 spreads the transposing writes over 16 banks)

// partial input gradient of one (k tile of 256, n chunk of 64, 32 samples): ws[n chunk][b][k]
__global__ void __launch_bounds__(256)
hier_linear_dgrad_part_k(const float* __restrict__ dY, int lddy, const float* __restrict__ Y, int ldy, const float* __restrict__ W,
                         float* __restrict__ ws, int B, int N, int K) {
  __shared__ __attribute__((aligned(16))) float dzt[HL_DX_NT * HL_DX_LD];      // [n][sample]: column n of dZ for this workgroup's samples
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int k = blockIdx.x * 256 + lane * 4, n0 = blockIdx.y * HL_DX_NT, b0 = blockIdx.z * HL_DX_BT;
  for (int i = t; i < HL_DX_NT * HL_DX_BT; i += 256) {
    const int bb = i / HL_DX_NT, n = i % HL_DX_NT;           // (consecutive threads read consecutive columns of one sample)
    const int64_t b = b0 + bb;
    dzt[n * HL_DX_LD + bb] = (b < B && Y[b * ldy + n0 + n] > 0.f) ? dY[b * lddy + n0 + n] : 0.f;
  }
  __syncthreads();
  float acc[8][4];
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = 0.f;
#pragma unroll 4
  for (int n = 0; n < HL_DX_NT; ++n) {
    const float4 w = *reinterpret_cast<const float4*>(W + (int64_t)(n0 + n) * K + k);
    const float4 d0 = *reinterpret_cast<const float4*>(&dzt[n * HL_DX_LD + wave * 8]);
    const float4 d1 = *reinterpret_cast<const float4*>(&dzt[n * HL_DX_LD + wave * 8 + 4]);
    const float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      acc[r][0] = fmaf(d[r], w.x, acc[r][0]);
      acc[r][1] = fmaf(d[r], w.y, acc[r][1]);
      acc[r][2] = fmaf(d[r], w.z, acc[r][2]);
      acc[r][3] = fmaf(d[r], w.w, acc[r][3]);
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int b = b0 + wave * 8 + r;
    if (b < B) *reinterpret_cast<float4*>(ws + ((int64_t)blockIdx.y * B + b) * K + k) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
  }
}

// dX[b, k] = the partial sums in chunk order
__global__ void __launch_bounds__(256)
hier_linear_dgrad_reduce_k(const float* __restrict__ ws, float* __restrict__ dX, int lddx, int B, int K, int NS) {
  const int k4n = K >> 2;
  const int64_t total = (int64_t)B * k4n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / k4n), k = (int)(i % k4n) * 4;
    float4 s = *reinterpret_cast<const float4*>(ws + (int64_t)b * K + k);
    for (int c = 1; c < NS; ++c) {
      const float4 v = *reinterpret_cast<const float4*>(ws + ((int64_t)c * B + b) * K + k);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(dX + (int64_t)b * lddx + k) = s;
  }
}

static int linear_check(const char* name, int B, int N, int K, int ldx, const void* X, const void* W) {
  MMRCA_REQUIRE(B >= 1 && B <= 65535, "%s: bad batch %d", name, B);
  MMRCA_REQUIRE(N >= HL_NT && N % HL_NT == 0 && N <= 1024, "%s: N=%d must be a multiple of %d, at most 1024", name, N, HL_NT);
  MMRCA_REQUIRE(K >= 256 && K % 256 == 0, "%s: K=%d must be a multiple of 256", name, K);
  MMRCA_REQUIRE(ldx >= K && ldx % 4 == 0, "%s: row pitch %d must be a multiple of 4 and at least K=%d", name, ldx, K);
  MMRCA_REQUIRE(X && W && ((uintptr_t)X & 15) == 0 && ((uintptr_t)W & 15) == 0, "%s: X and W must be 16-byte aligned", name);
  return 0;
}

// the forward's partial sums [K / 128][B][N] or the input gradient's [N / 64][B][K], whichever is larger
extern "C" int64_t mmrca_hier_linear_workspace_bytes(int B, int N, int K) {
  const int64_t fwd = (int64_t)((K + HL_KC - 1) / HL_KC) * B * N, bwd = (int64_t)((N + HL_DX_NT - 1) / HL_DX_NT) * B * K;
  return std::max(fwd, bwd) * (int64_t)sizeof(float);
}

extern "C" int mmrca_hier_linear_relu_fwd(const float* X, int ldx, const float* W, const float* b, float* Y, int ldy, float* ws,
                                          int64_t ws_bytes, int B, int N, int K, void* stream) {
  if (int rc = linear_check("hier_linear_relu_fwd", B, N, K, ldx, X, W)) return rc;
  MMRCA_REQUIRE(b && Y && ws && ((uintptr_t)ws & 15) == 0 && ldy >= N, "hier_linear_relu_fwd: null / misaligned pointer or ldy %d < N", ldy);
  MMRCA_REQUIRE(ws_bytes >= mmrca_hier_linear_workspace_bytes(B, N, K), "hier_linear_relu_fwd: workspace of %lld bytes, %lld needed",
                (long long)ws_bytes, (long long)mmrca_hier_linear_workspace_bytes(B, N, K));
  const int KS = K / HL_KC;
  hipLaunchKernelGGL(hier_linear_part_k, dim3(N / HL_NT, KS), dim3(256), 0, (hipStream_t)stream, X, ldx, W, ws, B, N, K);
  MMRCA_CHECK_LAUNCH("hier_linear_relu_fwd (partials)");
  hipLaunchKernelGGL(hier_linear_reduce_k, dim3(ew_grid((int64_t)B * N)), dim3(256), 0, (hipStream_t)stream, ws, b, Y, ldy, B, N, KS);
  MMRCA_CHECK_LAUNCH("hier_linear_relu_fwd (reduce)");
  return 0;
}

extern "C" int mmrca_hier_linear_relu_bwd(const float* dY, int lddy, const float* Y, int ldy, const float* X, int ldx, const float* W,
                                          float* dW, float* db, float* dX, int lddx, float* ws, int64_t ws_bytes, int B, int N, int K,
                                          void* stream) {
  if (int rc = linear_check("hier_linear_relu_bwd", B, N, K, ldx, X, W)) return rc;
  MMRCA_REQUIRE(dY && Y && dW && db && lddy >= N && ldy >= N && ((uintptr_t)dW & 15) == 0, "hier_linear_relu_bwd: null / misaligned pointer or pitch < N");
  hipLaunchKernelGGL(hier_linear_wgrad_k, dim3(K / 256, N / HL_BW_NT), dim3(256), 0, (hipStream_t)stream, dY, lddy, Y, ldy, X, ldx, dW, db, B, N, K);
  MMRCA_CHECK_LAUNCH("hier_linear_relu_bwd (weight gradient)");
  if (dX) {
    MMRCA_REQUIRE(lddx >= K && lddx % 4 == 0 && ((uintptr_t)dX & 15) == 0, "hier_linear_relu_bwd: dX pitch %d / alignment", lddx);
    MMRCA_REQUIRE(ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= mmrca_hier_linear_workspace_bytes(B, N, K),
                  "hier_linear_relu_bwd: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)mmrca_hier_linear_workspace_bytes(B, N, K));
    const int NS = N / HL_DX_NT, nbt = (B + HL_DX_BT - 1) / HL_DX_BT;
    MMRCA_REQUIRE(nbt <= 65535, "hier_linear_relu_bwd: batch %d too large", B);
    hipLaunchKernelGGL(hier_linear_dgrad_part_k, dim3(K / 256, NS, nbt), dim3(256), 0, (hipStream_t)stream, dY, lddy, Y, ldy, W, ws, B, N, K);
    MMRCA_CHECK_LAUNCH("hier_linear_relu_bwd (input gradient, partials)");
    hipLaunchKernelGGL(hier_linear_dgrad_reduce_k, dim3(ew_grid((int64_t)B * (K / 4))), dim3(256), 0, (hipStream_t)stream, ws, dX, lddx, B, K, NS);
    MMRCA_CHECK_LAUNCH("hier_linear_relu_bwd (input gradient, reduce)");
  }
  return 0;
}

MMRCA_SEED_EPOCH_EXPORT(hier_head)   // this translation unit's copy of the mask epoch (common.h)
