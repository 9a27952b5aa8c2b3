// Head of the bimodal GRU late-fusion model (multimodal_model.HierarchicalBimodalFusion; the reference's forward of that name,
// CVPR_code/multimodal_model.py:835-888): two 400-wide context GRUs over the projected text / image features, a Hadamard fusion
// tanh(a k1 + b k2 + bias), a 500-wide GRU over the fused rows, two p = 0.86 dropouts, Linear(900, 450) + ReLU, Linear(450, 4).
// The GRUs receive a 2-D tensor, so the "sequence" is the batch: row t of the batch is time step t (T = B), h_{-1} = 0.
//
//   1. a small fp32 Linear (forward, weight / bias gradient, input gradient) for every matrix product off the recurrent chain:
//      the 768 / 1280 -> 400 projections, W_ih x_t + b_ih for all t at once, concat_fc, the classifier, and after the backward
//      chain dW_ih, dW_hh, the bias sums and dx over all T;
//   2. the recurrent chain: ONE launch per time step, forward and backward, the hidden units spread over the chip.  Steps chain
//      through the stream; there is no wait between workgroups inside a launch.  Two GRUs of the same width share every launch
//      (blockIdx.y), so gru_text + gru_audio cost T launches, not 2 T;
//   3. the Hadamard fusion, forward and backward;
//   4. dropout with a counter-based mask on the shared mask epoch (common.h).
//
// fp32 arithmetic and storage throughout.  No atomics: every sum runs in a fixed order, so two runs give the same bits.  Weight
// gradients ACCUMULATE.
#include "common.h"
#include <algorithm>

// ---------------------------------------------------------------------------------------------------------------------------
// 1. Y [B, N] = act(X W^T + b), X [B, K] (row pitch ldx), W [N, K].  One wave per output column n and 8 samples: the lanes stride the
//    contraction (16-byte loads when K and the pitches allow, else one float), the tail lanes read a clamped address and contribute
//    zero, then a butterfly sum.  Meant for B <= a few hundred and N, K <= a few thousand.
// ---------------------------------------------------------------------------------------------------------------------------
#define GL_BT 8

template <int VEC> struct FV;
template <> struct FV<4> {
  float v[4];
  __device__ __forceinline__ static FV load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    FV r; r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w; return r;
  }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct FV<1> {
  float v[1];
  __device__ __forceinline__ static FV load(const float* p) { FV r; r.v[0] = *p; return r; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};

template <int VEC>
__global__ void __launch_bounds__(256)
gru_lin_fwd_k(const float* __restrict__ X, int ldx, const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ Y,
              int ldy, int B, int N, int K, int relu) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 4 + wave, b0 = blockIdx.y * GL_BT;
  if (n >= N) return;                          // wave-uniform; the kernel has no barrier
  float acc[GL_BT];
#pragma unroll
  for (int r = 0; r < GL_BT; ++r) acc[r] = 0.f;
  const float* wr = W + (int64_t)n * K;
  for (int k0 = 0; k0 < K; k0 += 64 * VEC) {
    const int k = k0 + lane * VEC;
    const bool ok = k < K;
    const int kk = ok ? k : 0;
    FV<VEC> w = FV<VEC>::load(wr + kk);
#pragma unroll
    for (int e = 0; e < VEC; ++e) w.v[e] = ok ? w.v[e] : 0.f;
#pragma unroll
    for (int r = 0; r < GL_BT; ++r) {
      const int b = min(b0 + r, B - 1);        // (rows behind the batch repeat the last one and are not stored)
      const FV<VEC> x = FV<VEC>::load(X + (int64_t)b * ldx + kk);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[r] = fmaf(w.v[e], x.v[e], acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < GL_BT; ++r) acc[r] = wave_sum(acc[r]);
  if (lane == 0) {
    const float bn = bias ? bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < GL_BT; ++r)
      if (b0 + r < B) {
        const float y = acc[r] + bn;
        Y[(int64_t)(b0 + r) * ldy + n] = relu ? fmaxf(y, 0.f) : y;
      }
  }
}

// dW[n, k] += sum_b dZ[b, n] X[b, k], db[n] += sum_b dZ[b, n] with dZ = dY (* (Y > 0) when Y is given): one thread per (n, VEC columns),
// the samples in order.
template <int VEC>
__global__ void __launch_bounds__(256)
gru_lin_wgrad_k(const float* __restrict__ dY, int lddy, const float* __restrict__ Y, int ldy, const float* __restrict__ X, int ldx,
                float* __restrict__ dW, float* __restrict__ db, int B, int N, int K) {
  const int kvn = K / VEC;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)N * kvn) return;
  const int n = (int)(idx / kvn), k = (int)(idx % kvn) * VEC;
  float acc[VEC], bsum = 0.f;
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
  for (int b = 0; b < B; ++b) {
    float dz = dY[(int64_t)b * lddy + n];
    if (Y) dz = Y[(int64_t)b * ldy + n] > 0.f ? dz : 0.f;
    const FV<VEC> x = FV<VEC>::load(X + (int64_t)b * ldx + k);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = fmaf(dz, x.v[e], acc[e]);
    bsum += dz;
  }
  float* p = dW + (int64_t)n * K + k;
  FV<VEC> g = FV<VEC>::load(p);
#pragma unroll
  for (int e = 0; e < VEC; ++e) g.v[e] += acc[e];
  g.store(p);
  if (db && k == 0) db[n] += bsum;
}

// dX[b, k] = sum_n dZ[b, n] W[n, k]: a workgroup owns 64 * VEC columns (a lane reads VEC consecutive k of every row: contiguous
// per wave) and 4 samples; its four waves take n = wave, wave + 4, ...; their partial sums meet in LDS and are added in wave order.
#define GL_DX_BT 4
template <int VEC>
__global__ void __launch_bounds__(256)
gru_lin_dgrad_k(const float* __restrict__ dY, int lddy, const float* __restrict__ Y, int ldy, const float* __restrict__ W,
                float* __restrict__ dX, int lddx, int B, int N, int K) {
  __shared__ float red[4][GL_DX_BT][64 * VEC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = (blockIdx.x * 64 + lane) * VEC, b0 = blockIdx.y * GL_DX_BT;
  const bool ok = k < K;
  const int kk = ok ? k : 0;
  float acc[GL_DX_BT][VEC];
#pragma unroll
  for (int r = 0; r < GL_DX_BT; ++r)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[r][e] = 0.f;
#pragma unroll 4
  for (int n = wave; n < N; n += 4) {
    const FV<VEC> w = FV<VEC>::load(W + (int64_t)n * K + kk);
#pragma unroll
    for (int r = 0; r < GL_DX_BT; ++r) {
      const int64_t b = min(b0 + r, B - 1);
      float dz = dY[b * lddy + n];
      if (Y) dz = Y[b * ldy + n] > 0.f ? dz : 0.f;
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[r][e] = fmaf(dz, w.v[e], acc[r][e]);
    }
  }
#pragma unroll
  for (int r = 0; r < GL_DX_BT; ++r)
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[wave][r][lane * VEC + e] = acc[r][e];
  __syncthreads();
  const int r = wave;                          // wave r finishes sample b0 + r
  if (ok && b0 + r < B) {
    FV<VEC> s;
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      s.v[e] = ((red[0][r][lane * VEC + e] + red[1][r][lane * VEC + e]) + red[2][r][lane * VEC + e]) + red[3][r][lane * VEC + e];
    s.store(dX + (int64_t)(b0 + r) * lddx + k);
  }
}

static inline bool a16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int lin_check(const char* name, int B, int N, int K, int ldx, int ldy, const void* X, const void* W, const void* Y) {
  MMRCA_REQUIRE(B >= 1 && B <= 65535 * GL_DX_BT, "%s: batch %d outside [1, %d]", name, B, 65535 * GL_DX_BT);
  MMRCA_REQUIRE(N >= 1 && N <= 65536 && K >= 1 && K <= 65536, "%s: N=%d, K=%d outside [1, 65536]", name, N, K);
  MMRCA_REQUIRE(ldx >= K, "%s: row pitch %d of X is smaller than K=%d", name, ldx, K);
  MMRCA_REQUIRE(ldy >= N, "%s: row pitch %d of Y / dY is smaller than N=%d", name, ldy, N);
  MMRCA_REQUIRE(X && W && Y, "%s: null pointer", name);
  return 0;
}

extern "C" int mmrca_gru_linear_fwd(const float* X, int ldx, const float* W, const float* b, float* Y, int ldy, int B, int N, int K,
                                    int relu, void* stream) {
  if (int rc = lin_check("gru_linear_fwd", B, N, K, ldx, ldy, X, W, Y)) return rc;
  const dim3 grid((N + 3) / 4, (B + GL_BT - 1) / GL_BT);
  if (K % 4 == 0 && ldx % 4 == 0 && a16(X) && a16(W))
    hipLaunchKernelGGL((gru_lin_fwd_k<4>), grid, dim3(256), 0, (hipStream_t)stream, X, ldx, W, b, Y, ldy, B, N, K, relu);
  else
    hipLaunchKernelGGL((gru_lin_fwd_k<1>), grid, dim3(256), 0, (hipStream_t)stream, X, ldx, W, b, Y, ldy, B, N, K, relu);
  MMRCA_CHECK_LAUNCH("gru_linear_fwd");
  return 0;
}

extern "C" int mmrca_gru_linear_bwd(const float* dY, int lddy, const float* Y, int ldy, const float* X, int ldx, const float* W, float* dW,
                                    float* db, float* dX, int lddx, int B, int N, int K, void* stream) {
  if (int rc = lin_check("gru_linear_bwd", B, N, K, ldx, lddy, X, W, dY)) return rc;
  MMRCA_REQUIRE(!Y || ldy >= N, "gru_linear_bwd: row pitch %d of Y is smaller than N=%d", ldy, N);
  MMRCA_REQUIRE(dW || dX, "gru_linear_bwd: neither dW nor dX is asked for");
  if (dW) {
    if (K % 4 == 0 && ldx % 4 == 0 && a16(X) && a16(dW))
      hipLaunchKernelGGL((gru_lin_wgrad_k<4>), dim3((unsigned)(((int64_t)N * (K / 4) + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dY, lddy, Y,
                         ldy, X, ldx, dW, db, B, N, K);
    else
      hipLaunchKernelGGL((gru_lin_wgrad_k<1>), dim3((unsigned)(((int64_t)N * K + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dY, lddy, Y, ldy, X,
                         ldx, dW, db, B, N, K);
    MMRCA_CHECK_LAUNCH("gru_linear_bwd (weight gradient)");
  }
  if (dX) {
    MMRCA_REQUIRE(lddx >= K, "gru_linear_bwd: row pitch %d of dX is smaller than K=%d", lddx, K);
    const int nb = (B + GL_DX_BT - 1) / GL_DX_BT;
    if (K % 4 == 0 && lddx % 4 == 0 && a16(dX) && a16(W))
      hipLaunchKernelGGL((gru_lin_dgrad_k<4>), dim3((K + 255) / 256, nb), dim3(256), 0, (hipStream_t)stream, dY, lddy, Y, ldy, W, dX, lddx, B, N, K);
    else
      hipLaunchKernelGGL((gru_lin_dgrad_k<1>), dim3((K + 63) / 64, nb), dim3(256), 0, (hipStream_t)stream, dY, lddy, Y, ldy, W, dX, lddx, B, N, K);
    MMRCA_CHECK_LAUNCH("gru_linear_bwd (input gradient)");
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// 2. the recurrent chain (torch's GRU cell and layout: weight_hh [3H, H], bias_hh [3H], gate rows r | z | n):
//      r = s(gi_r + W_hr h + b_hr)   z = s(gi_z + W_hz h + b_hz)   n = tanh(gi_n + r (W_hn h + b_hn))   h' = (1 - z) n + z h
//    gi [T, 3H] = W_ih x_t + b_ih comes from the Linear above.  hseq [T + 1, H]: row 0 is h_{-1} (the caller's; zeros for the model),
//    row t + 1 = h_t.  Saved for the backward: gates [T, 3H] = r | z | n and hn [T, H] = W_hn h + b_hn.
//
//    Forward step: one wave per hidden unit j.  The wave holds h_{t-1} in registers (two 16-byte pieces per lane, H <= 512; the lanes
//    behind H read a clamped address and hold zero), reads rows j, H + j, 2H + j of W_hh the same way and reduces the three dot
//    products by butterfly.
// ---------------------------------------------------------------------------------------------------------------------------
#define GRU_MAX_H 512
#define GRU_MAX_N 2

struct GruFwdOne { const float* gi; const float* whh; const float* bhh; float* hseq; float* gates; float* hn; };
struct GruFwdArgs { GruFwdOne g[GRU_MAX_N]; };

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

__global__ void __launch_bounds__(256)
gru_step_fwd_k(GruFwdArgs a, int t, int H) {
  const GruFwdOne g = a.g[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 4 + wave;
  if (j >= H) return;                          // wave-uniform; no barrier below
  const float* hp = g.hseq + (int64_t)t * H;
  float4 h[2];
  int kk[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int k = lane * 4 + 256 * i;
    const bool ok = k < H;
    kk[i] = ok ? k : 0;
    const float4 v = *reinterpret_cast<const float4*>(hp + kk[i]);
    h[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float s[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const float* row = g.whh + ((int64_t)q * H + j) * H;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float4 w = *reinterpret_cast<const float4*>(row + kk[i]);
      acc = fmaf(w.x, h[i].x, fmaf(w.y, h[i].y, fmaf(w.z, h[i].z, fmaf(w.w, h[i].w, acc))));
    }
    s[q] = wave_sum(acc);
  }
  if (lane == 0) {
    const float* gi = g.gi + (int64_t)t * 3 * H;
    const float hn = s[2] + g.bhh[2 * H + j];
    const float r = sigmoid_f(gi[j] + s[0] + g.bhh[j]);
    const float z = sigmoid_f(gi[H + j] + s[1] + g.bhh[H + j]);
    const float n = tanhf(gi[2 * H + j] + r * hn);
    g.hseq[(int64_t)(t + 1) * H + j] = (1.f - z) * n + z * hp[j];
    float* gt = g.gates + (int64_t)t * 3 * H;
    gt[j] = r;
    gt[H + j] = z;
    gt[2 * H + j] = n;
    g.hn[(int64_t)t * H + j] = hn;
  }
}

// Backward step t, given dh_t = dout[t] + carry[t] (carry[t]: what step t + 1 passed down; nothing at t = T - 1):
//   dn = dh (1 - z) (1 - n^2)    dz = dh (h_{t-1} - n) z (1 - z)    dr = dn hn r (1 - r)
//   dgi[t] = dr | dz | dn        (the gradient at gi:        feeds dW_ih, db_ih, dx)
//   dgh[t] = dr | dz | dn r      (the gradient at W_hh h + b_hh: feeds dW_hh, db_hh)
//   carry[t - 1] = W_hh^T dgh[t] + z dh
// The gate gradients are elementwise, so every workgroup recomputes all 3H of them into LDS (workgroup 0 also writes them out).  A
// workgroup then owns 16 columns k of W_hh: 4 threads read one 64-byte piece of a row, 64 such groups stride the 3H rows, and the 64
// partial sums are added in order.
#define GRU_BW_KT 16

struct GruBwdOne {
  const float* whh; const float* hseq; const float* gates; const float* hn; const float* dout; int lddout;
  float* carry; float* dgi; float* dgh;
};
struct GruBwdArgs { GruBwdOne g[GRU_MAX_N]; };

__global__ void __launch_bounds__(256)
gru_step_bwd_k(GruBwdArgs a, int t, int T, int H) {
  __shared__ float dg[3 * GRU_MAX_H];
  __shared__ __attribute__((aligned(16))) float red[64][GRU_BW_KT];
  const GruBwdOne g = a.g[blockIdx.y];
  const int tid = threadIdx.x;
  const float* gt = g.gates + (int64_t)t * 3 * H;
  const float* hp = g.hseq + (int64_t)t * H;
  const bool has_carry = t < T - 1;
  for (int j = tid; j < H; j += 256) {
    const float dh = g.dout[(int64_t)t * g.lddout + j] + (has_carry ? g.carry[(int64_t)t * H + j] : 0.f);
    const float r = gt[j], z = gt[H + j], n = gt[2 * H + j];
    const float dn = dh * (1.f - z) * (1.f - n * n);
    const float dz = dh * (hp[j] - n) * z * (1.f - z);
    const float dr = dn * g.hn[(int64_t)t * H + j] * r * (1.f - r);
    dg[j] = dr;
    dg[H + j] = dz;
    dg[2 * H + j] = dn * r;
    if (blockIdx.x == 0) {
      float* o = g.dgi + (int64_t)t * 3 * H;
      float* p = g.dgh + (int64_t)t * 3 * H;
      o[j] = dr; o[H + j] = dz; o[2 * H + j] = dn;
      p[j] = dr; p[H + j] = dz; p[2 * H + j] = dn * r;
    }
  }
  if (t == 0) return;                          // uniform: nothing reads the gradient at h_{-1}
  __syncthreads();
  const int c = tid & 3, jg = tid >> 2;
  const int k = blockIdx.x * GRU_BW_KT + c * 4;
  const bool ok = k < H;
  const int kk = ok ? k : 0;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int j = jg; j < 3 * H; j += 64) {
    const float4 w = *reinterpret_cast<const float4*>(g.whh + (int64_t)j * H + kk);
    const float d = dg[j];
    acc.x = fmaf(d, w.x, acc.x); acc.y = fmaf(d, w.y, acc.y); acc.z = fmaf(d, w.z, acc.z); acc.w = fmaf(d, w.w, acc.w);
  }
  *reinterpret_cast<float4*>(&red[jg][c * 4]) = acc;
  __syncthreads();
  if (tid < GRU_BW_KT) {
    const int kc = blockIdx.x * GRU_BW_KT + tid;
    if (kc < H) {
      float s = 0.f;
      for (int q = 0; q < 64; ++q) s += red[q][tid];
      const float dh = g.dout[(int64_t)t * g.lddout + kc] + (has_carry ? g.carry[(int64_t)t * H + kc] : 0.f);
      g.carry[(int64_t)(t - 1) * H + kc] = s + gt[H + kc] * dh;
    }
  }
}

static int gru_check(const char* name, int ngru, int T, int H) {
  MMRCA_REQUIRE(ngru >= 1 && ngru <= GRU_MAX_N, "%s: %d GRUs in one chain, 1 or %d are built", name, ngru, GRU_MAX_N);
  MMRCA_REQUIRE(T >= 1 && T <= 65536, "%s: T=%d outside [1, 65536]", name, T);
  MMRCA_REQUIRE(H >= 4 && H % 4 == 0 && H <= GRU_MAX_H, "%s: H=%d must be a multiple of 4 in [4, %d]", name, H, GRU_MAX_H);
  return 0;
}

extern "C" int mmrca_gru_fwd(int ngru, const float* const* gi, const float* const* whh, const float* const* bhh, float* const* hseq,
                             float* const* gates, float* const* hn, int T, int H, void* stream) {
  if (int rc = gru_check("gru_fwd", ngru, T, H)) return rc;
  MMRCA_REQUIRE(gi && whh && bhh && hseq && gates && hn, "gru_fwd: null pointer table");
  GruFwdArgs a;
  for (int i = 0; i < GRU_MAX_N; ++i) {
    const int s = std::min(i, ngru - 1);
    MMRCA_REQUIRE(gi[s] && whh[s] && bhh[s] && hseq[s] && gates[s] && hn[s], "gru_fwd: null pointer (GRU %d)", s);
    MMRCA_REQUIRE(a16(whh[s]) && a16(hseq[s]), "gru_fwd: weight_hh and hseq must be 16-byte aligned (GRU %d)", s);
    a.g[i] = GruFwdOne{gi[s], whh[s], bhh[s], hseq[s], gates[s], hn[s]};
  }
  for (int t = 0; t < T; ++t) {
    hipLaunchKernelGGL(gru_step_fwd_k, dim3((H + 3) / 4, ngru), dim3(256), 0, (hipStream_t)stream, a, t, H);
    MMRCA_CHECK_LAUNCH("gru_fwd");
  }
  return 0;
}

extern "C" int mmrca_gru_bwd(int ngru, const float* const* whh, const float* const* hseq, const float* const* gates, const float* const* hn,
                             const float* const* dout, const int* lddout, float* const* carry, float* const* dgi, float* const* dgh, int T,
                             int H, void* stream) {
  if (int rc = gru_check("gru_bwd", ngru, T, H)) return rc;
  MMRCA_REQUIRE(whh && hseq && gates && hn && dout && lddout && carry && dgi && dgh, "gru_bwd: null pointer table");
  GruBwdArgs a;
  for (int i = 0; i < GRU_MAX_N; ++i) {
    const int s = std::min(i, ngru - 1);
    MMRCA_REQUIRE(whh[s] && hseq[s] && gates[s] && hn[s] && dout[s] && carry[s] && dgi[s] && dgh[s], "gru_bwd: null pointer (GRU %d)", s);
    MMRCA_REQUIRE(a16(whh[s]), "gru_bwd: weight_hh must be 16-byte aligned (GRU %d)", s);
    MMRCA_REQUIRE(lddout[s] >= H, "gru_bwd: row pitch %d of dout is smaller than H=%d (GRU %d)", lddout[s], H, s);
    a.g[i] = GruBwdOne{whh[s], hseq[s], gates[s], hn[s], dout[s], lddout[s], carry[s], dgi[s], dgh[s]};
  }
  for (int t = T - 1; t >= 0; --t) {
    hipLaunchKernelGGL(gru_step_bwd_k, dim3((H + GRU_BW_KT - 1) / GRU_BW_KT, ngru), dim3(256), 0, (hipStream_t)stream, a, t, T, H);
    MMRCA_CHECK_LAUNCH("gru_bwd");
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// 3. Hadamard fusion: out[b, c] = tanh(a[b, c] k1[c] + x2[b, c] k2[c] + bias[c]); a, x2 [B, C] (pitches lda, ldb), out pitch ldo.
//    Backward, with d = (d1 + d2) (1 - out^2) (two gradients arrive at `out`: concat_fc's and gru_bimodal's; d2 may be null):
//    da = d k1, db = d k2, dk1 += sum_b d a, dk2 += sum_b d x2, dbias += sum_b d.  One thread per column, the samples in order.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
hadamard_fwd_k(const float* __restrict__ a, int lda, const float* __restrict__ x2, int ldb, const float* __restrict__ k1,
               const float* __restrict__ k2, const float* __restrict__ bias, float* __restrict__ out, int ldo, int B, int C) {
  const int64_t total = (int64_t)B * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t b = i / C;
    out[b * ldo + c] = tanhf(fmaf(a[b * lda + c], k1[c], fmaf(x2[b * ldb + c], k2[c], bias[c])));
  }
}

__global__ void __launch_bounds__(256)
hadamard_bwd_k(const float* __restrict__ d1, int ld1, const float* __restrict__ d2, int ld2, const float* __restrict__ a, int lda,
               const float* __restrict__ x2, int ldb, const float* __restrict__ out, int ldo, const float* __restrict__ k1,
               const float* __restrict__ k2, float* __restrict__ da, int ldda, float* __restrict__ db, int lddb, float* __restrict__ dk1,
               float* __restrict__ dk2, float* __restrict__ dbias, int B, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float w1 = k1[c], w2 = k2[c];
  float s1 = 0.f, s2 = 0.f, sb = 0.f;
  for (int64_t b = 0; b < B; ++b) {
    const float o = out[b * ldo + c];
    const float d = (d1[b * ld1 + c] + (d2 ? d2[b * ld2 + c] : 0.f)) * (1.f - o * o);
    da[b * ldda + c] = d * w1;
    db[b * lddb + c] = d * w2;
    s1 = fmaf(d, a[b * lda + c], s1);
    s2 = fmaf(d, x2[b * ldb + c], s2);
    sb += d;
  }
  dk1[c] += s1;
  dk2[c] += s2;
  dbias[c] += sb;
}

static inline int ew_grid(int64_t total) { return (int)std::min<int64_t>((total + 255) / 256, 2048); }

extern "C" int mmrca_hadamard_fwd(const float* a, int lda, const float* x2, int ldb, const float* k1, const float* k2, const float* bias,
                                  float* out, int ldo, int B, int C, void* stream) {
  MMRCA_REQUIRE(B >= 1 && C >= 1, "hadamard_fwd: bad shape B=%d C=%d", B, C);
  MMRCA_REQUIRE(lda >= C && ldb >= C && ldo >= C, "hadamard_fwd: a row pitch (%d, %d, %d) is smaller than C=%d", lda, ldb, ldo, C);
  MMRCA_REQUIRE(a && x2 && k1 && k2 && bias && out, "hadamard_fwd: null pointer");
  hipLaunchKernelGGL(hadamard_fwd_k, dim3(ew_grid((int64_t)B * C)), dim3(256), 0, (hipStream_t)stream, a, lda, x2, ldb, k1, k2, bias, out, ldo, B, C);
  MMRCA_CHECK_LAUNCH("hadamard_fwd");
  return 0;
}

extern "C" int mmrca_hadamard_bwd(const float* d1, int ld1, const float* d2, int ld2, const float* a, int lda, const float* x2, int ldb,
                                  const float* out, int ldo, const float* k1, const float* k2, float* da, int ldda, float* db, int lddb,
                                  float* dk1, float* dk2, float* dbias, int B, int C, void* stream) {
  MMRCA_REQUIRE(B >= 1 && C >= 1, "hadamard_bwd: bad shape B=%d C=%d", B, C);
  MMRCA_REQUIRE(ld1 >= C && (!d2 || ld2 >= C) && lda >= C && ldb >= C && ldo >= C && ldda >= C && lddb >= C,
                "hadamard_bwd: a row pitch is smaller than C=%d", C);
  MMRCA_REQUIRE(d1 && a && x2 && out && k1 && k2 && da && db && dk1 && dk2 && dbias, "hadamard_bwd: null pointer");
  hipLaunchKernelGGL(hadamard_bwd_k, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, d1, ld1, d2, ld2, a, lda, x2, ldb, out, ldo, k1, k2,
                     da, ldda, db, lddb, dk1, dk2, dbias, B, C);
  MMRCA_CHECK_LAUNCH("hadamard_bwd");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// 4. dropout: y[b, c] = x[b, c] * keep / (1 - p), keep = the counter hash of (seed + mask epoch, b * C + c) >= p.  The backward is the
//    same call on the gradient with the forward's seed.  y may be x.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
dropout_f32_k(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, int B, int C, float p, float inv_keep, uint64_t seed) {
  const int64_t total = (int64_t)B * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t b = i / C;
    const float keep = (p > 0.f && mmrca_uniform(seed, (uint64_t)i) < p) ? 0.f : inv_keep;
    y[b * ldy + c] = x[b * ldx + c] * keep;
  }
}

extern "C" int mmrca_dropout_f32(const float* x, int ldx, float* y, int ldy, int B, int C, float drop_p, uint64_t seed, void* stream) {
  MMRCA_REQUIRE(B >= 1 && C >= 1, "dropout_f32: bad shape B=%d C=%d", B, C);
  MMRCA_REQUIRE(ldx >= C && ldy >= C, "dropout_f32: a row pitch (%d, %d) is smaller than C=%d", ldx, ldy, C);
  MMRCA_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "dropout_f32: drop_p %f outside [0, 1)", (double)drop_p);
  MMRCA_REQUIRE(x && y, "dropout_f32: null pointer");
  hipLaunchKernelGGL(dropout_f32_k, dim3(ew_grid((int64_t)B * C)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, B, C, drop_p,
                     drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f, seed);
  MMRCA_CHECK_LAUNCH("dropout_f32");
  return 0;
}

MMRCA_SEED_EPOCH_EXPORT(gru)   // this translation unit's copy of the mask epoch (common.h)
