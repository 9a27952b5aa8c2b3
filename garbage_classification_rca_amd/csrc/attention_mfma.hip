// K3 (fast path): fused multi-head attention on v_mfma_f32_16x16x32_bf16, head dim 64, bf16 in/out, fp32 softmax.
//
// One workgroup (4 waves) per (batch, head).  The two [S,64] operands that every wave re-reads are staged once in
// LDS (128-B rows); scores, probabilities and their gradients never leave registers:
//   * the score tile is computed TRANSPOSED, S^T = K Q^T (keys on MFMA rows, queries on lanes), so a query's whole row
//     of the softmax lives in one lane column: the row max / sum are register reductions plus two lane shuffles, and
//     the fp32 accumulator registers ARE the next MFMA's B operand (P^T for O^T = V^T P^T) after a bf16 pack --
//     no LDS round trip for P.  The contraction order inside a 32-key step is permuted by that reuse
//     (key = 32u + 16(j>>2) + 4g + (j&3) for element j of lane group g); the V^T operand is fetched in the same order
//     with ds_read_b64_tr_b16 (hardware-transposed LDS read of row-major V).
//   * LDS images: "ROW" = 16-B chunks XOR (row>>1)&7 (conflict-free ds_read_b128 fragment reads);
//                 "TR"  = 32-B granules XOR (row>>1)&3 (conflict-free transposed reads, 2-way on row reads).
//   * backward = two kernels that recompute P from the saved log-sum-exp: dQ (a wave owns 16 queries, sweeps keys) and
//     dK/dV (a wave owns 16 keys, sweeps queries); no atomics, no fp32 scratch in HBM.
// Masked keys get -inf; a query whose keys are all masked outputs zeros and lse=+inf (torch SDPA semantics).
#include "common.h"
#include <type_traits>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

#define AT_DH 64
#define AT_MAX_S 512
#define AT_MAXKT (AT_MAX_S / 16)

enum { IMG_ROW = 0, IMG_TR = 1 };

__device__ __forceinline__ int img_off(int mode, int row, int c /*16-B chunk 0..7*/) {
  if (mode == IMG_ROW) return row * 128 + ((c ^ ((row >> 1) & 7)) << 4);
  return row * 128 + ((((c >> 1) ^ ((row >> 1) & 3)) << 5) | ((c & 1) << 4));
}

// stage rows [0,S) of a [S, ld] slice (64 bf16 per row) into an LDS image with global_load_lds (HBM -> LDS DMA, 16 B per
// lane, no VGPR round trip; the caller waits on vmcnt(0) before its barrier).  The DMA writes lane-linear (one wave
// instruction = 8 image rows of 128 B), so the image's XOR swizzle -- an involution within a row for both modes -- is
// applied to the per-lane SOURCE chunk.  Rows [S, Spad) receive a copy of row S-1 instead of zeros: every consumer
// multiplies them by an exact zero (keys >= S carry a -inf score bias, queries >= S a +inf log-sum-exp).
typedef __attribute__((address_space(3))) void at_lds_void;
typedef const __attribute__((address_space(1))) void at_gbl_void;
__device__ __forceinline__ void stage_rows(char* img, int mode, const bf16_t* __restrict__ src, int64_t ld, int S, int Spad) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  for (int j = wave; j < (Spad >> 3); j += nw) {
    const int row = 8 * j + (lane >> 3), slot = lane & 7;
    const int c = mode == IMG_ROW ? (slot ^ ((row >> 1) & 7)) : ((((slot >> 1) ^ ((row >> 1) & 3)) << 1) | (slot & 1));
    const int r = row < S ? row : S - 1;
    __builtin_amdgcn_global_load_lds((at_gbl_void*)(src + (int64_t)r * ld + c * 8), (at_lds_void*)(img + j * 1024), 16, 0, 0);
  }
}

// A-role fragment, rows rb..rb+15 of an image, contraction = the 64 columns (k-step ks of 32)
__device__ __forceinline__ bf16x8 frag_rows(const char* img, int mode, int rb, int ks, int lane) {
  const int r = rb + (lane & 15), c = 4 * ks + (lane >> 4);
  return *reinterpret_cast<const bf16x8*>(img + img_off(mode, r, c));
}

// A-role fragment of the TRANSPOSED image: D-rows = columns 16dt..16dt+15, contraction = image rows in the permuted
// order  row(j) = 32u + 16(j>>2) + 4g + (j&3)
__device__ __forceinline__ bf16x8 frag_cols_tr(const char* img, int u, int dt, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int r0 = 32 * u + 4 * g + q, r1 = r0 + 16;
  const int o0 = r0 * 128 + ((dt ^ ((r0 >> 1) & 3)) << 5) + 8 * p;
  const int o1 = r1 * 128 + ((dt ^ ((r1 >> 1) & 3)) << 5) + 8 * p;
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + o0));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + o1));
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3]; r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

// B-role fragment straight from HBM: lane (i = lane&15, g) holds row (row0+i) columns 32ks+8g .. +7
__device__ __forceinline__ bf16x8 frag_global(const bf16_t* __restrict__ base, int64_t ld, int row0, int S, int ks, int lane) {
  int r = row0 + (lane & 15);
  if (r > S - 1) r = S - 1;
  return *reinterpret_cast<const bf16x8*>(base + (int64_t)r * ld + 32 * ks + 8 * (lane >> 4));
}

__device__ __forceinline__ bf16x8 pack_pair(const f32x4& a, const f32x4& b) {
  bf16x8 r;
  r[0] = (bf16_t)a[0]; r[1] = (bf16_t)a[1]; r[2] = (bf16_t)a[2]; r[3] = (bf16_t)a[3];
  r[4] = (bf16_t)b[0]; r[5] = (bf16_t)b[1]; r[6] = (bf16_t)b[2]; r[7] = (bf16_t)b[3];
  return r;
}

// attention-probability dropout: keep-scale of element (row q, key) of head bh
__device__ __forceinline__ float attn_keep(float p, float sc, uint64_t seed, int64_t bh, int S, int q, int key) {
  return mmrca_uniform(seed, ((uint64_t)bh * S + q) * S + key) >= p ? sc : 0.f;
}

__device__ __forceinline__ float colgroup_max(float x) { x = fmaxf(x, __shfl_xor(x, 16, 64)); return fmaxf(x, __shfl_xor(x, 32, 64)); }
__device__ __forceinline__ float colgroup_sum(float x) { x += __shfl_xor(x, 16, 64); return x + __shfl_xor(x, 32, 64); }

// key validity as an additive score bias in LDS: 0 for a live key, -inf for a masked or padded one.  (Testing
// key_mask[] per score element cost a branch and a global load per element per query tile; the bias is one broadcast
// ds_read_b128 per key tile and folds into the scale multiply as an fma.)
__device__ __forceinline__ void stage_key_bias(float* kb, const int32_t* __restrict__ seq_mask, int S, int Spad) {
  for (int key = threadIdx.x; key < Spad; key += blockDim.x)
    kb[key] = (key < S && (!seq_mask || seq_mask[key] != 0)) ? 0.f : -INFINITY;
}

// Sequence b of the batch: rows [row0, row0 + S) of the token-major buffers.  Padded layout (cu == nullptr): row0 = b*Smax,
// S = Smax.  Packed layout: cu[B+1] are the cumulative sequence lengths (captions stored back to back without their
// padding), Smax only strides the lse / dropout-counter index spaces, which stay those of the padded layout.
#define AT_SEQ(b_, Smax_, cu_)                                      \
  const int row0 = (cu_) ? (cu_)[b_] : (b_) * (Smax_);              \
  const int S = (cu_) ? (cu_)[(b_) + 1] - (cu_)[b_] : (Smax_);      \
  if (S <= 0) return;

#define LOG2E 1.4426950408889634f
#define LN2 0.6931471805599453f

// ------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------
// NW waves per block share the two LDS images: LDS (2 x 28 KiB at S=197) allows two blocks per CU, so NW = 8 is what puts
// four waves on every SIMD (the kernels are latency-bound on LDS reads between dependent MFMAs) and halves the number of
// tiles a wave walks.
template <int NKT, bool DROP, int NW>     // key tiles of 16 (Spad = 16*NKT, NKT even); DROP: attention-probability dropout compiled in
__global__ void __launch_bounds__(64 * NW, NW / 2)
mha_fwd_mfma_k(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ key_mask, bf16_t* __restrict__ out,
               float* __restrict__ lse, int H, int Smax, float scale, float drop_p, uint64_t drop_seed,
               const int32_t* __restrict__ cu) {
  const float drop_sc = DROP ? 1.f / (1.f - drop_p) : 1.f;
  extern __shared__ __attribute__((aligned(16))) char sm[];
  constexpr int Spad = NKT * 16;
  char* Kimg = sm; char* Vimg = sm + Spad * 128;
  float* kb = reinterpret_cast<float*>(sm + 2 * Spad * 128);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  AT_SEQ(b, Smax, cu)
  const int64_t ld = 3LL * H * AT_DH;
  const bf16_t* Q = qkv + (int64_t)row0 * ld + h * AT_DH;
  const bf16_t* Kp = Q + H * AT_DH;
  const bf16_t* Vp = Kp + H * AT_DH;
  stage_rows(Kimg, IMG_ROW, Kp, ld, S, Spad);
  stage_rows(Vimg, IMG_TR, Vp, ld, S, Spad);
  stage_key_bias(kb, key_mask ? key_mask + row0 : nullptr, S, Spad);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const float c1 = scale * LOG2E;                    // scores live in the exp2 domain
  const int nqt = (S + 15) / 16;
  for (int qt = wave; qt < nqt; qt += NW) {
    const int q0 = qt * 16;
    const bf16x8 qf0 = frag_global(Q, ld, q0, S, 0, lane), qf1 = frag_global(Q, ld, q0, S, 1, lane);
    f32x4 s[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const bf16x8 kf0 = frag_rows(Kimg, IMG_ROW, kt * 16, 0, lane), kf1 = frag_rows(Kimg, IMG_ROW, kt * 16, 1, lane);
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf0, qf0, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf1, qf1, a, 0, 0, 0);
      s[kt] = a;
      // keep the scheduler from hoisting every K fragment of the row up front (it then needs > 128 VGPRs and spills);
      // with four waves per SIMD the other waves cover this tile's LDS latency
      if (NW > 4 && (kt & 1)) __builtin_amdgcn_sched_barrier(0);
    }
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const f32x4 bias = *reinterpret_cast<const f32x4*>(kb + kt * 16 + 4 * g);     // keys 16kt + 4g + r
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = fmaf(s[kt][r], c1, bias[r]);
        s[kt][r] = v;
        m = fmaxf(m, v);
      }
    }
    m = colgroup_max(m);
    float l = 0.f;
    const float msafe = m > -INFINITY ? m : 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) { const float e = __builtin_amdgcn_exp2f(s[kt][r] - msafe); s[kt][r] = e; l += e; }
    l = colgroup_sum(l);
    if (DROP) {      // dropout acts on the normalised probabilities: mask the numerators, keep the denominator
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          s[kt][r] *= attn_keep(drop_p, drop_sc, drop_seed, blockIdx.x, Smax, q0 + l16, kt * 16 + 4 * g + r);
    }
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NKT / 2; ++u) {
      const bf16x8 pf = pack_pair(s[2 * u], s[2 * u + 1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8 vf = frag_cols_tr(Vimg, u, dt, lane);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);   // O^T[d][q]
      }
      if (NW > 4) __builtin_amdgcn_sched_barrier(0);
    }
    const int q = q0 + l16;
    if (q < S) {
      const float inv = l > 0.f ? 1.f / l : 0.f;
      bf16_t* orow = out + ((int64_t)row0 + q) * (H * AT_DH) + h * AT_DH;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (bf16_t)(o[dt][r] * inv);
        *reinterpret_cast<bf16x4*>(orow + dt * 16 + 4 * g) = v;
      }
      if (g == 0) lse[((int64_t)b * H + h) * Smax + q] = l > 0.f ? m * LN2 + __logf(l) : INFINITY;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// forward with fp32 ACCURACY on the bf16 matrix cores ("bf16x3" attention: the bf16x3f mode's forward)
// ------------------------------------------------------------------------------------------------------
// q | k | v arrive as the two bf16 planes a bf16x3 GEMM wrote (value = hi + lo to 2^-17) and every product is formed as in
// gemm_x3.hip: S = K_hi Q_hi + K_lo Q_hi + K_hi Q_lo, O = V_hi P_hi + V_lo P_hi + V_hi P_lo with P = P_hi + P_lo split in registers
// (lo x lo is below fp32 resolution), fp32 softmax statistics in between -- the arithmetic of the fp32-matrix-core kernels of
// attention_f32.hip to ~1e-6, at the bf16 MFMA rate (the fp32 pipe is 1/16 of it: those kernels spend half of their 495 us per
// ViT layer in MFMAs).  Four LDS images (K_hi, K_lo, V_hi, V_lo) by LDS-DMA; same mask / packed-layout / dropout / lse contract as
// mha_fwd_mfma_k; the context is written as two planes (what the out-projection GEMM and the bf16 backward read).
template <int NKT, bool DROP, int NW>
__global__ void __launch_bounds__(64 * NW)
mha_fwd_x3_k(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ qkv_lo, const int32_t* __restrict__ key_mask,
             bf16_t* __restrict__ out_hi, bf16_t* __restrict__ out_lo, float* __restrict__ lse, int H, int Smax, float scale,
             float drop_p, uint64_t drop_seed, const int32_t* __restrict__ cu) {
  const float drop_sc = DROP ? 1.f / (1.f - drop_p) : 1.f;
  extern __shared__ __attribute__((aligned(16))) char sm[];
  constexpr int Spad = NKT * 16, IMG = Spad * 128;
  char* Kh = sm; char* Kl = sm + IMG; char* Vh = sm + 2 * IMG; char* Vl = sm + 3 * IMG;
  float* kb = reinterpret_cast<float*>(sm + 4 * IMG);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  AT_SEQ(b, Smax, cu)
  const int64_t ld = 3LL * H * AT_DH;
  const int64_t q_off = (int64_t)row0 * ld + h * AT_DH, k_off = q_off + H * AT_DH, v_off = k_off + H * AT_DH;
  stage_rows(Kh, IMG_ROW, qkv + k_off, ld, S, Spad);
  stage_rows(Kl, IMG_ROW, qkv_lo + k_off, ld, S, Spad);
  stage_rows(Vh, IMG_TR, qkv + v_off, ld, S, Spad);
  stage_rows(Vl, IMG_TR, qkv_lo + v_off, ld, S, Spad);
  stage_key_bias(kb, key_mask ? key_mask + row0 : nullptr, S, Spad);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const float c1 = scale * LOG2E;                    // scores live in the exp2 domain
  const int nqt = (S + 15) / 16;
  for (int qt = wave; qt < nqt; qt += NW) {
    const int q0 = qt * 16;
    const bf16x8 qh0 = frag_global(qkv + q_off, ld, q0, S, 0, lane), qh1 = frag_global(qkv + q_off, ld, q0, S, 1, lane);
    const bf16x8 ql0 = frag_global(qkv_lo + q_off, ld, q0, S, 0, lane), ql1 = frag_global(qkv_lo + q_off, ld, q0, S, 1, lane);
    f32x4 s[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const bf16x8 kh0 = frag_rows(Kh, IMG_ROW, kt * 16, 0, lane), kh1 = frag_rows(Kh, IMG_ROW, kt * 16, 1, lane);
      const bf16x8 kl0 = frag_rows(Kl, IMG_ROW, kt * 16, 0, lane), kl1 = frag_rows(Kl, IMG_ROW, kt * 16, 1, lane);
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl0, qh0, a, 0, 0, 0);      // the small terms first
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl1, qh1, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh0, ql0, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh1, ql1, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh0, qh0, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh1, qh1, a, 0, 0, 0);
      s[kt] = a;
      if (kt & 1) __builtin_amdgcn_sched_barrier(0);
    }
    float mm = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const f32x4 bias = *reinterpret_cast<const f32x4*>(kb + kt * 16 + 4 * g);     // keys 16kt + 4g + r
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = fmaf(s[kt][r], c1, bias[r]);
        s[kt][r] = v;
        mm = fmaxf(mm, v);
      }
    }
    mm = colgroup_max(mm);
    float ll = 0.f;
    const float msafe = mm > -INFINITY ? mm : 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) { const float e = __builtin_amdgcn_exp2f(s[kt][r] - msafe); s[kt][r] = e; ll += e; }
    ll = colgroup_sum(ll);
    if (DROP) {      // dropout acts on the normalised probabilities: mask the numerators, keep the denominator
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] *= attn_keep(drop_p, drop_sc, drop_seed, blockIdx.x, Smax, q0 + l16, kt * 16 + 4 * g + r);
    }
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NKT / 2; ++u) {
      const bf16x8 ph = pack_pair(s[2 * u], s[2 * u + 1]);
      f32x4 ra, rb;
#pragma unroll
      for (int r = 0; r < 4; ++r) { ra[r] = s[2 * u][r] - (float)ph[r]; rb[r] = s[2 * u + 1][r] - (float)ph[4 + r]; }
      const bf16x8 pl = pack_pair(ra, rb);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8 vh = frag_cols_tr(Vh, u, dt, lane), vl = frag_cols_tr(Vl, u, dt, lane);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vl, ph, o[dt], 0, 0, 0);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, pl, o[dt], 0, 0, 0);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, ph, o[dt], 0, 0, 0);   // O^T[d][q]
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    const int q = q0 + l16;
    if (q < S) {
      const float inv = ll > 0.f ? 1.f / ll : 0.f;
      const int64_t off = ((int64_t)row0 + q) * (H * AT_DH) + h * AT_DH;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 vh, vl;
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float v = o[dt][r] * inv; vh[r] = (bf16_t)v; vl[r] = (bf16_t)(v - (float)vh[r]); }
        *reinterpret_cast<bf16x4*>(out_hi + off + dt * 16 + 4 * g) = vh;
        *reinterpret_cast<bf16x4*>(out_lo + off + dt * 16 + 4 * g) = vl;
      }
      if (g == 0) lse[((int64_t)b * H + h) * Smax + q] = ll > 0.f ? mm * LN2 + __logf(ll) : INFINITY;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// bf16x3 forward over key CHUNKS (225 <= Smax <= 512: the text encoders at their full context in the bf16x3f mode)
// ------------------------------------------------------------------------------------------------------
// mha_fwd_x3_k keeps the four images of a whole head resident: 112 KiB at 14 key tiles, 256 KiB at S = 512 (a CU has 160).  Here the
// images hold AT_CK = 128 keys at a time (64 KiB + the key bias: two workgroups fit on a CU, so one stages while the other computes)
// and a workgroup of 8 waves owns 128 queries of one head, a wave 16 of them for the whole walk over the head's key chunks: its Q
// fragments, its O accumulators and a running maximum / sum per query row stay in registers.  Per chunk the arithmetic is
// mha_fwd_x3_k's (small terms first, P split in registers, exp2 domain); between chunks O and the sum are rescaled by
// exp2(m_old - m_new).  A chunk without a live key for a row gives m_new == m_old: factor 1 (also when both are -inf), numerators 0,
// so maximum, sum and O keep their bits -- which is why a packed run (only the live keys are walked: ceil(len / 128) chunks, and of
// the last one only its live 32-key pairs are staged and multiplied) equals the padded run on every kept row.  Chunk boundaries are
// the fixed key indices 128, 256, 384 in both layouts.  No atomics.
#define AT_CK 128
#define AT_CKT (AT_CK / 16)
template <bool DROP>
__global__ void __launch_bounds__(512, 4)
mha_fwd_x3_c_k(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ qkv_lo, const int32_t* __restrict__ key_mask,
               bf16_t* __restrict__ out_hi, bf16_t* __restrict__ out_lo, float* __restrict__ lse, int H, int Smax, float scale,
               float drop_p, uint64_t drop_seed, const int32_t* __restrict__ cu, int nqg) {
  const float drop_sc = DROP ? 1.f / (1.f - drop_p) : 1.f;
  extern __shared__ __attribute__((aligned(16))) char sm[];
  constexpr int IMG = AT_CK * 128;
  char* Kh = sm; char* Kl = sm + IMG; char* Vh = sm + 2 * IMG; char* Vl = sm + 3 * IMG;
  float* kb = reinterpret_cast<float*>(sm + 4 * IMG);           // the key bias of the WHOLE sequence: AT_MAX_S floats
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
  const int bh = blockIdx.x / nqg, qg = blockIdx.x % nqg;
  const int b = bh / H, h = bh % H;
  AT_SEQ(b, Smax, cu)
  if (qg * 128 >= S) return;                                    // (the whole workgroup: no barrier is left waiting)
  const int64_t ld = 3LL * H * AT_DH;
  const int64_t q_off = (int64_t)row0 * ld + h * AT_DH, k_off = q_off + H * AT_DH, v_off = k_off + H * AT_DH;
  const int nch = (S + AT_CK - 1) / AT_CK;
  stage_key_bias(kb, key_mask ? key_mask + row0 : nullptr, S, nch * AT_CK);
  const float c1 = scale * LOG2E;                    // scores live in the exp2 domain
  const int q0 = (qg * 8 + wave) * 16;
  const bool has_tile = q0 < S;                      // wave-uniform
  bf16x8 qh0, qh1, ql0, ql1;
  if (has_tile) {
    qh0 = frag_global(qkv + q_off, ld, q0, S, 0, lane); qh1 = frag_global(qkv + q_off, ld, q0, S, 1, lane);
    ql0 = frag_global(qkv_lo + q_off, ld, q0, S, 0, lane); ql1 = frag_global(qkv_lo + q_off, ld, q0, S, 1, lane);
  }
  float mrun = -INFINITY, lrun = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < nch; ++c) {
    const int key0 = c * AT_CK;
    const int nk = S - key0 < AT_CK ? S - key0 : AT_CK;         // live keys of this chunk, >= 1
    const int nkp = (nk + 31) & ~31;                            // staged and multiplied: whole 32-key pairs
    if (c) __syncthreads();                                     // every wave has left the previous chunk's images
    stage_rows(Kh, IMG_ROW, qkv + k_off + key0 * ld, ld, nk, nkp);
    stage_rows(Kl, IMG_ROW, qkv_lo + k_off + key0 * ld, ld, nk, nkp);
    stage_rows(Vh, IMG_TR, qkv + v_off + key0 * ld, ld, nk, nkp);
    stage_rows(Vl, IMG_TR, qkv_lo + v_off + key0 * ld, ld, nk, nkp);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!has_tile) continue;
    f32x4 s[AT_CKT];
#pragma unroll
    for (int kt = 0; kt < AT_CKT; ++kt) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (kt * 16 < nkp) {                                      // wave-uniform; rows past nkp were not staged
        const bf16x8 kh0 = frag_rows(Kh, IMG_ROW, kt * 16, 0, lane), kh1 = frag_rows(Kh, IMG_ROW, kt * 16, 1, lane);
        const bf16x8 kl0 = frag_rows(Kl, IMG_ROW, kt * 16, 0, lane), kl1 = frag_rows(Kl, IMG_ROW, kt * 16, 1, lane);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl0, qh0, a, 0, 0, 0);      // the small terms first
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl1, qh1, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh0, ql0, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh1, ql1, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh0, qh0, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh1, qh1, a, 0, 0, 0);
      }
      s[kt] = a;
      if (kt & 1) __builtin_amdgcn_sched_barrier(0);
    }
    float mc = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < AT_CKT; ++kt) {
      const f32x4 bias = *reinterpret_cast<const f32x4*>(kb + key0 + kt * 16 + 4 * g);     // keys key0 + 16kt + 4g + r
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = fmaf(s[kt][r], c1, bias[r]);
        s[kt][r] = v;
        mc = fmaxf(mc, v);
      }
    }
    const float mnew = fmaxf(mrun, colgroup_max(mc));
    // rescale factor of what the earlier chunks left: 1 when the maximum did not move (also -inf -> -inf, where the difference
    // would be NaN), 0 when this chunk holds the row's first live key
    const float alpha = mnew == mrun ? 1.f : __builtin_amdgcn_exp2f(mrun - mnew);
    const float msafe = mnew > -INFINITY ? mnew : 0.f;
    float lc = 0.f;
#pragma unroll
    for (int kt = 0; kt < AT_CKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) { const float e = __builtin_amdgcn_exp2f(s[kt][r] - msafe); s[kt][r] = e; lc += e; }
    lrun = lrun * alpha + colgroup_sum(lc);
    mrun = mnew;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
    if (DROP) {      // dropout acts on the normalised probabilities: mask the numerators, keep the denominator
#pragma unroll
      for (int kt = 0; kt < AT_CKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] *= attn_keep(drop_p, drop_sc, drop_seed, bh, Smax, q0 + l16, key0 + kt * 16 + 4 * g + r);
    }
#pragma unroll
    for (int u = 0; u < AT_CKT / 2; ++u) {
      if (u * 32 < nkp) {                                       // wave-uniform
        const bf16x8 ph = pack_pair(s[2 * u], s[2 * u + 1]);
        f32x4 ra, rb;
#pragma unroll
        for (int r = 0; r < 4; ++r) { ra[r] = s[2 * u][r] - (float)ph[r]; rb[r] = s[2 * u + 1][r] - (float)ph[4 + r]; }
        const bf16x8 pl = pack_pair(ra, rb);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16x8 vh = frag_cols_tr(Vh, u, dt, lane), vl = frag_cols_tr(Vl, u, dt, lane);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vl, ph, o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, pl, o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, ph, o[dt], 0, 0, 0);   // O^T[d][q]
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const int q = q0 + l16;
  if (has_tile && q < S) {
    const float inv = lrun > 0.f ? 1.f / lrun : 0.f;
    const int64_t off = ((int64_t)row0 + q) * (H * AT_DH) + h * AT_DH;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16x4 vh, vl;
#pragma unroll
      for (int r = 0; r < 4; ++r) { const float v = o[dt][r] * inv; vh[r] = (bf16_t)v; vl[r] = (bf16_t)(v - (float)vh[r]); }
      *reinterpret_cast<bf16x4*>(out_hi + off + dt * 16 + 4 * g) = vh;
      *reinterpret_cast<bf16x4*>(out_lo + off + dt * 16 + 4 * g) = vl;
    }
    if (g == 0) lse[((int64_t)b * H + h) * Smax + q] = lrun > 0.f ? mrun * LN2 + __logf(lrun) : INFINITY;
  }
}

// ------------------------------------------------------------------------------------------------------
// forward, persistent over heads (unmasked, no dropout, padded layout: the ViT's attention)
// ------------------------------------------------------------------------------------------------------
// The per-head kernel above spends half of its waves' lifetime parked: all waves of a (b,h) wait for the 50 KB K/V staging and
// for their Q fragments, then run stage -> QK^T -> softmax -> PV in lockstep on one or two tiles each.  Here a workgroup of NW
// waves (one query tile per wave) walks heads bh = blockIdx.x, + gridDim.x, ... with TWO sets of LDS images: the DMA for the
// next head and the next head's Q fragments are issued right after the barrier that opens the current head and land under
// its MFMAs.  Fragment reads are inline asm (a C++ LDS read next to an in-flight global_load_lds makes hipcc insert
// s_waitcnt vmcnt(0) in front of it, which would wait for the NEXT head's staging: see lds_asm.h); the key bias of the two
// partly dead key tiles lives in registers, so the loop body has no compiler-visible LDS access at all.
#define AT_DS_B128_OFF(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off))
#define AT_DS_TR_OFF(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off))
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}

template <int NKT, int NW>
__global__ void __launch_bounds__(64 * NW)
mha_fwd_mfma_p_k(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, float* __restrict__ lse, int H, int S, float scale, int nbh) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  constexpr int Spad = NKT * 16, IMG = Spad * 128;
  const unsigned lds0 = (unsigned)(uintptr_t)(at_lds_void*)sm;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
  const int64_t ld = 3LL * H * AT_DH;
  const float c1 = scale * LOG2E;
  const int nqt = (S + 15) / 16;
  const int qt = wave;
  const bool has_tile = qt < nqt;
  // per-lane byte offsets of the fragment reads inside an image; the XOR swizzles depend on (row >> 1) & 7 resp. & 3, which a
  // step of 16 (key tile) or 32 (key pair) rows does not change, so a tile / pair index is a plain multiple of 2 / 4 KiB
  const unsigned ksw = (l16 >> 1) & 7;
  const unsigned koff0 = l16 * 128 + (((unsigned)g ^ ksw) << 4), koff1 = l16 * 128 + (((unsigned)(4 + g) ^ ksw) << 4);
  const int qq = l16 >> 2, pp = l16 & 3, vsw = (2 * g + (qq >> 1)) & 3;
  unsigned voff[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) voff[dt] = (4 * g + qq) * 128 + ((dt ^ vsw) << 5) + 8 * pp;

  int bh = blockIdx.x;
  if (bh >= nbh) return;
  auto stage_head = [&](int slot, int bh_) {
    const bf16_t* Kp = qkv + (int64_t)(bh_ / H) * S * ld + (int64_t)H * AT_DH + (bh_ % H) * AT_DH;
    stage_rows(sm + slot * 2 * IMG, IMG_ROW, Kp, ld, S, Spad);
    stage_rows(sm + slot * 2 * IMG + IMG, IMG_TR, Kp + (int64_t)H * AT_DH, ld, S, Spad);
  };
  auto q_frags = [&](int bh_, bf16x8& f0, bf16x8& f1) {
    const bf16_t* Q = qkv + (int64_t)(bh_ / H) * S * ld + (bh_ % H) * AT_DH;
    f0 = frag_global(Q, ld, qt * 16, S, 0, lane); f1 = frag_global(Q, ld, qt * 16, S, 1, lane);
  };
  stage_head(0, bh);
  bf16x8 qf0, qf1;
  if (has_tile) q_frags(bh, qf0, qf1);
  int cur = 0;
  for (;;) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                    // images of head bh complete; the other slot's last readers have passed
    const int nxt = bh + (int)gridDim.x;
    if (nxt < nbh) stage_head(cur ^ 1, nxt);
    if (has_tile) {
      // instruction diet (the tile body is bound by VALU + LDS issue): LDS reads take their tile / pair index as an
      // immediate offset (no address arithmetic), the row maximum is taken over the raw scores and scale + maximum fold
      // into one fma inside the exponential's argument, the row sum comes from one all-ones MFMA per key pair
      const unsigned kb0 = lds0 + cur * 2 * IMG + koff0, kb1 = lds0 + cur * 2 * IMG + koff1, vimg = lds0 + cur * 2 * IMG + IMG;
      const unsigned vb[4] = {vimg + voff[0], vimg + voff[1], vimg + voff[2], vimg + voff[3]};
      f32x4 s[NKT];
      static_for<0, NKT>([&](auto ic) {
        constexpr int kt = decltype(ic)::value;
        bf16x8 kf0, kf1;
        AT_DS_B128_OFF(kf0, kb0, kt * 2048);
        AT_DS_B128_OFF(kf1, kb1, kt * 2048);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kf0), "+v"(kf1));
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf0, qf0, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf1, qf1, a, 0, 0, 0);
        s[kt] = a;
      });
      if (nxt < nbh) q_frags(nxt, qf0, qf1);     // the Q fragments are dead now: the next head's load straight into them
      float m = -INFINITY;              // maximum of the RAW scores of the live keys (c1 > 0)
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // keys of the last two key tiles that lie beyond S are dead (kept out of registers: the loop body must not spill --
          // a scratch reload counts in vmcnt and would wait for the next head's staging)
          if (kt >= NKT - 2) s[kt][r] = kt * 16 + 4 * g + r < S ? s[kt][r] : -INFINITY;
          m = fmaxf(m, s[kt][r]);
        }
      m = colgroup_max(m);
      const float mc = -m * c1;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] = __builtin_amdgcn_exp2f(fmaf(s[kt][r], c1, mc));
      f32x4 o[4], osum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      bf16x8 ones;
#pragma unroll
      for (int j = 0; j < 8; ++j) ones[j] = (bf16_t)1.0f;
      static_for<0, NKT / 2>([&](auto ic) {
        constexpr int u = decltype(ic)::value;
        const bf16x8 pf = pack_pair(s[2 * u], s[2 * u + 1]);
        bf16x4 lo[4], hi[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { AT_DS_TR_OFF(lo[dt], vb[dt], u * 4096); AT_DS_TR_OFF(hi[dt], vb[dt], u * 4096 + 2048); }
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo[0]), "+v"(hi[0]), "+v"(lo[1]), "+v"(hi[1]), "+v"(lo[2]), "+v"(hi[2]), "+v"(lo[3]), "+v"(hi[3]));
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_shufflevector(lo[dt], hi[dt], 0, 1, 2, 3, 4, 5, 6, 7), pf, o[dt], 0, 0, 0);   // O^T[d][q]
        osum = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pf, osum, 0, 0, 0);      // every row: sum_k P[q][k] (of the bf16 values PV uses)
      });
      const float l = osum[0];          // >= 1: the row maximum contributes exp2(0)
      m = m * c1;
      const int q = qt * 16 + l16;
      if (q < S) {
        const float inv = 1.f / l;
        const int b = bh / H, h = bh % H;
        bf16_t* orow = out + ((int64_t)b * S + q) * (H * AT_DH) + h * AT_DH;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          bf16x4 v;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = (bf16_t)(o[dt][r] * inv);
          *reinterpret_cast<bf16x4*>(orow + dt * 16 + 4 * g) = v;
        }
        if (g == 0) lse[(int64_t)bh * S + q] = m * LN2 + __logf(l);
      }
    }
    if (nxt >= nbh) break;
    bh = nxt; cur ^= 1;
  }
}

// ------------------------------------------------------------------------------------------------------
// bf16x3 forward, persistent over heads (round 6; unmasked, no dropout, padded layout, 193 <= S <= 224: the ViT's attention in the
// bf16x3f mode).  mha_fwd_x3_k above is one workgroup per head and CU -- its four images (K_hi K_lo V_hi V_lo, 112 KiB at S = 197) leave
// no room for a second workgroup or a second set of images -- so every head waits for its whole staging with nothing to overlap it:
// ~20 us per head of which the matrix pipe is busy ~4.  Here a 16-wave workgroup (one query tile per wave) walks heads bh =
// blockIdx.x, + gridDim.x, ... and the K and V image pairs TIME-SHARE the pipeline instead of being doubled: a head is two phases,
//   A: S^T = K Q^T (three plane pairs) + softmax -- reads the K pair only, while the V pair of the SAME head lands by LDS-DMA;
//   B: O^T = V^T P^T (three plane pairs)        -- reads the V pair only, while the K pair of the NEXT head lands,
// each closed by vmcnt(0) + barrier (the pair just read is free, the pair just loaded is complete).  The next head's Q fragments
// are loaded during phase B into the registers phase A has finished with.  All LDS reads are inline asm (see mha_fwd_mfma_p_k).
// ------------------------------------------------------------------------------------------------------
// stage_rows with the lane id passed in (an opaque copy: per-lane source offsets are then recomputed at every call instead of being
// hoisted out of the head loop and spilled) and 32-bit element offsets from a wave-uniform base
__device__ __forceinline__ void stage_rows_l(unsigned img_lds, int mode, const bf16_t* __restrict__ src, int ld, int S, int Spad, int wave, int lane, int nw) {
  for (int j = wave; j < (Spad >> 3); j += nw) {
    const int row = 8 * j + (lane >> 3), slot = lane & 7;
    const int c = mode == IMG_ROW ? (slot ^ ((row >> 1) & 7)) : ((((slot >> 1) ^ ((row >> 1) & 3)) << 1) | (slot & 1));
    const int r = row < S ? row : S - 1;
    __builtin_amdgcn_global_load_lds((at_gbl_void*)(src + (unsigned)(r * ld + c * 8)), (at_lds_void*)(uintptr_t)(img_lds + j * 1024), 16, 0, 0);
  }
}

template <int NKT, int NW>
__global__ void __launch_bounds__(64 * NW)
mha_fwd_x3_p_k(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ qkv_lo, bf16_t* __restrict__ out_hi, bf16_t* __restrict__ out_lo,
               float* __restrict__ lse, int H, int S, float scale, int nbh) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  constexpr int Spad = NKT * 16, IMG = Spad * 128;        // images: K_hi | K_lo | V_hi | V_lo
  const unsigned lds0 = (unsigned)(uintptr_t)(at_lds_void*)sm;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ld = 3 * H * AT_DH;
  const float c1 = scale * LOG2E;
  const int nqt = (S + 15) / 16;
  const int qt = wave;
  const bool has_tile = qt < nqt;

  int bh = blockIdx.x;
  if (bh >= nbh) return;
  auto head_base = [&](int bh_) { return (int64_t)(bh_ / H) * S * ld + (bh_ % H) * AT_DH; };       // wave-uniform
  auto stage_k = [&](int bh_) {
    int lo_ = lane; asm volatile("" : "+v"(lo_));
    const int64_t o = head_base(bh_) + (int64_t)H * AT_DH;
    stage_rows_l(lds0, IMG_ROW, qkv + o, ld, S, Spad, wave, lo_, NW);
    stage_rows_l(lds0 + IMG, IMG_ROW, qkv_lo + o, ld, S, Spad, wave, lo_, NW);
  };
  auto stage_v = [&](int bh_) {
    int lo_ = lane; asm volatile("" : "+v"(lo_));
    const int64_t o = head_base(bh_) + 2 * (int64_t)H * AT_DH;
    stage_rows_l(lds0 + 2 * IMG, IMG_TR, qkv + o, ld, S, Spad, wave, lo_, NW);
    stage_rows_l(lds0 + 3 * IMG, IMG_TR, qkv_lo + o, ld, S, Spad, wave, lo_, NW);
  };
  bf16x8 qh0, qh1, ql0, ql1;
  auto q_frags = [&](int bh_) {
    int lo_ = lane; asm volatile("" : "+v"(lo_));
    const int64_t o = head_base(bh_);
    int r = qt * 16 + (lo_ & 15);
    if (r > S - 1) r = S - 1;
    const unsigned e = (unsigned)(r * ld + 8 * (lo_ >> 4));
    qh0 = *reinterpret_cast<const bf16x8*>(qkv + o + e); qh1 = *reinterpret_cast<const bf16x8*>(qkv + o + e + 32);
    ql0 = *reinterpret_cast<const bf16x8*>(qkv_lo + o + e); ql1 = *reinterpret_cast<const bf16x8*>(qkv_lo + o + e + 32);
  };
  stage_k(bh);
  if (has_tile) q_frags(bh);
  for (;;) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                    // the K pair of head bh is complete; every wave has left the V pair of the previous head
    stage_v(bh);                        // lands under phase A
    const int nxt = bh + (int)gridDim.x;
    f32x4 s[NKT];
    float m = -INFINITY, l = 0.f;
    if (has_tile) {
      // ---- phase A: scores (the small terms first, as in mha_fwd_x3_k) and the softmax numerators
      int lo_ = lane; asm volatile("" : "+v"(lo_));
      const int g = lo_ >> 4, l16 = lo_ & 15;
      const unsigned ksw = (l16 >> 1) & 7;
      const unsigned kb0 = lds0 + l16 * 128 + (((unsigned)g ^ ksw) << 4), kb1 = lds0 + l16 * 128 + (((unsigned)(4 + g) ^ ksw) << 4);
      static_for<0, NKT>([&](auto ic) {
        constexpr int kt = decltype(ic)::value;
        bf16x8 kh0, kh1, kl0, kl1;
        AT_DS_B128_OFF(kh0, kb0, kt * 2048);
        AT_DS_B128_OFF(kh1, kb1, kt * 2048);
        AT_DS_B128_OFF(kl0, kb0, IMG + kt * 2048);
        AT_DS_B128_OFF(kl1, kb1, IMG + kt * 2048);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kh0), "+v"(kh1), "+v"(kl0), "+v"(kl1));
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl0, qh0, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl1, qh1, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh0, ql0, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh1, ql1, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh0, qh0, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh1, qh1, a, 0, 0, 0);
        s[kt] = a;
      });
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (kt >= NKT - 2) s[kt][r] = kt * 16 + 4 * g + r < S ? s[kt][r] : -INFINITY;      // keys past the sequence end are dead
          m = fmaxf(m, s[kt][r]);
        }
      m = colgroup_max(m);              // maximum of the RAW scores (c1 > 0); finite: there is no mask
      const float mc = -m * c1;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float e = __builtin_amdgcn_exp2f(fmaf(s[kt][r], c1, mc)); s[kt][r] = e; l += e; }
      l = colgroup_sum(l);              // fp32 row sum (>= 1)
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                    // the V pair of head bh is complete; every wave has left the K pair
    if (nxt < nbh) stage_k(nxt);        // lands under phase B
    if (has_tile) {
      // ---- phase B: O^T = V^T P^T with P = P_hi + P_lo split in registers
      int lo_ = lane; asm volatile("" : "+v"(lo_));
      const int g = lo_ >> 4, l16 = lo_ & 15;
      const int qq = l16 >> 2, pp = l16 & 3, vsw = (2 * g + (qq >> 1)) & 3;
      const unsigned vimg = lds0 + 2 * IMG + (4 * g + qq) * 128 + 8 * pp;
      f32x4 o[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      static_for<0, NKT / 2>([&](auto ic) {
        constexpr int u = decltype(ic)::value;
        // the next head's Q fragments, into the registers phase A has finished with -- once half of the numerators are consumed
        if constexpr (u == NKT / 4) { if (nxt < nbh) q_frags(nxt); }
        const bf16x8 ph = pack_pair(s[2 * u], s[2 * u + 1]);
        f32x4 ra, rb;
#pragma unroll
        for (int r = 0; r < 4; ++r) { ra[r] = s[2 * u][r] - (float)ph[r]; rb[r] = s[2 * u + 1][r] - (float)ph[4 + r]; }
        const bf16x8 pl = pack_pair(ra, rb);
#pragma unroll
        for (int d2 = 0; d2 < 4; d2 += 2) {          // two 16-column slabs of the head dim at a time (registers)
          bf16x4 hl[2], hh[2], ll_[2], lh[2];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const unsigned vb = vimg + (((d2 + e) ^ vsw) << 5);
            AT_DS_TR_OFF(hl[e], vb, u * 4096); AT_DS_TR_OFF(hh[e], vb, u * 4096 + 2048);
            AT_DS_TR_OFF(ll_[e], vb, IMG + u * 4096); AT_DS_TR_OFF(lh[e], vb, IMG + u * 4096 + 2048);
          }
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(hl[0]), "+v"(hh[0]), "+v"(ll_[0]), "+v"(lh[0]), "+v"(hl[1]), "+v"(hh[1]), "+v"(ll_[1]), "+v"(lh[1]));
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const bf16x8 vh = __builtin_shufflevector(hl[e], hh[e], 0, 1, 2, 3, 4, 5, 6, 7);
            const bf16x8 vl = __builtin_shufflevector(ll_[e], lh[e], 0, 1, 2, 3, 4, 5, 6, 7);
            o[d2 + e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vl, ph, o[d2 + e], 0, 0, 0);
            o[d2 + e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, pl, o[d2 + e], 0, 0, 0);
            o[d2 + e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, ph, o[d2 + e], 0, 0, 0);   // O^T[d][q]
          }
        }
      });
      int lp_ = lane; asm volatile("" : "+v"(lp_));
      const int gq = lp_ >> 4, q = qt * 16 + (lp_ & 15);
      if (q < S) {
        const float inv = 1.f / l;
        const int64_t hb = (int64_t)(bh / H) * S * (H * AT_DH) + (bh % H) * AT_DH;          // wave-uniform
        const unsigned off = (unsigned)(q * (H * AT_DH) + 4 * gq);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          bf16x4 vh, vl;
#pragma unroll
          for (int r = 0; r < 4; ++r) { const float v = o[dt][r] * inv; vh[r] = (bf16_t)v; vl[r] = (bf16_t)(v - (float)vh[r]); }
          *reinterpret_cast<bf16x4*>(out_hi + hb + off + dt * 16) = vh;
          *reinterpret_cast<bf16x4*>(out_lo + hb + off + dt * 16) = vl;
        }
        if (gq == 0) lse[(int64_t)bh * S + q] = m * c1 * LN2 + __logf(l);
      }
    }
    if (nxt >= nbh) break;
    bh = nxt;
  }
}

// ------------------------------------------------------------------------------------------------------
// backward, dQ: a wave owns 16 queries
// ------------------------------------------------------------------------------------------------------
template <int NKT, bool DROP, int NW>
__global__ void __launch_bounds__(64 * NW, NW / 2)
mha_bwd_dq_mfma_k(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ key_mask, const bf16_t* __restrict__ out,
                  const bf16_t* __restrict__ dout, const float* __restrict__ lse, bf16_t* __restrict__ dqkv,
                  int H, int Smax, float scale, float drop_p, uint64_t drop_seed, const int32_t* __restrict__ cu) {
  const float drop_sc = DROP ? 1.f / (1.f - drop_p) : 1.f;
  extern __shared__ __attribute__((aligned(16))) char sm[];
  constexpr int Spad = NKT * 16;
  char* Kimg = sm; char* Vimg = sm + Spad * 128;
  float* kb = reinterpret_cast<float*>(sm + 2 * Spad * 128);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  AT_SEQ(b, Smax, cu)
  const int64_t ld = 3LL * H * AT_DH, ldo = (int64_t)H * AT_DH;
  const bf16_t* Q = qkv + (int64_t)row0 * ld + h * AT_DH;
  const bf16_t* Kp = Q + H * AT_DH;
  const bf16_t* Vp = Kp + H * AT_DH;
  const bf16_t* O = out + (int64_t)row0 * ldo + h * AT_DH;
  const bf16_t* dO = dout + (int64_t)row0 * ldo + h * AT_DH;
  stage_rows(Kimg, IMG_TR, Kp, ld, S, Spad);      // row reads for S^T (2-way), transposed reads for dQ^T
  stage_rows(Vimg, IMG_ROW, Vp, ld, S, Spad);     // row reads for dP^T
  stage_key_bias(kb, key_mask ? key_mask + row0 : nullptr, S, Spad);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const float c1 = scale * LOG2E;
  const int nqt = (S + 15) / 16;
  for (int qt = wave; qt < nqt; qt += NW) {
    const int q0 = qt * 16;
    const int q = q0 + l16;
    const bf16x8 qf0 = frag_global(Q, ld, q0, S, 0, lane), qf1 = frag_global(Q, ld, q0, S, 1, lane);
    const bf16x8 df0 = frag_global(dO, ldo, q0, S, 0, lane), df1 = frag_global(dO, ldo, q0, S, 1, lane);
    const bf16x8 of0 = frag_global(O, ldo, q0, S, 0, lane), of1 = frag_global(O, ldo, q0, S, 1, lane);
    float dsum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) dsum += (float)df0[j] * (float)of0[j] + (float)df1[j] * (float)of1[j];
    dsum = colgroup_sum(dsum);                       // D_q = rowsum(dO * O)
    const float L2 = lse[((int64_t)b * H + h) * Smax + (q < S ? q : S - 1)] * LOG2E;      // +inf for a fully masked query
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int u = 0; u < NKT / 2; ++u) {      // rolled: keeps the live set small enough for 2 blocks per CU
      f32x4 ds2[2];
      bf16x8 kfr[2][2], vfr[2][2];
      f32x4 bias[2], sc[2], dpv[2];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int kt = 2 * u + hh;
        kfr[hh][0] = frag_rows(Kimg, IMG_TR, kt * 16, 0, lane); kfr[hh][1] = frag_rows(Kimg, IMG_TR, kt * 16, 1, lane);
        vfr[hh][0] = frag_rows(Vimg, IMG_ROW, kt * 16, 0, lane); vfr[hh][1] = frag_rows(Vimg, IMG_ROW, kt * 16, 1, lane);
        bias[hh] = *reinterpret_cast<const f32x4*>(kb + kt * 16 + 4 * g);
      }
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        sc[hh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr[hh][0], qf0, zero4, 0, 0, 0);
        dpv[hh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfr[hh][0], df0, zero4, 0, 0, 0);
      }
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        sc[hh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr[hh][1], qf1, sc[hh], 0, 0, 0);
        dpv[hh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfr[hh][1], df1, dpv[hh], 0, 0, 0);
      }
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int kt = 2 * u + hh;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(fmaf(sc[hh][r], c1, bias[hh][r]) - L2);          // 0 for masked keys / queries
          const float keep = DROP ? attn_keep(drop_p, drop_sc, drop_seed, blockIdx.x, Smax, q, kt * 16 + 4 * g + r) : 1.f;
          ds2[hh][r] = p * (DROP ? dpv[hh][r] * keep - dsum : dpv[hh][r] - dsum);                 // (the score scale is applied to dQ below)
        }
      }
      const bf16x8 dsf = pack_pair(ds2[0], ds2[1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols_tr(Kimg, u, dt, lane), dsf, dq[dt], 0, 0, 0);   // dQ^T[d][q]
    }
    bf16_t* drow = dqkv + ((int64_t)row0 + (q < S ? q : S - 1)) * ld + h * AT_DH;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (bf16_t)(dq[dt][r] * scale);
      if (q < S) *reinterpret_cast<bf16x4*>(drow + dt * 16 + 4 * g) = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// backward, dK/dV: a wave owns 16 keys
// ------------------------------------------------------------------------------------------------------
template <int NKT, bool DROP, int NW>
__global__ void __launch_bounds__(64 * NW, NW / 2)
mha_bwd_dkv_mfma_k(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ key_mask, const bf16_t* __restrict__ out,
                   const bf16_t* __restrict__ dout, const float* __restrict__ lse, bf16_t* __restrict__ dqkv,
                   int H, int Smax, float scale, float drop_p, uint64_t drop_seed, const int32_t* __restrict__ cu) {
  const float drop_sc = DROP ? 1.f / (1.f - drop_p) : 1.f;
  extern __shared__ __attribute__((aligned(16))) char sm[];
  constexpr int Spad = NKT * 16;
  char* Qimg = sm; char* Dimg = sm + Spad * 128;
  float* lse_s = reinterpret_cast<float*>(sm + 2 * Spad * 128);     // log-sum-exp in the exp2 domain
  float* dsum_s = lse_s + Spad;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  AT_SEQ(b, Smax, cu)
  const int64_t ld = 3LL * H * AT_DH, ldo = (int64_t)H * AT_DH;
  const bf16_t* Q = qkv + (int64_t)row0 * ld + h * AT_DH;
  const bf16_t* Kp = Q + H * AT_DH;
  const bf16_t* Vp = Kp + H * AT_DH;
  const bf16_t* O = out + (int64_t)row0 * ldo + h * AT_DH;
  const bf16_t* dO = dout + (int64_t)row0 * ldo + h * AT_DH;
  stage_rows(Qimg, IMG_TR, Q, ld, S, Spad);
  stage_rows(Dimg, IMG_TR, dO, ldo, S, Spad);
  for (int q = threadIdx.x; q < Spad; q += blockDim.x) {
    float a = 0.f, L = INFINITY;                 // padded query rows: lse=+inf -> P = 0
    if (q < S) {
      L = lse[((int64_t)b * H + h) * Smax + q] * LOG2E;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const bf16x8 x = *reinterpret_cast<const bf16x8*>(dO + (int64_t)q * ldo + c * 8);
        const bf16x8 y = *reinterpret_cast<const bf16x8*>(O + (int64_t)q * ldo + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) a += (float)x[j] * (float)y[j];
      }
    }
    lse_s[q] = L; dsum_s[q] = a;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const float c1 = scale * LOG2E;
  const int nkt = (S + 15) / 16;
  for (int kt = wave; kt < nkt; kt += NW) {
    const int k0 = kt * 16;
    const int key = k0 + l16;
    const float kbias = (key < S && (!key_mask || key_mask[row0 + key] != 0)) ? 0.f : -INFINITY;    // this lane's key
    const bf16x8 kf0 = frag_global(Kp, ld, k0, S, 0, lane), kf1 = frag_global(Kp, ld, k0, S, 1, lane);
    const bf16x8 vf0 = frag_global(Vp, ld, k0, S, 0, lane), vf1 = frag_global(Vp, ld, k0, S, 1, lane);
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll 1
    for (int u = 0; u < NKT / 2; ++u) {
      f32x4 p2[2], ds2[2];
      // all eight LDS fragments of the two query tiles first, then four independent MFMA chains (a dependent pair issued
      // back to back stalls on the first result), then the elementwise part
      bf16x8 qf[2][2], df[2][2];
      f32x4 Lq[2], Dq[2], sc[2], dpv[2];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int qt = 2 * u + hh;
        qf[hh][0] = frag_rows(Qimg, IMG_TR, qt * 16, 0, lane); qf[hh][1] = frag_rows(Qimg, IMG_TR, qt * 16, 1, lane);
        df[hh][0] = frag_rows(Dimg, IMG_TR, qt * 16, 0, lane); df[hh][1] = frag_rows(Dimg, IMG_TR, qt * 16, 1, lane);
        Lq[hh] = *reinterpret_cast<const f32x4*>(lse_s + qt * 16 + 4 * g);       // queries 16qt + 4g + r
        Dq[hh] = *reinterpret_cast<const f32x4*>(dsum_s + qt * 16 + 4 * g);
      }
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        sc[hh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[hh][0], kf0, zero4, 0, 0, 0);      // S[q][key]
        dpv[hh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[hh][0], vf0, zero4, 0, 0, 0);     // dP[q][key]
      }
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        sc[hh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[hh][1], kf1, sc[hh], 0, 0, 0);
        dpv[hh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[hh][1], vf1, dpv[hh], 0, 0, 0);
      }
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int qt = 2 * u + hh;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(fmaf(sc[hh][r], c1, kbias) - Lq[hh][r]);
          if (DROP) {
            const float keep = attn_keep(drop_p, drop_sc, drop_seed, blockIdx.x, Smax, qt * 16 + 4 * g + r, key);
            p2[hh][r] = p * keep;
            ds2[hh][r] = p * (dpv[hh][r] * keep - Dq[hh][r]);
          } else {
            p2[hh][r] = p;
            ds2[hh][r] = p * (dpv[hh][r] - Dq[hh][r]);                                     // (score scale applied to dK below)
          }
        }
      }
      const bf16x8 pf = pack_pair(p2[0], p2[1]), dsf = pack_pair(ds2[0], ds2[1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols_tr(Dimg, u, dt, lane), pf, dv[dt], 0, 0, 0);    // dV^T[d][key]
        dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols_tr(Qimg, u, dt, lane), dsf, dk[dt], 0, 0, 0);   // dK^T[d][key]
      }
    }
    bf16_t* krow = dqkv + ((int64_t)row0 + (key < S ? key : S - 1)) * ld + (int64_t)H * AT_DH + h * AT_DH;
    bf16_t* vrow = krow + (int64_t)H * AT_DH;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16x4 a, c;
#pragma unroll
      for (int r = 0; r < 4; ++r) { a[r] = (bf16_t)(dk[dt][r] * scale); c[r] = (bf16_t)dv[dt][r]; }
      if (key < S) {
        *reinterpret_cast<bf16x4*>(krow + dt * 16 + 4 * g) = a;
        *reinterpret_cast<bf16x4*>(vrow + dt * 16 + 4 * g) = c;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// backward for the ViT as ONE launch (unmasked, no dropout, padded layout)
// ------------------------------------------------------------------------------------------------------
// A two-kernel form (a dQ and a dK/dV launch) reads q|k|v, O and dO twice (~1.0 GB per ViT-B layer at B = 256) where the algorithm
// needs them once (0.62 GB incl. the dqkv store), and in-kernel stamps (tools/attn_stamps.py) show where a workgroup's time goes:
// not in the MFMA loops (6-8 k cycles per part with every operand in LDS) but in waiting -- for the staging DMA and for the per-tile
// operand fragments that come straight from HBM.  One workgroup per (b, h) runs BOTH parts, so every operand crosses HBM once.  S
// and dP are still formed in both orientations (28 MFMA passes instead of the 20 of a single-orientation kernel): the matrix pipe
// idles ~75 % of these kernels' time, the bytes and the exposed latencies are what count.  No atomics, no cross-wave reduction,
// same summation order per output element.
// Same work split as mha_bwd_dq_mfma_k / mha_bwd_dkv_mfma_k (a wave owns 16 queries / keys and sweeps the opposite tiles in pairs),
// but the inner loops are laid out by hand: hipcc's schedule of the C++ version waits on every LDS read right in front of the MFMA
// that consumes it (19 s_waitcnt per query pair at 108 VGPRs).  Here a pair issues its 8 row fragments and its row constants in one
// batch, and the transposed fragments of the second products right after the S / dP MFMAs, so that they land under the
// exponentials; the tile / pair index is an immediate offset of the asm ds_read (no address arithmetic in the loop).
// Row constants as the initial accumulator (the guide's attention-backward recipe): the prologue stores -lse/c1 and
// -rowsum(dO*O) per query, the S and dP MFMA chains start from them, and p = exp2(c1 * S'), dS = p * dP' need no subtraction.
// Two 8-wave workgroups per CU, so one's staging runs under the other's MFMAs.  The image pairs TIME-SHARE one 56-KiB region:
// K | V are staged first, together with the per-query constants (from whole dO / O rows), for the dQ part, whose Q / dO fragments
// come from global memory; after a barrier Q | dO are staged over them for the dK / dV part, whose key / value fragments hit this
// XCD's L2 (staged moments ago).  (A 16-wave form with all four images resident and no global fragment loads was measured slower
// in round 3: nothing overlapped its staging.)
template <int NKT, int NW>
__global__ void __launch_bounds__(64 * NW, NW / 2)
mha_bwd_fused_mfma_v_k(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                       const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int H, int S, float scale,
                       unsigned long long* __restrict__ stamps) {
  // stamps (tools/attn_stamps.py only, nullptr otherwise): s_memtime of wave 0 at kernel entry, after the first staging barrier,
  // between the two parts and at exit, [block][4]; written to a buffer nothing else reads
  unsigned long long t_in = 0, t_staged = 0, t_mid = 0;
  if (stamps) t_in = __builtin_amdgcn_s_memtime();
  extern __shared__ __attribute__((aligned(16))) char sm[];
  constexpr int Spad = NKT * 16, IMG = Spad * 128;
  constexpr int KB = 0, VB = IMG, QB = 0, DB = IMG, ST = 2 * IMG;      // Q | dO over K | V
  float* lse_s = reinterpret_cast<float*>(sm + ST);          // -lse / c1 in the exp2 domain (c1 * (S + this) = c1 S - L)
  float* dsum_s = lse_s + Spad;                              // -rowsum(dO * O)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int row0 = b * S;
  const int64_t ld = 3LL * H * AT_DH, ldo = (int64_t)H * AT_DH;
  const bf16_t* Q = qkv + (int64_t)row0 * ld + h * AT_DH;
  const bf16_t* Kp = Q + H * AT_DH;
  const bf16_t* Vp = Kp + H * AT_DH;
  const bf16_t* O = out + (int64_t)row0 * ldo + h * AT_DH;
  const bf16_t* dO = dout + (int64_t)row0 * ldo + h * AT_DH;
  const float c1 = scale * LOG2E, inv_c1 = 1.f / c1;
  const unsigned lds0 = (unsigned)(uintptr_t)(at_lds_void*)sm;
  const unsigned rsw = (l16 >> 1) & 3, ksw = (l16 >> 1) & 7;
  const unsigned roff0 = l16 * 128 + ((((unsigned)(g >> 1)) ^ rsw) << 5) + ((g & 1) << 4);           // TR image rows, k-step 0: chunk c = g
  const unsigned roff1 = l16 * 128 + ((((unsigned)(2 + (g >> 1))) ^ rsw) << 5) + ((g & 1) << 4);     // k-step 1: chunk c = 4 + g
  const int qq = l16 >> 2, pp = l16 & 3, vsw = (2 * g + (qq >> 1)) & 3;
  const int nt = (S + 15) / 16;

  auto stage_key_side = [&]() {
    stage_rows(sm + KB, IMG_TR, Kp, ld, S, Spad);      // row reads for S^T (2-way), transposed reads for dQ^T
    stage_rows(sm + VB, IMG_ROW, Vp, ld, S, Spad);     // row reads for dP^T
  };
  auto stage_query_images = [&]() {
    stage_rows(sm + QB, IMG_TR, Q, ld, S, Spad);
    stage_rows(sm + DB, IMG_TR, dO, ldo, S, Spad);
  };
  auto stage_row_constants = [&]() {
    // rowsum(dO * O): eight lanes per query row, one 16-byte chunk of each operand per lane (whole 128-byte rows per 8 lanes, two
    // loads per lane instead of a chain of sixteen), then a three-step butterfly
    for (int e = threadIdx.x; e < Spad * 8; e += blockDim.x) {
      const int q = e >> 3, c = e & 7;
      float a = 0.f;
      if (q < S) {
        const bf16x8 x = *reinterpret_cast<const bf16x8*>(dO + (int64_t)q * ldo + c * 8);
        const bf16x8 y = *reinterpret_cast<const bf16x8*>(O + (int64_t)q * ldo + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) a += (float)x[j] * (float)y[j];
      }
      a += __shfl_xor(a, 1, 64); a += __shfl_xor(a, 2, 64); a += __shfl_xor(a, 4, 64);
      if (c == 0) {
        const float L = q < S ? lse[((int64_t)b * H + h) * S + q] * LOG2E : INFINITY;      // padded query rows: lse=+inf -> P = 0
        lse_s[q] = -L * inv_c1; dsum_s[q] = -a;
      }
    }
  };

  // The per-tile operand fragments that come straight from global memory are PREFETCHED -- a wave's first query tile
  // (Q | dO rows) at kernel entry, under the staging DMA; its first key tile (K | V rows) before the second staging -- so that their latency (in-kernel stamps: ~25 k of a workgroup's ~57 k
  // cycles were spent waiting for exactly these loads) is not exposed for the first tiles (8 of the 13 per part).
  bf16x8 pq0, pq1, pd0, pd1, pk0, pk1, pv0, pv1;
  auto fetch_q = [&](int qt) {
    pq0 = frag_global(Q, ld, qt * 16, S, 0, lane); pq1 = frag_global(Q, ld, qt * 16, S, 1, lane);
    pd0 = frag_global(dO, ldo, qt * 16, S, 0, lane); pd1 = frag_global(dO, ldo, qt * 16, S, 1, lane);
  };
  auto fetch_k = [&](int kt) {
    pk0 = frag_global(Kp, ld, kt * 16, S, 0, lane); pk1 = frag_global(Kp, ld, kt * 16, S, 1, lane);
    pv0 = frag_global(Vp, ld, kt * 16, S, 0, lane); pv1 = frag_global(Vp, ld, kt * 16, S, 1, lane);
  };

  // ---- dQ: a wave's query tile(s) against every key pair (K | V images, row constants in LDS)
  auto dq_part = [&]() {
    const unsigned kb0 = lds0 + KB + roff0, kb1 = lds0 + KB + roff1;
    const unsigned vb0 = lds0 + VB + l16 * 128 + (((unsigned)g ^ ksw) << 4), vb1 = lds0 + VB + l16 * 128 + (((unsigned)(4 + g) ^ ksw) << 4);
    unsigned tk[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) tk[dt] = lds0 + KB + (4 * g + qq) * 128 + ((dt ^ vsw) << 5) + 8 * pp;
    auto dq_tile = [&](int qt, bf16x8 qf0, bf16x8 qf1, bf16x8 df0, bf16x8 df1) {
      const int q0 = qt * 16;
      const int q = q0 + l16;
      const float nl = lse_s[q], nd = dsum_s[q];      // row constants as the initial accumulators: S' = S - L/c1, dP' = dP - D
      f32x4 dq[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      static_for<0, NKT / 2>([&](auto ic) {
        constexpr int u = decltype(ic)::value;
        bf16x8 ka0, ka1, kc0, kc1, va0, va1, vc0, vc1;         // key tiles 2u (a) and 2u+1 (c), k-steps 0 / 1
        AT_DS_B128_OFF(ka0, kb0, (2 * u) * 2048);     AT_DS_B128_OFF(va0, vb0, (2 * u) * 2048);
        AT_DS_B128_OFF(kc0, kb0, (2 * u + 1) * 2048); AT_DS_B128_OFF(vc0, vb0, (2 * u + 1) * 2048);
        AT_DS_B128_OFF(ka1, kb1, (2 * u) * 2048);     AT_DS_B128_OFF(va1, vb1, (2 * u) * 2048);
        AT_DS_B128_OFF(kc1, kb1, (2 * u + 1) * 2048); AT_DS_B128_OFF(vc1, vb1, (2 * u + 1) * 2048);
        f32x4 sa = {nl, nl, nl, nl}, sc_ = {nl, nl, nl, nl}, pa = {nd, nd, nd, nd}, pc = {nd, nd, nd, nd};
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(ka0), "+v"(va0), "+v"(kc0), "+v"(vc0));
        sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka0, qf0, sa, 0, 0, 0);       // S'^T[key][q]
        pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va0, df0, pa, 0, 0, 0);       // dP'^T[key][q]
        sc_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc0, qf0, sc_, 0, 0, 0);
        pc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vc0, df0, pc, 0, 0, 0);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ka1), "+v"(va1), "+v"(kc1), "+v"(vc1));
        sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka1, qf1, sa, 0, 0, 0);
        pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va1, df1, pa, 0, 0, 0);
        sc_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc1, qf1, sc_, 0, 0, 0);
        pc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vc1, df1, pc, 0, 0, 0);
        bf16x4 klo[4], khi[4];                       // K^T fragments of the dQ product: in flight under the exponentials
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { AT_DS_TR_OFF(klo[dt], tk[dt], u * 4096); AT_DS_TR_OFF(khi[dt], tk[dt], u * 4096 + 2048); }
        f32x4 dsa, dsc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float xa = sa[r] * c1, xc = sc_[r] * c1;
          if (u == NKT / 2 - 1) {                    // only the last key pair holds keys beyond S (S > 16 (NKT - 2))
            xa = (2 * u) * 16 + 4 * g + r < S ? xa : -INFINITY;
            xc = (2 * u + 1) * 16 + 4 * g + r < S ? xc : -INFINITY;
          }
          dsa[r] = __builtin_amdgcn_exp2f(xa) * pa[r];        // p (dP - D); a padded query has lse = +inf -> p = 0
          dsc[r] = __builtin_amdgcn_exp2f(xc) * pc[r];        // (the score scale is applied to dQ below)
        }
        const bf16x8 dsf = pack_pair(dsa, dsc);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(klo[0]), "+v"(khi[0]), "+v"(klo[1]), "+v"(khi[1]), "+v"(klo[2]), "+v"(khi[2]), "+v"(klo[3]), "+v"(khi[3]));
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_shufflevector(klo[dt], khi[dt], 0, 1, 2, 3, 4, 5, 6, 7), dsf, dq[dt], 0, 0, 0);   // dQ^T[d][q]
      });
      bf16_t* drow = dqkv + ((int64_t)row0 + (q < S ? q : S - 1)) * ld + h * AT_DH;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (bf16_t)(dq[dt][r] * scale);
        if (q < S) *reinterpret_cast<bf16x4*>(drow + dt * 16 + 4 * g) = v;
      }
    };
    // the Q | dO images are not staged yet: fragments from global memory -- the first tile's were prefetched at kernel entry; a
    // second tile's are loaded here (prefetching them too costs 16 live registers inside the loop: spills)
    if (wave < nt) dq_tile(wave, pq0, pq1, pd0, pd1);
    for (int qt = wave + NW; qt < nt; qt += NW)
      dq_tile(qt, frag_global(Q, ld, qt * 16, S, 0, lane), frag_global(Q, ld, qt * 16, S, 1, lane), frag_global(dO, ldo, qt * 16, S, 0, lane),
              frag_global(dO, ldo, qt * 16, S, 1, lane));
  };

  // ---- dK / dV: a wave's key tile(s) against every query pair (Q | dO images, row constants in LDS)
  auto dkv_part = [&]() {
    unsigned tq[4], td[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const unsigned o = (4 * g + qq) * 128 + ((dt ^ vsw) << 5) + 8 * pp;
      tq[dt] = lds0 + QB + o; td[dt] = lds0 + DB + o;
    }
    const unsigned qb0 = lds0 + QB + roff0, qb1 = lds0 + QB + roff1, db0 = lds0 + DB + roff0, db1 = lds0 + DB + roff1;
    const unsigned lb = lds0 + ST + 16 * g, sb = lb + Spad * 4;      // row constants of queries 16 qt + 4 g + r
    auto dkv_tile = [&](int kt, bf16x8 kf0, bf16x8 kf1, bf16x8 vf0, bf16x8 vf1) {
      const int k0 = kt * 16;
      const int key = k0 + l16;
      const float kbias = key < S ? 0.f : -INFINITY;                        // this lane's key
      f32x4 dk[4], dv[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) { dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
      static_for<0, NKT / 2>([&](auto ic) {
        constexpr int u = decltype(ic)::value;
        bf16x8 qa0, qa1, qb0_, qb1_, da0, da1, db0_, db1_;      // row fragments of query tiles 2u (a) and 2u+1 (b), k-steps 0 / 1
        f32x4 sa, sb_, pa, pb;                                  // S' and dP' accumulators, started from the row constants
        AT_DS_B128_OFF(qa0, qb0, (2 * u) * 2048);     AT_DS_B128_OFF(da0, db0, (2 * u) * 2048);
        AT_DS_B128_OFF(qb0_, qb0, (2 * u + 1) * 2048); AT_DS_B128_OFF(db0_, db0, (2 * u + 1) * 2048);
        AT_DS_B128_OFF(sa, lb, (2 * u) * 64);          AT_DS_B128_OFF(pa, sb, (2 * u) * 64);
        AT_DS_B128_OFF(sb_, lb, (2 * u + 1) * 64);     AT_DS_B128_OFF(pb, sb, (2 * u + 1) * 64);
        AT_DS_B128_OFF(qa1, qb1, (2 * u) * 2048);     AT_DS_B128_OFF(da1, db1, (2 * u) * 2048);
        AT_DS_B128_OFF(qb1_, qb1, (2 * u + 1) * 2048); AT_DS_B128_OFF(db1_, db1, (2 * u + 1) * 2048);
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(qa0), "+v"(da0), "+v"(qb0_), "+v"(db0_), "+v"(sa), "+v"(pa), "+v"(sb_), "+v"(pb));
        sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa0, kf0, sa, 0, 0, 0);       // S'[q][key]
        pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da0, vf0, pa, 0, 0, 0);       // dP'[q][key]
        sb_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qb0_, kf0, sb_, 0, 0, 0);
        pb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(db0_, vf0, pb, 0, 0, 0);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(qa1), "+v"(da1), "+v"(qb1_), "+v"(db1_));
        sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa1, kf1, sa, 0, 0, 0);
        pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da1, vf1, pa, 0, 0, 0);
        sb_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qb1_, kf1, sb_, 0, 0, 0);
        pb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(db1_, vf1, pb, 0, 0, 0);
        bf16x4 dlo[4], dhi[4], qlo[4], qhi[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          AT_DS_TR_OFF(dlo[dt], td[dt], u * 4096); AT_DS_TR_OFF(dhi[dt], td[dt], u * 4096 + 2048);
          AT_DS_TR_OFF(qlo[dt], tq[dt], u * 4096); AT_DS_TR_OFF(qhi[dt], tq[dt], u * 4096 + 2048);
        }
        f32x4 p2a, p2b, dsa, dsb;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p2a[r] = __builtin_amdgcn_exp2f(fmaf(sa[r], c1, kbias));            // 0 for dead keys and padded queries
          p2b[r] = __builtin_amdgcn_exp2f(fmaf(sb_[r], c1, kbias));
          dsa[r] = p2a[r] * pa[r];                                            // (the score scale is applied to dK below)
          dsb[r] = p2b[r] * pb[r];
        }
        const bf16x8 pf = pack_pair(p2a, p2b), dsf = pack_pair(dsa, dsb);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(dlo[0]), "+v"(dhi[0]), "+v"(dlo[1]), "+v"(dhi[1]), "+v"(dlo[2]), "+v"(dhi[2]), "+v"(dlo[3]), "+v"(dhi[3]),
                     "+v"(qlo[0]), "+v"(qhi[0]), "+v"(qlo[1]), "+v"(qhi[1]), "+v"(qlo[2]), "+v"(qhi[2]), "+v"(qlo[3]), "+v"(qhi[3]));
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_shufflevector(dlo[dt], dhi[dt], 0, 1, 2, 3, 4, 5, 6, 7), pf, dv[dt], 0, 0, 0);    // dV^T[d][key]
          dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_shufflevector(qlo[dt], qhi[dt], 0, 1, 2, 3, 4, 5, 6, 7), dsf, dk[dt], 0, 0, 0);   // dK^T[d][key]
        }
      });
      bf16_t* krow = dqkv + ((int64_t)row0 + (key < S ? key : S - 1)) * ld + (int64_t)H * AT_DH + h * AT_DH;
      bf16_t* vrow = krow + (int64_t)H * AT_DH;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 a, c;
#pragma unroll
        for (int r = 0; r < 4; ++r) { a[r] = (bf16_t)(dk[dt][r] * scale); c[r] = (bf16_t)dv[dt][r]; }
        if (key < S) {
          *reinterpret_cast<bf16x4*>(krow + dt * 16 + 4 * g) = a;
          *reinterpret_cast<bf16x4*>(vrow + dt * 16 + 4 * g) = c;
        }
      }
    };
    if (wave < nt) dkv_tile(wave, pk0, pk1, pv0, pv1);
    for (int kt = wave + NW; kt < nt; kt += NW)
      dkv_tile(kt, frag_global(Kp, ld, kt * 16, S, 0, lane), frag_global(Kp, ld, kt * 16, S, 1, lane), frag_global(Vp, ld, kt * 16, S, 0, lane),
               frag_global(Vp, ld, kt * 16, S, 1, lane));
  };

  if (wave < nt) fetch_q(wave);         // lands under the staging below
  stage_key_side();
  stage_row_constants();                // reads whole dO / O rows: the dO fragments of the dQ part then hit L2
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (stamps) t_staged = __builtin_amdgcn_s_memtime();
  dq_part();
  if (wave < nt) fetch_k(wave);         // lands under the second staging
  __syncthreads();                      // every wave is done with the K | V images (the row constants stay)
  stage_query_images();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (stamps) t_mid = __builtin_amdgcn_s_memtime();
  dkv_part();
  if (stamps && threadIdx.x == 0) {
    const unsigned long long t_out = __builtin_amdgcn_s_memtime();
    stamps[4 * blockIdx.x + 0] = t_in; stamps[4 * blockIdx.x + 1] = t_staged; stamps[4 * blockIdx.x + 2] = t_mid; stamps[4 * blockIdx.x + 3] = t_out;
  }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
bool mmrca_mha_mfma_ok(int S, int dh, int dtype) { return dtype == MMRCA_BF16 && dh == AT_DH && S >= 1 && S <= AT_MAX_S; }

// CU count of the current device at the first call (the persistent kernels' grid bound), 256 if the query fails
static int attn_cu_count() {
  static const int ncu = [] {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n >= 1 ? n : 256;
  }();
  return ncu;
}

static int pick_nkt(int S) {
  const int need = (S + 31) / 32 * 2;            // key tiles, even
  const int opts[] = {2, 4, 8, 14, 16, 32};
  for (int o : opts) if (o >= need) return o;
  return 32;
}

#define K_FWD(N_, D_, W_) mha_fwd_mfma_k<N_, D_, W_>
#define K_DQ(N_, D_, W_) mha_bwd_dq_mfma_k<N_, D_, W_>
#define K_DKV(N_, D_, W_) mha_bwd_dkv_mfma_k<N_, D_, W_>
#define AT_LAUNCH1(KERNEL, NKT, DROP, NW, LDSBYTES, ...)                                                                        \
  do {                                                                                                                         \
    MMRCA_MAX_LDS((int)(LDSBYTES), KERNEL(NKT, DROP, NW)); \
    hipLaunchKernelGGL((KERNEL(NKT, DROP, NW)), dim3(B * H), dim3(64 * NW), LDSBYTES, st, __VA_ARGS__);                         \
  } while (0)
// small S: 4 waves.  S > 128: 8 waves when the kernel fits 128 VGPRs without spilling (W8_PLAIN / W8_DROP, per kernel)
#define AT_LAUNCH4(KERNEL, NKT, LDSBYTES, ...)                                          \
  do {                                                                                  \
    if (drop_p > 0.f) AT_LAUNCH1(KERNEL, NKT, true, 4, LDSBYTES, __VA_ARGS__);          \
    else AT_LAUNCH1(KERNEL, NKT, false, 4, LDSBYTES, __VA_ARGS__);                      \
  } while (0)
#define AT_LAUNCH8(KERNEL, NKT, W8_PLAIN, W8_DROP, LDSBYTES, ...)                       \
  do {                                                                                  \
    if (drop_p > 0.f) {                                                                 \
      if (W8_DROP) AT_LAUNCH1(KERNEL, NKT, true, 8, LDSBYTES, __VA_ARGS__);             \
      else AT_LAUNCH1(KERNEL, NKT, true, 4, LDSBYTES, __VA_ARGS__);                     \
    } else {                                                                            \
      if (W8_PLAIN) AT_LAUNCH1(KERNEL, NKT, false, 8, LDSBYTES, __VA_ARGS__);           \
      else AT_LAUNCH1(KERNEL, NKT, false, 4, LDSBYTES, __VA_ARGS__);                    \
    }                                                                                   \
  } while (0)

#define AT_SWITCH(KERNEL, EXTRA, W8_PLAIN, W8_DROP, W8_32, ...)                                                   \
  switch (nkt) {                                                                                                   \
    case 2: AT_LAUNCH4(KERNEL, 2, 2 * 2 * 16 * 128 + EXTRA(2), __VA_ARGS__); break;                                \
    case 4: AT_LAUNCH4(KERNEL, 4, 2 * 4 * 16 * 128 + EXTRA(4), __VA_ARGS__); break;                                \
    case 8: AT_LAUNCH4(KERNEL, 8, 2 * 8 * 16 * 128 + EXTRA(8), __VA_ARGS__); break;                                \
    case 14: AT_LAUNCH8(KERNEL, 14, W8_PLAIN, W8_DROP, 2 * 14 * 16 * 128 + EXTRA(14), __VA_ARGS__); break;         \
    case 16: AT_LAUNCH8(KERNEL, 16, W8_PLAIN, W8_DROP, 2 * 16 * 16 * 128 + EXTRA(16), __VA_ARGS__); break;         \
    default: AT_LAUNCH8(KERNEL, 32, (W8_PLAIN && W8_32), (W8_DROP && W8_32), 2 * 32 * 16 * 128 + EXTRA(32), __VA_ARGS__); break; \
  }
// ------------------------------------------------------------------------------------------------------
// backward for the ViT, PERSISTENT over heads: every operand crosses the fabric ONCE
// ------------------------------------------------------------------------------------------------------
// The fused kernel above time-shares one 56-KiB region between the K | V and the Q | dO images, so each of Q, K, V, dO is read
// twice (once as an image, once as per-tile fragments) and most of the second reads miss L2 (64 resident workgroups x ~126 KB per
// XCD against 4 MiB): PMC, corrected for 16-byte lanes: 689 MB fetched per launch against 389 MB of operands.
// The kernel is then bandwidth-shaped (3.9 TB/s of fabric traffic over its 235 us), so the re-reads are its time.
// Here ONE 16-wave workgroup per CU walks heads bh = blockIdx.x, + gridDim.x, ... with SIX image slots of 13 tiles (208 rows,
// 26 KiB; the seventh key / query pair of the loops reads 16 rows past an image, i.e. the first rows of the next slot or the
// zeroed pad behind the last one: finite values that every consumer multiplies by an exact zero):
//     slots 0,1 / 2,3: K | V of the even / odd heads of this workgroup;  slots 4,5: Q | dO of the current head
//   top of an iteration (vmcnt(0) + barrier): K | V, Q | dO and the row constants of head i are in LDS
//   1. the DMA of head i+1's K | V is issued into the other K | V pair            (lands under the dK / dV part)
//   2. dK / dV part: a wave's key tile against every query pair (Q | dO images; its K / V fragments from the K | V images)
//   3. every wave takes the Q | dO fragments and row constants of its query tile into registers; barrier (LDS only)
//   4. the DMA of head i+1's Q | dO is issued over slots 4,5 and the three waves without a tile compute head i+1's row constants
//      (from whole dO / O rows)                                                   (both land under the dQ part)
//   5. dQ part: a wave's query tile (fragments in registers) against every key pair (K | V images)
// All LDS reads of the loop are inline asm and nothing spills, so no compiler-made vmcnt(0) waits for the DMA in flight.
// QT = tiles per wave: with one tile per wave (16 waves) the kernel is bound by LDS reads -- every wave streams the whole opposite
// side's images (20 KB of fragment reads per pair and wave: ~23 k cycles of LDS bandwidth per head against ~12 k of MFMA); with
// QT = 2 (8 waves, 256 registers each) every fragment read feeds two tiles and the LDS traffic halves.
#define BWDP_VGPRS 216          // registers the compiler may allocate; v216 .. v251 are the row constants' landing registers (rc_issue)
template <int NKT, int NW, int QT>
__global__ void __launch_bounds__(64 * NW, 1) __attribute__((amdgpu_num_vgpr(BWDP_VGPRS)))
mha_bwd_p_mfma_v_k(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                   const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int H, int S, float scale, int nbh) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  constexpr int SROWS = (NKT - 1) * 16, IMG = SROWS * 128, NCONST = NKT * 16, CONSTB = 2 * NCONST * 4;
  constexpr int TOTAL = CONSTB + 6 * IMG + 2048;
  float* lse_s = reinterpret_cast<float*>(sm);               // -lse / c1 in the exp2 domain
  float* dsum_s = lse_s + NCONST;                            // -rowsum(dO * O)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t ld = 3LL * H * AT_DH, ldo = (int64_t)H * AT_DH;
  const float c1 = scale * LOG2E, inv_c1 = 1.f / c1;
  const unsigned lds0 = (unsigned)(uintptr_t)(at_lds_void*)sm;
  constexpr int TW = NKT / QT;                               // waves that own tiles QT w .. QT w + QT - 1 (a tile past S is all padding)
  static_assert(NKT % QT == 0 && TW < NW, "at least one wave without tiles computes the row constants");
  const bool has_tile = wave < TW;
  int bh = blockIdx.x;
  if (bh >= nbh) return;
  // LDS is zeroed once: the rows an image's last pair over-reads must be finite from the first head on
  for (int i = threadIdx.x * 16; i < TOTAL; i += 64 * NW * 16) *reinterpret_cast<f32x4*>(sm + i) = (f32x4){0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  const unsigned QB = lds0 + CONSTB + 4 * IMG, DB = lds0 + CONSTB + 5 * IMG;
  // Per-lane image offsets are re-derived at the start of every phase from an OPAQUE copy of the lane id: computed once up here
  // they (and the staging loops' per-lane source offsets, which LICM hoists out of the head loop) stay live across the whole
  // loop and the kernel spills -- and a scratch reload counts in vmcnt, i.e. it waits for the next head's DMA.
#define BWDP_LANE_OFFSETS()                                                                                                         \
  int lane_o = lane;                                                                                                                \
  asm volatile("" : "+v"(lane_o));                                                                                                  \
  const int g = lane_o >> 4, l16 = lane_o & 15;                                                                                     \
  const unsigned rsw = (l16 >> 1) & 3, ksw = (l16 >> 1) & 7;                                                                        \
  [[maybe_unused]] const unsigned roff0 = l16 * 128 + ((((unsigned)(g >> 1)) ^ rsw) << 5) + ((g & 1) << 4);       /* TR image rows, k-step 0 */ \
  [[maybe_unused]] const unsigned roff1 = l16 * 128 + ((((unsigned)(2 + (g >> 1))) ^ rsw) << 5) + ((g & 1) << 4); /* k-step 1 */   \
  [[maybe_unused]] const unsigned voff0 = l16 * 128 + (((unsigned)g ^ ksw) << 4), voff1 = l16 * 128 + (((unsigned)(4 + g) ^ ksw) << 4); /* ROW image rows */ \
  const int qq = l16 >> 2, pp = l16 & 3, vsw = (2 * g + (qq >> 1)) & 3;                                                             \
  unsigned toff[4];                                          /* transposed reads of a TR image */                                   \
  _Pragma("unroll") for (int dt = 0; dt < 4; ++dt) toff[dt] = (4 * g + qq) * 128 + ((dt ^ vsw) << 5) + 8 * pp;

  // stage_rows with the lane id made opaque at every call (see BWDP_LANE_OFFSETS)
  auto stage_img = [&](int slot, int mode, const bf16_t* __restrict__ src, int64_t ld_) {
    int lane_s = lane;
    asm volatile("" : "+v"(lane_s));
    char* img = sm + CONSTB + slot * IMG;
    for (int j = wave; j < (SROWS >> 3); j += NW) {
      const int row = 8 * j + (lane_s >> 3), slot8 = lane_s & 7;
      const int c = mode == IMG_ROW ? (slot8 ^ ((row >> 1) & 7)) : ((((slot8 >> 1) ^ ((row >> 1) & 3)) << 1) | (slot8 & 1));
      const int r = row < S ? row : S - 1;
      __builtin_amdgcn_global_load_lds((at_gbl_void*)(src + (int64_t)r * ld_ + c * 8), (at_lds_void*)(img + j * 1024), 16, 0, 0);
    }
  };
  auto stage_kv = [&](int pair, int bh_) {
    const bf16_t* Kp = qkv + (int64_t)(bh_ / H) * S * ld + (int64_t)H * AT_DH + (bh_ % H) * AT_DH;
    stage_img(2 * pair, IMG_TR, Kp, ld);
    stage_img(2 * pair + 1, IMG_ROW, Kp + (int64_t)H * AT_DH, ld);
  };
  auto stage_qd = [&](int bh_) {
    stage_img(4, IMG_TR, qkv + (int64_t)(bh_ / H) * S * ld + (bh_ % H) * AT_DH, ld);
    stage_img(5, IMG_TR, dout + (int64_t)(bh_ / H) * S * ldo + (bh_ % H) * AT_DH, ldo);
  };
  // row constants of head bh_ by the threads [t0, t0 + nthr) of the workgroup: eight lanes per query row, one 16-byte chunk of dO
  // and O per lane, a three-step butterfly; rows >= S get lse = +inf (P = 0).  The loads are inline asm in batches of RCB rows
  // per lane with ONE wait per batch: a C++ global load in a kernel that also uses global_load_lds is followed by s_waitcnt
  // vmcnt(0) at once (the ISA showed it), i.e. twenty serialized round trips per head for the three waves that do this.
  constexpr int RCB = QT == 1 ? 5 : 13;                     // rows per lane and batch
  auto row_constants = [&](int bh_, int t0, int nthr) {
    const bf16_t* O = out + (int64_t)(bh_ / H) * S * ldo + (bh_ % H) * AT_DH;
    const bf16_t* dO = dout + (int64_t)(bh_ / H) * S * ldo + (bh_ % H) * AT_DH;
    const float* Lp = lse + (int64_t)bh_ * S;
    int tid_o = threadIdx.x;
    asm volatile("" : "+v"(tid_o));
    for (int base = tid_o - t0; base < NCONST * 8; base += RCB * nthr) {
      bf16x8 x[RCB], y[RCB];
      float Lr[RCB];
#pragma unroll
      for (int i = 0; i < RCB; ++i) {
        const int e = base + i * nthr;
        int q = e >> 3;
        q = q < S ? q : S - 1;                      // (rows past S: a valid address, the value is not used)
        const bf16_t* pd = dO + (int64_t)q * ldo + (e & 7) * 8;
        const bf16_t* po = O + (int64_t)q * ldo + (e & 7) * 8;
        const float* pl = Lp + q;
        asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(x[i]) : "v"(pd) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(y[i]) : "v"(po) : "memory");
        asm volatile("global_load_dword %0, %1, off" : "=&v"(Lr[i]) : "v"(pl) : "memory");
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 0; i < RCB; ++i) asm volatile("" : "+v"(x[i]), "+v"(y[i]), "+v"(Lr[i]));
#pragma unroll
      for (int i = 0; i < RCB; ++i) {
        const int e = base + i * nthr;
        const int q = e >> 3, c = e & 7;
        float a = 0.f;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) a += (float)x[i][jj] * (float)y[i][jj];
        a += __shfl_xor(a, 1, 64); a += __shfl_xor(a, 2, 64); a += __shfl_xor(a, 4, 64);
        if (c == 0 && e < NCONST * 8) {
          const float L = q < S ? Lr[i] * LOG2E : INFINITY;
          lse_s[q] = -L * inv_c1; dsum_s[q] = q < S ? -a : 0.f;
        }
      }
    }
  };

  // ---- dK / dV of key tiles QT wave + t (fragments from the K | V images at kvb), against every query pair
  auto dkv_tile = [&](int bh_, unsigned kvb) {
    BWDP_LANE_OFFSETS()
    bf16x8 kf0[QT], kf1[QT], vf0[QT], vf1[QT];
    float kbias[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const int k0 = (QT * wave + t) * 16;
      kbias[t] = k0 + l16 < S ? 0.f : -INFINITY;                          // this lane's key of tile t
      AT_DS_B128_OFF(kf0[t], kvb + roff0 + k0 * 128, 0);       AT_DS_B128_OFF(kf1[t], kvb + roff1 + k0 * 128, 0);
      AT_DS_B128_OFF(vf0[t], kvb + IMG + voff0 + k0 * 128, 0); AT_DS_B128_OFF(vf1[t], kvb + IMG + voff1 + k0 * 128, 0);
    }
    // (the dO image sits IMG bytes behind the Q image and dsum_s NCONST floats behind lse_s: immediate offsets, no second address)
    unsigned tq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) tq[dt] = QB + toff[dt];
    const unsigned qb0 = QB + roff0, qb1 = QB + roff1;
    const unsigned lb = lds0 + 16 * g;                            // row constants of queries 16 qt + 4 g + r
    f32x4 dk[QT][4], dv[QT][4];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) { dk[t][dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[t][dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int t = 0; t < QT; ++t) asm volatile("" : "+v"(kf0[t]), "+v"(kf1[t]), "+v"(vf0[t]), "+v"(vf1[t]));
    static_for<0, NKT / 2>([&](auto ic) {
      constexpr int u = decltype(ic)::value;
      bf16x8 qa0, qa1, qb0_, qb1_, da0, da1, db0_, db1_;      // row fragments of query tiles 2u (a) and 2u+1 (b), k-steps 0 / 1
      f32x4 ca, cb, ea, eb;                                   // the row constants S' and dP' start from (same for every key tile)
      AT_DS_B128_OFF(qa0, qb0, (2 * u) * 2048);     AT_DS_B128_OFF(da0, qb0, IMG + (2 * u) * 2048);
      AT_DS_B128_OFF(qb0_, qb0, (2 * u + 1) * 2048); AT_DS_B128_OFF(db0_, qb0, IMG + (2 * u + 1) * 2048);
      AT_DS_B128_OFF(ca, lb, (2 * u) * 64);          AT_DS_B128_OFF(ea, lb, NCONST * 4 + (2 * u) * 64);
      AT_DS_B128_OFF(cb, lb, (2 * u + 1) * 64);      AT_DS_B128_OFF(eb, lb, NCONST * 4 + (2 * u + 1) * 64);
      AT_DS_B128_OFF(qa1, qb1, (2 * u) * 2048);     AT_DS_B128_OFF(da1, qb1, IMG + (2 * u) * 2048);
      AT_DS_B128_OFF(qb1_, qb1, (2 * u + 1) * 2048); AT_DS_B128_OFF(db1_, qb1, IMG + (2 * u + 1) * 2048);
      bf16x4 dlo[4], dhi[4], qlo[4], qhi[4];                  // the transposed fragments of the second products: in flight under the first
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        AT_DS_TR_OFF(dlo[dt], tq[dt], IMG + u * 4096); AT_DS_TR_OFF(dhi[dt], tq[dt], IMG + u * 4096 + 2048);
        AT_DS_TR_OFF(qlo[dt], tq[dt], u * 4096); AT_DS_TR_OFF(qhi[dt], tq[dt], u * 4096 + 2048);
      }
      // 12 + 16 LDS reads were issued (the 4-bit counter stalls the issue past 15 in flight); they complete in order, so at most 15
      // outstanding means the twelve row / constant reads have landed
      asm volatile("s_waitcnt lgkmcnt(15)" : "+v"(qa0), "+v"(da0), "+v"(qb0_), "+v"(db0_), "+v"(ca), "+v"(ea), "+v"(cb), "+v"(eb), "+v"(qa1), "+v"(da1),
                   "+v"(qb1_), "+v"(db1_));
      bf16x8 pf[QT], dsf[QT];
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        f32x4 sa = ca, sb_ = cb, pa = ea, pb = eb;
        sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa0, kf0[t], sa, 0, 0, 0);       // S'[q][key]
        pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da0, vf0[t], pa, 0, 0, 0);       // dP'[q][key]
        sb_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qb0_, kf0[t], sb_, 0, 0, 0);
        pb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(db0_, vf0[t], pb, 0, 0, 0);
        sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa1, kf1[t], sa, 0, 0, 0);
        pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da1, vf1[t], pa, 0, 0, 0);
        sb_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qb1_, kf1[t], sb_, 0, 0, 0);
        pb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(db1_, vf1[t], pb, 0, 0, 0);
        f32x4 p2a, p2b, dsa, dsb;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p2a[r] = __builtin_amdgcn_exp2f(fmaf(sa[r], c1, kbias[t]));          // 0 for dead keys and padded queries
          p2b[r] = __builtin_amdgcn_exp2f(fmaf(sb_[r], c1, kbias[t]));
          dsa[r] = p2a[r] * pa[r];                                            // (the score scale is applied to dK below)
          dsb[r] = p2b[r] * pb[r];
        }
        pf[t] = pack_pair(p2a, p2b); dsf[t] = pack_pair(dsa, dsb);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(dlo[0]), "+v"(dhi[0]), "+v"(dlo[1]), "+v"(dhi[1]), "+v"(dlo[2]), "+v"(dhi[2]), "+v"(dlo[3]), "+v"(dhi[3]),
                   "+v"(qlo[0]), "+v"(qhi[0]), "+v"(qlo[1]), "+v"(qhi[1]), "+v"(qlo[2]), "+v"(qhi[2]), "+v"(qlo[3]), "+v"(qhi[3]));
#pragma unroll
      for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dv[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_shufflevector(dlo[dt], dhi[dt], 0, 1, 2, 3, 4, 5, 6, 7), pf[t], dv[t][dt], 0, 0, 0);    // dV^T[d][key]
          dk[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_shufflevector(qlo[dt], qhi[dt], 0, 1, 2, 3, 4, 5, 6, 7), dsf[t], dk[t][dt], 0, 0, 0);   // dK^T[d][key]
        }
    });
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const int key = (QT * wave + t) * 16 + l16;
      bf16_t* krow = dqkv + ((int64_t)(bh_ / H) * S + (key < S ? key : S - 1)) * ld + (int64_t)H * AT_DH + (bh_ % H) * AT_DH;
      bf16_t* vrow = krow + (int64_t)H * AT_DH;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 a, c;
#pragma unroll
        for (int r = 0; r < 4; ++r) { a[r] = (bf16_t)(dk[t][dt][r] * scale); c[r] = (bf16_t)dv[t][dt][r]; }
        if (key < S) {
          *reinterpret_cast<bf16x4*>(krow + dt * 16 + 4 * g) = a;
          *reinterpret_cast<bf16x4*>(vrow + dt * 16 + 4 * g) = c;
        }
      }
    }
  };

  // ---- dQ of query tiles QT wave + t (their Q | dO fragments and row constants in registers), against every key pair at kvb
  auto dq_tile = [&](int bh_, unsigned kvb, const bf16x8 (&qf0)[QT], const bf16x8 (&qf1)[QT], const bf16x8 (&df0)[QT], const bf16x8 (&df1)[QT],
                     const float (&nl)[QT], const float (&nd)[QT]) {
    BWDP_LANE_OFFSETS()
    const unsigned kb0 = kvb + roff0, kb1 = kvb + roff1, vb0 = kvb + IMG + voff0, vb1 = kvb + IMG + voff1;
    unsigned tk[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) tk[dt] = kvb + toff[dt];
    f32x4 dq[QT][4];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) dq[t][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    static_for<0, NKT / 2>([&](auto ic) {
      constexpr int u = decltype(ic)::value;
      bf16x8 ka0, ka1, kc0, kc1, va0, va1, vc0, vc1;         // key tiles 2u (a) and 2u+1 (c), k-steps 0 / 1
      AT_DS_B128_OFF(ka0, kb0, (2 * u) * 2048);     AT_DS_B128_OFF(va0, vb0, (2 * u) * 2048);
      AT_DS_B128_OFF(kc0, kb0, (2 * u + 1) * 2048); AT_DS_B128_OFF(vc0, vb0, (2 * u + 1) * 2048);
      AT_DS_B128_OFF(ka1, kb1, (2 * u) * 2048);     AT_DS_B128_OFF(va1, vb1, (2 * u) * 2048);
      AT_DS_B128_OFF(kc1, kb1, (2 * u + 1) * 2048); AT_DS_B128_OFF(vc1, vb1, (2 * u + 1) * 2048);
      bf16x4 klo[4], khi[4];                       // K^T fragments of the dQ product: in flight under the first products
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) { AT_DS_TR_OFF(klo[dt], tk[dt], u * 4096); AT_DS_TR_OFF(khi[dt], tk[dt], u * 4096 + 2048); }
      asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(ka0), "+v"(va0), "+v"(kc0), "+v"(vc0), "+v"(ka1), "+v"(va1), "+v"(kc1), "+v"(vc1));
      bf16x8 dsf[QT];
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        f32x4 sa = {nl[t], nl[t], nl[t], nl[t]}, sc_ = sa, pa = {nd[t], nd[t], nd[t], nd[t]}, pc = pa;
        sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka0, qf0[t], sa, 0, 0, 0);       // S'^T[key][q]
        pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va0, df0[t], pa, 0, 0, 0);       // dP'^T[key][q]
        sc_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc0, qf0[t], sc_, 0, 0, 0);
        pc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vc0, df0[t], pc, 0, 0, 0);
        sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka1, qf1[t], sa, 0, 0, 0);
        pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va1, df1[t], pa, 0, 0, 0);
        sc_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc1, qf1[t], sc_, 0, 0, 0);
        pc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vc1, df1[t], pc, 0, 0, 0);
        f32x4 dsa, dsc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float xa = sa[r] * c1, xc = sc_[r] * c1;
          if (u == NKT / 2 - 1) {                    // only the last key pair holds keys beyond S (S > 16 (NKT - 2))
            xa = (2 * u) * 16 + 4 * g + r < S ? xa : -INFINITY;
            xc = (2 * u + 1) * 16 + 4 * g + r < S ? xc : -INFINITY;
          }
          dsa[r] = __builtin_amdgcn_exp2f(xa) * pa[r];        // p (dP - D); a padded query has lse = +inf -> p = 0
          dsc[r] = __builtin_amdgcn_exp2f(xc) * pc[r];        // (the score scale is applied to dQ below)
        }
        dsf[t] = pack_pair(dsa, dsc);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(klo[0]), "+v"(khi[0]), "+v"(klo[1]), "+v"(khi[1]), "+v"(klo[2]), "+v"(khi[2]), "+v"(klo[3]), "+v"(khi[3]));
#pragma unroll
      for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          dq[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_shufflevector(klo[dt], khi[dt], 0, 1, 2, 3, 4, 5, 6, 7), dsf[t], dq[t][dt], 0, 0, 0);   // dQ^T[d][q]
    });
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const int q = (QT * wave + t) * 16 + l16;
      bf16_t* drow = dqkv + ((int64_t)(bh_ / H) * S + (q < S ? q : S - 1)) * ld + (bh_ % H) * AT_DH;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (bf16_t)(dq[t][dt][r] * scale);
        if (q < S) *reinterpret_cast<bf16x4*>(drow + dt * 16 + 4 * g) = v;
      }
    }
  };

  // The same split in two for the steady state: EVERY thread issues the loads of its RC2 rows of head i+1 right after the mid
  // barrier (inline asm, destinations untouched until the wait) and reduces them after its dQ part, when they have long landed --
  // one wave alone needs three round trips per head for the 1,576 row chunks, which made IT the critical path (measured).
  // The loads stay in flight across the whole dQ part, so their destinations must be registers the COMPILER never touches: with "=v"
  // outputs it is free to copy a "defined" value before the wait (live-range split under pressure: seen once, DESIGN K2 round 4).
  // The kernel is therefore compiled for v0 .. v[BWDP_VGPRS - 1] (amdgpu_num_vgpr) and the loads land in FIXED registers above that
  // range, named in the asm text; they enter the compiler's view only through the v_movs of rc_finish, which sit BEHIND the
  // s_waitcnt in the same asm statement.  tools/check_inflight_regs.py verifies the ISA (CPU test).
  constexpr int RC2 = (NCONST * 8 + 64 * NW - 1) / (64 * NW);
  static_assert(RC2 == 4 && BWDP_VGPRS == 216, "the landing registers below are written out for four row chunks per thread: v216 .. v251");
#define RC_CLOB "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223", "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", \
                "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", \
                "v248", "v249", "v250", "v251"
#define RC_ISSUE(i, XR, YR, LR)                                                                                           \
  {                                                                                                                       \
    const int e = tid_o + (i) * 64 * NW;                                                                                  \
    int q = e >> 3;                                                                                                       \
    q = q < S ? q : S - 1;                                                                                                \
    const bf16_t* pd = dO + (int64_t)q * ldo + (e & 7) * 8;                                                               \
    const bf16_t* po = O + (int64_t)q * ldo + (e & 7) * 8;                                                                \
    const float* pl = Lp + q;                                                                                             \
    asm volatile("global_load_dwordx4 " XR ", %0, off\n\tglobal_load_dwordx4 " YR ", %1, off\n\tglobal_load_dword " LR ", %2, off" \
                 :: "v"(pd), "v"(po), "v"(pl) : "memory", RC_CLOB);                                                       \
  }
  auto rc_issue = [&](int bh_) {
    const bf16_t* O = out + (int64_t)(bh_ / H) * S * ldo + (bh_ % H) * AT_DH;
    const bf16_t* dO = dout + (int64_t)(bh_ / H) * S * ldo + (bh_ % H) * AT_DH;
    const float* Lp = lse + (int64_t)bh_ * S;
    int tid_o = threadIdx.x;
    asm volatile("" : "+v"(tid_o));
    RC_ISSUE(0, "v[216:219]", "v[232:235]", "v248")
    RC_ISSUE(1, "v[220:223]", "v[236:239]", "v249")
    RC_ISSUE(2, "v[224:227]", "v[240:243]", "v250")
    RC_ISSUE(3, "v[228:231]", "v[244:247]", "v251")
  };
  typedef uint32_t rc_u32x4 __attribute__((ext_vector_type(4)));
#define RC_TAKE(i, X0, X1, X2, X3, Y0, Y1, Y2, Y3, LR)                                                                    \
  {                                                                                                                       \
    rc_u32x4 xw, yw;                                                                                                      \
    asm volatile("s_waitcnt vmcnt(0)\n\tv_mov_b32 %0, " X0 "\n\tv_mov_b32 %1, " X1 "\n\tv_mov_b32 %2, " X2 "\n\tv_mov_b32 %3, " X3 "\n\t" \
                 "v_mov_b32 %4, " Y0 "\n\tv_mov_b32 %5, " Y1 "\n\tv_mov_b32 %6, " Y2 "\n\tv_mov_b32 %7, " Y3 "\n\tv_mov_b32 %8, " LR         \
                 : "=&v"(xw[0]), "=&v"(xw[1]), "=&v"(xw[2]), "=&v"(xw[3]), "=&v"(yw[0]), "=&v"(yw[1]), "=&v"(yw[2]), "=&v"(yw[3]), "=&v"(Lr[i]) \
                 :: "memory");                                                                                            \
    x[i] = __builtin_bit_cast(bf16x8, xw);                                                                                \
    y[i] = __builtin_bit_cast(bf16x8, yw);                                                                                \
  }
  auto rc_finish = [&]() {
    bf16x8 x[RC2], y[RC2];
    float Lr[RC2];
    RC_TAKE(0, "v216", "v217", "v218", "v219", "v232", "v233", "v234", "v235", "v248")
    RC_TAKE(1, "v220", "v221", "v222", "v223", "v236", "v237", "v238", "v239", "v249")
    RC_TAKE(2, "v224", "v225", "v226", "v227", "v240", "v241", "v242", "v243", "v250")
    RC_TAKE(3, "v228", "v229", "v230", "v231", "v244", "v245", "v246", "v247", "v251")
    int tid_o = threadIdx.x;
    asm volatile("" : "+v"(tid_o));
#pragma unroll
    for (int i = 0; i < RC2; ++i) {
      const int e = tid_o + i * 64 * NW;
      const int q = e >> 3, c = e & 7;
      float a = 0.f;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) a += (float)x[i][jj] * (float)y[i][jj];
      a += __shfl_xor(a, 1, 64); a += __shfl_xor(a, 2, 64); a += __shfl_xor(a, 4, 64);
      if (c == 0 && e < NCONST * 8) {
        const float L = q < S ? Lr[i] * LOG2E : INFINITY;
        lse_s[q] = -L * inv_c1; dsum_s[q] = q < S ? -a : 0.f;
      }
    }
  };
#undef RC_ISSUE
#undef RC_TAKE
#undef RC_CLOB

  // prologue: head 0 of this workgroup
  stage_kv(0, bh);
  stage_qd(bh);
  row_constants(bh, 0, 64 * NW);
  int cur = 0;
  for (;;) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                    // K | V (pair cur), Q | dO and the row constants of head bh are complete
    const int nxt = bh + (int)gridDim.x;
    const unsigned kvb = lds0 + CONSTB + (2 * cur) * IMG;
    if (nxt < nbh) stage_kv(cur ^ 1, nxt);
    if (has_tile) dkv_tile(bh, kvb);
    bf16x8 qf0[QT], qf1[QT], df0[QT], df1[QT];
    float nl[QT], nd[QT];
    if (has_tile) {                     // this wave's Q | dO fragments and row constants leave LDS before slots 4,5 are refilled
      BWDP_LANE_OFFSETS()
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        const unsigned q0b = (QT * wave + t) * 16 * 128;
        AT_DS_B128_OFF(qf0[t], QB + roff0 + q0b, 0); AT_DS_B128_OFF(qf1[t], QB + roff1 + q0b, 0);
        AT_DS_B128_OFF(df0[t], DB + roff0 + q0b, 0); AT_DS_B128_OFF(df1[t], DB + roff1 + q0b, 0);
        asm volatile("ds_read_b32 %0, %1" : "=v"(nl[t]) : "v"(lds0 + ((QT * wave + t) * 16 + l16) * 4));
        asm volatile("ds_read_b32 %0, %1" : "=v"(nd[t]) : "v"(lds0 + (NCONST + (QT * wave + t) * 16 + l16) * 4));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int t = 0; t < QT; ++t) asm volatile("" : "+v"(qf0[t]), "+v"(qf1[t]), "+v"(df0[t]), "+v"(df1[t]), "+v"(nl[t]), "+v"(nd[t]));
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // LDS only: the K | V DMA of head nxt stays in flight
    if (nxt < nbh) {
      stage_qd(nxt);
      rc_issue(nxt);
    }
    if (has_tile) dq_tile(bh, kvb, qf0, qf1, df0, df1, nl, nd);
    if (nxt >= nbh) break;
    rc_finish();
    bh = nxt; cur ^= 1;
  }
#undef BWDP_LANE_OFFSETS
}

#define BIAS_EXTRA(n) ((n) * 16 * 4)
#define STAT_EXTRA(n) (2 * (n) * 16 * 4)

int mmrca_mha_fwd_mfma(const void* qkv, const int32_t* key_mask, void* out, float* lse, int B, int H, int S, int dh,
                       float scale, float drop_p, uint64_t drop_seed, const int32_t* cu, hipStream_t st) {
  (void)dh;
  MMRCA_REQUIRE((((uintptr_t)qkv) & 15) == 0 && (((uintptr_t)out) & 7) == 0, "mha_fwd: qkv must be 16-byte aligned");
  const int nkt = pick_nkt(S);
  if (nkt == 14 && drop_p <= 0.f && !key_mask && !cu && S > 16 * 12) {     // the ViT's attention: 197 tokens, no mask
    const int ldsb = 4 * 14 * 16 * 128;
    const int nbh = B * H, grid = nbh < attn_cu_count() ? nbh : attn_cu_count();
    MMRCA_MAX_LDS(ldsb, mha_fwd_mfma_p_k<14, 16>);
    hipLaunchKernelGGL((mha_fwd_mfma_p_k<14, 16>), dim3(grid), dim3(1024), ldsb, st, (const bf16_t*)qkv, (bf16_t*)out, lse, H, S, scale, nbh);
    MMRCA_CHECK_LAUNCH("mha_fwd(mfma,persistent)");
    return 0;
  }
  AT_SWITCH(K_FWD, BIAS_EXTRA, true, false, false, (const bf16_t*)qkv, key_mask, (bf16_t*)out, lse, H, S, scale, drop_p, drop_seed, cu);
  MMRCA_CHECK_LAUNCH("mha_fwd(mfma)");
  return 0;
}

// bf16x3 attention forward: head dim 64; S <= 224 on the resident-image kernels (mha_fwd_x3_p_k, mha_fwd_x3_k), 225 <= S <= 512 on the
// chunked-key kernel (mha_fwd_x3_c_k)
bool mmrca_mha_x3_ok(int S, int dh) { return dh == AT_DH && S >= 1 && S <= AT_MAX_S; }
int mmrca_mha_fwd_x3_launch(const void* qkv_hi, const void* qkv_lo, const int32_t* key_mask, void* out_hi, void* out_lo, float* lse, int B, int H,
                            int S, int dh, float scale, float drop_p, uint64_t drop_seed, const int32_t* cu, hipStream_t st) {
  MMRCA_REQUIRE(mmrca_mha_x3_ok(S, dh), "mha_fwd_x3: needs head dim 64 and 1 <= S <= 512 (got S=%d dh=%d)", S, dh);
  MMRCA_REQUIRE(((((uintptr_t)qkv_hi) | ((uintptr_t)qkv_lo)) & 15) == 0 && ((((uintptr_t)out_hi) | ((uintptr_t)out_lo)) & 7) == 0, "mha_fwd_x3: alignment");
  if (S > 224) {      // key chunks of 128, 128 queries per workgroup
    const int ldsb = 4 * AT_CK * 128 + AT_MAX_S * 4, nqg = (S + 127) / 128;
    MMRCA_REQUIRE((int64_t)B * H * nqg <= 0x7fffffff, "mha_fwd_x3: grid too large");
    if (drop_p > 0.f) {
      MMRCA_MAX_LDS(ldsb, mha_fwd_x3_c_k<true>);
      hipLaunchKernelGGL((mha_fwd_x3_c_k<true>), dim3(B * H * nqg), dim3(512), ldsb, st, (const bf16_t*)qkv_hi, (const bf16_t*)qkv_lo, key_mask,
                         (bf16_t*)out_hi, (bf16_t*)out_lo, lse, H, S, scale, drop_p, drop_seed, cu, nqg);
    } else {
      MMRCA_MAX_LDS(ldsb, mha_fwd_x3_c_k<false>);
      hipLaunchKernelGGL((mha_fwd_x3_c_k<false>), dim3(B * H * nqg), dim3(512), ldsb, st, (const bf16_t*)qkv_hi, (const bf16_t*)qkv_lo, key_mask,
                         (bf16_t*)out_hi, (bf16_t*)out_lo, lse, H, S, scale, drop_p, drop_seed, cu, nqg);
    }
    MMRCA_CHECK_LAUNCH("mha_fwd_x3(chunked)");
    return 0;
  }
  const int nkt = pick_nkt(S);
  if (nkt == 14 && drop_p <= 0.f && !key_mask && !cu && S > 16 * 12) {     // the ViT's attention: 197 tokens, no mask
    const int ldsb = 4 * 14 * 16 * 128;
    const int nbh = B * H, grid = nbh < attn_cu_count() ? nbh : attn_cu_count();
    MMRCA_MAX_LDS(ldsb, mha_fwd_x3_p_k<14, 16>);
    hipLaunchKernelGGL((mha_fwd_x3_p_k<14, 16>), dim3(grid), dim3(1024), ldsb, st, (const bf16_t*)qkv_hi, (const bf16_t*)qkv_lo, (bf16_t*)out_hi,
                       (bf16_t*)out_lo, lse, H, S, scale, nbh);
    MMRCA_CHECK_LAUNCH("mha_fwd_x3(persistent)");
    return 0;
  }
#define LX3(NKT_, DROP_, NW_)                                                                                                      \
  do {                                                                                                                             \
    const int ldsb = 4 * NKT_ * 16 * 128 + BIAS_EXTRA(NKT_);                                                                       \
    MMRCA_MAX_LDS(ldsb, mha_fwd_x3_k<NKT_, DROP_, NW_>);      \
    hipLaunchKernelGGL((mha_fwd_x3_k<NKT_, DROP_, NW_>), dim3(B * H), dim3(64 * NW_), ldsb, st, (const bf16_t*)qkv_hi, (const bf16_t*)qkv_lo, key_mask, \
                       (bf16_t*)out_hi, (bf16_t*)out_lo, lse, H, S, scale, drop_p, drop_seed, cu);                                 \
  } while (0)
  const bool drop = drop_p > 0.f;
  switch (nkt) {
    case 2: if (drop) LX3(2, true, 4); else LX3(2, false, 4); break;
    case 4: if (drop) LX3(4, true, 4); else LX3(4, false, 4); break;
    case 8: if (drop) LX3(8, true, 8); else LX3(8, false, 8); break;
    default: if (drop) LX3(14, true, 8); else LX3(14, false, 8); break;
  }
#undef LX3
  MMRCA_CHECK_LAUNCH("mha_fwd_x3");
  return 0;
}

// diagnostic: device buffer [B*H][4] of uint64 that the fused backward fills with its phase stamps (nullptr = off, the default)
static unsigned long long* g_attn_stamps = nullptr;
extern "C" int mmrca_debug_attn_stamps(void* buf) { g_attn_stamps = (unsigned long long*)buf; return 0; }

int mmrca_mha_bwd_mfma(const void* qkv, const int32_t* key_mask, const void* out, const void* dout, const float* lse,
                       void* dqkv, int B, int H, int S, int dh, float scale, float drop_p, uint64_t drop_seed,
                       const int32_t* cu, hipStream_t st) {
  (void)dh;
  MMRCA_REQUIRE((((uintptr_t)qkv) & 15) == 0 && (((uintptr_t)out) & 15) == 0 && (((uintptr_t)dout) & 15) == 0 && (((uintptr_t)dqkv) & 7) == 0,
                "mha_bwd: buffers must be 16-byte aligned");
  const int nkt = pick_nkt(S);
  const bool vit = nkt == 14 && drop_p <= 0.f && !key_mask && !cu && S > 16 * 12;      // the ViT's attention
  if (vit && S <= 16 * 13) {
    // persistent 8-wave workgroups (two tiles per wave), six image slots: every operand crosses the fabric once
    const int nbh = B * H;
    const int grid = nbh < attn_cu_count() ? nbh : attn_cu_count();
    const int ldp = 2 * 14 * 16 * 4 + 6 * 13 * 16 * 128 + 2048;
    MMRCA_MAX_LDS(ldp, mha_bwd_p_mfma_v_k<14, 8, 2>);
    hipLaunchKernelGGL((mha_bwd_p_mfma_v_k<14, 8, 2>), dim3(grid), dim3(512), ldp, st, (const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)dout, lse,
                       (bf16_t*)dqkv, H, S, scale, nbh);
    MMRCA_CHECK_LAUNCH("mha_bwd(mfma,persistent)");
    return 0;
  }
  if (vit) {     // S in (208, 224]: one launch, two workgroups per CU: the Q | dO and K | V images time-share 56 KiB
    const int ldf = 2 * 14 * 16 * 128 + STAT_EXTRA(14);
    MMRCA_MAX_LDS(ldf, mha_bwd_fused_mfma_v_k<14, 8>);
    hipLaunchKernelGGL((mha_bwd_fused_mfma_v_k<14, 8>), dim3(B * H), dim3(512), ldf, st, (const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)dout, lse,
                       (bf16_t*)dqkv, H, S, scale, g_attn_stamps);
    MMRCA_CHECK_LAUNCH("mha_bwd(mfma,fused)");
    return 0;
  }
  AT_SWITCH(K_DQ, BIAS_EXTRA, true, true, true, (const bf16_t*)qkv, key_mask, (const bf16_t*)out, (const bf16_t*)dout, lse, (bf16_t*)dqkv, H, S, scale, drop_p, drop_seed, cu);
  AT_SWITCH(K_DKV, STAT_EXTRA, true, false, true, (const bf16_t*)qkv, key_mask, (const bf16_t*)out, (const bf16_t*)dout, lse, (bf16_t*)dqkv, H, S, scale, drop_p, drop_seed, cu);
  MMRCA_CHECK_LAUNCH("mha_bwd(mfma)");
  return 0;
}

MMRCA_SEED_EPOCH_EXPORT(attention_mfma)   // this translation unit's copy of the mask epoch (common.h)
