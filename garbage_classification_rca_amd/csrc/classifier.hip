// Linear classification head of the single-backbone classifiers (classifiers.py): logits = dropout(feat) W^T + b.
//
// The reference's heads are one nn.Linear behind an optional nn.Dropout: torchvision's vit_b_16 / vit_l_16 `heads.head`,
// efficientnet_v2_m / _l `classifier = Sequential(Dropout(p), Linear)`, shufflenet_v2 `fc`, and the text models' `drop` + `out`
// (CVPR_code/text_models.py).  B x F x C is at most 512 x 2048 x 16: launch-bound work, so both directions are one launch each and
// every product runs in fp32 whatever the feature dtype.
#include "common.h"

#define CLS_FWD_THREADS 256
#define CLS_BWD_WAVES 8
#define CLS_BWD_CHUNK 64      // samples of dlogits staged in LDS at a time

// inverted-dropout factor of feature (b, f): the counter hash of (seed + epoch, b*F + f), as every other dropout site
__device__ __forceinline__ float cls_keep(float p, float inv, uint64_t seed, int b, int F, int f) {
  return mmrca_uniform(seed, (uint64_t)b * (uint64_t)F + (uint64_t)f) >= p ? inv : 0.f;
}

// one workgroup per sample: each thread owns 4 consecutive features per step, C partial dot products in registers, then a
// fixed-order reduction (shuffles inside a wave, the 4 waves in order) -- the same logits for the same inputs on every run
template <typename T, int NC>
__global__ void __launch_bounds__(CLS_FWD_THREADS)
linear_cls_fwd_k(const T* __restrict__ feat, int ld, const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ logits,
                 int F, int C, float p, uint64_t seed) {
  __shared__ float red[CLS_FWD_THREADS / 64][NC];
  const int b = blockIdx.x, t = threadIdx.x;
  const float inv = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const T* x = feat + (int64_t)b * ld;
  float acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.f;
  for (int f = t * 4; f < F; f += CLS_FWD_THREADS * 4) {
    Vec4<T> xv = Vec4<T>::load(x + f);
    if (p > 0.f) {
#pragma unroll
      for (int k = 0; k < 4; ++k) xv.v[k] *= cls_keep(p, inv, seed, b, F, f + k);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < C) {
        const Vec4<float> w = Vec4<float>::load(W + (int64_t)c * F + f);
        acc[c] = fmaf(xv.v[0], w.v[0], fmaf(xv.v[1], w.v[1], fmaf(xv.v[2], w.v[2], fmaf(xv.v[3], w.v[3], acc[c]))));
      }
    }
  }
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const float s = wave_sum(acc[c]);
    if (lane == 0) red[wave][c] = s;
  }
  __syncthreads();
  if (t < C) {
    float s = bias[t];
#pragma unroll
    for (int w = 0; w < CLS_FWD_THREADS / 64; ++w) s += red[w][t];
    logits[(int64_t)b * C + t] = s;
  }
}

// one workgroup per 64 feature columns, one lane per column; wave w walks the samples w, w + 8, ... and the 8 waves' partial
// weight gradients are summed in wave order -- no atomics, a fixed summation order.  dfeat[b, f] = keep(b, f) * sum_c dl[b, c] W[c, f]
// needs only the lane's own column of W, so it comes out of the same pass.  db: workgroup 0, lanes c < C, samples in order.
template <typename T, int NC>
__global__ void __launch_bounds__(CLS_BWD_WAVES * 64)
linear_cls_bwd_k(const float* __restrict__ dlogits, const T* __restrict__ feat, int ld, const float* __restrict__ W, float* __restrict__ dW,
                 float* __restrict__ db, T* __restrict__ dfeat, int B, int F, int C, float p, uint64_t seed) {
  __shared__ float dls[CLS_BWD_CHUNK * NC];
  __shared__ float red[CLS_BWD_WAVES][NC][64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int f = blockIdx.x * 64 + lane;
  const bool col = f < F;
  const float inv = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float w[NC], acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    w[c] = (col && c < C) ? W[(int64_t)c * F + f] : 0.f;
    acc[c] = 0.f;
  }
  for (int b0 = 0; b0 < B; b0 += CLS_BWD_CHUNK) {
    const int nb = min(CLS_BWD_CHUNK, B - b0);
    __syncthreads();                           // (the previous chunk's readers are done)
    for (int i = t; i < nb * NC; i += CLS_BWD_WAVES * 64) {
      const int bb = i / NC, c = i - bb * NC;
      dls[i] = c < C ? dlogits[(int64_t)(b0 + bb) * C + c] : 0.f;
    }
    __syncthreads();
    if (col) {
      for (int bb = wave; bb < nb; bb += CLS_BWD_WAVES) {
        const int b = b0 + bb;
        const float m = p > 0.f ? cls_keep(p, inv, seed, b, F, f) : 1.f;
        const float xd = to_f(feat[(int64_t)b * ld + f]) * m;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const float d = dls[bb * NC + c];
          acc[c] = fmaf(d, xd, acc[c]);
          s = fmaf(d, w[c], s);
        }
        if (dfeat) dfeat[(int64_t)b * F + f] = from_f<T>(s * m);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) red[wave][c][lane] = acc[c];
  __syncthreads();
  if (wave == 0 && col) {
    for (int c = 0; c < C; ++c) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < CLS_BWD_WAVES; ++k) s += red[k][c][lane];
      dW[(int64_t)c * F + f] += s;
    }
  }
  if (blockIdx.x == 0 && wave == 1 && lane < C) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dlogits[(int64_t)b * C + lane];
    db[lane] += s;
  }
}

template <class F>
static int cls_dispatch_nc(int C, F&& f) {
  if (C <= 4) return f(std::integral_constant<int, 4>{});
  if (C <= 8) return f(std::integral_constant<int, 8>{});
  return f(std::integral_constant<int, 16>{});
}

static int cls_check(const char* name, const void* feat, int ld, int B, int F, int C, float p, int dtype) {
  MMRCA_REQUIRE(B >= 1 && F >= 4 && C >= 1 && C <= 16, "%s: bad shape B=%d F=%d C=%d (1 <= C <= 16)", name, B, F, C);
  MMRCA_REQUIRE(F % 4 == 0 && ld >= F && ld % 4 == 0, "%s: F (%d) and ld (%d) must be multiples of 4, ld >= F", name, F, ld);
  MMRCA_REQUIRE((uintptr_t)feat % (dtype == MMRCA_BF16 ? 8 : 16) == 0, "%s: feat must be aligned to 4 elements", name);
  MMRCA_REQUIRE(p >= 0.f && p < 1.f, "%s: drop_p %f outside [0, 1)", name, (double)p);
  return 0;
}

extern "C" int mmrca_linear_cls_fwd(const void* feat, int ld, const float* W, const float* b, float* logits, int B, int F, int C,
                                    float drop_p, uint64_t seed, int dtype, void* stream) {
  if (int rc = cls_check("linear_cls_fwd", feat, ld, B, F, C, drop_p, dtype)) return rc;
  MMRCA_REQUIRE(((uintptr_t)W & 15) == 0, "linear_cls_fwd: W must be 16-byte aligned");
  MMRCA_DISPATCH_DTYPE(dtype, "linear_cls_fwd", {
    return cls_dispatch_nc(C, [&](auto nc) {
      hipLaunchKernelGGL((linear_cls_fwd_k<T, decltype(nc)::value>), dim3(B), dim3(CLS_FWD_THREADS), 0, (hipStream_t)stream,
                         (const T*)feat, ld, W, b, logits, F, C, drop_p, seed);
      MMRCA_CHECK_LAUNCH("linear_cls_fwd");
      return 0;
    });
  })
}

extern "C" int mmrca_linear_cls_bwd(const float* dlogits, const void* feat, int ld, const float* W, float* dW, float* db, void* dfeat,
                                    int B, int F, int C, float drop_p, uint64_t seed, int dtype, void* stream) {
  if (int rc = cls_check("linear_cls_bwd", feat, ld, B, F, C, drop_p, dtype)) return rc;
  MMRCA_DISPATCH_DTYPE(dtype, "linear_cls_bwd", {
    return cls_dispatch_nc(C, [&](auto nc) {
      hipLaunchKernelGGL((linear_cls_bwd_k<T, decltype(nc)::value>), dim3((F + 63) / 64), dim3(CLS_BWD_WAVES * 64), 0, (hipStream_t)stream,
                         dlogits, (const T*)feat, ld, W, dW, db, (T*)dfeat, B, F, C, drop_p, seed);
      MMRCA_CHECK_LAUNCH("linear_cls_bwd");
      return 0;
    });
  })
}

MMRCA_SEED_EPOCH_EXPORT(classifier)   // this translation unit's copy of the mask epoch (common.h)
