// MobileBERT's row operators (transformers modeling_mobilebert.py): NoNorm -- the element-wise affine y = x * weight + bias the
// model uses wherever BERT has a LayerNorm (:55-62) -- fused with the residual add in front of it, and the trigram input embedding
// (:113-128).  Everything else of the model (GEMMs, dh = 32 attention, ReLU, classifier head) is existing library code.
//
// fp32 arithmetic on fp32 / bf16 operands; parameter gradients are fp32 and accumulate (+=).  16-byte accesses (4 fp32 / 8 bf16 per
// lane) when D, the row pitches and the pointers allow, one element per lane otherwise.  No host synchronisation, no allocation.
#include "common.h"

namespace {

template <typename T, int V> struct VecN {
  float v[V];
  typedef T raw_t __attribute__((ext_vector_type(V)));
  __device__ __forceinline__ static VecN load(const T* p) {
    VecN r;
    if constexpr (V == 1) { r.v[0] = to_f(*p); }
    else {
      raw_t t = *reinterpret_cast<const raw_t*>(p);
#pragma unroll
      for (int j = 0; j < V; ++j) r.v[j] = to_f((T)t[j]);
    }
    return r;
  }
  __device__ __forceinline__ void store(T* p) const {
    if constexpr (V == 1) { *p = from_f<T>(v[0]); }
    else {
      raw_t t;
#pragma unroll
      for (int j = 0; j < V; ++j) t[j] = from_f<T>(v[j]);
      *reinterpret_cast<raw_t*>(p) = t;
    }
  }
};

inline bool aligned_to(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }
template <typename T> constexpr int full_vec() { return 16 / (int)sizeof(T); }

// ---------------------------------------------------------------------------------------------------------------------
// NoNorm forward: s = x (+ res), y = s * gamma + beta.  One lane per V columns of one row.
// (x and sum_out may be the same buffer: a lane reads its V elements of x before it writes them.)
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, int V>
__global__ void __launch_bounds__(256)
nonorm_fwd_k(const T* x, const T* __restrict__ res, const T* __restrict__ gamma, const T* __restrict__ beta, T* sum_out,
             T* __restrict__ y, int64_t rows, int D, int64_t ld_x, int64_t ld_res, int64_t ld_sum, int64_t ld_y) {
  const int per_row = D / V;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * per_row) return;
  const int64_t r = idx / per_row;
  const int c = (int)(idx - r * per_row) * V;
  VecN<T, V> a = VecN<T, V>::load(x + r * ld_x + c);
  if (res) {
    const VecN<T, V> b = VecN<T, V>::load(res + r * ld_res + c);
#pragma unroll
    for (int j = 0; j < V; ++j) a.v[j] += b.v[j];
  }
  if (sum_out) {
    a.store(sum_out + r * ld_sum + c);
#pragma unroll
    for (int j = 0; j < V; ++j) a.v[j] = to_f(from_f<T>(a.v[j]));      // y is computed from the sum as stored (what the backward reads)
  }
  const VecN<T, V> g = VecN<T, V>::load(gamma + c), b2 = VecN<T, V>::load(beta + c);
#pragma unroll
  for (int j = 0; j < V; ++j) a.v[j] = fmaf(a.v[j], g.v[j], b2.v[j]);
  a.store(y + r * ld_y + c);
}

// ---------------------------------------------------------------------------------------------------------------------
// NoNorm backward, pass 1: ds_out = (dres +) dy * gamma, and per row slab the partial column sums of dy * s and of dy.
// Block = CT column lanes x (256 / CT) row lanes; a block owns CT * V columns and one slab of rows.  The row lanes' partials meet
// in LDS and are added in lane order; slab partials go to the workspace ws[slab][2][D] and pass 2 adds them in slab order: no
// atomics, the same bits every time.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, int V>
__global__ void __launch_bounds__(256)
nonorm_bwd_k(const T* __restrict__ dy, const T* __restrict__ s, const T* __restrict__ gamma, const T* dres, T* ds_out,
             float* __restrict__ ws, int64_t rows, int D, int64_t ld_dy, int64_t ld_s, int64_t ld_dres, int64_t ld_ds,
             int ct, int64_t rows_per_slab) {
  __shared__ float red[2][256 * V];
  const int rt = 256 / ct;
  const int tx = threadIdx.x % ct, ty = threadIdx.x / ct;
  const int c = (blockIdx.x * ct + tx) * V;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab;
  int64_t r1 = r0 + rows_per_slab;
  if (r1 > rows) r1 = rows;
  float a[V], b[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { a[j] = 0.f; b[j] = 0.f; }
  if (c < D) {
    const VecN<T, V> g = VecN<T, V>::load(gamma + c);
    for (int64_t r = r0 + ty; r < r1; r += rt) {
      const VecN<T, V> d = VecN<T, V>::load(dy + r * ld_dy + c), sv = VecN<T, V>::load(s + r * ld_s + c);
      VecN<T, V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        o.v[j] = d.v[j] * g.v[j];
        a[j] = fmaf(d.v[j], sv.v[j], a[j]);
        b[j] += d.v[j];
      }
      if (dres) {
        const VecN<T, V> e = VecN<T, V>::load(dres + r * ld_dres + c);
#pragma unroll
        for (int j = 0; j < V; ++j) o.v[j] += e.v[j];
      }
      o.store(ds_out + r * ld_ds + c);
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) { red[0][threadIdx.x * V + j] = a[j]; red[1][threadIdx.x * V + j] = b[j]; }
  __syncthreads();
  if (ty == 0 && c < D) {
    float* w = ws + (int64_t)blockIdx.y * 2 * D;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float sa = 0.f, sb = 0.f;
      for (int k = 0; k < rt; ++k) { sa += red[0][(k * ct + tx) * V + j]; sb += red[1][(k * ct + tx) * V + j]; }
      w[c + j] = sa;
      w[D + c + j] = sb;
    }
  }
}

// pass 2: dgamma += sum_slabs (dy * s), dbeta += sum_slabs dy, dbias += gamma * sum_slabs dy; one lane per column, slabs in order
template <typename T>
__global__ void __launch_bounds__(256)
nonorm_bwd_finish_k(const float* __restrict__ ws, const T* __restrict__ gamma, float* __restrict__ dgamma,
                    float* __restrict__ dbeta, float* __restrict__ dbias, int D, int nslab) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  float a = 0.f, b = 0.f;
  for (int k = 0; k < nslab; ++k) {
    a += ws[(int64_t)k * 2 * D + c];
    b += ws[(int64_t)k * 2 * D + D + c];
  }
  dgamma[c] += a;
  dbeta[c] += b;
  if (dbias) dbias[c] += to_f(gamma[c]) * b;
}

inline void nonorm_slabs(int64_t rows, int& nslab, int64_t& rows_per_slab) {
  int64_t n = (rows + 31) / 32;
  if (n > 256) n = 256;
  if (n < 1) n = 1;
  rows_per_slab = (rows + n - 1) / n;
  nslab = (int)((rows + rows_per_slab - 1) / rows_per_slab);
}

// ---------------------------------------------------------------------------------------------------------------------
// Trigram embedding.  Row r of the output is token p = perm ? perm[r] : r of the PADDED [B, T] id matrix (t = p % T):
//   out[r] = word[ids[p + 1]] (zeros at t = T - 1) | word[ids[p]] | word[ids[p - 1]] (zeros at t = 0).
// The neighbours are always taken from the padded matrix, so in the packed layout a caption's last row reads its own padding
// (or zeros), never the next caption's first token.  An id or a perm entry outside its table yields zeros.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t trigram_id(const int32_t* __restrict__ ids, int64_t p, int slot, int T, int64_t n_tok, int vocab) {
  if (p < 0 || p >= n_tok) return -1;
  const int t = (int)(p % T);
  int64_t q = p;
  if (slot == 0) { if (t == T - 1) return -1; q = p + 1; }
  else if (slot == 2) { if (t == 0) return -1; q = p - 1; }
  const int64_t id = ids[q];
  return (id < 0 || id >= vocab) ? -1 : id;
}

template <typename T, int V>
__global__ void __launch_bounds__(256)
trigram_fwd_k(const int32_t* __restrict__ ids, const int32_t* __restrict__ perm, const T* __restrict__ word, T* __restrict__ out,
              int64_t M, int Tn, int64_t n_tok, int E, int vocab) {
  const int per_slot = E / V, per_row = 3 * per_slot;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * per_row) return;
  const int64_t r = idx / per_row;
  const int rem = (int)(idx - r * per_row);
  const int slot = rem / per_slot, c = (rem - slot * per_slot) * V;
  const int64_t id = trigram_id(ids, perm ? (int64_t)perm[r] : r, slot, Tn, n_tok, vocab);
  VecN<T, V> a;
  if (id >= 0) a = VecN<T, V>::load(word + id * E + c);
  else {
#pragma unroll
    for (int j = 0; j < V; ++j) a.v[j] = 0.f;
  }
  a.store(out + r * 3 * E + slot * E + c);
}

// backward: the three column blocks of dout scatter into the fp32 dword with fp32 atomicAdd (ids repeat across rows and slots) --
// mmrca_embed_bwd's method; exact zeros (dead rows under class-token pooling) are skipped, and so are slots whose id is pad_id.
template <typename T, int V>
__global__ void __launch_bounds__(256)
trigram_bwd_k(const T* __restrict__ dout, const int32_t* __restrict__ ids, const int32_t* __restrict__ perm, float* __restrict__ dword,
              int64_t M, int Tn, int64_t n_tok, int E, int vocab, int pad_id) {
  const int per_slot = E / V, per_row = 3 * per_slot;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * per_row) return;
  const int64_t r = idx / per_row;
  const int rem = (int)(idx - r * per_row);
  const int slot = rem / per_slot, c = (rem - slot * per_slot) * V;
  const int64_t id = trigram_id(ids, perm ? (int64_t)perm[r] : r, slot, Tn, n_tok, vocab);
  if (id < 0 || id == pad_id) return;
  const VecN<T, V> d = VecN<T, V>::load(dout + r * 3 * E + slot * E + c);
#pragma unroll
  for (int j = 0; j < V; ++j)
    if (d.v[j] != 0.f) atomicAdd(dword + id * E + c + j, d.v[j]);
}

}  // namespace

extern "C" int mmrca_nonorm_fwd(const void* x, const void* res, const void* gamma, const void* beta, void* sum_out, void* y,
                                int64_t rows, int D, int64_t ld_x, int64_t ld_res, int64_t ld_sum, int64_t ld_y, int dtype,
                                void* stream) {
  MMRCA_REQUIRE(x && gamma && beta && y, "nonorm_fwd: null pointer");
  MMRCA_REQUIRE(D > 0 && ld_x >= D && ld_y >= D && (!res || ld_res >= D) && (!sum_out || ld_sum >= D), "nonorm_fwd: row pitch below D");
  if (rows <= 0) return 0;
  MMRCA_REQUIRE(rows * (int64_t)D < (1ll << 39), "nonorm_fwd: too many elements");
  MMRCA_DISPATCH_DTYPE(dtype, "nonorm_fwd", {
    constexpr int FV = full_vec<T>();
    const bool vec = D % FV == 0 && ld_x % FV == 0 && ld_y % FV == 0 && (!res || ld_res % FV == 0) && (!sum_out || ld_sum % FV == 0) &&
                     aligned_to(x, 16) && aligned_to(res, 16) && aligned_to(gamma, 16) && aligned_to(beta, 16) &&
                     aligned_to(sum_out, 16) && aligned_to(y, 16);
    const int64_t n = rows * (int64_t)(vec ? D / FV : D);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (vec)
      hipLaunchKernelGGL((nonorm_fwd_k<T, FV>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)x, (const T*)res, (const T*)gamma,
                         (const T*)beta, (T*)sum_out, (T*)y, rows, D, ld_x, ld_res, ld_sum, ld_y);
    else
      hipLaunchKernelGGL((nonorm_fwd_k<T, 1>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)x, (const T*)res, (const T*)gamma,
                         (const T*)beta, (T*)sum_out, (T*)y, rows, D, ld_x, ld_res, ld_sum, ld_y);
  })
  MMRCA_CHECK_LAUNCH("nonorm_fwd");
  return 0;
}

extern "C" int64_t mmrca_nonorm_bwd_workspace_bytes(int64_t rows, int D) {
  if (rows <= 0 || D <= 0) return 0;
  int nslab;
  int64_t rps;
  nonorm_slabs(rows, nslab, rps);
  return (int64_t)nslab * 2 * D * (int64_t)sizeof(float);
}

extern "C" int mmrca_nonorm_bwd(const void* dy, const void* s, const void* gamma, const void* dres, void* ds_out, float* dgamma,
                                float* dbeta, float* dbias, void* workspace, int64_t workspace_bytes, int64_t rows, int D,
                                int64_t ld_dy, int64_t ld_s, int64_t ld_dres, int64_t ld_ds, int dtype, void* stream) {
  MMRCA_REQUIRE(dy && s && gamma && ds_out && dgamma && dbeta && workspace, "nonorm_bwd: null pointer");
  MMRCA_REQUIRE(D > 0 && ld_dy >= D && ld_s >= D && ld_ds >= D && (!dres || ld_dres >= D), "nonorm_bwd: row pitch below D");
  if (rows <= 0) return 0;
  int nslab;
  int64_t rps;
  nonorm_slabs(rows, nslab, rps);
  MMRCA_REQUIRE(workspace_bytes >= (int64_t)nslab * 2 * D * (int64_t)sizeof(float) && aligned_to(workspace, 4),
                "nonorm_bwd: workspace of %lld bytes is below mmrca_nonorm_bwd_workspace_bytes(rows, D)", (long long)workspace_bytes);
  MMRCA_DISPATCH_DTYPE(dtype, "nonorm_bwd", {
    constexpr int FV = full_vec<T>();
    const bool vec = D % FV == 0 && ld_dy % FV == 0 && ld_s % FV == 0 && ld_ds % FV == 0 && (!dres || ld_dres % FV == 0) &&
                     aligned_to(dy, 16) && aligned_to(s, 16) && aligned_to(gamma, 16) && aligned_to(dres, 16) && aligned_to(ds_out, 16);
    const int cols = vec ? D / FV : D;                 // column lanes needed
    int ct = 1;
    while (ct < cols && ct < 256) ct *= 2;             // a power of two: divides the 256 lanes of a block
    const dim3 grid((unsigned)((cols + ct - 1) / ct), (unsigned)nslab);
    if (vec)
      hipLaunchKernelGGL((nonorm_bwd_k<T, FV>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)dy, (const T*)s, (const T*)gamma,
                         (const T*)dres, (T*)ds_out, (float*)workspace, rows, D, ld_dy, ld_s, ld_dres, ld_ds, ct, rps);
    else
      hipLaunchKernelGGL((nonorm_bwd_k<T, 1>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)dy, (const T*)s, (const T*)gamma,
                         (const T*)dres, (T*)ds_out, (float*)workspace, rows, D, ld_dy, ld_s, ld_dres, ld_ds, ct, rps);
    hipLaunchKernelGGL((nonorm_bwd_finish_k<T>), dim3((D + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)workspace,
                       (const T*)gamma, dgamma, dbeta, dbias, D, nslab);
  })
  MMRCA_CHECK_LAUNCH("nonorm_bwd");
  return 0;
}

extern "C" int mmrca_trigram_embed_fwd(const int32_t* ids, const int32_t* perm, const void* word, void* out, int64_t M, int B, int Tn,
                                       int E, int vocab, int dtype, void* stream) {
  MMRCA_REQUIRE(ids && word && out, "trigram_embed_fwd: null pointer");
  MMRCA_REQUIRE(B > 0 && Tn > 0 && E > 0 && vocab > 0 && (perm || M == (int64_t)B * Tn), "trigram_embed_fwd: bad shape (without perm, M must be B*T)");
  if (M <= 0) return 0;
  MMRCA_DISPATCH_DTYPE(dtype, "trigram_embed_fwd", {
    constexpr int FV = full_vec<T>();
    const bool vec = E % FV == 0 && aligned_to(word, 16) && aligned_to(out, 16);
    const int64_t n = M * 3 * (int64_t)(vec ? E / FV : E);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (vec)
      hipLaunchKernelGGL((trigram_fwd_k<T, FV>), grid, dim3(256), 0, (hipStream_t)stream, ids, perm, (const T*)word, (T*)out, M, Tn,
                         (int64_t)B * Tn, E, vocab);
    else
      hipLaunchKernelGGL((trigram_fwd_k<T, 1>), grid, dim3(256), 0, (hipStream_t)stream, ids, perm, (const T*)word, (T*)out, M, Tn,
                         (int64_t)B * Tn, E, vocab);
  })
  MMRCA_CHECK_LAUNCH("trigram_embed_fwd");
  return 0;
}

extern "C" int mmrca_trigram_embed_bwd(const void* dout, const int32_t* ids, const int32_t* perm, float* dword, int64_t M, int B,
                                       int Tn, int E, int vocab, int pad_id, int dtype, void* stream) {
  MMRCA_REQUIRE(dout && ids && dword, "trigram_embed_bwd: null pointer");
  MMRCA_REQUIRE(B > 0 && Tn > 0 && E > 0 && vocab > 0 && (perm || M == (int64_t)B * Tn), "trigram_embed_bwd: bad shape (without perm, M must be B*T)");
  if (M <= 0) return 0;
  MMRCA_DISPATCH_DTYPE(dtype, "trigram_embed_bwd", {
    constexpr int FV = full_vec<T>();
    const bool vec = E % FV == 0 && aligned_to(dout, 16);
    const int64_t n = M * 3 * (int64_t)(vec ? E / FV : E);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (vec)
      hipLaunchKernelGGL((trigram_bwd_k<T, FV>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)dout, ids, perm, dword, M, Tn,
                         (int64_t)B * Tn, E, vocab, pad_id);
    else
      hipLaunchKernelGGL((trigram_bwd_k<T, 1>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)dout, ids, perm, dword, M, Tn,
                         (int64_t)B * Tn, E, vocab, pad_id);
  })
  MMRCA_CHECK_LAUNCH("trigram_embed_bwd");
  return 0;
}
