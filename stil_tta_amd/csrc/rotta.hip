// Test-time adaptation, RoTTA (Yuan, Xie, Li, CVPR 2023, "Robust Test-Time Adaptation in Dynamic Scenarios"; definition as
// recalled: unpinned) on top of TENT (csrc/tta.hip): the category-balanced bank of test samples, its gather, the timeliness-weighted
// cross-entropy of the student against the teacher on the bank, and the teacher over A.  csrc/stil_rotta.h states the arithmetic.
//   bank_update  rows: one 256-thread workgroup per incoming row (tta_row_lse_h: lse, p, H are stil_entropy_rows' bit for bit) and the
//                first maximum; walk: ONE workgroup takes the samples in order -- a decision reads label, unc, age, occ and n as the
//                samples before it left them.  The per-slot arrays stay in global memory (a few KB, L2-resident; thread 0 writes, a
//                barrier publishes); LDS holds the reductions only.  An argmax carries (score, slot) and prefers the lower slot on
//                equal scores, so the order in which lanes meet does not matter.
//   bank_store   grid (chunk of 4096 floats, slot): the workgroups of slots nobody owns leave at once; 4 x 16 bytes per lane in
//                flight, consecutive lanes on consecutive 16 bytes; float by float when a row is not 16-byte aligned
//   rows         three launches as the selected-row losses: per row (both lse in double, ce, w -> ws), one workgroup (n, loss, counts,
//                gate), per row (dZ)
//   exchange, teacher   functors over the chunk walker of csrc/tta_common.h
// The argmax stays a reduction of its own: a (score, slot) pair needs two shuffles and two LDS arrays whoever writes them, so
// block_reduce (csrc/common.h) with a pair type would be no shorter.
#include "tta_common.h"
#include "stil_rotta.h"

struct RottaBest {
  double s;
  int i;
};
__device__ __forceinline__ RottaBest rotta_better(RottaBest a, RottaBest b) {
  return (b.s > a.s || (b.s == a.s && b.i < a.i)) ? b : a;
}
// the block's (maximal score, lowest index that reaches it) in every thread; shs / shi: >= 16 entries each
__device__ __forceinline__ RottaBest rotta_block_argmax(RottaBest v, double* shs, int* shi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    RottaBest t;
    t.s = __shfl_xor(v.s, o, 64);
    t.i = __shfl_xor(v.i, o, 64);
    v = rotta_better(v, t);
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if (l == 0) {
    shs[w] = v.s;
    shi[w] = v.i;
  }
  __syncthreads();
  RottaBest r = {shs[0], shi[0]};
  for (int i = 1; i < nw; ++i) r = rotta_better(r, RottaBest{shs[i], shi[i]});
  return r;
}

// ---- the bank's bookkeeping
__global__ __launch_bounds__(256) void rotta_update_rows_kernel(const float* __restrict__ Z, int ld, int K, double* __restrict__ lse,
                                                                 float* __restrict__ p, int ldp, float* __restrict__ H,
                                                                 int* __restrict__ yhat) {
  __shared__ float red[16];
  __shared__ double redd[16];
  __shared__ int redi[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  double L, h;
  tta_row_lse_h(zr, K, red, redd, L, h);
  RottaBest best = {-INFINITY, INT_MAX};
  for (int k = threadIdx.x; k < K; k += 256) {
    const double z = (double)zr[k];
    p[(long)r * ldp + k] = (float)exp(z - L);
    best = rotta_better(best, RottaBest{z, k});
  }
  best = rotta_block_argmax(best, redd, redi);
  if (threadIdx.x == 0) {
    lse[r] = L;
    H[r] = (float)h;
    yhat[r] = best.i < K ? best.i : 0;  // a row of NaNs has no maximum: class 0
  }
}

// label, unc, age, occ, n_io, owner carry no __restrict__: thread 0 writes them, a barrier publishes, every thread reads them back
__global__ __launch_bounds__(256) void rotta_walk_kernel(const float* __restrict__ H, const int* __restrict__ yhat, int B, int K, int N,
                                                          double lt, double lu, int* label, float* unc, int* age, int* occ, int* n_io,
                                                          int* owner, unsigned char* __restrict__ accepted, int* __restrict__ slot_of,
                                                          int* __restrict__ counts) {
  __shared__ double shs[16];
  __shared__ int shi[16];
  const int tid = threadIdx.x;
  for (int i = tid; i < N; i += 256) owner[i] = -1;
  int n = min(max(n_io[0], 0), N);  // read by every thread; written by thread 0 after the last barrier only
  const double lnK = log((double)K), dN = (double)N;
  int n_acc = 0, n_evict = 0;
  __syncthreads();
  for (int b = 0; b < B; ++b) {
    const int c = yhat[b];
    const float uf = H[b];
    const double s_new = 0.5 * lt + (K > 1 ? lu * (double)uf / lnK : 0.0);
    int slot = -1;
    bool filled = false;
    if (c >= 0 && c < K) {  // uniform across the block, as everything that follows
      const bool minority = (long)occ[c] * K < N;
      if (minority && n < N) {
        slot = n;
      } else {
        int mo = 0;
        if (minority) {
          for (int k = tid; k < K; k += 256) mo = max(mo, occ[k]);
          mo = block_reduce(mo, shi, [](int a, int b) { return max(a, b); });
        }
        RottaBest best = {-INFINITY, INT_MAX};
        for (int i = tid; i < n; i += 256) {
          const int li = label[i];
          const bool cand = minority ? (li >= 0 && li < K && occ[li] == mo) : (li == c);
          if (cand) {
            const double sc = lt / (1.0 + exp(-(double)age[i] / dN)) + (K > 1 ? lu * (double)unc[i] / lnK : 0.0);
            best = rotta_better(best, RottaBest{sc, i});
          }
        }
        best = rotta_block_argmax(best, shs, shi);
        if (best.i < n && best.s > s_new) {
          slot = best.i;
          filled = true;
        }
      }
    }
    __syncthreads();  // every read of this sample's decision is done before thread 0 writes
    if (slot >= 0) {
      if (tid == 0) {
        if (filled) {
          const int old = label[slot];
          if (old >= 0 && old < K) occ[old] -= 1;
        }
        label[slot] = c;
        unc[slot] = uf;
        age[slot] = 0;
        occ[c] += 1;
        owner[slot] = b;
      }
      if (filled) ++n_evict; else ++n;
      ++n_acc;
    }
    if (tid == 0) {
      accepted[b] = (unsigned char)(slot >= 0);
      slot_of[b] = slot;
    }
    __syncthreads();  // the accept is in place before the ages move
    for (int i = tid; i < n; i += 256) {
      const int a = age[i];
      if (a < INT_MAX) age[i] = a + 1;
    }
    __syncthreads();
  }
  if (tid == 0) {
    n_io[0] = n;
    counts[0] = n_acc;
    counts[1] = n_evict;
    counts[2] = n;
    counts[3] = 0;
  }
}

static inline bool rotta_lambda_ok(float v) { return v >= 0.0f && v <= 3.402823466e38f; }  // false for NaN

extern "C" int stil_rotta_bank_update(const float* Zt, int ld, int B, int K, int N, float lambda_t, float lambda_u, int* label, float* unc,
                                      int* age, int* occ, int* n, int* owner, double* lse, float* p, int ldp, float* H, int* yhat,
                                      unsigned char* accepted, int* slot_of, int* counts, void* stream) {
  STIL_REQUIRE(Zt && label && unc && age && occ && n && owner && lse && p && H && yhat && accepted && slot_of && counts,
               "stil_rotta_bank_update: null pointer");
  STIL_REQUIRE(B >= 1 && K >= 1 && N >= 1 && ld >= K && ldp >= K, "stil_rotta_bank_update: bad shape B=%d K=%d N=%d ld=%d ldp=%d", B, K, N, ld, ldp);
  STIL_REQUIRE(N <= STIL_ROTTA_MAX_SLOTS && K <= STIL_ROTTA_MAX_CLASSES, "stil_rotta_bank_update: N=%d K=%d beyond the bounds %d slots, %d classes", N, K,
               STIL_ROTTA_MAX_SLOTS, STIL_ROTTA_MAX_CLASSES);
  STIL_REQUIRE(rotta_lambda_ok(lambda_t) && rotta_lambda_ok(lambda_u), "stil_rotta_bank_update: lambda_t=%g lambda_u=%g must be finite and >= 0",
               (double)lambda_t, (double)lambda_u);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rotta_update_rows_kernel, dim3(B), dim3(256), 0, s, Zt, ld, K, lse, p, ldp, H, yhat);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(rotta_walk_kernel, dim3(1), dim3(256), 0, s, (const float*)H, (const int*)yhat, B, K, N, (double)lambda_t,
                     (double)lambda_u, label, unc, age, occ, n, owner, accepted, slot_of, counts);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

// ---- the gather into the bank
#define ROTTA_STORE_CHUNK 4096  // floats per workgroup: 256 lanes x 4 x 16 bytes
__global__ __launch_bounds__(256) void rotta_store_kernel(const float* __restrict__ x_img, const float* __restrict__ x_tab,
                                                           const int* __restrict__ owner, int B, long img_floats, int tab_floats,
                                                           int img_chunks, int vec_img, int vec_tab, float* __restrict__ bank_img,
                                                           float* __restrict__ bank_tab) {
  const int s = blockIdx.y;
  const int o = owner[s];
  if (o < 0 || o >= B) return;  // uniform across the block: the slot keeps its content
  int ch = blockIdx.x;
  const float* src;
  float* dst;
  long len;
  int vec;
  if (ch < img_chunks) {
    src = x_img + (long)o * img_floats;
    dst = bank_img + (long)s * img_floats;
    len = img_floats;
    vec = vec_img;
  } else {
    ch -= img_chunks;
    src = x_tab + (long)o * tab_floats;
    dst = bank_tab + (long)s * tab_floats;
    len = tab_floats;
    vec = vec_tab;
  }
  const long lo = (long)ch * ROTTA_STORE_CHUNK;
  const long hi = min(lo + ROTTA_STORE_CHUNK, len);
  if (vec) {  // len % 4 == 0 and both bases 16-byte aligned: so is every row and every chunk of it
    const float4* s4 = reinterpret_cast<const float4*>(src + lo);
    float4* d4 = reinterpret_cast<float4*>(dst + lo);
    const int n4 = (int)((hi - lo) >> 2);
    float4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = q * 256 + threadIdx.x;
      if (i < n4) v[q] = s4[i];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = q * 256 + threadIdx.x;
      if (i < n4) d4[i] = v[q];
    }
  } else {
    for (long i = lo + threadIdx.x; i < hi; i += 256) dst[i] = src[i];
  }
}

extern "C" int stil_rotta_bank_store(const float* x_img, const float* x_tab, const int* owner, int N, int B, long img_floats, int tab_floats,
                                     float* bank_img, float* bank_tab, void* stream) {
  STIL_REQUIRE(x_img && x_tab && owner && bank_img && bank_tab, "stil_rotta_bank_store: null pointer");
  STIL_REQUIRE(N >= 1 && N <= STIL_ROTTA_MAX_SLOTS && B >= 1, "stil_rotta_bank_store: N=%d must lie in [1, %d], B=%d >= 1", N, STIL_ROTTA_MAX_SLOTS, B);
  STIL_REQUIRE(img_floats >= 1 && tab_floats >= 1 && img_floats <= (long)INT_MAX, "stil_rotta_bank_store: img_floats=%ld tab_floats=%d",
               img_floats, tab_floats);
  const int vec_img = img_floats % 4 == 0 && (uintptr_t)x_img % 16 == 0 && (uintptr_t)bank_img % 16 == 0;
  const int vec_tab = tab_floats % 4 == 0 && (uintptr_t)x_tab % 16 == 0 && (uintptr_t)bank_tab % 16 == 0;
  const int img_chunks = cdiv(img_floats, ROTTA_STORE_CHUNK), tab_chunks = cdiv(tab_floats, ROTTA_STORE_CHUNK);
  hipLaunchKernelGGL(rotta_store_kernel, dim3(img_chunks + tab_chunks, N), dim3(256), 0, (hipStream_t)stream, x_img, x_tab, owner, B,
                     img_floats, tab_floats, img_chunks, vec_img, vec_tab, bank_img, bank_tab);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

// ---- the loss on the bank
__device__ __forceinline__ double rotta_row_lse(const float* __restrict__ zr, int K, float* red, double* redd) {
  float m = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) m = fmaxf(m, zr[k]);
  m = block_max(m, red);
  double s = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) s += exp((double)zr[k] - (double)m);
  s = block_sum_d(s, redd);
  return (double)m + log(s);
}

// ws (doubles): lse of the student [rows] | lse of the teacher [rows] | w [rows] | ce [rows]
__global__ __launch_bounds__(256) void rotta_rows_kernel(const float* __restrict__ Zs, int lds, const float* __restrict__ Zt, int ldt,
                                                          const int* __restrict__ label, const int* __restrict__ age, int rows, int K,
                                                          float* __restrict__ ce, float* __restrict__ w, double* __restrict__ ws) {
  __shared__ float red[16];
  __shared__ double redd[16];
  const int r = blockIdx.x;
  if (label[r] < 0) {  // uniform across the block: an empty slot
    if (threadIdx.x == 0) {
      ce[r] = 0.f;
      w[r] = 0.f;
      ws[r] = ws[rows + r] = ws[2 * (long)rows + r] = ws[3 * (long)rows + r] = 0.0;
    }
    return;
  }
  const float* zs = Zs + (long)r * lds;
  const float* zt = Zt + (long)r * ldt;
  const double Ls = rotta_row_lse(zs, K, red, redd), Lt = rotta_row_lse(zt, K, red, redd);
  double a = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) a -= exp((double)zt[k] - Lt) * ((double)zs[k] - Ls);
  a = block_sum_d(a, redd);
  if (threadIdx.x == 0) {
    const double e = exp(-(double)age[r] / (double)rows);
    const double wi = e / (1.0 + e);
    ce[r] = (float)a;
    w[r] = (float)wi;
    ws[r] = Ls;
    ws[rows + r] = Lt;
    ws[2 * (long)rows + r] = wi;
    ws[3 * (long)rows + r] = a;
  }
}

__global__ __launch_bounds__(256) void rotta_reduce_kernel(const int* __restrict__ label, int rows, const double* __restrict__ ws,
                                                            int* __restrict__ counts, float* __restrict__ loss,
                                                            const unsigned char* __restrict__ active,
                                                            unsigned char* __restrict__ active_out, int n_tensors) {
  __shared__ double redd[16];
  double nv = 0.0, s = 0.0;
  for (int i = threadIdx.x; i < rows; i += 256)
    if (label[i] >= 0) {
      nv += 1.0;
      s += ws[2 * (long)rows + i] * ws[3 * (long)rows + i];
    }
  nv = block_sum_d(nv, redd);  // integers below 2^53: exact
  s = block_sum_d(s, redd);
  const int n = (int)nv;
  if (threadIdx.x == 0) {
    counts[0] = n;
    counts[1] = rows;
    counts[2] = 0;
    counts[3] = 0;
    loss[0] = n > 0 ? (float)(s / nv) : 0.f;
  }
  tta_gate(active, active_out, n_tensors, n);
}

__global__ __launch_bounds__(256) void rotta_dz_kernel(const float* __restrict__ Zs, int lds, const float* __restrict__ Zt, int ldt,
                                                        const int* __restrict__ label, int rows, int K, double gscale,
                                                        const double* __restrict__ ws, const int* __restrict__ counts,
                                                        float* __restrict__ dZ, int ldd) {
  const int r = blockIdx.x;
  const int n = counts[0];
  float* dr = dZ + (long)r * ldd;
  if (n <= 0 || label[r] < 0) {  // uniform across the block
    for (int k = threadIdx.x; k < K; k += 256) dr[k] = 0.f;
    return;
  }
  const float* zs = Zs + (long)r * lds;
  const float* zt = Zt + (long)r * ldt;
  const double Ls = ws[r], Lt = ws[rows + r];
  const double f = gscale * ws[2 * (long)rows + r] / (double)n;
  for (int k = threadIdx.x; k < K; k += 256) dr[k] = (float)(f * (exp((double)zs[k] - Ls) - exp((double)zt[k] - Lt)));
}

extern "C" int stil_rotta_rows(const float* Zs, int lds, const float* Zt, int ldt, const int* label, const int* age, int rows, int K,
                               float grad_scale, float* ce, float* w, float* dZ, int ldd, int* counts, float* loss,
                               const unsigned char* active, unsigned char* active_out, int n_tensors, double* ws, void* stream) {
  STIL_REQUIRE(Zs && Zt && label && age && ce && w && dZ && counts && loss && ws, "stil_rotta_rows: null pointer");
  STIL_REQUIRE(rows >= 1 && K >= 1 && lds >= K && ldt >= K && ldd >= K, "stil_rotta_rows: bad shape rows=%d K=%d lds=%d ldt=%d ldd=%d", rows,
               K, lds, ldt, ldd);
  STIL_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (active && active_out)), "stil_rotta_rows: n_tensors=%d needs both masks", n_tensors);
  STIL_REQUIRE(grad_scale >= -3.402823466e38f && grad_scale <= 3.402823466e38f, "stil_rotta_rows: grad_scale=%g is not finite", (double)grad_scale);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rotta_rows_kernel, dim3(rows), dim3(256), 0, s, Zs, lds, Zt, ldt, label, age, rows, K, ce, w, ws);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(rotta_reduce_kernel, dim3(1), dim3(256), 0, s, label, rows, (const double*)ws, counts, loss, active, active_out, n_tensors);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(rotta_dz_kernel, dim3(rows), dim3(256), 0, s, Zs, lds, Zt, ldt, label, rows, K, (double)grad_scale, (const double*)ws,
                     (const int*)counts, dZ, ldd);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

// ---- the teacher over A's chunks
struct RottaExchange {  // A <-> teacher
  float4* __restrict__ params; float4* __restrict__ teacher;
  __device__ void operator()(long i, long ic) const {
    const float4 a = params[i];
    const float4 t = teacher[ic];
    params[i] = t;
    teacher[ic] = a;
  }
};

struct RottaTeacher {  // teacher <- (1 - nu) teacher + nu A
  const float4* __restrict__ params; float4* __restrict__ teacher; double nu;
  __device__ void operator()(long i, long ic) const {
    const float4 a = params[i];
    float4 t = teacher[ic];
    const double n1 = 1.0 - nu;
    t.x = (float)(n1 * (double)t.x + nu * (double)a.x);
    t.y = (float)(n1 * (double)t.y + nu * (double)a.y);
    t.z = (float)(n1 * (double)t.z + nu * (double)a.z);
    t.w = (float)(n1 * (double)t.w + nu * (double)a.w);
    teacher[ic] = t;
  }
};

extern "C" int stil_rotta_exchange(float* params, float* teacher, const int* achunks, int n_achunks, const int* chunk2tensor,
                                   const unsigned char* active, int n_tensors, long n, void* stream) {
  const TtaChunks c = {achunks, n_achunks, chunk2tensor, active, n_tensors, n / 1024};
  if (int rc = tta_slab_check("stil_rotta_exchange", c, n, {params, teacher})) return rc;
  if (n_achunks == 0) return STIL_OK;
  hipLaunchKernelGGL(tta_chunk_kernel<RottaExchange>, dim3(n_achunks), dim3(256), 0, (hipStream_t)stream, c,
                     RottaExchange{(float4*)params, (float4*)teacher});
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_rotta_teacher(const float* params, float* teacher, const int* achunks, int n_achunks, const int* chunk2tensor,
                                  const unsigned char* active, int n_tensors, long n, float nu, void* stream) {
  const TtaChunks c = {achunks, n_achunks, chunk2tensor, active, n_tensors, n / 1024};
  if (int rc = tta_slab_check("stil_rotta_teacher", c, n, {params, teacher})) return rc;
  STIL_REQUIRE(nu >= 0.0f && nu <= 1.0f, "stil_rotta_teacher: nu=%g is not inside [0, 1]", (double)nu);
  if (n_achunks == 0 || nu == 0.0f) return STIL_OK;
  hipLaunchKernelGGL(tta_chunk_kernel<RottaTeacher>, dim3(n_achunks), dim3(256), 0, (hipStream_t)stream, c,
                     RottaTeacher{(const float4*)params, (float4*)teacher, (double)nu});
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
