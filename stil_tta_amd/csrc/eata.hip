// Test-time adaptation, EATA (Niu et al., ICML 2022, "Efficient Test-Time Model Adaptation without Forgetting") on top of
// TENT (csrc/tta.hip): a reliable / non-redundant sample selection with per-sample weights, and a Fisher-weighted anchor
// of the adapted set A to its source values.  Per row r of Z [rows, K], with m [K] the running mean of the selected
// predictions (valid flag *m_valid), E0 = e_margin, d = d_margin, mu = momentum:
//   lse_r, p_rk, H_r                as stil_entropy_rows (tta_row_lse_h of csrc/tta_common.h: bit-identical)
//   c_r   = <m, p_r> / (max(|m|, 1e-8) max(|p_r|, 1e-8))     (m as it stood before the call; 0 while m is invalid)
//   rel_r = H_r < E0 ; sel_r = rel_r and (m invalid or |c_r| < d) ; w_r = exp(E0 - H_r)
//   n = sum sel, n_reliable = sum rel, L = (1/n) sum sel w H   (0 when n == 0)
//   m' = pbar (m invalid) | mu m + (1 - mu) pbar, pbar = (1/n) sum sel p ; untouched when n == 0
//   active_out[t] = active[t] and n > 0                        (the gate of the Adam step: n never leaves the device)
//   dZ_rk = sel_r w_r (-p_rk (log p_rk + H_r)) grad_scale / n  (0 when n == 0)
// Everything is formed in double and rounded once; reductions are wave64 shuffle trees plus a fixed-order sum of the wave
// partials or fixed-order loops; no float atomics: bit-identical on repetition.  Three launches: rows, reduce, dZ (tta_sel_dz_kernel of
// csrc/tta_common.h, which reads the double lse and H of the first back).
// The two slab kernels are functors over the chunk walker of csrc/tta_common.h (TtaChunks, which states the rule for the entries of
// `achunks`); Fisher estimate and source values are compact.
#include "tta_common.h"

__global__ __launch_bounds__(256) void eata_rows_kernel(const float* __restrict__ Z, int ld, int K, double e0, double dm,
                                                         const float* __restrict__ m, const int* __restrict__ m_valid,
                                                         double* __restrict__ lse, double* __restrict__ Hd,
                                                         float* __restrict__ p, int ldp, float* __restrict__ H,
                                                         float* __restrict__ c, float* __restrict__ w,
                                                         unsigned char* __restrict__ rel, unsigned char* __restrict__ sel,
                                                         int* __restrict__ counts) {
  __shared__ float red[16];
  __shared__ double redd[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  double L, h;
  tta_row_lse_h(zr, K, red, redd, L, h);
  const int valid = m_valid[0] != 0;
  double mp = 0.0, mm = 0.0, pp = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const double pk = exp((double)zr[k] - L);
    p[(long)r * ldp + k] = (float)pk;
    if (valid) {
      const double mk = (double)m[k];
      mp += mk * pk;
      mm += mk * mk;
    }
    pp += pk * pk;
  }
  double cos = 0.0;
  if (valid) {  // uniform across the block
    mp = block_sum_d(mp, redd);
    mm = block_sum_d(mm, redd);
    pp = block_sum_d(pp, redd);
    cos = mp / (fmax(sqrt(mm), 1e-8) * fmax(sqrt(pp), 1e-8));
  }
  if (threadIdx.x == 0) {
    const int is_rel = h < e0;
    lse[r] = L;
    Hd[r] = h;  // the dZ kernel reads the double H back: no second reduction
    H[r] = (float)h;
    c[r] = (float)cos;
    w[r] = (float)exp(e0 - h);
    rel[r] = (unsigned char)is_rel;
    sel[r] = (unsigned char)(is_rel && (!valid || fabs(cos) < dm));
    if (r == 0) counts[2] = valid;  // m's validity before this call: the reduce kernel's blocks read it while block 0 sets m_valid
  }
}

// grid = cdiv(K, 256): every block forms the sums itself (rows bytes), block 0 writes the scalars and the gate
__global__ __launch_bounds__(256) void eata_reduce_kernel(const float* __restrict__ p, int ldp, int rows, int K,
                                                           const float* __restrict__ H, const float* __restrict__ w,
                                                           const unsigned char* __restrict__ rel,
                                                           const unsigned char* __restrict__ sel, double mu,
                                                           float* __restrict__ m, int* __restrict__ m_valid,
                                                           int* __restrict__ counts, float* __restrict__ loss,
                                                           const unsigned char* __restrict__ active,
                                                           unsigned char* __restrict__ active_out, int n_tensors) {
  __shared__ double redd[16];
  const TtaSelSums sums = tta_sel_sums(rows, H, w, rel, sel, redd);
  const int n = (int)sums.n;
  const int valid = counts[2];
  if (n > 0) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < K) {
      double s = 0.0;
      for (int r = 0; r < rows; ++r)
        if (sel[r]) s += (double)p[(long)r * ldp + k];  // fixed order
      s /= sums.n;
      m[k] = (float)(valid ? mu * (double)m[k] + (1.0 - mu) * s : s);
    }
  }
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0) {
    counts[0] = n;
    counts[1] = (int)sums.n_rel;
    loss[0] = n > 0 ? (float)(sums.wh / sums.n) : 0.f;
    if (n > 0) m_valid[0] = 1;
  }
  tta_gate(active, active_out, n_tensors, n);
}

extern "C" int stil_eata_rows(const float* Z, int ld, int rows, int K, float e_margin, float d_margin, float momentum,
                              float grad_scale, float* m, int* m_valid, double* lse, double* Hd, float* p, int ldp, float* H,
                              float* c, float* w, unsigned char* rel, unsigned char* sel, float* dZ, int ldd, int* counts, float* loss,
                              const unsigned char* active, unsigned char* active_out, int n_tensors, void* stream) {
  STIL_REQUIRE(Z && m && m_valid && lse && Hd && p && H && c && w && rel && sel && dZ && counts && loss, "stil_eata_rows: null pointer");
  STIL_REQUIRE(rows >= 1 && K >= 1 && ld >= K, "stil_eata_rows: bad shape rows=%d K=%d ld=%d", rows, K, ld);
  STIL_REQUIRE(ldp >= K && ldd >= K, "stil_eata_rows: ldp=%d ldd=%d < K=%d", ldp, ldd, K);
  STIL_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (active && active_out)), "stil_eata_rows: n_tensors=%d needs both masks", n_tensors);
  STIL_REQUIRE(momentum >= 0.f && momentum <= 1.f && d_margin >= 0.f, "stil_eata_rows: momentum=%g d_margin=%g", (double)momentum, (double)d_margin);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(eata_rows_kernel, dim3(rows), dim3(256), 0, s, Z, ld, K, (double)e_margin, (double)d_margin, (const float*)m,
                     (const int*)m_valid, lse, Hd, p, ldp, H, c, w, rel, sel, counts);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(eata_reduce_kernel, dim3(cdiv(K, 256)), dim3(256), 0, s, (const float*)p, ldp, rows, K, (const float*)H,
                     (const float*)w, (const unsigned char*)rel, (const unsigned char*)sel, (double)momentum, m, m_valid, counts,
                     loss, active, active_out, n_tensors);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(tta_sel_dz_kernel<TtaWeightMargin>, dim3(rows), dim3(256), 0, s, Z, ld, K, TtaWeightMargin{(double)e_margin}, (double)grad_scale,
                     (const double*)lse, (const double*)Hd, (const unsigned char*)sel, (const int*)counts, dZ, ldd);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

// ---- the Fisher anchor and the Fisher accumulation over A's chunks
struct EataAnchor {  // grads += 2 alpha F (theta - theta0) -> the chunk's share of sum F (theta - theta0)^2
  const float4* __restrict__ params; const float4* __restrict__ theta0; const float4* __restrict__ fisher;
  float4* __restrict__ grads; double alpha;
  __device__ double operator()(long i, long ic) const {
    const float4 th = params[i];
    const float4 t0 = theta0[ic];
    const float4 ff = fisher[ic];
    float4 gg = grads[i];
    double s = 0.0;
#define ANCHOR1(T, T0, F, G)                                      \
  {                                                               \
    const double d = (double)T - (double)T0, fd = (double)F * d;  \
    s += fd * d;                                                  \
    G = (float)((double)G + 2.0 * alpha * fd);                    \
  }
    ANCHOR1(th.x, t0.x, ff.x, gg.x) ANCHOR1(th.y, t0.y, ff.y, gg.y) ANCHOR1(th.z, t0.z, ff.z, gg.z) ANCHOR1(th.w, t0.w, ff.w, gg.w)
#undef ANCHOR1
    grads[i] = gg;
    return s;
  }
};

__global__ __launch_bounds__(256) void eata_anchor_sum_kernel(const double* __restrict__ partial, int n, double alpha,
                                                               float* __restrict__ R) {
  __shared__ double redd[16];
  const double s = tta_partial_sum(partial, n, redd);
  if (threadIdx.x == 0) R[0] = (float)(alpha * s);
}

struct EataFisher {  // F += g^2 scale
  float4* __restrict__ fisher; const float4* __restrict__ grads; double scale;
  __device__ void operator()(long i, long ic) const {
    const float4 gg = grads[i];
    float4 ff = fisher[ic];
    ff.x = (float)((double)ff.x + (double)gg.x * (double)gg.x * scale);
    ff.y = (float)((double)ff.y + (double)gg.y * (double)gg.y * scale);
    ff.z = (float)((double)ff.z + (double)gg.z * (double)gg.z * scale);
    ff.w = (float)((double)ff.w + (double)gg.w * (double)gg.w * scale);
    fisher[ic] = ff;
  }
};

extern "C" int stil_eata_anchor(const float* params, const float* theta0, const float* fisher, float* grads, const int* achunks,
                                int n_achunks, const int* chunk2tensor, const unsigned char* active, int n_tensors, long n,
                                float alpha, double* partial, float* R, void* stream) {
  const TtaChunks c = {achunks, n_achunks, chunk2tensor, active, n_tensors, n / 1024};
  if (int rc = tta_slab_check("stil_eata_anchor", c, n, {params, theta0, fisher, grads}, {partial, R})) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (n_achunks > 0) {
    hipLaunchKernelGGL(tta_chunk_sum_kernel<EataAnchor>, dim3(n_achunks), dim3(256), 0, s, c,
                       EataAnchor{(const float4*)params, (const float4*)theta0, (const float4*)fisher, (float4*)grads, (double)alpha}, partial);
    STIL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(eata_anchor_sum_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, n_achunks, (double)alpha, R);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_eata_fisher_accum(float* fisher, const float* grads, const int* achunks, int n_achunks, const int* chunk2tensor,
                                      const unsigned char* active, int n_tensors, long n, float scale, void* stream) {
  const TtaChunks c = {achunks, n_achunks, chunk2tensor, active, n_tensors, n / 1024};
  if (int rc = tta_slab_check("stil_eata_fisher_accum", c, n, {fisher, grads})) return rc;
  if (n_achunks == 0) return STIL_OK;
  hipLaunchKernelGGL(tta_chunk_kernel<EataFisher>, dim3(n_achunks), dim3(256), 0, (hipStream_t)stream, c,
                     EataFisher{(float4*)fisher, (const float4*)grads, (double)scale});
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
