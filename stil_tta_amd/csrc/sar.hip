// Test-time adaptation, SAR (Niu et al., ICLR 2023, "Towards Stable Test-Time Adaptation in Dynamic Wild World") on top of
// TENT (csrc/tta.hip) and beside EATA (csrc/eata.hip): the entropy of the reliable rows, minimised at the adversarially
// perturbed point theta + rho g / |g|, and a model-recovery rule on a running mean of the loss.  Per row r of Z [rows, K],
// with E0 = margin and prior_r the selection of an earlier pass (all ones when there is none):
//   lse_r, p_rk, H_r                as stil_entropy_rows (tta_row_lse_h of csrc/tta_common.h: bit-identical)
//   sel_r = prior_r and H_r < E0 ; n = sum sel ; L = (1/n) sum sel H   (0 when n == 0; no weights)
//   active_out[t] = active[t] and n > 0                        (the gate of the Adam step: n never leaves the device)
//   dZ_rk = sel_r (-p_rk (log p_rk + H_r)) grad_scale / n      (0 when n == 0)
//   second pass: ema <- L | mu ema + (1 - mu) L when n > 0 ; recover = reset > 0 and ema held and ema < reset
// Everything is formed in double and rounded once; reductions are wave64 shuffle trees plus a fixed-order sum of the wave
// partials or fixed-order loops; no float atomics: bit-identical on repetition.  Three launches: rows, reduce, dZ
// (tta_sel_dz_kernel of csrc/tta_common.h with weight 1, which reads the double lse and H of the first back).
// The slab kernels walk A's chunks as csrc/tta_common.h lays down (TtaChunks, which states the rule for the entries of `achunks`):
// the square norm and the restore are functors over its kernel templates, perturb and recover are kernels of their own on its
// helper.  Saved values, the perturbation and the source values are compact.  What one block hands to another crosses a launch boundary.
#include "tta_common.h"

__global__ __launch_bounds__(256) void sar_rows_kernel(const float* __restrict__ Z, int ld, int K, double e0,
                                                        const unsigned char* __restrict__ prior, double* __restrict__ lse,
                                                        double* __restrict__ Hd, float* __restrict__ p, int ldp,
                                                        float* __restrict__ H, unsigned char* __restrict__ sel) {
  __shared__ float red[16];
  __shared__ double redd[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  double L, h;
  tta_row_lse_h(zr, K, red, redd, L, h);
  for (int k = threadIdx.x; k < K; k += 256) p[(long)r * ldp + k] = (float)exp((double)zr[k] - L);
  if (threadIdx.x == 0) {
    lse[r] = L;
    Hd[r] = h;  // the reduce and dZ kernels read the double H back: no second reduction, the same decision
    H[r] = (float)h;
    sel[r] = (unsigned char)((!prior || prior[r]) && h < e0);
  }
}

// one block: the counts, the loss, the gate, and (second pass) the running mean of the loss and the recovery flag
__global__ __launch_bounds__(256) void sar_reduce_kernel(int rows, double e0, const double* __restrict__ Hd,
                                                          const unsigned char* __restrict__ prior,
                                                          const unsigned char* __restrict__ sel, int* __restrict__ counts,
                                                          float* __restrict__ loss, const unsigned char* __restrict__ active,
                                                          unsigned char* __restrict__ active_out, int n_tensors,
                                                          float* __restrict__ ema, int* __restrict__ ema_valid, double mu,
                                                          double reset, int* __restrict__ recover) {
  __shared__ double redd[16];
  double nd = 0.0, nr = 0.0, np = 0.0, ls = 0.0;
  for (int i = threadIdx.x; i < rows; i += 256) {
    const double h = Hd[i];
    if (sel[i]) {
      nd += 1.0;
      ls += h;
    }
    if (h < e0) nr += 1.0;
    if (!prior || prior[i]) np += 1.0;
  }
  nd = block_sum_d(nd, redd);  // integers below 2^53: exact
  nr = block_sum_d(nr, redd);
  np = block_sum_d(np, redd);
  ls = block_sum_d(ls, redd);
  const int n = (int)nd;
  if (threadIdx.x == 0) {
    const double l = n > 0 ? ls / nd : 0.0;
    counts[0] = n;
    counts[1] = (int)nr;
    counts[2] = (int)np;
    counts[3] = 0;
    loss[0] = (float)l;
    if (ema) {
      int valid = ema_valid[0] != 0;
      float e = ema[0];
      if (n > 0) {
        e = (float)(valid ? mu * (double)e + (1.0 - mu) * l : l);
        valid = 1;
        ema[0] = e;
        ema_valid[0] = 1;
      }
      recover[0] = (reset > 0.0 && valid && (double)e < reset) ? 1 : 0;  // on the float the state holds
    }
  }
  tta_gate(active, active_out, n_tensors, n);
}

extern "C" int stil_sar_rows(const float* Z, int ld, int rows, int K, float margin, float grad_scale, const unsigned char* prior_sel,
                             double* lse, double* Hd, float* p, int ldp, float* H, unsigned char* sel, float* dZ, int ldd, int* counts,
                             float* loss, const unsigned char* active, unsigned char* active_out, int n_tensors, float* ema,
                             int* ema_valid, float momentum, float reset, int* recover, void* stream) {
  STIL_REQUIRE(Z && lse && Hd && p && H && sel && dZ && counts && loss, "stil_sar_rows: null pointer");
  STIL_REQUIRE(rows >= 1 && K >= 1 && ld >= K, "stil_sar_rows: bad shape rows=%d K=%d ld=%d", rows, K, ld);
  STIL_REQUIRE(ldp >= K && ldd >= K, "stil_sar_rows: ldp=%d ldd=%d < K=%d", ldp, ldd, K);
  STIL_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (active && active_out)), "stil_sar_rows: n_tensors=%d needs both masks", n_tensors);
  STIL_REQUIRE(!ema || (ema_valid && recover), "stil_sar_rows: ema needs ema_valid and recover");
  STIL_REQUIRE(!ema || (momentum >= 0.f && momentum <= 1.f && reset == reset), "stil_sar_rows: momentum=%g reset=%g", (double)momentum, (double)reset);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sar_rows_kernel, dim3(rows), dim3(256), 0, s, Z, ld, K, (double)margin, prior_sel, lse, Hd, p, ldp, H, sel);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(sar_reduce_kernel, dim3(1), dim3(256), 0, s, rows, (double)margin, (const double*)Hd, prior_sel,
                     (const unsigned char*)sel, counts, loss, active, active_out, n_tensors, ema, ema_valid, (double)momentum,
                     (double)reset, recover);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(tta_sel_dz_kernel<TtaWeightOne>, dim3(rows), dim3(256), 0, s, Z, ld, K, TtaWeightOne{}, (double)grad_scale,
                     (const double*)lse, (const double*)Hd, (const unsigned char*)sel, (const int*)counts, dZ, ldd);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

// ---- the slab kernels
struct SarSqnorm {  // the chunk's share of |g|^2
  const float4* __restrict__ grads;
  __device__ double operator()(long i, long) const {
    const float4 g = grads[i];
    return (double)g.x * (double)g.x + (double)g.y * (double)g.y + (double)g.z * (double)g.z + (double)g.w * (double)g.w;
  }
};

// every block sums the partials itself, in the same fixed order: the norm is one value for all of them
__global__ __launch_bounds__(256) void sar_perturb_kernel(TtaChunks c, float* __restrict__ params, const float* __restrict__ grads,
                                                           float* __restrict__ saved, float* __restrict__ e, double rho,
                                                           const double* __restrict__ partial, double* __restrict__ norm) {
  __shared__ double redd[16];
  const double nrm = sqrt(tta_partial_sum(partial, c.n_achunks, redd));
  const int j = blockIdx.x;
  if (j == 0 && threadIdx.x == 0) norm[0] = nrm;
  long i, ic;
  if (!c.at(j, i, ic)) return;
  const double f = rho / (nrm + 1e-12);
  const float4 g = reinterpret_cast<const float4*>(grads)[i];
  float4 th = reinterpret_cast<float4*>(params)[i];
  reinterpret_cast<float4*>(saved)[ic] = th;
  float4 d;
  d.x = (float)((double)g.x * f);
  d.y = (float)((double)g.y * f);
  d.z = (float)((double)g.z * f);
  d.w = (float)((double)g.w * f);
  reinterpret_cast<float4*>(e)[ic] = d;
  th.x += d.x;
  th.y += d.y;
  th.z += d.z;
  th.w += d.w;
  reinterpret_cast<float4*>(params)[i] = th;
}

__global__ void sar_zero_norm_kernel(double* __restrict__ norm) {  // an empty A: no gradient, no perturbation
  if (threadIdx.x == 0) norm[0] = 0.0;
}

struct SarRestore {  // A <- saved
  float4* __restrict__ params; const float4* __restrict__ saved;
  __device__ void operator()(long i, long ic) const { params[i] = saved[ic]; }
};

// grid = n_achunks + 1: the last block clears the step counts and the validity of the running mean
__global__ __launch_bounds__(256) void sar_recover_kernel(TtaChunks c, float* __restrict__ params, const float* __restrict__ theta0,
                                                           float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                           int* __restrict__ steps, const int* __restrict__ recover,
                                                           int* __restrict__ ema_valid) {
  if (recover[0] == 0) return;  // uniform across the grid
  const int j = blockIdx.x;
  if (j == c.n_achunks) {
    for (int t = threadIdx.x; t < c.n_tensors; t += 256)
      if (c.active[t]) steps[t] = 0;
    if (threadIdx.x == 0) ema_valid[0] = 0;
    return;
  }
  long i, ic;
  if (!c.at(j, i, ic)) return;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  reinterpret_cast<float4*>(params)[i] = reinterpret_cast<const float4*>(theta0)[ic];
  reinterpret_cast<float4*>(exp_avg)[i] = zero;
  reinterpret_cast<float4*>(exp_avg_sq)[i] = zero;
}

extern "C" int stil_sar_perturb(float* params, const float* grads, float* saved, float* e, const int* achunks, int n_achunks,
                                const int* chunk2tensor, const unsigned char* active, int n_tensors, long n, float rho, double* partial,
                                double* norm, void* stream) {
  const TtaChunks c = {achunks, n_achunks, chunk2tensor, active, n_tensors, n / 1024};
  if (int rc = tta_slab_check("stil_sar_perturb", c, n, {params, grads, saved, e}, {partial, norm})) return rc;
  STIL_REQUIRE(rho >= 0.f && rho <= 3.0e38f, "stil_sar_perturb: rho=%g must be a finite number >= 0", (double)rho);
  hipStream_t s = (hipStream_t)stream;
  if (n_achunks == 0) {
    hipLaunchKernelGGL(sar_zero_norm_kernel, dim3(1), dim3(64), 0, s, norm);
    STIL_LAUNCH_CHECK();
    return STIL_OK;
  }
  hipLaunchKernelGGL(tta_chunk_sum_kernel<SarSqnorm>, dim3(n_achunks), dim3(256), 0, s, c, SarSqnorm{(const float4*)grads}, partial);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(sar_perturb_kernel, dim3(n_achunks), dim3(256), 0, s, c, params, grads, saved, e, (double)rho, (const double*)partial, norm);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_sar_restore(float* params, const float* saved, const int* achunks, int n_achunks, const int* chunk2tensor,
                                const unsigned char* active, int n_tensors, long n, void* stream) {
  const TtaChunks c = {achunks, n_achunks, chunk2tensor, active, n_tensors, n / 1024};
  if (int rc = tta_slab_check("stil_sar_restore", c, n, {params, saved})) return rc;
  if (n_achunks == 0) return STIL_OK;
  hipLaunchKernelGGL(tta_chunk_kernel<SarRestore>, dim3(n_achunks), dim3(256), 0, (hipStream_t)stream, c,
                     SarRestore{(float4*)params, (const float4*)saved});
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_sar_recover(float* params, const float* theta0, float* exp_avg, float* exp_avg_sq, int* steps, const int* achunks,
                                int n_achunks, const int* chunk2tensor, const unsigned char* active, int n_tensors, long n,
                                const int* recover, int* ema_valid, void* stream) {
  const TtaChunks c = {achunks, n_achunks, chunk2tensor, active, n_tensors, n / 1024};
  if (int rc = tta_slab_check("stil_sar_recover", c, n, {params, theta0, exp_avg, exp_avg_sq}, {steps, recover, ema_valid})) return rc;
  hipLaunchKernelGGL(sar_recover_kernel, dim3(n_achunks + 1), dim3(256), 0, (hipStream_t)stream, c, params, theta0, exp_avg, exp_avg_sq, steps,
                     recover, ema_valid);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
