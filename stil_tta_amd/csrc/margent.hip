// MEMO's marginal entropy (Zhang, Levine, Finn, NeurIPS 2022, "MEMO: Test Time Robustness via Adaptation and Augmentation") for
// test-time adaptation on one test point at a time: the entropy of the mean prediction over V augmented views of each sample.
// include/stil_margent.h states the arithmetic.  Row r is view r % V of sample g = r / V.
//   logpbar_gk = logsumexp_v(z_(gV+v)k - lse_(gV+v)) - log V,   pbar_gk = exp(logpbar_gk),   Hbar_g = -sum_k pbar_gk logpbar_gk
//   dZ_rj      = grad_scale / V  p_rj ( sum_k p_rk logpbar_gk - logpbar_gj )
// The views of a sample couple through its marginal, hence three passes and a finish (four launches, no atomics):
//   rows     one 256-thread workgroup per row (tta_row_lse_h: lse and p are stil_entropy_rows' bit for bit)
//   columns  one thread per (sample, column) walks the sample's views in order, however many there are (log p recomputed from Z
//            and the double lse; loads coalesce across columns): logpbar -> ws, pbar, the workgroup's partial of Hbar -> ws
//   dz       one workgroup per row: the row's dot product with its sample's logpbar, then dZ
//   finish   one workgroup: Hbar of every sample from its partials, in order, and their mean
// ws (doubles): logpbar [groups, K] | partials of Hbar [groups, ceil(K / 256)]
#include "tta_common.h"

__global__ __launch_bounds__(256) void margent_rows_kernel(const float* __restrict__ Z, int ld, int K, double* __restrict__ lse,
                                                        float* __restrict__ p, int ldp) {
  __shared__ float red[16];
  __shared__ double redd[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  double L, h;
  tta_row_lse_h(zr, K, red, redd, L, h);
  if (threadIdx.x == 0) lse[r] = L;
  if (!p) return;
  for (int k = threadIdx.x; k < K; k += 256) p[(long)r * ldp + k] = (float)exp((double)zr[k] - L);
}

__global__ __launch_bounds__(256) void margent_cols_kernel(const float* __restrict__ Z, int ld, int views, int K, int nblk,
                                                        const double* __restrict__ lse, float* __restrict__ pbar, int ldb,
                                                        double* __restrict__ logpbar, double* __restrict__ hpart) {
  __shared__ double redd[16];
  const int g = blockIdx.x;
  const long r0 = (long)g * views;
  const double logv = log((double)views);
  for (int cb = blockIdx.y; cb < nblk; cb += gridDim.y) {   // cb is uniform over the workgroup: every thread reaches block_sum_d
    const int k = cb * 256 + threadIdx.x;
    double d = 0.0;
    if (k < K) {
      double m = -INFINITY;
      for (int v = 0; v < views; ++v) m = fmax(m, (double)Z[(r0 + v) * ld + k] - lse[r0 + v]);
      double s = 0.0;
      for (int v = 0; v < views; ++v) s += exp((double)Z[(r0 + v) * ld + k] - lse[r0 + v] - m);
      const double lpb = m + log(s) - logv;
      const double pb = exp(lpb);
      logpbar[(long)g * K + k] = lpb;
      pbar[(long)g * ldb + k] = (float)pb;
      d = -pb * lpb;
    }
    d = block_sum_d(d, redd);
    if (threadIdx.x == 0) hpart[(long)g * nblk + cb] = d;
  }
}

__global__ __launch_bounds__(256) void margent_dz_kernel(const float* __restrict__ Z, int ld, int views, int K, double gscale,
                                                      const double* __restrict__ lse, const double* __restrict__ logpbar,
                                                      float* __restrict__ dZ, int ldd) {
  __shared__ double redd[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  const double* lb = logpbar + (long)(r / views) * K;
  const double L = lse[r];
  double a = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) a += exp((double)zr[k] - L) * lb[k];
  const double dot = block_sum_d(a, redd);
  for (int k = threadIdx.x; k < K; k += 256) dZ[(long)r * ldd + k] = (float)(exp((double)zr[k] - L) * (dot - lb[k]) * gscale);
}

__global__ __launch_bounds__(256) void margent_finish_kernel(const double* __restrict__ hpart, int groups, int nblk,
                                                          float* __restrict__ Hbar, float* __restrict__ out) {
  __shared__ double redd[16];
  double s = 0.0;
  for (int g = threadIdx.x; g < groups; g += 256) {
    double h = 0.0;
    for (int i = 0; i < nblk; ++i) h += hpart[(long)g * nblk + i];
    Hbar[g] = (float)h;
    s += h;
  }
  s = block_sum_d(s, redd);
  if (threadIdx.x == 0) out[0] = (float)(s / (double)groups);
}

extern "C" int stil_marginal_entropy_groups(const float* Z, int ld, int groups, int views, int K, float grad_scale, double* lse,
                                            float* p, int ldp, float* pbar, int ldb, float* Hbar, float* dZ, int ldd, float* out,
                                            double* ws, void* stream) {
  STIL_REQUIRE(Z && lse && pbar && Hbar && out && ws, "stil_marginal_entropy_groups: null pointer");
  STIL_REQUIRE(groups >= 1 && views >= 1 && K >= 1 && ld >= K, "stil_marginal_entropy_groups: bad shape groups=%d views=%d K=%d ld=%d",
               groups, views, K, ld);
  STIL_REQUIRE((long)groups * (long)views <= 2147483647L, "stil_marginal_entropy_groups: groups=%d x views=%d overflows int", groups, views);
  STIL_REQUIRE(ldb >= K, "stil_marginal_entropy_groups: ldb=%d < K=%d", ldb, K);
  STIL_REQUIRE(!p || ldp >= K, "stil_marginal_entropy_groups: ldp=%d < K=%d", ldp, K);
  STIL_REQUIRE(!dZ || ldd >= K, "stil_marginal_entropy_groups: ldd=%d < K=%d", ldd, K);
  hipStream_t s = (hipStream_t)stream;
  const int rows = groups * views;
  const int nblk = cdiv(K, 256);
  double* logpbar = ws;
  double* hpart = ws + (long)groups * K;
  hipLaunchKernelGGL(margent_rows_kernel, dim3(rows), dim3(256), 0, s, Z, ld, K, lse, p, ldp);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(margent_cols_kernel, dim3(groups, nblk < 65535 ? nblk : 65535), dim3(256), 0, s, Z, ld, views, K, nblk,
                     (const double*)lse, pbar, ldb, logpbar, hpart);
  STIL_LAUNCH_CHECK();
  if (dZ) {
    hipLaunchKernelGGL(margent_dz_kernel, dim3(rows), dim3(256), 0, s, Z, ld, views, K, (double)grad_scale / (double)views,
                       (const double*)lse, (const double*)logpbar, dZ, ldd);
    STIL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(margent_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)hpart, groups, nblk, Hbar, out);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
