// SHOT's information maximisation (Liang et al., ICML 2020, "Do We Really Need to Access the Source Data?"; the SHOT-IM baseline
// of the TENT paper) for test-time adaptation: TENT's row entropy (csrc/tta.hip) minus the entropy of the batch-mean prediction,
// which is what penalises the collapse of every row onto one class.  include/stil_infomax.h states the arithmetic.
//   pbar_k = (1/rows) sum_r p_rk,   D = sum_k pbar_k log(pbar_k + eps),   c_k = dD/dpbar_k = log(pbar_k + eps) + pbar_k / (pbar_k + eps)
//   dZ_rk  = grad_scale p_rk ( -(log p_rk + H_r) + lambda (c_k - sum_j p_rj c_j) )
// The first loss whose gradient couples the rows, hence three passes and a finish (four launches, no atomics):
//   rows     one 256-thread workgroup per row (tta_row_lse_h: lse, p, H are stil_entropy_rows' bit for bit); H_r in double -> ws
//   columns  one thread per column walks the rows in order (p recomputed from Z and the double lse; loads coalesce across
//            columns): pbar, c -> ws, and the workgroup's partial of D -> ws
//   dz       one workgroup per row: the row's dot product with c, then dZ (with lambda == 0: stil_entropy_rows' expression)
//   finish   one workgroup: mean H (the sum behind stil_entropy_rows' mean) and D from the partials, in order
// ws (doubles): c [K] | partials of D [ceil(K / 256) <= K] | H [rows]
#include "tta_common.h"

__global__ __launch_bounds__(256) void infomax_rows_kernel(const float* __restrict__ Z, int ld, int K, double* __restrict__ lse,
                                                        float* __restrict__ p, int ldp, float* __restrict__ H,
                                                        double* __restrict__ hd) {
  __shared__ float red[16];
  __shared__ double redd[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  double L, h;
  tta_row_lse_h(zr, K, red, redd, L, h);
  if (threadIdx.x == 0) {
    lse[r] = L;
    H[r] = (float)h;
    hd[r] = h;
  }
  if (!p) return;
  for (int k = threadIdx.x; k < K; k += 256) p[(long)r * ldp + k] = (float)exp((double)zr[k] - L);
}

__global__ __launch_bounds__(256) void infomax_cols_kernel(const float* __restrict__ Z, int ld, int rows, int K, double eps,
                                                        const double* __restrict__ lse, float* __restrict__ pbar,
                                                        double* __restrict__ c, double* __restrict__ dpart) {
  __shared__ double redd[16];
  const int k = blockIdx.x * 256 + threadIdx.x;
  double d = 0.0;
  if (k < K) {
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s += exp((double)Z[(long)r * ld + k] - lse[r]);
    const double pb = s / (double)rows;
    const double lg = log(pb + eps);
    pbar[k] = (float)pb;
    c[k] = lg + pb / (pb + eps);
    d = pb * lg;
  }
  d = block_sum_d(d, redd);
  if (threadIdx.x == 0) dpart[blockIdx.x] = d;
}

__global__ __launch_bounds__(256) void infomax_dz_kernel(const float* __restrict__ Z, int ld, int K, double gscale, double lam,
                                                      const double* __restrict__ lse, const double* __restrict__ hd,
                                                      const double* __restrict__ c, float* __restrict__ dZ, int ldd) {
  __shared__ double redd[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  const double L = lse[r], h = hd[r];
  double dot = 0.0;
  if (lam != 0.0) {
    double a = 0.0;
    for (int k = threadIdx.x; k < K; k += 256) a += exp((double)zr[k] - L) * c[k];
    dot = block_sum_d(a, redd);
  }
  for (int k = threadIdx.x; k < K; k += 256) {
    const double lp = (double)zr[k] - L;
    const double pk = exp(lp);
    double g = -pk * (lp + h);
    if (lam != 0.0) g += lam * pk * (c[k] - dot);
    dZ[(long)r * ldd + k] = (float)(g * gscale);
  }
}

__global__ __launch_bounds__(256) void infomax_finish_kernel(const float* __restrict__ H, int rows, const double* __restrict__ dpart,
                                                          int nblk, double lam, float* __restrict__ out) {
  __shared__ double redd[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < rows; i += 256) s += (double)H[i];
  s = block_sum_d(s, redd);
  double d = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) d += dpart[i];
  d = block_sum_d(d, redd);
  if (threadIdx.x == 0) {
    const double mean = s / (double)rows;
    out[0] = (float)(lam != 0.0 ? mean + lam * d : mean);
    out[1] = (float)mean;
    out[2] = (float)d;
  }
}

extern "C" int stil_infomax_rows(const float* Z, int ld, int rows, int K, float grad_scale, float div_weight, float eps, double* lse,
                                 float* p, int ldp, float* H, float* pbar, float* dZ, int ldd, float* out, double* ws, void* stream) {
  STIL_REQUIRE(Z && lse && H && pbar && out && ws, "stil_infomax_rows: null pointer");
  STIL_REQUIRE(rows >= 1 && K >= 1 && ld >= K, "stil_infomax_rows: bad shape rows=%d K=%d ld=%d", rows, K, ld);
  STIL_REQUIRE(!p || ldp >= K, "stil_infomax_rows: ldp=%d < K=%d", ldp, K);
  STIL_REQUIRE(!dZ || ldd >= K, "stil_infomax_rows: ldd=%d < K=%d", ldd, K);
  STIL_REQUIRE(eps > 0.0f && eps <= 3.402823466e38f, "stil_infomax_rows: eps=%g is not finite and positive", (double)eps);
  STIL_REQUIRE(div_weight >= 0.0f && div_weight <= 3.402823466e38f, "stil_infomax_rows: div_weight=%g is not finite and >= 0", (double)div_weight);
  hipStream_t s = (hipStream_t)stream;
  const int nblk = cdiv(K, 256);
  double* c = ws;
  double* dpart = ws + K;
  double* hd = ws + 2 * (long)K;
  hipLaunchKernelGGL(infomax_rows_kernel, dim3(rows), dim3(256), 0, s, Z, ld, K, lse, p, ldp, H, hd);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(infomax_cols_kernel, dim3(nblk), dim3(256), 0, s, Z, ld, rows, K, (double)eps, (const double*)lse, pbar, c, dpart);
  STIL_LAUNCH_CHECK();
  if (dZ) {
    hipLaunchKernelGGL(infomax_dz_kernel, dim3(rows), dim3(256), 0, s, Z, ld, K, (double)grad_scale, (double)div_weight,
                       (const double*)lse, (const double*)hd, (const double*)c, dZ, ldd);
    STIL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(infomax_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)H, rows, (const double*)dpart, nblk,
                     (double)div_weight, out);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
