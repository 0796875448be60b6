// READ (Yang et al., ICLR 2024, "Test-time Adaptation against Multi-modal Reliability Bias") for test-time adaptation of the
// fusion attention: a confidence-aware row loss that pushes the rows whose confidence lies above gamma and damps those below,
// plus SHOT's batch-balance term (csrc/infomax.hip).  csrc/stil_read.h states the arithmetic.
//   c_r    = p_r[yhat_r], yhat_r the first maximum of z_r;   f_r = c_r (1 + ln gamma - ln c_r),   df/dc = ln(gamma / c)
//   dZ_rk  = grad_scale ( ln(gamma / c_r) c_r ([k == yhat_r] - p_rk) + lambda p_rk (ck_k - sum_j p_rj ck_j) )
// Four launches, no atomics:
//   rows     one 256-thread workgroup per row, any K >= 1 (every thread strides the row): tta_row_lse_h (lse, p are
//            stil_entropy_rows' bit for bit), the first maximum as stil_deyo_rows finds it, c_r and f_r by thread 0
//   columns  infomax_cols_kernel itself: pbar, ck -> ws, the partials of D -> ws (stil_infomax_rows' bits)
//   dz       one workgroup per row: c_r again from Z and the double lse, the row's dot product with ck, then dZ
//   finish   infomax_finish_kernel itself over f in place of H: mean f and D from the partials, in order
// ws (doubles): ck [K] | partials of D [ceil(K / 256) <= K]
// infomax_cols_kernel and infomax_finish_kernel are csrc/infomax.hip's, the one pair this file takes from a sibling rather than
// from a header: stil_hip.hip includes infomax.hip before this file.
#include "tta_common.h"
#include "stil_read.h"

__global__ __launch_bounds__(256) void read_rows_kernel(const float* __restrict__ Z, int ld, int K, double one_lgam,
                                                         double* __restrict__ lse, float* __restrict__ p, int ldp,
                                                         int* __restrict__ yhat, float* __restrict__ conf, float* __restrict__ f) {
  __shared__ float red[16];
  __shared__ double redd[16];
  __shared__ int redi[4];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  double L, h;
  tta_row_lse_h(zr, K, red, redd, L, h);
  float m = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) {
    const float z = zr[k];
    if (p) p[(long)r * ldp + k] = (float)exp((double)z - L);
    m = fmaxf(m, z);
  }
  m = block_max(m, red);
  int yi = INT_MAX;
  for (int k = threadIdx.x; k < K; k += 256)
    if (zr[k] == m) yi = min(yi, k);
  yi = block_reduce<4>(yi, redi, [](int a, int b) { return min(a, b); });
  if (yi >= K) yi = 0;  // a row without a maximum (every logit NaN): any index in range
  if (threadIdx.x == 0) {
    const double lc = (double)zr[yi] - L;  // ln c_r
    const double c = exp(lc);
    lse[r] = L;
    yhat[r] = yi;
    conf[r] = (float)c;
    f[r] = (float)(c * (one_lgam - lc));
  }
}

__global__ __launch_bounds__(256) void read_dz_kernel(const float* __restrict__ Z, int ld, int K, double gscale, double lam,
                                                       double lgam, const double* __restrict__ lse, const int* __restrict__ yhat,
                                                       const double* __restrict__ ck, float* __restrict__ dZ, int ldd) {
  __shared__ double redd[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  const double L = lse[r];
  const int yi = yhat[r];
  const double lc = (double)zr[yi] - L;
  const double a = (lgam - lc) * exp(lc);  // ln(gamma / c_r) c_r
  double dot = 0.0;
  if (lam != 0.0) {
    double s = 0.0;
    for (int k = threadIdx.x; k < K; k += 256) s += exp((double)zr[k] - L) * ck[k];
    dot = block_sum_d(s, redd);
  }
  for (int k = threadIdx.x; k < K; k += 256) {
    const double pk = exp((double)zr[k] - L);
    double g = a * ((k == yi ? 1.0 : 0.0) - pk);
    if (lam != 0.0) g += lam * pk * (ck[k] - dot);
    dZ[(long)r * ldd + k] = (float)(g * gscale);
  }
}

extern "C" int stil_read_rows(const float* Z, int ld, int rows, int K, float grad_scale, float gamma, float div_weight, float eps,
                              double* lse, float* p, int ldp, int* yhat, float* conf, float* f, float* pbar, float* dZ, int ldd,
                              float* out, double* ws, void* stream) {
  STIL_REQUIRE(Z && lse && yhat && conf && f && pbar && out && ws, "stil_read_rows: null pointer");
  STIL_REQUIRE(rows >= 1 && K >= 1 && ld >= K, "stil_read_rows: bad shape rows=%d K=%d ld=%d", rows, K, ld);
  STIL_REQUIRE(!p || ldp >= K, "stil_read_rows: ldp=%d < K=%d", ldp, K);
  STIL_REQUIRE(!dZ || ldd >= K, "stil_read_rows: ldd=%d < K=%d", ldd, K);
  STIL_REQUIRE(gamma > 0.0f && gamma <= 1.0f, "stil_read_rows: gamma=%g is not in (0, 1]", (double)gamma);
  STIL_REQUIRE(eps > 0.0f && eps <= 3.402823466e38f, "stil_read_rows: eps=%g is not finite and positive", (double)eps);
  STIL_REQUIRE(div_weight >= 0.0f && div_weight <= 3.402823466e38f, "stil_read_rows: div_weight=%g is not finite and >= 0", (double)div_weight);
  hipStream_t s = (hipStream_t)stream;
  const int nblk = cdiv(K, 256);
  const double lgam = log((double)gamma);
  double* ck = ws;
  double* dpart = ws + K;
  hipLaunchKernelGGL(read_rows_kernel, dim3(rows), dim3(256), 0, s, Z, ld, K, 1.0 + lgam, lse, p, ldp, yhat, conf, f);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(infomax_cols_kernel, dim3(nblk), dim3(256), 0, s, Z, ld, rows, K, (double)eps, (const double*)lse, pbar, ck, dpart);
  STIL_LAUNCH_CHECK();
  if (dZ) {
    hipLaunchKernelGGL(read_dz_kernel, dim3(rows), dim3(256), 0, s, Z, ld, K, (double)grad_scale, (double)div_weight, lgam,
                       (const double*)lse, (const int*)yhat, (const double*)ck, dZ, ldd);
    STIL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(infomax_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)f, rows, (const double*)dpart, nblk,
                     (double)div_weight, out);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
