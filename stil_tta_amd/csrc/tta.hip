// Test-time adaptation (TENT: Wang et al., ICLR 2021, "Tent: Fully Test-Time Adaptation by Entropy Minimization"), the
// hook STiLModel.test_step leaves as a TODO (models/Disentangle/STiLModel.py:523-524): the row softmax entropy of the
// multimodal logits, forward and backward in one launch, plus its batch mean.
//   lse_r = log sum_k exp(z_rk)                       in double, as the CLIP loss (csrc/loss.hip)
//   p_rk  = exp(z_rk - lse_r)                         formed in double, rounded once
//   H_r   = -sum_k p_rk log p_rk                      in double, rounded once
//   dZ_rk = -p_rk (log p_rk + H_r) * grad_scale       formed in double (the double H_r), rounded once
//   mean  = sum_r H_r / rows                          one workgroup, fixed order (no float atomics)
// One 256-thread workgroup (four waves) per row, any K >= 1: every thread strides the row, the reductions are wave64
// __shfl_xor trees and a fixed-order sum of the four wave partials, so the result is bit-identical on repetition.
#include "tta_common.h"

__global__ __launch_bounds__(256) void tta_entropy_rows_kernel(const float* __restrict__ Z, int ld, int K, double gscale,
                                                            double* __restrict__ lse, float* __restrict__ p, int ldp,
                                                            float* __restrict__ H, float* __restrict__ dZ, int ldd) {
  __shared__ float red[16];
  __shared__ double redd[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  double L, h;
  tta_row_lse_h(zr, K, red, redd, L, h);
  if (threadIdx.x == 0) {
    lse[r] = L;
    H[r] = (float)h;
  }
  if (!p && !dZ) return;
  for (int k = threadIdx.x; k < K; k += 256) {
    const double lp = (double)zr[k] - L;
    const double pk = exp(lp);
    if (p) p[(long)r * ldp + k] = (float)pk;
    if (dZ) dZ[(long)r * ldd + k] = (float)(-pk * (lp + h) * gscale);
  }
}

__global__ __launch_bounds__(256) void tta_entropy_mean_kernel(const float* __restrict__ H, int rows, float* __restrict__ mean) {
  __shared__ double redd[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < rows; i += 256) s += (double)H[i];
  s = block_sum_d(s, redd);
  if (threadIdx.x == 0) mean[0] = (float)(s / (double)rows);
}

extern "C" int stil_entropy_rows(const float* Z, int ld, int rows, int K, float grad_scale, double* lse, float* p, int ldp,
                                 float* H, float* dZ, int ldd, float* mean, void* stream) {
  STIL_REQUIRE(Z && lse && H && mean, "stil_entropy_rows: null pointer");
  STIL_REQUIRE(rows >= 1 && K >= 1 && ld >= K, "stil_entropy_rows: bad shape rows=%d K=%d ld=%d", rows, K, ld);
  STIL_REQUIRE(!p || ldp >= K, "stil_entropy_rows: ldp=%d < K=%d", ldp, K);
  STIL_REQUIRE(!dZ || ldd >= K, "stil_entropy_rows: ldd=%d < K=%d", ldd, K);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tta_entropy_rows_kernel, dim3(rows), dim3(256), 0, s, Z, ld, K, (double)grad_scale, lse, p, ldp, H, dZ, ldd);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(tta_entropy_mean_kernel, dim3(1), dim3(256), 0, s, (const float*)H, rows, mean);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
