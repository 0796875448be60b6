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
#include "common.h"

// lse and softmax entropy (double) of one row zr[0:K] by one 256-thread block: shared by stil_entropy_rows and the rows
// kernels of eata.hip, deyo.hip and sar.hip, whose lse, p and H are therefore bit-identical
__device__ __forceinline__ void tta_row_lse_h(const float* __restrict__ zr, int K, float* red, double* redd, double& L, double& h) {
  float m = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) m = fmaxf(m, zr[k]);
  m = block_max(m, red);
  double s = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) s += exp((double)zr[k] - (double)m);
  s = block_sum_d(s, redd);
  L = (double)m + log(s);
  double a = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const double lp = (double)zr[k] - L;
    a -= exp(lp) * lp;
  }
  h = block_sum_d(a, redd);
}

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

// ---- shared by the selected-row losses (csrc/eata.hip, deyo.hip, sar.hip): each is three launches, its own rows kernel, its
// own reduce kernel built from the two helpers below, and tta_sel_dz_kernel
struct TtaSelSums {
  double n, n_rel, wh;  // selected rows, reliable rows, sum over the selected rows of w H
};

// the sums of EATA's and DeYO's reduce kernels over the float w and H, by one 256-thread block, in every thread
__device__ __forceinline__ TtaSelSums tta_sel_sums(int rows, const float* __restrict__ H, const float* __restrict__ w,
                                                   const unsigned char* __restrict__ rel, const unsigned char* __restrict__ sel,
                                                   double* redd) {
  TtaSelSums s = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < rows; i += 256) {
    if (sel[i]) {
      s.n += 1.0;
      s.wh += (double)w[i] * (double)H[i];
    }
    if (rel[i]) s.n_rel += 1.0;
  }
  s.n = block_sum_d(s.n, redd);  // integers below 2^53: exact
  s.n_rel = block_sum_d(s.n_rel, redd);
  s.wh = block_sum_d(s.wh, redd);
  return s;
}

// the gate of the Adam step, by one 256-thread block: n never leaves the device
__device__ __forceinline__ void tta_gate(const unsigned char* __restrict__ active, unsigned char* __restrict__ active_out,
                                         int n_tensors, int n) {
  for (int t = threadIdx.x; t < n_tensors; t += 256) active_out[t] = (unsigned char)(active[t] && n > 0);
}

// the weight of selected row r, whose double entropy is h: EATA's exp(E0 - H_r), DeYO's stored double w_r, SAR's 1
struct TtaWeightMargin {
  double e0;
  __device__ double operator()(int, double h) const { return exp(e0 - h); }
};
struct TtaWeightStored {
  const double* __restrict__ Wd;
  __device__ double operator()(int r, double) const { return Wd[r]; }
};
struct TtaWeightOne {
  __device__ double operator()(int, double) const { return 1.0; }
};

// dZ_rk = sel_r weight_r (-p_rk (log p_rk + H_r)) grad_scale / n, 0 when n == 0; lse and Hd are the rows kernel's doubles
template <class Weight>
__global__ __launch_bounds__(256) void tta_sel_dz_kernel(const float* __restrict__ Z, int ld, int K, Weight weight, double gscale,
                                                          const double* __restrict__ lse, const double* __restrict__ Hd,
                                                          const unsigned char* __restrict__ sel, const int* __restrict__ counts,
                                                          float* __restrict__ dZ, int ldd) {
  const int r = blockIdx.x;
  const int n = counts[0];
  float* dr = dZ + (long)r * ldd;
  if (n <= 0 || !sel[r]) {  // uniform across the block
    for (int k = threadIdx.x; k < K; k += 256) dr[k] = 0.f;
    return;
  }
  const float* zr = Z + (long)r * ld;
  const double L = lse[r], h = Hd[r];
  const double f = weight(r, h) * gscale / (double)n;  // in this order in every instantiation; exact with weight 1
  for (int k = threadIdx.x; k < K; k += 256) {
    const double lp = (double)zr[k] - L;
    dr[k] = (float)(-exp(lp) * (lp + h) * f);
  }
}

// ---- shared by the slab kernels of eata.hip and sar.hip: one block per 1024-float chunk of A listed in `achunks`
__device__ __forceinline__ bool tta_chunk_live(int ch, long nchunks, const int* __restrict__ chunk2tensor,
                                               const unsigned char* __restrict__ active, int n_tensors) {
  if (ch < 0 || ch >= nchunks) return false;
  const int t = chunk2tensor[ch];
  return t >= 0 && t < n_tensors && active[t];
}

#define TTA_SLAB_REQUIRE(name) \
  STIL_REQUIRE(n >= 0 && n % 1024 == 0 && n_achunks >= 0 && n_tensors >= 0, name ": n=%ld must be a multiple of 1024, n_achunks=%d", n, n_achunks)
