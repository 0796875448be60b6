// Test-time adaptation, ROID (Marsden, Doebler, Yang, WACV 2024, "Universal Test-time Adaptation through Weight Ensembling,
// Diversity Weighting, and Prior Correction"; definition as recalled: unpinned) on top of TENT (csrc/tta.hip): the soft
// likelihood ratio of the rows a certainty-and-diversity selection keeps, the running mean prediction, the prior correction of
// the scores and the weight ensembling of A with its source values.  csrc/stil_roid.h states the arithmetic.
// The selection couples the rows through the minimum, the maximum and the mean over the batch, hence four launches, no atomics:
//   rows     one 256-thread workgroup per row (tta_row_lse_h: lse, p, H are stil_entropy_rows' bit for bit): the cosine with the
//            running mean as it stands, the soft likelihood ratio; Hd, d, slr in double -> ws
//   columns  one thread per column walks the rows in order, as the columns pass of csrc/infomax.hip: pbar (double) -> ws
//   finish   one workgroup: minimum, maximum, the normalised d and c, their mean, keep, w, loss, counts; then the running mean
//            (every cosine was read a launch ago) and the prior s -> ws
//   dz       one workgroup per row: the row's dot product with g, then dZ; with the correction, the row's dot product with s, then scores
// ws (doubles): Hd [rows] | d [rows] | slr [rows] | w [rows] | pbar [K] | s [K]
// The minima and maxima over the batch are block_reduce (csrc/common.h) with fmin, a maximum as -min(-v): what a NaN does is fmin's.
// The ensembling is a functor over the chunk walker of csrc/tta_common.h.
#include "tta_common.h"

__global__ __launch_bounds__(256) void roid_rows_kernel(const float* __restrict__ Z, int ld, int K, const float* __restrict__ ema,
                                                         double clip, double eps, double* __restrict__ lse, float* __restrict__ p,
                                                         int ldp, float* __restrict__ H, float* __restrict__ cosv,
                                                         float* __restrict__ slr, double* __restrict__ hd, double* __restrict__ dd,
                                                         double* __restrict__ sd) {
  __shared__ float red[16];
  __shared__ double redd[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  double L, h;
  tta_row_lse_h(zr, K, red, redd, L, h);
  double dot = 0.0, pp = 0.0, ee = 0.0, sl = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const double pk = exp((double)zr[k] - L);
    const double e = (double)ema[k];
    p[(long)r * ldp + k] = (float)pk;
    dot += pk * e;
    pp += pk * pk;
    ee += e * e;
    const double q = fmin(pk, clip);
    sl -= q * log(q / (1.0 - q) + eps);
  }
  dot = block_sum_d(dot, redd);
  pp = block_sum_d(pp, redd);
  ee = block_sum_d(ee, redd);
  sl = block_sum_d(sl, redd);
  if (threadIdx.x == 0) {
    const double c = dot / (sqrt(pp) * sqrt(ee));
    lse[r] = L;
    H[r] = (float)h;
    cosv[r] = (float)c;
    slr[r] = (float)sl;
    hd[r] = h;
    dd[r] = 1.0 - c;
    sd[r] = sl;
  }
}

__global__ __launch_bounds__(256) void roid_cols_kernel(const float* __restrict__ Z, int ld, int rows, int K,
                                                         const double* __restrict__ lse, float* __restrict__ pbar,
                                                         double* __restrict__ pbd) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  double s = 0.0;
  for (int r = 0; r < rows; ++r) s += exp((double)Z[(long)r * ld + k] - lse[r]);
  const double pb = s / (double)rows;
  pbar[k] = (float)pb;
  pbd[k] = pb;
}

__global__ __launch_bounds__(256) void roid_finish_kernel(int rows, int K, double tau, double mom, const double* __restrict__ hd,
                                                           const double* __restrict__ dd, const double* __restrict__ sd,
                                                           double* __restrict__ wd, const double* __restrict__ pbd,
                                                           double* __restrict__ sprior, float* __restrict__ dn, float* __restrict__ cn,
                                                           float* __restrict__ w, unsigned char* __restrict__ keep,
                                                           float* __restrict__ ema, float* __restrict__ prior,
                                                           int* __restrict__ counts, float* __restrict__ loss) {
  __shared__ double redd[16];
  double dmin = INFINITY, dmax = -INFINITY, cmin = INFINITY, cmax = -INFINITY;
  for (int i = threadIdx.x; i < rows; i += 256) {
    const double d = dd[i], c = -hd[i];
    dmin = fmin(dmin, d);
    dmax = fmax(dmax, d);
    cmin = fmin(cmin, c);
    cmax = fmax(cmax, c);
  }
  const auto least = [](double a, double b) { return fmin(a, b); };
  dmin = block_reduce(dmin, redd, least);
  dmax = -block_reduce(-dmax, redd, least);
  cmin = block_reduce(cmin, redd, least);
  cmax = -block_reduce(-cmax, redd, least);
  const double dr = dmax - dmin, cr = cmax - cmin;
  const bool ddeg = !(dr > 1e-9), cdeg = !(cr > 1e-9);  // the degenerate rule: that normalised quantity is 0 for every row
  double s = 0.0;
  for (int i = threadIdx.x; i < rows; i += 256) s += ddeg ? 0.0 : (dd[i] - dmin) / dr;
  const double mean = block_sum_d(s, redd) / (double)rows;
  double nk = 0.0, ls = 0.0;
  for (int i = threadIdx.x; i < rows; i += 256) {
    const double a = ddeg ? 0.0 : (dd[i] - dmin) / dr;
    const double b = cdeg ? 0.0 : (-hd[i] - cmin) / cr;
    const bool kp = !(a < mean);
    const double wi = kp ? exp(a * b / tau) : 0.0;
    dn[i] = (float)a;
    cn[i] = (float)b;
    w[i] = (float)wi;
    keep[i] = (unsigned char)kp;
    wd[i] = wi;
    if (kp) nk += 1.0;
    ls += wi * sd[i];
  }
  nk = block_sum_d(nk, redd);  // integers below 2^53: exact
  ls = block_sum_d(ls, redd);
  double pm = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) pm = fmax(pm, pbd[k]);
  pm = -block_reduce(-pm, redd, least);
  const double smooth = fmax(1.0 / (double)rows, 1.0 / (double)K) / pm;
  for (int k = threadIdx.x; k < K; k += 256) {
    const double pb = pbd[k];
    const double sk = (pb + smooth) / (1.0 + smooth * (double)K);
    sprior[k] = sk;
    if (prior) prior[k] = (float)sk;
    ema[k] = (float)(mom * (double)ema[k] + (1.0 - mom) * pb);
  }
  if (threadIdx.x == 0) {
    counts[0] = (int)nk;
    counts[1] = rows;
    counts[2] = ddeg ? 1 : 0;
    counts[3] = cdeg ? 1 : 0;
    loss[0] = (float)(ls / (double)rows);
  }
}

__global__ __launch_bounds__(256) void roid_dz_kernel(const float* __restrict__ Z, int ld, int rows, int K, double clip, double eps,
                                                       double gscale, const double* __restrict__ lse, const double* __restrict__ wd,
                                                       const unsigned char* __restrict__ keep, const double* __restrict__ sprior,
                                                       float* __restrict__ dZ, int ldd, float* __restrict__ scores, int lds) {
  __shared__ double redd[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  const double L = lse[r];
  float* dr = dZ + (long)r * ldd;
  if (!keep[r]) {  // uniform across the block
    for (int k = threadIdx.x; k < K; k += 256) dr[k] = 0.f;
  } else {
    double a = 0.0;
    for (int k = threadIdx.x; k < K; k += 256) {
      const double pk = exp((double)zr[k] - L);
      if (pk <= clip) {
        const double u = pk / (1.0 - pk);
        a += pk * (-log(u + eps) - u / ((u + eps) * (1.0 - pk)));
      }
    }
    const double dot = block_sum_d(a, redd);
    const double f = gscale * (wd[r] / (double)rows);
    for (int k = threadIdx.x; k < K; k += 256) {
      const double pk = exp((double)zr[k] - L);
      double g = 0.0;
      if (pk <= clip) {
        const double u = pk / (1.0 - pk);
        g = -log(u + eps) - u / ((u + eps) * (1.0 - pk));
      }
      dr[k] = (float)(f * pk * (g - dot));
    }
  }
  if (!scores) return;
  double b = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) b += exp((double)zr[k] - L) * sprior[k];
  const double den = block_sum_d(b, redd);
  for (int k = threadIdx.x; k < K; k += 256) scores[(long)r * lds + k] = (float)(exp((double)zr[k] - L) * sprior[k] / den);
}

extern "C" int stil_roid_rows(const float* Z, int ld, int rows, int K, float* ema, float tau, float clip, float eps, float momentum,
                              float grad_scale, int correct, double* lse, float* p, int ldp, float* H, float* cos, float* slr, float* dn,
                              float* cn, float* w, unsigned char* keep, float* pbar, float* prior, float* scores, int lds, float* dZ, int ldd,
                              int* counts, float* loss, double* ws, void* stream) {
  STIL_REQUIRE(Z && ema && lse && p && H && cos && slr && dn && cn && w && keep && pbar && dZ && counts && loss && ws,
               "stil_roid_rows: null pointer");
  STIL_REQUIRE(correct == 0 || correct == 1, "stil_roid_rows: correct=%d must be 0 or 1", correct);
  STIL_REQUIRE(!correct || (prior && scores), "stil_roid_rows: the prior correction needs prior and scores");
  STIL_REQUIRE(rows >= 1 && K >= 1 && ld >= K, "stil_roid_rows: bad shape rows=%d K=%d ld=%d", rows, K, ld);
  STIL_REQUIRE(ldp >= K && ldd >= K, "stil_roid_rows: ldp=%d ldd=%d < K=%d", ldp, ldd, K);
  STIL_REQUIRE(!correct || lds >= K, "stil_roid_rows: lds=%d < K=%d", lds, K);
  STIL_REQUIRE(tau > 0.0f && tau <= 3.402823466e38f, "stil_roid_rows: tau=%g is not finite and positive", (double)tau);
  STIL_REQUIRE(eps > 0.0f && eps <= 3.402823466e38f, "stil_roid_rows: eps=%g is not finite and positive", (double)eps);
  STIL_REQUIRE(clip > 0.0f && clip < 1.0f, "stil_roid_rows: clip=%g is not inside (0, 1)", (double)clip);
  STIL_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "stil_roid_rows: momentum=%g is not inside [0, 1]", (double)momentum);
  STIL_REQUIRE(grad_scale >= -3.402823466e38f && grad_scale <= 3.402823466e38f, "stil_roid_rows: grad_scale=%g is not finite", (double)grad_scale);
  hipStream_t s = (hipStream_t)stream;
  double* hd = ws;
  double* dd = ws + rows;
  double* sd = ws + 2 * (long)rows;
  double* wd = ws + 3 * (long)rows;
  double* pbd = ws + 4 * (long)rows;
  double* sprior = pbd + K;
  hipLaunchKernelGGL(roid_rows_kernel, dim3(rows), dim3(256), 0, s, Z, ld, K, (const float*)ema, (double)clip, (double)eps, lse, p, ldp, H,
                     cos, slr, hd, dd, sd);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(roid_cols_kernel, dim3(cdiv(K, 256)), dim3(256), 0, s, Z, ld, rows, K, (const double*)lse, pbar, pbd);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(roid_finish_kernel, dim3(1), dim3(256), 0, s, rows, K, (double)tau, (double)momentum, (const double*)hd,
                     (const double*)dd, (const double*)sd, wd, (const double*)pbd, sprior, dn, cn, w, keep, ema, prior, counts, loss);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(roid_dz_kernel, dim3(rows), dim3(256), 0, s, Z, ld, rows, K, (double)clip, (double)eps, (double)grad_scale,
                     (const double*)lse, (const double*)wd, (const unsigned char*)keep, (const double*)sprior, dZ, ldd,
                     correct ? scores : (float*)nullptr, lds);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

// ---- weight ensembling over A's chunks: A <- m A + (1 - m) theta0
struct RoidEnsemble {
  float4* __restrict__ params; const float4* __restrict__ theta0; double m;
  __device__ void operator()(long i, long ic) const {
    const float4 t0 = theta0[ic];
    if (m == 0.0) {  // uniform across the grid: a copy, whatever A holds
      params[i] = t0;
      return;
    }
    float4 th = params[i];
    const double n1 = 1.0 - m;
    th.x = (float)(m * (double)th.x + n1 * (double)t0.x);
    th.y = (float)(m * (double)th.y + n1 * (double)t0.y);
    th.z = (float)(m * (double)th.z + n1 * (double)t0.z);
    th.w = (float)(m * (double)th.w + n1 * (double)t0.w);
    params[i] = th;
  }
};

extern "C" int stil_roid_ensemble(float* params, const float* theta0, const int* achunks, int n_achunks, const int* chunk2tensor,
                                  const unsigned char* active, int n_tensors, long n, float momentum, void* stream) {
  const TtaChunks c = {achunks, n_achunks, chunk2tensor, active, n_tensors, n / 1024};
  if (int rc = tta_slab_check("stil_roid_ensemble", c, n, {params, theta0})) return rc;
  STIL_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "stil_roid_ensemble: momentum=%g is not inside [0, 1]", (double)momentum);
  if (n_achunks == 0 || momentum == 1.0f) return STIL_OK;
  hipLaunchKernelGGL(tta_chunk_kernel<RoidEnsemble>, dim3(n_achunks), dim3(256), 0, (hipStream_t)stream, c,
                     RoidEnsemble{(float4*)params, (const float4*)theta0, (double)momentum});
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
