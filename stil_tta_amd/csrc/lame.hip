// Test-time adaptation, LAME (Boudiaf, Mueller, Ben Ayed, Bertinetto, CVPR 2022, "Parameter-free Online Test-time Adaptation";
// definition and defaults as recalled from the paper and its published code: unpinned): the model and its normalisation stay at
// the source, the batch's output probabilities are corrected: rows whose features are neighbours are pulled towards the same
// prediction by fixed-point iterations of a Laplacian-regularised likelihood.  csrc/stil_lame.h states the arithmetic.
// The affinity, three launches, one 256-thread workgroup per row each:
//   norms        max(|f_i|, 1e-12) in double -> ws
//   neighbours   row i's distances, one wave per pair (lanes stride D, a shuffle tree), into LDS; then the RANK of every j among
//                them (ties to the lower j, a NaN as +inf): rank < k' writes nbr[i, rank] directly, no sort and no reduction
//   weights      every workgroup sums dk in the same fixed order (tta_partial_sum) -> s2, then wts
// The correction, 2 + max_steps + 1 launches, one workgroup per row each:
//   rows         tta_row_lse_h (lse and p are stil_entropy_rows' bit for bit), u = log(p + 1e-10), Y^0 = softmax(u)
//   graph        row i of A = (W + W^T) / 2 into LDS, then compacted in ascending j by one wave (ballot, prefix count) -> ws
//   step n       first E_(n-1), the fixed-order sum of the per-row partials step n - 1 left, in EVERY workgroup: all reach the same
//                decision, nobody waits for anybody; workgroup 0 records E_(n-1) and, when the rule fires or the count is full,
//                steps and the stopping word, on which the launches still enqueued return at once.  Otherwise row i of
//                Y^n = softmax(u + lambda A Y^(n-1)) (Jacobi: the iterate ping-pongs between two buffers) and its energy partial
// Nothing here needs the matrix cores: at the workload's largest shape the Gram products are 1e8 double multiply-adds per batch,
// small beside the model's forward.  Nobody has measured it.
#include "tta_common.h"
#include "stil_lame.h"

__global__ __launch_bounds__(256) void lame_norm_kernel(const float* __restrict__ F, int ldf, int D, double* __restrict__ nrm) {
  __shared__ double redd[16];
  const float* fi = F + (long)blockIdx.x * ldf;
  double s = 0.0;
  for (int d = threadIdx.x; d < D; d += 256) s += (double)fi[d] * (double)fi[d];
  s = block_sum_d(s, redd);
  if (threadIdx.x == 0) nrm[blockIdx.x] = fmax(sqrt(s), 1e-12);
}

__global__ __launch_bounds__(256) void lame_neighbours_kernel(const float* __restrict__ F, int ldf, int rows, int D, int k, int kp,
                                                               const double* __restrict__ nrm, int* __restrict__ nbr,
                                                               double* __restrict__ dk, double* __restrict__ d2sel) {
  __shared__ double dist[STIL_LAME_MAX_ROWS];
  const int i = blockIdx.x, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const float* fi = F + (long)i * ldf;
  const double ni = nrm[i];
  for (int j = w; j < rows; j += 4) {  // one wave per pair
    const float* fj = F + (long)j * ldf;
    double s = 0.0;
    for (int d = l; d < D; d += 64) s += (double)fi[d] * (double)fj[d];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (l == 0) {
      const double d2 = 2.0 - 2.0 * (s / (ni * nrm[j]));
      dist[j] = d2 < 0.0 ? 0.0 : d2;  // not fmax: a NaN stays a NaN
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < rows; j += 256) {
    if (j == i) continue;
    const double dj = dist[j];
    const double kj = dj != dj ? (double)INFINITY : dj;
    int rank = 0;
    for (int q = 0; q < rows; ++q) {  // the same address in every lane: a broadcast
      if (q == i) continue;
      double kq = dist[q];
      kq = kq != kq ? (double)INFINITY : kq;
      rank += (kq < kj || (kq == kj && q < j)) ? 1 : 0;
    }
    if (rank < kp) {  // the ranks are a permutation of 0 .. rows - 2: every slot below k' is written exactly once
      nbr[(long)i * k + rank] = j;
      d2sel[(long)i * kp + rank] = dj;
      if (rank == kp - 1) dk[i] = dj;
    }
  }
  for (int t = kp + threadIdx.x; t < k; t += 256) nbr[(long)i * k + t] = -1;
  if (kp == 0 && threadIdx.x == 0) dk[i] = 0.0;
}

__global__ __launch_bounds__(256) void lame_weights_kernel(int rows, int k, int kp, int kind, const double* __restrict__ dk,
                                                            const double* __restrict__ d2sel, float* __restrict__ wts) {
  __shared__ double redd[16];
  const int i = blockIdx.x;
  double s2 = 0.0;
  if (kind == STIL_LAME_RBF) s2 = tta_partial_sum(dk, rows, redd) / (double)rows;  // uniform across the grid
  for (int t = threadIdx.x; t < k; t += 256) {
    double wv = 0.0;
    if (t < kp) wv = (kind == STIL_LAME_KNN || s2 <= 1e-12) ? 1.0 : exp(-d2sel[(long)i * kp + t] / (2.0 * s2));
    wts[(long)i * k + t] = (float)wv;
  }
}

extern "C" int stil_lame_affinity(const float* F, int ldf, int rows, int D, int k, int kind, int* nbr, float* wts, double* dk, double* ws,
                                  void* stream) {
  STIL_REQUIRE(F && nbr && wts && dk && ws, "stil_lame_affinity: null pointer");
  STIL_REQUIRE(rows >= 1 && D >= 1 && k >= 1 && ldf >= D, "stil_lame_affinity: bad shape rows=%d D=%d k=%d ldf=%d", rows, D, k, ldf);
  STIL_REQUIRE(rows <= STIL_LAME_MAX_ROWS, "stil_lame_affinity: rows=%d exceeds STIL_LAME_MAX_ROWS=%d", rows, STIL_LAME_MAX_ROWS);
  STIL_REQUIRE(kind == STIL_LAME_KNN || kind == STIL_LAME_RBF, "stil_lame_affinity: kind=%d is neither knn (0) nor rbf (1)", kind);
  hipStream_t s = (hipStream_t)stream;
  const int kp = k < rows - 1 ? k : rows - 1;
  double* nrm = ws;
  double* d2sel = ws + rows;
  hipLaunchKernelGGL(lame_norm_kernel, dim3(rows), dim3(256), 0, s, F, ldf, D, nrm);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(lame_neighbours_kernel, dim3(rows), dim3(256), 0, s, F, ldf, rows, D, k, kp, (const double*)nrm, nbr, dk, d2sel);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(lame_weights_kernel, dim3(rows), dim3(256), 0, s, rows, k, kp, kind, (const double*)dk, (const double*)d2sel, wts);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

// ---- the correction
__device__ __forceinline__ double lame_block_max_d(double v, double* redd) {
  return block_reduce<4>(v, redd, [](double a, double b) { return fmax(a, b); });
}

__global__ __launch_bounds__(256) void lame_rows_kernel(const float* __restrict__ Z, int ld, int K, double* __restrict__ lse,
                                                         float* __restrict__ p, int ldp, double* __restrict__ u,
                                                         double* __restrict__ y0, int* __restrict__ stop) {
  __shared__ float red[16];
  __shared__ double redd[16];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  double L, h;
  tta_row_lse_h(zr, K, red, redd, L, h);
  if (threadIdx.x == 0) {
    lse[r] = L;
    if (r == 0) stop[0] = 0;  // the stopping word of this call: every step launch comes after this one
  }
  double* ur = u + (long)r * K;
  double m = -INFINITY;
  for (int c = threadIdx.x; c < K; c += 256) {
    const double pc = exp((double)zr[c] - L);
    p[(long)r * ldp + c] = (float)pc;
    const double uc = log(pc + 1e-10);
    ur[c] = uc;  // read back below by the thread that wrote it
    m = fmax(m, uc);
  }
  m = lame_block_max_d(m, redd);
  double s = 0.0;
  for (int c = threadIdx.x; c < K; c += 256) s += exp(ur[c] - m);
  s = block_sum_d(s, redd);
  for (int c = threadIdx.x; c < K; c += 256) y0[(long)r * K + c] = exp(ur[c] - m) / s;
}

// row i of A = (W + W^T) / 2, compacted: idx[i, 0:cnt[i]] ascending, val beside it
__global__ __launch_bounds__(256) void lame_graph_kernel(const int* __restrict__ nbr, const float* __restrict__ wts, int k, int rows,
                                                          double* __restrict__ val, int* __restrict__ idx, int* __restrict__ cnt) {
  __shared__ double arow[STIL_LAME_MAX_ROWS];
  const int i = blockIdx.x;
  for (int j = threadIdx.x; j < rows; j += 256) {
    double wij = 0.0, wji = 0.0;
    if (j != i)
      for (int t = 0; t < k; ++t) {
        if (nbr[(long)i * k + t] == j) wij += (double)wts[(long)i * k + t];
        if (nbr[(long)j * k + t] == i) wji += (double)wts[(long)j * k + t];
      }
    arow[j] = 0.5 * (wij + wji);  // commutative: A is symmetric bit for bit
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  int n = 0;
  for (int base = 0; base < rows; base += 64) {  // one wave keeps the order
    const int j = base + threadIdx.x;
    const double a = j < rows ? arow[j] : 0.0;
    const bool live = a != 0.0;  // a NaN is kept
    const unsigned long long mask = __ballot(live);
    if (live) {
      const int pos = n + __popcll(mask & ((1ull << threadIdx.x) - 1ull));
      idx[(long)i * rows + pos] = j;
      val[(long)i * rows + pos] = a;
    }
    n += __popcll(mask);
  }
  if (threadIdx.x == 0) cnt[i] = n;
}

// step n = 1 .. max_steps + 1 (the last one only closes the count)
__global__ __launch_bounds__(256) void lame_step_kernel(int n, int rows, int K, double lambda, int max_steps, double tol,
                                                         const double* __restrict__ val, const int* __restrict__ idx,
                                                         const int* __restrict__ cnt, const double* __restrict__ u,
                                                         const double* __restrict__ yprev, double* __restrict__ ynext,
                                                         float* __restrict__ Y, int ldy, const double* __restrict__ eprev,
                                                         double* __restrict__ enext, double* energy, int* __restrict__ steps,
                                                         int* stop) {
  __shared__ double redd[16];
  const int st = stop[0];
  if (st != 0 && st < n - 1) return;  // the rule fired in an earlier launch
  if (n >= 2) {
    const double E = tta_partial_sum(eprev, rows, redd);  // E_(n-1): the same bits in every workgroup
    bool last = n - 1 == max_steps;
    if (n >= 3 && tol > 0.0) {
      const double Ep = energy[n - 3];  // E_(n-2), recorded by the launch before this one
      last = last || fabs(E - Ep) <= tol * fabs(Ep);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      energy[n - 2] = E;
      if (last) {
        steps[0] = n - 1;
        stop[0] = n - 1;
      }
    }
    if (last) return;
  }
  const int i = blockIdx.x;
  const int ni = cnt[i];
  const double* vi = val + (long)i * rows;
  const int* ji = idx + (long)i * rows;
  const double* ui = u + (long)i * K;
  double* ti = ynext + (long)i * K;
  double m = -INFINITY;
  for (int c = threadIdx.x; c < K; c += 256) {
    double s = 0.0;
    for (int e = 0; e < ni; ++e) s += vi[e] * yprev[(long)ji[e] * K + c];  // ascending j
    const double tc = ui[c] + lambda * s;
    ti[c] = tc;  // read back below by the thread that wrote it
    m = fmax(m, tc);
  }
  m = lame_block_max_d(m, redd);
  double s = 0.0;
  for (int c = threadIdx.x; c < K; c += 256) s += exp(ti[c] - m);
  s = block_sum_d(s, redd);
  double e = 0.0;
  for (int c = threadIdx.x; c < K; c += 256) {
    const double tc = ti[c];
    const double y = exp(tc - m) / s;
    e += y * (log(fmax(y, 1e-20)) - tc);  // -u - lambda A Y^(n-1) is -tc
    ti[c] = y;
    Y[(long)i * ldy + c] = (float)y;
  }
  e = block_sum_d(e, redd);
  if (threadIdx.x == 0) enext[i] = e;
}

extern "C" int stil_lame_rows(const float* Z, int ld, int rows, int K, const int* nbr, const float* wts, int k, float lambda, int max_steps,
                              float tol, double* lse, float* p, int ldp, float* Y, int ldy, double* energy, int* steps, double* ws,
                              void* stream) {
  STIL_REQUIRE(Z && nbr && wts && lse && p && Y && energy && steps && ws, "stil_lame_rows: null pointer");
  STIL_REQUIRE(rows >= 1 && K >= 1 && k >= 1 && ld >= K, "stil_lame_rows: bad shape rows=%d K=%d k=%d ld=%d", rows, K, k, ld);
  STIL_REQUIRE(rows <= STIL_LAME_MAX_ROWS, "stil_lame_rows: rows=%d exceeds STIL_LAME_MAX_ROWS=%d", rows, STIL_LAME_MAX_ROWS);
  STIL_REQUIRE(ldp >= K && ldy >= K, "stil_lame_rows: ldp=%d ldy=%d < K=%d", ldp, ldy, K);
  STIL_REQUIRE(lambda >= 0.0f && lambda <= 3.402823466e38f, "stil_lame_rows: lambda=%g is not finite and non-negative", (double)lambda);
  STIL_REQUIRE(tol >= 0.0f && tol <= 3.402823466e38f, "stil_lame_rows: tol=%g is not finite and non-negative", (double)tol);
  STIL_REQUIRE(max_steps >= 1, "stil_lame_rows: max_steps=%d < 1", max_steps);
  hipStream_t s = (hipStream_t)stream;
  const long rr = (long)rows * rows, rk = (long)rows * K;
  double* val = ws;
  int* idx = (int*)(ws + rr);
  double* u = ws + 2 * rr;
  double* yb[2] = {u + rk, u + 2 * rk};
  double* eb[2] = {u + 3 * rk, u + 3 * rk + rows};
  int* cnt = (int*)(u + 3 * rk + 2 * (long)rows);
  int* stop = (int*)(u + 3 * rk + 3 * (long)rows);
  hipLaunchKernelGGL(lame_rows_kernel, dim3(rows), dim3(256), 0, s, Z, ld, K, lse, p, ldp, u, yb[0], stop);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(lame_graph_kernel, dim3(rows), dim3(256), 0, s, nbr, wts, k, rows, val, idx, cnt);
  STIL_LAUNCH_CHECK();
  for (long n = 1; n <= (long)max_steps + 1; ++n) {
    hipLaunchKernelGGL(lame_step_kernel, dim3(rows), dim3(256), 0, s, (int)n, rows, K, (double)lambda, max_steps, (double)tol, (const double*)val,
                       (const int*)idx, (const int*)cnt, (const double*)u, (const double*)yb[(n - 1) & 1], yb[n & 1], Y, ldy,
                       (const double*)eb[(n - 1) & 1], eb[n & 1], energy, steps, stop);
    STIL_LAUNCH_CHECK();
  }
  return STIL_OK;
}
