// Test-time BatchNorm with a source-statistics prior (Schneider et al., NeurIPS 2020): the layer normalises by
//   mu = (1 - rho) running_mean + rho mean_batch,   v = (1 - rho) running_var + rho var_batch (biased),   rho = B / (N + B).
// C ABI in include/stil_bnprior.h.  Per-channel work only: the wide passes (pilot, partial sums, tile sums, apply, dx) are the
// kernels of bn.hip, launched as they are; only the short kernels that FINISH a reduction are new.  They form the batch mean
// and variance exactly as their bn.hip counterparts do, blend them with the source statistics in double, and write the same
// [4, C] statistics block plus delta = (mu - mean_batch) * rstd; the backward finals fold rho and delta into the coefficient
// triple of bn_bwd_dx_kernel:  dx = gamma rstd [ g - rho (k2 + delta k3) - rho k3 xhat ],  k2 = mean g, k3 = mean g xhat.
// rho == 1 is today's BatchNorm: those calls run the bn.hip entry points themselves (NULL running buffers) and clear delta.
// The running buffers are read-only here, nothing is read back to the host, every sum keeps bn.hip's fixed order.

__device__ __forceinline__ void bn_prior_write_stats(int c, int C, double mean_b, double var_b, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ rmean,
                                                     const float* __restrict__ rvar, double rho, float eps,
                                                     float* __restrict__ stats, float* __restrict__ delta) {
  const double mu = (1.0 - rho) * (double)rmean[c] + rho * mean_b;
  const double v = (1.0 - rho) * (double)rvar[c] + rho * var_b;
  const double r = 1.0 / sqrt(v + (double)eps);
  const float muf = (float)mu, rstd = (float)r;
  stats[c] = muf; stats[C + c] = rstd; stats[2 * C + c] = gamma[c] * rstd; stats[3 * C + c] = beta[c];
  // from the ROUNDED mean and rstd, the ones every consumer forms xhat with: xhat_i + delta is then (x_i - mean_batch) * rstd to
  // rounding, and the two terms of the backward that cancel (rho k3 delta, rho k3 xhat_i) cancel on the device as well
  delta[c] = (float)(((double)muf - mean_b) * (double)rstd);
}

// two-pass statistics (bn_pilot_kernel + bn_stats_partial_kernel): the final of bn_stats_final_kernel, blended
__global__ __launch_bounds__(256) void bn_prior_stats_final_kernel(const float* __restrict__ Kp, const float* __restrict__ part, int nch, int M, int C,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    const float* __restrict__ rmean, const float* __restrict__ rvar, float rho,
                                                                    float* __restrict__ stats, float* __restrict__ delta, float eps) {
  __shared__ float sh[2 * 8 * 32];
  int c;
  float tot[2];
  if (!chunk_reduce<8, 2>(part, nch, C, sh, c, tot)) return;
  const float s1 = tot[0], s2 = tot[1];
  const float invM = 1.f / (float)M;
  const float d = s1 * invM;
  const float mean = Kp[c] + d;
  float var = s2 * invM - d * d;
  var = fmaxf(var, 0.f);
  bn_prior_write_stats(c, C, (double)mean, (double)var, gamma, beta, rmean, rvar, (double)rho, eps, stats, delta);
}

// per-tile partials of the conv GEMM's epilogue (bn_tiles_stage1_kernel): the final of bn_tiles_stage2_kernel, blended.  Mean and
// variance stay in double until the blend.
__device__ __forceinline__ void bn_prior_tiles_finish(int c, int C, double s1, double s2, double s3, int M, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ rmean,
                                                      const float* __restrict__ rvar, float rho, float eps, float* __restrict__ stats,
                                                      float* __restrict__ delta) {
  const double mean_d = s1 / (double)M;
  const double m2 = s3 + (s2 - s1 * mean_d);
  const double var_d = fmax(m2 / (double)M, 0.0);
  bn_prior_write_stats(c, C, mean_d, var_d, gamma, beta, rmean, rvar, (double)rho, eps, stats, delta);
}

__global__ __launch_bounds__(256) void bn_prior_tiles_stage2_kernel(const double* __restrict__ part, int nsplit, int M, int C,
                                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                     const float* __restrict__ rmean, const float* __restrict__ rvar, float rho,
                                                                     float* __restrict__ stats, float* __restrict__ delta, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int k = 0; k < nsplit; ++k) {
    s1 += part[((long)0 * nsplit + k) * C + c]; s2 += part[((long)1 * nsplit + k) * C + c]; s3 += part[((long)2 * nsplit + k) * C + c];
  }
  bn_prior_tiles_finish(c, C, s1, s2, s3, M, gamma, beta, rmean, rvar, rho, eps, stats, delta);
}

// one launch when a single split covers every tile (bn_tiles_fused_kernel's sums in its order)
__global__ __launch_bounds__(256) void bn_prior_tiles_fused_kernel(const float* __restrict__ ts, int nt, int tile_rows, int M, int C,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    const float* __restrict__ rmean, const float* __restrict__ rvar, float rho,
                                                                    float* __restrict__ stats, float* __restrict__ delta, float eps) {
  __shared__ double sh[3 * 8 * 32];
  const int cl = threadIdx.x & 31, lane = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (c < C)
    for (int t = lane; t < nt; t += 8) {
      const double n = (double)min(tile_rows, M - t * tile_rows);
      const double m = (double)ts[((long)t * 2) * C + c];
      s1 += n * m; s2 += n * m * m; s3 += (double)ts[((long)t * 2 + 1) * C + c];
    }
  sh[lane * 32 + cl] = s1; sh[256 + lane * 32 + cl] = s2; sh[512 + lane * 32 + cl] = s3;
  __syncthreads();
  if (lane != 0 || c >= C) return;
  double a = 0.0, b = 0.0, d = 0.0;
  for (int l = 0; l < 8; ++l) { a += sh[l * 32 + cl]; b += sh[256 + l * 32 + cl]; d += sh[512 + l * 32 + cl]; }
  bn_prior_tiles_finish(c, C, a, b, d, M, gamma, beta, rmean, rvar, rho, eps, stats, delta);
}

// ---- backward finals: dgamma / dbeta as bn.hip writes them; coef[0] = gamma*rstd, [1] = rho (k2 + delta k3), [2] = rho k3
__device__ __forceinline__ void bn_prior_bwd_write(int c, int C, float s1, float s2, int M, const float* __restrict__ gamma,
                                                   const float* __restrict__ stats, const float* __restrict__ delta, float rho,
                                                   float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ coef,
                                                   int accumulate) {
  if (dbeta) dbeta[c] = accumulate ? dbeta[c] + s1 : s1;
  if (dgamma) dgamma[c] = accumulate ? dgamma[c] + s2 : s2;
  const double k2 = (double)s1 / (double)M, k3 = (double)s2 / (double)M;
  coef[c] = gamma[c] * stats[C + c];
  coef[C + c] = (float)((double)rho * (k2 + (double)delta[c] * k3));
  coef[2 * C + c] = (float)((double)rho * k3);
}

__global__ __launch_bounds__(256) void bn_prior_bwd_final_kernel(const float* __restrict__ part, int nch, int M, int C,
                                                                  const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                  const float* __restrict__ delta, float rho, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta, float* __restrict__ coef, int accumulate) {
  __shared__ float sh[2 * 8 * 32];
  int c;
  float tot[2];
  if (!chunk_reduce<8, 2>(part, nch, C, sh, c, tot)) return;
  bn_prior_bwd_write(c, C, tot[0], tot[1], M, gamma, stats, delta, rho, dgamma, dbeta, coef, accumulate);
}

// 32 lanes x 8 column quads, one dwordx4 per lane and chunk (bn_bwd_final4_kernel's sums in its order)
__global__ __launch_bounds__(256) void bn_prior_bwd_final4_kernel(const float* __restrict__ part, int nch, int M, int C,
                                                                   const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                   const float* __restrict__ delta, float rho, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta, float* __restrict__ coef, int accumulate) {
  __shared__ float4 sh[2 * 32 * 8];
  const int cq = threadIdx.x & 7, lane = threadIdx.x >> 3;
  const int c = (blockIdx.x * 8 + cq) * 4;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  if (c < C)
    for (int i = lane; i < nch; i += 32) {
      const float4 u = *reinterpret_cast<const float4*>(part + (long)i * C + c);
      const float4 v = *reinterpret_cast<const float4*>(part + (long)(nch + i) * C + c);
      a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
      b.x += v.x; b.y += v.y; b.z += v.z; b.w += v.w;
    }
  sh[lane * 8 + cq] = a; sh[256 + lane * 8 + cq] = b;
  __syncthreads();
  if (lane != 0 || c >= C) return;
  for (int l = 1; l < 32; ++l) {
    const float4 u = sh[l * 8 + cq], v = sh[256 + l * 8 + cq];
    a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
    b.x += v.x; b.y += v.y; b.z += v.z; b.w += v.w;
  }
  const float s1[4] = {a.x, a.y, a.z, a.w}, s2[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) bn_prior_bwd_write(c + j, C, s1[j], s2[j], M, gamma, stats, delta, rho, dgamma, dbeta, coef, accumulate);
}

// per-tile sums of the input-gradient GEMM's epilogue (bn_bwd_tiles_stage1_kernel): the final of bn_bwd_tiles_final_kernel
__global__ __launch_bounds__(256) void bn_prior_bwd_tiles_final_kernel(const double* __restrict__ part, int nsplit, int M, int C,
                                                                        const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                        const float* __restrict__ delta, float rho, float* __restrict__ dgamma,
                                                                        float* __restrict__ dbeta, float* __restrict__ coef, int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int k = 0; k < nsplit; ++k) { a += part[((long)0 * nsplit + k) * C + c]; b += part[((long)1 * nsplit + k) * C + c]; }
  bn_prior_bwd_write(c, C, (float)a, (float)b, M, gamma, stats, delta, rho, dgamma, dbeta, coef, accumulate);
}

__global__ __launch_bounds__(256) void bn_prior_bwd_tiles_fused_kernel(const float* __restrict__ ts, int nt, int M, int C,
                                                                        const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                        const float* __restrict__ delta, float rho, float* __restrict__ dgamma,
                                                                        float* __restrict__ dbeta, float* __restrict__ coef, int accumulate) {
  __shared__ double sh[2 * 8 * 32];
  const int cl = threadIdx.x & 31, lane = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  double s1 = 0.0, s2 = 0.0;
  if (c < C)
    for (int t = lane; t < nt; t += 8) {
      s1 += (double)ts[((long)t * 2) * C + c];
      s2 += (double)ts[((long)t * 2 + 1) * C + c];
    }
  sh[lane * 32 + cl] = s1; sh[256 + lane * 32 + cl] = s2;
  __syncthreads();
  if (lane != 0 || c >= C) return;
  double a = 0.0, b = 0.0;
  for (int l = 0; l < 8; ++l) { a += sh[l * 32 + cl]; b += sh[256 + l * 32 + cl]; }
  bn_prior_bwd_write(c, C, (float)a, (float)b, M, gamma, stats, delta, rho, dgamma, dbeta, coef, accumulate);
}

// ---------------------------------------------------------------------------------------
static inline bool bn_prior_rho_ok(float rho) { return rho >= 0.f && rho <= 1.f; }   // false for NaN

static inline int bn_prior_clear_delta(float* delta, int C, hipStream_t s) {
  if (hipMemsetAsync(delta, 0, (size_t)C * sizeof(float), s) != hipSuccess) {
    stil_set_error("stil_bn_prior: clearing delta failed: %s", hipGetErrorString(hipGetLastError()));
    return STIL_EHIP;
  }
  return STIL_OK;
}

extern "C" int stil_bn_prior_fwd(const float* x, const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, float rho, const float* resid, float* z, float* stats, float* delta,
                                 int M, int C, int relu, float eps, float* workspace, size_t workspace_bytes, void* stream) {
  STIL_REQUIRE(x && gamma && beta && running_mean && running_var && z && stats && delta && workspace, "stil_bn_prior_fwd: null pointer");
  STIL_REQUIRE(bn_prior_rho_ok(rho), "stil_bn_prior_fwd: rho=%g must lie in [0, 1]", (double)rho);
  int ct = pick_ctile(C);
  STIL_REQUIRE(M > 0 && ct != 0, "stil_bn_prior_fwd: M=%d must be positive and C=%d a multiple of 64", M, C);
  int nch = bn_chunks(M, C, ct);
  STIL_REQUIRE(workspace_bytes >= ((size_t)2 * nch + 1) * C * sizeof(float), "stil_bn_prior_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (rho == 1.f) {   // the batch statistics alone: today's forward
    int rc = stil_bn_train_fwd(x, gamma, beta, nullptr, nullptr, nullptr, resid, z, stats, M, C, relu, eps, 0.f, workspace,
                               workspace_bytes, stream);
    return rc != STIL_OK ? rc : bn_prior_clear_delta(delta, C, s);
  }
  float* pilot = workspace + (size_t)2 * nch * C;
  int rpc = cdiv(M, nch);
  hipLaunchKernelGGL(bn_pilot_kernel, dim3(cdiv(C, 32)), dim3(256), 0, s, x, pilot, M, C);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(C / ct, nch), dim3(256), 0, s, x, pilot, workspace, M, C, ct, rpc);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_prior_stats_final_kernel, dim3(cdiv(C, 32)), dim3(256), 0, s, pilot, workspace, nch, M, C, gamma, beta,
                     running_mean, running_var, rho, stats, delta, eps);
  STIL_LAUNCH_CHECK();
  long total4 = (long)M * C / 4;
  int grid = (int)((total4 + 255) / 256 < 8192 ? (total4 + 255) / 256 : 8192);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(grid), dim3(256), 0, s, x, stats, resid, (const float*)nullptr, z, total4, C, relu);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_bn_prior_fwd_tiles(const float* x, const float* tilestats, int tile_rows, const float* gamma, const float* beta,
                                       const float* running_mean, const float* running_var, float rho, const float* resid,
                                       const float* resid_stats, float* z, float* stats, float* delta, int M, int C, int relu,
                                       float eps, void* workspace, size_t workspace_bytes, void* stream) {
  STIL_REQUIRE(x && tilestats && gamma && beta && running_mean && running_var && stats && delta && workspace,
               "stil_bn_prior_fwd_tiles: null pointer");
  STIL_REQUIRE(bn_prior_rho_ok(rho), "stil_bn_prior_fwd_tiles: rho=%g must lie in [0, 1]", (double)rho);
  STIL_REQUIRE(z || !resid, "stil_bn_prior_fwd_tiles: statistics-only call (z == NULL) cannot take a residual");
  STIL_REQUIRE(!resid_stats || resid, "stil_bn_prior_fwd_tiles: resid_stats without resid");
  STIL_REQUIRE(tile_rows > 0 && M > 0 && C > 0 && C % 4 == 0, "stil_bn_prior_fwd_tiles: bad shape M=%d C=%d tile_rows=%d", M, C, tile_rows);
  STIL_REQUIRE(workspace_bytes >= stil_bn_tiles_workspace_bytes(M, C, tile_rows) && ((uintptr_t)workspace % 8) == 0,
               "stil_bn_prior_fwd_tiles: workspace too small or not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (rho == 1.f) {
    int rc = stil_bn_train_fwd_tiles(x, tilestats, tile_rows, gamma, beta, nullptr, nullptr, nullptr, resid, resid_stats, z, stats, M, C,
                                     relu, eps, 0.f, workspace, workspace_bytes, stream);
    return rc != STIL_OK ? rc : bn_prior_clear_delta(delta, C, s);
  }
  const int nt = cdiv(M, tile_rows), nsplit = bn_tiles_nsplit(nt);
  if (nsplit == 1) {
    hipLaunchKernelGGL(bn_prior_tiles_fused_kernel, dim3(cdiv(C, 32)), dim3(256), 0, s, tilestats, nt, tile_rows, M, C, gamma, beta,
                       running_mean, running_var, rho, stats, delta, eps);
    STIL_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(bn_tiles_stage1_kernel, dim3(cdiv(C, 32), nsplit), dim3(256), 0, s, tilestats, nt, tile_rows, M, C,
                       cdiv(nt, nsplit), (double*)workspace);
    STIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_prior_tiles_stage2_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, (const double*)workspace, nsplit, M, C, gamma,
                       beta, running_mean, running_var, rho, stats, delta, eps);
    STIL_LAUNCH_CHECK();
  }
  if (!z) return STIL_OK;   // statistics only: the consumer applies them while it stages its operand
  long total4 = (long)M * C / 4;
  int grid = (int)((total4 + 255) / 256 < 8192 ? (total4 + 255) / 256 : 8192);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(grid), dim3(256), 0, s, x, stats, resid, resid_stats, z, total4, C, relu);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_bn_prior_bwd(const float* dz, const float* z, const float* x, const float* gamma, const float* stats,
                                 const float* delta, float rho, float* dx, float* gout, float* dgamma, float* dbeta, float* coef,
                                 int M, int C, int relu, int accumulate, float* workspace, size_t workspace_bytes, void* stream) {
  STIL_REQUIRE(dz && x && gamma && stats && delta && dx && coef && workspace, "stil_bn_prior_bwd: null pointer");
  STIL_REQUIRE(bn_prior_rho_ok(rho), "stil_bn_prior_bwd: rho=%g must lie in [0, 1]", (double)rho);
  STIL_REQUIRE(relu >= 0 && relu <= 2 && (relu != 1 || z), "stil_bn_prior_bwd: relu must be 0, 1 (needs z) or 2");
  int ct = pick_ctile(C);
  STIL_REQUIRE(M > 0 && ct != 0, "stil_bn_prior_bwd: M=%d must be positive and C=%d a multiple of 64", M, C);
  int nch = bn_chunks(M, C, ct);
  STIL_REQUIRE(workspace_bytes >= (size_t)2 * nch * C * sizeof(float), "stil_bn_prior_bwd: workspace too small");
  if (rho == 1.f)
    return stil_bn_train_bwd(dz, z, x, gamma, stats, dx, gout, dgamma, dbeta, coef, M, C, relu, accumulate, workspace, workspace_bytes,
                             stream);
  int rpc = cdiv(M, nch);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(C / ct, nch), dim3(256), 0, s, dz, z, x, stats, gout, workspace, M, C, ct, rpc, relu);
  STIL_LAUNCH_CHECK();
  if (((uintptr_t)workspace % 16) == 0)
    hipLaunchKernelGGL(bn_prior_bwd_final4_kernel, dim3(cdiv(C, 32)), dim3(256), 0, s, workspace, nch, M, C, gamma, stats, delta, rho,
                       dgamma, dbeta, coef, accumulate);
  else
    hipLaunchKernelGGL(bn_prior_bwd_final_kernel, dim3(cdiv(C, 32)), dim3(256), 0, s, workspace, nch, M, C, gamma, stats, delta, rho,
                       dgamma, dbeta, coef, accumulate);
  STIL_LAUNCH_CHECK();
  long total4 = (long)M * C / 4;
  int grid = (int)((total4 + 255) / 256 < 8192 ? (total4 + 255) / 256 : 8192);
  hipLaunchKernelGGL(bn_bwd_dx_kernel, dim3(grid), dim3(256), 0, s, gout ? gout : dz, z, x, stats, coef, dx, total4, C, gout ? 0 : relu);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_bn_prior_bwd_tiles(const float* dz, const float* z, const float* x, const float* gamma, const float* stats,
                                       const float* delta, float rho, const float* tilestats, int ntiles, float* dx, float* dgamma,
                                       float* dbeta, float* coef, int M, int C, int relu, int accumulate, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  STIL_REQUIRE(dz && x && gamma && stats && delta && tilestats && dx && coef && workspace, "stil_bn_prior_bwd_tiles: null pointer");
  STIL_REQUIRE(bn_prior_rho_ok(rho), "stil_bn_prior_bwd_tiles: rho=%g must lie in [0, 1]", (double)rho);
  STIL_REQUIRE(relu >= 0 && relu <= 2 && (relu != 1 || z), "stil_bn_prior_bwd_tiles: relu must be 0, 1 (needs z) or 2");
  STIL_REQUIRE(ntiles > 0 && M > 0 && C > 0 && C % 4 == 0, "stil_bn_prior_bwd_tiles: bad shape M=%d C=%d ntiles=%d", M, C, ntiles);
  STIL_REQUIRE(workspace_bytes >= stil_bn_bwd_tiles_workspace_bytes(ntiles, C) && ((uintptr_t)workspace % 8) == 0,
               "stil_bn_prior_bwd_tiles: workspace too small or not 8-byte aligned");
  if (rho == 1.f)
    return stil_bn_train_bwd_tiles(dz, z, x, gamma, stats, tilestats, ntiles, dx, dgamma, dbeta, coef, M, C, relu, accumulate, workspace,
                                   workspace_bytes, stream);
  hipStream_t s = (hipStream_t)stream;
  const int nsplit = bn_bwd_tiles_nsplit(ntiles);
  if (nsplit == 1) {
    hipLaunchKernelGGL(bn_prior_bwd_tiles_fused_kernel, dim3(cdiv(C, 32)), dim3(256), 0, s, tilestats, ntiles, M, C, gamma, stats, delta,
                       rho, dgamma, dbeta, coef, accumulate);
    STIL_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(bn_bwd_tiles_stage1_kernel, dim3(cdiv(C, 32), nsplit), dim3(256), 0, s, tilestats, ntiles, C, cdiv(ntiles, nsplit),
                       (double*)workspace);
    STIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_prior_bwd_tiles_final_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, (const double*)workspace, nsplit, M, C, gamma,
                       stats, delta, rho, dgamma, dbeta, coef, accumulate);
    STIL_LAUNCH_CHECK();
  }
  long total4 = (long)M * C / 4;
  int grid = (int)((total4 + 255) / 256 < 8192 ? (total4 + 255) / 256 : 8192);
  hipLaunchKernelGGL(bn_bwd_dx_kernel, dim3(grid), dim3(256), 0, s, dz, z, x, stats, coef, dx, total4, C, relu);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
