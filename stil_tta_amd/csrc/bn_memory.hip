// Test-time BatchNorm on a running estimate of the TARGET statistics that the adaptation owns (RoTTA's robust BatchNorm, Yuan
// et al., CVPR 2023; DUA, Mirza et al., CVPR 2022).  C ABI in stil_bnmemory.h (beside this file).  The forward of bn_prior.hip
// with the [C] pair (mem_mean, mem_var) in place of the running buffers, plus, per channel,
//   m' = (1 - alpha) m + alpha mean_batch,   s' = (1 - alpha) s + alpha c var_batch,   c = M / (M - 1) if unbiased and M > 1 else 1
// written to a SECOND pair (mem_mean_out, mem_var_out) by the one thread that finishes the channel's reduction: the finals below
// are bn_prior.hip's three with that one extra write.  The normalisation reads m, s alone, so a layer's forwards within one step all
// see the same estimate whichever of them writes m', s'.  m', s' are formed in double from the batch mean and variance the blend
// uses and rounded once.  No wide pass is new: pilot, partial sums, tile stage 1 and apply are bn.hip's kernels as they are.
// NULL outputs: the call IS stil_bn_prior_fwd(_tiles).  rho == 1: z / stats come from stil_bn_train_fwd(_tiles) itself (identical
// bits) and delta is cleared, as in bn_prior.hip; the final then runs once more over the partial sums that call left in the
// workspace (kStats = false) for the memory alone.

__device__ __forceinline__ void bn_memory_write(int c, double mean_b, double var_b, int M, const float* __restrict__ mem_mean,
                                                const float* __restrict__ mem_var, float* __restrict__ mem_mean_out,
                                                float* __restrict__ mem_var_out, double alpha, int unbiased) {
  const double corr = (unbiased && M > 1) ? (double)M / (double)(M - 1) : 1.0;
  mem_mean_out[c] = (float)((1.0 - alpha) * (double)mem_mean[c] + alpha * mean_b);
  mem_var_out[c] = (float)((1.0 - alpha) * (double)mem_var[c] + alpha * corr * var_b);
}

// bn_prior_stats_final_kernel + the memory
template <bool kStats>
__global__ __launch_bounds__(256) void bn_memory_stats_final_kernel(const float* __restrict__ Kp, const float* __restrict__ part, int nch, int M, int C,
                                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                     const float* __restrict__ mem_mean, const float* __restrict__ mem_var,
                                                                     float* __restrict__ mem_mean_out, float* __restrict__ mem_var_out,
                                                                     float alpha, int unbiased, float rho, float* __restrict__ stats,
                                                                     float* __restrict__ delta, float eps) {
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
  if (kStats) bn_prior_write_stats(c, C, (double)mean, (double)var, gamma, beta, mem_mean, mem_var, (double)rho, eps, stats, delta);
  bn_memory_write(c, (double)mean, (double)var, M, mem_mean, mem_var, mem_mean_out, mem_var_out, (double)alpha, unbiased);
}

// bn_prior_tiles_finish + the memory
template <bool kStats>
__device__ __forceinline__ void bn_memory_tiles_finish(int c, int C, double s1, double s2, double s3, int M, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ mem_mean,
                                                       const float* __restrict__ mem_var, float* __restrict__ mem_mean_out,
                                                       float* __restrict__ mem_var_out, float alpha, int unbiased, float rho, float eps,
                                                       float* __restrict__ stats, float* __restrict__ delta) {
  const double mean_d = s1 / (double)M;
  const double m2 = s3 + (s2 - s1 * mean_d);
  const double var_d = fmax(m2 / (double)M, 0.0);
  if (kStats) bn_prior_write_stats(c, C, mean_d, var_d, gamma, beta, mem_mean, mem_var, (double)rho, eps, stats, delta);
  bn_memory_write(c, mean_d, var_d, M, mem_mean, mem_var, mem_mean_out, mem_var_out, (double)alpha, unbiased);
}

template <bool kStats>
__global__ __launch_bounds__(256) void bn_memory_tiles_stage2_kernel(const double* __restrict__ part, int nsplit, int M, int C,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      const float* __restrict__ mem_mean, const float* __restrict__ mem_var,
                                                                      float* __restrict__ mem_mean_out, float* __restrict__ mem_var_out,
                                                                      float alpha, int unbiased, float rho, float* __restrict__ stats,
                                                                      float* __restrict__ delta, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int k = 0; k < nsplit; ++k) {
    s1 += part[((long)0 * nsplit + k) * C + c]; s2 += part[((long)1 * nsplit + k) * C + c]; s3 += part[((long)2 * nsplit + k) * C + c];
  }
  bn_memory_tiles_finish<kStats>(c, C, s1, s2, s3, M, gamma, beta, mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, rho, eps,
                                 stats, delta);
}

template <bool kStats>
__global__ __launch_bounds__(256) void bn_memory_tiles_fused_kernel(const float* __restrict__ ts, int nt, int tile_rows, int M, int C,
                                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                     const float* __restrict__ mem_mean, const float* __restrict__ mem_var,
                                                                     float* __restrict__ mem_mean_out, float* __restrict__ mem_var_out,
                                                                     float alpha, int unbiased, float rho, float* __restrict__ stats,
                                                                     float* __restrict__ delta, float eps) {
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
  bn_memory_tiles_finish<kStats>(c, C, a, b, d, M, gamma, beta, mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, rho, eps,
                                 stats, delta);
}

// ---------------------------------------------------------------------------------------
static inline bool bn_memory_overlap(const float* a, const float* b, int C) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, n = (uintptr_t)C * sizeof(float);
  return x < y + n && y < x + n;
}

// what both entries check of the memory's own arguments; `update` <- both outputs given
static inline int bn_memory_check(const char* who, const float* mem_mean, const float* mem_var, const float* mem_mean_out,
                                  const float* mem_var_out, float alpha, int unbiased, int C, bool* update) {
  STIL_REQUIRE(alpha >= 0.f && alpha <= 1.f, "%s: alpha=%g must lie in [0, 1]", who, (double)alpha);   // false for NaN
  STIL_REQUIRE(unbiased == 0 || unbiased == 1, "%s: unbiased=%d must be 0 or 1", who, unbiased);
  STIL_REQUIRE((mem_mean_out == nullptr) == (mem_var_out == nullptr), "%s: one memory output without the other", who);
  *update = mem_mean_out != nullptr;
  if (*update && mem_mean && mem_var && C > 0)
    STIL_REQUIRE(!bn_memory_overlap(mem_mean_out, mem_mean, C) && !bn_memory_overlap(mem_mean_out, mem_var, C) &&
                     !bn_memory_overlap(mem_var_out, mem_mean, C) && !bn_memory_overlap(mem_var_out, mem_var, C) &&
                     !bn_memory_overlap(mem_mean_out, mem_var_out, C),
                 "%s: the memory outputs alias the memory read or each other", who);
  return STIL_OK;
}

extern "C" int stil_bn_memory_fwd(const float* x, const float* gamma, const float* beta, const float* mem_mean, const float* mem_var,
                                  float* mem_mean_out, float* mem_var_out, float alpha, int unbiased, float rho, const float* resid,
                                  float* z, float* stats, float* delta, int M, int C, int relu, float eps, float* workspace,
                                  size_t workspace_bytes, void* stream) {
  bool update = false;
  int rc = bn_memory_check("stil_bn_memory_fwd", mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, C, &update);
  if (rc != STIL_OK) return rc;
  if (!update)
    return stil_bn_prior_fwd(x, gamma, beta, mem_mean, mem_var, rho, resid, z, stats, delta, M, C, relu, eps, workspace, workspace_bytes, stream);
  STIL_REQUIRE(x && gamma && beta && mem_mean && mem_var && z && stats && delta && workspace, "stil_bn_memory_fwd: null pointer");
  STIL_REQUIRE(bn_prior_rho_ok(rho), "stil_bn_memory_fwd: rho=%g must lie in [0, 1]", (double)rho);
  int ct = pick_ctile(C);
  STIL_REQUIRE(M > 0 && ct != 0, "stil_bn_memory_fwd: M=%d must be positive and C=%d a multiple of 64", M, C);
  int nch = bn_chunks(M, C, ct);
  STIL_REQUIRE(workspace_bytes >= ((size_t)2 * nch + 1) * C * sizeof(float), "stil_bn_memory_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* pilot = workspace + (size_t)2 * nch * C;
  if (rho == 1.f) {   // the batch statistics alone normalise: today's forward, then the final once more for the memory
    rc = stil_bn_train_fwd(x, gamma, beta, nullptr, nullptr, nullptr, resid, z, stats, M, C, relu, eps, 0.f, workspace, workspace_bytes,
                           stream);
    if (rc == STIL_OK) rc = bn_prior_clear_delta(delta, C, s);
    if (rc != STIL_OK) return rc;
    hipLaunchKernelGGL(bn_memory_stats_final_kernel<false>, dim3(cdiv(C, 32)), dim3(256), 0, s, pilot, workspace, nch, M, C, gamma, beta,
                       mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, rho, stats, delta, eps);
    STIL_LAUNCH_CHECK();
    return STIL_OK;
  }
  int rpc = cdiv(M, nch);
  hipLaunchKernelGGL(bn_pilot_kernel, dim3(cdiv(C, 32)), dim3(256), 0, s, x, pilot, M, C);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(C / ct, nch), dim3(256), 0, s, x, pilot, workspace, M, C, ct, rpc);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_memory_stats_final_kernel<true>, dim3(cdiv(C, 32)), dim3(256), 0, s, pilot, workspace, nch, M, C, gamma, beta,
                     mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, rho, stats, delta, eps);
  STIL_LAUNCH_CHECK();
  long total4 = (long)M * C / 4;
  int grid = (int)((total4 + 255) / 256 < 8192 ? (total4 + 255) / 256 : 8192);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(grid), dim3(256), 0, s, x, stats, resid, (const float*)nullptr, z, total4, C, relu);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

// the memory's share of the tile path: the final (one launch, or stage 1 + stage 2) over the per-tile partials
template <bool kStats>
static int bn_memory_tiles_final(const float* tilestats, int tile_rows, const float* gamma, const float* beta, const float* mem_mean,
                                 const float* mem_var, float* mem_mean_out, float* mem_var_out, float alpha, int unbiased, float rho,
                                 float* stats, float* delta, int M, int C, float eps, void* workspace, bool stage1_done, hipStream_t s) {
  const int nt = cdiv(M, tile_rows), nsplit = bn_tiles_nsplit(nt);
  if (nsplit == 1) {
    hipLaunchKernelGGL(bn_memory_tiles_fused_kernel<kStats>, dim3(cdiv(C, 32)), dim3(256), 0, s, tilestats, nt, tile_rows, M, C, gamma, beta,
                       mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, rho, stats, delta, eps);
    STIL_LAUNCH_CHECK();
    return STIL_OK;
  }
  if (!stage1_done) {
    hipLaunchKernelGGL(bn_tiles_stage1_kernel, dim3(cdiv(C, 32), nsplit), dim3(256), 0, s, tilestats, nt, tile_rows, M, C, cdiv(nt, nsplit),
                       (double*)workspace);
    STIL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(bn_memory_tiles_stage2_kernel<kStats>, dim3(cdiv(C, 256)), dim3(256), 0, s, (const double*)workspace, nsplit, M, C,
                     gamma, beta, mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, rho, stats, delta, eps);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_bn_memory_fwd_tiles(const float* x, const float* tilestats, int tile_rows, const float* gamma, const float* beta,
                                        const float* mem_mean, const float* mem_var, float* mem_mean_out, float* mem_var_out, float alpha,
                                        int unbiased, float rho, const float* resid, const float* resid_stats, float* z, float* stats,
                                        float* delta, int M, int C, int relu, float eps, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  bool update = false;
  int rc = bn_memory_check("stil_bn_memory_fwd_tiles", mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, C, &update);
  if (rc != STIL_OK) return rc;
  if (!update)
    return stil_bn_prior_fwd_tiles(x, tilestats, tile_rows, gamma, beta, mem_mean, mem_var, rho, resid, resid_stats, z, stats, delta, M, C,
                                   relu, eps, workspace, workspace_bytes, stream);
  STIL_REQUIRE(x && tilestats && gamma && beta && mem_mean && mem_var && stats && delta && workspace,
               "stil_bn_memory_fwd_tiles: null pointer");
  STIL_REQUIRE(bn_prior_rho_ok(rho), "stil_bn_memory_fwd_tiles: rho=%g must lie in [0, 1]", (double)rho);
  STIL_REQUIRE(z || !resid, "stil_bn_memory_fwd_tiles: statistics-only call (z == NULL) cannot take a residual");
  STIL_REQUIRE(!resid_stats || resid, "stil_bn_memory_fwd_tiles: resid_stats without resid");
  STIL_REQUIRE(tile_rows > 0 && M > 0 && C > 0 && C % 4 == 0, "stil_bn_memory_fwd_tiles: bad shape M=%d C=%d tile_rows=%d", M, C, tile_rows);
  STIL_REQUIRE(workspace_bytes >= stil_bn_tiles_workspace_bytes(M, C, tile_rows) && ((uintptr_t)workspace % 8) == 0,
               "stil_bn_memory_fwd_tiles: workspace too small or not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (rho == 1.f) {
    rc = stil_bn_train_fwd_tiles(x, tilestats, tile_rows, gamma, beta, nullptr, nullptr, nullptr, resid, resid_stats, z, stats, M, C, relu,
                                 eps, 0.f, workspace, workspace_bytes, stream);
    if (rc == STIL_OK) rc = bn_prior_clear_delta(delta, C, s);
    if (rc != STIL_OK) return rc;
    return bn_memory_tiles_final<false>(tilestats, tile_rows, gamma, beta, mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased,
                                        rho, stats, delta, M, C, eps, workspace, true, s);
  }
  rc = bn_memory_tiles_final<true>(tilestats, tile_rows, gamma, beta, mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, rho,
                                   stats, delta, M, C, eps, workspace, false, s);
  if (rc != STIL_OK) return rc;
  if (!z) return STIL_OK;   // statistics only: the consumer applies them while it stages its operand
  long total4 = (long)M * C / 4;
  int grid = (int)((total4 + 255) / 256 < 8192 ? (total4 + 255) / 256 : 8192);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(grid), dim3(256), 0, s, x, stats, resid, resid_stats, z, total4, C, relu);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
