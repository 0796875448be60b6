// Test-time BatchNorm on a running estimate of the TARGET statistics that the adaptation owns (RoTTA's robust BatchNorm, Yuan
// et al., CVPR 2023; DUA, Mirza et al., CVPR 2022).  C ABI in stil_bnmemory.h (beside this file).  The forward of bn_prior.hip
// with the [C] pair (mem_mean, mem_var) in place of the running buffers, plus, per channel,
//   m' = (1 - alpha) m + alpha mean_batch,   s' = (1 - alpha) s + alpha c var_batch,   c = M / (M - 1) if unbiased and M > 1 else 1
// written to a SECOND pair (mem_mean_out, mem_var_out) by the one thread that finishes the channel's reduction: the finish is
// bn_prior.hip's BnBlendFwd with its two outputs set, the kernels and launch sequences are bn.hip's.  The normalisation reads m, s
// alone, so a layer's forwards within one step all see the same estimate whichever of them writes m', s'.
// NULL outputs: the call is stil_bn_prior_fwd(_tiles) after the memory's own checks.  rho == 1: see bn_blend_fwd.
// This file holds what only the memory refuses, and the two entry points.

static inline bool bn_memory_overlap(const float* a, const float* b, int C) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, n = (uintptr_t)C * sizeof(float);
  return x < y + n && y < x + n;
}

// what both entries check of the memory's own arguments, outputs given or not
static inline int bn_memory_check(const char* who, const float* mem_mean, const float* mem_var, const float* mem_mean_out,
                                  const float* mem_var_out, float alpha, int unbiased, int C) {
  STIL_REQUIRE(alpha >= 0.f && alpha <= 1.f, "%s: alpha=%g must lie in [0, 1]", who, (double)alpha);   // false for NaN
  STIL_REQUIRE(unbiased == 0 || unbiased == 1, "%s: unbiased=%d must be 0 or 1", who, unbiased);
  STIL_REQUIRE((mem_mean_out == nullptr) == (mem_var_out == nullptr), "%s: one memory output without the other", who);
  if (mem_mean_out && mem_mean && mem_var && C > 0)
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
  const char* who = "stil_bn_memory_fwd";
  const int rc = bn_memory_check(who, mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, C);
  if (rc != STIL_OK) return rc;
  return bn_blend_fwd(who, x, gamma, beta, mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, rho, resid, z, stats, delta, M, C,
                      relu, eps, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int stil_bn_memory_fwd_tiles(const float* x, const float* tilestats, int tile_rows, const float* gamma, const float* beta,
                                        const float* mem_mean, const float* mem_var, float* mem_mean_out, float* mem_var_out, float alpha,
                                        int unbiased, float rho, const float* resid, const float* resid_stats, float* z, float* stats,
                                        float* delta, int M, int C, int relu, float eps, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  const char* who = "stil_bn_memory_fwd_tiles";
  const int rc = bn_memory_check(who, mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, C);
  if (rc != STIL_OK) return rc;
  return bn_blend_fwd_tiles(who, x, tilestats, tile_rows, gamma, beta, mem_mean, mem_var, mem_mean_out, mem_var_out, alpha, unbiased, rho,
                            resid, resid_stats, z, stats, delta, M, C, relu, eps, workspace, workspace_bytes, (hipStream_t)stream);
}
