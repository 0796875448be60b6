// Test-time BatchNorm with a source-statistics prior (Schneider et al., NeurIPS 2020): the layer normalises by
//   mu = (1 - rho) running_mean + rho mean_batch,   v = (1 - rho) running_var + rho var_batch (biased),   rho = B / (N + B).
// C ABI in include/stil_bnprior.h.  No kernel is written here: the wide passes, the reduction skeletons and the launch sequences
// are bn.hip's.  This file holds the two FINISHES of the family and its entry points.  The forward finish (BnBlendFwd) forms the
// batch mean and variance exactly as the training finish does, blends them with the source statistics in double, and writes the
// same [4, C] statistics block plus delta = (mu - mean_batch) * rstd; it also serves the BatchNorm memory (bn_memory.hip), whose
// source pair is the memory and which adds one write.  The backward finish (BnPriorBwd) folds rho and delta into the coefficient
// triple of bn_bwd_dx_kernel:  dx = gamma rstd [ g - rho (k2 + delta k3) - rho k3 xhat ],  k2 = mean g, k3 = mean g xhat.
// rho == 1 is today's BatchNorm: those calls run bn.hip's sequences with the TRAINING finishes (NULL running buffers) and clear
// delta.  The source pair is read-only here, nothing is read back to the host, every sum keeps bn.hip's fixed order.

// gamma, beta, src_mean, src_var: the channel's values, loaded by the caller ahead of every store
__device__ __forceinline__ void bn_prior_write_stats(int c, int C, double mean_b, double var_b, float gamma, float beta, float src_mean,
                                                     float src_var, double rho, float eps, float* __restrict__ stats,
                                                     float* __restrict__ delta) {
  const double mu = (1.0 - rho) * (double)src_mean + rho * mean_b;
  const double v = (1.0 - rho) * (double)src_var + rho * var_b;
  const double r = 1.0 / sqrt(v + (double)eps);
  const float muf = (float)mu, rstd = (float)r;
  stats[c] = muf; stats[C + c] = rstd; stats[2 * C + c] = gamma * rstd; stats[3 * C + c] = beta;
  // from the ROUNDED mean and rstd, the ones every consumer forms xhat with: xhat_i + delta is then (x_i - mean_batch) * rstd to
  // rounding, and the two terms of the backward that cancel (rho k3 delta, rho k3 xhat_i) cancel on the device as well
  delta[c] = (float)(((double)muf - mean_b) * (double)rstd);
}

// The memory's update (stil_bnmemory.h), per channel:
//   m' = (1 - alpha) m + alpha mean_batch,   s' = (1 - alpha) s + alpha c var_batch,   c = M / (M - 1) if unbiased and M > 1 else 1
// formed in double from the batch mean and variance the blend uses and rounded once.
__device__ __forceinline__ void bn_memory_write(int c, double mean_b, double var_b, int M, float mem_mean, float mem_var,
                                                float* __restrict__ mem_mean_out, float* __restrict__ mem_var_out, double alpha,
                                                int unbiased) {
  const double corr = (unbiased && M > 1) ? (double)M / (double)(M - 1) : 1.0;
  mem_mean_out[c] = (float)((1.0 - alpha) * (double)mem_mean + alpha * mean_b);
  mem_var_out[c] = (float)((1.0 - alpha) * (double)mem_var + alpha * corr * var_b);
}

// Forward finish of the prior and of the memory.  src_*: the source pair (running buffers, or the memory read).  mean_out / var_out:
// the memory written, both NULL for the prior and for a memory call that updates nothing.  kStats = false: the memory write alone
// (rho == 1, where the training finish has written stats already).  In the tile path mean and variance stay in double until the blend.
template <bool kStats>
struct BnBlendFwd {
  const float *gamma, *beta, *src_mean, *src_var;
  float *mean_out, *var_out;
  float alpha;
  int unbiased;
  float rho, eps;
  float *stats, *delta;
  __device__ __forceinline__ void write(int c, int C, int M, double mean_b, double var_b) const {
    // every load ahead of the first store (see BnTrainFwd::write)
    const float sm = src_mean[c], sv = src_var[c], g = kStats ? gamma[c] : 0.f, b = kStats ? beta[c] : 0.f;
    if (kStats) bn_prior_write_stats(c, C, mean_b, var_b, g, b, sm, sv, (double)rho, eps, stats, delta);
    if (mean_out) bn_memory_write(c, mean_b, var_b, M, sm, sv, mean_out, var_out, (double)alpha, unbiased);
  }
  __device__ __forceinline__ void chunk(int c, int C, int M, float K, float s1, float s2) const {
    float mean, var;
    bn_chunk_moments(K, s1, s2, M, mean, var);
    write(c, C, M, (double)mean, (double)var);
  }
  __device__ __forceinline__ void tiles(int c, int C, int M, double s1, double s2, double s3) const {
    double mean_d, var_d;
    bn_tile_moments(s1, s2, s3, M, mean_d, var_d);
    write(c, C, M, mean_d, fmax(var_d, 0.0));
  }
};

// Backward finish: dgamma / dbeta as bn.hip writes them; coef[0] = gamma*rstd, [1] = rho (k2 + delta k3), [2] = rho k3
struct BnPriorBwd {
  const float *gamma, *stats, *delta;
  float rho;
  float *dgamma, *dbeta, *coef;
  int accumulate;
  __device__ __forceinline__ void operator()(int c, int C, int M, float s1, float s2) const {
    // every load ahead of the first store (see BnTrainFwd::write)
    const float g = gamma[c], rstd = stats[C + c], dl = delta[c];
    const float b0 = (accumulate && dbeta) ? dbeta[c] : 0.f, g0 = (accumulate && dgamma) ? dgamma[c] : 0.f;
    if (dbeta) dbeta[c] = accumulate ? b0 + s1 : s1;
    if (dgamma) dgamma[c] = accumulate ? g0 + s2 : s2;
    const double k2 = (double)s1 / (double)M, k3 = (double)s2 / (double)M;
    coef[c] = g * rstd;
    coef[C + c] = (float)((double)rho * (k2 + (double)dl * k3));
    coef[2 * C + c] = (float)((double)rho * k3);
  }
};

// ---------------------------------------------------------------------------------------
static inline bool bn_prior_rho_ok(float rho) { return rho >= 0.f && rho <= 1.f; }   // false for NaN

static inline int bn_prior_clear_delta(float* delta, int C, hipStream_t s) {
  if (hipMemsetAsync(delta, 0, (size_t)C * sizeof(float), s) != hipSuccess) {
    stil_set_error("stil_bn_prior: clearing delta failed: %s", hipGetErrorString(hipGetLastError()));
    return STIL_EHIP;
  }
  return STIL_OK;
}

// The forwards of the prior and of the memory (`who`); the prior passes no memory outputs.  rho == 1: the batch statistics alone
// normalise, so z and stats come from the training finish (identical bits), delta is cleared, and with outputs the final runs once
// more over the sums that left in the workspace, for the memory alone.
static int bn_blend_fwd(const char* who, const float* x, const float* gamma, const float* beta, const float* src_mean,
                        const float* src_var, float* mean_out, float* var_out, float alpha, int unbiased, float rho, const float* resid,
                        float* z, float* stats, float* delta, int M, int C, int relu, float eps, float* workspace,
                        size_t workspace_bytes, hipStream_t s) {
  STIL_REQUIRE(x && gamma && beta && src_mean && src_var && z && stats && delta && workspace, "%s: null pointer", who);
  STIL_REQUIRE(bn_prior_rho_ok(rho), "%s: rho=%g must lie in [0, 1]", who, (double)rho);
  STIL_REQUIRE(M > 0, "%s: M=%d must be positive", who, M);
  if (rho != 1.f) {
    const BnBlendFwd<true> fin{gamma, beta, src_mean, src_var, mean_out, var_out, alpha, unbiased, rho, eps, stats, delta};
    return bn_fwd_two_pass(who, fin, x, resid, z, stats, M, C, relu, workspace, workspace_bytes, s);
  }
  const BnTrainFwd train{gamma, beta, nullptr, nullptr, nullptr, stats, eps, 0.f};
  int rc = bn_fwd_two_pass(who, train, x, resid, z, stats, M, C, relu, workspace, workspace_bytes, s);
  if (rc == STIL_OK) rc = bn_prior_clear_delta(delta, C, s);
  if (rc != STIL_OK || !mean_out) return rc;
  const BnBlendFwd<false> fin{gamma, beta, src_mean, src_var, mean_out, var_out, alpha, unbiased, rho, eps, stats, delta};
  return bn_fwd_two_pass(who, fin, x, resid, z, stats, M, C, relu, workspace, workspace_bytes, s, true);
}

static int bn_blend_fwd_tiles(const char* who, const float* x, const float* tilestats, int tile_rows, const float* gamma,
                              const float* beta, const float* src_mean, const float* src_var, float* mean_out, float* var_out,
                              float alpha, int unbiased, float rho, const float* resid, const float* resid_stats, float* z, float* stats,
                              float* delta, int M, int C, int relu, float eps, void* workspace, size_t workspace_bytes, hipStream_t s) {
  STIL_REQUIRE(x && tilestats && gamma && beta && src_mean && src_var && stats && delta && workspace, "%s: null pointer", who);
  STIL_REQUIRE(bn_prior_rho_ok(rho), "%s: rho=%g must lie in [0, 1]", who, (double)rho);
  if (rho != 1.f) {
    const BnBlendFwd<true> fin{gamma, beta, src_mean, src_var, mean_out, var_out, alpha, unbiased, rho, eps, stats, delta};
    return bn_fwd_tiles(who, fin, x, tilestats, tile_rows, resid, resid_stats, z, stats, M, C, relu, workspace, workspace_bytes, s);
  }
  const BnTrainFwd train{gamma, beta, nullptr, nullptr, nullptr, stats, eps, 0.f};
  int rc = bn_fwd_tiles(who, train, x, tilestats, tile_rows, resid, resid_stats, z, stats, M, C, relu, workspace, workspace_bytes, s);
  if (rc == STIL_OK) rc = bn_prior_clear_delta(delta, C, s);
  if (rc != STIL_OK || !mean_out) return rc;
  const BnBlendFwd<false> fin{gamma, beta, src_mean, src_var, mean_out, var_out, alpha, unbiased, rho, eps, stats, delta};
  return bn_fwd_tiles(who, fin, x, tilestats, tile_rows, resid, resid_stats, z, stats, M, C, relu, workspace, workspace_bytes, s, true);
}

extern "C" int stil_bn_prior_fwd(const float* x, const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, float rho, const float* resid, float* z, float* stats, float* delta,
                                 int M, int C, int relu, float eps, float* workspace, size_t workspace_bytes, void* stream) {
  return bn_blend_fwd("stil_bn_prior_fwd", x, gamma, beta, running_mean, running_var, nullptr, nullptr, 0.f, 0, rho, resid, z, stats, delta,
                      M, C, relu, eps, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int stil_bn_prior_fwd_tiles(const float* x, const float* tilestats, int tile_rows, const float* gamma, const float* beta,
                                       const float* running_mean, const float* running_var, float rho, const float* resid,
                                       const float* resid_stats, float* z, float* stats, float* delta, int M, int C, int relu,
                                       float eps, void* workspace, size_t workspace_bytes, void* stream) {
  return bn_blend_fwd_tiles("stil_bn_prior_fwd_tiles", x, tilestats, tile_rows, gamma, beta, running_mean, running_var, nullptr, nullptr,
                            0.f, 0, rho, resid, resid_stats, z, stats, delta, M, C, relu, eps, workspace, workspace_bytes,
                            (hipStream_t)stream);
}

extern "C" int stil_bn_prior_bwd(const float* dz, const float* z, const float* x, const float* gamma, const float* stats,
                                 const float* delta, float rho, float* dx, float* gout, float* dgamma, float* dbeta, float* coef,
                                 int M, int C, int relu, int accumulate, float* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "stil_bn_prior_bwd";
  STIL_REQUIRE(dz && x && gamma && stats && delta && dx && coef && workspace, "%s: null pointer", who);
  STIL_REQUIRE(bn_prior_rho_ok(rho), "%s: rho=%g must lie in [0, 1]", who, (double)rho);
  STIL_REQUIRE(M > 0, "%s: M=%d must be positive", who, M);
  hipStream_t s = (hipStream_t)stream;
  if (rho == 1.f)
    return bn_bwd_two_pass(who, BnTrainBwd{gamma, stats, dgamma, dbeta, coef, accumulate}, dz, z, x, stats, coef, dx, gout, M, C, relu,
                           workspace, workspace_bytes, s);
  return bn_bwd_two_pass(who, BnPriorBwd{gamma, stats, delta, rho, dgamma, dbeta, coef, accumulate}, dz, z, x, stats, coef, dx, gout, M, C,
                         relu, workspace, workspace_bytes, s);
}

extern "C" int stil_bn_prior_bwd_tiles(const float* dz, const float* z, const float* x, const float* gamma, const float* stats,
                                       const float* delta, float rho, const float* tilestats, int ntiles, float* dx, float* dgamma,
                                       float* dbeta, float* coef, int M, int C, int relu, int accumulate, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  const char* who = "stil_bn_prior_bwd_tiles";
  STIL_REQUIRE(dz && x && gamma && stats && delta && tilestats && dx && coef && workspace, "%s: null pointer", who);
  STIL_REQUIRE(bn_prior_rho_ok(rho), "%s: rho=%g must lie in [0, 1]", who, (double)rho);
  hipStream_t s = (hipStream_t)stream;
  if (rho == 1.f)
    return bn_bwd_tiles(who, BnTrainBwd{gamma, stats, dgamma, dbeta, coef, accumulate}, dz, z, x, stats, tilestats, ntiles, coef, dx, M, C,
                        relu, workspace, workspace_bytes, s);
  return bn_bwd_tiles(who, BnPriorBwd{gamma, stats, delta, rho, dgamma, dbeta, coef, accumulate}, dz, z, x, stats, tilestats, ntiles, coef,
                      dx, M, C, relu, workspace, workspace_bytes, s);
}
