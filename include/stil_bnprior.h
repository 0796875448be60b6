/* C ABI of libstil_hip.so: test-time BatchNorm with a source-statistics prior (Schneider et al., NeurIPS 2020, "Improving
 * robustness against common corruptions by covariate shift adaptation").  Kept apart from include/stil_hip.h, include/stil_tta.h
 * and include/stil_eata.h, whose entry points form their own ledgers; stil_tta_amd/_lib.py binds all four headers
 * (tests/test_bnprior_abi_ledger_cpu.py is this header's ledger).
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream).
 *
 * Per channel, with M rows, batch mean mu_b and BIASED batch variance v_b, the source statistics mu_s = running_mean and
 * v_s = running_var (read-only, used as stored) and rho = B / (N + B) in [0, 1]:
 *   mu = (1 - rho) mu_s + rho mu_b,   v = (1 - rho) v_s + rho v_b,   r = 1 / sqrt(v + eps),   xhat = (x - mu) r
 *   z = relu?( gamma xhat + beta + resid? ),   delta = (mu - mu_b) r
 * and, with g the gradient at z after the ReLU mask, k2 = mean g, k3 = mean g xhat:
 *   dgamma = sum g xhat,   dbeta = sum g,   dx = gamma r [ g - rho (k2 + delta k3) - rho k3 xhat ]
 * rho = 1 is training-mode BatchNorm on the batch statistics (delta = 0; the calls then run stil_bn_train_fwd(_tiles) with NULL
 * running buffers and stil_bn_train_bwd(_tiles) themselves: identical bits), rho = 0 eval-mode BatchNorm.  For rho < 1 the blend
 * and r are formed in double and rounded once; delta is formed from the rounded mu and r of the block, so that xhat + delta is
 * (x - mu_b) r to rounding.  No running buffer and no num_batches_tracked is written.
 *
 * The forward entries write the blended statistics block stats [4, C] = mu, r, a = gamma r, beta in the layout of
 * stil_bn_train_fwd, so its consumers (stil_gemm_nt a_bn / bstats, stil_wgrad_tn x_bn, resid_stats) work unchanged, and delta [C].
 * Arguments are those of the mirrored entry point of include/stil_hip.h: workspaces as stil_bn_workspace_bytes /
 * stil_bn_tiles_workspace_bytes / stil_bn_bwd_tiles_workspace_bytes size them, C a multiple of 64 for the two-pass entries and
 * of 4 for the tile entries, `resid`, `resid_stats`, z == NULL (statistics only), `gout`, `accumulate` and the three relu modes of
 * the backward (0 none, 1 mask from z, 2 mask recomputed from x and stats) as there.  A NULL required pointer, rho outside
 * [0, 1] or NaN, a bad shape or too small a workspace is refused before any launch. */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int stil_bn_prior_fwd(const float* x, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float rho, const float* resid, float* z, float* stats, float* delta,
                      int M, int C, int relu, float eps, float* workspace, size_t workspace_bytes, void* stream);
/* statistics from the per-tile partials of the producing GEMM (stil_gemm_nt colstats), as stil_bn_train_fwd_tiles */
int stil_bn_prior_fwd_tiles(const float* x, const float* tilestats, int tile_rows, const float* gamma, const float* beta,
                            const float* running_mean, const float* running_var, float rho, const float* resid,
                            const float* resid_stats, float* z, float* stats, float* delta, int M, int C, int relu,
                            float eps, void* workspace, size_t workspace_bytes, void* stream);
int stil_bn_prior_bwd(const float* dz, const float* z, const float* x, const float* gamma, const float* stats,
                      const float* delta, float rho, float* dx, float* gout, float* dgamma, float* dbeta, float* coef,
                      int M, int C, int relu, int accumulate, float* workspace, size_t workspace_bytes, void* stream);
/* sums from the per-tile partials of the GEMM that produced dz (stil_gemm_nt bstats), as stil_bn_train_bwd_tiles */
int stil_bn_prior_bwd_tiles(const float* dz, const float* z, const float* x, const float* gamma, const float* stats,
                            const float* delta, float rho, const float* tilestats, int ntiles, float* dx, float* dgamma,
                            float* dbeta, float* coef, int M, int C, int relu, int accumulate, void* workspace,
                            size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
