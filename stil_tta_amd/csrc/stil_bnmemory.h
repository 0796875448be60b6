/* C ABI of libstil_hip.so: test-time BatchNorm on a running estimate of the target statistics (RoTTA's robust BatchNorm, Yuan et
 * al., CVPR 2023, "Robust test-time adaptation in dynamic scenarios"; DUA, Mirza et al., CVPR 2022, "The norm must go on").
 * Kept beside its entry points (bn_memory.hip) and out of include/, whose headers form closed ledgers; stil_tta_amd/_lib.py binds it
 * through MEMORY_HEADERS (tests/test_bnmemory_abi_ledger_cpu.py is this header's ledger).
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream).
 *
 * The two entries are stil_bn_prior_fwd / stil_bn_prior_fwd_tiles of include/stil_bnprior.h with the memory m = mem_mean,
 * s = mem_var (read-only, [C]) in place of running_mean / running_var, and one more result.  Per channel, with M rows, batch mean
 * mu_b and BIASED batch variance v_b (formed exactly as there):
 *   mu = (1 - rho) m + rho mu_b,   v = (1 - rho) s + rho v_b,   r, stats [4, C], z, delta: as include/stil_bnprior.h
 *   m' = (1 - alpha) m + alpha mu_b  -> mem_mean_out
 *   s' = (1 - alpha) s + alpha c v_b -> mem_var_out,   c = M / (M - 1) if unbiased != 0 and M > 1, else 1
 * m', s' are formed in double and rounded once, by the thread that finishes the channel's reduction; the normalisation never sees
 * them.  The outputs must not overlap the memory read, nor each other.  mem_mean_out == mem_var_out == NULL: no update, the call is
 * stil_bn_prior_fwd(_tiles) on the same arguments, bit for bit.  rho = 1: z and stats are stil_bn_train_fwd(_tiles)'s bits (NULL
 * running buffers) and delta is cleared; the memory is updated all the same.  rho = 0: eval-mode BatchNorm on the memory.
 * The memory is a constant of the step: stil_bn_prior_bwd(_tiles) with the same rho and delta is the exact backward.
 *
 * Refused before any launch, nothing written: alpha outside [0, 1] or NaN, unbiased other than 0 / 1, exactly one of the two outputs
 * NULL, overlapping memory pointers, and whatever stil_bn_prior_fwd(_tiles) refuses (a NULL required pointer, rho outside [0, 1] or
 * NaN, a bad shape, too small a workspace). */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int stil_bn_memory_fwd(const float* x, const float* gamma, const float* beta, const float* mem_mean, const float* mem_var,
                       float* mem_mean_out, float* mem_var_out, float alpha, int unbiased, float rho, const float* resid,
                       float* z, float* stats, float* delta, int M, int C, int relu, float eps, float* workspace,
                       size_t workspace_bytes, void* stream);
/* statistics from the per-tile partials of the producing GEMM, as stil_bn_prior_fwd_tiles */
int stil_bn_memory_fwd_tiles(const float* x, const float* tilestats, int tile_rows, const float* gamma, const float* beta,
                             const float* mem_mean, const float* mem_var, float* mem_mean_out, float* mem_var_out, float alpha,
                             int unbiased, float rho, const float* resid, const float* resid_stats, float* z, float* stats,
                             float* delta, int M, int C, int relu, float eps, void* workspace, size_t workspace_bytes,
                             void* stream);

#ifdef __cplusplus
}
#endif
