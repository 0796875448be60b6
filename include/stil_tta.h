/* C ABI of libstil_hip.so: test-time adaptation.  Kept apart from include/stil_hip.h, whose entry points form the
 * training step's ledger (tests/test_abi_ledger_cpu.py); stil_tta_amd/_lib.py binds both headers.
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream). */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* TENT's loss (Wang et al., ICLR 2021, "Tent: Fully Test-Time Adaptation by Entropy Minimization", section 3), the hook
 * STiLModel.test_step leaves as a TODO (models/Disentangle/STiLModel.py:523-524): per row r of Z [rows, K] (row stride
 * ld >= K; any K >= 1),
 *   lse[r] = log sum_k exp(Z[r,k])                        (double)
 *   p[r,k] = softmax(Z[r])_k                              (row stride ldp >= K; NULL: not written)
 *   H[r]   = -sum_k p[r,k] log p[r,k]
 *   dZ[r,k] = -p[r,k] (log p[r,k] + H[r]) * grad_scale    (row stride ldd >= K; NULL: not written) = d(grad_scale sum_r H[r])/dZ
 *   mean[0] = sum_r H[r] / rows
 * lse, p, H and dZ are formed in double and rounded once; the mean is a fixed-order sum: bit-identical on repetition.
 * Columns K.. of p and dZ are not touched. */
int stil_entropy_rows(const float* Z, int ld, int rows, int K, float grad_scale, double* lse, float* p, int ldp,
                      float* H, float* dZ, int ldd, float* mean, void* stream);

#ifdef __cplusplus
}
#endif
