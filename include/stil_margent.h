/* C ABI of libstil_hip.so: the marginal-entropy loss of MEMO (Zhang, Levine, Finn, NeurIPS 2022, "MEMO: Test Time Robustness via
 * Adaptation and Augmentation") for test-time adaptation on augmented views of single test points, on top of TENT
 * (include/stil_tta.h).  Kept apart from include/stil_hip.h, include/stil_tta.h, include/stil_eata.h, include/stil_bnprior.h and
 * include/stil_infomax.h, whose entry points form their own ledgers; stil_tta_amd/_lib.py binds all six headers
 * (tests/test_margent_abi_ledger_cpu.py is this header's ledger).
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream). */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Entropy of the mean prediction over the views of each sample, forward and backward, of Z [groups * views, K] (row stride
 * ld >= K; any K >= 1, groups >= 1, views >= 1).  Row r belongs to group g = r / views: the views of one sample are consecutive
 * rows.  With V = views:
 *   lse[r], p[r,k] (stride ldp >= K; NULL: not written)           as stil_entropy_rows, bit for bit
 *   logpbar[g,k] = logsumexp_v( Z[gV+v,k] - lse[gV+v] ) - log V   (double; never the logarithm of an underflowed mean)
 *   pbar[g,k]    = exp(logpbar[g,k])                              (float [groups, ldb >= K])
 *   Hbar[g]      = - sum_k pbar[g,k] logpbar[g,k]                 (float [groups])
 *   dZ[r,j]      = grad_scale / V * p[r,j] * ( sum_k p[r,k] logpbar[g,k] - logpbar[g,j] )   (stride ldd >= K; NULL: not written)
 *                = d( grad_scale sum_g Hbar[g] ) / dZ
 *   out[0]       = sum_g Hbar[g] / groups                         (float [1])
 * With views == 1, Hbar is the row entropy and dZ is -grad_scale p (log p + H), TENT's.  Every p entering pbar and dZ is
 * recomputed from Z and the double lse, every quantity is formed in double and rounded once, and every sum over views, columns
 * or groups runs in a fixed order without float atomics: bit-identical on repetition.  Columns K.. of p, pbar and dZ, rows past
 * groups * views and groups past `groups` are not touched.
 * ws: at least groups * (K + (K + 255) / 256) doubles of scratch, written before it is read (the caller need not clear it).
 * The call allocates nothing, reads nothing back to the host and makes at most four launches.  A NULL required pointer (Z, lse,
 * pbar, Hbar, out, ws), groups < 1, views < 1, K < 1, a leading dimension below K or a groups * views that overflows int is
 * refused before any launch. */
int stil_marginal_entropy_groups(const float* Z, int ld, int groups, int views, int K, float grad_scale, double* lse, float* p,
                                 int ldp, float* pbar, int ldb, float* Hbar, float* dZ, int ldd, float* out, double* ws,
                                 void* stream);

#ifdef __cplusplus
}
#endif
