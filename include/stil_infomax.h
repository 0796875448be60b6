/* C ABI of libstil_hip.so: SHOT's information-maximisation loss (Liang et al., ICML 2020, "Do We Really Need to Access the
 * Source Data?  Source Hypothesis Transfer for Unsupervised Domain Adaptation"; the SHOT-IM baseline of the TENT paper) for
 * test-time adaptation, on top of TENT (include/stil_tta.h).  Kept apart from include/stil_hip.h, include/stil_tta.h,
 * include/stil_eata.h and include/stil_bnprior.h, whose entry points form their own ledgers; stil_tta_amd/_lib.py binds all
 * five headers (tests/test_shot_abi_ledger_cpu.py is this header's ledger).
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream). */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Row entropy minus the entropy of the batch-mean prediction, forward and backward, of Z [rows, K] (row stride ld >= K; any
 * K >= 1), with lambda = div_weight >= 0 and eps > 0:
 *   lse[r], p[r,k] (stride ldp >= K; NULL: not written), H[r]    as stil_entropy_rows, bit for bit, for every lambda
 *   pbar[k] = (1/rows) sum_r p[r,k]                               (float [K])
 *   D       = sum_k pbar[k] log(pbar[k] + eps)                    (minus the marginal entropy, in SHOT's eps form)
 *   c[k]    = log(pbar[k] + eps) + pbar[k] / (pbar[k] + eps)      (= dD / dpbar[k])
 *   dZ[r,k] = grad_scale p[r,k] ( -(log p[r,k] + H[r]) + lambda (c[k] - sum_j p[r,j] c[j]) )   (stride ldd >= K; NULL: not written)
 *           = d( grad_scale (sum_r H[r] + lambda rows D) ) / dZ
 *   out[0]  = sum_r H[r] / rows + lambda D,   out[1] = sum_r H[r] / rows,   out[2] = D       (float [3])
 * With lambda == 0, dZ and out[0] are those of stil_entropy_rows (its dZ and mean) bit for bit; out[1] is its mean for every
 * lambda.  The column means couple the rows: every p entering pbar and dZ is recomputed from Z and the double lse, every
 * quantity is formed in double and rounded once, and every sum over rows or columns runs in a fixed order without float
 * atomics: bit-identical on repetition.  Columns K.. of p and dZ and rows past `rows` are not touched.
 * ws: at least 2 K + rows doubles of scratch, written before it is read (the caller need not clear it).  The call allocates
 * nothing, reads nothing back to the host and makes at most four launches.  A NULL required pointer (Z, lse, H, pbar, out,
 * ws), rows < 1, K < 1, a leading dimension below K, an eps that is not finite and positive or a div_weight that is not
 * finite and non-negative is refused before any launch. */
int stil_infomax_rows(const float* Z, int ld, int rows, int K, float grad_scale, float div_weight, float eps, double* lse,
                      float* p, int ldp, float* H, float* pbar, float* dZ, int ldd, float* out, double* ws, void* stream);

#ifdef __cplusplus
}
#endif
