/* C ABI of libstil_hip.so: READ's confidence-aware loss with its batch-balance term (Yang et al., ICLR 2024, "Test-time
 * Adaptation against Multi-modal Reliability Bias"; constants and form as recalled: unpinned) for test-time adaptation of the
 * fusion attention, on top of TENT (include/stil_tta.h) and SHOT-IM (include/stil_infomax.h).  Kept beside its kernels (read.hip)
 * and out of include/, whose headers form closed ledgers; stil_tta_amd/_lib.py binds it through READ_HEADERS
 * (tests/test_read_abi_ledger_cpu.py is this header's ledger).
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream). */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Confidence-aware loss plus batch balance, forward and backward, of Z [rows, K] (row stride ld >= K; any K >= 1), with gamma in
 * (0, 1], lambda = div_weight >= 0 and eps > 0:
 *   lse[r], p[r,k] (stride ldp >= K; NULL: not written)           as stil_entropy_rows, bit for bit
 *   yhat[r] = the first maximum of Z[r,:]                           (int [rows]; the convention of stil_deyo_rows)
 *   conf[r] = c_r = p[r, yhat[r]]                                   (float [rows], the very bits of that entry of p)
 *   f[r]    = c_r log(e gamma / c_r) = c_r (1 + ln gamma - ln c_r)  (float [rows]; df/dc = ln(gamma / c): minimising it raises the
 *                                                                    confidence of rows above gamma and lowers that of rows below)
 *   pbar[k] = (1/rows) sum_r p[r,k],   D = sum_k pbar[k] log(pbar[k] + eps),   ck[k] = log(pbar[k] + eps) + pbar[k] / (pbar[k] + eps)
 *                                                                   as stil_infomax_rows: pbar and D are its bits for the same Z, eps
 *   dZ[r,k] = grad_scale ( ln(gamma / c_r) c_r ([k == yhat[r]] - p[r,k]) + lambda p[r,k] (ck[k] - sum_j p[r,j] ck[j]) )
 *           = d( grad_scale (sum_r f[r] + lambda rows D) ) / dZ, yhat held fixed      (stride ldd >= K; NULL: not written)
 *   out[0]  = sum_r f[r] / rows + lambda D,   out[1] = sum_r f[r] / rows,   out[2] = D       (float [3])
 * With gamma = 1/e, f = -c ln c.  Every quantity is formed in double from Z and the double lse and rounded once; every sum over
 * rows or columns runs in a fixed order without float atomics: bit-identical on repetition.  Columns K.. of p and dZ and rows past
 * `rows` are not touched.
 * ws: at least 2 K doubles of scratch, written before it is read (the caller need not clear it).  The call allocates nothing, reads
 * nothing back to the host and makes at most four launches.  A NULL required pointer (Z, lse, yhat, conf, f, pbar, out, ws),
 * rows < 1, K < 1, a leading dimension below K, a gamma outside (0, 1] or NaN, an eps that is not finite and positive or a
 * div_weight that is not finite and non-negative is refused before any launch. */
int stil_read_rows(const float* Z, int ld, int rows, int K, float grad_scale, float gamma, float div_weight, float eps,
                   double* lse, float* p, int ldp, int* yhat, float* conf, float* f, float* pbar,
                   float* dZ, int ldd, float* out, double* ws, void* stream);

#ifdef __cplusplus
}
#endif
