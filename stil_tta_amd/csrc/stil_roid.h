/* C ABI of libstil_hip.so: ROID (Marsden, Doebler, Yang, WACV 2024, "Universal Test-time Adaptation through Weight Ensembling,
 * Diversity Weighting, and Prior Correction"; definition as recalled: unpinned) as a test-time adaptation loss on top of TENT
 * (include/stil_tta.h): the soft likelihood ratio of the rows a certainty-and-diversity selection keeps, the running mean
 * prediction, the prior correction of the scores, and the weight ensembling of the adapted set with its source values.
 * Kept beside its kernels (roid.hip) and out of include/, whose headers form closed ledgers; stil_tta_amd/_lib.py binds it
 * through ROID_HEADERS (tests/test_roid_abi_ledger_cpu.py is this header's ledger).
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream). */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The row loss of the logits Z [rows, K] (row stride ld >= K; any rows >= 1, any K >= 1) against the running mean prediction
 * ema [K] (float; it starts at 1 / K and is read as it stands BEFORE the call), with tau > 0, clip in (0, 1), eps > 0, momentum in
 * [0, 1]:
 *   lse[r], p[r,k], H[r]      as stil_entropy_rows, bit for bit (double [rows]; float, stride ldp >= K; float [rows]); Hd[r] is the
 *                             entropy before its rounding
 *   cos[r]   = <p_r, ema> / (|p_r| |ema|);   d_r = 1 - cos[r];   c_r = -Hd[r]
 *   slr[r]   = -sum_k q_k log(q_k / (1 - q_k) + eps),   q = min(p, clip)                     (the soft likelihood ratio)
 *   dn[r]    = (d_r - min d) / (max d - min d),   cn[r] likewise from c                       (minimum and maximum over the rows)
 *              THE DEGENERATE RULE, this project's: when a range is <= 1e-9 that normalised quantity is 0 for every row (rows == 1,
 *              identical rows; the published code divides 0 by 0 there).  Both ranges degenerate: every row is kept with weight 1
 *   keep[r]  = !(dn[r] < mean_r dn);   w[r] = keep ? exp(dn[r] cn[r] / tau) : 0               (bytes [rows]; float [rows]; constants of dZ)
 *   loss     = (1 / rows) sum_r w[r] slr[r]            (float [1]; the divisor is the batch size, not the number kept, as published)
 *   counts   = {rows kept, rows, d range degenerate, c range degenerate}                      (int [4])
 *   g_k      = [p_k <= clip] (-log(u_k + eps) - u_k / ((u_k + eps)(1 - q_k))),   u = q / (1 - q)
 *   dZ[r,k]  = grad_scale (w[r] / rows) p_k (g_k - sum_j p_j g_j)      (stride ldd >= K; rows with keep = 0 are zeroed): with
 *              grad_scale = 1, d loss / d Z
 *   pbar[k]  = (1 / rows) sum_r p[r,k]  over ALL rows                                          (float [K])
 *   ema[k]  <- momentum ema[k] + (1 - momentum) pbar[k]          (in the finishing launch: after every cosine has been read)
 *   smooth   = max(1 / rows, 1 / K) / max_k pbar_k;   prior[k] = s_k = (pbar_k + smooth) / (1 + smooth K)       (float [K])
 *   scores[r,k] = p[r,k] s_k / sum_j p[r,j] s_j                  (correct != 0 only; stride lds >= K)
 * The published code multiplies the LOGITS by s; here the probabilities are corrected and renormalised, so every row of scores
 * is a distribution.
 * Every decision and sum is formed in double from the float inputs (p, pbar, d, c and the weights stay double between the
 * launches) and every output is rounded once; every sum runs in a fixed order without atomics: bit-identical on repetition.
 * Columns K.. of p, dZ and scores, and rows past `rows`, are not touched.  With correct == 0 scores is neither read nor written
 * and may be NULL, and prior may be NULL (not written).
 * ws: at least 4 rows + 2 K doubles of scratch (written before it is read).  The call allocates nothing, reads nothing back to the
 * host and makes four launches: one 256-thread workgroup per row; one thread per column for pbar; one workgroup for minimum,
 * maximum, mean, weights, loss, counts, ema and s; one workgroup per row for dZ and scores.
 * A NULL required pointer (Z, ema, lse, p, H, cos, slr, dn, cn, w, keep, pbar, dZ, counts, loss, ws; prior and scores when
 * correct != 0), rows < 1, K < 1, a leading dimension below K, a tau or eps that is not finite and positive, a clip outside (0, 1),
 * a momentum outside [0, 1], a grad_scale that is not finite, a NaN, or a correct other than 0 or 1, is refused before any launch:
 * nothing is written. */
int stil_roid_rows(const float* Z, int ld, int rows, int K, float* ema, float tau, float clip, float eps, float momentum,
                   float grad_scale, int correct, double* lse, float* p, int ldp, float* H, float* cos, float* slr, float* dn,
                   float* cn, float* w, unsigned char* keep, float* pbar, float* prior, float* scores, int lds, float* dZ, int ldd,
                   int* counts, float* loss, double* ws, void* stream);

/* Weight ensembling over the adapted set A, in the layout of stil_sar_restore (include/stil_sar.h): `achunks` lists the 1024-float
 * slab chunks of A, chunk j of the compact theta0 belongs to slab chunk achunks[j]:
 *   params[i] <- momentum params[i] + (1 - momentum) theta0[i]     formed in double, rounded once; momentum in [0, 1]
 * Only chunks that are in range, whose tensor is in range and active, are written; a skipped entry never forms an address.
 * momentum == 1 launches nothing (params is bit-identical); momentum == 0 copies theta0.  One launch, one block per listed chunk.
 * A NULL pointer, an n that is no multiple of 1024 or negative, a negative n_achunks or n_tensors, a slab that is not 16-byte
 * aligned, or a momentum outside [0, 1] or NaN, is refused before any launch: nothing is written. */
int stil_roid_ensemble(float* params, const float* theta0, const int* achunks, int n_achunks, const int* chunk2tensor,
                       const unsigned char* active, int n_tensors, long n, float momentum, void* stream);

#ifdef __cplusplus
}
#endif
