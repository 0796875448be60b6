/* C ABI of libstil_hip.so: STiL's own unlabelled-data branch as a test-time adaptation loss -- consensus-guided pseudo-labels
 * (CGPL) over the three classifier heads, smoothed by the prototype classifier (PGLS), and a soft cross-entropy per head
 * (models/Disentangle/STiLModel.py:255-303 with use_ema False; restated in oracle/stil_oracle.py's training_step), on top of TENT
 * (include/stil_tta.h).  Kept beside its kernels (cgpl.hip) and out of include/, whose headers form closed ledgers;
 * stil_tta_amd/_lib.py binds it through CGPL_HEADERS (tests/test_cgpl_abi_ledger_cpu.py is this header's ledger).
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream). */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Pseudo-labels, selection, the three soft cross-entropies and their gradients, of the logits Zm, Zi, Zt [rows, K] (multimodal,
 * imaging, tabular head; one row stride ld >= K; any K >= 1), the normalised multimodal projection feat [rows, Dp], the prototypes
 * protos [K, Dp], the temperature T > 0, rate in [0, 1], the threshold th and one byte per row, coin [rows]:
 *   lse3[h, r]  = log sum_k exp(Z_h[r,k]), h = 0 (m), 1 (i), 2 (t)         (double [3, rows]; lse3[0] as stil_entropy_rows, bit for bit)
 *   p[r,k]      = exp(Zm[r,k] - lse3[0, r])                                (stride ldp >= K; NULL: not written; stil_entropy_rows' bits)
 *   top_h[r]    = the FIRST maximum of Z_h[r,:]                            (the convention of stil_deyo_rows)
 *   case[r]     = 1: top_m == top_i == top_t;  2 (2_i): top_m == top_i != top_t;  3 (2_t): top_m == top_t != top_i;  4: otherwise
 *   a[r,k]      = the mean of the agreeing heads' logits: (m + i + t) / 3 | (m + i) / 2 | (m + t) / 2 | m
 *   q0[r,:]     = softmax(a[r,:]);   tp[r,:] = softmax_k(feat[r,:] . protos[k,:] / T)                 (tp only when rate < 1)
 *   q[r,k]      = rate q0 + (1 - rate) tp                                  (float [rows, K], stride ldp: the pseudo-label)
 *   conf[r]     = max_k (rate p[r,k] + (1 - rate) tp[r,k]);   mask1[r] = conf[r] >= th   (compared in double, before conf is rounded)
 *   w_m = mask1 & case 1;   w_i = mask1 & (case 1 | case 3 | case 4 & coin);   w_t = mask1 & (case 1 | case 2 | case 4 & !coin)
 *   ce3[h, r]   = -sum_k q[r,k] (Z_h[r,k] - lse3[h, r])                    (float [3, rows], every row, selected or not)
 *   dZ_h[r,k]   = grad_scale w_h[r] (exp(Z_h[r,k] - lse3[h, r]) - q[r,k])  (dZm, dZi, dZt, stride ldd >= K; each may be NULL: not
 *                                                                           written; q held constant.  Rows with w_h = 0 are zeroed)
 *   flags[r,:]  = {case[r], mask1[r], mask1[r], 0}                         (bytes [rows, 4], the layout of stil_cgpl_pgls)
 *   out         = {sum_h sum_r w_h ce_h / rows, and the same sum for h = m, i, t alone}                (float [4])
 *   counts      = {n = #mask1, #case 1, #case 2 (2_i), #case 3 (2_t), #case 4}                         (int [5])
 *   gate[t]     = active[t] && n > 0, t < n_tensors                        (the gate of the Adam step, as stil_eata_rows writes it)
 * With grad_scale = 1 / rows, dZ_h = d out[0] / d Z_h: the reference's .mean() runs over all rows, masked ones included.
 * Unlike stil_cgpl_pgls (include/stil_hip.h), which takes top_h as argmax(softmax) in fp32 and reproduces ATen's rounding ties,
 * top_h is the first maximum of the logits themselves; in exact arithmetic the two coincide.  Distribution alignment is not applied.
 * Every quantity is formed in double from the float inputs and rounded once; every sum runs in a fixed order without atomics:
 * bit-identical on repetition.  Columns K.. of p, q and dZ_h and rows past `rows` are not touched.
 * feat and protos may be NULL exactly when rate == 1; then neither they nor ws are read.  ws: at least rows K doubles of scratch when
 * rate < 1 (written before it is read), else it may be NULL.  The call allocates nothing, reads nothing back to the host and makes two
 * launches: one 256-thread workgroup per row, then one workgroup for out, counts and gate.
 * A NULL required pointer (Zm, Zi, Zt, coin, lse3, q, conf, flags, ce3, counts, out; active and gate when n_tensors > 0; feat, protos
 * and ws when rate < 1), rows < 1, K < 1, Dp < 1, a leading dimension below K, a rate outside [0, 1] or NaN, or with rate < 1 a T that
 * is not finite and positive, is refused before any launch: nothing is written. */
int stil_cgpl_rows(const float* Zm, const float* Zi, const float* Zt, int ld, const float* feat, const float* protos,
                   const unsigned char* coin, int rows, int K, int Dp, float T, float rate, float th, float grad_scale,
                   double* lse3, float* p, float* q, int ldp, float* conf, unsigned char* flags, float* ce3,
                   float* dZm, float* dZi, float* dZt, int ldd, int* counts, float* out,
                   const unsigned char* active, unsigned char* gate, int n_tensors, double* ws, void* stream);

#ifdef __cplusplus
}
#endif
