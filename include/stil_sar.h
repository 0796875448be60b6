/* C ABI of libstil_hip.so: SAR test-time adaptation (Niu et al., ICLR 2023, "Towards Stable Test-Time Adaptation in Dynamic
 * Wild World"), on top of TENT (include/stil_tta.h) and beside EATA (include/stil_eata.h) and DeYO (include/stil_deyo.h).
 * Kept apart from the other seven headers, whose entry points form their own ledgers; this one's is
 * tests/test_sar_abi_ledger_cpu.py.  stil_tta_amd/_lib.py binds all eight headers.
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream). */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The row loss of SAR's two passes (section 4 of the paper: the reliable-sample entropy S(x) of eq. 2, unweighted), per row r
 * of Z [rows, K] (row stride ld >= K; any K >= 1):
 *   lse[r], p[r,k] (stride ldp >= K), H[r]          as stil_entropy_rows, bit for bit; Hd[r] = H_r before its rounding to float
 *   sel[r] = (prior_sel == NULL or prior_sel[r]) and Hd_r < margin                        (0/1 bytes; prior_sel: bytes, NULL in
 *            the first pass, the first pass's sel in the second)
 *   counts = {n = sum sel, number of rows with Hd_r < margin, number of rows the prior admits (rows when NULL), 0}   (int[4])
 *   loss[0] = (1/n) sum_r sel Hd                    (0 when n == 0)
 *   active_out[t] = active[t] and n > 0, t < n_tensors   (the gate of the Adam step; n_tensors == 0: masks may be NULL)
 *   dZ[r,k] = sel[r] (-p[r,k] (log p[r,k] + H[r])) grad_scale / n   (stride ldd >= K; rows with sel = 0 are zero; all zero
 *           when n == 0) = d(grad_scale loss)/dZ
 * With ema != NULL (the second pass; ema_valid and recover are then required) the running mean of the loss and the
 * model-recovery decision follow, on the device:
 *   n > 0:  ema[0] <- loss when ema_valid[0] == 0, else momentum ema[0] + (1 - momentum) loss;  ema_valid[0] <- 1
 *   recover[0] <- reset > 0 and ema_valid[0] and ema[0] < reset     (on the values just written; reset <= 0: never raised)
 * Decisions are taken on the double-precision H; every output is formed in double and rounded once; the sums are
 * fixed-order: bit-identical on repetition.  Columns K.. of p and dZ are not touched.  Nothing is read back to the host. */
int stil_sar_rows(const float* Z, int ld, int rows, int K, float margin, float grad_scale, const unsigned char* prior_sel,
                  double* lse, double* Hd, float* p, int ldp, float* H, unsigned char* sel, float* dZ, int ldd, int* counts,
                  float* loss, const unsigned char* active, unsigned char* active_out, int n_tensors, float* ema,
                  int* ema_valid, float momentum, float reset, int* recover, void* stream);

/* SAR's ascent step (eq. 4-5) over the flat slab of stil_adam_step (n floats, a multiple of 1024; chunk2tensor [n/1024],
 * active [n_tensors]).  achunks [n_achunks] lists the slab chunks of the adapted set A; saved and e are compact, chunk j of
 * them belonging to slab chunk achunks[j].  Over every listed chunk whose tensor is active (entries out of range, padding
 * chunks (-1) and inactive tensors are skipped: no address is ever formed from them):
 *   norm[0] = sqrt(sum grads^2)           (double; partial: n_achunks doubles of scratch, skipped chunks 0; fixed-order sum)
 *   saved <- params;  e <- rho grads / (norm + 1e-12);  params <- params + e      (the float sum of the float e)
 * Only A's chunks of `params` are written; chunks of saved / e that belong to skipped entries are not touched. */
int stil_sar_perturb(float* params, const float* grads, float* saved, float* e, const int* achunks, int n_achunks,
                     const int* chunk2tensor, const unsigned char* active, int n_tensors, long n, float rho, double* partial,
                     double* norm, void* stream);

/* params <- saved over the same chunks: a pure copy (bit-exact). */
int stil_sar_restore(float* params, const float* saved, const int* achunks, int n_achunks, const int* chunk2tensor,
                     const unsigned char* active, int n_tensors, long n, void* stream);

/* SAR's model recovery, decided on the device: when recover[0] != 0, over the same chunks params <- theta0 (compact),
 * exp_avg <- 0 and exp_avg_sq <- 0 (slabs of n floats), steps[t] <- 0 for every active tensor t < n_tensors, and
 * ema_valid[0] <- 0; when recover[0] == 0 nothing is written. */
int stil_sar_recover(float* params, const float* theta0, float* exp_avg, float* exp_avg_sq, int* steps, const int* achunks,
                     int n_achunks, const int* chunk2tensor, const unsigned char* active, int n_tensors, long n,
                     const int* recover, int* ema_valid, void* stream);

#ifdef __cplusplus
}
#endif
