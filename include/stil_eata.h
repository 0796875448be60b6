/* C ABI of libstil_hip.so: EATA test-time adaptation (Niu et al., ICML 2022, "Efficient Test-Time Model Adaptation without
 * Forgetting"), on top of TENT (include/stil_tta.h).  Kept apart from include/stil_hip.h and include/stil_tta.h, whose
 * entry points form their own ledgers (tests/test_abi_ledger_cpu.py, tests/test_tta_abi_ledger_cpu.py);
 * stil_tta_amd/_lib.py binds all three headers.
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream). */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* EATA's sample selection and weighted entropy loss (sections 3.1, eq. 3-6 of the paper), per row r of Z [rows, K] (row stride
 * ld >= K; any K >= 1), with m [K] the running mean of the selected predictions and m_valid[0] its validity flag:
 *   lse[r], p[r,k] (stride ldp >= K), H[r]          as stil_entropy_rows, bit for bit; Hd[r] = H_r before its rounding to float
 *   c[r]   = <m, p_r> / (max(|m|, 1e-8) max(|p_r|, 1e-8))   with m as it stood before the call (0 while m is invalid)
 *   rel[r] = H_r < e_margin;  sel[r] = rel[r] and (m invalid or |c_r| < d_margin)        (0/1 bytes)
 *   w[r]   = exp(e_margin - H_r)
 *   counts = {n = sum sel, n_reliable = sum rel, validity of m before the call, unused}    (int[4])
 *   loss[0] = (1/n) sum_r sel w H                    (0 when n == 0)
 *   m      <- pbar = (1/n) sum_r sel p_r when m was invalid, else momentum m + (1 - momentum) pbar; m_valid[0] <- 1;
 *             both untouched when n == 0
 *   active_out[t] = active[t] and n > 0, t < n_tensors   (the gate of the Adam step; n_tensors == 0: masks may be NULL)
 *   dZ[r,k] = sel[r] w[r] (-p[r,k] (log p[r,k] + H[r])) grad_scale / n   (stride ldd >= K; all zero when n == 0)
 *           = d(grad_scale loss)/dZ with w held constant
 * Decisions are taken on the double-precision H and c; every output is formed in double and rounded once; the sums are
 * fixed-order: bit-identical on repetition.  Columns K.. of p and dZ are not touched.  Nothing is read back to the host. */
int stil_eata_rows(const float* Z, int ld, int rows, int K, float e_margin, float d_margin, float momentum,
                   float grad_scale, float* m, int* m_valid, double* lse, double* Hd, float* p, int ldp, float* H,
                   float* c, float* w, unsigned char* rel, unsigned char* sel, float* dZ, int ldd, int* counts, float* loss,
                   const unsigned char* active, unsigned char* active_out, int n_tensors, void* stream);

/* EATA's anti-forgetting regulariser (section 3.2, eq. 8) over the flat slab of stil_adam_step (n floats, a multiple of 1024;
 * chunk2tensor [n/1024], active [n_tensors]).  achunks [n_achunks] lists the slab chunks of the adapted set A; theta0 and
 * fisher are compact, chunk j of them belonging to slab chunk achunks[j].  For every listed chunk whose tensor is active
 * (entries out of range, padding chunks (-1) and inactive tensors are skipped):
 *   grads[i] += 2 alpha fisher (params[i] - theta0)
 *   R[0] = alpha sum fisher (params - theta0)^2     (partial: n_achunks doubles of scratch; fixed-order sum)
 * Only A's chunks of `grads` are read or written. */
int stil_eata_anchor(const float* params, const float* theta0, const float* fisher, float* grads, const int* achunks,
                     int n_achunks, const int* chunk2tensor, const unsigned char* active, int n_tensors, long n,
                     float alpha, double* partial, float* R, void* stream);

/* Fisher accumulation (section 3.2, eq. 7): fisher[j*1024 + i] += grads[achunks[j]*1024 + i]^2 * scale over the same chunks. */
int stil_eata_fisher_accum(float* fisher, const float* grads, const int* achunks, int n_achunks, const int* chunk2tensor,
                           const unsigned char* active, int n_tensors, long n, float scale, void* stream);

#ifdef __cplusplus
}
#endif
