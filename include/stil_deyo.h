/* C ABI of libstil_hip.so: DeYO test-time adaptation (Lee et al., ICLR 2024, "Entropy is not enough for test-time adaptation:
 * from the perspective of disentangled factors"), on top of TENT (include/stil_tta.h) and beside EATA (include/stil_eata.h).
 * Kept apart from the other six headers, whose entry points form their own ledgers; this one's is
 * tests/test_deyo_abi_ledger_cpu.py.  stil_tta_amd/_lib.py binds all seven headers.
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream). */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The patch-shuffled second view: src, dst float [B, C, H, W], contiguous, not overlapping; H % grid == 0, W % grid == 0,
 * ph = H / grid, pw = W / grid; perm int32 [B, grid^2].  Destination patch slot s = (y / ph) grid + (x / pw) of image b receives
 * source patch perm[b, s]: dst[b, c, y, x] = src[b, c, (q / grid) ph + y % ph, (q % grid) pw + x % pw], q = perm[b, s], the same q
 * for every channel.  A perm entry outside [0, grid^2) maps the slot to itself (q = s): no address is ever formed from an
 * out-of-range entry.  A pure copy (bit-exact), one launch; 16-byte loads and stores per lane when pw % 4 == 0 and both
 * pointers are 16-byte aligned, 4-byte ones otherwise.  C H W must be below 2^31. */
int stil_patch_shuffle(const float* src, float* dst, int B, int C, int H, int W, int grid, const int* perm, void* stream);

/* DeYO's two-stage sample selection and weighted entropy loss (sections 3.2-3.3 of the paper), per row r of Z [rows, K]
 * (row stride ld >= K; any K >= 1), the logits of the batch, and Zs [rows, K] (row stride lds >= K), the logits of the
 * same rows with their images patch-shuffled:
 *   lse[r], p[r,k] (stride ldp >= K), H[r]       as stil_entropy_rows, bit for bit; Hd[r] = H_r before its rounding to float
 *   yhat[r] = the first maximum of Z[r]
 *   plpd[r] = p[r, yhat] - softmax(Zs[r])[yhat]   (the pseudo-label probability difference; formed in double)
 *   rel[r]  = H_r < ent_margin;  sel[r] = rel[r] and plpd_r > plpd_margin                  (0/1 bytes)
 *   w[r]    = a_ent exp(e0 - H_r) + a_plpd exp(plpd_r);  Wd[r] = w_r before its rounding to float
 *   counts  = {n = sum sel, n_reliable = sum rel, 0, 0}                                    (int[4])
 *   loss[0] = (1/n) sum_r sel w H                 (0 when n == 0)
 *   active_out[t] = active[t] and n > 0, t < n_tensors   (the gate of the Adam step; n_tensors == 0: masks may be NULL)
 *   dZ[r,k] = sel[r] w[r] (-p[r,k] (log p[r,k] + H[r])) grad_scale / n   (stride ldd >= K; all zero when n == 0)
 *           = d(grad_scale loss)/dZ with w held constant
 * Decisions are taken on the double-precision H and plpd; every output is formed in double and rounded once; the sums are
 * fixed-order: bit-identical on repetition.  Columns K.. of p and dZ are not touched.  Nothing is read back to the host.
 * With a_plpd = 0, plpd_margin < -1, ent_margin = e0 and a_ent = 1 the loss, dZ, sel and counts[0] are those of stil_eata_rows
 * with an invalid m, bit for bit. */
int stil_deyo_rows(const float* Z, int ld, const float* Zs, int lds, int rows, int K, float ent_margin, float plpd_margin,
                   float e0, float a_ent, float a_plpd, float grad_scale, double* lse, double* Hd, double* Wd, float* p, int ldp,
                   float* H, float* plpd, float* w, int* yhat, unsigned char* rel, unsigned char* sel, float* dZ, int ldd,
                   int* counts, float* loss, const unsigned char* active, unsigned char* active_out, int n_tensors,
                   void* stream);

#ifdef __cplusplus
}
#endif
