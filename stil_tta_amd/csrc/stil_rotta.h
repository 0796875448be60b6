/* C ABI of libstil_hip.so: RoTTA (Yuan, Xie, Li, CVPR 2023, "Robust Test-Time Adaptation in Dynamic Scenarios"; definition as
 * recalled: unpinned) on top of TENT (include/stil_tta.h): a category-balanced bank of test samples held on the device (which
 * samples stay is decided by pseudo-label, age and uncertainty), the timeliness-weighted cross-entropy of a student against a
 * teacher on that bank, and the teacher over the adapted set A (a swap with A, and its exponential moving average).
 * Kept beside its kernels (rotta.hip) and out of include/, whose headers form closed ledgers; stil_tta_amd/_lib.py binds it
 * through ROTTA_HEADERS (tests/test_rotta_abi_ledger_cpu.py is this header's ledger).
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream).  Nothing here is timed. */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The bounds of stil_rotta_bank_update: the bank's slots N and the classes K (occ[c] K stays far inside an int; the walk is one
 * workgroup, whose cost per sample grows with N / 256 and K / 256). */
#define STIL_ROTTA_MAX_SLOTS 4096
#define STIL_ROTTA_MAX_CLASSES 65536

/* The bank's bookkeeping moved over the B incoming samples, from the teacher's logits Zt [B, K] (row stride ld >= K).  The bank:
 *   label [N] int (-1: empty), unc [N] float, age [N] int, occ [K] int (filled slots per class), n [1] int (filled slots: always
 *   the prefix [0, n)); 1 <= N <= STIL_ROTTA_MAX_SLOTS, 1 <= K <= STIL_ROTTA_MAX_CLASSES; lambda_t, lambda_u finite and >= 0.
 * Two launches.  The first, one 256-thread workgroup per row:
 *   lse[b], p[b,k], H[b]   as stil_entropy_rows, bit for bit (double [B]; float, stride ldp >= K; float [B])
 *   yhat[b]                the first maximum of Zt[b]                                              (int [B])
 * The second is ONE workgroup that walks the samples in order, every decision depending on the ones before it.  For sample b, with
 * c = yhat[b], u = H[b] (the float), and in double
 *   s_new    = lambda_t / 2 + lambda_u u / ln K
 *   score(i) = lambda_t / (1 + exp(-age[i] / N)) + lambda_u unc[i] / ln K          (K == 1: both uncertainty terms are 0, not 0/0)
 *   if occ[c] K < N (integers):   if n < N: b is accepted into slot n, n += 1
 *                                 else the candidate is the slot of maximal score among the slots whose label is a class of
 *                                 maximal occupancy
 *   else                          the candidate is the slot of maximal score among the slots with label c
 *   a candidate is taken, and b accepted into it, iff score(candidate) > s_new (strictly); equal scores: the lowest slot index
 *   on accept: occ[old label] -= 1 when the slot was filled; label[slot] = c, unc[slot] = u, age[slot] = 0, occ[c] += 1,
 *              owner[slot] = b
 *   after every sample, accepted or not: age += 1 on all filled slots, the new one included (saturating at INT_MAX)
 * Outputs:
 *   owner [N] int          the incoming sample that owns the slot at the END of the call, -1 when the slot keeps its content (a
 *                          sample accepted and evicted within the same call owns nothing)
 *   accepted [B] bytes, slot_of [B] int (-1: not accepted)   as of the sample's own turn
 *   counts [4] int         {accepted, evictions (accepted into a filled slot), n after, 0}
 * One call on B samples leaves label, unc, age, occ, n, accepted and slot_of as B calls on one sample each, bit for bit.
 * A filled slot whose label lies outside [0, K), or an n outside [0, N], is never used as an index (the slot counts as a class of
 * occupancy 0; n is clamped).  Columns K.. of p and entries past B, N, K are not touched.  No atomics, fixed order: bit-identical
 * on repetition.  The call allocates nothing and reads nothing back.
 * A NULL pointer, B < 1, K < 1, N < 1, ld < K, ldp < K, N or K beyond the bounds, or a lambda that is negative, not finite or NaN,
 * is refused before any launch: nothing is written. */
int stil_rotta_bank_update(const float* Zt, int ld, int B, int K, int N, float lambda_t, float lambda_u, int* label, float* unc,
                           int* age, int* occ, int* n, int* owner, double* lse, float* p, int ldp, float* H, int* yhat,
                           unsigned char* accepted, int* slot_of, int* counts, void* stream);

/* The samples the update accepted, gathered into the bank: for every slot s < N with 0 <= owner[s] < B
 *   bank_img[s, 0:img_floats] <- x_img[owner[s], 0:img_floats];   bank_tab[s, 0:tab_floats] <- x_tab[owner[s], 0:tab_floats]
 * a bit-exact copy with one writer per element (no race); every other slot, and an owner outside [0, B), is left alone.  One
 * launch over (chunk of 4096 floats, slot); the workgroups of untouched slots leave at once.  The image rows move as 16-byte
 * loads and stores, consecutive lanes on consecutive 16 bytes, when img_floats is a multiple of 4 and both image bases are
 * 16-byte aligned, else float by float; the table rows likewise by tab_floats and their own bases.  The bytes moved are
 * 2 x (owned slots) x 4 (img_floats + tab_floats).  1 <= N <= STIL_ROTTA_MAX_SLOTS.
 * A NULL pointer, N < 1 or beyond the bound, B < 1, img_floats < 1 or tab_floats < 1 is refused before any launch. */
int stil_rotta_bank_store(const float* x_img, const float* x_tab, const int* owner, int N, int B, long img_floats, int tab_floats,
                          float* bank_img, float* bank_tab, void* stream);

/* The loss on the bank: student logits Zs [rows, K] (stride lds >= K) against teacher logits Zt [rows, K] (stride ldt >= K),
 * rows = N the bank's slots, with the slots' label and age:
 *   pt = softmax(Zt_i), ps = softmax(Zs_i), both through a log-sum-exp in double
 *   v_i = [label[i] >= 0];  n = sum_i v_i
 *   e_i = exp(-age[i] / rows);  w[i] = v_i e_i / (1 + e_i)      (RoTTA's timeliness weight: 1/2 at age 0, 0 for huge ages)
 *   ce[i] = -sum_k pt_ik log ps_ik                              (float [rows]; 0 for an empty slot)
 *   loss  = (1 / n) sum_i w[i] ce[i]                            (float [1]; 0 when n == 0)
 *   dZ[i,k] = grad_scale w[i] (ps_ik - pt_ik) / n               (stride ldd >= K; exactly 0 for an empty slot and when n == 0):
 *             with grad_scale = 1, d loss / d Zs (the teacher and the weights are constants)
 *   counts = {n, rows, 0, 0}                                    (int [4])
 *   active_out[t] = active[t] and n > 0                         (the gate of the Adam step, as stil_eata_rows writes it; n_tensors
 *                                                                == 0: neither mask is read or written)
 * Everything is formed in double and rounded once; fixed-order sums, no atomics: bit-identical on repetition.  Columns K.. of dZ
 * and entries past rows are not touched.  ws: at least 4 rows doubles of scratch (written before it is read).  Three launches:
 * one workgroup per row; one workgroup for n, loss, counts and the gate; one workgroup per row for dZ.  Nothing is read back.
 * A NULL required pointer, rows < 1, K < 1, a leading dimension below K, a grad_scale that is not finite, or n_tensors < 0 (or > 0
 * without both masks), is refused before any launch: nothing is written. */
int stil_rotta_rows(const float* Zs, int lds, const float* Zt, int ldt, const int* label, const int* age, int rows, int K,
                    float grad_scale, float* ce, float* w, float* dZ, int ldd, int* counts, float* loss, const unsigned char* active,
                    unsigned char* active_out, int n_tensors, double* ws, void* stream);

/* A <-> teacher over the adapted set A, in the layout of stil_sar_restore (include/stil_sar.h): `achunks` lists the 1024-float
 * slab chunks of A, chunk j of the compact `teacher` belongs to slab chunk achunks[j].  A bit-exact swap, its own inverse.  Only
 * chunks that are in range, whose tensor is in range and active, are touched; a skipped entry never forms an address.  One
 * launch, one block per listed chunk (a chunk listed twice would race: the list of a CompactState names each chunk once).
 * A NULL pointer, an n that is no multiple of 1024 or negative, a negative n_achunks or n_tensors, or a slab that is not 16-byte
 * aligned, is refused before any launch: nothing is written. */
int stil_rotta_exchange(float* params, float* teacher, const int* achunks, int n_achunks, const int* chunk2tensor,
                        const unsigned char* active, int n_tensors, long n, void* stream);

/* The teacher's moving average, same layout:  teacher[j] <- (1 - nu) teacher[j] + nu params[i], formed in double, rounded once;
 * nu in [0, 1].  nu == 0 launches nothing (teacher is bit-identical); nu == 1 copies A.  `active` may be the gated mask of
 * stil_rotta_rows: a batch with n == 0 then moves no teacher.  Refusals as stil_rotta_exchange, and a nu outside [0, 1] or NaN. */
int stil_rotta_teacher(const float* params, float* teacher, const int* achunks, int n_achunks, const int* chunk2tensor,
                       const unsigned char* active, int n_tensors, long n, float nu, void* stream);

#ifdef __cplusplus
}
#endif
