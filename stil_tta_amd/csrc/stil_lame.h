/* C ABI of libstil_hip.so: LAME (Boudiaf, Mueller, Ben Ayed, Bertinetto, CVPR 2022, "Parameter-free Online Test-time Adaptation";
 * definition and defaults as recalled from the paper and its published code: unpinned), the forward-only correction of a batch's
 * output probabilities: rows whose features are neighbours are pulled towards the same prediction by a few fixed-point
 * iterations of a Laplacian-regularised likelihood.  Nothing of the model is read or written: the inputs are the logits and the
 * features of one batch.
 * Kept beside its kernels (lame.hip) and out of include/, whose headers form closed ledgers; stil_tta_amd/_lib.py binds it
 * through LAME_HEADERS (tests/test_lame_abi_ledger_cpu.py is this header's ledger).
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream).
 * Both entries form every decision and sum in double from the float inputs and round every output once; every sum runs in a
 * fixed order without atomics (bit-identical on repetition); no workgroup waits on another inside a launch; neither allocates
 * nor reads anything back to the host.
 * Unlike the published code, on purpose: everything is formed in double; the energy uses A Y^(n-1), exactly what the update read;
 * the tie and NaN rules of the neighbour selection are this project's; the "linear" affinity is not built. */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STIL_LAME_MAX_ROWS 2048 /* rows of one batch: a row's distances are ranked in the LDS of its workgroup */
#define STIL_LAME_KNN 0         /* kind: w_ij = 1 on the neighbours */
#define STIL_LAME_RBF 1         /* kind: w_ij = exp(-d2_ij / (2 s2)) on the neighbours */

/* The k-nearest-neighbour affinity over the features F [rows, D] (row stride ldf >= D; 1 <= rows <= STIL_LAME_MAX_ROWS, any D >= 1,
 * any k >= 1), with k' = min(k, rows - 1):
 *   fhat_i  = f_i / max(|f_i|, 1e-12);   d2_ij = max(0, 2 - 2 <fhat_i, fhat_j>)       (a NaN stays a NaN)
 *   N_i     = the k' indices j != i of smallest d2_ij, in ascending order of d2; ties go to the lower j; a NaN distance orders
 *             as +inf and after every finite one: the order is total and every index written is in range whatever F holds
 *   nbr[i,t] = the t-th entry of N_i for t < k', -1 for k' <= t < k                    (int [rows, k], dense)
 *   dk[i]   = d2 from i to its k'-th neighbour, 0 when k' == 0                         (double [rows])
 *   s2      = (1 / rows) sum_i dk[i]                                                   (kind STIL_LAME_RBF only)
 *   wts[i,t] = 1 (STIL_LAME_KNN);  exp(-d2_ij / (2 s2)), j = nbr[i,t], and 1 when s2 <= 1e-12 (STIL_LAME_RBF);  0 for k' <= t < k
 *                                                                                      (float [rows, k], dense)
 * The Gram products are formed in double: rows^2 D double multiply-adds per call, 1e8 at rows 256 and D 1536.  Nobody has measured it.
 * Rows past `rows` of nbr, wts and dk are not touched.
 * ws: at least rows (1 + min(k, rows)) doubles of scratch (written before it is read).  Three launches: one workgroup per row for
 * the norms; one workgroup per row for that row's distances (one wave per pair, in LDS) and their ranks, which give nbr and dk
 * without a sort; one workgroup per row for s2 (every workgroup sums dk in the same order) and wts.
 * A NULL pointer (F, nbr, wts, dk, ws), rows < 1, D < 1, k < 1, rows > STIL_LAME_MAX_ROWS, ldf < D, or a kind other than the two,
 * is refused before any launch: nothing is written. */
int stil_lame_affinity(const float* F, int ldf, int rows, int D, int k, int kind, int* nbr, float* wts, double* dk, double* ws,
                       void* stream);

/* The correction of the logits Z [rows, K] (row stride ld >= K; 1 <= rows <= STIL_LAME_MAX_ROWS, any K >= 1) under the affinity
 * (nbr, wts) [rows, k] of stil_lame_affinity (entries of nbr outside [0, rows) stand for no neighbour), lambda >= 0, max_steps >= 1,
 * tol >= 0:
 *   lse[r], p[r,c]  as stil_entropy_rows, bit for bit (double [rows]; float, stride ldp >= K); pd = softmax(Z) before its rounding
 *   W_ij    = sum over the t with nbr[i,t] == j of wts[i,t] (one t at most from stil_lame_affinity), W_ii = 0;   A = (W + W^T) / 2
 *   u       = log(pd + 1e-10);   Y^0 = softmax(u)
 *   Y^n_i   = softmax_c(u_i + lambda sum_j A_ij Y^(n-1)_j),  n = 1, 2, ...      (Jacobi: every row reads the previous iterate)
 *   E_n     = sum_ic Y^n_ic (-u_ic - lambda (A Y^(n-1))_ic + log max(Y^n_ic, 1e-20))
 *   stop after step n >= 2 when |E_n - E_(n-1)| <= tol |E_(n-1)|; tol == 0 switches the rule off; at most max_steps steps run
 *   steps[0] = the number of steps performed (int [1]);   Y = Y^steps (float [rows, K], stride ldy >= K)
 *   energy[n-1] = E_n for n = 1..steps (double [max_steps]); the entries from `steps` on are not touched
 * rows == 1 or no neighbour at all is no special case: A = 0, Y = softmax(u), steps = 2 (with tol > 0 and max_steps >= 2).
 * The sum over j runs in ascending j over the non-zero A_ij; E_n is the fixed-order sum of one partial per row.
 * Columns K.. of p and Y, and rows past `rows`, are not touched.
 * ws: at least 2 rows^2 + 3 rows K + 3 rows + 2 doubles of scratch (written before it is read):
 *   the non-zero A_ij of every row [rows, rows] | their j (int) [rows, rows] | u [rows, K] | Y ping [rows, K] | Y pong [rows, K] |
 *   energy partials [2, rows] | non-zeros per row (int) [rows] | the stopping word
 * The call makes 2 + max_steps + 1 launches, one workgroup per row each: the rows (lse, p, u, Y^0), the graph (every row of A,
 * compacted in ascending j), then one launch per step and a last one that only closes the count.  The stopping rule is decided on the device: the launch of step n + 1
 * first has every workgroup sum the per-row partials of E_n in the same fixed order, so all reach the same decision; once the rule
 * has fired, the launches still enqueued return at once on the stopping word read from ws.
 * A NULL pointer (Z, nbr, wts, lse, p, Y, energy, steps, ws), rows < 1, K < 1, k < 1, rows > STIL_LAME_MAX_ROWS, a leading dimension
 * below K, a lambda or tol that is negative or not finite, or max_steps < 1, is refused before any launch: nothing is written. */
int stil_lame_rows(const float* Z, int ld, int rows, int K, const int* nbr, const float* wts, int k, float lambda, int max_steps,
                   float tol, double* lse, float* p, int ldp, float* Y, int ldy, double* energy, int* steps, double* ws,
                   void* stream);

#ifdef __cplusplus
}
#endif
