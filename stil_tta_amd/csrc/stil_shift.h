/* C ABI of libstil_hip.so: the shifted test stream -- image corruptions and tabular shifts applied to a batch on the device
 * (stil_tta_amd/shift.py).  Kept beside its kernels (shift.hip) and out of include/, whose headers form closed
 * ledgers; stil_tta_amd/_lib.py binds it through SHIFT_HEADERS (tests/test_shift_abi_ledger_cpu.py is this header's ledger).
 * Every entry returns 0 on success (STIL_OK) and a negative code otherwise (message: stil_last_error()).
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream).
 *
 * Common to all entries.  Images are float32 [B, C, H, W], contiguous; tables are float32 [B, n_cols] with the num_cat categorical
 * code columns first.  No entry allocates, synchronises or uses atomics: a repeated call gives the same bits.  `out` must not
 * overlap `x`.  clip(v) = lo where v < lo, hi where v > hi, else v (NaN passes; lo = -inf, hi = +inf disables it).
 * Random numbers: h(seed, ctr) is the 64 -> 32-bit counter hash of stil_tab_corrupt_draw; r24(ctr) = h >> 8 and
 * u(ctr) = r24(ctr) 2^-24, exact in float32.  Counters are 64-bit and global to the stream: element i of a call is element
 * e = offset + i of the stream, where `offset` counts the elements earlier calls consumed (the host keeps it).  The normal of
 * element e belongs to pair j = e >> 1: u1 = (r24(2j) + 1) 2^-24, u2 = u(2j + 1), rho = sqrt(-2 ln u1); g(e) = rho cos(2 pi u2) for
 * even e and rho sin(2 pi u2) for odd e, in float32.  Two calls that cut a range of elements anywhere, at an odd element too, give
 * the bits of one call over the whole range.
 * A NULL required pointer, an empty shape, an overlapping out, an unknown kind, a strength outside its range or NaN, or an empty or
 * NaN clip range is refused before any launch: nothing is written. */
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Noise over n = B C H W elements.
 *   kind 0 (Gaussian, strength = sigma >= 0):  out = clip(x + strength g(e))
 *   kind 1 (impulse, strength = amount in [0, 1]): u(e) < strength / 2: lo;  strength / 2 <= u(e) < strength: hi;  otherwise x
 *                                               (float32 against float32, exact on both sides)
 * 16-byte accesses when x and out are 16-byte aligned and n % 4 == 0, else 4-byte ones; the bits do not depend on which. */
int stil_shift_noise(const float* x, float* out, long n, int kind, float strength, float lo, float hi, unsigned long long seed,
                     unsigned long long offset, void* stream);

/* Contrast: m[b,c] = the mean of plane (b, c), accumulated in double in a fixed order and rounded to float32 into mean_ws [B C];
 * out = clip((x - m) factor + m), factor >= 0.  A constant plane comes back bit for bit.  Two launches. */
int stil_shift_contrast(const float* x, float* out, int B, int C, int HW, float factor, float lo, float hi, float* mean_ws, void* stream);

/* Brightness: the value of HSV moved by delta at constant hue and saturation, in closed form (C must be 3):
 *   V = max(r, g, b);  V' = min(max(V, 0) + delta, hi);  V > 0: out_c = clip(x_c (V' / V));  otherwise out_c = V' for every c. */
int stil_shift_brightness(const float* x, float* out, int B, int C, int HW, float delta, float lo, float hi, void* stream);

/* Pixelate: every s x s block, cut from the top-left (edge blocks are smaller when s does not divide H or W), is replaced by its
 * mean; the block is added row-major in float32 and divided by its pixel count.  s = 1 copies bit for bit; s >= max(H, W) is one
 * block per plane.  One thread adds a block, so the cost per thread grows with s^2.  Two launches (one for s = 1). */
int stil_shift_pixelate(const float* x, float* out, int B, int C, int H, int W, int s, void* stream);

/* Tabular shifts.  cat_len: int32 [num_cat], the number of codes of each categorical column (>= 1; may be NULL when num_cat == 0);
 * col_on: uint8 [n_cols], the columns in play; col_std, col_fill: float [n_cols].  Element e = offset + b n_cols + c; a column with
 * col_on == 0 is copied, as is every cell the rule of its kind does not name:
 *   kind 0 (noise, strength >= 0):        continuous columns (c >= num_cat): out = x + (strength col_std[c]) g(e)
 *   kind 1 (missing, strength in [0, 1]): u(e) < strength: out = col_fill[c]
 *   kind 2 (categorical flip, strength in [0, 1]): categorical columns: u(2e) < strength: out = (r24(2e + 1) cat_len[c]) >> 24,
 *                                          integer arithmetic, always < cat_len[c] */
int stil_shift_tab(const float* x, float* out, int B, int n_cols, int num_cat, const int* cat_len, const unsigned char* col_on,
                   const float* col_std, const float* col_fill, int kind, float strength, unsigned long long seed,
                   unsigned long long offset, void* stream);

#ifdef __cplusplus
}
#endif
