// Test-time adaptation, DeYO (Lee et al., ICLR 2024, "Entropy is not enough for test-time adaptation: from the perspective of
// disentangled factors") on top of TENT (csrc/tta.hip), beside EATA (csrc/eata.hip): a second, forward-only look at every
// image with its patches shuffled (object shape destroyed, local texture and colour kept), and a row loss that keeps the rows
// that are confident (H_r < tau_Ent) AND whose predicted-class probability drops under that destruction (PLPD_r > tau_PLPD).
//
// stil_patch_shuffle: dst[b, c, y, x] = src[b, c, (q / g) ph + y % ph, (q % g) pw + x % pw], q = perm[b, (y / ph) g + x / pw]
//   (q outside [0, g^2): q = the slot itself).  One launch, grid = (chunks of one image, images): one lane per 16 bytes of dst
//   (pw % 4 == 0: a 16-byte piece never straddles a patch, source and destination pieces are both aligned) or per float.
//   Stores are fully coalesced; loads are coalesced in runs of pw floats.  In-image offsets are 32-bit (C H W < 2^31), the image
//   base is 64-bit.
// stil_deyo_rows, per row r of Z and Zs [rows, K]:
//   lse_r, p_rk, H_r                as stil_entropy_rows (tta_row_lse_h of csrc/tta_common.h: bit-identical)
//   yhat_r = first maximum of Z_r ; plpd_r = p_r[yhat_r] - softmax(Zs_r)[yhat_r]
//   rel_r = H_r < tau_Ent ; sel_r = rel_r and plpd_r > tau_PLPD ; w_r = a_ent exp(E0 - H_r) + a_plpd exp(plpd_r)
//   n = sum sel, n_reliable = sum rel, L = (1/n) sum sel w H   (0 when n == 0)
//   active_out[t] = active[t] and n > 0                        (the gate of the Adam step: n never leaves the device)
//   dZ_rk = sel_r w_r (-p_rk (log p_rk + H_r)) grad_scale / n  (0 when n == 0)
// Everything is formed in double and rounded once; reductions are wave64 shuffle trees plus a fixed-order sum of the wave
// partials; no float atomics: bit-identical on repetition.  Three launches: rows, reduce, dZ (tta_sel_dz_kernel of
// csrc/tta_common.h, which reads the double lse, H and w of the first back).  The loss and f = w grad_scale / n come from the code
// eata.hip uses (tta_sel_sums, tta_sel_dz_kernel), so that with a_ent = 1, a_plpd = 0 the results are stil_eata_rows's
// (m invalid) bit for bit.
#include "tta_common.h"

template <int VEC>
__global__ __launch_bounds__(256) void patch_shuffle_kernel(const float* __restrict__ src, float* __restrict__ dst, unsigned H,
                                                             unsigned W, unsigned g, unsigned ph, unsigned pw, unsigned per_image,
                                                             const int* __restrict__ perm) {
  // per_image = C H W / VEC pieces; j indexes the piece inside image b
  const unsigned j = blockIdx.x * 256u + threadIdx.x;
  if (j >= per_image) return;
  const unsigned b = blockIdx.y;
  const unsigned wv = W / VEC;
  const unsigned t = j / wv, x = (j - t * wv) * VEC;  // t = c H + y
  const unsigned c = t / H, y = t - c * H;
  const unsigned py = y / ph, px = x / pw;
  const unsigned slot = py * g + px, g2 = g * g;
  unsigned q = (unsigned)perm[(size_t)b * g2 + slot];
  if (q >= g2) q = slot;  // negative entries wrap above g2 too: the slot stays in place
  const unsigned qy = q / g, qx = q - qy * g;
  const unsigned sy = qy * ph + (y - py * ph), sx = qx * pw + (x - px * pw);
  const size_t base = (size_t)b * per_image * VEC;
  const size_t so = base + ((size_t)c * H + sy) * W + sx, d = base + (size_t)j * VEC;
  if (VEC == 4)
    *reinterpret_cast<float4*>(dst + d) = *reinterpret_cast<const float4*>(src + so);
  else
    dst[d] = src[so];
}

extern "C" int stil_patch_shuffle(const float* src, float* dst, int B, int C, int H, int W, int grid, const int* perm,
                                  void* stream) {
  STIL_REQUIRE(src && dst && perm, "stil_patch_shuffle: null pointer");
  STIL_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && grid >= 1, "stil_patch_shuffle: bad shape B=%d C=%d H=%d W=%d grid=%d", B, C, H, W, grid);
  STIL_REQUIRE(B <= 65535, "stil_patch_shuffle: B=%d above 65535", B);
  STIL_REQUIRE(H % grid == 0 && W % grid == 0, "stil_patch_shuffle: grid=%d must divide H=%d and W=%d", grid, H, W);
  STIL_REQUIRE(grid <= 32768, "stil_patch_shuffle: grid=%d too large", grid);
  const long chw = (long)C * H * W;
  STIL_REQUIRE(chw < (1L << 31), "stil_patch_shuffle: C H W = %ld must stay below 2^31", chw);
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst, bytes = (uintptr_t)B * chw * sizeof(float);
  STIL_REQUIRE(s0 + bytes <= d0 || d0 + bytes <= s0, "stil_patch_shuffle: src and dst overlap");
  const unsigned ph = H / grid, pw = W / grid;
  hipStream_t s = (hipStream_t)stream;
  if (pw % 4 == 0 && s0 % 16 == 0 && d0 % 16 == 0) {
    const unsigned per = (unsigned)(chw / 4);
    hipLaunchKernelGGL(patch_shuffle_kernel<4>, dim3(cdiv(per, 256), B), dim3(256), 0, s, src, dst, (unsigned)H, (unsigned)W,
                       (unsigned)grid, ph, pw, per, perm);
  } else {
    const unsigned per = (unsigned)chw;
    hipLaunchKernelGGL(patch_shuffle_kernel<1>, dim3(cdiv(per, 256), B), dim3(256), 0, s, src, dst, (unsigned)H, (unsigned)W,
                       (unsigned)grid, ph, pw, per, perm);
  }
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

__global__ __launch_bounds__(256) void deyo_rows_kernel(const float* __restrict__ Z, int ld, const float* __restrict__ Zs, int lds,
                                                         int K, double tau_ent, double tau_plpd, double e0, double a_ent,
                                                         double a_plpd, double* __restrict__ lse, double* __restrict__ Hd,
                                                         double* __restrict__ Wd, float* __restrict__ p, int ldp,
                                                         float* __restrict__ H, float* __restrict__ plpd, float* __restrict__ w,
                                                         int* __restrict__ yhat, unsigned char* __restrict__ rel,
                                                         unsigned char* __restrict__ sel) {
  __shared__ float red[16];
  __shared__ double redd[16];
  __shared__ int redi[4];
  const int r = blockIdx.x;
  const float* zr = Z + (long)r * ld;
  const float* zs = Zs + (long)r * lds;
  double L, h;
  tta_row_lse_h(zr, K, red, redd, L, h);
  float m = -INFINITY, ms = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) {
    const float z = zr[k];
    p[(long)r * ldp + k] = (float)exp((double)z - L);
    m = fmaxf(m, z);
    ms = fmaxf(ms, zs[k]);
  }
  m = block_max(m, red);
  ms = block_max(ms, red);
  int yi = INT_MAX;
  double ss = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) {
    if (zr[k] == m) yi = min(yi, k);
    ss += exp((double)zs[k] - (double)ms);
  }
  yi = block_reduce<4>(yi, redi, [](int a, int b) { return min(a, b); });
  if (yi >= K) yi = 0;  // a row without a maximum (every logit NaN): any index in range
  ss = block_sum_d(ss, redd);
  if (threadIdx.x == 0) {
    const double Ls = (double)ms + log(ss);
    const double d = exp((double)zr[yi] - L) - exp((double)zs[yi] - Ls);
    const double wd = a_ent * exp(e0 - h) + a_plpd * exp(d);
    const int is_rel = h < tau_ent;
    lse[r] = L;
    Hd[r] = h;  // the dZ kernel reads the double H and w back: no second reduction
    Wd[r] = wd;
    H[r] = (float)h;
    plpd[r] = (float)d;
    w[r] = (float)wd;
    yhat[r] = yi;
    rel[r] = (unsigned char)is_rel;
    sel[r] = (unsigned char)(is_rel && d > tau_plpd);
  }
}

// one block: n, n_reliable, the loss and the gate
__global__ __launch_bounds__(256) void deyo_reduce_kernel(int rows, const float* __restrict__ H, const float* __restrict__ w,
                                                           const unsigned char* __restrict__ rel,
                                                           const unsigned char* __restrict__ sel, int* __restrict__ counts,
                                                           float* __restrict__ loss, const unsigned char* __restrict__ active,
                                                           unsigned char* __restrict__ active_out, int n_tensors) {
  __shared__ double redd[16];
  const TtaSelSums sums = tta_sel_sums(rows, H, w, rel, sel, redd);
  const int n = (int)sums.n;
  if (threadIdx.x == 0) {
    counts[0] = n;
    counts[1] = (int)sums.n_rel;
    counts[2] = 0;
    counts[3] = 0;
    loss[0] = n > 0 ? (float)(sums.wh / sums.n) : 0.f;
  }
  tta_gate(active, active_out, n_tensors, n);
}

extern "C" int stil_deyo_rows(const float* Z, int ld, const float* Zs, int lds, int rows, int K, float ent_margin,
                              float plpd_margin, float e0, float a_ent, float a_plpd, float grad_scale, double* lse, double* Hd,
                              double* Wd, float* p, int ldp, float* H, float* plpd, float* w, int* yhat, unsigned char* rel,
                              unsigned char* sel, float* dZ, int ldd, int* counts, float* loss, const unsigned char* active,
                              unsigned char* active_out, int n_tensors, void* stream) {
  STIL_REQUIRE(Z && Zs && lse && Hd && Wd && p && H && plpd && w && yhat && rel && sel && dZ && counts && loss, "stil_deyo_rows: null pointer");
  STIL_REQUIRE(rows >= 1 && K >= 1 && ld >= K && lds >= K, "stil_deyo_rows: bad shape rows=%d K=%d ld=%d lds=%d", rows, K, ld, lds);
  STIL_REQUIRE(ldp >= K && ldd >= K, "stil_deyo_rows: ldp=%d ldd=%d < K=%d", ldp, ldd, K);
  STIL_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (active && active_out)), "stil_deyo_rows: n_tensors=%d needs both masks", n_tensors);
  STIL_REQUIRE(a_ent >= 0.f && a_plpd >= 0.f && a_ent < INFINITY && a_plpd < INFINITY, "stil_deyo_rows: a_ent=%g a_plpd=%g", (double)a_ent, (double)a_plpd);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(deyo_rows_kernel, dim3(rows), dim3(256), 0, s, Z, ld, Zs, lds, K, (double)ent_margin, (double)plpd_margin,
                     (double)e0, (double)a_ent, (double)a_plpd, lse, Hd, Wd, p, ldp, H, plpd, w, yhat, rel, sel);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(deyo_reduce_kernel, dim3(1), dim3(256), 0, s, rows, (const float*)H, (const float*)w, (const unsigned char*)rel,
                     (const unsigned char*)sel, counts, loss, active, active_out, n_tensors);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(tta_sel_dz_kernel<TtaWeightStored>, dim3(rows), dim3(256), 0, s, Z, ld, K, TtaWeightStored{Wd}, (double)grad_scale,
                     (const double*)lse, (const double*)Hd, (const unsigned char*)sel, (const int*)counts, dZ, ldd);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
