// STiL's unlabelled-data branch as a test-time adaptation loss (models/Disentangle/STiLModel.py:255-303 with use_ema False): the
// consensus-guided pseudo-label over the three classifier heads (CGPL), smoothed by the prototype classifier (PGLS), and one soft
// cross-entropy per head on the rows its case assigns to it.  csrc/stil_cgpl.h states the arithmetic.
// Two launches, no atomics:
//   rows    one 256-thread workgroup per row, any K >= 1 (every thread strides the row): tta_row_lse_h for each head (lse3[0] and p
//           are stil_entropy_rows' bit for bit), the first maximum of each head as stil_deyo_rows finds it, the case, the softmax of
//           the agreeing heads' mean logits, with rate < 1 the prototype logits (one wave per class, lanes over Dp: coalesced reads
//           of protos) -> ws and their softmax, then q, conf, mask1, the three cross-entropies and the three dZ
//   finish  one workgroup: out, counts and the gate of the Adam step from ce3, flags and coin, in a fixed order
// ws (doubles): the prototype logits [rows, K], only when rate < 1.
#include "tta_common.h"
#include "stil_cgpl.h"

struct CgplRowsArgs {
  const float* zm; const float* zi; const float* zt; int ld;
  const float* feat; const float* protos; const unsigned char* coin;
  int K, Dp;
  double T, rate, th, gscale;
  double* lse3; float* p; float* q; int ldp;
  float* conf; unsigned char* flags; float* ce3;
  float* dz[3]; int ldd;
  double* ws;
};

// the rows each head learns from (STiLModel.py:301-303): bit 0 multimodal, bit 1 imaging, bit 2 tabular
__device__ __forceinline__ int cgpl_weights(int cs, int mask1, int coin) {
  if (!mask1) return 0;
  const int wm = cs == 1;
  const int wi = cs == 1 || cs == 3 || (cs == 4 && coin);
  const int wt = cs == 1 || cs == 2 || (cs == 4 && !coin);
  return wm | (wi << 1) | (wt << 2);
}

// the mean of the agreeing heads' logits at column k
__device__ __forceinline__ double cgpl_mean_logit(int cs, const float* __restrict__ zm, const float* __restrict__ zi,
                                                  const float* __restrict__ zt, int k) {
  const double m = (double)zm[k];
  if (cs == 1) return (m + (double)zi[k] + (double)zt[k]) / 3.0;
  if (cs == 2) return (m + (double)zi[k]) / 2.0;
  if (cs == 3) return (m + (double)zt[k]) / 2.0;
  return m;
}

// log sum_k exp(v_k) of K doubles produced by `at(k)`, by one 256-thread block
template <class At>
__device__ __forceinline__ double cgpl_lse_d(int K, At at, double* redd) {
  double m = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) m = fmax(m, at(k));
  m = block_reduce<4>(m, redd, [](double a, double b) { return fmax(a, b); });
  double s = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) s += exp(at(k) - m);
  s = block_sum_d(s, redd);
  return m + log(s);
}

__global__ __launch_bounds__(256) void cgpl_rows_kernel(CgplRowsArgs a) {
  __shared__ float red[16];
  __shared__ double redd[16];
  __shared__ int redi[4];
  const int r = blockIdx.x, rows = gridDim.x, K = a.K, tid = threadIdx.x;
  const float* zh[3] = {a.zm + (long)r * a.ld, a.zi + (long)r * a.ld, a.zt + (long)r * a.ld};
  double L[3], h_unused;
  int top[3];
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    tta_row_lse_h(zh[h], K, red, redd, L[h], h_unused);
    top[h] = tta_first_max(zh[h], K, red, redi);
  }
  int cs;
  if (top[0] == top[1] && top[0] == top[2]) cs = 1;
  else if (top[0] == top[1]) cs = 2;
  else if (top[0] == top[2]) cs = 3;
  else cs = 4;
  const double La = cgpl_lse_d(K, [&](int k) { return cgpl_mean_logit(cs, zh[0], zh[1], zh[2], k); }, redd);
  const bool smooth = a.rate < 1.0;
  double* tl = a.ws ? a.ws + (long)r * K : nullptr;  // the prototype logits of this row
  double Lt = 0.0;
  if (smooth) {
    const float* f = a.feat + (long)r * a.Dp;
    const int w = tid >> 6, lane = tid & 63;
    for (int k = w; k < K; k += 4) {  // uniform per wave
      const float* pr = a.protos + (long)k * a.Dp;
      double s = 0.0;
      for (int c = lane; c < a.Dp; c += 64) s += (double)f[c] * (double)pr[c];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (lane == 0) tl[k] = s / a.T;
    }
    __syncthreads();  // the block's own global writes, before any of its threads reads them
    Lt = cgpl_lse_d(K, [&](int k) { return tl[k]; }, redd);
  }
  // q, p, the confidence and the three cross-entropies
  double cmax = -INFINITY, ce[3] = {0.0, 0.0, 0.0};
  for (int k = tid; k < K; k += 256) {
    const double pm = exp((double)zh[0][k] - L[0]);
    double qk = exp(cgpl_mean_logit(cs, zh[0], zh[1], zh[2], k) - La), pred = pm;
    if (smooth) {
      const double tp = exp(tl[k] - Lt);
      qk = a.rate * qk + (1.0 - a.rate) * tp;
      pred = a.rate * pm + (1.0 - a.rate) * tp;
    }
    if (a.p) a.p[(long)r * a.ldp + k] = (float)pm;
    a.q[(long)r * a.ldp + k] = (float)qk;
    cmax = fmax(cmax, pred);
#pragma unroll
    for (int h = 0; h < 3; ++h) ce[h] -= qk * ((double)zh[h][k] - L[h]);
  }
  cmax = block_reduce<4>(cmax, redd, [](double a, double b) { return fmax(a, b); });
#pragma unroll
  for (int h = 0; h < 3; ++h) ce[h] = block_sum_d(ce[h], redd);
  const int mask1 = cmax >= a.th;
  const int wbits = cgpl_weights(cs, mask1, a.coin[r] != 0);
  if (tid == 0) {
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      a.lse3[(long)h * rows + r] = L[h];
      a.ce3[(long)h * rows + r] = (float)ce[h];
    }
    a.conf[r] = (float)cmax;
    a.flags[(long)r * 4 + 0] = (unsigned char)cs;
    a.flags[(long)r * 4 + 1] = (unsigned char)mask1;
    a.flags[(long)r * 4 + 2] = (unsigned char)mask1;
    a.flags[(long)r * 4 + 3] = 0;
  }
  if (!a.dz[0] && !a.dz[1] && !a.dz[2]) return;
  for (int k = tid; k < K; k += 256) {
    double qk = 0.0;
    if (wbits) {
      qk = exp(cgpl_mean_logit(cs, zh[0], zh[1], zh[2], k) - La);
      if (smooth) qk = a.rate * qk + (1.0 - a.rate) * exp(tl[k] - Lt);
    }
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      if (!a.dz[h]) continue;
      const bool on = (wbits >> h) & 1;  // uniform across the block
      a.dz[h][(long)r * a.ldd + k] = on ? (float)(a.gscale * (exp((double)zh[h][k] - L[h]) - qk)) : 0.f;
    }
  }
}

// one block: the four losses, the five counts and the gate
__global__ __launch_bounds__(256) void cgpl_finish_kernel(int rows, const float* __restrict__ ce3, const unsigned char* __restrict__ flags,
                                                           const unsigned char* __restrict__ coin, int* __restrict__ counts,
                                                           float* __restrict__ out, const unsigned char* __restrict__ active,
                                                           unsigned char* __restrict__ gate, int n_tensors) {
  __shared__ double redd[16];
  double s[3] = {0.0, 0.0, 0.0}, c[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < rows; i += 256) {
    const int cs = flags[(long)i * 4], mask1 = flags[(long)i * 4 + 1];
    const int wbits = cgpl_weights(cs, mask1, coin[i] != 0);
#pragma unroll
    for (int h = 0; h < 3; ++h)
      if ((wbits >> h) & 1) s[h] += (double)ce3[(long)h * rows + i];
    if (mask1) c[0] += 1.0;
    if (cs >= 1 && cs <= 4) c[cs] += 1.0;
  }
#pragma unroll
  for (int h = 0; h < 3; ++h) s[h] = block_sum_d(s[h], redd);
#pragma unroll
  for (int j = 0; j < 5; ++j) c[j] = block_sum_d(c[j], redd);  // integers below 2^53: exact
  const int n = (int)c[0];
  if (threadIdx.x == 0) {
    const double R = (double)rows;
    out[0] = (float)((s[0] + s[1] + s[2]) / R);
#pragma unroll
    for (int h = 0; h < 3; ++h) out[1 + h] = (float)(s[h] / R);
#pragma unroll
    for (int j = 0; j < 5; ++j) counts[j] = (int)c[j];
  }
  tta_gate(active, gate, n_tensors, n);
}

extern "C" int stil_cgpl_rows(const float* Zm, const float* Zi, const float* Zt, int ld, const float* feat, const float* protos,
                              const unsigned char* coin, int rows, int K, int Dp, float T, float rate, float th, float grad_scale,
                              double* lse3, float* p, float* q, int ldp, float* conf, unsigned char* flags, float* ce3, float* dZm,
                              float* dZi, float* dZt, int ldd, int* counts, float* out, const unsigned char* active,
                              unsigned char* gate, int n_tensors, double* ws, void* stream) {
  STIL_REQUIRE(Zm && Zi && Zt && coin && lse3 && q && conf && flags && ce3 && counts && out, "stil_cgpl_rows: null pointer");
  STIL_REQUIRE(rows >= 1 && K >= 1 && Dp >= 1 && ld >= K, "stil_cgpl_rows: bad shape rows=%d K=%d Dp=%d ld=%d", rows, K, Dp, ld);
  STIL_REQUIRE(ldp >= K, "stil_cgpl_rows: ldp=%d < K=%d", ldp, K);
  STIL_REQUIRE((!dZm && !dZi && !dZt) || ldd >= K, "stil_cgpl_rows: ldd=%d < K=%d", ldd, K);
  STIL_REQUIRE(rate >= 0.0f && rate <= 1.0f, "stil_cgpl_rows: rate=%g is not in [0, 1]", (double)rate);
  STIL_REQUIRE(rate == 1.0f || (feat && protos && ws), "stil_cgpl_rows: rate=%g < 1 needs feat, protos and ws", (double)rate);
  STIL_REQUIRE(rate == 1.0f || (T > 0.0f && T <= 3.402823466e38f), "stil_cgpl_rows: T=%g is not finite and positive", (double)T);
  STIL_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (active && gate)), "stil_cgpl_rows: n_tensors=%d needs both masks", n_tensors);
  hipStream_t s = (hipStream_t)stream;
  CgplRowsArgs a;
  a.zm = Zm; a.zi = Zi; a.zt = Zt; a.ld = ld;
  a.feat = feat; a.protos = protos; a.coin = coin;
  a.K = K; a.Dp = Dp;
  a.T = (double)T; a.rate = (double)rate; a.th = (double)th; a.gscale = (double)grad_scale;
  a.lse3 = lse3; a.p = p; a.q = q; a.ldp = ldp;
  a.conf = conf; a.flags = flags; a.ce3 = ce3;
  a.dz[0] = dZm; a.dz[1] = dZi; a.dz[2] = dZt; a.ldd = ldd;
  a.ws = rate == 1.0f ? nullptr : ws;
  hipLaunchKernelGGL(cgpl_rows_kernel, dim3(rows), dim3(256), 0, s, a);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(cgpl_finish_kernel, dim3(1), dim3(256), 0, s, rows, (const float*)ce3, (const unsigned char*)flags, coin, counts,
                     out, active, gate, n_tensors);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
