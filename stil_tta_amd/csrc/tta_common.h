// What the test-time adaptation kernels share (csrc/tta.hip and the files beside it): the row entropy core, the pieces of the
// selected-row losses, the first maximum of a row, and the walker over the chunks of the adapted set A with its two kernel
// templates, its sum of partials and the argument check of its entry points.
#pragma once
#include "common.h"
#include <limits.h>
#include <initializer_list>

// lse and softmax entropy (double) of one row zr[0:K] by one 256-thread block: shared by stil_entropy_rows and the rows
// kernels of eata.hip, deyo.hip and sar.hip, whose lse, p and H are therefore bit-identical
__device__ __forceinline__ void tta_row_lse_h(const float* __restrict__ zr, int K, float* red, double* redd, double& L, double& h) {
  float m = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) m = fmaxf(m, zr[k]);
  m = block_max(m, red);
  double s = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) s += exp((double)zr[k] - (double)m);
  s = block_sum_d(s, redd);
  L = (double)m + log(s);
  double a = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const double lp = (double)zr[k] - L;
    a -= exp(lp) * lp;
  }
  h = block_sum_d(a, redd);
}

// the first maximum of zr[0:K] by one 256-thread block, in every thread; `redi`: one int per wave
__device__ __forceinline__ int tta_first_max(const float* __restrict__ zr, int K, float* red, int* redi) {
  float m = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) m = fmaxf(m, zr[k]);
  m = block_max(m, red);
  int yi = INT_MAX;
  for (int k = threadIdx.x; k < K; k += 256)
    if (zr[k] == m) yi = min(yi, k);
  yi = block_reduce<4>(yi, redi, [](int a, int b) { return min(a, b); });
  return yi >= K ? 0 : yi;  // a row without a maximum (every logit NaN): any index in range
}

// ---- shared by the selected-row losses (csrc/eata.hip, deyo.hip, sar.hip): each is three launches, its own rows kernel, its
// own reduce kernel built from the two helpers below, and tta_sel_dz_kernel
struct TtaSelSums {
  double n, n_rel, wh;  // selected rows, reliable rows, sum over the selected rows of w H
};

// the sums of EATA's and DeYO's reduce kernels over the float w and H, by one 256-thread block, in every thread
__device__ __forceinline__ TtaSelSums tta_sel_sums(int rows, const float* __restrict__ H, const float* __restrict__ w,
                                                   const unsigned char* __restrict__ rel, const unsigned char* __restrict__ sel,
                                                   double* redd) {
  TtaSelSums s = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < rows; i += 256) {
    if (sel[i]) {
      s.n += 1.0;
      s.wh += (double)w[i] * (double)H[i];
    }
    if (rel[i]) s.n_rel += 1.0;
  }
  s.n = block_sum_d(s.n, redd);  // integers below 2^53: exact
  s.n_rel = block_sum_d(s.n_rel, redd);
  s.wh = block_sum_d(s.wh, redd);
  return s;
}

// the gate of the Adam step, by one 256-thread block: n never leaves the device
__device__ __forceinline__ void tta_gate(const unsigned char* __restrict__ active, unsigned char* __restrict__ active_out,
                                         int n_tensors, int n) {
  for (int t = threadIdx.x; t < n_tensors; t += 256) active_out[t] = (unsigned char)(active[t] && n > 0);
}

// the weight of selected row r, whose double entropy is h: EATA's exp(E0 - H_r), DeYO's stored double w_r, SAR's 1
struct TtaWeightMargin {
  double e0;
  __device__ double operator()(int, double h) const { return exp(e0 - h); }
};
struct TtaWeightStored {
  const double* __restrict__ Wd;
  __device__ double operator()(int r, double) const { return Wd[r]; }
};
struct TtaWeightOne {
  __device__ double operator()(int, double) const { return 1.0; }
};

// dZ_rk = sel_r weight_r (-p_rk (log p_rk + H_r)) grad_scale / n, 0 when n == 0; lse and Hd are the rows kernel's doubles
template <class Weight>
__global__ __launch_bounds__(256) void tta_sel_dz_kernel(const float* __restrict__ Z, int ld, int K, Weight weight, double gscale,
                                                          const double* __restrict__ lse, const double* __restrict__ Hd,
                                                          const unsigned char* __restrict__ sel, const int* __restrict__ counts,
                                                          float* __restrict__ dZ, int ldd) {
  const int r = blockIdx.x;
  const int n = counts[0];
  float* dr = dZ + (long)r * ldd;
  if (n <= 0 || !sel[r]) {  // uniform across the block
    for (int k = threadIdx.x; k < K; k += 256) dr[k] = 0.f;
    return;
  }
  const float* zr = Z + (long)r * ld;
  const double L = lse[r], h = Hd[r];
  const double f = weight(r, h) * gscale / (double)n;  // in this order in every instantiation; exact with weight 1
  for (int k = threadIdx.x; k < K; k += 256) {
    const double lp = (double)zr[k] - L;
    dr[k] = (float)(-exp(lp) * (lp + h) * f);
  }
}

// ---- the slab kernels: one 256-thread block per 1024-float chunk of A listed in `achunks`, one float4 per lane.  An entry that is
// out of range, padding (chunk2tensor < 0) or belongs to an inactive tensor is dead: its block writes nothing (a reducing kernel
// writes partial[j] = 0).  chunk2tensor and active are read as stil_adam_step reads them.  The buffers beside the slab (source
// values, saved values, Fisher estimate, teacher) are compact: chunk j of them belongs to slab chunk achunks[j].
__device__ __forceinline__ bool tta_chunk_live(int ch, long nchunks, const int* __restrict__ chunk2tensor,
                                               const unsigned char* __restrict__ active, int n_tensors) {
  if (ch < 0 || ch >= nchunks) return false;
  const int t = chunk2tensor[ch];
  return t >= 0 && t < n_tensors && active[t];
}

struct TtaChunks {
  const int* __restrict__ achunks; int n_achunks;
  const int* __restrict__ chunk2tensor; const unsigned char* __restrict__ active; int n_tensors;
  long nchunks;
  // for the calling thread of block j: i, its float4 of the slab, and ic, its float4 of the compact buffers -> live (uniform across the block)
  __device__ __forceinline__ bool at(int j, long& i, long& ic) const {
    const int ch = achunks[j];
    i = (long)ch * 256 + threadIdx.x;
    ic = (long)j * 256 + threadIdx.x;
    return tta_chunk_live(ch, nchunks, chunk2tensor, active, n_tensors);
  }
};

// grid = n_achunks: op(i, ic) on every live chunk
template <class Op>
__global__ __launch_bounds__(256) void tta_chunk_kernel(TtaChunks c, Op op) {
  long i, ic;
  if (c.at(blockIdx.x, i, ic)) op(i, ic);
}

// grid = n_achunks: partial[j] = the block's sum of the doubles op(i, ic), 0 for a dead chunk
template <class Op>
__global__ __launch_bounds__(256) void tta_chunk_sum_kernel(TtaChunks c, Op op, double* __restrict__ partial) {
  __shared__ double redd[16];
  const int j = blockIdx.x;
  long i, ic;
  if (!c.at(j, i, ic)) {  // uniform across the block
    if (threadIdx.x == 0) partial[j] = 0.0;
    return;
  }
  const double s = block_sum_d(op(i, ic), redd);
  if (threadIdx.x == 0) partial[j] = s;
}

// sum of partial[0:n] by one 256-thread block, in every thread, in a fixed order: whoever calls it gets the same bits
__device__ __forceinline__ double tta_partial_sum(const double* __restrict__ partial, int n, double* redd) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
  return block_sum_d(s, redd);
}

// what every slab entry point checks before it launches anything: `slabs` are walked by float4, `others` only have to be there
static inline int tta_slab_check(const char* name, const TtaChunks& c, long n, std::initializer_list<const void*> slabs,
                                 std::initializer_list<const void*> others = {}) {
  bool null = !c.achunks || !c.chunk2tensor || !c.active, misaligned = false;
  for (const void* p : slabs) {
    null |= !p;
    misaligned |= (uintptr_t)p % 16 != 0;
  }
  for (const void* p : others) null |= !p;
  STIL_REQUIRE(!null, "%s: null pointer", name);
  STIL_REQUIRE(n >= 0 && n % 1024 == 0 && c.n_achunks >= 0 && c.n_tensors >= 0, "%s: n=%ld must be a multiple of 1024, n_achunks=%d", name, n,
               c.n_achunks);
  STIL_REQUIRE(!misaligned, "%s: slabs must be 16-byte aligned", name);
  return STIL_OK;
}
