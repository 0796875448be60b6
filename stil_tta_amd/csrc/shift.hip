// The shifted test stream: image corruptions and tabular shifts as batch kernels.  C ABI: stil_shift.h.
// Every kernel is a pure function of (input, strength, seed, position in the stream): random numbers come from aug_hash
// (augment.hip) on 64-bit counters that are global to the stream, element i of a call draws at counter offset + i, so a stream cut
// into batches of any size yields the same samples bit for bit.  The 16-byte and the scalar path of a kernel are one template
// (V elements per thread), so which one a call takes never changes a bit of the result.  No allocation, no atomics, no sync.
#include "common.h"
#include "stil_shift.h"

// 24-bit uniform of counter `ctr`: r24 = hash >> 8; r24 * 2^-24 is exact in float32
__device__ __forceinline__ unsigned int shift_r24(unsigned long long seed, unsigned long long ctr) { return aug_hash(seed, ctr) >> 8; }
__device__ __forceinline__ float shift_u24(unsigned long long seed, unsigned long long ctr) { return (float)shift_r24(seed, ctr) * 0x1p-24f; }

// Box-Muller pair j: u1 in (0, 1] from counter 2j, u2 in [0, 1) from counter 2j + 1 -> (rho cos 2 pi u2, rho sin 2 pi u2).
// rho <= sqrt(48 ln 2) = 5.77: finite.  sincospif takes the angle in half turns, so 2 u2 is exact and no range reduction runs.
__device__ __forceinline__ void shift_gauss_pair(unsigned long long seed, unsigned long long j, float& gc, float& gs) {
  const float u1 = (float)(shift_r24(seed, 2ULL * j) + 1u) * 0x1p-24f;
  const float u2 = shift_u24(seed, 2ULL * j + 1ULL);
  const float rho = sqrtf(-2.f * logf(u1));
  float s, c;
  sincospif(2.f * u2, &s, &c);
  gc = rho * c;
  gs = rho * s;
}
// the normal of element e: the even member of pair e >> 1 takes the cosine, the odd one the sine
__device__ __forceinline__ float shift_gauss(unsigned long long seed, unsigned long long e) {
  float gc, gs;
  shift_gauss_pair(seed, e >> 1, gc, gs);
  return (e & 1ULL) ? gs : gc;
}
// clip that lets NaN through and is the identity on (-inf, inf)
__device__ __forceinline__ float shift_clip(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int V> struct ShiftVec;
template <> struct ShiftVec<1> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[1]) { v[0] = p[0]; }
  static __device__ __forceinline__ void store(float* p, const float (&v)[1]) { p[0] = v[0]; }
};
template <> struct ShiftVec<4> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// ---------------------------------------------------------------- Gaussian / impulse noise
// Thread t owns elements V t .. V t + V - 1; a pair of normals is drawn once and serves both its members when both are the
// thread's (always, for V = 4 and an even offset; an odd offset splits the thread's first and last pair with its neighbours).
template <int V>
__global__ __launch_bounds__(256) void shift_noise_kernel(const float* __restrict__ x, float* __restrict__ out, long groups, int kind,
                                                           float strength, float lo, float hi, unsigned long long seed,
                                                           unsigned long long offset) {
  const float half = 0.5f * strength;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
    float v[V];
    ShiftVec<V>::load(x + i * V, v);
    const unsigned long long e0 = offset + (unsigned long long)i * V;
    if (kind == 0) {
      unsigned long long have = ~0ULL;   // no pair index reaches 2^64 - 1
      float gc = 0.f, gs = 0.f;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const unsigned long long e = e0 + k, j = e >> 1;
        if (j != have) { shift_gauss_pair(seed, j, gc, gs); have = j; }
        v[k] = shift_clip(fmaf(strength, (e & 1ULL) ? gs : gc, v[k]), lo, hi);
      }
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float u = shift_u24(seed, e0 + k);
        v[k] = u < half ? lo : (u < strength ? hi : v[k]);
      }
    }
    ShiftVec<V>::store(out + i * V, v);
  }
}

// ---------------------------------------------------------------- contrast
// mean of every plane: one workgroup per plane, double accumulation in a fixed order, rounded once to float
__global__ __launch_bounds__(256) void shift_plane_mean_kernel(const float* __restrict__ x, float* __restrict__ mean, int HW) {
  __shared__ double red[16];
  const float* p = x + (long)blockIdx.x * HW;
  double s = 0.0;
  for (int i = threadIdx.x; i < HW; i += 256) s += (double)p[i];
  s = block_sum_d(s, red);
  if (threadIdx.x == 0) mean[blockIdx.x] = (float)(s / (double)HW);
}

template <int V>   // V = 4 only when HW % 4 == 0: a group never straddles two planes
__global__ __launch_bounds__(256) void shift_contrast_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                              float* __restrict__ out, long groups, int HW, float factor, float lo, float hi) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
    float v[V];
    ShiftVec<V>::load(x + i * V, v);
    const float m = mean[(i * V) / HW];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = shift_clip(fmaf(v[k] - m, factor, m), lo, hi);
    ShiftVec<V>::store(out + i * V, v);
  }
}

// ---------------------------------------------------------------- brightness: the V of HSV moved by delta, hue and saturation kept
template <int V>   // V = 4 only when HW % 4 == 0
__global__ __launch_bounds__(256) void shift_brightness_kernel(const float* __restrict__ x, float* __restrict__ out, long groups, int HW,
                                                                float delta, float lo, float hi) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
    const long pix0 = i * V, b = pix0 / HW;
    const long base = b * 3 * HW + (pix0 - b * HW);
    float r[V], g[V], bl[V];
    ShiftVec<V>::load(x + base, r);
    ShiftVec<V>::load(x + base + HW, g);
    ShiftVec<V>::load(x + base + 2L * HW, bl);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float val = fmaxf(r[k], fmaxf(g[k], bl[k]));
      const float nv = fminf(fmaxf(val, 0.f) + delta, hi);
      if (val > 0.f) {
        const float ratio = nv / val;
        r[k] = shift_clip(r[k] * ratio, lo, hi); g[k] = shift_clip(g[k] * ratio, lo, hi); bl[k] = shift_clip(bl[k] * ratio, lo, hi);
      } else {
        r[k] = g[k] = bl[k] = nv;
      }
    }
    ShiftVec<V>::store(out + base, r);
    ShiftVec<V>::store(out + base + HW, g);
    ShiftVec<V>::store(out + base + 2L * HW, bl);
  }
}

// ---------------------------------------------------------------- pixelate
// Pass 1: one thread per s x s block (cut from the top-left, smaller at the right and bottom edge) adds the block row-major in
// float32 and leaves the mean in the block's top-left pixel of `out`.  Pass 2: every other pixel copies its block's top-left
// pixel, which pass 2 never writes.
__global__ __launch_bounds__(256) void shift_pixelate_mean_kernel(const float* __restrict__ x, float* __restrict__ out, long blocks, int H, int W,
                                                                   int s, int nbh, int nbw) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < blocks; i += (long)gridDim.x * 256) {
    const long plane = i / ((long)nbh * nbw);
    const int r = (int)(i - plane * nbh * nbw), by = r / nbw, bx = r - by * nbw;
    const int y0 = by * s, x0 = bx * s, bh = min(s, H - y0), bw = min(s, W - x0);
    const float* p = x + plane * H * W + (long)y0 * W + x0;
    float sum = 0.f;
    for (int yy = 0; yy < bh; ++yy)
      for (int xx = 0; xx < bw; ++xx) {
        const float t = p[(long)yy * W + xx];
        sum = (yy | xx) ? sum + t : t;
      }
    out[plane * H * W + (long)y0 * W + x0] = sum / (float)(bh * bw);
  }
}

__global__ __launch_bounds__(256) void shift_pixelate_fill_kernel(float* out, long n, int H, int W, int s) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long plane = i / ((long)H * W);
    const int r = (int)(i - plane * H * W), y = r / W, xq = r - y * W;
    const int y0 = (y / s) * s, x0 = (xq / s) * s;
    if (y != y0 || xq != x0) out[i] = out[plane * H * W + (long)y0 * W + x0];
  }
}

// ---------------------------------------------------------------- tabular shifts
__global__ __launch_bounds__(256) void shift_tab_kernel(const float* __restrict__ x, float* __restrict__ out, long n, int n_cols, int num_cat,
                                                         const int* __restrict__ cat_len, const unsigned char* __restrict__ col_on,
                                                         const float* __restrict__ col_std, const float* __restrict__ col_fill, int kind,
                                                         float strength, unsigned long long seed, unsigned long long offset) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int c = (int)(i % n_cols);
    const unsigned long long e = offset + (unsigned long long)i;
    float v = x[i];
    if (col_on[c]) {
      if (kind == 0) {
        if (c >= num_cat) v = fmaf(strength * col_std[c], shift_gauss(seed, e), v);
      } else if (kind == 1) {
        if (shift_u24(seed, e) < strength) v = col_fill[c];
      } else if (c < num_cat) {
        if (shift_u24(seed, 2ULL * e) < strength)
          v = (float)(unsigned int)(((unsigned long long)shift_r24(seed, 2ULL * e + 1ULL) * (unsigned long long)(unsigned int)cat_len[c]) >> 24);
      }
    }
    out[i] = v;
  }
}

// ---------------------------------------------------------------- C ABI
static inline bool shift_overlap(const float* x, const float* out, long n) {
  const uintptr_t a = (uintptr_t)x, b = (uintptr_t)out, len = (uintptr_t)n * sizeof(float);
  return a < b + len && b < a + len;
}
static inline bool shift_vec_ok(const float* x, const float* out) { return (((uintptr_t)x | (uintptr_t)out) % 16) == 0; }

extern "C" int stil_shift_noise(const float* x, float* out, long n, int kind, float strength, float lo, float hi, unsigned long long seed,
                                unsigned long long offset, void* stream) {
  STIL_REQUIRE(x && out && n > 0, "stil_shift_noise: null pointer or empty shape");
  STIL_REQUIRE(!shift_overlap(x, out, n), "stil_shift_noise: out overlaps x (in place is not supported)");
  STIL_REQUIRE(kind == 0 || kind == 1, "stil_shift_noise: kind=%d is neither 0 (Gaussian) nor 1 (impulse)", kind);
  STIL_REQUIRE(strength >= 0.f && strength <= 3.0e38f && (kind == 0 || strength <= 1.f), "stil_shift_noise: strength=%g outside %s", (double)strength,
               kind == 0 ? "[0, inf)" : "[0, 1]");
  STIL_REQUIRE(lo <= hi, "stil_shift_noise: clip range [%g, %g] is empty or NaN", (double)lo, (double)hi);
  if (n % 4 == 0 && shift_vec_ok(x, out))
    hipLaunchKernelGGL(shift_noise_kernel<4>, dim3(ew_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, x, out, n / 4, kind, strength, lo, hi, seed, offset);
  else
    hipLaunchKernelGGL(shift_noise_kernel<1>, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, x, out, n, kind, strength, lo, hi, seed, offset);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_shift_contrast(const float* x, float* out, int B, int C, int HW, float factor, float lo, float hi, float* mean_ws,
                                   void* stream) {
  STIL_REQUIRE(x && out && mean_ws && B > 0 && C > 0 && HW > 0, "stil_shift_contrast: null pointer or empty shape");
  const long planes = (long)B * C, n = planes * HW;
  STIL_REQUIRE(planes <= 0x7fffffffL, "stil_shift_contrast: B * C = %ld planes exceed the grid", planes);
  STIL_REQUIRE(!shift_overlap(x, out, n), "stil_shift_contrast: out overlaps x (in place is not supported)");
  STIL_REQUIRE(factor >= 0.f && factor <= 3.0e38f, "stil_shift_contrast: factor=%g is not finite and non-negative", (double)factor);
  STIL_REQUIRE(lo <= hi, "stil_shift_contrast: clip range [%g, %g] is empty or NaN", (double)lo, (double)hi);
  hipLaunchKernelGGL(shift_plane_mean_kernel, dim3((unsigned)planes), dim3(256), 0, (hipStream_t)stream, x, mean_ws, HW);
  STIL_LAUNCH_CHECK();
  if (HW % 4 == 0 && shift_vec_ok(x, out))
    hipLaunchKernelGGL(shift_contrast_kernel<4>, dim3(ew_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, x, (const float*)mean_ws, out, n / 4, HW,
                       factor, lo, hi);
  else
    hipLaunchKernelGGL(shift_contrast_kernel<1>, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, x, (const float*)mean_ws, out, n, HW, factor,
                       lo, hi);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_shift_brightness(const float* x, float* out, int B, int C, int HW, float delta, float lo, float hi, void* stream) {
  STIL_REQUIRE(x && out && B > 0 && HW > 0, "stil_shift_brightness: null pointer or empty shape");
  STIL_REQUIRE(C == 3, "stil_shift_brightness: C=%d, the HSV value shift takes 3 channels", C);
  const long pixels = (long)B * HW;
  STIL_REQUIRE(!shift_overlap(x, out, 3 * pixels), "stil_shift_brightness: out overlaps x (in place is not supported)");
  STIL_REQUIRE(delta >= -3.0e38f && delta <= 3.0e38f, "stil_shift_brightness: delta=%g is not finite", (double)delta);
  STIL_REQUIRE(lo <= hi, "stil_shift_brightness: clip range [%g, %g] is empty or NaN", (double)lo, (double)hi);
  if (HW % 4 == 0 && shift_vec_ok(x, out))
    hipLaunchKernelGGL(shift_brightness_kernel<4>, dim3(ew_grid(pixels / 4)), dim3(256), 0, (hipStream_t)stream, x, out, pixels / 4, HW, delta, lo, hi);
  else
    hipLaunchKernelGGL(shift_brightness_kernel<1>, dim3(ew_grid(pixels)), dim3(256), 0, (hipStream_t)stream, x, out, pixels, HW, delta, lo, hi);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_shift_pixelate(const float* x, float* out, int B, int C, int H, int W, int s, void* stream) {
  STIL_REQUIRE(x && out && B > 0 && C > 0 && H > 0 && W > 0, "stil_shift_pixelate: null pointer or empty shape");
  STIL_REQUIRE(s >= 1, "stil_shift_pixelate: block size s=%d must be at least 1", s);
  const long planes = (long)B * C, n = planes * H * W;
  STIL_REQUIRE(!shift_overlap(x, out, n), "stil_shift_pixelate: out overlaps x (in place is not supported)");
  const int se = s < (H > W ? H : W) ? s : (H > W ? H : W);   // s >= the image: one block per plane
  const int nbh = cdiv(H, se), nbw = cdiv(W, se);
  const long blocks = planes * nbh * nbw;
  hipLaunchKernelGGL(shift_pixelate_mean_kernel, dim3(ew_grid(blocks)), dim3(256), 0, (hipStream_t)stream, x, out, blocks, H, W, se, nbh, nbw);
  STIL_LAUNCH_CHECK();
  if (se > 1) {
    hipLaunchKernelGGL(shift_pixelate_fill_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, out, n, H, W, se);
    STIL_LAUNCH_CHECK();
  }
  return STIL_OK;
}

extern "C" int stil_shift_tab(const float* x, float* out, int B, int n_cols, int num_cat, const int* cat_len, const unsigned char* col_on,
                              const float* col_std, const float* col_fill, int kind, float strength, unsigned long long seed,
                              unsigned long long offset, void* stream) {
  STIL_REQUIRE(x && out && col_on && col_std && col_fill && B > 0 && n_cols > 0, "stil_shift_tab: null pointer or empty shape");
  STIL_REQUIRE(num_cat >= 0 && num_cat <= n_cols && (num_cat == 0 || cat_len), "stil_shift_tab: num_cat=%d outside [0, %d] or cat_len missing",
               num_cat, n_cols);
  const long n = (long)B * n_cols;
  STIL_REQUIRE(!shift_overlap(x, out, n), "stil_shift_tab: out overlaps x (in place is not supported)");
  STIL_REQUIRE(kind >= 0 && kind <= 2, "stil_shift_tab: kind=%d is none of 0 (noise), 1 (missing), 2 (categorical flip)", kind);
  STIL_REQUIRE(strength >= 0.f && strength <= 3.0e38f && (kind == 0 || strength <= 1.f), "stil_shift_tab: strength=%g outside %s", (double)strength,
               kind == 0 ? "[0, inf)" : "[0, 1]");
  hipLaunchKernelGGL(shift_tab_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, x, out, n, n_cols, num_cat, cat_len, col_on, col_std,
                     col_fill, kind, strength, seed, offset);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
