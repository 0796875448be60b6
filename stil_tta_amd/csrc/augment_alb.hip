// Albumentations branch of the input pipeline (utils/utils.py:46-256 with augmentation_speedup=True, the branch every
// shipped config selects): albumentations 1.3.1 / OpenCV 4.x transforms on HWC images with 3 channels, uint8 (DVM .npy)
// or float32 in [0, 1] (cardiac .npy), as batch kernels.  Same rules as augment.hip: random draws are ARGUMENTS (the host
// draws them, tests inject them), one launch per batch and op, and a sample whose op is off is copied bit for bit.
// Every stage returns the source type (uint8 stages round, as each albumentations stage does); the last stage writes the
// float CHW tensor (convert_to_ts: float32(v / 255.0); convert_to_ts_01: a copy).  The pixel definitions are restated in
// numpy in tests/alb_restate.py; the device matches them bit for bit.
// Arithmetic is written without FP contraction (ALB_EXACT) so that every float / double result equals numpy's.
#include "common.h"
#include <algorithm>
#include <cfloat>

#define ALB_EXACT _Pragma("clang fp contract(off)")
#define ALB_MAX_WG 64     // partial grey sums per image (stil_alb_color's workspace is [B, ALB_MAX_WG] doubles)
#define ALB_MAX_K 31      // largest Gaussian kernel (the reference uses 29 and 19)

__device__ __forceinline__ float alb_sat_u8(float v) { return fminf(fmaxf(rintf(v), 0.f), 255.f); }   // saturate_cast<uchar>
__device__ __forceinline__ float alb_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// ---------------------------------------------------------------- loads / stores of whole RGB pixels
// 4 consecutive pixels per lane: 12 bytes (three dword loads) for uint8, 48 bytes (three 16-byte loads) for float32 when
// the image holds a multiple of 4 pixels and the pointers are aligned (`vec`, decided on the host); otherwise per pixel.
__device__ __forceinline__ void alb_load4(const unsigned char* img, long g, long npix, bool vec, float (&v)[4][3]) {
  if (vec) {
    const unsigned int* q = reinterpret_cast<const unsigned int*>(img + 12 * g);
    const unsigned int w[3] = {q[0], q[1], q[2]};
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i / 3][i % 3] = (float)((w[i / 4] >> (8 * (i % 4))) & 0xffu);
    return;
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const long px = 4 * g + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[p][c] = px < npix ? (float)img[px * 3 + c] : 0.f;
  }
}
__device__ __forceinline__ void alb_load4(const float* img, long g, long npix, bool vec, float (&v)[4][3]) {
  if (vec) {
    const float4* q = reinterpret_cast<const float4*>(img + 12 * g);
    const float4 a = q[0], b = q[1], c = q[2];
    const float w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i / 3][i % 3] = w[i];
    return;
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const long px = 4 * g + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[p][c] = px < npix ? img[px * 3 + c] : 0.f;
  }
}
// values are already in range (uint8: integers 0..255)
__device__ __forceinline__ void alb_store4(unsigned char* img, long g, long npix, bool vec, const float (&v)[4][3]) {
  if (vec) {
    unsigned int w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 12; ++i) w[i / 4] |= ((unsigned int)v[i / 3][i % 3]) << (8 * (i % 4));
    unsigned int* q = reinterpret_cast<unsigned int*>(img + 12 * g);
    q[0] = w[0]; q[1] = w[1]; q[2] = w[2];
    return;
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const long px = 4 * g + p;
    if (px < npix)
#pragma unroll
      for (int c = 0; c < 3; ++c) img[px * 3 + c] = (unsigned char)v[p][c];
  }
}
__device__ __forceinline__ void alb_store4(float* img, long g, long npix, bool vec, const float (&v)[4][3]) {
  if (vec) {
    float4* q = reinterpret_cast<float4*>(img + 12 * g);
    q[0] = make_float4(v[0][0], v[0][1], v[0][2], v[1][0]);
    q[1] = make_float4(v[1][1], v[1][2], v[2][0], v[2][1]);
    q[2] = make_float4(v[2][2], v[3][0], v[3][1], v[3][2]);
    return;
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const long px = 4 * g + p;
    if (px < npix)
#pragma unroll
      for (int c = 0; c < 3; ++c) img[px * 3 + c] = v[p][c];
  }
}
template <typename T> __device__ __forceinline__ void alb_load1(const T* img, long px, float (&v)[3]) {
  v[0] = (float)img[px * 3]; v[1] = (float)img[px * 3 + 1]; v[2] = (float)img[px * 3 + 2];
}
__device__ __forceinline__ void alb_store1(unsigned char* img, long px, const float (&v)[3]) {
  img[px * 3] = (unsigned char)alb_sat_u8(v[0]); img[px * 3 + 1] = (unsigned char)alb_sat_u8(v[1]); img[px * 3 + 2] = (unsigned char)alb_sat_u8(v[2]);
}
__device__ __forceinline__ void alb_store1(float* img, long px, const float (&v)[3]) {
  img[px * 3] = v[0]; img[px * 3 + 1] = v[1]; img[px * 3 + 2] = v[2];
}

// ---------------------------------------------------------------- colour: ColorJitter (+ ToGray)
// cv2.cvtColor(RGB2GRAY): uint8 in fixed point (coefficients 0.299 / 0.587 / 0.114 scaled by 2^14), float32 as written
__device__ __forceinline__ float alb_gray(const float (&v)[3], bool u8) {
  ALB_EXACT;
  if (u8) return (float)(((int)v[0] * 4899 + (int)v[1] * 9617 + (int)v[2] * 1868 + 8192) >> 14);
  return v[0] * 0.299f + v[1] * 0.587f + v[2] * 0.114f;
}

// HSV -> RGB of cv2 (HSV2RGB_f core): h in units where 6 / hscale is a full turn, s and v in [0, 1]
__device__ __forceinline__ void alb_hsv2rgb(float h, float s, float v, float hscale, float (&rgb)[3]) {
  ALB_EXACT;
  if (s == 0.f) { rgb[0] = rgb[1] = rgb[2] = v; return; }
  h = h * hscale;
  while (h < 0.f) h += 6.f;
  while (h >= 6.f) h -= 6.f;
  int sector = (int)floorf(h);
  h = h - (float)sector;
  if (sector < 0 || sector >= 6) { sector = 0; h = 0.f; }
  const float tab[4] = {v, v * (1.f - s), v * (1.f - s * h), v * (1.f - s * (1.f - h))};
  const int sd[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};   // (b, g, r) per sector
  rgb[2] = tab[sd[sector][0]]; rgb[1] = tab[sd[sector][1]]; rgb[0] = tab[sd[sector][2]];
}

struct AlbLuts {        // per-image tables in LDS
  unsigned char bri[256], con[256], hue[256];
  int sdiv[256], hdiv[256];   // cv2's 8-bit RGB2HSV division tables: round((255 << 12) / v), round((180 << 12) / (6 diff))
};

struct AlbColorArgs {
  const void* src; void* dst; int H, W;
  const int* order; const double* fac; const unsigned char* cj_on; const unsigned char* gray_on;
  double* gpart; int nblk; int vec;
};

// one ColorJitter op (0 brightness, 1 contrast, 2 saturation, 3 hue) on one pixel; uint8 values are integers 0..255
__device__ __forceinline__ void alb_cj_op(int op, float (&v)[3], bool u8, const AlbLuts& L, const float (&fp)[6]) {
  ALB_EXACT;
  if (op == 0) {          // adjust_brightness_torchvision
    if (u8) { for (int c = 0; c < 3; ++c) v[c] = (float)L.bri[(int)v[c]]; }
    else { for (int c = 0; c < 3; ++c) v[c] = alb_clamp01(v[c] * fp[0]); }
  } else if (op == 1) {   // adjust_contrast_torchvision (fp[1] = factor, fp[5] = mean * (1 - factor))
    if (u8) { for (int c = 0; c < 3; ++c) v[c] = (float)L.con[(int)v[c]]; }
    else if (fp[1] == 0.f) { v[0] = v[1] = v[2] = fp[5]; }
    else { for (int c = 0; c < 3; ++c) v[c] = alb_clamp01(v[c] * fp[1] + fp[5]); }
  } else if (op == 2) {   // adjust_saturation_torchvision: cv2.addWeighted(img, f, gray3, 1 - f, 0)
    const float g = alb_gray(v, u8);
    for (int c = 0; c < 3; ++c) {
      const float t = v[c] * fp[2] + g * fp[4];
      v[c] = u8 ? alb_sat_u8(t) : alb_clamp01(t);
    }
  } else {                // adjust_hue_torchvision
    if (u8) {             // cv2 8-bit RGB2HSV (H in [0, 180)), LUT on H, HSV2RGB through float
      const int r = (int)v[0], g = (int)v[1], b = (int)v[2];
      const int vmax = max(r, max(g, b)), vmin = min(r, min(g, b)), diff = vmax - vmin;
      const int vr = vmax == r ? -1 : 0, vg = vmax == g ? -1 : 0;
      const int s = (diff * L.sdiv[vmax] + (1 << 11)) >> 12;
      int h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
      h = (h * L.hdiv[diff] + (1 << 11)) >> 12;
      h += h < 0 ? 180 : 0;
      float rgb[3];
      alb_hsv2rgb((float)L.hue[h], (float)s * (1.f / 255.f), (float)vmax * (1.f / 255.f), 6.f / 180.f, rgb);
      for (int c = 0; c < 3; ++c) v[c] = alb_sat_u8(rgb[c] * 255.f);
    } else {              // cv2 float RGB2HSV (H in degrees), H = mod(H + 360 f, 360), HSV2RGB
      const float r = v[0], g = v[1], b = v[2];
      const float vmax = fmaxf(r, fmaxf(g, b)), vmin = fminf(r, fminf(g, b));
      float diff = vmax - vmin;
      const float s = diff / (fabsf(vmax) + FLT_EPSILON);
      diff = (float)(60.0 / (double)(diff + FLT_EPSILON));
      float h = vmax == r ? (g - b) * diff : (vmax == g ? (b - r) * diff + 120.f : (r - g) * diff + 240.f);
      if (h < 0.f) h += 360.f;
      h = h + fp[3];
      h = fmodf(h, 360.f);
      if (h < 0.f) h += 360.f;
      alb_hsv2rgb(h, s, vmax, 6.f / 360.f, v);
    }
  }
}

__device__ __forceinline__ bool alb_identity(int op, double f) { return op == 3 ? f == 0.0 : f == 1.0; }

// Tables of one image, built exactly as albumentations builds them in numpy (np.arange(256) * f in double, clip, astype).
__device__ void alb_build_luts(AlbLuts& L, const double* f, double mean, bool hue_on) {
  ALB_EXACT;
  const int i = threadIdx.x;   // blockDim == 256
  const double x = (double)i;
  L.bri[i] = (unsigned char)(int)fmin(fmax(x * f[0], 0.0), 255.0);
  L.con[i] = f[1] == 0.0 ? (unsigned char)(int)(mean + 0.5) : (unsigned char)(int)fmin(fmax(x * f[1] + mean * (1.0 - f[1]), 0.0), 255.0);
  if (hue_on) {
    // int16 arange + a Python float is float32 under numpy 1.23's value-based casting (the reference's pin)
    float h = fmodf((float)i + (float)(180.0 * f[3]), 180.f);
    if (h < 0.f) h += 180.f;
    L.hue[i] = (unsigned char)(int)h;
    L.sdiv[i] = i ? (int)rint((double)(255 << 12) / (1.0 * i)) : 0;
    L.hdiv[i] = i ? (int)rint((double)(180 << 12) / (6.0 * i)) : 0;
  }
}

// float per-pixel factors: fp = (f_b, f_c, f_s, 360 f_h, 1 - f_s, mean (1 - f_c)) rounded to float32 (numpy's scalar casting)
__device__ __forceinline__ void alb_float_params(const double* f, double mean, float (&fp)[6]) {
  ALB_EXACT;
  fp[0] = (float)f[0]; fp[1] = (float)f[1]; fp[2] = (float)f[2];
  fp[3] = (float)(f[3] * 360.0); fp[4] = (float)(1.0 - f[2]);
  fp[5] = f[1] == 0.0 ? (float)mean : (float)(mean * (1.0 - f[1]));
}

// pass 1: the ops that precede contrast in the sample's order, then the grey sum of the result (what the contrast op
// takes the mean of).  uint8: an integer sum (exact, independent of how pixels are split over workgroups).
template <typename T>
__global__ __launch_bounds__(256) void alb_color_mean_kernel(AlbColorArgs a) {
  ALB_EXACT;
  __shared__ AlbLuts L;
  __shared__ double red[4];
  constexpr bool u8 = sizeof(T) == 1;
  const int b = blockIdx.y;
  const double* f = a.fac + 4 * b;
  if (!a.cj_on[b] || f[1] == 1.0) return;   // pass 2 reads the partials only where contrast is applied
  const int* ord = a.order + 4 * b;
  int npre = 0;
  while (npre < 4 && ord[npre] != 1) ++npre;
  bool hue_pre = false;
  for (int k = 0; k < npre; ++k) hue_pre |= ord[k] == 3 && f[3] != 0.0;
  alb_build_luts(L, f, 0.0, hue_pre);
  float fp[6];
  alb_float_params(f, 0.0, fp);
  __syncthreads();
  const long npix = (long)a.H * a.W, ng = (npix + 3) / 4;
  const T* img = (const T*)a.src + (long)b * npix * 3;
  unsigned long long isum = 0;
  double fsum = 0.0;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < ng; g += (long)a.nblk * 256) {
    float v[4][3];
    alb_load4(img, g, npix, a.vec, v);
    for (int p = 0; p < 4; ++p) {
      if (4 * g + p >= npix) break;
      for (int k = 0; k < npre; ++k)
        if (!alb_identity(ord[k], f[ord[k]])) alb_cj_op(ord[k], v[p], u8, L, fp);
      const float gr = alb_gray(v[p], u8);
      if (u8) isum += (unsigned long long)gr; else fsum += (double)gr;
    }
  }
  double s = u8 ? (double)isum : fsum;   // uint8: exact below 2^53
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) a.gpart[(long)b * ALB_MAX_WG + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// pass 2: the whole chain (ColorJitter in the sample's order, then ToGray), src -> dst (may alias)
template <typename T>
__global__ __launch_bounds__(256) void alb_color_apply_kernel(AlbColorArgs a) {
  ALB_EXACT;
  __shared__ AlbLuts L;
  constexpr bool u8 = sizeof(T) == 1;
  const int b = blockIdx.y;
  const double* f = a.fac + 4 * b;
  const bool cj = a.cj_on[b] != 0, gr = a.gray_on[b] != 0;
  const long npix = (long)a.H * a.W, ng = (npix + 3) / 4;
  const T* src = (const T*)a.src + (long)b * npix * 3;
  T* dst = (T*)a.dst + (long)b * npix * 3;
  if (!cj && !gr) {
    if (src == dst) return;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < ng; g += (long)a.nblk * 256) {
      float v[4][3];
      alb_load4(src, g, npix, a.vec, v);
      alb_store4(dst, g, npix, a.vec, v);
    }
    return;
  }
  double mean = 0.0;
  if (cj && f[1] != 1.0) {   // fixed-order sum of the partials: every workgroup of the image gets the same mean
    double s = 0.0;
    for (int i = 0; i < a.nblk; ++i) s += a.gpart[(long)b * ALB_MAX_WG + i];
    mean = s / (double)npix;
  }
  const int* ord = a.order + 4 * b;
  int ops[4], nops = 0;
  bool hue_on = false;
  if (cj)
    for (int k = 0; k < 4; ++k)
      if (!alb_identity(ord[k], f[ord[k]])) { ops[nops++] = ord[k]; hue_on |= ord[k] == 3; }
  alb_build_luts(L, f, mean, hue_on);
  float fp[6];
  alb_float_params(f, mean, fp);
  __syncthreads();
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < ng; g += (long)a.nblk * 256) {
    float v[4][3];
    alb_load4(src, g, npix, a.vec, v);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      for (int k = 0; k < nops; ++k) alb_cj_op(ops[k], v[p], u8, L, fp);
      if (gr) { const float gv = alb_gray(v[p], u8); v[p][0] = v[p][1] = v[p][2] = gv; }
    }
    alb_store4(dst, g, npix, a.vec, v);
  }
}

// ---------------------------------------------------------------- Gaussian blur: cv2.GaussianBlur(img, (k, k), sigma)
// Weights exp(-0.5 / sigma^2 * x^2), x = i - (k-1)/2, normalised in double, rounded to float; border reflect-101.
// Separable in one launch: a 16 x 32 output tile stages its source rows (with the halo) as float in LDS, the row pass
// writes a float intermediate to LDS, the column pass reads it; uint8 rounds once at the end.  sigma[b] <= 0 copies.
#define ALB_BTX 32
#define ALB_BTY 16
template <typename T>
__global__ __launch_bounds__(256) void alb_blur_kernel(const T* __restrict__ src, T* __restrict__ dst, const double* __restrict__ sigma,
                                                        int H, int W, int ksize) {
  ALB_EXACT;
  __shared__ float stage[(ALB_BTY + ALB_MAX_K - 1) * (ALB_BTX + ALB_MAX_K - 1) * 3];
  __shared__ float mid[(ALB_BTY + ALB_MAX_K - 1) * ALB_BTX * 3];
  __shared__ double tw[ALB_MAX_K];
  __shared__ float w[ALB_MAX_K];
  const int b = blockIdx.z, x0 = blockIdx.x * ALB_BTX, y0 = blockIdx.y * ALB_BTY, half = ksize >> 1;
  const long npix = (long)H * W;
  const T* img = src + (long)b * npix * 3;
  T* out = dst + (long)b * npix * 3;
  const double sg = sigma[b];
  if (!(sg > 0.0)) {
    for (int i = threadIdx.x; i < ALB_BTX * ALB_BTY; i += 256) {
      const int y = y0 + i / ALB_BTX, x = x0 + i % ALB_BTX;
      if (y < H && x < W)
        for (int c = 0; c < 3; ++c) out[((long)y * W + x) * 3 + c] = img[((long)y * W + x) * 3 + c];
    }
    return;
  }
  if (threadIdx.x < ksize) {
    const double xx = (double)threadIdx.x - (double)(ksize - 1) * 0.5;
    tw[threadIdx.x] = exp(-0.5 / (sg * sg) * xx * xx);
  }
  __syncthreads();
  if (threadIdx.x < ksize) {
    double s = 0.0;
    for (int t = 0; t < ksize; ++t) s += tw[t];
    w[threadIdx.x] = (float)(tw[threadIdx.x] * (1.0 / s));
  }
  const int rows = min(ALB_BTY, H - y0) + 2 * half, cols = min(ALB_BTX, W - x0), scols = cols + 2 * half;
  for (int i = threadIdx.x; i < rows * scols; i += 256) {   // source rows y0-half .. and columns x0-half .., reflected
    const int r = i / scols, c = i - r * scols;
    const long px = (long)reflect101(y0 - half + r, H) * W + reflect101(x0 - half + c, W);
    for (int ch = 0; ch < 3; ++ch) stage[i * 3 + ch] = (float)img[px * 3 + ch];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rows * cols; i += 256) {    // row pass
    const int r = i / cols, c = i - r * cols;
    const float* s = stage + (r * scols + c) * 3;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int t = 0; t < ksize; ++t)
      for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + w[t] * s[t * 3 + ch];
    for (int ch = 0; ch < 3; ++ch) mid[i * 3 + ch] = acc[ch];
  }
  __syncthreads();
  const int orows = min(ALB_BTY, H - y0);
  for (int i = threadIdx.x; i < orows * cols; i += 256) {   // column pass
    const int r = i / cols, c = i - r * cols;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int t = 0; t < ksize; ++t)
      for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + w[t] * mid[((r + t) * cols + c) * 3 + ch];
    alb_store1(out, (long)(y0 + r) * W + x0 + c, acc);
  }
}

// ---------------------------------------------------------------- crop + resize (cv2 INTER_LINEAR) + flip
// box[b] = (top, left, h, w) (RandomResizedCrop; the whole image for A.Resize); output pixel dx samples
// fx = float((dx + 0.5) * (1 / (P / w)) - 0.5), floor, fraction; an index below 0 or at / past the last pixel clamps to the
// edge with weight 0.  flip[b] mirrors the output (HorizontalFlip after the crop).  out_chw: the final float [B,3,P,P]
// (uint8: float32(v / 255.0) of the rounded uint8 value); else dst: HWC of the source type.
__device__ __forceinline__ void alb_lin_coord(int d, int n, int P, int& i0, int& i1, float& fr) {
  ALB_EXACT;
  const double scale = 1.0 / ((double)P / (double)n);
  float fx = (float)(((double)d + 0.5) * scale - 0.5);
  int sx = (int)floorf(fx);
  fx = fx - (float)sx;
  if (sx < 0) { fx = 0.f; sx = 0; }
  if (sx >= n - 1) { fx = 0.f; sx = n - 1; }
  i0 = sx; i1 = min(sx + 1, n - 1); fr = fx;
}

template <typename T>
__global__ __launch_bounds__(256) void alb_resize_kernel(const T* __restrict__ src, T* __restrict__ dst, float* __restrict__ out_chw,
                                                          const int* __restrict__ box, const unsigned char* __restrict__ flip,
                                                          int H, int W, int P) {
  ALB_EXACT;
  constexpr bool u8 = sizeof(T) == 1;
  const int b = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= P * P) return;
  const int oy = pix / P, ox = pix - oy * P;
  // clamped to the image (the host checks boxes; a bad device-side box changes the picture, never reads outside it)
  const int top = min(max(box[b * 4 + 0], 0), H - 1), left = min(max(box[b * 4 + 1], 0), W - 1);
  const int ch = min(max(box[b * 4 + 2], 1), H - top), cw = min(max(box[b * 4 + 3], 1), W - left);
  const int sx_o = (flip && flip[b]) ? P - 1 - ox : ox;
  int y0, y1, x0, x1;
  float fy, fx;
  alb_lin_coord(oy, ch, P, y0, y1, fy);
  alb_lin_coord(sx_o, cw, P, x0, x1, fx);
  const T* img = src + (long)b * H * W * 3;
  float a[3], bb[3], c[3], d[3], v[3];
  alb_load1(img, (long)(top + y0) * W + left + x0, a); alb_load1(img, (long)(top + y0) * W + left + x1, bb);
  alb_load1(img, (long)(top + y1) * W + left + x0, c); alb_load1(img, (long)(top + y1) * W + left + x1, d);
  const float gx = 1.f - fx, gy = 1.f - fy;
  for (int k = 0; k < 3; ++k) {
    v[k] = (a[k] * gx + bb[k] * fx) * gy + (c[k] * gx + d[k] * fx) * fy;
    if (u8) v[k] = alb_sat_u8(v[k]);
  }
  if (out_chw) {
    const long plane = (long)P * P;
    float* o = out_chw + (long)b * 3 * plane + pix;
    for (int k = 0; k < 3; ++k) o[k * plane] = u8 ? (float)((double)v[k] / 255.0) : v[k];
  } else {
    alb_store1(dst + (long)b * P * P * 3, pix, v);
  }
}

// ---------------------------------------------------------------- rotation: A.Rotate = cv2.warpAffine, bilinear, reflect-101
// minv[b]: the inverse affine map warpAffine uses (getRotationMatrix2D((W/2-0.5, H/2-0.5), angle, 1) inverted, built on the
// host).  The source position is quantised to 1/32 pixel as cv2 does (AB_BITS = 10, INTER_BITS = 5); each of the 4 taps is
// reflected on its own; weights (1-ax)(1-ay) ... are exact multiples of 1/1024.  flip_first[b]: a HorizontalFlip applied to
// the image before the rotation.  on[b] == 0: a copy (flipped if flip_first[b]).
template <typename T>
__global__ __launch_bounds__(256) void alb_rotate_kernel(const T* __restrict__ src, T* __restrict__ dst, const double* __restrict__ minv,
                                                          const unsigned char* __restrict__ on, const unsigned char* __restrict__ flip_first,
                                                          int H, int W) {
  ALB_EXACT;
  const int b = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= H * W) return;
  const int y = pix / W, x = pix - y * W;
  const bool fl = flip_first && flip_first[b];
  const T* img = src + (long)b * H * W * 3;
  T* out = dst + (long)b * H * W * 3;
  float v[3];
  if (!on[b]) {
    alb_load1(img, (long)y * W + (fl ? W - 1 - x : x), v);
    alb_store1(out, pix, v);
    return;
  }
  const double* M = minv + 6 * b;
  const int adelta = (int)rint(M[0] * (double)x * 1024.0), bdelta = (int)rint(M[3] * (double)x * 1024.0);
  const int X0 = (int)rint((M[1] * (double)y + M[2]) * 1024.0) + 16, Y0 = (int)rint((M[4] * (double)y + M[5]) * 1024.0) + 16;
  const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
  const int sx = X >> 5, sy = Y >> 5;
  const float ax = (float)(X & 31) * (1.f / 32.f), ay = (float)(Y & 31) * (1.f / 32.f);
  int xs[2] = {reflect101(sx, W), reflect101(sx + 1, W)};
  const int ys[2] = {reflect101(sy, H), reflect101(sy + 1, H)};
  if (fl) { xs[0] = W - 1 - xs[0]; xs[1] = W - 1 - xs[1]; }
  float a[3], bb[3], c[3], d[3];
  alb_load1(img, (long)ys[0] * W + xs[0], a); alb_load1(img, (long)ys[0] * W + xs[1], bb);
  alb_load1(img, (long)ys[1] * W + xs[0], c); alb_load1(img, (long)ys[1] * W + xs[1], d);
  const float w00 = (1.f - ay) * (1.f - ax), w01 = (1.f - ay) * ax, w10 = ay * (1.f - ax), w11 = ay * ax;
  for (int k = 0; k < 3; ++k) v[k] = a[k] * w00 + bb[k] * w01 + c[k] * w10 + d[k] * w11;
  alb_store1(out, pix, v);
}

// ---------------------------------------------------------------- HWC -> float CHW (convert_to_ts / convert_to_ts_01)
template <typename T>
__global__ __launch_bounds__(256) void alb_to_tensor_kernel(const T* __restrict__ src, float* __restrict__ out, int H, int W, int vec) {
  ALB_EXACT;
  constexpr bool u8 = sizeof(T) == 1;
  const int b = blockIdx.y;
  const long npix = (long)H * W, ng = (npix + 3) / 4;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= ng) return;
  float v[4][3];
  alb_load4(src + (long)b * npix * 3, g, npix, vec, v);
  float* o = out + (long)b * 3 * npix;
  for (int c = 0; c < 3; ++c) {
    float t[4];
    for (int p = 0; p < 4; ++p) t[p] = u8 ? (float)((double)v[p][c] / 255.0) : v[p][c];
    if (vec) {
      *reinterpret_cast<float4*>(o + c * npix + 4 * g) = make_float4(t[0], t[1], t[2], t[3]);
    } else {
      for (int p = 0; p < 4; ++p)
        if (4 * g + p < npix) o[c * npix + 4 * g + p] = t[p];
    }
  }
}

// ---------------------------------------------------------------- C ABI
#define ALB_ONE_IMAGE(fn, a, b) STIL_REQUIRE(((a) != nullptr) != ((b) != nullptr), fn ": exactly one of the uint8 / float32 image pointers (null image pointer)")
static bool alb_aligned(const void* p, int a) { return ((uintptr_t)p % a) == 0; }

extern "C" int stil_alb_color(const unsigned char* src_u8, const float* src_f32, unsigned char* dst_u8, float* dst_f32, int B, int H, int W,
                              const int* order, const double* factors, const unsigned char* cj_on, const unsigned char* gray_on,
                              double* gpart, int wg_per_image, void* stream) {
  ALB_ONE_IMAGE("stil_alb_color", src_u8, src_f32);
  STIL_REQUIRE(src_u8 ? dst_u8 != nullptr && dst_f32 == nullptr : dst_f32 != nullptr && dst_u8 == nullptr,
               "stil_alb_color: null image pointer (the destination must have the source type)");
  STIL_REQUIRE(order && factors && cj_on && gray_on && gpart, "stil_alb_color: null draw or workspace pointer");
  STIL_REQUIRE(B > 0 && H > 0 && W > 0, "stil_alb_color: empty shape (B=%d, H=%d, W=%d)", B, H, W);
  STIL_REQUIRE(wg_per_image >= 0 && wg_per_image <= ALB_MAX_WG, "stil_alb_color: wg_per_image=%d outside [0, %d]", wg_per_image, ALB_MAX_WG);
  const long npix = (long)H * W, ng = (npix + 3) / 4;
  int nblk = wg_per_image;
  if (nblk == 0) nblk = (int)std::max(1L, std::min<long>({(long)ALB_MAX_WG, (long)cdiv(2048, B), (long)cdiv(ng, 1024)}));   // ~2048 workgroups per launch
  nblk = (int)std::min<long>(nblk, (long)cdiv(ng, 256));
  const bool u8 = src_u8 != nullptr;
  const void* s = u8 ? (const void*)src_u8 : (const void*)src_f32;
  void* d = u8 ? (void*)dst_u8 : (void*)dst_f32;
  const int al = u8 ? 4 : 16;
  AlbColorArgs a{s, d, H, W, order, factors, cj_on, gray_on, gpart, nblk, (npix % 4 == 0 && alb_aligned(s, al) && alb_aligned(d, al)) ? 1 : 0};
  const dim3 grid(nblk, B);
  if (u8) {
    hipLaunchKernelGGL(alb_color_mean_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, a);
    STIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(alb_color_apply_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(alb_color_mean_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, a);
    STIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(alb_color_apply_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, a);
  }
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_alb_blur(const unsigned char* src_u8, const float* src_f32, unsigned char* dst_u8, float* dst_f32, int B, int H, int W,
                             const double* sigma, int ksize, void* stream) {
  ALB_ONE_IMAGE("stil_alb_blur", src_u8, src_f32);
  STIL_REQUIRE(src_u8 ? dst_u8 != nullptr : dst_f32 != nullptr, "stil_alb_blur: null image pointer (the destination must have the source type)");
  STIL_REQUIRE(sigma && B > 0 && H > 0 && W > 0, "stil_alb_blur: null sigma or empty shape");
  STIL_REQUIRE(ksize > 0 && ksize % 2 == 1 && ksize <= ALB_MAX_K, "stil_alb_blur: ksize=%d must be odd, positive and at most %d", ksize, ALB_MAX_K);
  STIL_REQUIRE(src_u8 ? (const void*)src_u8 != (void*)dst_u8 : (const void*)src_f32 != (void*)dst_f32, "stil_alb_blur: cannot run in place");
  const dim3 grid(cdiv(W, ALB_BTX), cdiv(H, ALB_BTY), B);
  if (src_u8) hipLaunchKernelGGL(alb_blur_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, src_u8, dst_u8, sigma, H, W, ksize);
  else hipLaunchKernelGGL(alb_blur_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, src_f32, dst_f32, sigma, H, W, ksize);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_alb_resize(const unsigned char* src_u8, const float* src_f32, unsigned char* dst_u8, float* dst_f32, float* out_chw, int B,
                               int H, int W, const int* box, const unsigned char* flip, int P, void* stream) {
  ALB_ONE_IMAGE("stil_alb_resize", src_u8, src_f32);
  const bool hwc = src_u8 ? dst_u8 != nullptr : dst_f32 != nullptr;
  STIL_REQUIRE(hwc != (out_chw != nullptr), "stil_alb_resize: null image pointer (exactly one of dst of the source type / out_chw)");
  STIL_REQUIRE(box && B > 0 && H > 0 && W > 0, "stil_alb_resize: null box or empty shape");
  STIL_REQUIRE(P > 0, "stil_alb_resize: P=%d must be positive", P);
  const dim3 grid(cdiv((long)P * P, 256), B);
  if (src_u8) hipLaunchKernelGGL(alb_resize_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, src_u8, dst_u8, out_chw, box, flip, H, W, P);
  else hipLaunchKernelGGL(alb_resize_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, src_f32, dst_f32, out_chw, box, flip, H, W, P);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_alb_rotate(const unsigned char* src_u8, const float* src_f32, unsigned char* dst_u8, float* dst_f32, int B, int H, int W,
                               const double* minv, const unsigned char* on, const unsigned char* flip_first, void* stream) {
  ALB_ONE_IMAGE("stil_alb_rotate", src_u8, src_f32);
  STIL_REQUIRE(src_u8 ? dst_u8 != nullptr : dst_f32 != nullptr, "stil_alb_rotate: null image pointer (the destination must have the source type)");
  STIL_REQUIRE(minv && on && B > 0 && H > 0 && W > 0, "stil_alb_rotate: null matrix / flag pointer or empty shape");
  STIL_REQUIRE(src_u8 ? (const void*)src_u8 != (void*)dst_u8 : (const void*)src_f32 != (void*)dst_f32, "stil_alb_rotate: cannot run in place");
  const dim3 grid(cdiv((long)H * W, 256), B);
  if (src_u8) hipLaunchKernelGGL(alb_rotate_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, src_u8, dst_u8, minv, on, flip_first, H, W);
  else hipLaunchKernelGGL(alb_rotate_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, src_f32, dst_f32, minv, on, flip_first, H, W);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

extern "C" int stil_alb_to_tensor(const unsigned char* src_u8, const float* src_f32, float* out, int B, int H, int W, void* stream) {
  ALB_ONE_IMAGE("stil_alb_to_tensor", src_u8, src_f32);
  STIL_REQUIRE(out != nullptr, "stil_alb_to_tensor: null image pointer (out)");
  STIL_REQUIRE(B > 0 && H > 0 && W > 0, "stil_alb_to_tensor: empty shape");
  const long npix = (long)H * W;
  const void* s = src_u8 ? (const void*)src_u8 : (const void*)src_f32;
  const int vec = (npix % 4 == 0 && alb_aligned(s, src_u8 ? 4 : 16) && alb_aligned(out, 16)) ? 1 : 0;
  const dim3 grid(cdiv((npix + 3) / 4, 256), B);
  if (src_u8) hipLaunchKernelGGL(alb_to_tensor_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, src_u8, out, H, W, vec);
  else hipLaunchKernelGGL(alb_to_tensor_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, src_f32, out, H, W, vec);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
