"""Cases, seeded inputs and references shared by tests/test_gpu_augment_kernels.py and tests/test_augment_cases_cpu.py (no test
lives here; nothing here needs a GPU or the library).  The kernels are the input pipeline: csrc/augment.hip (stil_tab_corrupt,
stil_aug_gray_mean, stil_aug_resize, stil_aug_blur, stil_aug_rotate, stil_aug_hue) and the geometry cases of csrc/augment_alb.hip
that tests/test_gpu_augment_alb.py leaves out.  Every image kernel runs one thread per pixel in blocks of 256 (`blockIdx.x * 256 +
threadIdx.x` against H * W or P * P), stil_tab_corrupt one wave per row striding by 64: the shapes sit at 1, below one block, at
255 / 256 / 257 and past one wave.

Two statements of every float kernel:
  * `*_reference`: float64, written from the operation's definition (F.interpolate, F.pad(mode="reflect"), torchvision's colour
    formulas).  It receives the kernel's own fp32 arguments (angle, sigma, jitter, hue, the grey mean, the grey weights) upcast to
    float64, and uint8 sources divided by 255, so only the arithmetic differs from the kernel.
  * `*_restate`: fp32 numpy in the kernel's documented operation order (uint8 sources times fp32(1 / 255), the lerp
    a + l * (b - a), sequential tap sums, the butterfly reduction of the grey mean).  It is the yardstick: E_* below is its largest
    error against the float64 reference over the kernel's case table, measured by tests/test_augment_cases_cpu.py, and the GPU
    check allows ALLOW = 4 times that (device sinf / cosf / expf differ from the host's by a few ulp, FP contraction rounds
    differently).  Every allowance stays below CAP = 1e-4: one mis-indexed pixel of a random uint8 image is at least 1 / 255.

Images are numpy arrays as the kernels take them: uint8 HWC [B, H, W, 3] or float32 CHW [B, 3, H, W]; results are [.., 3, h, w]."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from kernel_edge_cases import SENT, f32  # noqa: F401  (one sentinel for the suite)

F32 = np.float32
INV255 = F32(1.0 / 255.0)               # the `scale` the wrappers pass for uint8 sources (convert_to_ts)
GRAY_W = (F32(0.2989), F32(0.587), F32(0.114))   # gray_of() in augment.hip
DEG2RAD = F32(0.017453292519943295)     # aug_rotate_kernel
FMTS = ("u8", "f32")

ALLOW = 4.0
CAP = 1e-4
# largest |fp32 restatement - float64 reference| over each kernel's case table (measured on the CPU by
# tests/test_augment_cases_cpu.py::test_measured_errors_are_the_constants, which prints them; rounded up to two digits).
# The restatements take expf / sinf / cosf as the correctly rounded value, so the figures do not depend on the host's libm.
E_GRAY_MEAN = 8.3e-8    # measured 8.24e-08 (uint8 1x257, brightness per sample)
E_RESIZE = 3.3e-6       # measured 3.24e-06 (uint8 64x5 -> 15x15): the fp32 sample position, times a step of up to 255 / 255 per pixel
E_COLOUR = 2.7e-6       # measured 2.65e-06 (float 33x31 -> 17x17, contrast and saturation 1.8): the resize error through the colour steps
E_BLUR = 4.1e-7         # measured 4.08e-07 (uint8 15x40, ksize 29, sigma 2): 29 taps twice, sequential fp32 sums
E_ROTATE = 7.1e-6       # measured 7.07e-06 (float 37x53 at 720.5 degrees): fp32 sin / cos move a corner tap by ~1e-5 pixels
E_HUE = 8.1e-7          # measured 8.08e-07 (16x16, hue 0.07 / -0.1)
TOL = {"gray_mean": ALLOW * E_GRAY_MEAN, "resize": ALLOW * E_RESIZE, "colour": ALLOW * E_COLOUR, "blur": ALLOW * E_BLUR,
       "rotate": ALLOW * E_ROTATE, "hue": ALLOW * E_HUE}


def rng(*key):
    return np.random.default_rng([int(k) for k in key])


def max_err(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max())


def check(kind, got, ref, what=""):
    """the one float comparison of this family: max |got - float64 reference| <= 4 * the measured fp32 error of `kind`"""
    got = np.asarray(got)
    assert got.shape == np.asarray(ref).shape, (kind, what, got.shape, np.asarray(ref).shape)
    assert bool(np.isfinite(got).all()), f"{kind} {what}: not finite"
    err = max_err(got, ref)
    assert err <= TOL[kind], f"{kind} {what}: max err {err:.3e} > {TOL[kind]:.3e}"
    return err


# ---------------------------------------------------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------------------------------------------------
def image(fmt, B, H, W, *key, lo=0.0, hi=1.0):
    """uint8 HWC [B, H, W, 3] or float32 CHW [B, 3, H, W] in [lo, hi)"""
    g = rng(H, W, B, *key)
    if fmt == "u8":
        return g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    return (g.random((B, 3, H, W), dtype=np.float32) * F32(hi - lo) + F32(lo)).astype(np.float32)


def is_u8(img):
    return img.dtype == np.uint8


def hw(img):
    return (img.shape[1], img.shape[2]) if is_u8(img) else (img.shape[2], img.shape[3])


def scale_of(img):
    return float(INV255) if is_u8(img) else 1.0


def raw32(img):
    """[B, 3, H, W] fp32, unscaled (what aug_fetch returns)"""
    return np.ascontiguousarray(img.transpose(0, 3, 1, 2)).astype(np.float32) if is_u8(img) else img


def src64(img):
    """[B, 3, H, W] float64 in the kernel's output scale: uint8 / 255, float as is"""
    return np.ascontiguousarray(img.transpose(0, 3, 1, 2)).astype(np.float64) / 255.0 if is_u8(img) else img.astype(np.float64)


def gray(x):
    """x [3, ...] -> [...] in x's dtype, left to right as gray_of()"""
    dt = x.dtype.type
    return dt(GRAY_W[0]) * x[0] + dt(GRAY_W[1]) * x[1] + dt(GRAY_W[2]) * x[2]


def clamp01(x):
    return np.minimum(np.maximum(x, x.dtype.type(0)), x.dtype.type(1))


# =====================================================================================================================
# stil_tab_corrupt: exact
# =====================================================================================================================
TAB_NCOLS = (1, 63, 64, 65, 200)
TAB_KS = (0, 1, 64, 65, "n_cols")
TAB_BS = (1, 5)
TAB_NROWS = (1, 37)


def tab_ks(n_cols):
    return sorted({n_cols if k == "n_cols" else k for k in TAB_KS if k == "n_cols" or k <= n_cols})


TAB_TABLE = tuple((B, n, N, k) for n in TAB_NCOLS for k in tab_ks(n) for B in TAB_BS for N in TAB_NROWS)


def tab_case(B, n_cols, n_rows, k):
    """marginal[c, r] = 1000 c + r + 0.5 (a transposed or mis-strided read names another (c, r)); clean[b, c] = -(1000 b + c) - 0.25;
    idx: k DISTINCT columns per row, pos: table rows with replacement"""
    g = rng(B, n_cols, n_rows, k, 11)
    marginal = (1000.0 * np.arange(n_cols)[:, None] + np.arange(n_rows)[None, :] + 0.5).astype(np.float32)
    clean = (-(1000.0 * np.arange(B)[:, None] + np.arange(n_cols)[None, :]) - 0.25).astype(np.float32)
    idx = np.stack([g.permutation(n_cols)[:k] for _ in range(B)]).astype(np.int32).reshape(B, k)
    pos = g.integers(0, n_rows, (B, k)).astype(np.int32)
    return dict(marginal=marginal, clean=clean, idx=idx, pos=pos)


def tab_reference(c):
    out = c["clean"].copy()
    for b in range(out.shape[0]):
        out[b, c["idx"][b]] = c["marginal"][c["idx"][b], c["pos"][b]]
    return out


# =====================================================================================================================
# stil_aug_gray_mean
# =====================================================================================================================
GM_SHAPES = ((1, 1), (3, 5), (15, 17), (16, 16), (1, 257), (25, 40))       # H * W = 1, 15, 255, 256, 257, 1000
GM_BRIGHTNESS = (0.0, 0.4, 1.8)        # one per sample of the batch of 3; 1.8 makes the clamp active
GM_JUNK = 9.0                          # the three jitter columns the kernel must not read


def gm_image(fmt, H, W):
    """float sources reach outside [0, 1]: the clamp works on both sides"""
    return image(fmt, 3, H, W, 21, lo=-0.3, hi=1.3)


def gm_jitter():
    j = np.full((3, 4), GM_JUNK, dtype=np.float32)
    j[:, 0] = GM_BRIGHTNESS
    return j


def gray_mean_reference(img, brightness=None):
    """-> float64 [B]; brightness: fp32 [B] or None (1)"""
    x = src64(img)
    out = []
    for b in range(len(x)):
        br = 1.0 if brightness is None else float(F32(brightness[b]))
        out.append(gray(clamp01(x[b] * br)).mean())
    return np.array(out, dtype=np.float64)


def gray_mean_restate(img, brightness=None):
    """fp32 in the kernel's order: (v * scale) * br, thread t sums pixels t, t + 256, ..; xor butterfly over each wave of 64; the
    four waves left to right; / (H * W)"""
    x, sc = raw32(img), F32(scale_of(img))
    lane = np.arange(64)
    out = []
    for b in range(len(x)):
        br = F32(1.0) if brightness is None else F32(brightness[b])
        g = gray(clamp01(x[b].reshape(3, -1) * sc * br))
        n = g.shape[0]
        part = np.zeros(256, dtype=np.float32)
        for start in range(0, n, 256):
            chunk = g[start:start + 256]
            part[:len(chunk)] = part[:len(chunk)] + chunk
        total = F32(0.0)
        for w in range(4):
            v = part[64 * w:64 * w + 64].copy()
            for o in (32, 16, 8, 4, 2, 1):
                v = v + v[lane ^ o]
            total = F32(total + v[0])
        out.append(F32(total / F32(n)))
    return np.array(out, dtype=np.float32)


# =====================================================================================================================
# stil_aug_resize
# =====================================================================================================================
RS_PS = (1, 15, 16, 17)                # P * P = 1, 225, 256, 289
RS_SOURCES = ((1, 1), (1, 9), (9, 1), (33, 31), (64, 5))
RS_BOX_NAMES = ("whole", "last pixel", "one column", "one row", "right-bottom border", "interior, upsampled")
RS_JITTER_SHAPES = ((33, 31, 17), (64, 5, 16))
IDENTITY_JITTER = (1.0, 1.0, 1.0, 0.0)
RS_JITTERS = (                         # batches of 3: every sample of a batch has its own factors
    ((0.0, 1.0, 1.0, 0.0), (1.8, 1.0, 1.0, 0.0), (1.0, 0.0, 1.0, 0.0)),
    ((1.0, 1.8, 1.0, 0.0), (1.0, 1.0, 0.0, 0.0), (1.0, 1.0, 1.8, 0.0)),
    ((1.3, 0.6, 1.5, 1.0), (0.4, 1.7, 0.3, 0.0), (1.8, 0.2, 1.7, 1.0)),
)
RS_BAD_SHAPE = (33, 31, 16)
RS_BAD_BOXES = (
    (-3, 4, 10, 10), (4, -5, 10, 10), (-2, -2, 40, 40),          # negative top / left
    (5, 5, 0, 7), (5, 5, 7, -2), (5, 5, -4, 0),                  # a size of 0 or below
    (20, 20, 30, 5), (5, 25, 5, 30), (32, 30, 2, 2),             # a size past the border
    (33, 3, 4, 4), (40, 3, 4, 4), (3, 31, 4, 400),               # top / left at or beyond H / W
)


def resize_boxes(H, W):
    """the six boxes of RS_BOX_NAMES as int32 [6, 4] = (top, left, height, width); where an axis is too short for an interior
    box (n < 3) the box spans it"""
    def inner(n):
        return (n // 3, max(1, n // 5)) if n >= 3 else (0, n)
    (t, h), (l, w) = inner(H), inner(W)
    return np.array([[0, 0, H, W], [H - 1, W - 1, 1, 1], [0, W // 2, H, 1], [H // 2, 0, 1, W],
                     [H - max(1, H // 2), W - max(1, W // 2), max(1, H // 2), max(1, W // 2)], [t, l, h, w]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def resize_source(fmt, H, W):
    """one image per box; the last one is 0 everywhere and full scale inside its interior box: a neighbour read from outside the
    crop would show"""
    img = image(fmt, 6, H, W, 31)
    t, l, h, w = resize_boxes(H, W)[5]
    if is_u8(img):
        img[5] = 0
        img[5, t:t + h, l:l + w] = 255
    else:
        img[5] = 0.0
        img[5, :, t:t + h, l:l + w] = 1.0
    img.setflags(write=False)
    return img


def clamp_box(box, H, W):
    """aug_sample's clamp: a bad box changes the picture, never reads outside it"""
    top, left = min(max(int(box[0]), 0), H - 1), min(max(int(box[1]), 0), W - 1)
    return top, left, min(max(int(box[2]), 1), H - top), min(max(int(box[3]), 1), W - left)


def colour(x, jit, gmean):
    """x [3, h, w] in its own dtype; torchvision's float ops in the kernel's fixed order, the clamp after each"""
    dt = x.dtype.type
    br, ct, sa, gr = (dt(F32(v)) for v in jit)
    m, one = dt(F32(gmean)), dt(1)
    x = clamp01(x * br)
    x = clamp01(ct * x + (one - ct) * m)
    x = clamp01(sa * x + (one - sa) * gray(x))
    if gr != 0:
        x = np.broadcast_to(gray(x), x.shape).copy()
    return x


def resize_reference(img, boxes, P, flip=None, jitter=None, gmean=None):
    """float64: crop -> F.interpolate(bilinear, align_corners=False) -> flip -> colour -> clamp; boxes are clamped as the kernel
    clamps them (the identity on every valid box)"""
    x = src64(img)
    H, W = hw(img)
    out = []
    for b in range(len(x)):
        t, l, h, w = clamp_box(boxes[b], H, W)
        crop = torch.from_numpy(np.ascontiguousarray(x[b, :, t:t + h, l:l + w]))[None]
        y = F.interpolate(crop, size=(P, P), mode="bilinear", align_corners=False)[0].numpy()
        if flip is not None and flip[b]:
            y = y[:, :, ::-1]
        if jitter is not None:
            y = colour(np.ascontiguousarray(y), jitter[b], gmean[b])
        out.append(clamp01(np.ascontiguousarray(y)))
    return np.stack(out)


def resize_restate(img, boxes, P, flip=None, jitter=None, gmean=None):
    """fp32 in aug_sample's order: sy = ch / P, f = max((o + 0.5) sy - 0.5, 0), the neighbours clamped to the crop, the lerp
    a + l (b - a) on unscaled pixels, * scale, colour, clamp"""
    x, sc = raw32(img), F32(scale_of(img))
    H, W = hw(img)
    o = np.arange(P, dtype=np.float32)
    out = []
    for b in range(len(x)):
        t, l, h, w = clamp_box(boxes[b], H, W)

        def axis(n, coords):
            f = np.maximum((coords + F32(0.5)) * (F32(n) / F32(P)) - F32(0.5), F32(0))
            i0 = np.minimum(f.astype(np.int64), n - 1)
            return i0, np.minimum(i0 + 1, n - 1), (f - i0.astype(np.float32)).astype(np.float32)
        y0, y1, ly = axis(h, o)
        x0, x1, lx = axis(w, F32(P - 1) - o if flip is not None and flip[b] else o)
        s = x[b]
        a, bb = s[:, (t + y0)[:, None], (l + x0)[None, :]], s[:, (t + y0)[:, None], (l + x1)[None, :]]
        c, d = s[:, (t + y1)[:, None], (l + x0)[None, :]], s[:, (t + y1)[:, None], (l + x1)[None, :]]
        lx, ly = lx[None, None, :], ly[None, :, None]
        t0, t1 = a + lx * (bb - a), c + lx * (d - c)
        v = (t0 + ly * (t1 - t0)) * sc
        if jitter is not None:
            v = colour(v, jitter[b], gmean[b])
        out.append(clamp01(v))
    return np.stack(out).astype(np.float32)


def jitter_gmean(img, jitter):
    """the contrast constant the host passes: the float64 grey mean of the brightness-adjusted source, rounded to fp32"""
    return gray_mean_reference(img, np.asarray(jitter, dtype=np.float32)[:, 0]).astype(np.float32)


# =====================================================================================================================
# stil_aug_blur
# =====================================================================================================================
BL_GEOMS = ((15, 40, 3), (15, 40, 29), (40, 15, 3), (40, 15, 29), (32, 33, 63), (2, 86, 3), (15, 17, 3), (16, 16, 3))   # H, W, ksize
BL_SIGMAS = ((-1.0, 0.05, 2.0), (0.0, 0.1, 50.0), (0.9, 2.0, 0.0))     # batches of 3 over {-1, 0, 0.05, 0.1, 0.9, 2.0, 50}


def blur_weights(k, sigma, dt):
    """exp(-0.5 (x / sigma)^2), normalised; fp32: -0.5f * (x / sg) * (x / sg) left to right, the sum tap by tap"""
    x = (np.arange(k) - k // 2).astype(dt)
    sg = dt(F32(sigma))
    if not sg > 0:
        return (np.arange(k) == k // 2).astype(dt)
    q = x / sg
    w = np.exp((dt(-0.5) * q * q).astype(np.float64)).astype(dt)        # fp32: expf rounded correctly, whatever the host's SIMD exp does
    s = dt(0)
    for v in w:
        s = dt(s + v)
    return (w / s).astype(dt)


def blur_reference(img, sigma, k):
    """float64: F.pad(mode="reflect") by the radius, the weights applied along rows, then along columns; sigma <= 0 copies"""
    x = torch.from_numpy(src64(img))
    H, W = hw(img)
    r = k // 2
    out = []
    for b in range(len(x)):
        if not float(F32(sigma[b])) > 0:
            out.append(x[b].numpy())
            continue
        w = blur_weights(k, sigma[b], np.float64)
        pad = F.pad(x[b:b + 1], (r, r, r, r), mode="reflect")[0]
        rows = sum(float(w[t]) * pad[:, :, t:t + W] for t in range(k))
        out.append(sum(float(w[t]) * rows[:, t:t + H] for t in range(k)).numpy())
    return np.stack(out)


def _reflect_blur(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def blur_restate(img, sigma, k):
    """fp32 in aug_blur_kernel's order: pass 0 along rows on v * scale, pass 1 along columns, acc += (w[t] / wsum) * v tap by tap"""
    x, sc = raw32(img), F32(scale_of(img))
    H, W = hw(img)
    r = k // 2
    out = []
    for b in range(len(x)):
        w = blur_weights(k, sigma[b], np.float32)
        s = x[b] * sc
        acc = np.zeros_like(s)
        for t in range(k):
            acc = acc + w[t] * s[:, :, _reflect_blur(np.arange(W) + t - r, W)]
        mid, acc = acc, np.zeros_like(s)
        for t in range(k):
            acc = acc + w[t] * mid[:, _reflect_blur(np.arange(H) + t - r, H)]
        out.append(acc)
    return np.stack(out).astype(np.float32)


# =====================================================================================================================
# stil_aug_rotate
# =====================================================================================================================
RT_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 50), (50, 2), (15, 17), (16, 16), (3, 86), (37, 53))
RT_ANGLE_SET = (0.0, 1e-3, 17.5, 45.0, -44.0, 90.0, -90.0, 180.0, 270.0, 360.0, 720.5)
RT_ANGLES = ((0.0, 17.5, 90.0), (1e-3, 45.0, -90.0), (-44.0, 180.0, 720.5), (270.0, 360.0, 0.0))    # batches of 3


def reflect101(i, n):
    """cv2.BORDER_REFLECT_101 with Python's non-negative %; an axis of one pixel has no period: every tap is pixel 0"""
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = i % period
    return np.where(i < n, i, period - i)


def rotate_taps(H, W, angle, dt=np.float32):
    """-> (floor(fx), floor(fy), lx, ly) of every output pixel, [H, W]; fp32 follows aug_rotate_kernel (th = angle * DEG2RAD,
    cosf / sinf), float64 takes the fp32 angle times pi / 180"""
    ys, xs = np.meshgrid(np.arange(H, dtype=dt), np.arange(W, dtype=dt), indexing="ij")
    if dt is np.float32:
        th = F32(F32(angle) * DEG2RAD)
        ca, sa = F32(np.cos(np.float64(th))), F32(np.sin(np.float64(th)))     # cosf / sinf rounded correctly, on any host
    else:
        th = float(F32(angle)) * np.pi / 180.0
        ca, sa = np.cos(th), np.sin(th)
    cx, cy = dt(0.5) * dt(W - 1), dt(0.5) * dt(H - 1)
    dx, dy = xs - cx, ys - cy
    fx, fy = ca * dx - sa * dy + cx, sa * dx + ca * dy + cy
    flx, fly = np.floor(fx), np.floor(fy)
    return flx.astype(np.int64), fly.astype(np.int64), (fx - flx).astype(dt), (fy - fly).astype(dt)


def rotate_reference(img, angle):
    """float64: A.Rotate's geometry (cv2.getRotationMatrix2D about ((W-1)/2, (H-1)/2), bilinear, BORDER_REFLECT_101)"""
    x = src64(img)
    H, W = hw(img)
    out = []
    for b in range(len(x)):
        flx, fly, lx, ly = rotate_taps(H, W, angle[b], np.float64)
        X0, X1, Y0, Y1 = reflect101(flx, W), reflect101(flx + 1, W), reflect101(fly, H), reflect101(fly + 1, H)
        s = x[b]
        out.append((s[:, Y0, X0] * (1 - lx) + s[:, Y0, X1] * lx) * (1 - ly) + (s[:, Y1, X0] * (1 - lx) + s[:, Y1, X1] * lx) * ly)
    return np.stack(out)


def rotate_restate(img, angle):
    x, sc = raw32(img), F32(scale_of(img))
    H, W = hw(img)
    out = []
    for b in range(len(x)):
        flx, fly, lx, ly = rotate_taps(H, W, angle[b], np.float32)
        X0, X1, Y0, Y1 = reflect101(flx, W), reflect101(flx + 1, W), reflect101(fly, H), reflect101(fly + 1, H)
        s = x[b]
        a, bb, c, d = s[:, Y0, X0], s[:, Y0, X1], s[:, Y1, X0], s[:, Y1, X1]
        t0, t1 = a + lx * (bb - a), c + lx * (d - c)
        out.append((t0 + ly * (t1 - t0)) * sc)
    return np.stack(out).astype(np.float32)


# =====================================================================================================================
# stil_aug_hue
# =====================================================================================================================
HUE_SHAPES = ((1, 1), (15, 17), (16, 16), (20, 24))
HUE_SET = (0.0, 0.07, -0.1, 0.5, -0.5)
HUE_CALLS = (                          # (hue [3] or None, gray [3] or None)
    ((0.07, -0.1, 0.0), None),
    ((0.5, -0.5, 0.07), (0.0, 0.0, 0.0)),
    ((0.0, 0.5, -0.1), (0.0, 1.0, 1.0)),
    ((-0.5, 0.07, 0.5), (1.0, 0.0, 0.0)),
    (None, (1.0, 0.0, 1.0)),
)
# grey, black, white, the primaries, the secondaries (the two largest channels tie), dimmer ties.  Primaries and secondaries sit
# at h = j / 6: a shift of +-0.5 = 3 / 6 lands them on a sector boundary again, where the two sectors give the same colour.
HUE_PLANTS = ((0.4, 0.4, 0.4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0),
              (1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0), (0.75, 0.75, 0.25), (0.25, 0.5, 0.5), (0.625, 0.125, 0.625))


@functools.lru_cache(maxsize=None)
def hue_image(H, W):
    """float32 CHW [3, 3, H, W] in [0, 1); sample b starts with the plants from number 4 b on (a 1x1 image holds one each)"""
    img = image("f32", 3, H, W, 41)
    flat = img.reshape(3, 3, -1)
    for b in range(3):
        for p in range(min(H * W, len(HUE_PLANTS))):
            flat[b, :, p] = HUE_PLANTS[(p + 4 * b) % len(HUE_PLANTS)]
    img.setflags(write=False)
    return img


def hue_steps(x, hf):
    """torchvision's _rgb2hsv / adjust_hue / _hsv2rgb on x [3, ...] in its own dtype -> (rgb, sector, h + hue before the wrap)"""
    dt = x.dtype.type
    r, g, b = x[0], x[1], x[2]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    eq = maxc == minc
    cr = maxc - minc
    one = np.ones_like(maxc)
    s = cr / np.where(eq, one, maxc)
    dv = np.where(eq, one, cr)
    rc, gc, bc = (maxc - r) / dv, (maxc - g) / dv, (maxc - b) / dv
    h = np.where(maxc == r, bc - gc, np.where(maxc == g, dt(2) + rc - bc, dt(4) + gc - rc))
    h = np.fmod(h / dt(6) + dt(1), dt(1))
    moved = h + dt(F32(hf))
    h = moved - np.floor(moved)
    h6 = h * dt(6)
    fi = np.floor(h6)
    f = h6 - fi
    i = fi.astype(np.int64) % 6
    p, q, t = clamp01(maxc * (dt(1) - s)), clamp01(maxc * (dt(1) - f * s)), clamp01(maxc * (dt(1) - (dt(1) - f) * s))
    v = maxc
    pick = lambda *c: np.choose(i, c)
    return np.stack((pick(v, q, p, p, t, v), pick(t, v, v, q, p, p), pick(p, p, t, v, v, q))), i, moved


def hue_apply(img, hue, gray_on, dt):
    """the kernel on a batch in dtype dt: the hue shift where hue[b] != 0, then the grey image where gray[b] != 0"""
    out = []
    for b in range(len(img)):
        x = img[b].astype(dt)
        if hue is not None and float(F32(hue[b])) != 0.0:
            x = hue_steps(x, hue[b])[0]
        if gray_on is not None and float(gray_on[b]) != 0.0:
            x = np.broadcast_to(gray(x), x.shape).copy()
        out.append(x)
    return np.stack(out)


def hue_reference(img, hue, gray_on):
    return hue_apply(img, hue, gray_on, np.float64)


def hue_restate(img, hue, gray_on):
    return hue_apply(img, hue, gray_on, np.float32)


# =====================================================================================================================
# part B: the geometry of csrc/augment_alb.hip that tests/test_gpu_augment_alb.py leaves out (reference: tests/alb_restate.py)
# =====================================================================================================================
ALB_NPIX = ((1, 1), (1, 3), (2, 2), (1, 5), (33, 31), (32, 32), (25, 41))     # H * W = 1, 3, 4, 5, 1023, 1024, 1025
ALB_MISALIGNED = (4, 8)                # npix % 4 == 0, run from a base address 1 element into its buffer
ALB_WG = ((256, 256), (5, 5))          # wg_per_image = 64: 64 workgroups really run / clipped to 1
ALB_BLUR_KS = (3, 31)
ALB_BLUR_TILE = tuple((H, W) for H in (15, 16, 17) for W in (31, 32, 33))
ALB_BLUR_SHORT = ((1, 40), (40, 1), (2, 3), (1, 1))      # shorter than the radius of ksize 29
ALB_RESIZE_PS = (1, 15, 16, 17)
ALB_RESIZE_SOURCES = ((1, 1), (1, 9), (9, 1))
ALB_ROT_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 50), (15, 17), (16, 16))
ALB_ROT_ANGLES = (0.0, 90.0, -90.0, 180.0, 45.0)


def alb_image(fmt, B, H, W, *key):
    """HWC [B, H, W, 3]: uint8 or float32 in [0, 1)"""
    g = rng(H, W, B, 51, *key)
    return g.integers(0, 256, (B, H, W, 3), dtype=np.uint8) if fmt == "u8" else g.random((B, H, W, 3), dtype=np.float32)


def alb_color_draws(B, *key):
    """-> order int32 [B, 4], factors float64 [B, 4], cj_on, gray_on uint8 [B]: sample 0 has every op and the grey conversion,
    sample 1 is switched off (a copy), the rest are drawn"""
    g = rng(B, 52, *key)
    order = np.argsort(g.random((B, 4)), 1).astype(np.int32)
    fac = np.concatenate([g.uniform(0.2, 1.8, (B, 3)), g.uniform(-0.2, 0.2, (B, 1))], 1)
    cj_on, gray_on = np.ones(B, np.uint8), (g.random(B) < 0.4).astype(np.uint8)
    fac[0], gray_on[0] = [1.3, 0.6, 1.4, 0.1], 1
    if B > 1:
        cj_on[1], gray_on[1] = 0, 0
    return order, fac, cj_on, gray_on
