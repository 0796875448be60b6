"""numpy restatement of the albumentations branch's pixel definitions (utils/utils.py:46-256, augmentation_speedup=True),
the one place the device kernels of csrc/augment_alb.hip are checked against.  Images are one HWC array [H, W, 3], uint8 or
float32 in [0, 1]; every op returns the source type, as each albumentations 1.3.1 stage does.

Exact (albumentations 1.3.1's functional code under numpy 1.23, the reference's pin): the brightness / contrast LUTs built
in float64, the hue LUT in float32 (value-based casting of int16 + float), each truncated by astype(uint8), the float brightness / contrast formulas, the identity factors, flip, crop geometry, to-tensor.
Chosen rounding rules (as recalled from OpenCV 4.x, NOT pinned against cv2, which is absent offline; they may differ from it
by 1 uint8 LSB in places): the uint8 grey weights, addWeighted in float32, 8-bit RGB<->HSV, and the single round-to-nearest
of blur, resize and rotate.  A session with cv2 available can diff each function below against it.

All float32 arithmetic is written one IEEE operation at a time (numpy never fuses), in the order the kernels use.
"""
import math

import numpy as np

f32 = np.float32


def sat_u8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def gray(img):
    """cv2.cvtColor(RGB2GRAY) -> [H, W] of the image's type."""
    if img.dtype == np.uint8:
        r, g, b = (img[..., c].astype(np.int64) for c in range(3))
        return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)
    return img[..., 0] * f32(0.299) + img[..., 1] * f32(0.587) + img[..., 2] * f32(0.114)


def to_gray(img):
    """A.ToGray: the grey image in all 3 channels."""
    return np.repeat(gray(img)[..., None], 3, axis=2)


def brightness(img, f):
    if f == 1:
        return img
    if img.dtype == np.uint8:
        lut = np.clip(np.arange(256) * f, 0, 255).astype(np.uint8)
        return lut[img]
    return np.clip(img * f32(f), 0, 1).astype(np.float32)


def gray_mean(img):
    """the mean adjust_contrast blends with: uint8 = integer sum / N in double; float = the float grey image summed in double"""
    g = gray(img)
    if img.dtype == np.uint8:
        return float(int(g.astype(np.int64).sum())) / g.size
    return float(g.astype(np.float64).sum()) / g.size


def contrast(img, f):
    if f == 1:
        return img
    mean = gray_mean(img)
    if img.dtype == np.uint8:
        if f == 0:
            return np.full_like(img, int(mean + 0.5))
        lut = np.clip(np.arange(256) * f + mean * (1 - f), 0, 255).astype(np.uint8)
        return lut[img]
    if f == 0:
        return np.full_like(img, f32(mean))
    return np.clip(img * f32(f) + f32(mean * (1 - f)), 0, 1).astype(np.float32)


def saturation(img, f):
    """cv2.addWeighted(img, f, gray3, 1 - f, 0) in float32, rounded to nearest-even and saturated for uint8"""
    if f == 1:
        return img
    g = gray(img).astype(np.float32)[..., None]
    t = img.astype(np.float32) * f32(f) + g * f32(1 - f)
    return sat_u8(t) if img.dtype == np.uint8 else np.clip(t, 0, 1).astype(np.float32)


def _hsv2rgb(h, s, v, hscale):
    """cv2 HSV2RGB float core; h, s, v float32 arrays -> [.., 3] float32"""
    h = h * f32(hscale)
    h = np.where(h < 0, h + f32(6), h)
    h = np.where(h >= 6, h - f32(6), h)
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(np.float32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, f32(0), h)
    one = f32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], -1)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    pick = lambda k: np.take_along_axis(tab, sd[sector, k][..., None], -1)[..., 0]
    out = np.stack([pick(2), pick(1), pick(0)], -1)
    grey = (s == 0)[..., None]
    return np.where(grey, np.stack([v, v, v], -1), out).astype(np.float32)


def rgb2hsv_u8(img):
    """OpenCV's 8-bit RGB2HSV: H in [0, 180), S, V in [0, 255] (integer division tables, 12-bit fixed point)"""
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(r, np.maximum(g, b))
    vmin = np.minimum(r, np.minimum(g, b))
    diff = v - vmin
    i = np.arange(256)
    with np.errstate(divide="ignore"):
        sdiv = np.where(i > 0, np.rint((255 << 12) / (1.0 * i)), 0).astype(np.int64)
        hdiv = np.where(i > 0, np.rint((180 << 12) / (6.0 * i)), 0).astype(np.int64)
    vr = np.where(v == r, -1, 0)
    vg = np.where(v == g, -1, 0)
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return h, s, v


def hue(img, f):
    if f == 0:
        return img
    if img.dtype == np.uint8:
        h, s, v = rgb2hsv_u8(img)
        # int16 arange + a Python float is float32 under numpy 1.23's value-based casting (the reference's pin)
        lut = np.mod(np.arange(256, dtype=np.int16).astype(np.float32) + f32(180 * f), f32(180)).astype(np.uint8)
        h = lut[h]
        rgb = _hsv2rgb(h.astype(np.float32), s.astype(np.float32) * (f32(1) / f32(255)), v.astype(np.float32) * (f32(1) / f32(255)), f32(6) / f32(180))
        return sat_u8(rgb * f32(255))
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    eps = f32(np.finfo(np.float32).eps)
    v = np.maximum(r, np.maximum(g, b))
    vmin = np.minimum(r, np.minimum(g, b))
    diff = v - vmin
    s = diff / (np.abs(v) + eps)
    d = (60.0 / (diff + eps).astype(np.float64)).astype(np.float32)
    hh = np.where(v == r, (g - b) * d, np.where(v == g, (b - r) * d + f32(120), (r - g) * d + f32(240)))
    hh = np.where(hh < 0, hh + f32(360), hh)
    hh = hh + f32(f * 360.0)
    hh = np.fmod(hh, f32(360))
    hh = np.where(hh < 0, hh + f32(360), hh).astype(np.float32)
    return _hsv2rgb(hh, s, v, f32(6) / f32(360))


_OPS = (brightness, contrast, saturation, hue)


def color_jitter(img, order, factors):
    """A.ColorJitter.apply: the four ops in the image's order; factors = (brightness, contrast, saturation, hue)"""
    for i in order:
        img = _OPS[i](img, factors[i])
    return img


def _reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def blur_weights(k, sigma):
    x = np.arange(k) - (k - 1) * 0.5
    t = np.exp(-0.5 / (sigma * sigma) * x * x)
    s = 0.0
    for v in t:          # left to right, as the kernel sums
        s += v
    return (t * (1.0 / s)).astype(np.float32)


def _reflect(i, n):
    """cv2.BORDER_REFLECT (the edge pixel repeated): what the blur must NOT use"""
    p = 2 * n
    i = np.mod(i, p)
    return np.where(i < n, i, p - 1 - i)


def gaussian_blur(img, k, sigma):
    """cv2.GaussianBlur(img, (k, k), sigma): separable, float32 accumulation tap by tap, reflect-101, one rounding"""
    return gaussian_blur_border(img, k, sigma)


def gaussian_blur_border(img, k, sigma, edge_repeat=False):
    if not sigma > 0:
        return img
    w = blur_weights(k, sigma)
    H, W = img.shape[:2]
    half = k // 2
    x = img.astype(np.float32)
    border = _reflect if edge_repeat else _reflect101
    cols = border(np.arange(W)[:, None] + np.arange(k)[None, :] - half, W)
    rows = border(np.arange(H)[:, None] + np.arange(k)[None, :] - half, H)
    acc = np.zeros_like(x)
    for t in range(k):
        acc = acc + w[t] * x[:, cols[:, t]]
    mid = acc
    acc = np.zeros_like(x)
    for t in range(k):
        acc = acc + w[t] * mid[rows[:, t]]
    return sat_u8(acc) if img.dtype == np.uint8 else acc


def _lin(n_out, n_in):
    d = np.arange(n_out)
    scale = 1.0 / (n_out / n_in)
    fx = ((d + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = fx - sx.astype(np.float32)
    lo = sx < 0
    fx, sx = np.where(lo, f32(0), fx), np.where(lo, 0, sx)
    hi = sx >= n_in - 1
    fx, sx = np.where(hi, f32(0), fx), np.where(hi, n_in - 1, sx)
    return sx, np.minimum(sx + 1, n_in - 1), fx.astype(np.float32)


def resize_crop(img, box, P, flip=False):
    """crop box (top, left, h, w) -> cv2.resize INTER_LINEAR to P x P -> optional HorizontalFlip; source type"""
    t, l, h, w = (int(v) for v in box)
    c = img[t:t + h, l:l + w].astype(np.float32)
    y0, y1, fy = _lin(P, h)
    x0, x1, fx = _lin(P, w)
    gx, gy = (f32(1) - fx)[None, :, None], (f32(1) - fy)[:, None, None]
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = c[y0][:, x0] * gx + c[y0][:, x1] * fx
    bot = c[y1][:, x0] * gx + c[y1][:, x1] * fx
    out = top * gy + bot * fy
    out = sat_u8(out) if img.dtype == np.uint8 else out.astype(np.float32)
    return out[:, ::-1].copy() if flip else out


def rotation_matrix(angle, H, W):
    """getRotationMatrix2D((W/2 - 0.5, H/2 - 0.5), angle, 1), inverted as warpAffine does -> float64 [6]"""
    cx, cy = float(np.float32(W / 2 - 0.5)), float(np.float32(H / 2 - 0.5))
    a = angle * (math.pi / 180)
    al, be = math.cos(a), math.sin(a)
    M = [al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0], M[1], M[3], M[4] = A11, M[1] * -D, M[3] * -D, A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return np.array(M, dtype=np.float64)


def rotate(img, angle, flip_first=False):
    """A.Rotate: cv2.warpAffine with the source position quantised to 1/32 pixel, bilinear, reflect-101, same size"""
    if flip_first:
        img = img[:, ::-1]
    H, W = img.shape[:2]
    M = rotation_matrix(angle, H, W)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    adelta = np.rint(M[0] * x * 1024.0).astype(np.int64)
    bdelta = np.rint(M[3] * x * 1024.0).astype(np.int64)
    X0 = np.rint((M[1] * y + M[2]) * 1024.0).astype(np.int64) + 16
    Y0 = np.rint((M[4] * y + M[5]) * 1024.0).astype(np.int64) + 16
    X, Y = (X0 + adelta) >> 5, (Y0 + bdelta) >> 5
    sx, sy = X >> 5, Y >> 5
    ax, ay = (X & 31).astype(np.float32) * f32(1 / 32), (Y & 31).astype(np.float32) * f32(1 / 32)
    x0, x1 = _reflect101(sx, W), _reflect101(sx + 1, W)
    y0, y1 = _reflect101(sy, H), _reflect101(sy + 1, H)
    s = img.astype(np.float32)
    one = f32(1)
    w00, w01, w10, w11 = ((one - ay) * (one - ax))[..., None], ((one - ay) * ax)[..., None], (ay * (one - ax))[..., None], (ay * ax)[..., None]
    out = s[y0, x0] * w00 + s[y0, x1] * w01 + s[y1, x0] * w10 + s[y1, x1] * w11
    return sat_u8(out) if img.dtype == np.uint8 else out.astype(np.float32)


def to_tensor(img):
    """convert_to_ts (uint8: float32(v / 255.0)) / convert_to_ts_01 (float32: as is) -> float32 [3, H, W]"""
    x = (img / 255.0).astype(np.float32) if img.dtype == np.uint8 else img.astype(np.float32)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def apply_chain(img, stages, d, i, P):
    """The image i of a batch through the stages of stil_tta_amd.augment._alb_policy with the batch draws d ->
    float32 [3, P, P] (the albumentations Compose of one sample, restated)."""
    cropped = False
    for name, prm in stages:
        if name == "cj":
            if d["cj_on"][i]:
                img = color_jitter(img, d["order"][i], d["factors"][i])
        elif name == "gray":
            if d["gray_on"][i]:
                img = to_gray(img)
        elif name == "blur":
            img = gaussian_blur(img, prm["k"], float(d["sigma"][i]))
        elif name == "rotate":
            if d["rot_on"][i]:
                img = rotate(img, float(d["angle"][i]))
        elif name == "flip":                       # drawn into flip_first before the crop, flip after it
            if d["flip" if cropped else "flip_first"][i]:
                img = img[:, ::-1].copy()
        elif name == "rrc":
            img, cropped = resize_crop(img, d["boxes"][i], P), True
        elif name == "resize":                     # A.Resize: the whole image
            img = resize_crop(img, (0, 0) + img.shape[:2], P)
        elif name == "to_tensor":
            return to_tensor(img)
    raise AssertionError("a chain ends with to_tensor")
