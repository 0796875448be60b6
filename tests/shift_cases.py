"""The cases of tests/test_gpu_shift.py as data, and the definitions of csrc/stil_shift.h restated in numpy: the counter hash in
uint64, the arithmetic kinds (Gaussian noise, contrast, brightness, pixelate, tabular noise) in a dtype the caller picks (float64
is the model, float32 the yardstick of tests/test_shift_cpu.py), the selection kinds (impulse, missing, categorical flip) in
integers, so that those are compared bit for bit.

Every strength, bound and operand is the float32 the kernel receives; `dtype` only sets the precision of the arithmetic on them.
This module imports neither the library nor CUDA: tests/test_shift_cpu.py runs everything here on the host."""
import numpy as np

U64 = np.uint64
SENT = -777.0
INF = float("inf")

# ---------------------------------------------------------------------------------------------------------------- cases
NOISE_SHAPES = [(2, 3, 5, 7), (1, 3, 16, 16), (3, 1, 1, 1)]     # 210 elements (4-byte path), 768 (16-byte path), 3
NOISE_OFFSETS = [0, 1, 2 ** 32 - 5]                              # even, odd (pairs straddle the 16-byte groups), past 32 bits
NOISE_STRENGTH = {0: 0.38, 1: 0.27}                              # kind: the severity-5 strength
CONTRAST_HW = (1, 63, 64, 65, 1027, 50176)                       # below / at / above one wave, ragged, a 224 x 224 plane
CONTRAST_BC = (2, 3)
CONTRAST_FACTORS = (0.4, 0.05)
BRIGHT_DELTAS = (0.1, 0.5)
PIX_SIDES = (1, 2, 3, 8, 64)
PIX_IMAGES = ((5, 7), (16, 16))
PIX_BC = (2, 3)
TAB_LAYOUTS = ((7, 0), (7, 7), (9, 4))                           # (n_cols, num_cat)
TAB_BATCHES = (1, 12, 257)
TAB_STRENGTH = {0: 2.0, 1: 0.3, 2: 0.5}
TAB_CAT_LEN = (3, 1, 4, 5, 2, 6, 2)                              # a column with one code included
SEED = 2024


def rng(*key):
    return np.random.default_rng([int(k) for k in key])


def f32(v):
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------- the hash
def aug_hash(seed, ctr):
    """aug_hash of csrc/augment.hip on a uint64 array of counters -> uint32 (as uint64 values)"""
    ctr = np.asarray(ctr, dtype=U64)
    with np.errstate(over="ignore"):
        z = U64(int(seed) & (2 ** 64 - 1)) + U64(0x9E3779B97F4A7C15) * (ctr + U64(1))
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        z = z ^ (z >> U64(31))
    return (z >> U64(16)) & U64(0xFFFFFFFF)


def r24(seed, ctr):
    return aug_hash(seed, ctr) >> U64(8)


def counters(offset, n):
    with np.errstate(over="ignore"):
        return U64(int(offset) & (2 ** 64 - 1)) + np.arange(n, dtype=U64)


def times2(e, plus=0):
    with np.errstate(over="ignore"):
        return e * U64(2) + U64(plus)


def gauss(seed, e, dtype=np.float64):
    """the normal of stream element e: pair j = e >> 1, the even member takes the cosine, the odd one the sine"""
    e = np.asarray(e, dtype=U64)
    j = e >> U64(1)
    u1 = ((r24(seed, times2(j)) + U64(1)).astype(np.float64) * 2.0 ** -24).astype(dtype)      # exact in float32
    u2 = (r24(seed, times2(j, 1)).astype(np.float64) * 2.0 ** -24).astype(dtype)
    rho = np.sqrt(dtype(-2.0) * np.log(u1))
    ang = dtype(2.0 * np.pi) * u2
    return np.where((e & U64(1)) == U64(1), rho * np.sin(ang), rho * np.cos(ang)).astype(dtype)


def hit(seed, ctr, strength):
    """u(ctr) < strength, both float32 and exact: r24 < strength 2^24, compared in float64 (exact on both sides)"""
    return r24(seed, ctr).astype(np.float64) < float(np.float32(strength)) * 2.0 ** 24


def clip(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


# ---------------------------------------------------------------------------------------------------------------- definitions
def noise_model(x, kind, strength, lo, hi, seed, offset, dtype=np.float64):
    x = np.asarray(x, dtype=np.float32)
    e = counters(offset, x.size).reshape(x.shape)
    if kind == 0:
        return clip(x.astype(dtype) + dtype(f32(strength)) * gauss(seed, e, dtype), dtype(lo), dtype(hi)).astype(dtype)
    half = f32(0.5) * f32(strength)
    return np.where(hit(seed, e, half), np.float32(lo), np.where(hit(seed, e, strength), np.float32(hi), x)).astype(np.float32)


def contrast_model(x, factor, lo, hi, dtype=np.float64):
    """x [B, C, HW] -> (out, m [B, C] float32): the plane mean is a float32 by definition (double sum, rounded once)"""
    x = np.asarray(x, dtype=np.float32)
    m = x.astype(np.float64).mean(axis=2).astype(np.float32)
    md = m.astype(dtype)[:, :, None]
    return clip((x.astype(dtype) - md) * dtype(f32(factor)) + md, dtype(lo), dtype(hi)).astype(dtype), m


def brightness_model(x, delta, lo, hi, dtype=np.float64):
    """x [B, 3, HW]"""
    x = np.asarray(x, dtype=np.float32).astype(dtype)
    val = x.max(axis=1, keepdims=True)
    nv = np.minimum(np.maximum(val, dtype(0)) + dtype(f32(delta)), dtype(hi))
    pos = val > 0
    ratio = nv / np.where(pos, val, dtype(1))
    return np.where(pos, clip(x * ratio, dtype(lo), dtype(hi)), np.broadcast_to(nv, x.shape)).astype(dtype)


def pixelate_model(x, s, dtype=np.float64):
    """x [B, C, H, W]"""
    x = np.asarray(x, dtype=np.float32).astype(dtype)
    out = np.empty_like(x)
    H, W = x.shape[2:]
    for y0 in range(0, H, s):
        for x0 in range(0, W, s):
            blk = x[:, :, y0:y0 + s, x0:x0 + s]
            tot = np.zeros(x.shape[:2], dtype=dtype)
            for yy in range(blk.shape[2]):              # row-major, one element after the other: the kernel's order in float32
                for xx in range(blk.shape[3]):
                    tot = tot + blk[:, :, yy, xx]
            out[:, :, y0:y0 + s, x0:x0 + s] = (tot / dtype(blk.shape[2] * blk.shape[3]))[:, :, None, None]
    return out


def tab_model(x, num_cat, cat_len, col_on, col_std, col_fill, kind, strength, seed, offset, dtype=np.float64):
    """x [B, n_cols] -> noise: `dtype`; missing / categorical flip: float32, exact"""
    x = np.asarray(x, dtype=np.float32)
    B, n = x.shape
    e = counters(offset, B * n).reshape(B, n)
    cols = np.arange(n)[None, :]
    on = np.asarray(col_on, dtype=bool)[None, :]
    if kind == 0:
        amp = (np.float32(strength) * np.asarray(col_std, dtype=np.float32)).astype(dtype)[None, :]   # the float32 product of the kernel
        return np.where(on & (cols >= num_cat), x.astype(dtype) + amp * gauss(seed, e, dtype), x.astype(dtype)).astype(dtype)
    if kind == 1:
        return np.where(on & hit(seed, e, strength), np.asarray(col_fill, dtype=np.float32)[None, :], x).astype(np.float32)
    lens = np.ones(n, dtype=np.uint64)
    lens[:num_cat] = np.asarray(cat_len, dtype=np.uint64)[:num_cat]
    code = ((r24(seed, times2(e, 1)) * lens[None, :]) >> U64(24)).astype(np.float32)
    return np.where(on & (cols < num_cat) & hit(seed, times2(e), strength), code, x).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- inputs
def image_input(shape, seed=0):
    return rng(SEED, seed, *shape).random(shape, dtype=np.float32)


def contrast_input(HW, seed=0):
    B, C = CONTRAST_BC
    x = image_input((B, C, HW), seed)
    x[0, 1] = np.float32(0.7)             # a constant plane
    return x


def brightness_input(HW=37, seed=0):
    """[2, 3, HW]: random pixels, then the edges -- exact zeros in one, two and all three channels, V = 2^-20, r = g = b, V so large
    that V + delta passes hi, a negative channel under a positive V, and a pixel with no positive channel"""
    x = image_input((2, 3, HW), seed)
    x[0, 0, 0] = 0.0
    x[0, :2, 1] = 0.0
    x[0, :, 2] = 0.0
    x[0, :, 3] = (2.0 ** -20, 2.0 ** -21, 0.0)
    x[0, :, 4] = 0.4
    x[0, :, 5] = (0.95, 0.5, 0.25)
    x[0, :, 6] = (1.0, 1.0, 0.5)
    x[1, :, 0] = (0.5, -0.125, 0.25)
    x[1, :, 1] = (-0.5, -0.25, 0.0)
    return x


def table_input(B, n_cols, num_cat, seed=0):
    g = rng(SEED, seed, B, n_cols, num_cat)
    x = g.normal(size=(B, n_cols)).astype(np.float32) * 3 + 1
    for c in range(num_cat):
        x[:, c] = g.integers(0, TAB_CAT_LEN[c], size=B).astype(np.float32)
    return x


def table_stats(n_cols, num_cat):
    """explicit vectors (cat_len, col_std, col_fill): a zero deviation among the continuous columns, valid codes as categorical fills"""
    g = rng(SEED, 99, n_cols, num_cat)
    std = (g.random(n_cols) * 2 + 0.25).astype(np.float32)
    fill = g.normal(size=n_cols).astype(np.float32)
    for c in range(num_cat):
        fill[c] = float(TAB_CAT_LEN[c] - 1)
    if num_cat < n_cols:
        std[n_cols - 1] = 0.0
    return np.asarray(TAB_CAT_LEN[:num_cat], dtype=np.int32), std, fill


def table_columns(n_cols):
    """the column sets the tabular cases run with: all, a fixed subset, none"""
    some = np.zeros(n_cols, dtype=np.uint8)
    some[[0, 2, n_cols - 2, n_cols - 1]] = 1
    return {"all": np.ones(n_cols, dtype=np.uint8), "some": some, "none": np.zeros(n_cols, dtype=np.uint8)}


def arithmetic_cases():
    """every arithmetic case of the GPU module as (kind, label, fn(dtype) -> array): the float32-against-float64 yardstick of
    tests/test_shift_cpu.py runs over exactly these"""
    out = []
    for shape in NOISE_SHAPES:
        for off in NOISE_OFFSETS:
            for lo, hi in ((0.0, 1.0), (-INF, INF)):
                out.append(("gaussian_noise", f"{shape}@{off} clip {lo}", lambda dt, s=shape, o=off, lo=lo, hi=hi:
                            noise_model(image_input(s), 0, NOISE_STRENGTH[0], lo, hi, SEED, o, dt)))
    for HW in CONTRAST_HW:
        for fac in CONTRAST_FACTORS:
            out.append(("contrast", f"HW {HW} factor {fac}", lambda dt, h=HW, f=fac: contrast_model(contrast_input(h), f, 0.0, 1.0, dt)[0]))
    for d in BRIGHT_DELTAS:
        for lo, hi in ((0.0, 1.0), (-INF, INF)):
            out.append(("brightness", f"delta {d} clip {lo}", lambda dt, d=d, lo=lo, hi=hi: brightness_model(brightness_input(), d, lo, hi, dt)))
    for H, W in PIX_IMAGES:
        for s in PIX_SIDES:
            out.append(("pixelate", f"{H}x{W} s {s}", lambda dt, H=H, W=W, s=s: pixelate_model(image_input(PIX_BC + (H, W)), s, dt)))
    for n_cols, num_cat in TAB_LAYOUTS:
        for B in TAB_BATCHES:
            cat_len, std, fill = table_stats(n_cols, num_cat)
            out.append(("tab_noise", f"{n_cols}/{num_cat} B {B}", lambda dt, B=B, n=n_cols, k=num_cat, a=(cat_len, std, fill):
                        tab_model(table_input(B, n, k), k, a[0], table_columns(n)["all"], a[1], a[2], 0, TAB_STRENGTH[0], SEED, 3, dt)))
    return out
