"""A shifted test stream: the image corruptions and tabular shifts a test-time adaptation method is evaluated
against, applied on the device to batches that are already there, and the stream wrapper that makes a shifted sample a function of
(seed, position in the stream) only.

    stats = TableStats.from_table(train_table, field_lengths)            # once, on the SOURCE table
    spec = ShiftSpec(image=("gaussian_noise", 3), tabular=("tab_missing", 0.2), seed=7, stats=stats)
    fit.test(model, test_loader, ckpt, shift=spec)                       # or fit.test_shifts(model, loader, {name: spec, ...})

Image shifts (float32 [B, C, H, W] in the clip range, (0, 1) by default): gaussian_noise, impulse_noise, contrast, brightness,
gaussian_blur, pixelate.  Tabular shifts (float32 [B, n_cols], the categorical code columns first): tab_noise, tab_missing,
tab_cat_flip.  A shift is named (name, severity 1..5) or (name, strength as a float); SEVERITY holds the five strengths.

What is recalled, not pinned: the Gaussian, impulse, contrast, brightness and blur rows of SEVERITY are the ImageNet-C constants
(Hendrycks & Dietterich, ICLR 2019, "Benchmarking Neural Network Robustness to Common Corruptions and Perturbations") as recalled;
the paper's code is not available offline, so neither the constants nor its pixel formulas (its brightness goes through skimage's
HSV conversion, its contrast takes one mean per image, its blur is skimage's) are checked against it.  The definitions that hold
here are the ones csrc/stil_shift.h states.  The pixelate and tabular rows are this project's own.

Random numbers are counters, not state: element i of a call draws at counter offset + i of a 64-bit stream, ShiftStream keeps the
two offsets (image elements, table cells) as augment.TabularCorruptor keeps `drawn`, and the image stream is seeded with 2 seed,
the tabular one with 2 seed + 1.  So a stream cut into batches of 16 or of 8 yields the same samples bit for bit, and a new
ShiftStream of the same spec reproduces it.  One rank only: a multi-rank stream would need the global position of every sample.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import lib
from .ops import _chk, _p, _stream

IMAGE_SHIFTS = ("gaussian_noise", "impulse_noise", "contrast", "brightness", "gaussian_blur", "pixelate")
TABULAR_SHIFTS = ("tab_noise", "tab_missing", "tab_cat_flip")

SEVERITY = {
    "gaussian_noise": (0.08, 0.12, 0.18, 0.26, 0.38),     # sigma
    "impulse_noise": (0.03, 0.06, 0.09, 0.17, 0.27),      # fraction of elements set to lo or hi
    "contrast": (0.4, 0.3, 0.2, 0.1, 0.05),               # factor about the plane's mean
    "brightness": (0.1, 0.2, 0.3, 0.4, 0.5),              # delta of the HSV value
    "gaussian_blur": (1.0, 2.0, 3.0, 4.0, 6.0),           # sigma in pixels
    "pixelate": (2.0, 3.0, 4.0, 6.0, 8.0),                # block side s
    "tab_noise": (0.1, 0.25, 0.5, 1.0, 2.0),              # in standard deviations of the source column
    "tab_missing": (0.1, 0.2, 0.3, 0.5, 0.7),             # fraction of cells replaced by the source column's fill value
    "tab_cat_flip": (0.05, 0.1, 0.2, 0.3, 0.5),           # fraction of categorical cells redrawn uniformly
}
_UNIT = ("impulse_noise", "tab_missing", "tab_cat_flip")   # strengths that are probabilities
_TAB_KIND = {"tab_noise": 0, "tab_missing": 1, "tab_cat_flip": 2}
_MASK64 = (1 << 64) - 1


def resolve(shift, names: Sequence[str] = IMAGE_SHIFTS + TABULAR_SHIFTS) -> Tuple[str, float]:
    """(name, severity 1..5 as an int) or (name, strength as a float) -> (name, strength), validated."""
    if not (isinstance(shift, (tuple, list)) and len(shift) == 2):
        raise ValueError(f"a shift is (name, severity 1..5) or (name, strength as a float), got {shift!r}")
    name, level = shift
    if name not in names:
        raise ValueError(f"unknown shift {name!r}: one of {tuple(names)}")
    if isinstance(level, (bool, np.bool_)) or not isinstance(level, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name}: the level must be a severity 1..5 (int) or a strength (float), got {level!r}")
    if isinstance(level, (int, np.integer)):
        if not 1 <= int(level) <= 5:
            raise ValueError(f"{name}: severity {level} outside 1..5 (pass a float to name a strength)")
        return name, float(SEVERITY[name][int(level) - 1])
    s = float(level)
    if not math.isfinite(s):
        raise ValueError(f"{name}: strength {s} is not finite")
    if name == "pixelate":
        if s < 1 or s != int(s):
            raise ValueError(f"pixelate: block side s={s} must be a whole number >= 1")
    elif name != "brightness" and s < 0:
        raise ValueError(f"{name}: strength {s} is negative")
    if name in _UNIT and s > 1:
        raise ValueError(f"{name}: {s} is a fraction and cannot exceed 1")
    return name, s


def _clip(clip):
    if clip is None:
        return -math.inf, math.inf
    lo, hi = float(clip[0]), float(clip[1])
    if not lo <= hi:
        raise ValueError(f"clip range ({lo}, {hi}) is empty")
    return lo, hi


def _image(x: torch.Tensor, channels: Optional[int] = None) -> torch.Tensor:
    """validate an image batch -> an uninitialised tensor like it for the result"""
    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0):
        raise ValueError("image shifts take a non-empty float32 [B, C, H, W] tensor, got "
                         + (f"{x.dtype} {tuple(x.shape)}" if torch.is_tensor(x) else type(x).__name__))
    if channels is not None and x.shape[1] != channels:
        raise ValueError(f"this shift takes {channels} channels, got {x.shape[1]}")
    if not x.is_contiguous():
        raise ValueError("image shifts take contiguous tensors")
    _chk(x)
    return torch.empty_like(x)


def _counter(v, what):
    v = int(v)
    if v < 0:
        raise ValueError(f"{what}={v} is negative")
    return v & _MASK64


# ---------------------------------------------------------------------------------------------------- image shifts
def _noise(x, kind, strength, seed, offset, clip):
    lo, hi = _clip(clip)
    seed, offset = _counter(seed, "seed"), _counter(offset, "offset")
    out = _image(x)
    lib().shift_noise(_p(x), _p(out), x.numel(), kind, float(strength), lo, hi, seed, offset, _stream())
    return out


def gaussian_noise(x, sigma: float, seed: int = 0, offset: int = 0, clip=(0.0, 1.0)) -> torch.Tensor:
    """clip(x + sigma g): g the standard normal of the element's position in the stream (offset + its index in x)."""
    if not (math.isfinite(sigma) and sigma >= 0):
        raise ValueError(f"gaussian_noise: sigma={sigma} must be finite and non-negative")
    return _noise(x, 0, sigma, seed, offset, clip)


def impulse_noise(x, amount: float, seed: int = 0, offset: int = 0, clip=(0.0, 1.0)) -> torch.Tensor:
    """salt and pepper: a fraction amount / 2 of the elements becomes clip[0], as many clip[1]."""
    if not 0 <= amount <= 1:
        raise ValueError(f"impulse_noise: amount={amount} outside [0, 1]")
    if clip is None or not all(math.isfinite(float(c)) for c in clip):
        raise ValueError("impulse_noise writes the ends of the clip range: it needs a finite one")
    return _noise(x, 1, amount, seed, offset, clip)


def contrast(x, factor: float, clip=(0.0, 1.0), return_mean: bool = False):
    """clip((x - m) factor + m), m the mean of the element's [H, W] plane (float32 [B, C] with return_mean)."""
    if not (math.isfinite(factor) and factor >= 0):
        raise ValueError(f"contrast: factor={factor} must be finite and non-negative")
    lo, hi = _clip(clip)
    out = _image(x)
    B, C, H, W = x.shape
    mean = torch.empty((B, C), dtype=torch.float32, device=x.device)
    lib().shift_contrast(_p(x), _p(out), B, C, H * W, float(factor), lo, hi, _p(mean), _stream())
    return (out, mean) if return_mean else out


def brightness(x, delta: float, clip=(0.0, 1.0)) -> torch.Tensor:
    """the HSV value of every pixel moved by delta (and capped at clip[1]) at constant hue and saturation; 3 channels."""
    if not math.isfinite(delta):
        raise ValueError(f"brightness: delta={delta} is not finite")
    lo, hi = _clip(clip)
    out = _image(x, channels=3)
    B, C, H, W = x.shape
    lib().shift_brightness(_p(x), _p(out), B, C, H * W, float(delta), lo, hi, _stream())
    return out


def pixelate(x, s: int) -> torch.Tensor:
    """every s x s block (cut from the top-left) replaced by its mean."""
    if isinstance(s, bool) or s != int(s) or int(s) < 1:
        raise ValueError(f"pixelate: block side s={s} must be a whole number >= 1")
    out = _image(x)
    B, C, H, W = x.shape
    lib().shift_pixelate(_p(x), _p(out), B, C, H, W, int(min(int(s), max(H, W))), _stream())
    return out


def blur_ksize(sigma: float, H: int, W: int) -> int:
    """min(63, 2 ceil(4 sigma) + 1), reduced to the largest odd size whose radius is below min(H, W)"""
    k = min(63, 2 * int(math.ceil(4.0 * sigma)) + 1)
    return min(k, 2 * (min(H, W) - 1) + 1)


def gaussian_blur(x, sigma: float) -> torch.Tensor:
    """augment.gaussian_blur (separable, reflected borders) at one sigma for the batch, on a kernel that covers 4 sigma; 3 channels.
    A kernel of one tap (sigma = 0, or an image one pixel wide) copies."""
    if not (math.isfinite(sigma) and sigma >= 0):
        raise ValueError(f"gaussian_blur: sigma={sigma} must be finite and non-negative")
    _image(x, channels=3)         # validation only: the blur allocates its own output
    from . import augment
    B, _, H, W = x.shape
    k = blur_ksize(sigma, H, W)
    if k < 3 or sigma == 0:
        return x.clone()
    return augment.gaussian_blur(x, torch.full((B,), float(sigma), dtype=torch.float32, device=x.device), k)


def apply_image(name: str, strength: float, x, seed: int = 0, offset: int = 0, clip=(0.0, 1.0)) -> torch.Tensor:
    """one image shift by name at a strength (see resolve) on the elements offset .. offset + x.numel() of the stream"""
    if name == "gaussian_noise":
        return gaussian_noise(x, strength, seed, offset, clip)
    if name == "impulse_noise":
        return impulse_noise(x, strength, seed, offset, clip)
    if name == "contrast":
        return contrast(x, strength, clip)
    if name == "brightness":
        return brightness(x, strength, clip)
    if name == "gaussian_blur":
        return gaussian_blur(x, strength)
    if name == "pixelate":
        return pixelate(x, int(strength))
    raise ValueError(f"unknown image shift {name!r}: one of {IMAGE_SHIFTS}")


# ---------------------------------------------------------------------------------------------------- tabular shifts
class TableStats:
    """What the tabular shifts need to know of the SOURCE table, formed once: cat_len [num_cat] (codes per categorical column),
    col_std [n_cols] (population standard deviation), col_fill [n_cols] (the mean of a continuous column, the mode of a
    categorical one, the smallest code on ties).  Columns are laid out as TabEmbedFn takes them: categorical codes first."""

    def __init__(self, cat_len, col_std, col_fill):
        self.cat_len = torch.as_tensor(np.asarray(cat_len, dtype=np.int64).reshape(-1), dtype=torch.int32)
        self.col_std = torch.as_tensor(np.asarray(col_std, dtype=np.float64).reshape(-1), dtype=torch.float32)
        self.col_fill = torch.as_tensor(np.asarray(col_fill, dtype=np.float64).reshape(-1), dtype=torch.float32)
        self.num_cat, self.n_cols = int(self.cat_len.numel()), int(self.col_std.numel())
        if self.n_cols < 1 or self.col_fill.numel() != self.n_cols or self.num_cat > self.n_cols:
            raise ValueError(f"TableStats: {self.num_cat} categorical lengths, {self.n_cols} deviations, {self.col_fill.numel()} fill values")
        if self.num_cat and int(self.cat_len.min()) < 1:
            raise ValueError("TableStats: every categorical column has at least one code")
        if not bool(torch.isfinite(self.col_std).all() and (self.col_std >= 0).all() and torch.isfinite(self.col_fill).all()):
            raise ValueError("TableStats: deviations must be finite and non-negative, fill values finite")
        self._dev = {}

    @classmethod
    def from_table(cls, table, field_lengths) -> "TableStats":
        from .modules import split_field_lengths
        cat, con = split_field_lengths(field_lengths)
        t = np.asarray(torch.as_tensor(table).detach().cpu().double().numpy())
        if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] != len(cat) + len(con):
            raise ValueError(f"table {t.shape} does not have the {len(cat)} + {len(con)} columns of field_lengths")
        fill = t.mean(axis=0)
        for c, n in enumerate(cat):
            codes = t[:, c]
            if not bool(np.all((codes == np.floor(codes)) & (codes >= 0) & (codes < n))):
                raise ValueError(f"categorical column {c} holds values that are no codes in [0, {n})")
            fill[c] = float(np.argmax(np.bincount(codes.astype(np.int64), minlength=n)))   # first maximum: the smallest code on ties
        return cls(cat, t.std(axis=0), fill)

    def to(self, device):
        """(cat_len, col_std, col_fill) on `device`, uploaded once"""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = tuple(v.to(device).contiguous() for v in (self.cat_len, self.col_std, self.col_fill))
        return self._dev[key]


def column_mask(n_cols: int, columns=None) -> torch.Tensor:
    """uint8 [n_cols]: the columns in play (all of them for None)"""
    if columns is None:
        return torch.ones(n_cols, dtype=torch.uint8)
    cols = [int(c) for c in columns]
    if any(isinstance(c, bool) for c in columns) or any(not 0 <= c < n_cols for c in cols):
        raise ValueError(f"columns {list(columns)} outside [0, {n_cols})")
    on = torch.zeros(n_cols, dtype=torch.uint8)
    on[cols] = 1
    return on


def tab_shift(x, stats: TableStats, name: str, strength: float, seed: int = 0, offset: int = 0, col_on=None) -> torch.Tensor:
    """one tabular shift (TABULAR_SHIFTS) on the cells offset .. offset + x.numel() of the stream; col_on: uint8 [n_cols] on x's
    device (column_mask), None = every column."""
    if name not in _TAB_KIND:
        raise ValueError(f"unknown tabular shift {name!r}: one of {TABULAR_SHIFTS}")
    if not isinstance(stats, TableStats):
        raise ValueError("a tabular shift needs the source table's TableStats")
    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 2 and x.numel() > 0 and x.shape[1] == stats.n_cols):
        raise ValueError(f"tabular shifts take a non-empty float32 [B, {stats.n_cols}] tensor, got "
                         + (f"{x.dtype} {tuple(x.shape)}" if torch.is_tensor(x) else type(x).__name__))
    if not x.is_contiguous():
        raise ValueError("tabular shifts take contiguous tensors")
    if not (math.isfinite(strength) and strength >= 0) or (name in _UNIT and strength > 1):
        raise ValueError(f"{name}: strength {strength} outside {'[0, 1]' if name in _UNIT else '[0, inf)'}")
    if col_on is not None and not (torch.is_tensor(col_on) and col_on.dtype == torch.uint8 and col_on.shape == (stats.n_cols,)
                                   and col_on.device == x.device and col_on.is_contiguous()):
        raise ValueError(f"col_on must be a uint8 [{stats.n_cols}] tensor on x's device")
    seed, offset = _counter(seed, "seed"), _counter(offset, "offset")
    _chk(x)
    cat_len, col_std, col_fill = stats.to(x.device)
    col_on = column_mask(stats.n_cols).to(x.device) if col_on is None else col_on
    out = torch.empty_like(x)
    lib().shift_tab(_p(x), _p(out), x.shape[0], stats.n_cols, stats.num_cat, _p(cat_len) if stats.num_cat else None, _p(col_on), _p(col_std),
                    _p(col_fill), _TAB_KIND[name], float(strength), seed, offset, _stream())
    return out


# ---------------------------------------------------------------------------------------------------- the stream
class ShiftSpec:
    """One shifted domain: at most one image shift and one tabular shift, each (name, severity 1..5) or (name, strength as a float).
    columns: the tabular shift touches only these columns, the same ones for the whole stream (a failed sensor or field).
    clip: the image range, None = no clipping.  stats: the source table's TableStats, needed by a tabular shift."""

    def __init__(self, image=None, tabular=None, seed: int = 0, columns=None, clip=(0.0, 1.0), stats: Optional[TableStats] = None):
        self.image = None if image is None else resolve(image, IMAGE_SHIFTS)
        self.tabular = None if tabular is None else resolve(tabular, TABULAR_SHIFTS)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 63):
            raise ValueError(f"seed={seed!r} must be an integer in [0, 2^63)")
        self.seed = int(seed)
        self.clip = None if clip is None else _clip(clip)
        if self.image is not None and self.image[0] == "impulse_noise" and (self.clip is None or not all(math.isfinite(c) for c in self.clip)):
            raise ValueError("impulse_noise writes the ends of the clip range: it needs a finite one")
        if stats is not None and not isinstance(stats, TableStats):
            raise ValueError("stats must be a TableStats")
        if self.tabular is not None and stats is None:
            raise ValueError(f"the tabular shift {self.tabular[0]} needs stats (TableStats.from_table on the source table)")
        if columns is not None and self.tabular is None:
            raise ValueError("columns restrict a tabular shift, and none is given")
        self.stats = stats
        self.columns = None if columns is None else tuple(int(c) for c in columns)
        self.col_on = None if self.tabular is None else column_mask(stats.n_cols, columns)

    def __repr__(self):
        return f"ShiftSpec(image={self.image}, tabular={self.tabular}, seed={self.seed}, columns={self.columns}, clip={self.clip})"


class ShiftStream:
    """The spec applied to a stream of batches.  stream(batch) maps ((img, tab, ...), y, ...) to the same structure with the shifted
    image and table, everything else untouched, and advances the two counters (image elements, table cells) by B C H W and
    B n_cols, whatever the shift draws."""

    def __init__(self, spec: ShiftSpec):
        if not isinstance(spec, ShiftSpec):
            raise ValueError("ShiftStream takes a ShiftSpec")
        self.spec = spec
        self.image_drawn, self.table_drawn = 0, 0
        self._col_on = {}

    def __call__(self, batch):
        if not (isinstance(batch, (tuple, list)) and len(batch) >= 1 and isinstance(batch[0], (tuple, list)) and len(batch[0]) >= 2):
            raise ValueError("ShiftStream takes batches ((image, table, ...), y, ...)")
        sp = self.spec
        img, tab = batch[0][0], batch[0][1]
        new_img, new_tab = img, tab
        if sp.image is not None:
            new_img = apply_image(sp.image[0], sp.image[1], img, (2 * sp.seed) & _MASK64, self.image_drawn, sp.clip)
        if sp.tabular is not None:
            key = str(tab.device) if torch.is_tensor(tab) else None
            if key is not None and key not in self._col_on:
                self._col_on[key] = sp.col_on.to(tab.device)
            new_tab = tab_shift(tab, sp.stats, sp.tabular[0], sp.tabular[1], (2 * sp.seed + 1) & _MASK64, self.table_drawn, self._col_on.get(key))
        self.image_drawn += int(img.numel())
        self.table_drawn += int(tab.numel())
        x = type(batch[0])([new_img, new_tab, *batch[0][2:]])
        return type(batch)([x, *batch[1:]])


class ShiftedLoader:
    """`loader` under `spec`: every batch moved to `device` and shifted; each pass (__iter__) starts a fresh ShiftStream, so every
    pass over an unshuffled loader yields the same shifted samples."""

    def __init__(self, loader, spec: ShiftSpec, device="cuda"):
        if not isinstance(spec, ShiftSpec):
            raise ValueError("ShiftedLoader takes a ShiftSpec")
        self.loader, self.spec, self.device = loader, spec, device

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        from .fit import _to_device
        stream = ShiftStream(self.spec)
        for batch in self.loader:
            yield stream(_to_device(batch, self.device))


def class_ordered(labels, seed: int = 0) -> torch.Tensor:
    """The class-ordered stream: an index order (int64 [N], host) that sorts the samples by label, stably (samples of one class keep
    their order), the classes themselves in a random order drawn from `seed`.  Pass it to augment.IndexLoader(order=...)."""
    y = np.asarray(torch.as_tensor(labels).detach().cpu().numpy()).reshape(-1)
    classes = np.unique(y)
    perm = torch.randperm(len(classes), generator=torch.Generator().manual_seed(int(seed))).numpy()
    rank = np.empty(len(classes), dtype=np.int64)
    rank[perm] = np.arange(len(classes))             # classes[perm[0]] comes first
    return torch.from_numpy(np.argsort(rank[np.searchsorted(classes, y)], kind="stable").astype(np.int64))
