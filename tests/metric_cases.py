"""Cases, seeded inputs and references shared by tests/test_gpu_metric_kernels.py and tests/test_metric_cases_cpu.py (no test
lives here; nothing here needs a GPU).  The kernels are the ones every reported number comes out of (csrc/metrics.hip:
stil_metric_topk, stil_metric_binary, stil_auroc), the shapes their branch points: topk_hits_kernel runs one 64-lane wave per row
and four rows per block, binary_hits_kernel 256 rows per block, auroc_scan_kernel walks a class's N sorted flags 1024 at a time.

The references are written from the definitions, never from the kernels' algorithm, and they are exact:
  top-k     the target is in the top k when its position in torch.sort(row, descending=True, stable=True) (fp32, CPU) is < k:
            NaN ranks above every number, among equals the lower index is first;
  binary    (p > thr) == (y == 1) on fp32 values: a NaN score predicts 0, a label other than 1 is "not 1";
  AUROC     per class by pairs, U2 = 2 #(s+ > s-) + #(s+ == s-) over all positive / negative pairs (fp32 comparisons, Python
            integers, no sort and no search), value = fp32(U2 / (2.0 n_pos n_neg)), 0 when a side is empty; macro = the float64 sum
            of the fp32 per-class values in class order, over K, rounded once to fp32.  These are the IEEE operations of
            auroc_u_kernel / auroc_macro_kernel and the build has no fast-math: the device has to equal them bit for bit.
            A label outside [0, K) is a negative for every class; in the binary task (K = 1) so is every label other than 1.
A NaN among AUROC scores is out of contract (include/stil_hip.h); `auroc_nan_column_case` holds what is pinned about it."""
import functools
from collections import namedtuple

import numpy as np
import torch

from kernel_edge_cases import NAN, SENT, TIE_PLACEMENTS, gen  # noqa: F401  (one sentinel, one seed rule, one pair of tie placements for the suite)

INF = float("inf")
SUB = float(np.float32(1e-45))          # the smallest fp32 subnormal
FMAX = float(np.finfo(np.float32).max)
WAVE, TOPK_ROWS, BIN_BLOCK, SCAN_TRIP = 64, 4, 256, 1024      # lanes per row / rows per block / rows per block / flags per trip
BAD_LABELS = (-1, None, 2 ** 40)        # None: K in the multiclass task, 2 in the binary one


# =====================================================================================================================
# AUROC
# =====================================================================================================================
Auroc = namedtuple("Auroc", "N K kind layout pad")
AUROC_NS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
AUROC_KS = (1, 2, 3, 5)
AUROC_KINDS = ("softmax", "logits", "tied", "two", "const", "specials")
AUROC_LAYOUTS = ("random", "one_pos", "one_neg", "absent", "one_class", "bad_labels")
AUROC_WIDE = Auroc(300, 286, "softmax", "random", 3)            # ld = K + 3, the padding holds NaN
SPECIALS = (0.0, -0.0, INF, -INF, SUB, -SUB, FMAX, -FMAX)


def _auroc_table():
    combos = [(k, l) for k in AUROC_KINDS for l in AUROC_LAYOUTS]
    shapes = [(N, K) for N in AUROC_NS for K in AUROC_KS]
    # every (N, K) once, walking through every (kind, layout) pair (60 shapes, 36 pairs, step 7 is coprime to 36)
    t = [Auroc(N, K, *combos[(7 * i) % len(combos)], 0) for i, (N, K) in enumerate(shapes)]
    # every kind on columns longer than one, two and three trips of the scan; every layout within one trip and beyond it
    t += [Auroc(N, 3, kind, "random", 0) for N in (1025, 2049, 3073) for kind in AUROC_KINDS]
    t += [Auroc(N, K, "tied", lay, 0) for N in (65, 1025) for K in (1, 5) for lay in AUROC_LAYOUTS]
    t += [Auroc(N, 2, "specials", lay, 0) for N in (257, 1025) for lay in AUROC_LAYOUTS]
    t.append(AUROC_WIDE)
    return tuple(dict.fromkeys(t))


AUROC_TABLE = _auroc_table()


def auroc_id(c):
    return f"N{c.N}_K{c.K}_{c.kind}_{c.layout}" + (f"_ld{c.K + c.pad}" if c.pad else "")


def _labels(c, g):
    """[N] int64.  Multiclass: "one_pos" class 0 has one positive; "one_neg" class 0 has one negative; "absent" class K - 1 has
    no row (K >= 2); "one_class" every row is class K - 1; "bad_labels" every fourth row holds -1, K or 2^40.  Binary: the same
    about label 1 ("absent": no positive; "one_class": no negative; bad labels -1, 2, 2^40)."""
    N, K = c.N, c.K
    hi = 2 if K == 1 else K
    y = torch.randint(0, hi, (N,), generator=g)
    where = int(torch.randint(0, N, (1,), generator=g))
    one = 1 if K == 1 else 0                                   # the class the "one_*" layouts are about
    if c.layout == "one_pos":
        y = torch.zeros(N, dtype=torch.int64) if K == 1 else torch.randint(1, K, (N,), generator=g)
        y[where] = one
    elif c.layout == "one_neg":
        y = torch.full((N,), one, dtype=torch.int64)
        y[where] = 0 if K == 1 else 1 + where % (K - 1)
    elif c.layout == "absent":
        y = torch.zeros(N, dtype=torch.int64) if K == 1 else torch.randint(0, K - 1, (N,), generator=g)
    elif c.layout == "one_class":
        y = torch.full((N,), hi - 1, dtype=torch.int64)
    elif c.layout == "bad_labels":
        bad = torch.tensor([hi if b is None else b for b in BAD_LABELS])
        rows = torch.arange(N)
        y = torch.where(rows % 4 == 1, bad[(rows // 4) % 3], y)
    return y


def _scores(c, g):
    N, K = c.N, c.K
    r = torch.randn(N, K, generator=g)
    if c.kind == "softmax":
        return torch.sigmoid(2.0 * r) if K == 1 else torch.softmax(2.0 * r, 1)
    if c.kind == "logits":
        return 3.0 * r
    if c.kind == "tied":
        t = torch.round(3.0 * r * 10.0) / 10.0                 # one decimal: many ties; +0.0 and -0.0 both, rows 0 and 1 at the least
        t[:2] = torch.tensor([[0.0], [-0.0]])[:min(N, 2)]
        return t
    if c.kind == "two":
        return torch.where(r > 0, 1.0, -1.0)
    if c.kind == "const":
        return torch.full((N, K), 0.25)
    assert c.kind == "specials"
    pool = torch.tensor(SPECIALS)
    pick = torch.randint(0, len(SPECIALS), (N, K), generator=g)
    return torch.where(torch.rand(N, K, generator=g) < 0.6, pool[pick], torch.round(r * 10.0) / 10.0)


def positives(y, K):
    """[N, K] bool: row i is a positive of class c"""
    y = np.asarray(y, dtype=np.int64)
    return (y == 1)[:, None] if K == 1 else y[:, None] == np.arange(K)[None, :]


@functools.lru_cache(maxsize=None)
def auroc_case(c):
    """-> (scores [N, K + pad] fp32 with NaN in the padding, labels [N] int64), both torch CPU tensors.  "specials" columns get
    +0.0 and -0.0 on two positives and on two negatives of every class that has them."""
    g = gen(c.N, c.K, AUROC_KINDS.index(c.kind), AUROC_LAYOUTS.index(c.layout), 83)
    y = _labels(c, g)
    s = _scores(c, g).to(torch.float32)
    if c.kind == "specials":
        pos = positives(y.numpy(), c.K)
        for k in range(c.K):
            for rows in (np.flatnonzero(pos[:, k])[:2], np.flatnonzero(~pos[:, k])[:2]):
                for r, z in zip(rows, (0.0, -0.0)):
                    s[int(r), k] = z
    if c.pad:
        s = torch.cat([s, torch.full((c.N, c.pad), NAN)], 1)
    return s, y


def auroc_reference(s, y, K):
    """-> (per [K] fp32, macro fp32 scalar, U2 [K] Python ints, n_pos [K], n_neg [K]) by pairs, on the first K columns of s"""
    s = np.asarray(s, dtype=np.float32)[:, :K]
    pos = positives(y, K)
    per, u2s, nps, nns = np.zeros(K, dtype=np.float32), [], [], []
    for k in range(K):
        sp, sn = s[pos[:, k], k], s[~pos[:, k], k]
        n_pos, n_neg = int(sp.size), int(sn.size)
        u2 = 2 * int((sp[:, None] > sn[None, :]).sum(dtype=np.int64)) + int((sp[:, None] == sn[None, :]).sum(dtype=np.int64))
        per[k] = np.float32(u2 / (2.0 * n_pos * n_neg)) if n_pos and n_neg else np.float32(0)
        u2s.append(u2); nps.append(n_pos); nns.append(n_neg)
    total = 0.0
    for k in range(K):
        total += float(per[k])
    return per, np.float32(total / K), u2s, nps, nns


@functools.lru_cache(maxsize=None)
def auroc_expected(c):
    s, y = auroc_case(c)
    return auroc_reference(s.numpy(), y.numpy(), c.K)


AUROC_NAN_SHAPE, AUROC_NAN_COLUMN = (300, 3), 1


@functools.lru_cache(maxsize=None)
def auroc_nan_column_case():
    """-> (scores with NaN on every third row of column 1, the same scores with numbers there, labels).  Out of contract; pinned
    only: the call returns, the other classes' values are the bit patterns they have without the NaNs, the sentinels stand."""
    N, K = AUROC_NAN_SHAPE
    g = gen(N, K, 89)
    clean = (torch.round(3.0 * torch.randn(N, K, generator=g) * 10.0) / 10.0).to(torch.float32)
    y = torch.randint(0, K, (N,), generator=g)
    dirty = clean.clone()
    dirty[::3, AUROC_NAN_COLUMN] = NAN
    return dirty, clean, y


# =====================================================================================================================
# top-k
# =====================================================================================================================
Topk = namedtuple("Topk", "name N K pad fill")
TOPK_KS = (1, 2, 63, 64, 65, 129, 286, 1000)
TOPK_NS = (1, 3, 4, 5, 257)
TOPK_K_SMALL = (1, 2, 5)                 # and k = K
TOPK_BAD_TARGETS = (-1, None, 2 ** 40, -2 ** 63)    # None: K
TOPK_PAD = 5
TIE_K = 130
NAN_KS = (3, 65, 130)
NAN_PLACEMENTS = ("all", "at_target", "below_target", "above_target", "around_target")

TOPK_GRID = tuple(Topk(f"grid_K{K}_N{N}", N, K, 0, None) for K in TOPK_KS for N in TOPK_NS)
TOPK_PLANTED = (Topk("ties", None, TIE_K, 0, None), Topk("zeros", None, TIE_K, 0, None), Topk("infs", None, TIE_K, 0, None),
                Topk("bad_targets", None, 5, 0, None), Topk("ld_nan", 37, 65, TOPK_PAD, NAN), Topk("ld_inf", 37, 65, TOPK_PAD, INF))
TOPK_NAN = tuple(Topk(f"nan_K{K}", None, K, 0, None) for K in NAN_KS)
TOPK_TABLE = TOPK_GRID + TOPK_PLANTED + TOPK_NAN
TOPK_BY_NAME = {c.name: c for c in TOPK_TABLE}


def topk_ks(c):
    return tuple(dict.fromkeys(TOPK_K_SMALL + (c.K,)))


def _signed_tenths(g, *shape):
    return (torch.round(torch.randn(*shape, generator=g) * 10.0) / 10.0).to(torch.float32)


def tie_rows(K=TIE_K):
    """[(row [K], target, what)]: the row's maximum sits at two columns -- in two lanes of the wave, or in one lane on two trips
    of the K loop (kernel_edge_cases.TIE_PLACEMENTS) -- and the target is the first of them, the second, or neither."""
    g = gen(K, 97)
    out = []
    for a, b in TIE_PLACEMENTS:
        for t, what in ((a, "first"), (b, "second"), (b + 1, "neither")):
            r = _signed_tenths(g, K).clamp(-3.0, 3.0)
            r[a] = r[b] = 4.0
            out.append((r, t, ("lane" if (b - a) % WAVE == 0 else "lanes", what)))
    return out


def _planted(c):
    K = c.K
    g = gen(K, len(c.name), 101)
    rows, tg = [], []
    if c.name == "ties":
        for r, t, _ in tie_rows(K):
            rows.append(r); tg.append(t)
    elif c.name == "zeros":          # +0.0 and -0.0 tie: the lower index is first, whichever sign it carries
        for a, b in TIE_PLACEMENTS:
            for za, zb in ((0.0, -0.0), (-0.0, 0.0)):
                for t in (a, b, b + 1):
                    r = -1.0 - torch.rand(K, generator=g)
                    r[a], r[b] = za, zb
                    rows.append(r); tg.append(t)
    elif c.name == "infs":
        for a, b in TIE_PLACEMENTS:
            for top, low in ((INF, -INF), (INF, 0.5), (4.0, -INF)):
                for t in (a, b, b + 1, 0):
                    r = _signed_tenths(g, K).clamp(-3.0, 3.0)
                    r[a] = r[b] = top
                    r[0] = r[b + 1] = low
                    rows.append(r); tg.append(t)
    elif c.name == "bad_targets":
        bad = [K if b is None else b for b in TOPK_BAD_TARGETS]
        tg = [0, bad[0], 4, bad[1], bad[2], 2, bad[3], 1, 3]
        rows = list(_signed_tenths(g, len(tg), K))
    else:
        raise KeyError(c.name)
    return torch.stack(rows).to(torch.float32), torch.tensor(tg, dtype=torch.int64)


def nan_rows(K):
    """[(row [K], target, placement)] for every NAN_PLACEMENTS entry at targets in the first trip and (K > 64) beyond it;
    "below" / "above" are about the index: a NaN at a lower index than the target, at a higher one, one on each side"""
    g = gen(K, 103)
    out = []
    for t in sorted({0, 1, K // 2, K - 1} & set(range(K))):
        for place in NAN_PLACEMENTS:
            r = _signed_tenths(g, K)
            r[t] = 5.0                                          # the target leads every number of its row
            if place == "all":
                r[:] = NAN
            elif place == "at_target":
                r[t] = NAN
            elif place == "below_target":
                if t == 0:
                    continue
                r[t - 1 if t % 2 else 0] = NAN
            elif place == "above_target":
                if t == K - 1:
                    continue
                r[K - 1 if t % 2 else t + 1] = NAN
            else:
                if t == 0 or t == K - 1:
                    continue
                r[0] = r[K - 1] = NAN
            out.append((r, t, place))
    # a NaN target among other NaNs: beaten by the NaNs at lower indices only
    if K >= 3:
        r = _signed_tenths(g, K)
        r[0] = r[K // 2] = r[K - 1] = NAN
        out += [(r, 0, "nan_target_first"), (r, K // 2, "nan_target_second"), (r, K - 1, "nan_target_third")]
    return out


@functools.lru_cache(maxsize=None)
def topk_case(c):
    """-> (scores [N, K + pad] fp32, targets [N] int64).  The grid: signed logits rounded to one decimal, targets in [0, K)."""
    if c.name.startswith("grid") or c.pad:
        g = gen(c.N, c.K, c.pad, 107)
        s, y = _signed_tenths(g, c.N, c.K), torch.randint(0, c.K, (c.N,), generator=g)
    elif c.name.startswith("nan"):
        rows = nan_rows(c.K)
        s, y = torch.stack([r for r, _, _ in rows]), torch.tensor([t for _, t, _ in rows], dtype=torch.int64)
    else:
        s, y = _planted(c)
    if c.pad:
        s = torch.cat([s, torch.full((s.shape[0], c.pad), c.fill)], 1)
    return s, y


def topk_reference(s, y, K, k):
    """-> [N] bool hits.  A target outside [0, K) is no hit (its row still counts as a sample)."""
    s = torch.as_tensor(s, dtype=torch.float32)[:, :K]
    y = torch.as_tensor(y, dtype=torch.int64)
    order = torch.sort(s, dim=1, descending=True, stable=True).indices
    valid = (y >= 0) & (y < K)
    pos = (order == torch.where(valid, y, torch.zeros_like(y))[:, None]).to(torch.int64).argmax(1)
    return valid & (pos < k)


def topk_parent_rule(s, y, K, k):
    """the expression this kernel and oracle/metrics_oracle.py carried before NaN was ranked: beat = (v > st) | (v == st & j < t).
    Kept to show which cases tell the two apart (tests/test_metric_cases_cpu.py); nothing is compared with it on the GPU."""
    s = np.asarray(s, dtype=np.float32)[:, :K]
    y = np.asarray(y, dtype=np.int64)
    valid = (y >= 0) & (y < K)
    t = np.where(valid, y, 0)
    st = s[np.arange(s.shape[0]), t][:, None]
    with np.errstate(invalid="ignore"):
        beat = ((s > st) | ((s == st) & (np.arange(K)[None, :] < t[:, None]))).sum(1)
    return torch.from_numpy(valid & (beat < k))


# =====================================================================================================================
# binary accuracy
# =====================================================================================================================
Binary = namedtuple("Binary", "N thr")
BINARY_NS = (1, 63, 64, 65, 255, 256, 257, 513)
BINARY_THRS = (0.5, 0.0)
BINARY_LABELS = (0, 1, 2, -1)
BINARY_TABLE = tuple(Binary(N, thr) for N in BINARY_NS for thr in BINARY_THRS)


def binary_planted(thr):
    t = np.float32(thr)
    return (float(t), float(np.nextafter(t, np.float32(1))), float(np.nextafter(t, np.float32(-1))), 0.0, -0.0, NAN, INF, -INF)


@functools.lru_cache(maxsize=None)
def binary_case(c):
    """-> (scores [N] fp32, labels [N] int64): the planted values (at the threshold, one ulp either side, both zeros, NaN, both
    infinities) on two rows of every three, each under every label of {0, 1, 2, -1}; the rest random on both sides."""
    g = gen(c.N, int(c.thr * 2), 109)
    p = torch.rand(c.N, generator=g) + (c.thr - 0.5)
    rows = torch.arange(c.N)
    planted = torch.tensor(binary_planted(c.thr))
    nth = rows - rows // 3                                      # the ordinal of a planted row among the planted ones
    p = torch.where(rows % 3 != 2, planted[nth % len(planted)], p).to(torch.float32)
    y = torch.tensor(BINARY_LABELS)[torch.where(rows % 3 != 2, nth // len(planted), rows) % 4]
    return p, y


def binary_reference(p, y, thr):
    """-> [N] bool hits"""
    p, y = np.asarray(p, dtype=np.float32), np.asarray(y, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        return (p > np.float32(thr)) == (y == 1)


# =====================================================================================================================
# what the tables reach
# =====================================================================================================================
def coverage_gaps(auroc=AUROC_TABLE, topk=TOPK_TABLE, binary=BINARY_TABLE, ties=None):
    """the named branch points no case crosses, computed from the case data"""
    ties = [what for c in topk if c.name == "ties" for _, _, what in tie_rows(c.K)] if ties is None else ties
    shapes = [tuple(topk_case(c)[0].shape) for c in topk]
    checks = (
        ("auroc", "second trip of the scan", any(c.N > SCAN_TRIP for c in auroc)),
        ("auroc", "a scan of full trips only", any(c.N > SCAN_TRIP and c.N % SCAN_TRIP == 0 for c in auroc)),
        ("auroc", "two-valued column beyond one trip", any(c.N > SCAN_TRIP and c.kind == "two" for c in auroc)),
        ("auroc", "ld > K", any(c.pad for c in auroc)),
        ("topk", "second trip of the K loop", any(c.K > WAVE for c in topk)),
        ("topk", "row not in wave 0 of its block", any(n > 1 for n, _ in shapes)),
        ("topk", "partial last block", any(n > TOPK_ROWS and n % TOPK_ROWS for n, _ in shapes)),
        ("topk", "more than one block", any(n > TOPK_ROWS for n, _ in shapes)),
        ("topk", "tie within a lane", any(w[0] == "lane" for w in ties)),
        ("topk", "tie across lanes", any(w[0] == "lanes" for w in ties)),
        ("topk", "ld > K", any(c.pad for c in topk)),
        ("binary", "partial last block", any(c.N > BIN_BLOCK and c.N % BIN_BLOCK for c in binary)),
        ("binary", "row not in wave 0 of its block", any(c.N > WAVE for c in binary)),
        ("binary", "a full block", any(c.N % BIN_BLOCK == 0 for c in binary)),
    )
    gaps = [(f, what) for f, what, ok in checks if not ok]
    gaps += [("auroc", f"kind {k}") for k in AUROC_KINDS if k not in {c.kind for c in auroc}]
    gaps += [("auroc", f"layout {l}") for l in AUROC_LAYOUTS if l not in {c.layout for c in auroc}]
    gaps += [("topk", f"tie target {w}") for w in ("first", "second", "neither") if w not in {x[1] for x in ties}]
    return gaps
