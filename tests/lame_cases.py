"""Inputs and float64 restatement of csrc/stil_lame.h (LAME, Boudiaf et al., CVPR 2022; definition as recalled: unpinned), shared by
tests/test_gpu_lame.py and tests/test_lame_cpu.py.  The restatement is written from the definition, not from the kernels: plain torch
double, torch.sort(stable=True) for the ties.

The definition.  Inputs: logits Z [rows, K], features F [rows, D]; k >= 1, a kind, lambda >= 0, max_steps >= 1, tol >= 0.
  p = softmax(Z);  fhat_i = f_i / max(|f_i|, 1e-12);  d2_ij = max(0, 2 - 2 <fhat_i, fhat_j>);  k' = min(k, rows - 1)
  N_i = the k' indices j != i of smallest d2_ij, ascending; ties to the lower j; a NaN distance orders as +inf, after every finite one
  "knn": w_ij = 1 on N_i;  "rbf": w_ij = exp(-d2_ij / (2 s2)), s2 = mean_i d2(i, its k'-th neighbour), and 1 when s2 <= 1e-12
  A = (W + W^T) / 2;  u = log(p + 1e-10);  Y^0 = softmax(u);  Y^n_i = softmax(u_i + lambda sum_j A_ij Y^(n-1)_j)
  E_n = sum_ik Y^n_ik (-u_ik - lambda (A Y^(n-1))_ik + log max(Y^n_ik, 1e-20))
  stop after step n >= 2 when |E_n - E_(n-1)| <= tol |E_(n-1)| (tol = 0: never); steps = the steps performed; the scores are Y^steps
The two entry points meet at the float32 weights stil_lame_affinity writes: lame_ref64 rounds the weights once there, as the ABI does.
lambda and tol are float arguments of the ABI: the restatement takes their float32 values (f32)."""
import functools

import numpy as np
import torch

SHAPES = ((1, 3, 8), (2, 3, 8), (3, 2, 4), (6, 1, 4), (7, 5, 16), (33, 7, 24), (64, 10, 48), (65, 283, 96), (257, 5, 300))   # rows, K, D
SPECIAL = ((7, 5, 16), (33, 7, 24), (65, 283, 96))   # the shapes the tied / zero / nan features are run on
KINDS = ("knn", "rbf")
FKINDS = ("plain", "tied", "zero", "nan")
LAMS = (0.0, 1.0, 2.5)
STOPS = ((0.0, 7), (1e-8, 100))   # tol, max_steps
BAND = 0.05      # no energy ratio of a case lies within 5 % of tol
GAP = 1e-9       # no neighbour decision of a case hangs on a smaller d2 gap (exact ties, decided by the tie rule, apart)


def f32(x):
    return float(np.float32(x))


def ks_of(rows):
    """k in 1, 5, rows - 1 and one above rows"""
    return tuple(sorted({1, 5, rows + 3} | ({rows - 1} if rows >= 2 else set())))


# the seeds of rows_cases(): picked so that the BAND condition holds and the energy does not rise from step 2 on (a Jacobi update can
# oscillate, on a one-neighbour graph above all: tests/test_lame_cpu.py asserts both); every other case uses seed 0
SEEDS = {(3, 2, 4, "plain", 1, "rbf", 1.0, 0.0, 7): 2, (7, 5, 16, "plain", 1, "knn", 2.5, 0.0, 7): 1,
         (33, 7, 24, "plain", 1, "knn", 1.0, 1e-8, 100): 1, (257, 5, 300, "plain", 5, "rbf", 2.5, 1e-8, 100): 1,
         (7, 5, 16, "tied", 1, "knn", 1.0, 0.0, 7): 1, (65, 283, 96, "tied", 68, "rbf", 1.0, 1e-8, 100): 3}


def inputs(rows, K, D, fkind, seed=0):
    """-> Z [rows, K], F [rows, D] float32.  tied: every odd row's features duplicate the row before it; zero: one all-zero feature
    row; nan: one NaN feature"""
    g = torch.Generator().manual_seed(7919 * rows + 31 * K + D + 1000003 * seed)
    Z = (2.0 * torch.randn(rows, K, generator=g, dtype=torch.float64)).float()
    F = torch.randn(rows, D, generator=g, dtype=torch.float64).float()
    if fkind == "tied":
        F[1::2] = F[0::2][: F[1::2].shape[0]]
    elif fkind == "zero":
        F[rows // 2] = 0.0
    elif fkind == "nan":
        F[rows // 3, D // 2] = float("nan")
    else:
        assert fkind == "plain"
    return Z, F


def distances(F):
    """-> d2 [rows, rows] float64 (the diagonal is not used); a NaN stays a NaN"""
    F = F.double()
    nrm = F.pow(2).sum(1).sqrt()
    nrm = torch.where(nrm < 1e-12, torch.full_like(nrm, 1e-12), nrm)
    fhat = F / nrm[:, None]
    g = torch.stack([(fhat[i][None, :] * fhat).sum(1) for i in range(F.shape[0])])   # row by row: duplicated rows give the same bits
    d2 = 2.0 - 2.0 * g
    return torch.where(d2 < 0, torch.zeros_like(d2), d2)


def sorted_others(d2):
    """-> cols [rows, rows - 1] the j != i of every row in the order of the definition, keys [rows, rows - 1] their sort keys"""
    rows = d2.shape[0]
    idx = torch.arange(rows)
    cols = torch.stack([torch.cat((idx[:i], idx[i + 1:])) for i in range(rows)]) if rows > 1 else torch.zeros((1, 0), dtype=torch.long)
    key = torch.where(torch.isnan(d2), torch.full_like(d2, float("inf")), d2).gather(1, cols)
    skey, order = torch.sort(key, dim=1, stable=True)
    return cols.gather(1, order), skey


def check_gaps(F, fkind, k):
    """No neighbour decision of the features F at k hangs on a d2 gap below GAP: among the chosen ones and the first one left out of
    every row, consecutive sort keys are further apart, or exactly equal (which the tie rule decides; never on plain features)"""
    d2 = distances(F)
    rows = F.shape[0]
    kp = min(k, rows - 1)
    _, skey = sorted_others(d2)
    head = skey[:, : min(kp + 1, rows - 1)]
    if head.shape[1] < 2:
        return
    a, b = head[:, :-1], head[:, 1:]
    tie = a == b   # inf == inf included
    gap = torch.where(tie, torch.zeros_like(a), b - a)
    assert bool((tie | (gap > GAP)).all()), f"a neighbour decision hangs on a gap of {float(gap[~tie].min()):.3e}"
    if fkind == "plain":
        assert not bool(tie.any()), "plain features must not tie"


def affinity_ref64(F, k, kind):
    """-> dict(nbr [rows, k] int32 (-1: padding), wts [rows, k] float64 (0: padding), dk [rows] float64, s2, d2)"""
    assert kind in KINDS and k >= 1
    rows = F.shape[0]
    d2 = distances(F)
    kp = min(k, rows - 1)
    near = sorted_others(d2)[0][:, :kp]
    dn = d2.gather(1, near)
    dk = dn[:, kp - 1].clone() if kp > 0 else torch.zeros(rows, dtype=torch.float64)
    s2 = float(dk.mean())
    if kind == "knn" or s2 <= 1e-12:
        w = torch.ones_like(dn)
    else:
        w = torch.exp(-dn / (2.0 * s2))
    nbr = torch.full((rows, k), -1, dtype=torch.int32)
    wts = torch.zeros((rows, k), dtype=torch.float64)
    nbr[:, :kp] = near.int()
    wts[:, :kp] = w
    return dict(nbr=nbr, wts=wts, dk=dk, s2=s2, d2=d2)


def rows_ref64(Z, nbr, wts, lam, max_steps, tol):
    """-> dict(p, lse, Y [rows, K], energy [steps], steps, ratios [steps - 1] = |E_n - E_(n-1)| / |E_(n-1)|, A), all float64"""
    Z = Z.double()
    rows = Z.shape[0]
    lam, tol = f32(lam), f32(tol)
    lse = torch.logsumexp(Z, dim=1)
    p = torch.exp(Z - lse[:, None])
    W = torch.zeros((rows, rows), dtype=torch.float64)
    i, j = torch.arange(rows)[:, None].expand_as(nbr), nbr.long()
    live = (j >= 0) & (j < rows) & (j != i)
    W.index_put_((i[live], j[live]), wts.double()[live], accumulate=True)
    A = 0.5 * (W + W.T)
    u = torch.log(p + 1e-10)
    Y = torch.softmax(u, dim=1)
    energy, ratios = [], []
    for n in range(1, max_steps + 1):
        AY = A @ Y
        Y = torch.softmax(u + lam * AY, dim=1)
        energy.append(float((Y * (-u - lam * AY + torch.log(Y.clamp(min=1e-20)))).sum()))
        if n >= 2:
            d, e = abs(energy[-1] - energy[-2]), abs(energy[-2])
            ratios.append(d / e if e > 0 else (0.0 if d == 0 else float("inf")))
            if tol > 0 and d <= tol * e:
                break
    return dict(p=p, lse=lse, Y=Y, energy=torch.tensor(energy, dtype=torch.float64), steps=len(energy), ratios=ratios, A=A)


def lame_ref64(Z, F, k, kind, lam, max_steps, tol):
    """The whole definition: the affinity, its weights rounded to float32 (what stil_lame_affinity hands to stil_lame_rows), the
    iteration.  -> rows_ref64's dict plus nbr, wts (float64, before the rounding), dk"""
    a = affinity_ref64(F, k, kind)
    r = rows_ref64(Z, a["nbr"], a["wts"].float(), lam, max_steps, tol)
    r.update(nbr=a["nbr"], wts=a["wts"], dk=a["dk"])
    return r


def affinity_cases():
    """(rows, D, fkind, k, kind): every shape with plain features, the SPECIAL shapes with the three degenerate kinds too"""
    out = []
    for rows, K, D in SHAPES:
        for fkind in FKINDS if (rows, K, D) in SPECIAL else ("plain",):
            for k in ks_of(rows):
                for kind in KINDS:
                    out.append((rows, D, fkind, k, kind))
    return out


def rows_cases():
    """(rows, K, D, fkind, k, kind, lam, tol, max_steps): every shape at every lambda and both stopping modes on plain features, k and
    the kind cycling so that each shape meets every k and both kinds; the SPECIAL shapes on the degenerate features at both modes"""
    out = []
    for si, (rows, K, D) in enumerate(SHAPES):
        ks = ks_of(rows)
        for li, lam in enumerate(LAMS):
            for ti, (tol, steps) in enumerate(STOPS):
                out.append((rows, K, D, "plain", ks[(si + 2 * li + ti) % len(ks)], KINDS[(li + ti) % 2], lam, tol, steps))
    for si, (rows, K, D) in enumerate(SPECIAL):
        ks = ks_of(rows)
        for fi, fkind in enumerate(FKINDS[1:]):
            for ti, (tol, steps) in enumerate(STOPS):
                out.append((rows, K, D, fkind, ks[(si + fi + ti) % len(ks)], KINDS[(fi + ti) % 2], (1.0, 2.5)[(si + fi) % 2], tol, steps))
    return out


@functools.lru_cache(maxsize=None)
def affinity_case(rows, D, fkind, k, kind):
    """-> F, affinity_ref64's dict: computed once, shared, left unchanged"""
    _, F = inputs(rows, 3, D, fkind)
    return F, affinity_ref64(F, k, kind)


@functools.lru_cache(maxsize=None)
def rows_case(rows, K, D, fkind, k, kind, lam, tol, max_steps):
    """-> Z, F, lame_ref64's dict: computed once, shared, left unchanged"""
    Z, F = inputs(rows, K, D, fkind, SEEDS.get((rows, K, D, fkind, k, kind, lam, tol, max_steps), 0))
    return Z, F, lame_ref64(Z, F, k, kind, lam, max_steps, tol)


def band_clear(ratios, tol):
    """no ratio lies within BAND of tol: the stopping step is decided with margin"""
    t = f32(tol)
    return t == 0 or all(not (t * (1 - BAND) <= r <= t * (1 + BAND)) for r in ratios)


# ---- the reason the method exists: a class-ordered batch whose features know the classes better than the logits do
PROPERTY = dict(rows=48, classes=3, K=8, D=32, k=5, kind="knn", lam=1.0, max_steps=100, tol=1e-8, seed=0)
MARGIN = 1e-3        # rows whose top-two margin in the restatement's Y exceeds it have a decided argmax
MAX_EXCLUDED = 4     # that condition may exclude this many rows at most


def property_batch(seed=None):
    """-> Z [48, 8], F [48, 32] float32, y [48]: 16 consecutive rows of each of 3 of the 8 classes; the features are the class centre
    plus unit noise, the logits 2 onehot + 1.5 noise"""
    c = PROPERTY
    g = torch.Generator().manual_seed(104729 + (c["seed"] if seed is None else seed))
    centres = torch.randn(c["K"], c["D"], generator=g, dtype=torch.float64)
    classes = torch.randperm(c["K"], generator=g)[: c["classes"]]
    y = classes.repeat_interleave(c["rows"] // c["classes"])
    F = centres[y] + torch.randn(c["rows"], c["D"], generator=g, dtype=torch.float64)
    Z = 2.0 * torch.nn.functional.one_hot(y, c["K"]).double() + 1.5 * torch.randn(c["rows"], c["K"], generator=g, dtype=torch.float64)
    return Z.float(), F.float(), y


@functools.lru_cache(maxsize=None)
def property_ref(seed=None):
    c = PROPERTY
    Z, F, y = property_batch(seed)
    return Z, F, y, lame_ref64(Z, F, c["k"], c["kind"], c["lam"], c["max_steps"], c["tol"])
