"""Cases, seeded inputs and references shared by tests/test_gpu_match_kernels.py and tests/test_match_cases_cpu.py (no test lives
here; nothing here needs a GPU).  The kernels are the four that carry the unsupervised loss of the Match baselines
(csrc/loss.hip: stil_contrast_graph, stil_simmatch_unfold, stil_freematch_update, stil_freematch_entropy).  Each runs one
workgroup per row, or one workgroup in all, with 256 threads striding N, R or K: the shapes below sit at 1, 2, 255 / 256 / 257,
past 256, and at the widest the baselines use.

References are the operation written from the reference project's definition (models/MatchModel/CoMatch.py:100-110,
simmatch_model.py:270-282, FreeMatchFolder/freematch_model.py:128-165, freematch_utils.py:17-45) with torch ops in a chosen
dtype -- float64 is the reference, float32 (ATen on the CPU) the yardstick: the CPU test asserts that fp32 ATen meets, against
float64, the very checks the GPU test applies to the kernel.  Scalars a kernel receives as `float` (threshold, c_smooth,
momentum, inv_rows) and the kernels' own 1e-7f / 1e-12f are rounded to fp32 before the float64 reference uses them, so the
reference states the kernel's problem and not a nearby one.  Discrete outputs (argmax, masks, edges) are planted, never read
off a reference: the top-1 column of every row is chosen here, ties are exact in fp32 and the first index wins."""
import functools

import numpy as np
import torch

from kernel_edge_cases import MIN_GAP, NAN, SENT, f32, gen  # noqa: F401  (one gap, one sentinel, one seed rule for the suite)

EPS_CONTRAST = 1e-7             # log(p + 1e-7f) in contrast_graph_kernel
EPS_ENTROPY = 1e-12             # log(v + 1e-12f) in freematch_entropy_kernel
PAD = 3                         # leading dimensions N + PAD, margins of PAD rows


# =====================================================================================================================
# stil_contrast_graph
# =====================================================================================================================
CONTRAST_TH = 0.7
CONTRAST_NS = (1, 2, 255, 256, 257, 513, 2597)
CONTRAST_BIG = (37, 2597)
CONTRAST_TABLE = tuple((rows, N) for N in CONTRAST_NS[:-1] for rows in (1, 3)) + (CONTRAST_BIG,)
CONTRAST_INV_ROWS = (None, 0.25)                        # None: 1 / rows, the mean the baselines take
CONTRAST_NO_EDGE = (3, 257, 1.5)                        # rows, N, threshold > 1: no row has an edge
_ROW1_KIND = {1: "diag", 2: "th", 255: "all", 256: "th", 257: "sat", 513: "rand"}
_BIG_KINDS = ("rand", "diag", "all", "th", "sat", "eps")
EPS_ROW_EDGES = 20                                      # edges of an "eps" row beside its diagonal


def contrast_kinds(rows, N):
    """the planted kind of every row: "diag" (the only edge is the diagonal), "all" (every entry is an edge), "th" (entries at
    fp32(th) -- edges -- and at the next float below -- none), "sat" (one S = 5, the rest -5), "eps" (edges at S = -5 among
    S = 5: p < 1e-7 on every edge), "rand" """
    if (rows, N) == CONTRAST_BIG:
        return [_BIG_KINDS[r % len(_BIG_KINDS)] for r in range(rows)]
    if rows == 1:
        return [_ROW1_KIND[N]]
    return ["th", "diag" if N % 2 else "all", "sat"][:rows]


@functools.lru_cache(maxsize=None)
def contrast_case(rows, N):
    """-> dict: S [rows, N] in [-5, 5] (a cosine over T = 0.2), Q [rows, N] in [0, 1] with Q[r, r % N] = 1 (the diagonal, where
    the width has one), the threshold, the kinds, and the planted truth: `edges` (Q >= fp32(th)), `at_th` / `below` (the
    entries equal to fp32(th) / to the next float towards 0).  Off the planted entries Q keeps 0.05 away from the threshold."""
    g = gen(rows, N, 61)
    th32 = np.float32(CONTRAST_TH)
    below32 = np.nextafter(th32, np.float32(0))
    r01 = lambda *s: torch.rand(*s, generator=g)
    S = 10.0 * r01(rows, N) - 5.0
    Q = torch.where(r01(rows, N) < 0.3, 0.75 + 0.25 * r01(rows, N), 0.65 * r01(rows, N))
    kinds = contrast_kinds(rows, N)
    cols = torch.arange(N)
    for r, kind in enumerate(kinds):
        d = r % N
        if kind == "diag":
            Q[r] = 0.65 * r01(N)
        elif kind == "all":
            Q[r] = 0.75 + 0.25 * r01(N)
        elif kind == "th":
            phase = (cols - d) % 4
            Q[r][phase == 1] = float(th32)
            Q[r][phase == 2] = float(below32)
        elif kind == "sat":
            S[r] = -5.0
            S[r, (d + 1) % N] = 5.0
        elif kind == "eps":
            e = torch.zeros(N, dtype=torch.bool)
            e[(d + 1 + 123 * torch.arange(EPS_ROW_EDGES)) % N] = True
            e[d] = True
            Q[r] = torch.where(e, 0.75 + 0.25 * r01(N), 0.65 * r01(N))
            S[r] = torch.where(e, torch.tensor(-5.0), torch.tensor(5.0))
        Q[r, d] = 1.0
    t32 = torch.tensor(float(th32))
    return dict(rows=rows, N=N, S=S, Q=Q, th=CONTRAST_TH, kinds=kinds, edges=Q >= t32, at_th=Q == t32, below=Q == torch.tensor(float(below32)))


def contrast_reference(S, Q, th, inv_rows, dtype):
    """CoMatch.py:100-110 on S = log(sim): the edges are Q >= th, w = Q on the edges over its row sum, p = exp(S) on the edges
    over the whole row's sum, row_loss = -sum(log(p + 1e-7) w) over the edges; dS = d(inv_rows * sum(row_loss)) / dS.
    A row without an edge gives 0 / 0 there; the kernel's 0 is pinned apart (CONTRAST_NO_EDGE)."""
    th, eps, inv = f32(th), f32(EPS_CONTRAST), f32(inv_rows)
    s, q = S.detach().clone().to(dtype).requires_grad_(), Q.to(dtype)
    sim = torch.exp(s)
    pos = (q >= th).to(dtype)
    w = q * pos
    w = w / w.sum(1, keepdim=True)
    p = sim * pos / sim.sum(1, keepdim=True)
    row_loss = -(torch.log(p + eps) * pos * w).sum(1)
    (dS,) = torch.autograd.grad(row_loss.sum() * inv, s)
    return {"row_loss": row_loss.detach(), "dS": dS, "p": p.detach(), "mean": row_loss.detach().mean()}


# =====================================================================================================================
# stil_simmatch_unfold
# =====================================================================================================================
UNFOLD_TABLE = ((1, 1, 1), (3, 2, 2), (5, 255, 5), (5, 256, 5), (5, 257, 5), (2, 1025, 286), (2, 600, 1000))
UNFOLD_CS = (0.0, 0.9, 1.0)
UNFOLD_ONE_CLASS = (3, 2, 2)                            # every bank entry carries the same class here


@functools.lru_cache(maxsize=None)
def unfold_case(R, N, K):
    """-> tpo [R, N] (a softmax over the bank), probs [R, K] (a softmax over the classes), labels [N] int64 in [0, K): class
    K - 1 occurs, class 0 has no bank entry wherever K > 1."""
    g = gen(R, N, K, 67)
    tpo = (2.0 * torch.randn(R, N, generator=g)).softmax(1)
    probs = torch.randn(R, K, generator=g).softmax(1)
    labels = torch.zeros(N, dtype=torch.int64) if K == 1 else torch.randint(1, K, (N,), generator=g)
    labels[0] = K - 1
    return tpo, probs, labels


def unfold_reference(tpo, probs, labels, c_smooth, dtype):
    """simmatch_model.py:270-282: teacher = tpo * probs[:, labels] over its row sum; pseudo = probs * c + agg * (1 - c) with
    agg[r, k] = the sum of tpo[r, j] over the bank entries of class k, or probs itself from c = 1 on"""
    c = f32(c_smooth)
    R, K = probs.shape
    t, p, lab = tpo.to(dtype), probs.to(dtype), labels.expand(R, -1)
    teacher = t * p.gather(1, lab)
    teacher = teacher / teacher.sum(1, keepdim=True)
    agg = torch.zeros(R, K, dtype=dtype).scatter_add(1, lab, t)
    return {"teacher": teacher, "pseudo": p * c + agg * (1.0 - c) if c < 1.0 else p, "agg": agg}


# =====================================================================================================================
# stil_freematch_update
# =====================================================================================================================
UPDATE_TABLE = ((1, 1), (1, 5), (2, 2), (255, 3), (256, 3), (257, 3), (300, 286), (40, 1000))
UPDATE_MOMENTA = (0.999, 0.0, 1.0)
UPDATE_TIME_P = 0.75
UPDATE_CALLS = 2
UPDATE_MAX_TRIES = 50


def update_tie_rows(R, K):
    if K < 2 or R < 2:
        return []
    return [1] if R < 255 else [1, 100, R - 1]


def _plant_probs(g, R, K):
    """-> (probs [R, K] fp32, top [R] int64, ties [(row, c0, c1)]).  Probabilities are planted, not pushed through a softmax:
    row r holds v in [0.55, 0.95] at column (7 (r // 2) + 3) % K (two rows a column:
    with momentum 0 a row then falls below a threshold its neighbour raised) over a background that sums to 1 - v (so top-1 leads top-2 by 0.1 at
    the least); a tie row holds the same float at two columns (0.5 each at K = 2, else 0.45 over a background of 0.1)."""
    v = 0.55 + 0.4 * torch.rand(R, generator=g)
    top = (7 * (torch.arange(R) // 2) + 3) % K
    if K == 1:
        return torch.ones(R, 1), top, []
    rows = torch.arange(R)
    bg = torch.randn(R, K, generator=g).softmax(1)
    bg[rows, top] = 0.0
    p = bg * ((1.0 - v) / bg.sum(1))[:, None]
    p[rows, top] = v
    ties = []
    for t in update_tie_rows(R, K):
        a = int(top[t])
        b = (a + 1 + t % (K - 1)) % K
        c0, c1 = min(a, b), max(a, b)
        rest = torch.rand(K, generator=g) + 0.1
        rest[[c0, c1]] = 0.0
        p[t] = rest * (0.1 / float(rest.sum())) if K > 2 else rest
        p[t, c0] = p[t, c1] = 0.5 if K == 2 else 0.45
        top[t] = c0
        ties.append((t, c0, c1))
    return p, top, ties


def update_at_threshold(R, momentum):
    """momentum 0 on one row: the new time_p IS the row's maximum and p_model[idx] / max(p_model) is 1, so the row sits exactly
    on its threshold (mask 1: `>=`), in fp32 and in float64 alike"""
    return R == 1 and f32(momentum) == 0.0


def update_reference(probs, top, state, momentum, dtype):
    """freematch_model.py:128-165 (clip_thresh off, as the baselines run it): the three moving averages, then
    mask = max >= time_p * p_model[argmax] / max(p_model) on the UPDATED state.  `top` is the planted argmax.
    state = (p_model, label_hist, time_p) -> dict with the new state, mask, the row maxima `mx` and thresholds `thr`."""
    m = f32(momentum)
    p_model, label_hist, time_p = (s.to(dtype) for s in state)
    p = probs.to(dtype)
    R, K = p.shape
    mx = p.gather(1, top[:, None])[:, 0]
    tp = time_p * m + (1.0 - m) * mx.mean()
    pm = p_model * m + (1.0 - m) * p.mean(0)
    hist = torch.bincount(top, minlength=K).to(dtype)
    lh = label_hist * m + (1.0 - m) * (hist / hist.sum())
    thr = tp * (pm / pm.max())[top]
    return {"p_model": pm, "label_hist": lh, "time_p": tp, "mask": (mx >= thr).float(), "mx": mx, "thr": thr}


def _update_draw(R, K, momentum, attempt):
    g = gen(R, K, UPDATE_MOMENTA.index(momentum), attempt, 71)
    u = lambda: (1.0 + 0.2 * torch.rand(K, generator=g)) / K
    p_model, label_hist = u(), u()
    c = dict(R=R, K=K, momentum=momentum, p_model=p_model / p_model.sum(), label_hist=label_hist / label_hist.sum(),
             time_p=torch.tensor([UPDATE_TIME_P]), calls=[_plant_probs(g, R, K) for _ in range(UPDATE_CALLS)])
    return c


def update_run_reference(c, dtype):
    """the UPDATE_CALLS consecutive calls: each starts from the state the one before left"""
    state, out = (c["p_model"], c["label_hist"], c["time_p"]), []
    for probs, top, _ in c["calls"]:
        out.append(update_reference(probs, top, state, c["momentum"], dtype))
        state = tuple(out[-1][k] for k in ("p_model", "label_hist", "time_p"))
    return out


@functools.lru_cache(maxsize=None)
def update_case(R, K, momentum):
    """-> dict: the initial state (p_model, label_hist near uniform, time_p = 0.75) and UPDATE_CALLS planted batches.  The draw is
    repeated (the attempt number enters the seed) until every row of every call keeps MIN_GAP between its maximum and its
    float64 threshold; the one-row momentum-0 cases sit ON the threshold by construction and are exempt."""
    for attempt in range(UPDATE_MAX_TRIES):
        c = _update_draw(R, K, momentum, attempt)
        if update_at_threshold(R, momentum) or all(float((o["mx"] - o["thr"]).abs().min()) >= MIN_GAP for o in update_run_reference(c, torch.float64)):
            return c
    raise AssertionError(f"no draw of ({R}, {K}, {momentum}) keeps its rows off the threshold")


# =====================================================================================================================
# stil_freematch_entropy
# =====================================================================================================================
ENTROPY_TABLE = ((1, 1), (1, 5), (2, 2), (255, 3), (256, 3), (257, 3), (300, 286), (513, 65), (40, 1000))
ENTROPY_MASKS = ("mixed", "full", "empty", "odd")
ENTROPY_MARGIN = 4.0            # the planted top-1 logit, over 0.5 * randn
ENTROPY_TIE_ROW = 3             # selected by every non-empty mask
ENTROPY_MIN_GRAD = 1e-4


@functools.lru_cache(maxsize=None)
def entropy_case(R, K):
    """-> dict: logits z [R, K] with the planted top-1 column `top` (K <= 3: r % 2, so class 2 of K = 3 is predicted by no row;
    else (7 r + 3) % K), a tie row (R >= 4, K >= 2: row 3 holds the same logit at `tie` = (c0, c1), c0 wins; at K = 3 c1 is
    class 2, which only a last-index argmax would predict), p_model and label_hist near uniform, label_hist exactly 0 at
    `zero_class` = top[0] where K >= 3."""
    g = gen(R, K, 73)
    z = 0.5 * torch.randn(R, K, generator=g)
    top = (torch.arange(R) % 2) % K if K <= 3 else (7 * torch.arange(R) + 3) % K
    z[torch.arange(R), top] = ENTROPY_MARGIN + 0.25 * torch.rand(R, generator=g)
    tie = None
    if R > ENTROPY_TIE_ROW and K >= 2:
        c0 = int(top[ENTROPY_TIE_ROW])
        c0, c1 = (c0, c0 + 1) if c0 + 1 < K else (c0 - 1, c0)
        z[ENTROPY_TIE_ROW, c0] = z[ENTROPY_TIE_ROW, c1] = ENTROPY_MARGIN
        top[ENTROPY_TIE_ROW] = c0
        tie = (c0, c1)
    u = lambda: (1.0 + 0.2 * torch.rand(K, generator=g)) / K
    p_model, label_hist = u(), u()
    zero_class = int(top[0]) if K >= 3 else None
    if zero_class is not None:
        label_hist[zero_class] = 0.0
    return dict(R=R, K=K, z=z, top=top, tie=tie, p_model=p_model / p_model.sum(), label_hist=label_hist, zero_class=zero_class)


def entropy_mask(R, kind):
    """[R] floats; non-zero means selected, as with mask.bool(): "odd" selects with 0.5 and -1.0"""
    r = torch.arange(R)
    if kind == "mixed":
        return (r % 3 != 2).float()
    if kind == "odd":
        return torch.where(r % 4 != 1, torch.where(r % 2 == 0, 0.5, -1.0), 0.0)
    return torch.ones(R) if kind == "full" else torch.zeros(R)


def entropy_has_gradient(c, mask):
    """the loss moves with z only when the selected rows predict two classes at the least"""
    return len(set(c["top"][mask != 0].tolist())) >= 2


def _inf0(x):
    return torch.where(torch.isinf(x), torch.zeros_like(x), x)


def entropy_reference(c, mask, dtype):
    """freematch_utils.py:17-45 over the rows with mask != 0: a = normalise(p_model * inf0(1 / label_hist)), hist = the share of
    each class among the (planted) predictions, v = normalise(mean softmax(z) * inf0(1 / hist)), both scalers constants;
    loss = sum(a log(v + 1e-12)); dz = d loss / d z.  An empty mask: loss 0, dz 0 (freematch_model.py skips the term)."""
    K, sel = c["K"], mask != 0
    z = c["z"].detach().clone().to(dtype).requires_grad_()
    if not bool(sel.any()):
        return {"loss": torch.zeros((), dtype=dtype), "dz": torch.zeros_like(z.detach()), "hist": None, "a": None}
    ps = z[sel].softmax(-1)
    hist = torch.bincount(c["top"][sel], minlength=K).to(dtype)
    hist = hist / hist.sum()
    a = c["p_model"].to(dtype) * _inf0(1.0 / c["label_hist"].to(dtype))
    a = a / a.sum()
    v = ps.mean(0) * _inf0(1.0 / hist)
    v = v / v.sum()
    loss = (a * torch.log(v + f32(EPS_ENTROPY))).sum()
    (dz,) = torch.autograd.grad(loss, z)
    return {"loss": loss.detach(), "dz": dz, "hist": hist, "a": a}
