"""Inputs and the restatements of RoTTA's kernels (stil_tta_amd/csrc/stil_rotta.h; definition as recalled: unpinned) shared by
tests/test_rotta_cpu.py and tests/test_gpu_rotta.py: the teacher logits and starting banks of every bank-update case, the walk over
the samples restated with its scores in float64 or float32 and the smallest margin any of its decisions hangs on, the loss on the
bank by autograd, and the teacher's moving average."""
import functools
import math

import numpy as np
import torch

NS = (1, 4, 8)                   # slots; 1: every decision is about slot 0
KS = (1, 2, 5, 300)              # classes; 1: the uncertainty terms vanish; 300 > N: a class's share N / K lies below one slot
BS = (1, 7, 70)                  # incoming samples; 70 > N forces evictions of samples the same call accepted
STARTS = ("empty", "half", "full")   # full: every slot filled and all but one of one class
LAMBDA_T, LAMBDA_U = 1.0, 1.0
MIN_MARGIN = 5e-5                # the bar tests/test_roid_cpu.py holds its selections to
INT_MAX = 2 ** 31 - 1


def f32(v):
    """v as the float32 the C ABI receives"""
    return float(np.float32(v))


def update_cases():
    return [(N, K, B, s) for N in NS for K in KS for B in BS for s in STARTS]


def _logits(B, K, seed):
    """float32 logits [B, K]: uniform in [-1, 1] scaled row by row from 0.5 to 6, so the entropies spread over (0, ln K)"""
    g = torch.Generator().manual_seed(seed)
    z = 2.0 * torch.rand(B, K, generator=g) - 1.0
    scale = 0.5 + 5.5 * torch.rand(B, 1, generator=g)
    return (z * scale).float().contiguous()


def start_bank(N, K, start, seed):
    """-> dict(label int32 [N], unc float32 [N], age int32 [N], occ int32 [K], n int32 [1]) of a consistent bank: filled slots are the
    prefix [0, n), occ counts their labels.  empty: n = 0; half: n = N // 2, labels drawn; full: n = N, every label 0 but the last
    slot's (class 1 when there is one): a full but unbalanced bank."""
    g = np.random.default_rng(seed)
    n = {"empty": 0, "half": N // 2, "full": N}[start]
    label = np.full(N, -1, dtype=np.int32)
    unc = np.zeros(N, dtype=np.float32)
    age = np.zeros(N, dtype=np.int32)
    if start == "half":
        label[:n] = g.integers(0, K, n)
    elif start == "full":
        label[:n] = 0
        if K > 1 and N > 1:
            label[n - 1] = 1
    if K > 1:
        unc[:n] = (g.random(n) * math.log(K)).astype(np.float32)
    age[:n] = g.integers(1, 3 * N + 1, n)
    occ = np.bincount(label[:n], minlength=K).astype(np.int32)
    return dict(label=label, unc=unc, age=age, occ=occ, n=np.array([n], dtype=np.int32))


def rows_ref(z, dtype=torch.float64):
    """-> (lse, p, H, yhat) of the logits z in `dtype`; yhat the first maximum of the float32 logits (exact in any dtype)"""
    x = z.to(dtype)
    logp = torch.log_softmax(x, dim=1)
    p = logp.exp()
    H = -(p * logp).sum(dim=1)
    yhat = torch.tensor([int(np.argmax(r)) for r in z.numpy()], dtype=torch.int32)   # numpy's argmax: the first maximum
    return torch.logsumexp(x, dim=1), p, H, yhat


def bank_walk(H, yhat, N, K, bank, lt=LAMBDA_T, lu=LAMBDA_U, ft=np.float64):
    """stil_rotta_bank_update's second launch restated: the samples in order, every score formed in `ft` from H (the row entropies,
    any float array) and the bank's own unc / age.  -> dict: the bank after (label, unc [ft], age, occ, n), owner, accepted, slot_of,
    counts, and margin, the smallest distance any decision keeps from flipping: |score(candidate) - s_new| of every comparison and the
    lead of every argmax over the best candidate that is not its exact twin (the same age and unc: a tie in any arithmetic, which
    the lowest slot wins)."""
    label, age, occ = bank["label"].copy(), bank["age"].astype(np.int64), bank["occ"].copy()
    unc = bank["unc"].astype(ft)
    n = int(bank["n"][0])
    B = len(H)
    H = np.asarray(H, dtype=ft)
    lt, lu, lnK, dN = ft(lt), ft(lu), ft(math.log(K)) if K > 1 else ft(1.0), ft(N)
    owner = np.full(N, -1, dtype=np.int32)
    accepted, slot_of = np.zeros(B, dtype=np.uint8), np.full(B, -1, dtype=np.int32)
    n_acc = n_evict = 0
    margin = float("inf")

    def score(i):
        s = lt / (ft(1.0) + np.exp(-ft(age[i]) / dN))
        return s + (lu * unc[i] / lnK if K > 1 else ft(0.0))

    for b in range(B):
        c, u = int(yhat[b]), H[b]
        s_new = ft(0.5) * lt + (lu * u / lnK if K > 1 else ft(0.0))
        slot, filled = -1, False
        minority = int(occ[c]) * K < N
        if minority and n < N:
            slot = n
        else:
            mo = int(occ.max())
            cand = [i for i in range(n) if (occ[label[i]] == mo if minority else label[i] == c)]
            sc = [score(i) for i in cand]
            best = max(range(len(cand)), key=lambda j: (sc[j], -cand[j]))
            for j in range(len(cand)):
                if j != best and not (age[cand[j]] == age[cand[best]] and unc[cand[j]] == unc[cand[best]]):
                    margin = min(margin, float(sc[best] - sc[j]))
            margin = min(margin, abs(float(sc[best] - s_new)))
            if sc[best] > s_new:
                slot, filled = cand[best], True
        if slot >= 0:
            if filled:
                occ[label[slot]] -= 1
                n_evict += 1
            else:
                n += 1
            label[slot], unc[slot], age[slot], owner[slot] = c, u, 0, b
            occ[c] += 1
            n_acc += 1
            accepted[b], slot_of[b] = 1, slot
        age[:n] = np.minimum(age[:n] + 1, INT_MAX)
    return dict(label=label, unc=unc, age=age.astype(np.int32), occ=occ, n=np.array([n], dtype=np.int32), owner=owner, accepted=accepted,
                slot_of=slot_of, counts=np.array([n_acc, n_evict, n, 0], dtype=np.int32), margin=margin)


def _case_at(N, K, B, start, seed):
    z = _logits(B, K, seed)
    bank = start_bank(N, K, start, seed + 1)
    lse, p, H, yhat = rows_ref(z)
    return z, bank, dict(lse=lse, p=p, H=H, yhat=yhat, **bank_walk(H.numpy(), yhat.numpy(), N, K, bank))


@functools.lru_cache(maxsize=None)
def update_case(N, K, B, start):
    """-> (logits, starting bank, float64 reference) of one case, computed once (read-only).  The seed is the first of 1000 (100 N +
    K) + 10 B + start's index, + 1, + 2, ... at which the float64 walk keeps a margin of 2 x MIN_MARGIN: a draw that puts two scores
    closer than that is replaced, not tolerated (tests/test_rotta_cpu.py holds the bar, in float32 as well)."""
    base = 1000 * (100 * N + K) + 10 * B + STARTS.index(start)
    for seed in range(base, base + 200, 3):
        z, bank, ref = _case_at(N, K, B, start, seed)
        if ref["margin"] >= 2 * MIN_MARGIN:
            return z, bank, ref
    raise AssertionError(f"no well-conditioned draw for {(N, K, B, start)}")


def one_class_stream(B, K, c):
    """logits of B samples whose first maximum is class c throughout, at varying confidence"""
    z = _logits(B, K, 77)
    z[:, c] = z.max(dim=1).values + torch.linspace(0.5, 4.0, B)
    return z.contiguous()


# ---------------------------------------------------------------------------------------------- the loss on the bank
ROWS = (1, 5, 64, 70)
LOSS_KS = (1, 2, 7, 300)
AGES = ("zero", "mixed", "huge")


def loss_cases():
    return [(r, k, a) for r in ROWS for k in LOSS_KS for a in AGES]


def loss_input(rows, K, ages):
    """-> (student logits, teacher logits [rows, K] float32, label int32 [rows] (about a quarter of the slots empty, never all; one
    slot: filled), age int32 [rows]: 0 | drawn from [0, 4 rows] | 10^6)"""
    g = torch.Generator().manual_seed(500 * rows + K)
    zs = (3.0 * torch.randn(rows, K, generator=g)).float()
    zt = (zs + 1.5 * torch.randn(rows, K, generator=g)).float()
    label = torch.randint(0, K, (rows,), generator=g).to(torch.int32)
    if rows > 1:
        label[torch.rand(rows, generator=g) < 0.25] = -1
        label[0] = 0
    age = {"zero": torch.zeros(rows, dtype=torch.int32), "mixed": torch.randint(0, 4 * rows + 1, (rows,), generator=g).to(torch.int32),
           "huge": torch.full((rows,), 10 ** 6, dtype=torch.int32)}[ages]
    return zs.contiguous(), zt.contiguous(), label, age


def rotta_forward(xs, xt, label, age):
    """stil_rotta_rows restated: xs (differentiable) and xt in one floating dtype.  -> dict(loss (differentiable), ce, w, n)"""
    rows = xs.shape[0]
    v = (label >= 0).to(xs.dtype)
    n = int((label >= 0).sum())
    e = torch.exp(-age.to(xs.dtype) / rows)
    w = v * e / (1.0 + e)
    ce = -(torch.softmax(xt, dim=1) * torch.log_softmax(xs, dim=1)).sum(dim=1) * v
    loss = (w * ce).sum() / n if n > 0 else 0.0 * xs.sum()
    return dict(loss=loss, ce=ce.detach(), w=w, n=n)


def loss_ref(zs, zt, label, age, dtype):
    x = zs.detach().to(dtype).clone().requires_grad_(True)
    out = rotta_forward(x, zt.to(dtype), label, age)
    (g,) = torch.autograd.grad(out["loss"], [x])
    out["loss"] = out["loss"].detach()
    out["grad"] = g
    return out


@functools.lru_cache(maxsize=None)
def loss_ref64(rows, K, ages):
    return loss_ref(*loss_input(rows, K, ages), torch.float64)


def teacher_ref(teacher, params, nu):
    """(1 - nu) teacher + nu params in float64 at the float32 nu, rounded once"""
    nu = f32(nu)
    return ((1.0 - nu) * teacher.double() + nu * params.double()).float()
