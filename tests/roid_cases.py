"""Inputs and the restatement of ROID's row loss (stil_tta_amd/csrc/stil_roid.h) shared by tests/test_roid_cpu.py and
tests/test_gpu_roid.py: the logits and running means of every case, the loss by autograd in float64 or float32 (the weights and
the mask under no_grad, the 1e-9 rule included), the closed-form gradient of the header, and the weight ensembling."""
import functools

import numpy as np
import torch

ROWS = (1, 2, 7, 130, 512)       # 1: both ranges degenerate; 130, 512: the finishing workgroup and the column walk stride over the rows
KS = (1, 2, 286, 1000, 5000)     # 1: p = 1, everything degenerate; 286, 1000, 5000: more than one pass of a 256-thread workgroup
KINDS = ("spread", "peaked", "tied")
EMAS = ("uniform", "skewed")
TAU, CLIP, EPS, MOMENTUM = 1.0 / 3.0, 0.99, 1e-5, 0.9
RANGE_FLOOR = 1e-9               # the project's degenerate rule


def f32(v):
    """v as the float32 the C ABI receives"""
    return float(np.float32(v))


def roid_cases():
    return [(r, k, kind, e) for r in ROWS for k in KS for kind in KINDS for e in EMAS]


def roid_input(rows, K, kind):
    """float32 logits [rows, K] from generator seed 1000 rows + K, z = 2 rand - 1:
    spread: row r scaled by linspace(0.5, 8, rows)[r] (rows = 1: by 3), from near-uniform to confident rows;
    peaked: z * 2, then one drawn column per row raised by linspace(1, 12, rows)[r];
    tied:   row 0 times 3, repeated: every row identical, both ranges are 0 and only the 1e-9 rule decides."""
    g = torch.Generator().manual_seed(1000 * rows + K)
    z = 2.0 * torch.rand(rows, K, generator=g) - 1.0
    if kind == "spread":
        scale = torch.linspace(0.5, 8.0, rows) if rows > 1 else torch.tensor([3.0])
        z = z * scale[:, None]
    elif kind == "peaked":
        z = z * 2.0
        col = torch.randint(0, K, (rows,), generator=g)
        z[torch.arange(rows), col] += torch.linspace(1.0, 12.0, rows)
    elif kind == "tied":
        z = (z[0:1] * 3.0).repeat(rows, 1)
    else:
        raise ValueError(kind)
    return z.float().contiguous()


def roid_ema(K, kind):
    """the running mean prediction before the call, float32 [K]: uniform 1 / K (the state's start), or softmax(4 rand(K)), seed 7 + K"""
    if kind == "uniform":
        return torch.full((K,), 1.0 / K, dtype=torch.float32)
    g = torch.Generator().manual_seed(7 + K)
    return torch.softmax(4.0 * torch.rand(K, generator=g), dim=0).float().contiguous()


def _minmax(v):
    """-> (v min-max normalised, or zeros when its range is <= 1e-9; whether it was; the range)"""
    lo, hi = v.min(), v.max()
    rng = float(hi - lo)
    if rng <= RANGE_FLOOR:
        return torch.zeros_like(v), True, rng
    return (v - lo) / (hi - lo), False, rng


def roid_forward(x, ema, tau, clip, eps, momentum):
    """ROID's row loss of the logits x [rows, K] (any floating dtype; differentiable in x) against the running mean `ema` [K] of the
    same dtype, as csrc/stil_roid.h states it.  -> dict: loss (differentiable), and detached lse, probs, H, cos, slr, dn, cn, w, keep,
    counts, pbar, ema (after the update), prior, scores, margin (min_r |dn_r - mean dn|; inf when the d range is degenerate and the
    rule, not a comparison of close numbers, decides), d_range, c_range."""
    rows, K = x.shape
    logp = torch.log_softmax(x, dim=1)
    p = logp.exp()
    H = -(p * logp).sum(dim=1)
    with torch.no_grad():
        pd = p.detach()
        cos = (pd @ ema) / (pd.norm(dim=1) * ema.norm())
        dn, ddeg, d_range = _minmax(1.0 - cos)
        cn, cdeg, c_range = _minmax(-H.detach())
        mean = dn.mean()
        keep = ~(dn < mean)
        w = torch.where(keep, torch.exp(dn * cn / tau), torch.zeros_like(dn))
        margin = float("inf") if ddeg else float((dn - mean).abs().min())
    q = p.clamp(max=clip)
    slr = -(q * torch.log(q / (1.0 - q) + eps)).sum(dim=1)
    loss = (w * slr).sum() / rows
    with torch.no_grad():
        pbar = pd.mean(dim=0)
        ema_new = momentum * ema + (1.0 - momentum) * pbar
        smooth = max(1.0 / rows, 1.0 / K) / pbar.max()
        prior = (pbar + smooth) / (1.0 + smooth * K)
        sc = pd * prior[None, :]
        scores = sc / sc.sum(dim=1, keepdim=True)
    counts = torch.tensor([int(keep.sum()), rows, int(ddeg), int(cdeg)], dtype=torch.int32)
    return dict(loss=loss, lse=torch.logsumexp(x.detach(), dim=1), probs=pd, H=H.detach(), cos=cos, slr=slr.detach(), dn=dn, cn=cn, w=w,
                keep=keep, counts=counts, pbar=pbar, ema=ema_new, prior=prior, scores=scores, margin=margin, d_range=d_range,
                c_range=c_range)


def roid_ref(z, ema, dtype, tau=TAU, clip=CLIP, eps=EPS, momentum=MOMENTUM):
    """roid_forward in `dtype` at the scalars as the float32 the kernel receives, with grad = d loss / d z by autograd"""
    x = z.detach().to(dtype).clone().requires_grad_(True)
    out = roid_forward(x, ema.detach().to(dtype), f32(tau), f32(clip), f32(eps), f32(momentum))
    (g,) = torch.autograd.grad(out["loss"], [x])
    out["loss"] = out["loss"].detach()
    out["grad"] = g
    return out


@functools.lru_cache(maxsize=None)
def roid_ref64(rows, K, kind, ema_kind):
    """the float64 reference of one case, computed once (read-only)"""
    return roid_ref(roid_input(rows, K, kind), roid_ema(K, ema_kind), torch.float64)


def closed_form_dz(z, w, clip, eps, grad_scale):
    """dZ of csrc/stil_roid.h in z's dtype, the weights w [rows] given:
    g_k = [p_k <= clip] (-log(u_k + eps) - u_k / ((u_k + eps)(1 - q_k))), u = q / (1 - q), q = min(p, clip);
    dZ[r,k] = grad_scale (w_r / rows) p_k (g_k - sum_j p_j g_j)"""
    rows = z.shape[0]
    p = torch.softmax(z, dim=1)
    q = p.clamp(max=clip)
    u = q / (1.0 - q)
    g = torch.where(p <= clip, -torch.log(u + eps) - u / ((u + eps) * (1.0 - q)), torch.zeros_like(p))
    return grad_scale * (w[:, None] / rows) * p * (g - (p * g).sum(dim=1, keepdim=True))


def ensemble_ref(params, theta0, momentum):
    """momentum params + (1 - momentum) theta0 in float64 at the float32 momentum, rounded once"""
    m = f32(momentum)
    return (m * params.double() + (1.0 - m) * theta0.double()).float()
