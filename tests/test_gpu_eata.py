"""EATA test-time adaptation (Niu et al., ICML 2022, "Efficient Test-Time Model Adaptation without Forgetting") in
STiLModel.test_step: sample selection and the Fisher anchor on top of TENT (tests/test_gpu_tta.py).

1. stil_eata_rows against float64 (close() at TOL of test_gpu_ops; decisions, counts, flag and gate exactly) on constructed
   inputs whose every decision is far from its threshold (tests/test_eata_cpu.py checks that), ld = K + 3 views, sentinels,
   repetition, bad arguments, n == 0 cases; tie to stil_entropy_rows.
2. stil_eata_anchor / stil_eata_fisher_accum against float64 on a synthetic flat layout.
3. The step against the contract restated here in float64 on the oracle, on the device's ReLU / max-pool decisions.  The
   suite's random states give uninformative logits, so the test scales model.classifier_multimodal.{weight,bias} (x15 DVM, x10 cardiac) and
   passes tta_e_margin / tta_d_margin explicitly, placed by a float64 pre-pass in the middle of the widest gap of the
   sorted H (|c|) between the 25th and 75th percentile.  The |c| are those of the reliable rows: in these collapsed random
   states the confident rows all predict one class, so a margin placed among the |c| of all rows leaves the redundancy
   filter one outcome on the reliable ones.  THE TEST SETS THE ADAPTATION STATE'S m DIRECTLY before the second batch (to the
   float64 softmax of the batch's most confident row outside its modal class, valid) so that the redundancy filter has both outcomes; the third
   batch runs on the m the device carried over.  The restatement starts from the same m.
4. Properties: n == 0 batch, no weight-gradient product, no synchronisation beyond a "tent" step's, state rules, Fisher
   round trip, fit.test(tta_fisher_loader=...)."""
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_gpu_ops import TOL, close  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
import contextlib  # noqa: E402
import test_gpu_tta as T  # noqa: E402

SENTINEL = -7.25
ROWS = (1, 7, 512)
KS = (1, 2, 286, 1000, 5000)
VARIANTS = ("mixed_valid", "mixed_invalid", "tied_valid")
D_MARGIN = 0.5
MU = 0.9


# ------------------------------------------------------------------------------------------ check 1: the row kernel
def eata_cases():
    return [(r, k, v) for r in ROWS for k in KS for v in VARIANTS]


def eata_input(rows, K, variant, seed=0):
    """-> (Z [rows, K] float32, E0, d, m [K] float32, valid).  Row r belongs to family r % 4:
    0 one logit +60 on a class other than 0 (H ~ 0, c ~ 0: selected); 1 every logit tied (H = ln K: unreliable);
    2 THE fixed peaked row (+60 on class 0), whose softmax is m (|c| = 1: redundant while m is valid);
    3 one logit +8 on a class other than 0 (a moderate entropy: reliable or not with K, weight well away from exp(E0)).
    "tied_valid": every row tied (n == 0).  K == 1: E0 = 0 and H = 0, nothing is reliable (n == 0)."""
    g = torch.Generator().manual_seed(seed + 1000 * rows + K)
    z = torch.rand(rows, K, generator=g) * 2.0 - 1.0
    fixed = torch.zeros(K)
    fixed[0] = 60.0
    for r in range(rows):
        fam = 1 if variant == "tied_valid" else r % 4
        j = 0 if K == 1 else 1 + int(torch.randint(0, K - 1, (1,), generator=g))
        if fam == 0:
            z[r, j] += 60.0
        elif fam == 1:
            z[r] = 3.5
        elif fam == 2:
            z[r] = fixed
        else:
            z[r, j] += 8.0
    e0 = float(np.float32(0.4 * math.log(K)))
    m = torch.softmax(fixed.double(), 0).float()
    return z.float(), e0, D_MARGIN, m, int(variant != "mixed_invalid")


def eata_ref(z, e0, d, mu, m, valid, dtype, grad_scale=1.0):
    """The contract's steps 1-5 with autograd in `dtype`."""
    x = z.detach().to(dtype).clone().requires_grad_(True)
    logp = torch.log_softmax(x, dim=1)
    p = logp.exp()
    H = -(p * logp).sum(dim=1)
    md = m.to(dtype)
    pd, Hd = p.detach(), H.detach()
    c = (pd @ md) / (md.norm().clamp_min(1e-8) * pd.norm(dim=1).clamp_min(1e-8)) if valid else torch.zeros_like(Hd)
    rel = Hd < e0
    sel = rel & (c.abs() < d) if valid else rel
    w = torch.exp(e0 - Hd)
    n = int(sel.sum())
    if n > 0:
        loss = (sel.to(dtype) * w * H).sum() / n
        (g,) = torch.autograd.grad(loss * grad_scale, [x])
        pbar = (sel.to(dtype)[:, None] * pd).sum(0) / n
        m_new, valid_new = (mu * md + (1 - mu) * pbar if valid else pbar), 1
    else:
        loss, g, m_new, valid_new = torch.zeros((), dtype=dtype), torch.zeros_like(x), md, valid
    return dict(loss=loss.detach(), grad=g, probs=pd, H=Hd, lse=torch.logsumexp(x.detach(), dim=1), cos=c, w=w, rel=rel, sel=sel,
                n=n, n_rel=int(rel.sum()), m=m_new, valid=valid_new)


def _run_rows(L, zb, ld, rows, K, e0, d, m, valid, gs, nt=5):
    dev = "cuda"
    o = dict(m=torch.full((K + 1,), SENTINEL, device=dev), mv=torch.tensor([valid, 77], dtype=torch.int32, device=dev),
             lse=torch.full((rows + 1,), SENTINEL, dtype=torch.float64, device=dev),
             Hd=torch.full((rows + 1,), SENTINEL, dtype=torch.float64, device=dev), p=torch.full((rows + 1, ld), SENTINEL, device=dev),
             H=torch.full((rows + 1,), SENTINEL, device=dev), c=torch.full((rows + 1,), SENTINEL, device=dev),
             w=torch.full((rows + 1,), SENTINEL, device=dev), rel=torch.full((rows + 1,), 9, dtype=torch.uint8, device=dev),
             sel=torch.full((rows + 1,), 9, dtype=torch.uint8, device=dev), dZ=torch.full((rows + 1, ld), SENTINEL, device=dev),
             counts=torch.full((5,), -3, dtype=torch.int32, device=dev), loss=torch.full((2,), SENTINEL, device=dev),
             act=torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8, device=dev), gate=torch.full((nt + 1,), 9, dtype=torch.uint8, device=dev))
    o["m"][:K] = m.cuda()
    L.eata_rows(zb.data_ptr(), ld, rows, K, e0, d, MU, gs, o["m"].data_ptr(), o["mv"].data_ptr(), o["lse"].data_ptr(), o["Hd"].data_ptr(), o["p"].data_ptr(), ld,
                o["H"].data_ptr(), o["c"].data_ptr(), o["w"].data_ptr(), o["rel"].data_ptr(), o["sel"].data_ptr(), o["dZ"].data_ptr(), ld,
                o["counts"].data_ptr(), o["loss"].data_ptr(), o["act"].data_ptr(), o["gate"].data_ptr(), nt, None)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize("rows,K,variant", eata_cases())
def test_eata_rows_against_float64(rows, K, variant):
    from stil_tta_amd._lib import lib
    L = lib()
    z, e0, d, m, valid = eata_input(rows, K, variant)
    gs = float(np.float32(0.75))
    ref = eata_ref(z, e0, d, MU, m, valid, torch.float64, gs)
    for pad in (0, 3):
        ld = K + pad
        zb = torch.full((rows + 1, ld), SENTINEL, dtype=torch.float32)
        zb[:rows, :K] = z
        zb = zb.cuda()
        a, b = (_run_rows(L, zb, ld, rows, K, e0, d, m, valid, gs) for _ in range(2))
        for k in a:
            assert torch.equal(a[k], b[k]), f"{k}: not bit-identical on repetition"
        # sentinels: padding columns, the row past the end, the element past every vector
        assert bool((a["p"][rows] == SENTINEL).all() and (a["dZ"][rows] == SENTINEL).all())
        for k in ("H", "c", "w", "lse", "Hd"):
            assert float(a[k][rows]) == SENTINEL, k
        assert int(a["rel"][rows]) == 9 and int(a["sel"][rows]) == 9 and int(a["gate"][5]) == 9
        assert float(a["m"][K]) == SENTINEL and int(a["mv"][1]) == 77 and int(a["counts"][4]) == -3 and float(a["loss"][1]) == SENTINEL
        if pad:
            assert bool((a["p"][:, K:] == SENTINEL).all() and (a["dZ"][:, K:] == SENTINEL).all())
        # decisions, counts, flag, gate: exact
        assert torch.equal(a["sel"][:rows].bool(), ref["sel"]) and torch.equal(a["rel"][:rows].bool(), ref["rel"])
        assert int(a["counts"][0]) == ref["n"] and int(a["counts"][1]) == ref["n_rel"] and int(a["counts"][2]) == valid
        assert int(a["mv"][0]) == ref["valid"]
        assert a["gate"][:5].tolist() == ([1, 0, 1, 1, 0] if ref["n"] > 0 else [0] * 5)
        close(a["lse"][:rows], ref["lse"], name="lse")
        close(a["p"][:rows, :K], ref["probs"], name="probs")
        close(a["H"][:rows], ref["H"], name="H")
        assert torch.equal(a["Hd"][:rows].float(), a["H"][:rows])
        close(a["c"][:rows], ref["cos"], name="cos")
        close(a["w"][:rows], ref["w"], name="w")
        close(a["loss"][:1], ref["loss"].view(1), name="loss")
        close(a["m"][:K], ref["m"], name="m")
        close(a["dZ"][:rows, :K], ref["grad"], name="dZ")
        if ref["n"] == 0:
            assert bool((a["dZ"][:rows, :K] == 0).all()) and torch.equal(a["m"][:K], m) and float(a["loss"][0]) == 0.0
        # tie to TENT's kernel: p, H, lse bit for bit; dZ row r = sel_r w_r (rows / n) x its dZ row, both as the gradient of
        # grad_scale x their loss: TENT's loss is the mean over rows, so its kernel takes grad_scale / rows (EntropyFn passes 1 / R)
        lse = torch.empty(rows, dtype=torch.float64, device="cuda")
        p = torch.empty(rows, ld, device="cuda")
        H = torch.empty(rows, device="cuda")
        dZ = torch.empty(rows, ld, device="cuda")
        mean = torch.empty(1, device="cuda")
        L.entropy_rows(zb.data_ptr(), ld, rows, K, float(np.float32(gs / rows)), lse.data_ptr(), p.data_ptr(), ld, H.data_ptr(), dZ.data_ptr(), ld, mean.data_ptr(), None)
        torch.cuda.synchronize()
        assert torch.equal(a["lse"][:rows], lse.cpu()) and torch.equal(a["H"][:rows], H.cpu())
        assert torch.equal(a["p"][:rows, :K], p.cpu()[:, :K])
        if ref["n"] > 0:
            f = a["sel"][:rows].double() * a["w"][:rows].double() * (rows / ref["n"])
            close(a["dZ"][:rows, :K], f[:, None] * dZ.cpu()[:, :K].double(), name="dZ against stil_entropy_rows")


def test_eata_rows_rejects_bad_arguments():
    from stil_tta_amd._lib import lib
    fn = lib()._dll.stil_eata_rows
    z = torch.zeros(4, 8, device="cuda")
    m = torch.zeros(8, device="cuda")
    mv = torch.zeros(1, dtype=torch.int32, device="cuda")
    lse, hd = (torch.zeros(4, dtype=torch.float64, device="cuda") for _ in range(2))
    p, dz = torch.zeros(4, 8, device="cuda"), torch.zeros(4, 8, device="cuda")
    H, c, w = (torch.zeros(4, device="cuda") for _ in range(3))
    rel, sel = (torch.zeros(4, dtype=torch.uint8, device="cuda") for _ in range(2))
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    act, gate = (torch.zeros(3, dtype=torch.uint8, device="cuda") for _ in range(2))

    def call(ld=8, rows=4, K=8, ldp=8, ldd=8, mu=0.9, d=0.05, m_=m, act_=act, nt=3):
        import ctypes
        f32 = ctypes.c_float
        return fn(z.data_ptr(), ld, rows, K, f32(1.0), f32(d), f32(mu), f32(1.0), None if m_ is None else m_.data_ptr(), mv.data_ptr(), lse.data_ptr(), hd.data_ptr(), p.data_ptr(), ldp,
                  H.data_ptr(), c.data_ptr(), w.data_ptr(), rel.data_ptr(), sel.data_ptr(), dz.data_ptr(), ldd, cnt.data_ptr(), loss.data_ptr(),
                  None if act_ is None else act_.data_ptr(), gate.data_ptr(), nt, None)
    assert call() == 0
    assert call(ld=7) != 0 and call(K=0) != 0 and call(rows=0) != 0 and call(ldp=4) != 0 and call(ldd=4) != 0
    assert call(mu=1.5) != 0 and call(d=-1.0) != 0 and call(m_=None) != 0 and call(act_=None) != 0 and call(nt=-1) != 0
    assert call(act_=None, nt=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ check 2: the slab kernels
C2T = [0, 0, -1, 1, 2, 2, -1, 3, -1, 1, -1, -1]
ACTIVE = [1, 0, 1, 1]
ACHUNKS = [0, 1, 3, 4, 5, 6, 7, 12, -5, 99]      # 3: inactive tensor; 6: padding; 12, -5, 99: out of range
LIVE = [0, 1, 4, 5, 7]


def slab_input(seed=3):
    g = torch.Generator().manual_seed(seed)
    n = len(C2T) * 1024
    tot = n + 1024                                   # one sentinel chunk past the slab
    params = torch.randn(tot, generator=g)
    grads = torch.randn(tot, generator=g) * 1e-2
    nc = len(ACHUNKS) * 1024
    theta0 = torch.randn(nc, generator=g) * 0.1
    for j, ch in enumerate(ACHUNKS):
        if 0 <= ch <= len(C2T):
            theta0[j * 1024:(j + 1) * 1024] += params[ch * 1024:(ch + 1) * 1024]
    fisher = torch.rand(nc, generator=g) * 1e-3
    return n, params, grads, theta0, fisher


def slab_ref(dtype, alpha, scale):
    n, params, grads, theta0, fisher = slab_input()
    g, F = grads.to(dtype).clone(), fisher.to(dtype).clone()
    R = torch.zeros((), dtype=dtype)
    for j, ch in enumerate(ACHUNKS):
        if ch not in LIVE:
            continue
        s, sc = slice(ch * 1024, (ch + 1) * 1024), slice(j * 1024, (j + 1) * 1024)
        dlt = params[s].to(dtype) - theta0[sc].to(dtype)
        R = R + alpha * (fisher[sc].to(dtype) * dlt * dlt).sum()
        g[s] += 2 * alpha * fisher[sc].to(dtype) * dlt
        F[sc] += grads[s].to(dtype) ** 2 * scale
    return g, R, F


def test_slab_kernels_against_float64():
    from stil_tta_amd._lib import lib
    L = lib()
    alpha, scale = float(np.float32(37.5)), float(np.float32(1.0 / 3.0))
    n, params, grads, theta0, fisher = slab_input()
    g64, R64, F64 = slab_ref(torch.float64, alpha, scale)
    c2t = torch.tensor(C2T, dtype=torch.int32).cuda()
    act = torch.tensor(ACTIVE, dtype=torch.uint8).cuda()
    ach = torch.tensor(ACHUNKS, dtype=torch.int32).cuda()
    outs = []
    for rep in range(2):
        P, G, T0, F = params.cuda(), grads.cuda(), theta0.cuda(), fisher.cuda()
        part = torch.full((len(ACHUNKS) + 1,), SENTINEL, dtype=torch.float64, device="cuda")
        R = torch.full((2,), SENTINEL, device="cuda")
        L.eata_fisher_accum(F.data_ptr(), G.data_ptr(), ach.data_ptr(), len(ACHUNKS), c2t.data_ptr(), act.data_ptr(), len(ACTIVE), n, scale, None)
        Fa = F.cpu()
        F = fisher.cuda()
        L.eata_anchor(P.data_ptr(), T0.data_ptr(), F.data_ptr(), G.data_ptr(), ach.data_ptr(), len(ACHUNKS), c2t.data_ptr(), act.data_ptr(),
                      len(ACTIVE), n, alpha, part.data_ptr(), R.data_ptr(), None)
        torch.cuda.synchronize()
        assert torch.equal(P.cpu(), params) and torch.equal(T0.cpu(), theta0) and torch.equal(F.cpu(), fisher)
        outs.append((G.cpu(), R.cpu(), Fa, part.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b), "not bit-identical on repetition"
    G, R, Fa, part = outs[0]
    for ch in range(len(C2T) + 1):
        s = slice(ch * 1024, (ch + 1) * 1024)
        if ch not in LIVE:
            assert torch.equal(G[s], grads[s]), f"gradient chunk {ch} outside A changed"
    for j, ch in enumerate(ACHUNKS):
        if ch not in LIVE:
            assert torch.equal(Fa[j * 1024:(j + 1) * 1024], fisher[j * 1024:(j + 1) * 1024]), f"Fisher chunk {j} changed"
            assert float(part[j]) == 0.0
    assert float(R[1]) == SENTINEL and float(part[len(ACHUNKS)]) == SENTINEL
    close(G, g64, name="grads")
    close(R[:1], R64.view(1), name="R")
    close(Fa, F64, name="fisher")
    fa, fn = L._dll.stil_eata_anchor, L._dll.stil_eata_fisher_accum
    import ctypes
    f32 = ctypes.c_float
    P, G, T0, F = params.cuda(), grads.cuda(), theta0.cuda(), fisher.cuda()
    part = torch.zeros(len(ACHUNKS), dtype=torch.float64, device="cuda")
    Rb = torch.zeros(1, device="cuda")
    ok = (P.data_ptr(), T0.data_ptr(), F.data_ptr(), G.data_ptr(), ach.data_ptr(), len(ACHUNKS), c2t.data_ptr(), act.data_ptr(), len(ACTIVE))
    assert fa(*ok, ctypes.c_long(n + 5), f32(1.0), part.data_ptr(), Rb.data_ptr(), None) != 0            # n not a multiple of 1024
    assert fa(*ok[:3], None, *ok[4:], ctypes.c_long(n), f32(1.0), part.data_ptr(), Rb.data_ptr(), None) != 0
    assert fa(ok[0] + 4, *ok[1:], ctypes.c_long(n), f32(1.0), part.data_ptr(), Rb.data_ptr(), None) != 0  # misaligned
    assert fn(F.data_ptr(), G.data_ptr(), ach.data_ptr(), -1, c2t.data_ptr(), act.data_ptr(), len(ACTIVE), ctypes.c_long(n), f32(1.0), None) != 0
    assert fn(F.data_ptr(), None, ach.data_ptr(), 2, c2t.data_ptr(), act.data_ptr(), len(ACTIVE), ctypes.c_long(n), f32(1.0), None) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ check 3: the step, restated
LOGIT_SCALE = 15.0      # DVM (K = 286); x30 also separates the rows, but puts the fp32 forward error on p (x scale) at the 3e-5 bar
CARDIAC_SCALE = 10.0    # K = 2: x30 saturates every row (H = 0 in float64); x10 gives H in [0.015, 0.15]


def scaled_state(hp, seed, scale=None):
    sd = T.initial_state(hp, seed)
    scale = (CARDIAC_SCALE if hp.num_classes == 2 else LOGIT_SCALE) if scale is None else scale
    for k in ("model.classifier_multimodal.weight", "model.classifier_multimodal.bias"):
        sd[k] = sd[k] * scale
    return sd


def widest_gap(v):
    """v: 1-D float64.  -> (middle, half-width) of the widest gap between consecutive sorted values whose positions lie
    between the 25th and the 75th percentile."""
    s = torch.sort(v.double()).values
    n = s.numel()
    lo, hi = n // 4, (3 * n) // 4
    gaps = s[lo + 1:hi + 1] - s[lo:hi]
    i = int(torch.argmax(gaps))
    return float((s[lo + i] + s[lo + i + 1]) / 2), float(gaps[i] / 2)


def _forward(sd, keys, x, hp, dtype, decisions):
    s = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k in keys:
        s[k].requires_grad_(True)
    ctx = O.force_decisions(*decisions) if decisions is not None else contextlib.nullcontext()
    with ctx as d:
        out_m = O.backbone_forward_all(s, "model.", x[0].to(dtype), x[1].to(dtype), hp, train=True, masks=None)[0]
    flips = {t: v for t, v in d.get("flips", {}).items() if v[0]} if d is not None else {}
    return s, out_m, flips


def eata_restated(sd, keys, x, hp, dtype, m, valid, mu, margins=None, fisher=None, theta0=None, alpha=0.0, decisions=None, m_row=None):
    """The contract on one batch in `dtype` on a copy of the state.  margins None: the pre-pass (E0 and d from widest_gap of
    this forward's H and the reliable rows' |c|; m_row not None: take m = softmax of this forward's most confident row outside the modal class, valid).  -> dict"""
    s, out_m, flips = _forward(sd, keys, x, hp, dtype, decisions)
    logp = torch.log_softmax(out_m, dim=1)
    p = logp.exp()
    H = -(p * logp).sum(dim=1)
    pd, Hd = p.detach(), H.detach()
    if m_row is not None:                              # the most confident row outside the batch's modal class
        am = pd.argmax(dim=1)
        other = (am != am.mode().values).nonzero().flatten()
        m, valid = pd[int(other[Hd[other].argmin()])].float(), 1
    md = m.to(dtype)
    c = (pd @ md) / (md.norm().clamp_min(1e-8) * pd.norm(dim=1).clamp_min(1e-8)) if valid else torch.zeros_like(Hd)
    gaps = {}
    if margins is None:
        e0, gaps["H"] = widest_gap(Hd)
        dm, gaps["c"] = widest_gap(c.abs()[Hd < e0]) if valid else (0.05, float("inf"))   # over the reliable rows: see the module docstring
        margins = (float(np.float32(e0)), float(np.float32(dm)))
    e0, dm = margins
    rel = Hd < e0
    sel = rel & (c.abs() < dm) if valid else rel
    w = torch.exp(e0 - Hd)
    n = int(sel.sum())
    assert n > 0
    l_ent = (sel.to(dtype) * w * H).sum() / n
    g = dict(zip(keys, [t.detach() for t in torch.autograd.grad(l_ent, [s[k] for k in keys])]))
    pbar = (sel.to(dtype)[:, None] * pd).sum(0) / n
    m_new = mu * md + (1 - mu) * pbar if valid else pbar
    R = torch.zeros((), dtype=dtype)
    ga = {k: torch.zeros_like(v) for k, v in g.items()}
    if fisher is not None:
        for k in keys:
            dlt = s[k].detach() - theta0[k].to(dtype)
            R = R + alpha * (fisher[k].to(dtype) * dlt * dlt).sum()
            ga[k] = 2 * alpha * fisher[k].to(dtype) * dlt
    return dict(p=pd, H=Hd, c=c, sel=sel, rel=rel, n=n, l_ent=l_ent.detach(), R=R, g_ent=g, g_anchor=ga, g={k: g[k] + ga[k] for k in keys},
                m=m_new, m_in=m, valid_in=valid, margins=margins, gaps=gaps, flips=flips)


def fisher_restated(sd, keys, xs, hp, dtype, decisions=None):
    F = None
    for i, x in enumerate(xs):
        s, out_m, _ = _forward(sd, keys, x, hp, dtype, None if decisions is None else decisions[i])
        loss = torch.nn.functional.cross_entropy(out_m, out_m.detach().argmax(dim=1))
        g = torch.autograd.grad(loss, [s[k] for k in keys])
        F = [t.detach() ** 2 / len(xs) for t in g] if F is None else [a + t.detach() ** 2 / len(xs) for a, t in zip(F, g)]
    return dict(zip(keys, F))


def _norm(d):
    return math.sqrt(sum(float(v.double().pow(2).sum()) for v in d.values()))


# (label, hparams, B, tta_params, batch seeds, Fisher batch seeds, state seed)
PARITY = [
    ("dvm_b64_bn_online_fisher", lambda: T.dvm_hp(64), 64, "bn", (201, 205, 203), (211, 212), 11),
    ("dvm_b32_norm", lambda: T.dvm_hp(32), 32, "norm", (301,), (), 21),
    ("cardiac_b32_bn", lambda: T.cardiac_hp(32), 32, "bn", (401,), (), 31),
]


@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_eata_step_matches_the_contract_restated_in_float64(case):
    """Bars are TENT's (tests/test_gpu_tta.py): predictions <= 3e-5 scaled, every gradient of A <= 3 e32 + 1e-4, Adam within
    2.2 lr step, everything else bit-identical; the selection equals the float64 one on every row; F <= 3 e32_F + 2e-4."""
    import test_gpu_step as S
    label, mk_hp, B, which, seeds, fseeds, sseed = case
    hp = mk_hp()
    lr = 1e-3
    sd = scaled_state(hp, sseed)
    m = T.make_model(hp, sd, tta=True, tta_method="eata", tta_params=which, tta_lr=lr, tta_probs_momentum=MU, tta_fisher_alpha=1.0)
    m.freeze()
    keys = T.adapted_keys(m)
    bad = []
    F64 = None
    sd0 = {k: v.cpu() for k, v in m.state_dict().items()}
    if fseeds:
        fb = [T.tta_batch(hp, B, s) for s in fseeds]
        before = T.full_state(m)
        decs = []
        for b in fb:                                   # the decisions of every Fisher batch, one traced pass each
            with S._trace_decisions() as trace:
                m.estimate_tta_fisher([T.to_dev(b)])
                torch.cuda.synchronize()
                decs.append(S._device_decisions(m, trace))
        assert m.estimate_tta_fisher([T.to_dev(b) for b in fb]) == len(fb)
        torch.cuda.synchronize()
        after = T.full_state(m)
        for k in before:
            assert torch.equal(before[k], after[k]), f"estimate_tta_fisher changed {k}"
        Fd = {k: v.cpu().double() for k, v in m.tta_fisher_state().items()}
        xs = [b[0] for b in fb]
        F64 = fisher_restated(sd0, keys, xs, hp, torch.float64, decs)
        F64free = fisher_restated(sd0, keys, xs, hp, torch.float64)
        F32 = fisher_restated(sd0, keys, xs, hp, torch.float32)
        ratios = []
        for k in keys:
            e32, err = T._rel(F32[k].double(), F64free[k]), T._rel(Fd[k], F64[k])
            ratios.append((err / (3 * e32 + 2e-4), k, err, e32))
            if err > 3 * e32 + 2e-4:
                bad.append(("fisher " + k, err, e32))
        print(f"[{label}] Fisher error / (3*e32_F + 2e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
    theta0 = {k: sd0[k] for k in keys}
    opt = {}
    for step, seed in enumerate(seeds, start=1):
        x, y = T.tta_batch(hp, B, seed)
        sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
        st = m._tent                                   # None before the first adapted batch of a run without a Fisher estimate
        if step == 1:
            m_in, valid = torch.zeros(hp.num_classes), 0
            pre = eata_restated(sd_before, keys, x, hp, torch.float64, m_in, valid, MU, fisher=F64, theta0=theta0, alpha=1.0)
        elif step == 2:                               # m set by the test: softmax of this batch's most confident minority-class row (float64 pre-pass)
            pre = eata_restated(sd_before, keys, x, hp, torch.float64, None, 0, MU, fisher=F64, theta0=theta0, alpha=1.0, m_row=0)
            m_in, valid = pre["m_in"], 1
            st.m.copy_(m_in.cuda())
            st.m_valid.fill_(1)
            if F64 is not None:                        # alpha: the anchor's gradient as large as the entropy's here
                m.hp.tta_fisher_alpha = float(np.float32(_norm(pre["g_ent"]) / _norm(pre["g_anchor"])))
                print(f"[{label}] tta_fisher_alpha = {m.hp.tta_fisher_alpha:.4g}")
        else:                                          # m as the device carried it over
            m_in, valid = st.m.cpu().clone(), int(st.m_valid.cpu()[0])
            assert valid == 1
            pre = eata_restated(sd_before, keys, x, hp, torch.float64, m_in, valid, MU, fisher=F64, theta0=theta0, alpha=1.0)
        alpha = float(m.hp.tta_fisher_alpha)
        e0, dm = pre["margins"]
        frac = pre["n"] / B
        print(f"[{label}] batch {step}: E0 {e0:.4f} (half gap {pre['gaps']['H']:.2e}) d {dm:.4f} (half gap {pre['gaps']['c']:.2e}) selected {pre['n']}/{B}")
        m.hp.tta_e_margin, m.hp.tta_d_margin = e0, dm
        before = T.full_state(m)
        with S._trace_decisions() as trace:
            m.test_step(T.to_dev((x, y)), step - 1)
            torch.cuda.synchronize()
            decisions = S._device_decisions(m, trace)
        kw = dict(margins=(e0, dm), fisher=F64, theta0=theta0, alpha=alpha)
        r64 = eata_restated(sd_before, keys, x, hp, torch.float64, m_in, valid, MU, decisions=decisions, **kw)
        r64free = eata_restated(sd_before, keys, x, hp, torch.float64, m_in, valid, MU, **kw)
        r32 = eata_restated(sd_before, keys, x, hp, torch.float32, m_in, valid, MU, **kw)
        S._check_flips(r64["flips"])
        # the margins this test uses are well placed on ITS trajectory (tests/test_eata_cpu.py checks an fp32-emulated one)
        eH = float((r32["H"].double() - r64free["H"]).abs().max())
        ec = float((r32["c"].double() - r64free["c"]).abs()[r64free["rel"]].max())
        print(f"[{label}] batch {step}: fp32 restatement error H {eH:.2e} |c| (reliable rows) {ec:.2e}; selected fraction {frac:.3f}")
        if pre["gaps"]["H"] < 100 * eH or (valid and pre["gaps"]["c"] < 100 * ec) or not 0.25 <= frac <= 0.75:
            bad.append((step, "conditioning", pre["gaps"], eH, ec, frac))
        if valid and not (bool((r64free["rel"] & ~r64free["sel"]).any()) and bool(r64free["sel"].any())):
            bad.append((step, "the redundancy filter has one outcome only"))
        lt, st = m.last_tta, m._tent
        d = S._scaled(lt["probs"].cpu().double().numpy(), r64["p"].numpy())
        print(f"[{label}] batch {step}: predictions scaled error {d:.2e} (fp32 restatement: {S._scaled(r32['p'].double().numpy(), r64free['p'].numpy()):.2e}); selected {r64['n']} reliable {int(r64['rel'].sum())}")
        if d > 3e-5:
            bad.append((step, "predictions", d))
        if not torch.equal(lt["selected"].cpu().bool(), r64["sel"]) or not torch.equal(lt["reliable"].cpu().bool(), r64["rel"]):
            bad.append((step, "selection", int((lt["selected"].cpu().bool() != r64["sel"]).sum())))
        if int(lt["n_selected"]) != r64["n"] or int(lt["n_reliable"]) != int(r64["rel"].sum()):
            bad.append((step, "counts", int(lt["n_selected"]), r64["n"]))
        close(lt["loss_entropy"].view(1), r64["l_ent"].view(1), name="loss_entropy")
        close(lt["loss_anchor"].view(1), r64["R"].view(1), name="loss_anchor")
        close(lt["loss"].view(1), (r64["l_ent"] + r64["R"]).view(1), name="loss")
        close(st.m.cpu(), r64["m"], name="m")
        if F64 is not None and step == len(seeds):
            ratio = _norm(r64["g_anchor"]) / _norm(r64["g_ent"])
            print(f"[{label}] batch {step}: |grad R| / |grad L_ent| = {ratio:.3f} at alpha {alpha:.4g}")
            assert 0.1 <= ratio <= 10.0, ratio
        gd = T.device_grads(m)
        ratios = []
        for k in keys:
            e32, err = T._rel(r32["g"][k].double(), r64free["g"][k]), T._rel(gd[k], r64["g"][k])
            ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
            if err > 3 * e32 + 1e-4:
                bad.append((step, "grad " + k, err, e32))
        print(f"[{label}] batch {step}: gradient error / (3*e32 + 1e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
        sd32 = {k: v.clone() for k, v in sd_before.items()}
        O.adam_step(sd32, r32["g"], opt, step, lr)
        after = T.full_state(m)
        aset = set(keys)
        for k, v in after.items():
            if k in aset:
                dev = float((v.cpu() - sd32[k]).abs().max())
                if dev > 2.2 * lr * step:
                    bad.append((step, "adam " + k, dev))
            elif not torch.equal(v, before[k]):
                bad.append((step, "changed " + k))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


# ------------------------------------------------------------------------------------------ check 4: properties
def _small(which="bn", method="eata", **tta):
    hp = T.dvm_hp(16, img_size=64)
    sd = scaled_state(hp, 5)
    tta.setdefault("tta_e_margin", 3.0)
    return hp, sd, (lambda: T.make_model(hp, sd, tta=True, tta_method=method, tta_params=which, **tta))


def _eata_state(m):
    st = m._tent
    return dict(exp_avg=st.exp_avg.clone(), exp_avg_sq=st.exp_avg_sq.clone(), steps=st.steps.clone(), m=st.m.clone(), m_valid=st.m_valid.clone())


def test_a_batch_that_selects_nothing_moves_nothing_and_still_scores():
    hp, sd, mk = _small()
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, 11)), T.to_dev(T.tta_batch(hp, 16, 12))
    m = mk()
    m.test_step(b1, 0)
    assert int(m.last_tta["n_selected"]) > 0 and int(m._tent.steps.max()) == 1
    s1, e1 = T.full_state(m), _eata_state(m)
    m.hp.tta_e_margin = 0.0                           # entropies are positive: nothing is reliable
    p = m.test_step(b2, 1)
    torch.cuda.synchronize()
    assert int(m.last_tta["n_selected"]) == 0 and int(m.last_tta["n_reliable"]) == 0 and float(m.last_tta["loss"]) == 0.0
    s2, e2 = T.full_state(m), _eata_state(m)
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    for k in e1:
        assert torch.equal(e1[k], e2[k]), k
    assert p.shape == (16, hp.num_classes) and bool(torch.isfinite(p).all())
    close(p.sum(1), torch.ones(16), name="scores")


@pytest.mark.parametrize("which", ["bn", "norm"])
def test_eata_step_issues_no_weight_gradient_product(which, monkeypatch):
    from stil_tta_amd._lib import lib
    hp, sd, mk = _small(which)
    m = mk()
    L = lib()
    calls = []
    for name in ("wgrad_tn", "wgrad_tn_partial"):
        orig = getattr(L, name)
        monkeypatch.setitem(L.__dict__, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    A0 = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    m.estimate_tta_fisher([T.to_dev(T.tta_batch(hp, 16, 8))])
    m.test_step(T.to_dev(T.tta_batch(hp, 16, 7)), 0)
    torch.cuda.synchronize()
    assert calls == [], f"{len(calls)} weight-gradient launches in an EATA step"
    assert any(not torch.equal(m.state_dict()[k], v) for k, v in A0.items()), "the EATA step adapted nothing"


def _sync_warnings(m, batches):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            for i, b in enumerate(batches):
                m.test_step(b, i)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return [str(w.message) for w in rec if "synchroniz" in str(w.message).lower()]


def test_eata_step_synchronises_no_more_than_a_tent_step():
    hp, sd, mk = _small()
    _, _, mk_tent = _small(method="tent")
    batches = [T.to_dev(T.tta_batch(hp, 16, 30 + i)) for i in range(3)]
    e, t = mk(), mk_tent()
    e.estimate_tta_fisher(batches[:1])
    for mm in (e, t):                                  # first batch outside the count: lazy state, layouts
        mm.test_step(batches[0], 0)
    # control: the counter sees a device -> host read
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            float(e.last_tta["loss"])
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert any("synchroniz" in str(w.message).lower() for w in rec), "the sync counter sees nothing"
    we, wt = _sync_warnings(e, batches[1:]), _sync_warnings(t, batches[1:])
    print(f"synchronising calls over two steps: eata {len(we)}, tent {len(wt)}")
    assert len(we) <= len(wt), (we, wt)
    e.hp.tta_e_margin = 0.0                            # and the n == 0 decision stays on the device too
    assert len(_sync_warnings(e, batches[1:])) <= len(wt)


def test_state_rules_reset_episodic_and_load_state_dict():
    hp, sd, mk = _small()
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, 11)), T.to_dev(T.tta_batch(hp, 16, 12))
    fb = [T.to_dev(T.tta_batch(hp, 16, 13))]
    o = mk()
    A0 = {k: v.clone() for k, v in o.state_dict().items() if k in set(T.adapted_keys(o))}
    o.estimate_tta_fisher(fb)
    F = o.tta_fisher_state()
    assert set(F) == set(T.adapted_keys(o)) and any(float(v.abs().max()) > 0 for v in F.values())
    assert list(o.state_dict().keys()) == list(sd.keys())   # the Fisher estimate is not in state_dict()
    fresh = mk()
    fresh.load_tta_fisher(F)
    q1 = fresh.test_step(b1, 0).clone()
    q2 = fresh.test_step(b2, 1).clone()
    sq = T.full_state(fresh)
    # round trip: the loaded estimate reproduces the next steps bit for bit
    assert torch.equal(o.test_step(b1, 0), q1) and torch.equal(o.test_step(b2, 1), q2)
    so = T.full_state(o)
    for k in so:
        assert torch.equal(so[k], sq[k]), k
    assert int(o._tent.m_valid[0]) == 1
    # reset_tta: A restored, moments and m cleared, F kept
    o.reset_tta()
    for k, v in A0.items():
        assert torch.equal(o.state_dict()[k], v), k
    st = o._tent
    assert int(st.m_valid[0]) == 0 and float(st.m.abs().max()) == 0 and int(st.steps.max()) == 0 and float(st.exp_avg.abs().max()) == 0
    for k, v in o.tta_fisher_state().items():
        assert torch.equal(v, F[k]), k
    assert torch.equal(o.test_step(b1, 2), q1) and torch.equal(o.test_step(b2, 3), q2)
    # episodic: every batch is a first batch (m invalid, A = A0: filter and anchor inert)
    _, _, mk_ep = _small(tta_episodic=True)
    ep = mk_ep()
    ep.load_tta_fisher(F)
    ep.test_step(b1, 0)
    p2 = ep.test_step(b2, 1).clone()
    assert float(ep.last_tta["loss_anchor"]) == 0.0 and int(ep.last_tta["n_selected"]) == int(ep.last_tta["n_reliable"])
    f2 = mk()
    assert torch.equal(f2.test_step(b2, 0), p2)
    assert not torch.equal(p2, q2), "online batch 2 equals the episodic one: nothing carried over"
    # load_state_dict drops everything, F included
    o.load_state_dict({k: v.cuda() for k, v in sd.items()})
    assert o._tent is None and o.tta_fisher_state() == {}
    with pytest.raises(ValueError):
        o.load_tta_fisher({k: v for k, v in list(F.items())[:-1]})
    _, _, mk_tent = _small(method="tent")
    with pytest.raises(ValueError):
        mk_tent().load_tta_fisher(F)


def test_fisher_estimate_from_iterables_without_len_short_and_empty():
    """estimate_tta_fisher on a generator (materialised: the list's estimate bit for bit), on an iterable shorter than
    max_batches (the N / seen rescale) and on empty ones.  The short path against the list, elementwise:
    |a - b| <= 8 2^-24 max(|a|, |b|) + 2^-126, exact zeros equal.  Every term g^2 / N is non-negative, so relative errors add:
    the list path rounds twice (one per accumulation), the short path three times (two accumulations, the rescale) and carries
    the float32 1/5 scale; together at most 6 2^-24 to first order.  The floor covers subnormal g^2."""
    hp, sd, mk = _small()
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, 11)), T.to_dev(T.tta_batch(hp, 16, 12))
    ref = mk()
    assert ref.estimate_tta_fisher([b1, b2]) == 2
    F = ref.tta_fisher_state()
    assert any(float(v.abs().max()) > 0 for v in F.values())
    g = mk()
    assert g.estimate_tta_fisher(b for b in (b1, b2)) == 2
    Fg = g.tta_fisher_state()
    assert set(Fg) == set(F)
    for k in F:
        assert torch.equal(Fg[k], F[k]), k
    s = mk()
    assert s.estimate_tta_fisher((b for b in (b1, b2)), max_batches=5) == 2
    Fs = s.tta_fisher_state()
    assert set(Fs) == set(F)
    worst = 0.0
    for k in F:
        a, b = Fs[k].double(), F[k].double()
        assert torch.equal(a == 0, b == 0), k
        bound = 8 * 2.0 ** -24 * torch.maximum(a.abs(), b.abs()) + 2.0 ** -126
        worst = max(worst, float(((a - b).abs() / bound).max()))
        assert bool(((a - b).abs() <= bound).all()), (k, float(((a - b).abs() / bound).max()))
    print(f"short iterable against the list: worst |a - b| / bound {worst:.3f}")
    e = mk()
    with pytest.raises(ValueError):
        e.estimate_tta_fisher([])
    with pytest.raises(ValueError):
        e.estimate_tta_fisher(iter([]), 3)
    assert e.tta_fisher_state() == {}


def test_freeze_and_inference_mode():
    hp, sd, mk = _small()
    b, fb = T.to_dev(T.tta_batch(hp, 16, 14)), [T.to_dev(T.tta_batch(hp, 16, 15))]
    a, c = mk(), mk()
    a.freeze()
    c.freeze()
    with torch.inference_mode():
        a.estimate_tta_fisher(fb)
        pa = a.test_step(b, 0)
    c.estimate_tta_fisher(fb)
    pc = c.test_step(b, 0)
    assert torch.equal(pa, pc)
    sa, sc = T.full_state(a), T.full_state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert not any(q.requires_grad for q in a.parameters())


def test_fit_test_estimates_the_fisher_after_the_checkpoint_load(tmp_path):
    from stil_tta_amd import fit
    hp, sd, mk = _small()
    loader = [T.tta_batch(hp, 16, 20 + i) for i in range(3)]
    floader = [T.tta_batch(hp, 16, 40 + i) for i in range(3)]
    ck = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": {k: v.clone() for k, v in sd.items()}}, ck)
    a = mk()
    a.load_state_dict({k: v.cuda() for k, v in scaled_state(hp, 77).items()})   # other weights: the estimate must be the checkpoint's
    a.estimate_tta_fisher([T.to_dev(floader[0])])
    ra = fit.test(a, loader, ck, tta_fisher_loader=floader, tta_fisher_batches=2)
    h = mk()
    h.freeze()
    h.estimate_tta_fisher([T.to_dev(b) for b in floader[:2]])
    Fh = h.tta_fisher_state()
    h.acc_test.reset()
    h.auc_test.reset()
    for i, bt in enumerate(loader):
        h.test_step(T.to_dev(bt), i)
    rh = {k: float(v) for k, v in h.test_epoch_end().items()}
    assert ra.keys() == rh.keys() and all(ra[k] == rh[k] or (ra[k] != ra[k] and rh[k] != rh[k]) for k in ra), (ra, rh)
    Fa = a.tta_fisher_state()
    for k in Fh:
        assert torch.equal(Fa[k], Fh[k]), k
    sa, sh = T.full_state(a), T.full_state(h)
    for k in sa:
        assert torch.equal(sa[k], sh[k]), k
    n = mk()
    fit.test(n, loader, ck)                            # default: no estimate
    assert n.tta_fisher_state() == {}
