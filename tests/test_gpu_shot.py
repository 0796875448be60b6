"""SHOT-IM test-time adaptation (Liang et al., ICML 2020, "Do We Really Need to Access the Source Data?"; the SHOT-IM baseline of
the TENT paper) in STiLModel.test_step: row entropy minus the entropy of the batch-mean prediction, on top of TENT
(tests/test_gpu_tta.py).

1. stil_infomax_rows against float64 autograd (close() at TOL of test_gpu_ops), ld = K + 3 views, sentinels, repetition; K = 1.
2. div_weight = 0 is stil_entropy_rows bit for bit; lse, p, H and the mean entropy are for every weight.
3. Bad arguments are refused.
4. The step against SHOT-IM restated here in float64 on the oracle, on the device's ReLU / max-pool decisions.
5. tta_div_weight = 0 is tta_method "tent" bit for bit, with and without tta_bn_prior.
6. The properties of a TENT step, re-checked with tta_method "shot_im".
tests/test_shot_cpu.py checks on the CPU that the inputs used here are well-conditioned (fp32 ATen and the fp32 oracle meet the
same bars)."""
import contextlib
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_gpu_ops import TOL, close  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
import test_gpu_tta as T  # noqa: E402

SENTINEL = -7.25
ROWS = (1, 7, 130, 512)          # 130, 512: the column means run across more than one workgroup of rows
KS = (1, 2, 286, 1000, 5000)
KINDS = ("uniform80", "tied", "spike60", "one_class", "mild")
LAMBDAS = (1.0, 0.3)
EPS = 1e-5


def f32(v):
    """v as the float32 the C ABI receives"""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------ check 1: the entry point
def shot_cases():
    return [(r, k, kind, lam) for r in ROWS for k in KS for kind in KINDS for lam in LAMBDAS]


def shot_input(rows, K, kind, seed=0):
    """float32 logits [rows, K]: T.entropy_input's three kinds, and with its seeding
    one_class: uniform in +-1 with +60 on column K // 2 of EVERY row (the collapsed batch: every other pbar[k] << eps);
    mild: 3 x uniform in +-1."""
    if kind in T.ENT_KINDS:
        return T.entropy_input(rows, K, kind, seed)
    g = torch.Generator().manual_seed(seed + 1000 * rows + K)
    z = torch.rand(rows, K, generator=g) * 2.0 - 1.0
    if kind == "one_class":
        z[:, K // 2] += 60.0
    else:
        z = z * 3.0
    return z.float()


def shot_loss(out_m, lam, eps):
    """SHOT's information-maximisation loss of logits, with the exact row entropy (lam = 0 is TENT's loss).
    -> (loss, mean row entropy, D, log p, row entropies, mean prediction)"""
    logp = torch.log_softmax(out_m, dim=1)
    p = logp.exp()
    H = -(p * logp).sum(dim=1)
    pbar = p.mean(dim=0)
    D = (pbar * torch.log(pbar + eps)).sum()
    ent = H.mean()
    return ent + lam * D, ent, D, logp, H, pbar


def shot_ref(z, lam, eps, dtype):
    """The loss with autograd in `dtype`: -> dict(loss, ent, D, grad, probs, H, lse, pbar)."""
    x = z.detach().to(dtype).clone().requires_grad_(True)
    loss, ent, D, logp, H, pbar = shot_loss(x, lam, eps)
    (g,) = torch.autograd.grad(loss, [x])
    return dict(loss=loss.detach(), ent=ent.detach(), D=D.detach(), grad=g, probs=logp.exp().detach(), H=H.detach(),
                lse=torch.logsumexp(x.detach(), dim=1), pbar=pbar.detach())


@functools.lru_cache(maxsize=None)
def shot_ref64(rows, K, kind, lam):
    """the float64 reference of one case, computed once (read-only), at the weight and eps the kernel receives"""
    return shot_ref(shot_input(rows, K, kind), f32(lam), f32(EPS), torch.float64)


def _run_infomax(L, zb, ld, rows, K, gs, lam, eps, dz=True):
    dev = "cuda"
    o = dict(lse=torch.full((rows + 1,), SENTINEL, dtype=torch.float64, device=dev), p=torch.full((rows + 1, ld), SENTINEL, device=dev),
             H=torch.full((rows + 1,), SENTINEL, device=dev), pbar=torch.full((K + 1,), SENTINEL, device=dev),
             dZ=torch.full((rows + 1, ld), SENTINEL, device=dev), out=torch.full((4,), SENTINEL, device=dev),
             ws=torch.full((2 * K + rows + 1,), SENTINEL, dtype=torch.float64, device=dev))   # not cleared: written before it is read
    L.infomax_rows(zb.data_ptr(), ld, rows, K, gs, lam, eps, o["lse"].data_ptr(), o["p"].data_ptr(), ld, o["H"].data_ptr(),
                   o["pbar"].data_ptr(), o["dZ"].data_ptr() if dz else None, ld, o["out"].data_ptr(), o["ws"].data_ptr(), None)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _run_entropy(L, zb, ld, rows, K, gs):
    lse = torch.empty(rows, dtype=torch.float64, device="cuda")
    p = torch.empty(rows, ld, device="cuda")
    H = torch.empty(rows, device="cuda")
    dZ = torch.empty(rows, ld, device="cuda")
    mean = torch.empty(1, device="cuda")
    L.entropy_rows(zb.data_ptr(), ld, rows, K, gs, lse.data_ptr(), p.data_ptr(), ld, H.data_ptr(), dZ.data_ptr(), ld, mean.data_ptr(), None)
    torch.cuda.synchronize()
    return dict(lse=lse.cpu(), p=p.cpu()[:, :K], H=H.cpu(), dZ=dZ.cpu()[:, :K], mean=mean.cpu())


def _padded(z, rows, K, pad):
    zb = torch.full((rows + 1, K + pad), SENTINEL, dtype=torch.float32)
    zb[:rows, :K] = z
    return zb.cuda()


@pytest.mark.parametrize("rows,K,kind,lam", shot_cases())
def test_infomax_rows_against_float64(rows, K, kind, lam):
    from stil_tta_amd._lib import lib
    L = lib()
    z = shot_input(rows, K, kind)
    ref = shot_ref64(rows, K, kind, lam)
    gs, lam32, eps32 = f32(1.0 / rows), f32(lam), f32(EPS)
    for pad in (0, 3):
        ld = K + pad
        zb = _padded(z, rows, K, pad)
        a, b = (_run_infomax(L, zb, ld, rows, K, gs, lam32, eps32) for _ in range(2))
        for k in a:
            if k != "ws":
                assert torch.equal(a[k], b[k]), f"{k}: not bit-identical on repetition"
        # sentinels: padding columns, the row past the end, the element past every vector
        assert bool((a["p"][rows] == SENTINEL).all() and (a["dZ"][rows] == SENTINEL).all())
        assert float(a["H"][rows]) == SENTINEL and float(a["lse"][rows]) == SENTINEL and float(a["pbar"][K]) == SENTINEL
        assert float(a["out"][3]) == SENTINEL and float(a["ws"][2 * K + rows]) == SENTINEL
        if pad:
            assert bool((a["p"][:, K:] == SENTINEL).all() and (a["dZ"][:, K:] == SENTINEL).all())
        close(a["lse"][:rows], ref["lse"], name="lse")
        close(a["p"][:rows, :K], ref["probs"], name="probs")
        close(a["H"][:rows], ref["H"], name="H")
        close(a["pbar"][:K], ref["pbar"], name="pbar")
        close(a["dZ"][:rows, :K], ref["grad"] * (gs * rows), name="dZ")   # grad_scale as the float32 the kernel receives
        close(a["out"][0:1], ref["loss"].view(1), name="out[0]")
        close(a["out"][1:2], ref["ent"].view(1), name="out[1]")
        close(a["out"][2:3], ref["D"].view(1), name="out[2]")
        if K == 1:
            # one class: p = 1 exactly, so dZ = 0 and D = log(1 + eps) to the rounding of a float32 of that size (2^-41) and the
            # double logarithm's
            assert bool((a["dZ"][:rows, :K] == 0).all())
            assert abs(float(a["out"][2]) - math.log1p(eps32)) <= 1e-12
        # tie to TENT's kernel for every weight: lse, p, H and the mean row entropy bit for bit
        t = _run_entropy(L, zb, ld, rows, K, gs)
        assert torch.equal(a["lse"][:rows], t["lse"]) and torch.equal(a["H"][:rows], t["H"]) and torch.equal(a["p"][:rows, :K], t["p"])
        assert torch.equal(a["out"][1:2], t["mean"])
    # dZ == NULL: the other outputs are unchanged
    c = _run_infomax(L, zb, ld, rows, K, gs, lam32, eps32, dz=False)
    assert bool((c["dZ"] == SENTINEL).all())
    for k in ("lse", "p", "H", "pbar", "out"):
        assert torch.equal(c[k], a[k]), k


# ------------------------------------------------------------------------------------------ check 2: div_weight = 0
@pytest.mark.parametrize("rows,K,kind", [(r, k, kind) for r in ROWS for k in KS for kind in KINDS])
def test_zero_weight_is_entropy_rows_bit_for_bit(rows, K, kind):
    from stil_tta_amd._lib import lib
    L = lib()
    z = shot_input(rows, K, kind)
    gs = f32(1.0 / rows)
    for pad in (0, 3):
        ld = K + pad
        zb = _padded(z, rows, K, pad)
        a = _run_infomax(L, zb, ld, rows, K, gs, 0.0, f32(EPS))
        t = _run_entropy(L, zb, ld, rows, K, gs)
        assert torch.equal(a["lse"][:rows], t["lse"]) and torch.equal(a["H"][:rows], t["H"])
        assert torch.equal(a["p"][:rows, :K], t["p"]) and torch.equal(a["dZ"][:rows, :K], t["dZ"])
        assert torch.equal(a["out"][0:1], t["mean"]) and torch.equal(a["out"][1:2], t["mean"])


# ------------------------------------------------------------------------------------------ check 3: bad arguments
def test_infomax_rows_rejects_bad_arguments():
    from stil_tta_amd._lib import lib
    fn = lib()._dll.stil_infomax_rows
    z, p, dz = (torch.zeros(4, 8, device="cuda") for _ in range(3))
    lse = torch.zeros(4, dtype=torch.float64, device="cuda")
    H = torch.zeros(4, device="cuda")
    pbar = torch.zeros(8, device="cuda")
    out = torch.zeros(3, device="cuda")
    ws = torch.zeros(2 * 8 + 4, dtype=torch.float64, device="cuda")
    ptr = dict(z=z, lse=lse, p=p, H=H, pbar=pbar, dz=dz, out=out, ws=ws)

    def call(ld=8, rows=4, K=8, ldp=8, ldd=8, lam=1.0, eps=1e-5, null=()):
        q = {k: (None if k in null else v.data_ptr()) for k, v in ptr.items()}
        c32 = ctypes.c_float
        return fn(q["z"], ld, rows, K, c32(0.25), c32(lam), c32(eps), q["lse"], q["p"], ldp, q["H"], q["pbar"], q["dz"], ldd, q["out"], q["ws"], None)
    assert call() == 0
    assert call(null=("p",)) == 0 and call(null=("dz",)) == 0 and call(null=("p", "dz"), ldp=0, ldd=0) == 0   # optional outputs
    for k in ("z", "lse", "H", "pbar", "out", "ws"):
        assert call(null=(k,)) < 0, k
    assert call(rows=0) < 0 and call(K=0) < 0 and call(rows=-1) < 0
    assert call(ld=7) < 0 and call(ldp=7) < 0 and call(ldd=7) < 0
    for bad in (0.0, -1e-5, float("inf"), float("nan")):
        assert call(eps=bad) < 0, bad
    for bad in (-0.5, float("inf"), float("-inf"), float("nan")):
        assert call(lam=bad) < 0, bad
    assert call(lam=0.0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ check 4: the step, restated
HEAD_SCALE = 8.0    # the random states give near-uniform rows; x16 and x32 put the fp32 oracle itself past the 3e-5 prediction bar


def parity_state(hp, sseed, head_scale):
    sd = T.initial_state(hp, sseed)
    if head_scale is not None:
        k = "model.classifier_multimodal.weight"
        sd[k] = sd[k] * head_scale
    return sd


def shot_restated(sd, keys, x, hp, dtype, lam, eps, decisions=None):
    """SHOT-IM on one batch, on a deep copy of the state (the oracle updates running statistics in place):
    out_m of O.backbone_forward_all(train=True, masks=None), shot_loss, autograd w.r.t. A.
    -> dict(p, g {key: gradient}, flips, l_ent, D, pbar)"""
    s = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k in keys:
        s[k].requires_grad_(True)
    ctx = O.force_decisions(*decisions) if decisions is not None else contextlib.nullcontext()
    with ctx as d:
        out_m = O.backbone_forward_all(s, "model.", x[0].to(dtype), x[1].to(dtype), hp, train=True, masks=None)[0]
        loss, ent, D, logp, _, pbar = shot_loss(out_m, lam, eps)
        g = torch.autograd.grad(loss, [s[k] for k in keys])
    flips = {t: v for t, v in d.get("flips", {}).items() if v[0]} if d is not None else {}
    return dict(p=logp.exp().detach(), g=dict(zip(keys, [t.detach() for t in g])), flips=flips, l_ent=ent.detach(), D=D.detach(),
                pbar=pbar.detach())


# (label, hparams, B, tta_params, batch seeds (online), state seed, head scale)
PARITY = [
    ("dvm64_b16_x8", lambda: T.dvm_hp(16, img_size=64), 16, "bn", (501, 502), 41, HEAD_SCALE),
    ("cardiac64_b16_norm", lambda: T.cardiac_hp(16, img_size=64), 16, "norm", (601,), 51, None),
]
PARITY_LR = 1e-3


@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_shot_im_step_matches_shot_im_restated_in_float64(case):
    """Bars are TENT's (tests/test_gpu_tta.py): predictions <= 3e-5 scaled, every gradient of A <= 3 e32 + 1e-4, Adam within
    2.2 lr step, everything outside A bit-identical; the two loss values within close() at TOL of float64."""
    import test_gpu_step as S
    label, mk_hp, B, which, seeds, sseed, head = case
    hp = mk_hp()
    lr = PARITY_LR
    sd = parity_state(hp, sseed, head)
    m = T.make_model(hp, sd, tta=True, tta_method="shot_im", tta_params=which, tta_lr=lr)
    m.freeze()
    lam, eps = m.hp.tta_div_weight, m.hp.tta_div_eps
    assert (lam, eps) == (1.0, 1e-5)
    keys = T.adapted_keys(m)
    assert len(keys) == (106 if which == "bn" else 106 + 2 * (1 + 4 * 2) + 2 * 2)
    opt = {}
    bad = []
    for step, seed in enumerate(seeds, start=1):
        x, y = T.tta_batch(hp, B, seed)
        before = T.full_state(m)
        sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
        with S._trace_decisions() as trace:
            m.test_step(T.to_dev((x, y)), step - 1)
            torch.cuda.synchronize()
            decisions = S._device_decisions(m, trace)
        lt = m.last_tta
        probs = lt["probs"].cpu().double()
        r64 = shot_restated(sd_before, keys, x, hp, torch.float64, lam, eps, decisions)
        r64free = shot_restated(sd_before, keys, x, hp, torch.float64, lam, eps)
        r32 = shot_restated(sd_before, keys, x, hp, torch.float32, lam, eps)
        S._check_flips(r64["flips"])
        d = S._scaled(probs.numpy(), r64["p"].numpy())
        print(f"[{label}] batch {step}: predictions scaled error {d:.2e}; flips {({t: v[0] for t, v in r64['flips'].items()})}")
        if d > 3e-5:
            bad.append((step, "predictions", d))
        for name, got, want in (("loss_entropy", lt["loss_entropy"], r64["l_ent"]), ("loss_diversity", lt["loss_diversity"], r64["D"])):
            got, want = float(got), float(want)
            ratio = abs(got - want) / (TOL * (1.0 + 2.0 * abs(want)))
            print(f"[{label}] batch {step}: {name} {got:.6f} (float64 {want:.6f}), error / close() bound {ratio:.3f}")
        close(lt["loss_entropy"].view(1), r64["l_ent"].view(1), name="loss_entropy")
        close(lt["loss_diversity"].view(1), r64["D"].view(1), name="loss_diversity")
        close(lt["loss"].view(1), (r64["l_ent"] + lam * r64["D"]).view(1), name="loss")
        close(lt["marginal"], r64["pbar"], name="marginal")
        close(lt["probs"], torch.softmax(lt["y_hat_m"].double(), dim=1), name="probs against softmax(y_hat_m)")
        gd = T.device_grads(m)
        ratios = []
        for k in keys:
            e32 = T._rel(r32["g"][k].double(), r64free["g"][k])
            err = T._rel(gd[k], r64["g"][k])
            ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
            if err > 3 * e32 + 1e-4:
                bad.append((step, "grad " + k, err, e32))
        print(f"[{label}] batch {step}: gradient error / (3*e32 + 1e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
        # Adam over A (fp32 oracle, its own moments) from the same parameters
        sd32 = {k: v.clone() for k, v in sd_before.items()}
        O.adam_step(sd32, r32["g"], opt, step, lr)
        after = T.full_state(m)
        aset = set(keys)
        worst_adam = 0.0
        for k, v in after.items():
            if k in aset:
                dev = float((v.cpu() - sd32[k]).abs().max())
                worst_adam = max(worst_adam, dev / (2.2 * lr * step))
                if dev > 2.2 * lr * step:
                    bad.append((step, "adam " + k, dev))
            elif not torch.equal(v, before[k]):
                bad.append((step, "changed " + k))
        print(f"[{label}] batch {step}: Adam deviation / (2.2 lr step), worst: {worst_adam:.3f}")
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


# ------------------------------------------------------------------------------------------ check 5: weight 0 is TENT
def _small(which="bn", method="shot_im", **tta):
    hp = T.dvm_hp(16, img_size=64)
    sd = T.initial_state(hp, 5)
    return hp, sd, (lambda: T.make_model(hp, sd, tta=True, tta_method=method, tta_params=which, **tta))


def _adapt_state(m):
    st = m._tent
    out = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    out.update({"#tta_exp_avg": st.exp_avg.clone(), "#tta_exp_avg_sq": st.exp_avg_sq.clone(), "#tta_steps": st.steps.clone()})
    return out


@pytest.mark.parametrize("prior", [None, 16])
def test_zero_div_weight_is_tent_bit_for_bit(prior):
    hp, sd, mk0 = _small(tta_div_weight=0.0, tta_bn_prior=prior)
    _, _, mkt = _small(method="tent", tta_bn_prior=prior)
    _, _, mk1 = _small(tta_div_weight=1.0, tta_bn_prior=prior)
    batches = [T.to_dev(T.tta_batch(hp, 16, 11)), T.to_dev(T.tta_batch(hp, 16, 12))]
    s, t, w = mk0(), mkt(), mk1()
    for i, b in enumerate(batches):
        ps, pt = s.test_step(b, i), t.test_step(b, i)
        assert torch.equal(ps, pt) and torch.equal(s.last_tta["probs"], t.last_tta["probs"]), f"batch {i}: scores"
        assert torch.equal(s.last_tta["loss"], t.last_tta["loss"]) and torch.equal(s.last_tta["y_hat_m"], t.last_tta["y_hat_m"])
        a, c = _adapt_state(s), _adapt_state(t)
        assert a.keys() == c.keys()
        for k in a:
            assert torch.equal(a[k], c[k]), f"batch {i}: {k}"
        assert int(s._tent.steps.max()) == i + 1
    w.test_step(batches[0], 0)
    aw = _adapt_state(w)
    t1 = mkt()
    t1.test_step(batches[0], 0)
    c1 = _adapt_state(t1)
    assert any(not torch.equal(aw[k], c1[k]) for k in T.adapted_keys(w)), "tta_div_weight = 1 left A where TENT leaves it"


# ------------------------------------------------------------------------------------------ check 6: inherited properties
@pytest.mark.parametrize("which", ["bn", "norm"])
def test_shot_im_step_issues_no_weight_gradient_product(which, monkeypatch):
    from stil_tta_amd._lib import lib
    hp, sd, mk = _small(which)
    m = mk()
    L = lib()
    calls = []
    for name in ("wgrad_tn", "wgrad_tn_partial"):
        orig = getattr(L, name)
        monkeypatch.setitem(L.__dict__, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    A0 = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    m.test_step(T.to_dev(T.tta_batch(hp, 16, 7)), 0)
    torch.cuda.synchronize()
    assert calls == [], f"{len(calls)} weight-gradient launches in a SHOT-IM step"
    assert any(not torch.equal(m.state_dict()[k], v) for k, v in A0.items()), "the SHOT-IM step adapted nothing"


def test_episodic_mode_and_reset():
    hp, sd, mk = _small(tta_episodic=True)
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, 11)), T.to_dev(T.tta_batch(hp, 16, 12))
    m = mk()
    m.test_step(b1, 0)
    p2 = m.test_step(b2, 1).clone()
    s2 = T.full_state(m)
    f = mk()
    q2 = f.test_step(b2, 0).clone()
    t2 = T.full_state(f)
    assert torch.equal(p2, q2)
    for k in s2:
        assert torch.equal(s2[k], t2[k]), k
    # online: batch 2 sees batch 1's adaptation; reset_tta() restores A bit for bit
    _, _, mk_on = _small()
    o = mk_on()
    A0 = {k: v.clone() for k, v in o.state_dict().items() if k in set(T.adapted_keys(o))}
    o.test_step(b1, 0)
    r2 = o.test_step(b2, 1).clone()
    assert not torch.equal(r2, q2), "online batch 2 equals the episodic one: nothing carried over"
    o.reset_tta()
    for k, v in A0.items():
        assert torch.equal(o.state_dict()[k], v), k
    assert torch.equal(o.test_step(b2, 2), q2), "after reset_tta() the next batch starts from the source values and fresh moments"


def test_freeze_and_inference_mode():
    hp, sd, mk = _small()
    b = T.to_dev(T.tta_batch(hp, 16, 14))
    a, c = mk(), mk()
    a.freeze()
    c.freeze()
    with torch.inference_mode():
        pa = a.test_step(b, 0)
    pc = c.test_step(b, 0)
    assert torch.equal(pa, pc)
    sa, sc = T.full_state(a), T.full_state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert any(not torch.equal(sa[k], v) for k, v in T.full_state(mk()).items() if k in set(T.adapted_keys(a)))
    assert not any(q.requires_grad for q in a.parameters()) and not any(q.requires_grad for q in c.parameters())


def test_fit_test_takes_the_adapting_path(tmp_path):
    from stil_tta_amd import fit
    hp, sd, mk = _small()
    loader = [T.tta_batch(hp, 16, 20 + i) for i in range(3)]
    ck = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": {k: v.clone() for k, v in sd.items()}}, ck)
    a = mk()
    a.test_step(T.to_dev(loader[0]), 0)          # adaptation state from an earlier run: the checkpoint load must discard it
    a.load_state_dict({k: v.cuda() for k, v in T.initial_state(hp, 77).items()})
    assert a._tent is None
    a.test_step(T.to_dev(loader[1]), 0)
    ra = fit.test(a, loader, ck)
    h = mk()
    h.freeze()
    h.acc_test.reset()
    h.auc_test.reset()
    for i, bt in enumerate(loader):
        h.test_step(T.to_dev(bt), i)
    rh = {k: float(v) for k, v in h.test_epoch_end().items()}
    assert ra.keys() == rh.keys() and all(ra[k] == rh[k] or (ra[k] != ra[k] and rh[k] != rh[k]) for k in ra), (ra, rh)
    sa, sh = T.full_state(a), T.full_state(h)
    for k in sa:
        assert torch.equal(sa[k], sh[k]), k
    off = T.make_model(hp, sd, tta=True)
    fit.test(off, loader, ck)
    so = T.full_state(off)
    assert any(not torch.equal(so[k], sa[k]) for k in T.adapted_keys(a)), "fit.test with SHOT-IM left A where the run without TTA leaves it"


def test_ragged_last_batch():
    hp, sd, mk = _small()
    m = mk()
    m.test_step(T.to_dev(T.tta_batch(hp, 16, 11)), 0)
    A1 = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    p = m.test_step(T.to_dev(T.tta_batch(hp, 5, 12)), 1)
    torch.cuda.synchronize()
    lt = m.last_tta
    assert p.shape == (5, hp.num_classes) and lt["probs"].shape == (5, hp.num_classes) and lt["marginal"].shape == (hp.num_classes,)
    for k in ("loss", "loss_entropy", "loss_diversity", "marginal", "probs"):
        assert lt[k].is_cuda and bool(torch.isfinite(lt[k]).all()), k
    close(lt["marginal"].sum().view(1), torch.ones(1), name="sum of the marginal")
    close(lt["marginal"], lt["probs"].double().mean(0), name="marginal against the mean of probs")
    assert int(m._tent.steps.max()) == 2
    assert any(not torch.equal(m.state_dict()[k], v) for k, v in A1.items()), "the short batch adapted nothing"
