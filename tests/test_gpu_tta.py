"""Test-time adaptation (TENT: Wang et al., ICLR 2021, "Tent: Fully Test-Time Adaptation by Entropy Minimization") in
STiLModel.test_step, the hook the reference leaves as a TODO (models/Disentangle/STiLModel.py:523-524).

1. stil_entropy_rows against float64 (close() at TOL of test_gpu_ops), ld > K views, sentinels, repetition.
2. The TTA step against TENT restated here in float64 on the oracle, on the device's ReLU / max-pool decisions.
3. No weight-gradient product runs in a TTA step.
4. Episodic mode and reset_tta().
5. `tta: True` without `tta_method` is exactly `tta: False`.
6. freeze() + torch.inference_mode().
7. fit.test takes the adapting path; the checkpoint load resets the TTA state.
tests/test_tta_cpu.py checks on the CPU that the inputs used here are well-conditioned (fp32 ATen meets the same bars)."""
import contextlib
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
from oracle.make_golden import randomize_state  # noqa: E402

# ------------------------------------------------------------------------------------------ the entropy entry point
ENT_ROWS = (1, 7, 512)
ENT_K = (1, 2, 286, 1000, 5000)
ENT_KINDS = ("uniform80", "tied", "spike60")
SENTINEL = -7.25


def entropy_cases():
    return [(r, k, kind) for r in ENT_ROWS for k in ENT_K for kind in ENT_KINDS]


def entropy_input(rows, K, kind, seed=0):
    """float32 logits [rows, K]: uniform in +-80 / every logit tied / one logit 60 above the rest (uniform in +-1)."""
    g = torch.Generator().manual_seed(seed + 1000 * rows + K)
    if kind == "uniform80":
        return (torch.rand(rows, K, generator=g) * 160.0 - 80.0).float()
    if kind == "tied":
        return torch.full((rows, K), 3.5, dtype=torch.float32)
    z = torch.rand(rows, K, generator=g) * 2.0 - 1.0
    z[torch.arange(rows), torch.randint(0, K, (rows,), generator=g)] += 60.0
    return z.float()


def entropy_ref(z, dtype):
    """TENT's loss with autograd in `dtype`: -> dict(loss, grad, probs, H, lse)."""
    x = z.detach().to(dtype).clone().requires_grad_(True)
    logp = torch.log_softmax(x, dim=1)
    p = logp.exp()
    H = -(p * logp).sum(dim=1)
    loss = H.mean()
    (g,) = torch.autograd.grad(loss, [x])
    return dict(loss=loss.detach(), grad=g, probs=p.detach(), H=H.detach(), lse=torch.logsumexp(x.detach(), dim=1))


@pytest.mark.parametrize("rows,K,kind", entropy_cases())
def test_entropy_rows_against_float64(rows, K, kind):
    from stil_tta_amd._lib import lib
    L = lib()
    z = entropy_input(rows, K, kind)
    ref = entropy_ref(z, torch.float64)
    gs = float(np.float32(1.0 / rows))
    for pad in (0, 3):
        ld = K + pad
        zb = torch.full((rows + 1, ld), SENTINEL, dtype=torch.float32)
        zb[:rows, :K] = z
        zb = zb.cuda()
        outs = []
        for rep in range(2):
            lse = torch.full((rows + 1,), SENTINEL, dtype=torch.float64, device="cuda")
            p = torch.full((rows + 1, ld), SENTINEL, device="cuda")
            H = torch.full((rows + 1,), SENTINEL, device="cuda")
            dZ = torch.full((rows + 1, ld), SENTINEL, device="cuda")
            mean = torch.full((2,), SENTINEL, device="cuda")
            L.entropy_rows(zb.data_ptr(), ld, rows, K, gs, lse.data_ptr(), p.data_ptr(), ld, H.data_ptr(), dZ.data_ptr(), ld,
                           mean.data_ptr(), None)
            torch.cuda.synchronize()
            outs.append((lse.cpu(), p.cpu(), H.cpu(), dZ.cpu(), mean.cpu()))
        lse, p, H, dZ, mean = outs[0]
        for a, b in zip(outs[0], outs[1]):
            assert torch.equal(a, b), "not bit-identical on repetition"
        # sentinels: the padding columns and the row past the end are untouched
        assert bool((p[rows] == SENTINEL).all() and (dZ[rows] == SENTINEL).all())
        assert float(H[rows]) == SENTINEL and float(lse[rows]) == SENTINEL and float(mean[1]) == SENTINEL
        if pad:
            assert bool((p[:, K:] == SENTINEL).all() and (dZ[:, K:] == SENTINEL).all())
        close(lse[:rows], ref["lse"], name="lse")
        close(p[:rows, :K], ref["probs"], name="probs")
        close(H[:rows], ref["H"], name="H")
        close(dZ[:rows, :K], ref["grad"] * (gs * rows), name="dZ")   # grad_scale as the float32 the kernel receives
        close(mean[:1], ref["loss"].view(1), name="mean")


def test_entropy_rows_rejects_bad_arguments():
    from stil_tta_amd._lib import lib
    L = lib()
    z = torch.zeros(4, 8, device="cuda")
    lse = torch.zeros(4, dtype=torch.float64, device="cuda")
    H = torch.zeros(4, device="cuda")
    mean = torch.zeros(1, device="cuda")
    fn = L._dll.stil_entropy_rows
    assert fn(z.data_ptr(), 7, 4, 8, 1.0, lse.data_ptr(), None, 8, H.data_ptr(), None, 8, mean.data_ptr(), None) != 0   # ld < K
    assert fn(z.data_ptr(), 8, 4, 0, 1.0, lse.data_ptr(), None, 8, H.data_ptr(), None, 8, mean.data_ptr(), None) != 0   # K = 0
    assert fn(z.data_ptr(), 8, 4, 8, 1.0, lse.data_ptr(), z.data_ptr(), 4, H.data_ptr(), None, 8, mean.data_ptr(), None) != 0  # ldp < K
    assert fn(z.data_ptr(), 8, 4, 8, 1.0, None, None, 8, H.data_ptr(), None, 8, mean.data_ptr(), None) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ models and batches
def dvm_hp(B, **over):
    """DVM-native: 128 px, 4 categorical + 13 continuous columns, K = 286."""
    return O.default_hparams(batch_size=B, **over)


def cardiac_hp(B, **over):
    """cardiac: K = 2, 26 categorical + 49 continuous = 75 columns, 128 px."""
    return O.default_hparams(batch_size=B, num_classes=2, target="CAD", field_lengths=[4] * 26 + [1] * 49, **over)


def initial_state(hp, seed):
    return randomize_state(O.init_state(hp, seed=seed), seed=seed + 1)


def tta_batch(hp, B, seed):
    """(x, y) of test_step: [image, tabular], labels (CPU)."""
    b = O.synthetic_batch(hp, B, seed=seed)
    img = torch.cat((b["l"][0][1], b["u"][0][1]))
    tab = torch.cat((b["l"][1][1], b["u"][1][1]))
    y = torch.cat((b["l"][2], b["u"][2]))
    return [img, tab], y


def make_model(hp, sd, **tta):
    from stil_tta_amd import STiLModel
    d = dict(vars(hp))
    d["mi_dropout"] = False
    d.update(tta)
    m = STiLModel(d)
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    m.setup_device("cuda")
    return m


def to_dev(batch):
    x, y = batch
    return [x[0].cuda(), x[1].cuda()], y.cuda()


def adapted_keys(m):
    return m.tta_param_names()


def device_grads(m):
    """the TTA gradients of A (state_dict names) left in the TTA gradient slab by the last adapted batch"""
    st = m._tent
    out = {}
    for n in m.tta_param_names():
        out[n] = st._slots[m.flat.names.index(n[len("model."):])].detach().cpu().double()
    return out


def full_state(m):
    """every device tensor a TTA step must leave alone outside A: state_dict (parameters, BN buffers, EMA teacher, prototypes)
    and the training Adam slabs"""
    f = m.flat
    out = {k: v.detach().clone() for k, v in m.state_dict().items()}
    out.update({"#exp_avg": f.exp_avg.clone(), "#exp_avg_sq": f.exp_avg_sq.clone(), "#steps": f.steps.clone(), "#ema": f.ema.clone()})
    return out


# ------------------------------------------------------------------------------------------ TENT restated (float64 oracle)
def tent_restated(sd, keys, x, hp, dtype, decisions=None):
    """TENT on one batch, on a deep copy of the state (the oracle updates running statistics in place):
    out_m of O.backbone_forward_all(train=True, masks=None), loss = mean row entropy of softmax(out_m), autograd w.r.t. A.
    -> (softmax(out_m), {key: gradient}, flips)"""
    s = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k in keys:
        s[k].requires_grad_(True)
    ctx = O.force_decisions(*decisions) if decisions is not None else contextlib.nullcontext()
    with ctx as d:
        out_m = O.backbone_forward_all(s, "model.", x[0].to(dtype), x[1].to(dtype), hp, train=True, masks=None)[0]
        logp = torch.log_softmax(out_m, dim=1)
        p = logp.exp()
        loss = -(p * logp).sum(dim=1).mean()
        g = torch.autograd.grad(loss, [s[k] for k in keys])
    flips = {t: v for t, v in d.get("flips", {}).items() if v[0]} if d is not None else {}
    return p.detach(), dict(zip(keys, [t.detach() for t in g])), flips


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


# (label, hparams, B, tta_params, batch seeds, state seed)
PARITY = [
    ("dvm_b64_bn_online", lambda: dvm_hp(64), 64, "bn", (201, 202), 11),
    ("dvm_b32_norm", lambda: dvm_hp(32), 32, "norm", (301,), 21),
    ("cardiac_b32_bn", lambda: cardiac_hp(32), 32, "bn", (401,), 31),
]


@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_tta_step_matches_tent_restated_in_float64(case):
    import test_gpu_step as S
    label, mk_hp, B, which, seeds, sseed = case
    hp = mk_hp()
    lr = 1e-3
    sd = initial_state(hp, sseed)
    m = make_model(hp, sd, tta=True, tta_method="tent", tta_params=which, tta_lr=lr)
    m.freeze()
    keys = adapted_keys(m)
    assert len(keys) == (106 if which == "bn" else 106 + 2 * (1 + 4 * 2) + 2 * 2)
    opt = {}
    bad = []
    for step, seed in enumerate(seeds, start=1):
        x, y = tta_batch(hp, B, seed)
        before = full_state(m)
        sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
        with S._trace_decisions() as trace:
            m.test_step(to_dev((x, y)), step - 1)
            torch.cuda.synchronize()
            decisions = S._device_decisions(m, trace)
        probs = m.last_tta["probs"].cpu().double()
        p64, g64, flips = tent_restated(sd_before, keys, x, hp, torch.float64, decisions)
        _, g64free, _ = tent_restated(sd_before, keys, x, hp, torch.float64)
        _, g32, _ = tent_restated(sd_before, keys, x, hp, torch.float32)
        S._check_flips(flips)
        d = S._scaled(probs.numpy(), p64.numpy())
        print(f"[{label}] batch {step}: predictions scaled error {d:.2e}; flips {({t: v[0] for t, v in flips.items()})}")
        if d > 3e-5:
            bad.append((step, "predictions", d))
        gd = device_grads(m)
        ratios = []
        for k in keys:
            e32 = _rel(g32[k].double(), g64free[k])
            err = _rel(gd[k], g64[k])
            ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
            if err > 3 * e32 + 1e-4:
                bad.append((step, "grad " + k, err, e32))
        print(f"[{label}] batch {step}: gradient error / (3*e32 + 1e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
        # Adam over A (fp32 oracle, its own moments) from the same parameters
        sd32 = {k: v.clone() for k, v in sd_before.items()}
        O.adam_step(sd32, g32, opt, step, lr)
        after = full_state(m)
        aset = set(keys)
        for k, v in after.items():
            if k in aset:
                dev = float((v.cpu() - sd32[k]).abs().max())
                if dev > 2.2 * lr * step:
                    bad.append((step, "adam " + k, dev))
            elif not torch.equal(v, before[k]):
                bad.append((step, "changed " + k))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


# ------------------------------------------------------------------------------------------ properties
def _small(which="bn", **tta):
    hp = dvm_hp(16, img_size=64)
    sd = initial_state(hp, 5)
    return hp, sd, (lambda: make_model(hp, sd, tta=True, tta_method="tent", tta_params=which, **tta))


@pytest.mark.parametrize("which", ["bn", "norm"])
def test_tta_step_issues_no_weight_gradient_product(which, monkeypatch):
    from stil_tta_amd._lib import lib
    from stil_tta_amd.driver import train_step
    from stil_tta_amd.flat import StilAdam
    hp, sd, mk = _small(which)
    m = mk()
    L = lib()
    calls = []
    for name in ("wgrad_tn", "wgrad_tn_partial"):
        orig = getattr(L, name)
        monkeypatch.setitem(L.__dict__, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    A0 = {k: v.clone() for k, v in m.state_dict().items() if k in set(adapted_keys(m))}
    m.test_step(to_dev(tta_batch(hp, 16, 7)), 0)
    torch.cuda.synchronize()
    assert calls == [], f"{len(calls)} weight-gradient launches in a TTA step"
    assert any(not torch.equal(m.state_dict()[k], v) for k, v in A0.items()), "the TTA step adapted nothing"
    # the counter sees the training step's products (control)
    t = mk()
    t.train()
    train_step(t, StilAdam(t.flat, lr=1e-4), _train_batch(hp))
    torch.cuda.synchronize()
    assert len(calls) > 0


def _train_batch(hp):
    b = O.synthetic_batch(hp, 16, seed=3)
    return {k: ([v[0][0].cuda(), v[0][1].cuda()], [v[1][0].cuda(), v[1][1].cuda()], v[2].cuda(), v[3].cuda(), v[4].cuda()) for k, v in b.items()}


def test_episodic_mode_and_reset():
    hp, sd, mk = _small(tta_episodic=True)
    b1, b2 = to_dev(tta_batch(hp, 16, 11)), to_dev(tta_batch(hp, 16, 12))
    m = mk()
    m.test_step(b1, 0)
    p2 = m.test_step(b2, 1).clone()
    s2 = full_state(m)
    f = mk()
    q2 = f.test_step(b2, 0).clone()
    t2 = full_state(f)
    assert torch.equal(p2, q2)
    for k in s2:
        assert torch.equal(s2[k], t2[k]), k
    # online: batch 2 sees batch 1's adaptation; reset_tta() restores A bit for bit
    _, _, mk_on = _small()
    o = mk_on()
    A0 = {k: v.clone() for k, v in o.state_dict().items() if k in set(adapted_keys(o))}
    o.test_step(b1, 0)
    r2 = o.test_step(b2, 1).clone()
    assert not torch.equal(r2, q2), "online batch 2 equals the episodic one: nothing carried over"
    o.reset_tta()
    for k, v in A0.items():
        assert torch.equal(o.state_dict()[k], v), k
    assert torch.equal(o.test_step(b2, 2), q2), "after reset_tta() the next batch starts from the source values and fresh moments"


def test_tta_true_without_method_is_tta_false():
    hp = dvm_hp(16, img_size=64)
    sd = initial_state(hp, 5)
    b = to_dev(tta_batch(hp, 16, 13))
    a = make_model(hp, sd, tta=True)
    c = make_model(hp, sd, tta=False)
    before = full_state(a)
    pa, pc = a.test_step(b, 0), c.test_step(b, 0)
    assert torch.equal(pa, pc)
    sa, sc = full_state(a), full_state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]) and torch.equal(sa[k], before[k]), k
    assert a._tent is None


def test_freeze_and_inference_mode():
    hp, sd, mk = _small()
    b = to_dev(tta_batch(hp, 16, 14))
    a, c = mk(), mk()
    a.freeze()
    c.freeze()
    with torch.inference_mode():
        pa = a.test_step(b, 0)
    pc = c.test_step(b, 0)
    assert torch.equal(pa, pc)
    sa, sc = full_state(a), full_state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert any(not torch.equal(sa[k], v) for k, v in full_state(mk()).items() if k in set(adapted_keys(a)))
    assert not any(q.requires_grad for q in a.parameters()) and not any(q.requires_grad for q in c.parameters())


def test_fit_test_takes_the_adapting_path(tmp_path):
    from stil_tta_amd import fit
    hp, sd, mk = _small()
    loader = [tta_batch(hp, 16, 20 + i) for i in range(3)]
    ck = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": {k: v.clone() for k, v in sd.items()}}, ck)
    a = mk()
    a.test_step(to_dev(loader[0]), 0)          # TTA state from an earlier run: the checkpoint load must discard it
    a.load_state_dict({k: v.cuda() for k, v in initial_state(hp, 77).items()})
    a.test_step(to_dev(loader[1]), 0)
    ra = fit.test(a, loader, ck)
    h = mk()
    h.freeze()
    h.acc_test.reset()
    h.auc_test.reset()
    for i, bt in enumerate(loader):
        h.test_step(to_dev(bt), i)
    rh = {k: float(v) for k, v in h.test_epoch_end().items()}
    assert ra.keys() == rh.keys() and all(ra[k] == rh[k] or (ra[k] != ra[k] and rh[k] != rh[k]) for k in ra), (ra, rh)
    sa, sh = full_state(a), full_state(h)
    for k in sa:
        assert torch.equal(sa[k], sh[k]), k
    off = make_model(hp, sd, tta=True)
    fit.test(off, loader, ck)
    so = full_state(off)
    assert any(not torch.equal(so[k], sa[k]) for k in adapted_keys(a)), "fit.test with TTA left A where the run without TTA leaves it"
