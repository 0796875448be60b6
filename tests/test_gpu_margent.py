"""Marginal-entropy test-time adaptation over augmented views (MEMO: Zhang, Levine, Finn, NeurIPS 2022, "MEMO: Test Time Robustness
via Adaptation and Augmentation") in STiLModel.test_step, on top of TENT (tests/test_gpu_tta.py).

1. stil_marginal_entropy_groups against float64 autograd (close() at TOL of test_gpu_ops), ld = K + 3 views, sentinels, repetition;
   lse and p are stil_entropy_rows' bit for bit; views == 1 is stil_entropy_rows at TOL.
2. Bad arguments are refused and nothing is written.
3. The step against the contract restated here in float64 on the oracle: the adapting pass on the views rebuilt from the recorded
   draws (the device's ReLU / max-pool decisions), Adam, and the scoring forward on the clean batch from the updated state.
4. The properties of a TENT step, re-checked with tta_method "marginal_entropy", and what is new: the views' generator.
tests/test_margent_cpu.py checks on the CPU that the inputs used here are well-conditioned (fp32 ATen and the fp32 oracle meet the
same bars) and that the views are informative (the loss is not row entropy in disguise).

Measured on an MI355X (the step test prints these), as fractions of each bar, batches 1 / 2:
    dvm64_b2_v8_x8     loss 0.003 / 0.002, marginal 0.031 / 0.013, marginal_entropy 0.007 / 0.001 of the close() bound; worst
                       gradient 0.131 / 0.0022 of 3 e32 + 1e-4; Adam 0.909 / 0.081 of 2.2 lr step; predictions 6.1e-7 / 2.4e-7 (bar 3e-5)
    cardiac64_b1_v16   loss, marginal, marginal_entropy <= 0.002; worst gradient 0.100 / 0.145; Adam 0.909 / 0.909 (episodic: both
                       are first steps); predictions 1.4e-8 / 4.0e-8"""
import contextlib
import ctypes
import functools
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
import test_gpu_tta as T  # noqa: E402
from test_gpu_bnprior import blended_oracle  # noqa: E402

SENTINEL = -7.25
GV = ((1, 1), (1, 8), (3, 2), (5, 33), (64, 4), (2, 300))   # (2, 300): more views than a workgroup has threads
KS = (1, 2, 286, 1000, 5000)                                 # 286, 1000, 5000: more columns than a workgroup has threads
KINDS = ("uniform80", "tied", "mild", "spike60", "views_disagree", "views_agree")


def f32(v):
    """v as the float32 the C ABI receives"""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------ check 1: the entry point
def margent_cases():
    return [(g, v, k, kind) for g, v in GV for k in KS for kind in KINDS]


def margent_input(G, V, K, kind, seed=0):
    """float32 logits [G V, K], row g V + v = view v of sample g: T.entropy_input's three kinds, and with its seeding
    mild: 3 x uniform in +-1;
    views_disagree: uniform in +-1 with +12 on class (g + v) % K of view v (confident rows, a spread marginal);
    views_agree: uniform in +-1 with +12 on class g % K of every view of sample g (confident rows, a confident marginal)."""
    rows = G * V
    if kind in T.ENT_KINDS:
        return T.entropy_input(rows, K, kind, seed)
    g = torch.Generator().manual_seed(seed + 1000 * rows + K)
    z = torch.rand(rows, K, generator=g) * 2.0 - 1.0
    if kind == "mild":
        return (z * 3.0).float()
    r = torch.arange(rows)
    cls = (r // V + (r % V if kind == "views_disagree" else 0)) % K
    z[r, cls] += 12.0
    return z.float()


def margent_loss(out_m, G, V):
    """MEMO's loss of logits [G V, K] in log-sum-exp form -> (loss, log p, log pbar [G, K], Hbar [G])"""
    logp = torch.log_softmax(out_m, dim=1)
    logpbar = torch.logsumexp(logp.view(G, V, -1), dim=1) - math.log(V)
    Hbar = -(logpbar.exp() * logpbar).sum(dim=1)
    return Hbar.mean(), logp, logpbar, Hbar


def margent_ref(z, G, V, dtype):
    """The loss with autograd in `dtype`: -> dict(loss, grad, probs, lse, pbar, Hbar)."""
    x = z.detach().to(dtype).clone().requires_grad_(True)
    loss, logp, logpbar, Hbar = margent_loss(x, G, V)
    (g,) = torch.autograd.grad(loss, [x])
    return dict(loss=loss.detach(), grad=g, probs=logp.exp().detach(), lse=torch.logsumexp(x.detach(), dim=1),
                pbar=logpbar.exp().detach(), Hbar=Hbar.detach())


@functools.lru_cache(maxsize=None)
def margent_ref64(G, V, K, kind):
    """the float64 reference of one case, computed once (read-only)"""
    return margent_ref(margent_input(G, V, K, kind), G, V, torch.float64)


def ws_doubles(G, K):
    return G * (K + (K + 255) // 256)


def _run_margent(L, zb, ld, G, V, K, gs, dz=True, p=True):
    dev = "cuda"
    rows = G * V
    o = dict(lse=torch.full((rows + 1,), SENTINEL, dtype=torch.float64, device=dev), p=torch.full((rows + 1, ld), SENTINEL, device=dev),
             pbar=torch.full((G + 1, ld), SENTINEL, device=dev), Hbar=torch.full((G + 1,), SENTINEL, device=dev),
             dZ=torch.full((rows + 1, ld), SENTINEL, device=dev), out=torch.full((2,), SENTINEL, device=dev),
             ws=torch.full((ws_doubles(G, K) + 1,), SENTINEL, dtype=torch.float64, device=dev))   # not cleared: written before it is read
    L.marginal_entropy_groups(zb.data_ptr(), ld, G, V, K, gs, o["lse"].data_ptr(), o["p"].data_ptr() if p else None, ld,
                              o["pbar"].data_ptr(), ld, o["Hbar"].data_ptr(), o["dZ"].data_ptr() if dz else None, ld,
                              o["out"].data_ptr(), o["ws"].data_ptr(), None)
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


@pytest.mark.parametrize("G,V,K,kind", margent_cases())
def test_marginal_entropy_groups_against_float64(G, V, K, kind):
    from stil_tta_amd._lib import lib
    L = lib()
    rows = G * V
    z = margent_input(G, V, K, kind)
    ref = margent_ref64(G, V, K, kind)
    gs = f32(1.0 / G)
    for pad in (0, 3):
        ld = K + pad
        zb = _padded(z, rows, K, pad)
        a, b = (_run_margent(L, zb, ld, G, V, K, gs) for _ in range(2))
        for k in a:
            if k != "ws":
                assert torch.equal(a[k], b[k]), f"{k}: not bit-identical on repetition"
        # sentinels: padding columns, the row / sample past the end, the element past every vector
        assert bool((a["p"][rows] == SENTINEL).all() and (a["dZ"][rows] == SENTINEL).all() and (a["pbar"][G] == SENTINEL).all())
        assert float(a["Hbar"][G]) == SENTINEL and float(a["lse"][rows]) == SENTINEL
        assert float(a["out"][1]) == SENTINEL and float(a["ws"][ws_doubles(G, K)]) == SENTINEL
        if pad:
            assert bool((a["p"][:, K:] == SENTINEL).all() and (a["dZ"][:, K:] == SENTINEL).all() and (a["pbar"][:, K:] == SENTINEL).all())
        assert bool(torch.isfinite(a["dZ"][:rows, :K]).all() and torch.isfinite(a["pbar"][:G, :K]).all())
        close(a["lse"][:rows], ref["lse"], name="lse")
        close(a["p"][:rows, :K], ref["probs"], name="probs")
        close(a["pbar"][:G, :K], ref["pbar"], name="pbar")
        close(a["Hbar"][:G], ref["Hbar"], name="Hbar")
        close(a["dZ"][:rows, :K], ref["grad"] * (gs * G), name="dZ")   # grad_scale as the float32 the kernel receives
        close(a["out"][0:1], ref["loss"].view(1), name="out[0]")
        if K == 1:
            assert bool((a["dZ"][:rows, :K] == 0).all() and (a["pbar"][:G, :K] == 1).all() and (a["Hbar"][:G] == 0).all())
        # tie to TENT's kernel: lse and p bit for bit; with one view per sample Hbar and dZ are its H and dZ
        t = _run_entropy(L, zb, ld, rows, K, f32(1.0 / rows))
        assert torch.equal(a["lse"][:rows], t["lse"]) and torch.equal(a["p"][:rows, :K], t["p"])
        if V == 1:
            close(a["Hbar"][:G], t["H"].double(), name="Hbar against stil_entropy_rows' H")
            close(a["dZ"][:rows, :K], t["dZ"].double(), name="dZ against stil_entropy_rows' dZ")
            close(a["out"][0:1], t["mean"].double(), name="out[0] against stil_entropy_rows' mean")
    # p == NULL, dZ == NULL: the other outputs are unchanged
    c = _run_margent(L, zb, ld, G, V, K, gs, dz=False, p=False)
    assert bool((c["dZ"] == SENTINEL).all() and (c["p"] == SENTINEL).all())
    for k in ("lse", "pbar", "Hbar", "out"):
        assert torch.equal(c[k], a[k]), k


# ------------------------------------------------------------------------------------------ check 2: bad arguments
def test_marginal_entropy_groups_rejects_bad_arguments():
    from stil_tta_amd._lib import lib
    fn = lib()._dll.stil_marginal_entropy_groups
    G, V, K = 2, 3, 8
    z = torch.zeros(G * V, K, device="cuda")
    new = dict(lse=lambda: torch.full((G * V,), SENTINEL, dtype=torch.float64, device="cuda"), p=lambda: torch.full((G * V, K), SENTINEL, device="cuda"),
               pbar=lambda: torch.full((G, K), SENTINEL, device="cuda"), Hbar=lambda: torch.full((G,), SENTINEL, device="cuda"),
               dz=lambda: torch.full((G * V, K), SENTINEL, device="cuda"), out=lambda: torch.full((1,), SENTINEL, device="cuda"),
               ws=lambda: torch.full((ws_doubles(G, K),), SENTINEL, dtype=torch.float64, device="cuda"))
    ptr = {k: f() for k, f in new.items()}

    def call(ld=K, groups=G, views=V, k=K, ldp=K, ldb=K, ldd=K, null=()):
        q = {n: (None if n in null else v.data_ptr()) for n, v in ptr.items()}
        q["z"] = None if "z" in null else z.data_ptr()
        return fn(q["z"], ld, groups, views, k, ctypes.c_float(0.5), q["lse"], q["p"], ldp, q["pbar"], ldb, q["Hbar"], q["dz"], ldd,
                  q["out"], q["ws"], None)

    for k in ("z", "lse", "pbar", "Hbar", "out", "ws"):
        assert call(null=(k,)) < 0, k
    assert call(groups=0) < 0 and call(views=0) < 0 and call(k=0) < 0 and call(groups=-1) < 0 and call(views=-3) < 0
    assert call(ld=K - 1) < 0 and call(ldp=K - 1) < 0 and call(ldb=K - 1) < 0 and call(ldd=K - 1) < 0
    assert call(groups=1 << 16, views=1 << 15) < 0 and call(groups=2147483647, views=2) < 0   # groups x views overflows int
    torch.cuda.synchronize()
    for k, v in ptr.items():
        assert bool((v == SENTINEL).all()), f"a refused call wrote {k}"
    assert call() == 0
    assert call(null=("p",)) == 0 and call(null=("dz",)) == 0 and call(null=("p", "dz"), ldp=0, ldd=0) == 0   # optional outputs
    torch.cuda.synchronize()
    assert not bool((ptr["Hbar"] == SENTINEL).any())


# ------------------------------------------------------------------------------------------ check 3: the step, restated
HEAD_SCALE = 8.0


def parity_state(hp, sseed, head_scale):
    sd = T.initial_state(hp, sseed)
    if head_scale is not None:
        k = "model.classifier_multimodal.weight"
        sd[k] = sd[k] * head_scale
    return sd


def margent_restated(sd, keys, views, table, hp, dtype, G, V, N, decisions=None):
    """The adapting pass of MEMO on G V rows (views [G V, 3, P, P], table [G V, C]; CPU), on a deep copy of the state: out_m of
    O.backbone_forward_all(train=True, masks=None) under the BatchNorm blend at G V images, margent_loss, autograd w.r.t. A.
    -> dict(g {key: gradient}, flips, loss, pbar, Hbar, out_m)"""
    s = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k in keys:
        s[k].requires_grad_(True)
    ctx = O.force_decisions(*decisions) if decisions is not None else contextlib.nullcontext()
    with blended_oracle(N, G * V), ctx as d:
        out_m = O.backbone_forward_all(s, "model.", views.to(dtype), table.to(dtype), hp, train=True, masks=None)[0]
        loss, _, logpbar, Hbar = margent_loss(out_m, G, V)
        g = torch.autograd.grad(loss, [s[k] for k in keys])
    flips = {t: v for t, v in d.get("flips", {}).items() if v[0]} if d is not None else {}
    return dict(g=dict(zip(keys, [t.detach() for t in g])), flips=flips, loss=loss.detach(), pbar=logpbar.exp().detach(),
                Hbar=Hbar.detach(), out_m=out_m.detach())


def scores_restated(sd, x, hp, dtype, N, decisions=None):
    """The scoring forward: softmax(out_m) of the clean batch under the blend at its own B images -> (p, flips)"""
    keys = [k for k in sd if k.endswith("bn1.weight")][:1]
    with blended_oracle(N, x[0].shape[0]):
        p, _, flips = T.tent_restated(sd, keys, x, hp, dtype, decisions)
    return p, flips


# (label, hparams, B, V, tta_params, batch seeds, state seed, head scale, episodic)
PARITY = [
    ("dvm64_b2_v8_x8", lambda: T.dvm_hp(2, img_size=64), 2, 8, "bn", (501, 502), 41, HEAD_SCALE, False),
    ("cardiac64_b1_v16", lambda: T.cardiac_hp(1, img_size=64), 1, 16, "norm", (601, 602), 51, None, True),
]
PARITY_LR = 1e-3
PARITY_N = 16


class split_trace:
    """ops._trace for the duration of a marginal_entropy step, in two parts: the decisions of the adapting pass (`adapt`) and
    those of the scoring forward after it (`score`), which would otherwise overwrite them."""

    def __enter__(self):
        from stil_tta_amd import ops, tta
        self.ops, self.tta, self.orig = ops, tta, tta.adapting_pass
        self.adapt = None

        def wrapped(*a, **k):
            r = self.orig(*a, **k)
            self.adapt, ops._trace = ops._trace, {"relu": {}, "pool": {}}
            return r
        tta.adapting_pass = wrapped
        ops._trace = {"relu": {}, "pool": {}}
        return self

    def __exit__(self, *a):
        self.score = self.ops._trace
        self.ops._trace = None
        self.tta.adapting_pass = self.orig


@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_marginal_entropy_step_matches_the_contract_restated_in_float64(case):
    """Bars are TENT's (tests/test_gpu_tta.py): every gradient of A <= 3 e32 + 1e-4, Adam within 2.2 lr step, everything outside A
    bit-identical; loss, marginal and marginal_entropy within close() at TOL of float64; the predictions of the scoring forward
    (a second oracle forward, from the device's post-update state, on the clean batch) <= 3e-5 scaled."""
    import test_gpu_step as S
    from stil_tta_amd import tta
    label, mk_hp, B, V, which, seeds, sseed, head, episodic = case
    hp = mk_hp()
    lr, N = PARITY_LR, PARITY_N
    sd = parity_state(hp, sseed, head)
    m = T.make_model(hp, sd, tta=True, tta_method="marginal_entropy", tta_params=which, tta_lr=lr, tta_views=V, tta_bn_prior=N,
                     tta_episodic=episodic)
    m.freeze()
    keys = T.adapted_keys(m)
    assert len(keys) == (106 if which == "bn" else 106 + 2 * (1 + 4 * 2) + 2 * 2)
    source = {k: v.cpu() for k, v in m.state_dict().items()}
    opt, bad = {}, []
    for step, seed in enumerate(seeds, start=1):
        x, y = T.tta_batch(hp, B, seed)
        before = T.full_state(m)
        sd_before = source if episodic else {k: v.cpu() for k, v in m.state_dict().items()}   # what the adapting pass starts from
        with split_trace() as tr:
            m.test_step(T.to_dev((x, y)), step - 1)
            torch.cuda.synchronize()
        d_adapt, d_score = S._device_decisions(m, tr.adapt), S._device_decisions(m, tr.score)
        lt = m.last_tta
        assert set(lt) == {"loss", "marginal", "marginal_entropy", "y_hat_m", "probs", "draws"} and isinstance(lt["draws"], dict)
        views, tab, draws = tta.make_views(m, T.to_dev((x, y))[0], lt["draws"])
        views2, tab2, _ = tta.make_views(m, T.to_dev((x, y))[0], lt["draws"])
        assert draws is lt["draws"] and torch.equal(views, views2) and torch.equal(tab, tab2), "the views do not rebuild bit for bit"
        assert views.shape == (B * V, 3, hp.img_size, hp.img_size) and torch.equal(tab.cpu(), x[1].repeat_interleave(V, 0))
        assert float((views[0] - views[1]).abs().max()) > 0, "two views of one sample are the same image"
        views, tab = views.cpu(), tab.cpu()
        r64 = margent_restated(sd_before, keys, views, tab, hp, torch.float64, B, V, N, d_adapt)
        r64free = margent_restated(sd_before, keys, views, tab, hp, torch.float64, B, V, N)
        r32 = margent_restated(sd_before, keys, views, tab, hp, torch.float32, B, V, N)
        S._check_flips(r64["flips"])
        for name, got, want in (("loss", lt["loss"].view(1), r64["loss"].view(1)), ("marginal", lt["marginal"], r64["pbar"]),
                                ("marginal_entropy", lt["marginal_entropy"], r64["Hbar"])):
            assert got.is_cuda
            err = (got.cpu().double() - want).abs()
            ratio = float((err / (TOL * (1.0 + want.abs() + want.abs().max()))).max())
            print(f"[{label}] batch {step}: {name} error / close() bound {ratio:.3f} (loss {float(r64['loss']):.6f})")
            close(got, want, name=name)
        gd = T.device_grads(m)
        ratios = []
        for k in keys:
            e32 = T._rel(r32["g"][k].double(), r64free["g"][k])
            err = T._rel(gd[k], r64["g"][k])
            ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
            if err > 3 * e32 + 1e-4:
                bad.append((step, "grad " + k, err, e32))
        print(f"[{label}] batch {step}: gradient error / (3*e32 + 1e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
        # Adam over A (fp32 oracle, its own moments) from the same parameters; episodic: a fresh optimiser every batch
        sd32 = {k: v.clone() for k, v in sd_before.items()}
        if episodic:
            opt = {}
        nstep = 1 if episodic else step
        O.adam_step(sd32, r32["g"], opt, nstep, lr)
        after = T.full_state(m)
        aset = set(keys)
        worst_adam = 0.0
        for k, v in after.items():
            if k in aset:
                dev = float((v.cpu() - sd32[k]).abs().max())
                worst_adam = max(worst_adam, dev / (2.2 * lr * nstep))
                if dev > 2.2 * lr * nstep:
                    bad.append((step, "adam " + k, dev))
            elif not torch.equal(v, before[k]):
                bad.append((step, "changed " + k))
        print(f"[{label}] batch {step}: Adam deviation / (2.2 lr step), worst: {worst_adam:.3f}")
        # the scores: the clean batch, from the device's post-update state
        sd_after = {k: v.cpu() for k, v in m.state_dict().items()}
        p64, flips = scores_restated(sd_after, x, hp, torch.float64, N, d_score)
        p32, _ = scores_restated(sd_after, x, hp, torch.float32, N)
        S._check_flips(flips)
        d = S._scaled(lt["probs"].cpu().double().numpy(), p64.numpy())
        print(f"[{label}] batch {step}: predictions scaled error {d:.2e} (fp32 restatement {S._scaled(p32.double().numpy(), p64.numpy()):.2e})")
        if d > 3e-5:
            bad.append((step, "predictions", d))
        assert lt["probs"].shape == (B, hp.num_classes)
        close(lt["probs"], torch.softmax(lt["y_hat_m"].double(), dim=1), name="probs against softmax(y_hat_m)")
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


# ------------------------------------------------------------------------------------------ check 4: properties
SMALL_B, SMALL_V = 2, 8


def _small(which="bn", method="marginal_entropy", B=SMALL_B, **tta):
    hp = T.dvm_hp(B, img_size=64)
    sd = parity_state(hp, 5, HEAD_SCALE)
    tta.setdefault("tta_views", SMALL_V)
    return hp, sd, (lambda: T.make_model(hp, sd, tta=True, tta_method=method, tta_params=which, **tta))


def _adapt_state(m):
    st = m._tent
    out = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    out.update({"#tta_exp_avg": st.exp_avg.clone(), "#tta_exp_avg_sq": st.exp_avg_sq.clone(), "#tta_steps": st.steps.clone()})
    return out


@pytest.mark.parametrize("which", ["bn", "norm"])
def test_step_issues_no_weight_gradient_product(which, monkeypatch):
    from stil_tta_amd._lib import lib
    hp, sd, mk = _small(which)
    m = mk()
    L = lib()
    calls = []
    for name in ("wgrad_tn", "wgrad_tn_partial"):
        orig = getattr(L, name)
        monkeypatch.setitem(L.__dict__, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    A0 = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    m.test_step(T.to_dev(T.tta_batch(hp, SMALL_B, 7)), 0)
    torch.cuda.synchronize()
    assert calls == [], f"{len(calls)} weight-gradient launches in a marginal-entropy step"
    assert any(not torch.equal(m.state_dict()[k], v) for k, v in A0.items()), "the step adapted nothing"


def _sync_warnings(fn):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return [str(x.message) for x in w if "called a synchronizing" in str(x.message)]   # not the mode's own one-time notice


def test_step_synchronises_no_more_than_views_plus_a_tent_step():
    from stil_tta_amd.augment import ImageAugmenter
    hp, sd, mk = _small()
    _, _, mkt = _small(method="tent")
    m, t = mk(), mkt()
    B, V = SMALL_B, SMALL_V
    aug = ImageAugmenter(img_size=hp.img_size, target=hp.target, kind=m.hp.tta_view_policy, augmentation_rate=1.0, seed=m.hp.tta_view_seed)
    batches = [T.to_dev(T.tta_batch(hp, B, 11 + i)) for i in range(2)]

    def tent_on_views(b, i):
        (img, tab), y = b
        draws = aug.draw(B * V, img.shape[2], img.shape[3])
        views = aug(img.repeat_interleave(V, dim=0), draws, want_orig=False)[0]
        t.test_step(([views, tab.repeat_interleave(V, dim=0)], y.repeat_interleave(V, dim=0)), i)

    m.test_step(batches[0], 0)          # the first batch creates the states
    tent_on_views(batches[0], 0)
    torch.cuda.synchronize()
    ours = _sync_warnings(lambda: m.test_step(batches[1], 1))
    theirs = _sync_warnings(lambda: tent_on_views(batches[1], 1))
    print(f"synchronising calls: marginal_entropy step {len(ours)}, views + tent step {len(theirs)}")
    assert len(ours) <= len(theirs), (ours, theirs)


def test_same_view_seed_is_bit_identical_and_another_seed_is_not():
    hp, sd, mk = _small()
    _, _, mk_other = _small(tta_view_seed=7)
    a, c, o = mk(), mk(), mk_other()
    for i in range(2):
        b = T.to_dev(T.tta_batch(hp, SMALL_B, 11 + i))
        pa, pc, po = a.test_step(b, i).clone(), c.test_step(b, i).clone(), o.test_step(b, i).clone()
        assert torch.equal(pa, pc), f"batch {i}: scores"
        sa, sc = _adapt_state(a), _adapt_state(c)
        for k in sa:
            assert torch.equal(sa[k], sc[k]), f"batch {i}: {k}"
        for k, v in a.last_tta["draws"].items():
            assert np.array_equal(v, c.last_tta["draws"][k]), k
        assert int(a._tent.steps.max()) == i + 1
    assert not np.array_equal(a.last_tta["draws"]["boxes"], o.last_tta["draws"]["boxes"]) and not torch.equal(pa, po)


def test_episodic_mode_reset_and_the_views_generator():
    hp, sd, mk = _small(tta_episodic=True)
    b1, b2 = T.to_dev(T.tta_batch(hp, SMALL_B, 11)), T.to_dev(T.tta_batch(hp, SMALL_B, 12))
    m = mk()
    A0 = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    m.test_step(b1, 0)
    d1 = m.last_tta["draws"]
    A1 = _adapt_state(m)
    m.test_step(b1, 1)                       # the same batch again: from the source values, with the NEXT draws
    d2 = m.last_tta["draws"]
    assert not np.array_equal(d1["boxes"], d2["boxes"]), "an episode restarted the views' generator"
    assert int(m._tent.steps.max()) == 1
    # every batch starts from the source values: batch 2 after batch 1 equals batch 2 on the second draws of a fresh model
    from stil_tta_amd import tta
    g = mk()
    tta._state(g)
    g._tent.views.draw(SMALL_B * SMALL_V, hp.img_size, hp.img_size)
    g._tent.views.draw(SMALL_B * SMALL_V, hp.img_size, hp.img_size)
    p3 = m.test_step(b2, 2).clone()
    q3 = g.test_step(b2, 0).clone()
    assert torch.equal(p3, q3), "episodic: batch 3 depends on the batches before it beyond the generator's position"
    sm, sg = T.full_state(m), T.full_state(g)
    for k in sm:
        assert torch.equal(sm[k], sg[k]), k
    # online: the adaptation carries over; reset_tta() restores A bit for bit and leaves the generator running
    _, _, mk_on = _small()
    o = mk_on()
    o.test_step(b1, 0)
    for k in A1:
        assert torch.equal(_adapt_state(o)[k], A1[k]), k      # the first batch is the episodic one
    o.test_step(b2, 1)
    assert int(o._tent.steps.max()) == 2
    aug = o._tent.views
    o.reset_tta()
    for k, v in A0.items():
        assert torch.equal(o.state_dict()[k], v), k
    assert o._tent.views is aug and int(o._tent.steps.max()) == 0 and o._tent.source is None
    o.load_state_dict({k: v.cuda() for k, v in sd.items()})
    assert o._tent is None, "load_state_dict keeps the adaptation state (and the views' generator)"
    o.test_step(b1, 0)
    assert all(np.array_equal(v, d1[k]) for k, v in o.last_tta["draws"].items()), "a new state does not restart the generator from tta_view_seed"


def test_freeze_and_inference_mode():
    hp, sd, mk = _small()
    b = T.to_dev(T.tta_batch(hp, SMALL_B, 14))
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


def test_scores_come_after_the_update():
    """One sample, episodic: the scores differ from bn_adapt's (the same forward before any update) and equal bn_adapt's on a
    model that carries the adapted parameters."""
    hp, sd, mk = _small(B=1, tta_episodic=True, tta_bn_prior=16, tta_views=SMALL_V, tta_lr=1e-2)
    b = T.to_dev(T.tta_batch(hp, 1, 31))
    m = mk()
    p = m.test_step(b, 0).clone()
    n = T.make_model(hp, sd, tta=True, tta_method="bn_adapt", tta_bn_prior=16)
    p0 = n.test_step(b, 0).clone()
    assert not torch.equal(p, p0), "the scores are those of the source model: taken before the update"
    n.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    assert torch.equal(n.test_step(b, 0), p)


def test_fit_test_takes_the_adapting_path(tmp_path):
    from stil_tta_amd import fit
    hp, sd, mk = _small()
    loader = [T.tta_batch(hp, SMALL_B, 20 + i) for i in range(3)]
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
    assert any(not torch.equal(so[k], sa[k]) for k in T.adapted_keys(a)), "fit.test with marginal_entropy left A where the run without TTA leaves it"


def test_ragged_last_batch():
    hp, sd, mk = _small(tta_bn_prior=16)
    m = mk()
    K = hp.num_classes
    m.test_step(T.to_dev(T.tta_batch(hp, 3, 11)), 0)
    assert m.last_tta["marginal"].shape == (3, K) and m.last_tta["probs"].shape == (3, K)
    A1 = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    p = m.test_step(T.to_dev(T.tta_batch(hp, 1, 12)), 1)
    torch.cuda.synchronize()
    lt = m.last_tta
    assert p.shape == (1, K) and lt["probs"].shape == (1, K) and lt["marginal"].shape == (1, K) and lt["marginal_entropy"].shape == (1,)
    assert lt["draws"]["boxes"].shape[0] == SMALL_V
    for k in ("loss", "marginal", "marginal_entropy", "probs", "y_hat_m"):
        assert lt[k].is_cuda and bool(torch.isfinite(lt[k]).all()), k
    close(lt["marginal"].sum(1), torch.ones(1), name="sum of the marginal")
    close(lt["loss"].view(1), lt["marginal_entropy"].double().mean().view(1), name="loss against the mean of marginal_entropy")
    assert int(m._tent.steps.max()) == 2
    assert any(not torch.equal(m.state_dict()[k], v) for k, v in A1.items()), "the one-sample batch adapted nothing"


def test_tent_does_not_see_the_view_keys():
    """tta_method "tent" runs what it ran: the three new keys change nothing in it, and it holds no augmenter."""
    hp, sd, _ = _small()
    a = T.make_model(hp, sd, tta=True, tta_method="tent")
    c = T.make_model(hp, sd, tta=True, tta_method="tent", tta_views=3, tta_view_policy="weak", tta_view_seed=1)
    for i in range(2):
        b = T.to_dev(T.tta_batch(hp, 16, 11 + i))
        assert torch.equal(a.test_step(b, i), c.test_step(b, i))
    sa, sc = _adapt_state(a), _adapt_state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert a._tent.views is None and set(a.last_tta) == {"loss", "y_hat_m", "probs"}
    from stil_tta_amd import tta
    with pytest.raises(ValueError):
        tta.make_views(a, T.to_dev(T.tta_batch(hp, 2, 1))[0])
