"""CPU side of marginal-entropy test-time adaptation (tests/test_gpu_margent.py): the hparams rules, the closed-form gradient of
include/stil_margent.h against float64 autograd, and the conditions on the inputs the GPU tests use -- fp32 ATen and the fp32
oracle meet the GPU bars against float64 there, so a kernel or step that misses them is wrong, not unlucky; and the views move
the predictions enough that a kernel which computed row entropy instead would miss them."""
import math
import os
import sys

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import test_gpu_margent as G  # noqa: E402
import test_gpu_tta as T  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402


def _model(**over):
    from stil_tta_amd import STiLModel
    d = dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False)
    d.update(over)
    return STiLModel(d)


def test_marginal_entropy_keys_and_defaults():
    m = _model(tta=True, tta_method="marginal_entropy")
    assert m._tta_on() and not _model(tta=False, tta_method="marginal_entropy")._tta_on() and not _model(tta=True)._tta_on()
    hp = m.hp
    assert (hp.tta_views, hp.tta_view_policy, hp.tta_view_seed) == (32, "hard_eval", 2022)
    assert (hp.tta_lr, hp.tta_episodic, hp.tta_params, hp.tta_bn_prior) == (1e-3, False, "bn", None)
    from stil_tta_amd import tta
    assert "marginal_entropy" in tta.METHODS and "memo" not in tta.METHODS
    assert callable(tta.marginal_entropy_step) and callable(tta.marginal_entropy) and callable(tta.make_views)
    assert m._tent is None and m.last_tta == {}
    from stil_tta_amd._lib import TTA_HEADERS
    (header,) = [p for p in TTA_HEADERS if os.path.basename(p) == "stil_margent.h"]
    assert os.path.exists(header)


def test_adapted_set_is_tents():
    for which in ("bn", "norm"):
        assert _model(tta=True, tta_method="marginal_entropy", tta_params=which).tta_param_names() == \
            _model(tta=True, tta_method="tent", tta_params=which).tta_param_names()


@pytest.mark.parametrize("method", [None, "tent", "marginal_entropy"])
def test_view_keys_are_checked_whatever_the_method(method):
    for bad in (0, -1, 1.0, 32.5, "32", None, True, False, float("nan")):
        with pytest.raises(ValueError):
            _model(tta=True, tta_method=method, tta_views=bad)
    for bad in ("augmix", "HARD_EVAL", "", None, 1, ("weak",)):
        with pytest.raises(ValueError):
            _model(tta=True, tta_method=method, tta_view_policy=bad)
    for bad in (1.5, "2022", None, -1):
        with pytest.raises(ValueError):
            _model(tta=True, tta_method=method, tta_view_seed=bad)
    for pol in ("contrastive", "hard_eval", "soft_eval", "weak", "strong"):
        m = _model(tta=True, tta_method=method, tta_views=1, tta_view_policy=pol, tta_view_seed=0)
        assert (m.hp.tta_views, m.hp.tta_view_policy, m.hp.tta_view_seed) == (1, pol, 0)


def test_memo_saint_and_all_parameters_are_still_refused():
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="memo")
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="MARGINAL_ENTROPY")
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="marginal_entropy", tta_params="all")
    with pytest.raises(NotImplementedError):
        _model(tta=True, tta_method="marginal_entropy", tabular_encoder="saint")
    with pytest.raises(NotImplementedError):
        _model(tta_method="marginal_entropy", algorithm_name="STiL_SAINT")


def closed_form_dz(z, G_, V, gs):
    """dZ of include/stil_margent.h, restated in z's dtype"""
    logp = torch.log_softmax(z, dim=1)
    p = logp.exp()
    logpbar = (torch.logsumexp(logp.view(G_, V, -1), dim=1) - math.log(V)).repeat_interleave(V, dim=0)
    return gs / V * p * ((p * logpbar).sum(1, keepdim=True) - logpbar)


@pytest.mark.parametrize("G_,V,K", [(1, 1, 1), (1, 8, 5), (3, 2, 2), (5, 33, 13)])
def test_closed_form_gradient_is_float64_autograd(G_, V, K):
    """dZ of include/stil_margent.h, restated in float64, is the autograd gradient of grad_scale sum_g Hbar_g; with one view it is
    TENT's -p (log p + H)."""
    g = torch.Generator().manual_seed(100 * G_ * V + K)
    z = 4.0 * torch.randn(G_ * V, K, generator=g, dtype=torch.float64)
    gs = 0.37
    ref = G.margent_ref(z, G_, V, torch.float64)
    want = ref["grad"] * gs * G_
    dz = closed_form_dz(z, G_, V, gs)
    assert float((dz - want).abs().max()) <= 1e-13 * (1.0 + float(want.abs().max()))
    if V == 1:
        t = T.entropy_ref(z, torch.float64)
        assert float((dz - t["grad"] * gs * G_).abs().max()) <= 1e-13 * (1.0 + float(want.abs().max()))


@pytest.mark.parametrize("G_,V,K,kind", G.margent_cases())
def test_fp32_aten_marginal_entropy_meets_tol(G_, V, K, kind):
    """fp32 ATen, in log-sum-exp form, meets every bar of test_marginal_entropy_groups_against_float64 on its inputs."""
    z = G.margent_input(G_, V, K, kind)
    r64 = G.margent_ref64(G_, V, K, kind)
    r32 = G.margent_ref(z, G_, V, torch.float32)
    if kind == "views_disagree" and K > V:
        assert float(r64["probs"].max(1).values.min()) > 0.9 and float(r64["pbar"].max()) < 1.2 / V   # confident rows, a spread marginal
    if kind == "views_agree" and K > 1:
        assert float(r64["pbar"].max(1).values.min()) > 0.9
    for k in ("lse", "probs", "pbar", "Hbar", "grad", "loss"):
        assert bool(torch.isfinite(r64[k]).all()), k
        a, b = (r[k].view(-1) if r[k].ndim == 0 else r[k] for r in (r32, r64))
        close(a, b, TOL, name=k)
    close(closed_form_dz(z.float(), G_, V, G.f32(1.0 / G_)), r64["grad"] * (G.f32(1.0 / G_) * G_), TOL, name="closed form in fp32")


def cpu_views(x, V):
    """V views of every image of x = [images [B, 3, P, P], table [B, C]], made on the CPU: flips, shifts and brightness
    scalings, sample-major as tta.make_views lays them out -> (views [B V, 3, P, P], table [B V, C])"""
    img, tab = x
    out = []
    for b in range(img.shape[0]):
        for v in range(V):
            t = img[b]
            if v % 2:
                t = t.flip(-1)
            t = torch.roll(t, shifts=((3 * v) % 7, (5 * v) % 11), dims=(-2, -1))
            out.append(t * (0.6 + 0.8 * v / max(V - 1, 1)))
    return torch.stack(out), tab.repeat_interleave(V, dim=0)


@pytest.mark.parametrize("case", G.PARITY, ids=[c[0] for c in G.PARITY])
def test_fp32_oracle_meets_the_bars_and_the_views_are_informative(case):
    """The step test's bars on the loss, marginal and marginal_entropy (close() at TOL) and on the predictions of the scoring
    forward (_scaled <= 3e-5) are reachable: the fp32 oracle meets them against float64 on every batch, on CPU-made views; later
    batches are reached by the fp32 oracle's own Adam steps (the GPU test reaches them by the device's).  And at this head scale
    the views disagree enough that the loss is not row entropy in disguise: dZ differs from TENT's dZ on the same rows by at
    least 0.1 relative, so a kernel that computed row entropy would miss the GPU bars (TOL) by orders of magnitude."""
    from test_gpu_step import _scaled
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    label, mk_hp, B, V, which, seeds, sseed, head, episodic = case
    hp = mk_hp()
    N = G.PARITY_N
    source = G.parity_state(hp, sseed, head)
    sd = {k: v.clone() for k, v in source.items()}
    keys = _model(**{**vars(hp), "tta": True, "tta_method": "marginal_entropy", "tta_params": which}).tta_param_names()
    opt = {}
    for step, seed in enumerate(seeds, start=1):
        if episodic:
            sd, opt = {k: v.clone() for k, v in source.items()}, {}
        x, _ = T.tta_batch(hp, B, seed)
        views, tab = cpu_views(x, V)
        r32 = G.margent_restated(sd, keys, views, tab, hp, torch.float32, B, V, N)
        r64 = G.margent_restated(sd, keys, views, tab, hp, torch.float64, B, V, N)
        close(r32["loss"].view(1), r64["loss"].view(1), TOL, name="loss")
        close(r32["pbar"], r64["pbar"], TOL, name="marginal")
        close(r32["Hbar"], r64["Hbar"], TOL, name="marginal_entropy")
        me = G.margent_ref(r64["out_m"], B, V, torch.float64)["grad"]
        te = T.entropy_ref(r64["out_m"], torch.float64)["grad"]
        apart = T._rel(me, te)
        worst = max(T._rel(r32["g"][k].double(), r64["g"][k]) for k in keys)
        O.adam_step(sd, r32["g"], opt, 1 if episodic else step, G.PARITY_LR)
        p32, _ = G.scores_restated(sd, x, hp, torch.float32, N)
        p64, _ = G.scores_restated(sd, x, hp, torch.float64, N)
        d = _scaled(p32.double().numpy(), p64.numpy())
        print(f"[{label}] batch {step}: loss {float(r64['loss']):.5f} (fp32 off by {abs(float(r32['loss']) - float(r64['loss'])):.2e}), "
              f"row entropy of the same rows {float(T.entropy_ref(r64['out_m'], torch.float64)['loss']):.5f}; dZ against TENT's dZ "
              f"{apart:.3f} relative; worst e32 {worst:.2e}; scoring predictions scaled error {d:.2e}")
        assert d <= 3e-5
        assert apart >= 0.1, f"the views move the predictions too little: dZ is within {apart:.3f} of TENT's"
