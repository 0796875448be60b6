"""CPU side of ROID test-time adaptation (tests/test_gpu_roid.py): the hparams rules, the closed-form gradient of
stil_tta_amd/csrc/stil_roid.h against float64 autograd, and the conditions on the inputs the GPU tests use -- no selection hangs on
a margin fp32 could flip and fp32 ATen meets the GPU bars against float64 there, so a kernel that misses them is wrong, not unlucky."""
import os
import sys

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import roid_cases as C  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402


def _model(**over):
    from stil_tta_amd import STiLModel
    d = dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False)
    d.update(over)
    return STiLModel(d)


def test_roid_keys_and_defaults():
    from stil_tta_amd import tta
    m = _model(tta=True, tta_method="roid")
    assert m._tta_on() and not _model(tta=False, tta_method="roid")._tta_on()
    hp = m.hp
    assert (hp.tta_roid_temperature, hp.tta_roid_src_momentum, hp.tta_roid_clip, hp.tta_roid_eps, hp.tta_roid_prior_correction) == \
        (1.0 / 3.0, 0.99, 0.99, 1e-5, True)
    assert hp.tta_probs_momentum == 0.9
    assert "roid" in tta.METHODS and tta.STEPS["roid"] is tta.roid_step and callable(tta.roid_loss)
    assert issubclass(tta.RoidState, tta.CompactState)
    assert m._tent is None and m.last_tta == {}
    d = _model().hp     # the keys exist whatever the method
    assert (d.tta_roid_temperature, d.tta_roid_src_momentum, d.tta_roid_clip, d.tta_roid_eps, d.tta_roid_prior_correction) == \
        (1.0 / 3.0, 0.99, 0.99, 1e-5, True)


def test_adapted_set_is_tents():
    for which in ("bn", "norm"):
        assert _model(tta=True, tta_method="roid", tta_params=which).tta_param_names() == \
            _model(tta=True, tta_method="tent", tta_params=which).tta_param_names()


@pytest.mark.parametrize("method", [None, "tent", "roid"])
def test_roid_keys_are_checked_whatever_the_method(method):
    nan, inf = float("nan"), float("inf")
    bad = dict(tta_roid_temperature=(0, 0.0, -1.0, inf, nan, "1", None, True),
               tta_roid_src_momentum=(-0.01, 1.01, inf, nan, "0.99", None, True),
               tta_roid_clip=(0, 0.0, 1, 1.0, 1.5, -0.5, inf, nan, "0.99", None, True),
               tta_roid_eps=(0, 0.0, -1e-5, inf, nan, "1e-5", None, True),
               tta_roid_prior_correction=(None, 0, 1, "True", 1.0))
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=key):
                _model(tta=True, tta_method=method, **{key: v})
    ok = _model(tta=True, tta_method=method, tta_roid_temperature=2, tta_roid_src_momentum=0, tta_roid_clip=0.5, tta_roid_eps=1e-8,
                tta_roid_prior_correction=False).hp
    assert (ok.tta_roid_temperature, ok.tta_roid_src_momentum, ok.tta_roid_clip, ok.tta_roid_eps, ok.tta_roid_prior_correction) == \
        (2, 0, 0.5, 1e-8, False)
    assert _model(tta=True, tta_method=method, tta_roid_src_momentum=1).hp.tta_roid_src_momentum == 1


def test_the_running_means_momentum_is_checked_where_roid_reads_it():
    for v in (-0.1, 1.1, float("nan"), float("inf"), None, "0.9", True):
        with pytest.raises(ValueError, match="tta_probs_momentum"):
            _model(tta=True, tta_method="roid", tta_probs_momentum=v)
    for v in (0, 0.0, 0.5, 1, 1.0):
        assert _model(tta=True, tta_method="roid", tta_probs_momentum=v).hp.tta_probs_momentum == v


def test_roid_composes_as_tent_and_fusion_and_saint_stay_refused():
    hp = _model(tta=True, tta_method="roid", tta_params="norm", tta_bn_prior=16, tta_bn_momentum=0.05, tta_episodic=True).hp
    assert (hp.tta_params, hp.tta_bn_prior, hp.tta_bn_momentum, hp.tta_episodic) == ("norm", 16, 0.05, True)
    with pytest.raises(ValueError, match="fusion"):
        _model(tta=True, tta_method="roid", tta_params="fusion")
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="ROID")
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="roid", tta_params="all")
    with pytest.raises(NotImplementedError):
        _model(tta=True, tta_method="roid", tabular_encoder="saint")
    with pytest.raises(NotImplementedError):
        _model(tta_method="roid", algorithm_name="STiL_SAINT")


@pytest.mark.parametrize("rows,K", [(1, 1), (1, 5), (2, 2), (7, 2), (9, 13), (33, 300)])
@pytest.mark.parametrize("clip", [0.99, 0.6])
def test_closed_form_gradient_is_float64_autograd(rows, K, clip):
    """dZ of csrc/stil_roid.h, restated in float64 with the weights held constant, is the autograd gradient of grad_scale x loss;
    clip 0.6 puts columns on both sides of the clip."""
    g = torch.Generator().manual_seed(100 * rows + K)
    z = 3.0 * torch.randn(rows, K, generator=g, dtype=torch.float64)
    ema = torch.softmax(torch.randn(K, generator=g, dtype=torch.float64), dim=0)
    gs = 0.37
    x = z.clone().requires_grad_(True)
    out = C.roid_forward(x, ema, C.TAU, clip, C.EPS, C.MOMENTUM)
    (ref,) = torch.autograd.grad(out["loss"], [x])
    p = out["probs"]
    if K > 1 and clip < 0.9 and rows > 1:
        assert bool((p > clip).any()) and bool((p <= clip).any())
    dz = C.closed_form_dz(z, out["w"], clip, C.EPS, gs)
    assert float((dz - gs * ref).abs().max()) <= 1e-13 * (1.0 + gs * float(ref.abs().max()))
    assert bool((dz[~out["keep"]] == 0).all())
    if K == 1:
        assert bool((dz == 0).all()) and bool((ref == 0).all())


@pytest.mark.parametrize("rows,K,kind,ema_kind", C.roid_cases())
def test_the_cases_are_well_posed(rows, K, kind, ema_kind):
    """What tests/test_gpu_roid.py relies on, case by case.  No row left out: every quantity is finite and a range is either far
    above the 1e-9 rule or (numerically) zero.  spread / peaked: the smallest |dn_r - mean dn| is >= 5e-5 wherever a comparison of
    numbers decides (rows == 1 and K == 1 are decided by the rule: every dn is exactly 0), fp32 ATen flips no keep decision and
    meets close() at TOL on everything else.  tied: well-posed only through the rule -- both ranges degenerate, every weight 1."""
    r64 = C.roid_ref64(rows, K, kind, ema_kind)
    for k in ("loss", "lse", "probs", "H", "cos", "slr", "dn", "cn", "w", "pbar", "ema", "prior", "scores", "grad"):
        assert bool(torch.isfinite(r64[k]).all()), k
    for k in ("d_range", "c_range"):
        assert r64[k] <= 1e-13 or r64[k] >= 1e-6, (k, r64[k])
    assert r64["counts"].tolist()[1] == rows and int(r64["counts"][0]) == int(r64["keep"].sum()) >= 1
    close(r64["scores"].sum(1), torch.ones(rows, dtype=torch.float64), 1e-12, name="rows of scores")
    degenerate = rows == 1 or K == 1 or kind == "tied"
    assert r64["counts"].tolist()[2:] == ([1, 1] if degenerate else [0, 0])
    if degenerate:
        assert bool(r64["keep"].all()) and bool((r64["w"] == 1).all()) and r64["margin"] == float("inf")
    if K == 1:
        assert bool((r64["grad"] == 0).all())
    if kind == "tied":
        return
    assert r64["margin"] >= 5e-5, r64["margin"]
    r32 = C.roid_ref(C.roid_input(rows, K, kind), C.roid_ema(K, ema_kind), torch.float32)
    assert torch.equal(r32["keep"], r64["keep"]) and torch.equal(r32["counts"], r64["counts"])
    for k in ("loss", "lse", "probs", "H", "cos", "slr", "dn", "cn", "w", "pbar", "ema", "prior", "scores", "grad"):
        a, b = (r[k].view(-1) if r[k].ndim == 0 else r[k] for r in (r32, r64))
        close(a, b, TOL, name=k)


def test_the_smallest_margin_is_where_it_was_measured():
    worst = min((C.roid_ref64(*c)["margin"], c) for c in C.roid_cases() if c[2] != "tied")
    print(f"smallest float64 margin |dn_r - mean dn|: {worst[0]:.3e} at {worst[1]}")
    assert worst[1] == (130, 5000, "spread", "uniform") and 9.0e-5 <= worst[0] <= 9.5e-5


def test_momentum_one_makes_the_ensemble_the_identity():
    g = torch.Generator().manual_seed(3)
    a, t0 = torch.randn(4096, generator=g), torch.randn(4096, generator=g)
    a[:3] = torch.tensor([0.0, 1e-38, -3.0e38])
    assert torch.equal(C.ensemble_ref(a, t0, 1.0), a)
    assert torch.equal(C.ensemble_ref(a, t0, 0.0), t0)
    m = C.ensemble_ref(a, t0, 0.99)
    assert not torch.equal(m, a) and float((m - (0.99 * a.double() + 0.01 * t0.double()).float()).abs().max()) <= 1e-6
