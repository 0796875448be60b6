"""CPU side of RoTTA test-time adaptation (tests/test_gpu_rotta.py; definition as recalled: unpinned): the hparams rules, and the
conditions on the inputs the GPU tests use -- the bank's decisions restated in float64 and in float32 agree on every case and none
hangs on a margin below 5e-5, and fp32 ATen meets the loss kernel's bars against float64, so a kernel that misses them is wrong, not
unlucky."""
import os
import sys

import numpy as np
import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import rotta_cases as C  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402

KEYS = ("tta_rotta_capacity", "tta_rotta_nu", "tta_rotta_lambda_t", "tta_rotta_lambda_u")


def _model(**over):
    from stil_tta_amd import STiLModel
    d = dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False)
    d.update(over)
    return STiLModel(d)


def test_rotta_is_registered_with_its_keys_and_defaults():
    from stil_tta_amd import tta
    m = _model(tta=True, tta_method="rotta", tta_bn_momentum=0.05)
    assert m._tta_on() and not _model(tta=False, tta_method="rotta", tta_bn_momentum=0.05)._tta_on()
    assert tuple(getattr(m.hp, k) for k in KEYS) == (64, 0.001, 1.0, 1.0)
    assert "rotta" in tta.METHODS and tta.STEPS["rotta"] is tta.rotta_step and callable(tta.rotta_loss)
    assert issubclass(tta.RottaState, tta.CompactState)
    assert m._tent is None and m.last_tta == {}
    assert tuple(getattr(_model().hp, k) for k in KEYS) == (64, 0.001, 1.0, 1.0)   # the keys exist whatever the method
    for which in ("bn", "norm"):
        assert _model(tta=True, tta_method="rotta", tta_bn_momentum=0.05, tta_params=which).tta_param_names() == \
            _model(tta=True, tta_method="tent", tta_params=which).tta_param_names()


def test_rotta_requires_the_bn_memory():
    with pytest.raises(ValueError, match="tta_bn_momentum"):
        _model(tta=True, tta_method="rotta")
    with pytest.raises(ValueError, match="0.05"):
        _model(tta_method="rotta", tta_bn_momentum=None)
    hp = _model(tta=True, tta_method="rotta", tta_params="norm", tta_bn_prior=16, tta_bn_momentum=0.05, tta_episodic=True).hp
    assert (hp.tta_params, hp.tta_bn_prior, hp.tta_bn_momentum, hp.tta_episodic) == ("norm", 16, 0.05, True)
    with pytest.raises(ValueError, match="fusion"):
        _model(tta=True, tta_method="rotta", tta_bn_momentum=0.05, tta_params="fusion")
    with pytest.raises(NotImplementedError):
        _model(tta=True, tta_method="rotta", tta_bn_momentum=0.05, tabular_encoder="saint")
    with pytest.raises(NotImplementedError):
        _model(tta_method="rotta", tta_bn_momentum=0.05, algorithm_name="STiL_SAINT")


@pytest.mark.parametrize("method", [None, "tent", "rotta"])
def test_rotta_keys_are_checked_whatever_the_method(method):
    nan, inf = float("nan"), float("inf")
    bad = dict(tta_rotta_capacity=(0, -1, 1.0, 64.0, "64", None, True, 4097, inf, nan),
               tta_rotta_nu=(-0.001, 1.001, inf, nan, "0.001", None, True),
               tta_rotta_lambda_t=(-1.0, -1e-9, inf, nan, "1", None, True),
               tta_rotta_lambda_u=(-1.0, -1e-9, inf, nan, "1", None, True))
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=key):
                _model(tta=True, tta_method=method, tta_bn_momentum=0.05, **{key: v})
    ok = _model(tta=True, tta_method=method, tta_bn_momentum=0.05, tta_rotta_capacity=1, tta_rotta_nu=0, tta_rotta_lambda_t=0,
                tta_rotta_lambda_u=2.5).hp
    assert tuple(getattr(ok, k) for k in KEYS) == (1, 0, 0, 2.5)
    assert _model(tta=True, tta_method=method, tta_bn_momentum=0.05, tta_rotta_nu=1, tta_rotta_capacity=4096).hp.tta_rotta_nu == 1


def test_make_views_refuses_the_methods_without_views():
    from stil_tta_amd import tta
    with pytest.raises(ValueError, match="rotta"):
        tta.make_views(_model(tta=True, tta_method="tent"), None)


@pytest.mark.parametrize("N,K,B,start", C.update_cases())
def test_the_banks_decisions_are_well_conditioned(N, K, B, start):
    """What tests/test_gpu_rotta.py relies on, case by case: the walk restated with float64 scores and with float32 scores (from the
    float32 entropies) takes identical decisions, and no accept / evict comparison or argmax hangs on a margin below 5e-5."""
    z, bank, r64 = C.update_case(N, K, B, start)
    assert r64["margin"] >= C.MIN_MARGIN, r64["margin"]
    _, _, H32, yhat = C.rows_ref(z, torch.float32)
    r32 = C.bank_walk(H32.numpy(), yhat.numpy(), N, K, bank, ft=np.float32)
    assert r32["margin"] >= C.MIN_MARGIN, r32["margin"]
    for k in ("label", "age", "occ", "n", "owner", "accepted", "slot_of", "counts"):
        assert np.array_equal(r32[k], r64[k]), k
    close(torch.from_numpy(r32["unc"]), torch.from_numpy(r64["unc"]), TOL, name="unc")
    # the invariants of a bank: the filled slots are the prefix, occ counts their labels, an owner is a sample the call accepted
    n = int(r64["n"][0])
    assert 0 <= n <= N and bool((r64["label"][:n] >= 0).all()) and bool((r64["label"][n:] == -1).all())
    assert np.array_equal(np.bincount(r64["label"][:n], minlength=K), r64["occ"])
    assert int(r64["counts"][0]) == int(r64["accepted"].sum()) and int(r64["counts"][2]) == n
    for s, b in enumerate(r64["owner"]):
        assert b == -1 or (r64["accepted"][b] and r64["slot_of"][b] == s)
    if B > N and K > 1:
        lost = [b for b in range(B) if r64["accepted"][b] and r64["owner"][r64["slot_of"][b]] != b]
        assert lost or start != "empty", "no sample was accepted and evicted within the call: the case does not cover it"


def test_the_cases_cover_every_branch_of_the_decision():
    """Over all cases: additions to a bank with room, evictions from the classes of maximal occupancy, evictions from the sample's
    own class, refusals, and N / K below one slot."""
    adds = evictions = refusals = 0
    for case in C.update_cases():
        r = C.update_case(*case)[2]
        adds += int(r["counts"][0] - r["counts"][1])
        evictions += int(r["counts"][1])
        refusals += int((r["accepted"] == 0).sum())
    assert adds > 100 and evictions > 100 and refusals > 100, (adds, evictions, refusals)
    N, K = 8, 5
    r = C.bank_walk(*(lambda z: (C.rows_ref(z)[2].numpy(), C.rows_ref(z)[3].numpy()))(C.one_class_stream(70, K, 2)), N, K,
                    C.start_bank(N, K, "empty", 0))
    assert r["occ"].tolist() == [0, 0, 2, 0, 0] and int(r["n"][0]) == 2, "a one-class stream holds that class to its share"


@pytest.mark.parametrize("rows,K,ages", C.loss_cases())
def test_fp32_aten_meets_the_loss_kernels_bars(rows, K, ages):
    r64 = C.loss_ref64(rows, K, ages)
    zs, zt, label, age = C.loss_input(rows, K, ages)
    r32 = C.loss_ref(zs, zt, label, age, torch.float32)
    assert r32["n"] == r64["n"] == int((label >= 0).sum()) >= 1
    for k in ("loss", "ce", "w", "grad"):
        assert bool(torch.isfinite(r64[k]).all()), k
        a, b = (r[k].view(-1) if r[k].ndim == 0 else r[k] for r in (r32, r64))
        close(a, b, TOL, name=k)
    assert bool((r64["grad"][label < 0] == 0).all()) and bool((r64["w"][label < 0] == 0).all())
    if ages == "zero":
        assert bool((r64["w"][label >= 0] == 0.5).all())
    if ages == "huge" and rows == 1:
        assert float(r64["w"][0]) == 0.0, "exp(-10^6) underflows to a weight of exactly 0"
    if K == 1:
        assert bool((r64["grad"] == 0).all())


def test_an_empty_bank_has_no_loss_and_the_teacher_average_has_its_ends():
    zs, zt, label, age = C.loss_input(5, 7, "mixed")
    out = C.loss_ref(zs, zt, torch.full_like(label, -1), age, torch.float64)
    assert out["n"] == 0 and float(out["loss"]) == 0.0 and bool((out["grad"] == 0).all())
    g = torch.Generator().manual_seed(3)
    t, a = torch.randn(4096, generator=g), torch.randn(4096, generator=g)
    assert torch.equal(C.teacher_ref(t, a, 0.0), t) and torch.equal(C.teacher_ref(t, a, 1.0), a)
    m = C.teacher_ref(t, a, 0.001)
    assert not torch.equal(m, t) and float((m - t).abs().max()) <= 1e-2
