"""CPU side of SAR test-time adaptation (tests/test_gpu_sar.py): the hparams rules, the float64 references the GPU tests use
(the row contract as the analytic gradient against autograd, the ascent step), and the conditions on the GPU tests' inputs --
every selection decision is far from its threshold, the ascent step moves the entropies, and fp32 ATen meets the GPU bars
against float64 there, so a kernel or step that misses them is wrong, not unlucky."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import test_gpu_eata as E  # noqa: E402
import test_gpu_sar as R  # noqa: E402
import test_gpu_tta as T  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402


def _model(**over):
    from stil_tta_amd import STiLModel
    d = dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False)
    d.update(over)
    return STiLModel(d)


def test_sar_keys_and_defaults():
    from stil_tta_amd import tta
    assert "sar" in tta.METHODS
    m = _model(tta=True, tta_method="sar")
    assert m._tta_on() and not _model(tta=False, tta_method="sar")._tta_on()
    hp = m.hp
    assert (hp.tta_sar_rho, hp.tta_sar_reset) == (0.05, None)
    assert (hp.tta_e_margin, hp.tta_lr, hp.tta_episodic, hp.tta_params) == (None, 1e-3, False, "bn")
    assert len(m.tta_param_names()) == 106
    # the defaults resolve: 0.2 at the fraction ln K / ln 1000 of the maximal entropy; K = 286 is the default model's
    assert hp.num_classes == 286 and tta.sar_reset_value(hp) == 0.2 * math.log(286) / math.log(1000)
    assert abs(tta.sar_reset_value(hp) - 0.16376) < 1e-5
    two = _model(tta=True, tta_method="sar", num_classes=2).hp
    assert tta.sar_reset_value(two) == 0.2 * math.log(2) / math.log(1000) and abs(tta.sar_reset_value(two) - 0.020069) < 1e-6
    k1000 = copy.copy(hp)
    k1000.num_classes = 1000
    assert abs(tta.sar_reset_value(k1000) - 0.2) < 1e-15                      # the published constant where it was published
    for v, want in ((False, 0.0), (0.3, 0.3), (1, 1.0)):
        hp2 = copy.copy(hp)
        hp2.tta_sar_reset = v
        assert tta.sar_reset_value(hp2) == want
    assert tta.SAR_EMA_MOMENTUM == 0.9


def test_check_hparams_accepts_and_rejects():
    from stil_tta_amd import tta
    base = _model(tta=True, tta_method="sar", tta_sar_rho=0, tta_sar_reset=False)
    assert (base.hp.tta_sar_rho, base.hp.tta_sar_reset) == (0, False)

    def check(method="sar", **kw):
        hp = copy.copy(base.hp)
        hp.tta_method = method
        for k, v in kw.items():
            setattr(hp, k, v)
        tta.check_hparams(hp)
    for kw in (dict(tta_sar_rho=0.0), dict(tta_sar_rho=2), dict(tta_sar_rho=1e-3), dict(tta_sar_reset=None), dict(tta_sar_reset=False),
               dict(tta_sar_reset=0.2), dict(tta_sar_reset=3), dict(tta_sar_reset=1e-9)):
        check(**kw)
    for method in ("sar", "tent", None):               # the keys are checked whatever the method
        for kw in (dict(tta_sar_rho=-0.05), dict(tta_sar_rho=float("nan")), dict(tta_sar_rho=float("inf")), dict(tta_sar_rho=None),
                   dict(tta_sar_rho="0.05"), dict(tta_sar_rho=True), dict(tta_sar_rho=False), dict(tta_sar_rho=[0.05]),
                   dict(tta_sar_reset=0), dict(tta_sar_reset=0.0), dict(tta_sar_reset=-0.2), dict(tta_sar_reset=True),
                   dict(tta_sar_reset=float("nan")), dict(tta_sar_reset=float("inf")), dict(tta_sar_reset="0.2"), dict(tta_sar_reset=[0.2])):
            with pytest.raises(ValueError):
                check(method, **kw)
    with pytest.raises(ValueError):
        check("SAR")
    with pytest.raises(ValueError):                     # through the constructor too
        _model(tta=True, tta_method="sar", tta_sar_rho=-1.0)
    with pytest.raises(NotImplementedError):
        _model(tta=True, tta_method="sar", tabular_encoder="saint")
    with pytest.raises(NotImplementedError):
        _model(tta_method="sar", algorithm_name="STiL_SAINT")


def _analytic(z, margin, prior, dtype, gs):
    """The row contract written out as the kernel forms it: dZ = sel (-p (log p + H)) gs / n."""
    x = z.to(dtype)
    logp = torch.log_softmax(x, dim=1)
    p = logp.exp()
    H = -(p * logp).sum(dim=1)
    sel = (H < margin) & (torch.ones_like(H, dtype=torch.bool) if prior is None else prior.bool())
    n = int(sel.sum())
    if n == 0:
        return torch.zeros_like(x), torch.zeros((), dtype=dtype)
    return sel.to(dtype)[:, None] * (-p * (logp + H[:, None])) * gs / n, (sel.to(dtype) * H).sum() / n


@pytest.mark.parametrize("rows,K", [(r, k) for r in R.ROWS for k in R.KS])
def test_row_kernel_inputs_are_far_from_every_threshold_and_fp32_aten_meets_tol(rows, K):
    """No row has |H - margin| below 1e-3 (K == 1: H = 0 = margin exactly, in every precision); every running-mean variant leaves
    the mean at least 1e-3 from its threshold; the analytic gradient is autograd's; fp32 ATen meets close() / TOL."""
    z, margin = R.sar_input(rows, K)
    gs = 0.75
    seen = set()
    for pkind, ename in R.COMBOS:
        prior = R.prior_of(pkind, rows)
        r64, r32 = R.sar_ref(z, margin, prior, torch.float64, gs), R.sar_ref(z, margin, prior, torch.float32, gs)
        if K == 1:
            assert margin == 0.0 and bool((r64["H"] == 0).all()) and bool((r32["H"] == 0).all()) and r64["n"] == 0
        else:
            assert float((r64["H"] - margin).abs().min()) >= 1e-3
        if pkind == "zeros":
            assert r64["n"] == 0 and r64["n_prior"] == 0
        elif K > 1:
            assert r64["n"] > 0
            if rows >= 7:
                assert 0 < r64["n_rel"] < rows
                if pkind == "mixed":
                    assert r64["n"] < r64["n_rel"] and r64["n_prior"] < rows
        assert torch.equal(r32["sel"], r64["sel"])
        for k in ("lse", "probs", "H", "loss", "grad"):
            assert bool(torch.isfinite(r64[k]).all()), k
            a, b = (r[k].view(-1) if r[k].ndim == 0 else r[k] for r in (r32, r64))
            close(a, b, TOL, name=k)
        g, loss = _analytic(z, margin, prior, torch.float64, gs)
        close(g, r64["grad"], 1e-12, name="analytic dZ against autograd")
        close(loss.view(1), r64["loss"].view(1), 1e-12, name="analytic loss")
        use, valid, ema0, reset = R.ema_case(ename, r64)
        new, held, rec = R.ema_ref(float(r64["loss"]), r64["n"], valid, ema0, R.MU, reset)
        new32, held32, rec32 = R.ema_ref(float(r32["loss"]), r32["n"], valid, ema0, R.MU, reset)
        assert (held, rec) == (held32, rec32)
        if use and reset > 0 and held:
            assert abs(new - reset) >= 1e-3, (ename, new, reset)
        if use:
            seen.add((valid, held, rec, reset > 0))
    # invalid and valid running means; recovery off, not reached, reached; a threshold set while no mean is held
    if K > 1:
        assert {(0, 1, 0, False), (0, 1, 1, True), (1, 1, 0, False), (1, 1, 0, True), (1, 1, 1, True), (0, 0, 0, True)} <= seen, seen


def test_the_ascent_step_reference_in_fp32_meets_tol_and_has_length_rho():
    n, params, grads, theta0, _ = E.slab_input()
    n64, e64 = R.perturb_ref(grads, torch.float64, R.RHO_SLAB)
    n32, e32 = R.perturb_ref(grads, torch.float32, R.RHO_SLAB)
    close(n32.view(1), n64.view(1), TOL, name="norm")
    assert sorted(e64) == [j for j, ch in enumerate(E.ACHUNKS) if ch in E.LIVE] and len(e64) == len(E.LIVE)
    for j in e64:
        close(e32[j], e64[j], TOL, name=f"e chunk {j}")
    assert abs(math.sqrt(sum(float(v.pow(2).sum()) for v in e64.values())) - R.RHO_SLAB) < 1e-9
    # it is the gradient of rho |g| -- the first-order rise of a loss whose gradient is g, along its steepest ascent
    g = torch.cat([grads[ch * 1024:(ch + 1) * 1024] for ch in E.LIVE]).double().requires_grad_(True)
    (d,) = torch.autograd.grad(R.RHO_SLAB * g.norm(), [g])
    close(torch.cat([e64[j] for j in sorted(e64)]), d, 1e-9, name="e against autograd of rho |g|")
    nz, ez = R.perturb_ref(torch.zeros_like(grads), torch.float64, R.RHO_SLAB)
    assert float(nz) == 0.0 and all(bool((v == 0).all()) for v in ez.values())


@pytest.mark.parametrize("case", R.PARITY, ids=[c[0] for c in R.PARITY])
def test_parity_batches_are_well_conditioned(case):
    """The preconditions of the GPU step test (R.conditions) on the fp32 restatement's own trajectory: E0 sits in a gap whose
    half-width is >= 100 x the fp32 restatement's error on H in pass 1 and, among the rows pass 1 kept, in pass 2; 25 to 75 % of the
    rows are selected in pass 1; at rho = R.RHO the ascent step moves the entropies of those rows by >= 100 x that error on average;
    the fp32 selections are the float64 ones.  The online batches are reached by the fp32 restatement's own Adam steps."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from stil_tta_amd import STiLModel
    label, mk_hp, B, which, seeds, sseed = case
    hp = mk_hp()
    lr = 1e-3
    sd = E.scaled_state(hp, sseed)
    d = dict(vars(hp))
    d.update(tta=True, tta_method="sar", tta_params=which)
    keys = STiLModel(d).tta_param_names()
    opt = {}
    for step, seed in enumerate(seeds, start=1):
        x, _ = T.tta_batch(hp, B, seed)
        pre = R.sar_pass(sd, keys, x, hp, torch.float64)
        r1_32 = R.sar_pass(sd, keys, x, hp, torch.float32, pre["e0"])
        _, e32 = R.ascent(r1_32["g"], R.RHO)
        sd_pert = R.perturbed(sd, e32)
        r2 = R.sar_pass(sd_pert, keys, x, hp, torch.float64, pre["e0"], prior=r1_32["sel"])
        r2_32 = R.sar_pass(sd_pert, keys, x, hp, torch.float32, pre["e0"], prior=r1_32["sel"])
        bad = R.conditions(label, step, B, pre, r1_32, r2, r2_32)
        assert not bad, bad
        assert r2["n"] > 0, "pass 2 keeps no row: the Adam step of the GPU test would be gated off"
        if step < len(seeds):
            O.adam_step(sd, r2_32["g"], opt, step, lr)
