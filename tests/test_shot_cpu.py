"""CPU side of SHOT-IM test-time adaptation (tests/test_gpu_shot.py): the hparams rules, the closed-form gradient of
include/stil_infomax.h against float64 autograd, and the conditions on the inputs the GPU tests use -- fp32 ATen and the fp32
oracle meet the GPU bars against float64 there, so a kernel or step that misses them is wrong, not unlucky."""
import os
import sys

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import test_gpu_shot as G  # noqa: E402
import test_gpu_tta as T  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402


def _model(**over):
    from stil_tta_amd import STiLModel
    d = dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False)
    d.update(over)
    return STiLModel(d)


def test_shot_im_keys_and_defaults():
    m = _model(tta=True, tta_method="shot_im")
    assert m._tta_on() and not _model(tta=False, tta_method="shot_im")._tta_on() and not _model(tta=True)._tta_on()
    hp = m.hp
    assert (hp.tta_div_weight, hp.tta_div_eps) == (1.0, 1e-5)
    assert (hp.tta_lr, hp.tta_episodic, hp.tta_params, hp.tta_bn_prior) == (1e-3, False, "bn", None)
    from stil_tta_amd import tta
    assert "shot_im" in tta.METHODS and callable(tta.shot_im_step) and callable(tta.infomax)
    assert m._tent is None and m.last_tta == {}


def test_adapted_set_is_tents():
    for which in ("bn", "norm"):
        assert _model(tta=True, tta_method="shot_im", tta_params=which).tta_param_names() == \
            _model(tta=True, tta_method="tent", tta_params=which).tta_param_names()
    names = _model(tta=True, tta_method="shot_im", tta_params="norm").tta_param_names()
    assert not any("classifier" in n for n in names), "SHOT freezes the classifier head: it is never adapted"


@pytest.mark.parametrize("method", [None, "tent", "shot_im"])
def test_weight_and_eps_are_checked_whatever_the_method(method):
    for bad in (-0.1, float("inf"), float("nan"), "1", None, True):
        with pytest.raises(ValueError):
            _model(tta=True, tta_method=method, tta_div_weight=bad)
    for bad in (0.0, -1e-5, float("inf"), float("nan"), "1e-5", None, True):
        with pytest.raises(ValueError):
            _model(tta=True, tta_method=method, tta_div_eps=bad)
    m = _model(tta=True, tta_method=method, tta_div_weight=0, tta_div_eps=1e-8)
    assert (m.hp.tta_div_weight, m.hp.tta_div_eps) == (0, 1e-8)


def test_other_methods_and_saint_are_still_refused():
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="memo")
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="SHOT_IM")
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="shot_im", tta_params="all")
    with pytest.raises(NotImplementedError):
        _model(tta=True, tta_method="shot_im", tabular_encoder="saint")
    with pytest.raises(NotImplementedError):
        _model(tta_method="shot_im", algorithm_name="STiL_SAINT")


@pytest.mark.parametrize("rows,K", [(1, 1), (1, 5), (7, 2), (9, 13)])
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_closed_form_gradient_is_float64_autograd(rows, K, lam):
    """dZ of include/stil_infomax.h, restated in float64, is the autograd gradient of grad_scale (sum_r H_r + lam rows D)."""
    g = torch.Generator().manual_seed(100 * rows + K)
    z = 4.0 * torch.randn(rows, K, generator=g, dtype=torch.float64)
    eps, gs = 1e-5, 0.37
    ref = G.shot_ref(z, lam, eps, torch.float64)
    logp = torch.log_softmax(z, dim=1)
    p = logp.exp()
    H = -(p * logp).sum(1, keepdim=True)
    pbar = p.mean(0)
    c = torch.log(pbar + eps) + pbar / (pbar + eps)
    dz = gs * p * (-(logp + H) + lam * (c[None, :] - (p * c[None, :]).sum(1, keepdim=True)))
    assert float((dz - ref["grad"] * gs * rows).abs().max()) <= 1e-13 * (1.0 + float(ref["grad"].abs().max()) * gs * rows)


@pytest.mark.parametrize("rows,K,kind,lam", G.shot_cases())
def test_fp32_aten_infomax_meets_tol(rows, K, kind, lam):
    """fp32 ATen meets every bar of test_infomax_rows_against_float64 on its inputs; one_class is the collapsed batch."""
    z = G.shot_input(rows, K, kind)
    r64 = G.shot_ref64(rows, K, kind, lam)
    r32 = G.shot_ref(z, G.f32(lam), G.f32(G.EPS), torch.float32)
    if kind == "one_class" and K > 1:
        others = torch.ones(K, dtype=torch.bool)
        others[K // 2] = False
        assert float(r64["pbar"][others].max()) < 1e-3 * G.EPS and float(r64["pbar"][K // 2]) > 0.999
    for k in ("lse", "probs", "H", "pbar", "grad", "loss", "ent", "D"):
        assert bool(torch.isfinite(r64[k]).all()), k
        a, b = (r[k].view(-1) if r[k].ndim == 0 else r[k] for r in (r32, r64))
        close(a, b, TOL, name=k)


@pytest.mark.parametrize("case", G.PARITY, ids=[c[0] for c in G.PARITY])
def test_fp32_oracle_meets_the_prediction_and_loss_bars(case):
    """The step test's bars on predictions (_scaled <= 3e-5) and on the two loss values (close() at TOL) are reachable: the
    fp32 oracle meets them against float64 on every batch; the online batches are reached by the fp32 oracle's own Adam steps
    (the GPU test reaches them by the device's)."""
    from test_gpu_step import _scaled
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    label, mk_hp, B, which, seeds, sseed, head = case
    hp = mk_hp()
    sd = G.parity_state(hp, sseed, head)
    keys = _model(**{**vars(hp), "tta": True, "tta_method": "shot_im", "tta_params": which}).tta_param_names()
    opt = {}
    for step, seed in enumerate(seeds, start=1):
        x, _ = T.tta_batch(hp, B, seed)
        r32 = G.shot_restated(sd, keys, x, hp, torch.float32, 1.0, G.EPS)
        r64 = G.shot_restated(sd, keys, x, hp, torch.float64, 1.0, G.EPS)
        d = _scaled(r32["p"].double().numpy(), r64["p"].numpy())
        worst = max(T._rel(r32["g"][k].double(), r64["g"][k]) for k in keys)
        print(f"[{label}] batch {step}: fp32 oracle predictions scaled error {d:.2e}; loss_entropy {float(r64['l_ent']):.5f} "
              f"(fp32 off by {abs(float(r32['l_ent']) - float(r64['l_ent'])):.2e}), loss_diversity {float(r64['D']):.5f} "
              f"(fp32 off by {abs(float(r32['D']) - float(r64['D'])):.2e}); worst e32 {worst:.2e}; "
              f"largest marginal {float(r64['pbar'].max()):.3f}")
        assert d <= 3e-5
        close(r32["l_ent"].view(1), r64["l_ent"].view(1), TOL, name="loss_entropy")
        close(r32["D"].view(1), r64["D"].view(1), TOL, name="loss_diversity")
        if step < len(seeds):
            O.adam_step(sd, r32["g"], opt, step, G.PARITY_LR)
