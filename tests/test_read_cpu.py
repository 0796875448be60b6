"""CPU side of READ test-time adaptation (tests/test_gpu_read.py): the hparams rules, the adapted set, the closed-form gradient of
csrc/stil_read.h against float64 autograd, and the conditions on the inputs the GPU tests use -- fp32 ATen and the fp32 oracle meet
the GPU bars against float64 there, the predicted class is unambiguous and rows lie on both sides of gamma, so a kernel or step
that misses them is wrong, not unlucky."""
import math
import os
import sys

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import test_gpu_read as G  # noqa: E402
import test_gpu_tta as T  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402
from test_gpu_shot import f32, parity_state  # noqa: E402


def _model(**over):
    from stil_tta_amd import STiLModel
    d = dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False)
    d.update(over)
    return STiLModel(d)


def _read(**over):
    return _model(**{**dict(tta=True, tta_method="read", tta_params="fusion"), **over})


# ------------------------------------------------------------------------------------------ keys, refusals, the adapted set
def test_read_keys_and_defaults():
    m = _read()
    assert m._tta_on() and not _read(tta=False)._tta_on()
    hp = m.hp
    assert hp.tta_read_gamma is None
    assert (hp.tta_div_weight, hp.tta_div_eps) == (1.0, 1e-5)
    assert (hp.tta_lr, hp.tta_episodic, hp.tta_bn_prior, hp.tta_bn_momentum) == (1e-3, False, None, None)
    assert _model().hp.tta_params == "bn" and _model().hp.tta_read_gamma is None
    from stil_tta_amd import tta
    assert tta.PARAMS == ("bn", "norm", "fusion")
    assert tta.read_gamma(hp) == math.exp(-1.0) and tta.read_gamma(_read(tta_read_gamma=0.5).hp) == 0.5
    assert _read(tta_read_gamma=1).hp.tta_read_gamma == 1 and _read(tta_div_weight=0).hp.tta_div_weight == 0
    assert m._tent is None and m.last_tta == {}


def test_read_is_a_registered_method():
    from stil_tta_amd import tta
    assert "read" in tta.METHODS and tta.STEPS["read"] is tta.read_step and callable(tta.read_loss) and callable(tta.fusion_pass)


def test_read_and_fusion_need_each_other():
    with pytest.raises(ValueError, match="fusion"):
        _model(tta=True, tta_method="read")                       # tta_params defaults to "bn"
    with pytest.raises(ValueError, match="fusion"):
        _model(tta=True, tta_method="read", tta_params="norm")
    for method in (None, "tent", "eata", "shot_im", "bn_adapt", "marginal_entropy", "deyo", "sar"):
        with pytest.raises(ValueError, match="read"):
            _model(tta=True, tta_method=method, tta_params="fusion")
    with pytest.raises(ValueError, match="read"):
        _model(tta=True, tta_method="dua", tta_bn_momentum=0.1, tta_params="fusion")


def test_bad_gamma_is_refused_whatever_the_method():
    for method, params in ((None, "bn"), ("tent", "bn"), ("read", "fusion")):
        for bad in (0.0, -0.1, 1.0000001, 2, float("inf"), float("nan"), "0.3", True, False):
            with pytest.raises(ValueError, match="tta_read_gamma"):
                _model(tta=True, tta_method=method, tta_params=params, tta_read_gamma=bad)
        assert _model(tta=True, tta_method=method, tta_params=params, tta_read_gamma=0.25).hp.tta_read_gamma == 0.25


def test_read_refuses_the_batchnorm_prior_and_memory():
    for key, v in (("tta_bn_prior", 16), ("tta_bn_prior", 0), ("tta_bn_momentum", 0.05), ("tta_bn_momentum", 1.0)):
        with pytest.raises(ValueError, match=key):
            _read(**{key: v})


def test_all_and_saint_are_still_refused():
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="read", tta_params="all")
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="tent", tta_params="all")
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="READ", tta_params="fusion")
    with pytest.raises(NotImplementedError):
        _read(tabular_encoder="saint")
    with pytest.raises(NotImplementedError):
        _model(tta_method="read", tta_params="fusion", algorithm_name="STiL_SAINT")


def test_adapted_set_is_the_last_fusion_layers_qkv():
    m1 = _read()
    assert m1.tta_param_names() == ["model.transformer.0.attn.qkv.weight", "model.transformer.0.attn.qkv.bias"]
    m2 = _read(multimodal_transformer_num_layers=2)
    assert m2.tta_param_names() == ["model.transformer.1.attn.qkv.weight", "model.transformer.1.attn.qkv.bias"]
    for m in (m1, m2):
        sd = m.state_dict()
        C = m.hp.multimodal_embedding_dim
        w, b = (sd[n] for n in m.tta_param_names())
        assert tuple(w.shape) == (3 * C, C) and tuple(b.shape) == (3 * C,)
        assert m.tta_param_names() == G.fusion_keys(m.hp)
    # the other adapted sets are what they were
    assert len(_model(tta=True, tta_method="tent").tta_param_names()) == 106


# ------------------------------------------------------------------------------------------ the closed form
@pytest.mark.parametrize("rows,K", [(1, 1), (1, 5), (7, 2), (9, 13)])
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("gamma", [math.exp(-1.0), 0.1, 1.0])
def test_closed_form_gradient_is_float64_autograd(rows, K, lam, gamma):
    """dZ of csrc/stil_read.h, restated in float64, is the autograd gradient of grad_scale (sum_r f_r + lam rows D), and
    out[0] is its value over rows."""
    g = torch.Generator().manual_seed(100 * rows + K)
    z = 2.0 * torch.randn(rows, K, generator=g, dtype=torch.float64)
    eps, gs = 1e-5, 0.37
    ref = G.read_ref(z, gamma, lam, eps, torch.float64)
    logp = torch.log_softmax(z, dim=1)
    p = logp.exp()
    yhat = G.first_max(z)
    c = p.gather(1, yhat.view(-1, 1))
    onehot = torch.zeros_like(p).scatter_(1, yhat.view(-1, 1), 1.0)
    pbar = p.mean(0)
    ck = torch.log(pbar + eps) + pbar / (pbar + eps)
    dz = gs * (torch.log(gamma / c) * c * (onehot - p) + lam * p * (ck[None, :] - (p * ck[None, :]).sum(1, keepdim=True)))
    assert float((dz - ref["grad"] * gs * rows).abs().max()) <= 1e-13 * (1.0 + float(ref["grad"].abs().max()) * gs * rows)
    f = c.squeeze(1) * torch.log(math.e * gamma / c.squeeze(1))
    assert float((f - ref["f"]).abs().max()) <= 1e-14
    assert abs(float(f.mean() + lam * (pbar * torch.log(pbar + eps)).sum()) - float(ref["loss"])) <= 1e-14
    if gamma == math.exp(-1.0):
        assert float((f + c.squeeze(1) * torch.log(c.squeeze(1))).abs().max()) <= 1e-14   # gamma = 1/e: f = -c ln c


# ------------------------------------------------------------------------------------------ reachability of the kernel bar
def test_near_gamma_rows_lie_on_both_sides_of_the_sign_change():
    for rows in T.ENT_ROWS:
        for K in T.ENT_K:
            z = G.read_input(rows, K, "near_gamma")
            c = torch.softmax(z.double(), dim=1).max(dim=1).values
            assert bool(((c > 1.0 / K - 1e-12) & (c <= 1.0)).all())
            if K == 1:
                assert bool((c == 1).all())
            elif rows >= 7 and K > 2:      # K = 2: c > 0.5 > 1.5 / e, one side only
                assert int((c < G.GAMMA).sum()) >= rows // 4 and int((c > G.GAMMA).sum()) >= rows // 4, (rows, K)
            if K > 1:
                top2 = z.double().topk(2, dim=1).values
                assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-3, "the predicted class must be unambiguous"


@pytest.mark.parametrize("rows,K,kind,lam", G.read_cases())
def test_fp32_aten_read_meets_tol(rows, K, kind, lam):
    """fp32 ATen meets every bar of test_read_rows_against_float64 on its inputs, with the same yhat."""
    z = G.read_input(rows, K, kind)
    r64 = G.read_ref64(rows, K, kind, lam)
    r32 = G.read_ref(z, f32(G.GAMMA), f32(lam), f32(G.EPS), torch.float32)
    assert torch.equal(r32["yhat"], r64["yhat"])
    worst = 0.0
    for k in ("lse", "probs", "conf", "f", "pbar", "grad", "loss", "conf_loss", "D"):
        assert bool(torch.isfinite(r64[k]).all()), k
        a, b = (r[k].view(-1) if r[k].ndim == 0 else r[k] for r in (r32, r64))
        if k == "grad":
            b64 = b.double()
            worst = float(((a.double() - b64).abs() / (TOL * (1.0 + b64.abs() + float(b64.abs().max())))).max())
        close(a, b, TOL, name=k)
    print(f"rows {rows} K {K} {kind} lam {lam}: fp32 dZ error / bar {worst:.3f}")


# ------------------------------------------------------------------------------------------ reachability of the step bars
@pytest.mark.parametrize("case", G.PARITY, ids=[c[0] for c in G.PARITY])
def test_fp32_oracle_meets_the_step_bars_and_the_cases_are_well_posed(case):
    """On every batch of every step case: the fp32 restatement's predictions are within _scaled <= 3e-5 of float64; the gap between
    the two largest float64 logits of every row is at least 100 times that row's fp32-float64 logit difference (yhat is
    unambiguous); at least a quarter of the rows lie below gamma and at least a quarter above.  The online batches are reached by
    the fp32 oracle's own Adam steps (the GPU test reaches them by the device's)."""
    from test_gpu_step import _scaled
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    label, mk_hp, B, seeds, sseed, head, gamma = case
    hp = mk_hp()
    sd = parity_state(hp, sseed, head)
    gam = G.case_gamma(gamma)
    keys = _read(**{**vars(hp), "tta_read_gamma": gamma}).tta_param_names()
    assert keys == G.fusion_keys(hp)
    opt = {}
    for step, seed in enumerate(seeds, start=1):
        x, _ = T.tta_batch(hp, B, seed)
        r32 = G.read_restated(sd, keys, x, hp, torch.float32, gam, 1.0, G.EPS)
        r64 = G.read_restated(sd, keys, x, hp, torch.float64, gam, 1.0, G.EPS)
        d = _scaled(r32["p"].double().numpy(), r64["p"].numpy())
        top2 = r64["out_m"].topk(2, dim=1).values
        gap = top2[:, 0] - top2[:, 1]
        dz = (r32["out_m"].double() - r64["out_m"]).abs().max(dim=1).values
        ratio = float((gap / dz.clamp_min(1e-300)).min())
        below, above = int((r64["conf"] < gam).sum()), int((r64["conf"] > gam).sum())
        worst = max(T._rel(r32["g"][k].double(), r64["g"][k]) for k in keys)
        print(f"[{label}] batch {step}: fp32 oracle predictions scaled error {d:.2e}; smallest gap / logit error {ratio:.2e}; "
              f"{below} rows below gamma = {gam:.4f}, {above} above (confidences {float(r64['conf'].min()):.3f} .. "
              f"{float(r64['conf'].max()):.3f}, median {float(r64['conf'].median()):.3f}); worst e32 {worst:.2e}")
        assert d <= 3e-5
        assert torch.equal(r32["yhat"], r64["yhat"]) and ratio >= 100.0
        assert 4 * below >= B and 4 * above >= B
        assert all(bool(torch.isfinite(r64["g"][k]).all()) and float(r64["g"][k].norm()) > 0 for k in keys)
        if step < len(seeds):
            O.adam_step(sd, r32["g"], opt, step, G.PARITY_LR)
