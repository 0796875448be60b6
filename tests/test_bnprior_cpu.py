"""CPU side of test-time BatchNorm with a source-statistics prior (include/stil_bnprior.h, ops.bn_prior, tta_bn_prior, tta_method
"bn_adapt"): the closed-form backward the HIP kernels implement against float64 autograd of the blended forward, and the
hparams rules.  tests/test_gpu_bnprior.py checks the kernels and the steps against the same restatement (blended_bn)."""
import os
import sys

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

EPS = 1e-5


def blended_bn(x, gamma, beta, mu_s, v_s, rho, resid=None, relu=False, mask=None):
    """The blended forward on rows x [M, C] in x's dtype, differentiable: z = relu?(gamma xhat + beta + resid?).
    mask (optional, bool [M, C]): the ReLU decisions to use instead of the forward's own.  -> (z, xhat, mu, r, delta)"""
    mu_b = x.mean(0)
    v_b = ((x - mu_b) ** 2).mean(0)
    mu = (1 - rho) * mu_s + rho * mu_b
    v = (1 - rho) * v_s + rho * v_b
    r = 1.0 / torch.sqrt(v + EPS)
    xhat = (x - mu) * r
    z = gamma * xhat + beta
    if resid is not None:
        z = z + resid
    if relu:
        z = z * mask.to(z.dtype) if mask is not None else torch.relu(z)
    return z, xhat, mu, r, (mu - mu_b) * r


def closed_form_backward(g, xhat, gamma, r, delta, rho):
    """dx, dgamma, dbeta of include/stil_bnprior.h from g = dL/dz after the ReLU mask."""
    k2, k3 = g.mean(0), (g * xhat).mean(0)
    dx = gamma * r * (g - rho * (k2 + delta * k3) - rho * k3 * xhat)
    return dx, (g * xhat).sum(0), g.sum(0)


@pytest.mark.parametrize("M", [1, 49])
@pytest.mark.parametrize("rho", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("relu,resid", [(False, False), (True, False), (True, True)])
def test_closed_form_backward_is_float64_autograd_of_the_blended_forward(M, rho, relu, resid):
    C = 6
    g_ = torch.Generator().manual_seed(100 * M + int(10 * rho))
    x = (3.0 + 2.0 * torch.randn(M, C, generator=g_, dtype=torch.float64)).requires_grad_()
    gamma = (0.5 + torch.rand(C, generator=g_, dtype=torch.float64)).requires_grad_()
    beta = (0.3 * torch.randn(C, generator=g_, dtype=torch.float64)).requires_grad_()
    mu_s = 3.0 + torch.randn(C, generator=g_, dtype=torch.float64)
    v_s = 0.5 + 4.0 * torch.rand(C, generator=g_, dtype=torch.float64)
    v_s[0] = 0.0
    res = torch.randn(M, C, generator=g_, dtype=torch.float64) if resid else None
    dz = torch.randn(M, C, generator=g_, dtype=torch.float64)
    z, xhat, mu, r, delta = blended_bn(x, gamma, beta, mu_s, v_s, rho, res, relu)
    dx_a, dgamma_a, dbeta_a = torch.autograd.grad(z, [x, gamma, beta], dz)
    g = dz * (z.detach() > 0) if relu else dz
    dx, dgamma, dbeta = closed_form_backward(g, xhat.detach(), gamma.detach(), r.detach(), delta.detach(), rho)
    for name, a, b in (("dx", dx, dx_a), ("dgamma", dgamma, dgamma_a), ("dbeta", dbeta, dbeta_a)):
        assert float((a - b).abs().max()) <= 1e-11 * (1.0 + float(b.abs().max())), (name, float((a - b).abs().max()))
    if rho == 1.0:
        assert float(delta.detach().abs().max()) == 0.0
    if rho == 1.0 and M > 1:   # training-mode BatchNorm (ATen refuses one value per channel)
        ref = torch.nn.functional.batch_norm(x.detach(), None, None, gamma.detach(), beta.detach(), training=True, eps=EPS)
        zz = ref + res if resid else ref
        assert float(((torch.relu(zz) if relu else zz) - z.detach()).abs().max()) <= 1e-12 * (1.0 + float(z.detach().abs().max()))
    if rho == 0.0:   # eval mode: the gradient passes straight through
        ref = torch.nn.functional.batch_norm(x.detach(), mu_s, v_s, gamma.detach(), beta.detach(), training=False, eps=EPS)
        zz = ref + res if resid else ref
        assert float(((torch.relu(zz) if relu else zz) - z.detach()).abs().max()) <= 1e-12 * (1.0 + float(z.detach().abs().max()))
        assert torch.equal(dx, gamma.detach() * r.detach() * g)


def _model(**over):
    from stil_tta_amd import STiLModel
    d = dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False)
    d.update(over)
    return STiLModel(d)


def test_hparam_rules():
    assert _model().hp.tta_bn_prior is None
    for bad in (-1.0, float("nan"), float("inf"), "16", True):
        with pytest.raises(ValueError):
            _model(tta=True, tta_method="tent", tta_bn_prior=bad)
    for ok in (0, 0.0, 16, 2.5):
        assert _model(tta=True, tta_method="eata", tta_bn_prior=ok).hp.tta_bn_prior == ok
    m = _model(tta=True, tta_method="bn_adapt")
    assert m._tta_on() and m._tent is None
    assert not _model(tta=False, tta_method="bn_adapt")._tta_on()
    assert _model(tta=True, tta_method="bn_adapt", tta_bn_prior=16.0)._tta_on()
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="memo")
    with pytest.raises(NotImplementedError):
        _model(tta=True, tta_method="bn_adapt", tabular_encoder="saint")


def test_bn_prior_scope_arguments():
    from stil_tta_amd import ops
    assert ops.bn_prior(0, 8).rho == 1.0 and ops.bn_prior(16, 16).rho == 0.5 and ops.bn_prior(64.0, 8).rho == 8 / 72
    for N, B in ((-1, 8), (float("nan"), 8), (float("inf"), 8), (16, 0)):
        with pytest.raises(ValueError):
            ops.bn_prior(N, B)
    assert ops._bn_prior is None
    with ops.bn_prior(16, 16):
        assert ops._bn_prior == 0.5
        with ops.bn_prior(0, 4):
            assert ops._bn_prior == 1.0
        assert ops._bn_prior == 0.5
    assert ops._bn_prior is None
