"""CPU side of the test-time BatchNorm memory (csrc/stil_bnmemory.h, ops.bn_memory, tta.BnMemory, tta_bn_momentum, tta_method
"dua"): defaults and refusals (hparams, scope, and the C ABI's, which refuses before any launch and so needs no GPU), DUA's schedule,
the unchanged prior backward against float64 autograd of the forward with the memory detached, a stream of updates against the
unrolled EMA, and the fp32 ATen restatement against the bar tests/test_gpu_bnmemory.py holds the kernels to, on its inputs."""
import ctypes
import os
import sys

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from bnmemory_cases import RHO_ALPHA, SHAPES, TOL, layer_inputs, memory_bn, momentum  # noqa: E402
from test_bnprior_cpu import EPS, _model, closed_form_backward  # noqa: E402


def test_defaults_are_off():
    hp = _model().hp
    assert hp.tta_bn_momentum is None and hp.tta_bn_momentum_decay == 1.0 and hp.tta_bn_momentum_min == 0.0
    m = _model(tta=True, tta_method="tent")
    assert m._bn_mem is None
    from stil_tta_amd import tta
    assert "dua" in tta.METHODS and tta.STEPS["dua"] is tta.dua_step


def test_hparam_refusals():
    for key, bads in (("tta_bn_momentum", (0, 0.0, -0.1, 1.5, True, False, float("nan"), float("inf"), "0.1")),
                      ("tta_bn_momentum_decay", (0.0, -1.0, 1.01, True, None, float("nan"), float("inf"), "1")),
                      ("tta_bn_momentum_min", (-0.01, 1.5, True, None, float("nan"), float("inf"), "0"))):
        for bad in bads:
            with pytest.raises(ValueError):
                _model(**{"tta": True, "tta_method": "tent", "tta_bn_momentum": 0.05, key: bad})
    with pytest.raises(ValueError, match="tta_bn_momentum"):
        _model(tta=True, tta_method="dua")
    for method in ("tent", "eata", "shot_im", "marginal_entropy", "deyo", "sar", "bn_adapt", "dua"):
        m = _model(tta=True, tta_method=method, tta_bn_momentum=0.1, tta_bn_momentum_decay=0.94, tta_bn_momentum_min=0.005)
        assert m._tta_on() and m._bn_mem is None and m._tent is None
    assert _model(tta=True, tta_method="tent", tta_bn_momentum=1, tta_bn_momentum_min=0).hp.tta_bn_momentum == 1
    with pytest.raises(NotImplementedError):
        _model(tta=True, tta_method="dua", tta_bn_momentum=0.1, tabular_encoder="saint")


def test_the_schedule_in_closed_form():
    from stil_tta_amd import tta
    hp = _model(tta=True, tta_method="dua", tta_bn_momentum=0.1, tta_bn_momentum_decay=0.94, tta_bn_momentum_min=0.005).hp
    want = [0.1 * 0.94 + 0.005, 0.1 * 0.94 ** 2 + 0.005]
    assert abs(want[0] - 0.099) < 1e-15 and abs(want[1] - 0.09336) < 1e-15
    for t in (1, 2, 3, 10, 100, 1000):
        a = tta.bn_momentum(hp, t)
        assert abs(a - (0.1 * 0.94 ** t + 0.005)) <= 1e-15 and a == momentum(0.1, 0.94, 0.005, t)
    assert abs(tta.bn_momentum(hp, 1000) - 0.005) < 1e-15     # the floor
    flat = _model(tta=True, tta_method="tent", tta_bn_momentum=0.05).hp
    assert all(tta.bn_momentum(flat, t) == 0.05 for t in (1, 2, 50))
    capped = _model(tta=True, tta_method="tent", tta_bn_momentum=0.9, tta_bn_momentum_min=0.5).hp
    assert tta.bn_momentum(capped, 1) == 1.0


def test_scope_arguments_and_nesting():
    from stil_tta_amd import ops
    for rho, alpha in ((-0.1, 0.5), (1.1, 0.5), (float("nan"), 0.5), (0.5, -0.1), (0.5, 1.1), (0.5, float("nan"))):
        with pytest.raises(ValueError):
            ops.bn_memory(object(), rho, alpha)
    assert ops._bn_memory is None
    mem = object()
    with ops.bn_memory(mem, 0.2, 0.5, unbiased=True, update=False) as _:
        s = ops._bn_memory
        assert s.mem is mem and (s.rho, s.alpha, s.unbiased, s.update) == (0.2, 0.5, True, False)
        with ops.bn_memory(mem, 1.0, 0.1):
            assert ops._bn_memory.rho == 1.0 and ops._bn_memory.update
        assert ops._bn_memory is s
    assert ops._bn_memory is None
    with ops.bn_prior(16, 16), pytest.raises(RuntimeError):
        with ops.bn_memory(mem, 0.2, 0.5):
            pass
    assert ops._bn_memory is None and ops._bn_prior is None


def test_the_c_abi_refuses_bad_memory_arguments_before_any_launch():
    """No GPU is needed: every refusal returns before the first launch.  The pointers are never dereferenced."""
    from stil_tta_amd._lib import lib
    L = lib()
    D = L._dll
    C, M = 64, 49
    P = ctypes.c_void_p
    base = 1 << 20
    x, ga, be, mm, mv, om, ov, z, st, dl, ws, ts = (P(base * (i + 1)) for i in range(12))

    def fwd(alpha=0.5, unb=0, rho=0.5, m=mm, v=mv, o1=om, o2=ov, C_=C, nb=1 << 20, xx=x):
        return D.stil_bn_memory_fwd(xx, ga, be, m, v, o1, o2, alpha, unb, rho, None, z, st, dl, M, C_, 1, EPS, ws, nb, None)

    def fwd_t(alpha=0.5, unb=0, rho=0.5, m=mm, v=mv, o1=om, o2=ov, C_=C, nb=1 << 20, xx=x):
        return D.stil_bn_memory_fwd_tiles(xx, ts, 64, ga, be, m, v, o1, o2, alpha, unb, rho, None, None, z, st, dl, M, C_, 1, EPS, ws, nb, None)

    for fn in (fwd, fwd_t):
        for alpha in (-0.1, 1.5, float("nan"), float("inf")):
            assert fn(alpha=alpha) != 0 and "alpha" in L.last_error(), (fn.__name__, alpha)
            assert fn(alpha=alpha, o1=None, o2=None) != 0 and "alpha" in L.last_error()      # also when nothing would be updated
        assert fn(unb=2) != 0 and "unbiased" in L.last_error()
        assert fn(o1=None) != 0 and "without the other" in L.last_error() and fn(o2=None) != 0 and "without the other" in L.last_error()
        for kw in (dict(o1=mm), dict(o1=mv), dict(o2=mm), dict(o2=mv), dict(o2=om), dict(o1=P(base * 4 + 4 * (C - 1))),
                   dict(o2=P(base * 5 - 4 * (C - 1)))):
            assert fn(**kw) != 0 and "alias" in L.last_error(), (fn.__name__, kw)
        for rho in (-0.1, 1.5, float("nan")):
            assert fn(rho=rho) != 0 and "rho" in L.last_error()
            assert fn(rho=rho, o1=None, o2=None) != 0 and "rho" in L.last_error()
        assert fn(xx=None) != 0 and "null" in L.last_error() and fn(m=None) != 0 and "null" in L.last_error() and fn(v=None) != 0
        assert fn(nb=8) != 0 and "workspace" in L.last_error()
        assert fn(nb=8, o1=None, o2=None) != 0 and "workspace" in L.last_error()
    assert fwd(C_=4) != 0 and "64" in L.last_error() and fwd_t(C_=6) != 0


# ------------------------------------------------------------------------------------------ the backward is the prior's
@pytest.mark.parametrize("M", [1, 2, 49])
@pytest.mark.parametrize("rho,alpha", [(0.05, 0.05), (0.2, 0.5), (1.0, 0.1)])
@pytest.mark.parametrize("relu,resid", [(False, False), (True, False), (True, True)])
def test_prior_backward_is_float64_autograd_of_the_memory_forward(M, rho, alpha, relu, resid):
    """The memory is a constant of the step and m', s' feed nothing the loss sees: closed_form_backward at the same rho and delta is
    the gradient, to the 1e-11 of tests/test_bnprior_cpu.py."""
    C = 6
    g_ = torch.Generator().manual_seed(100 * M + int(100 * rho))
    x = (3.0 + 2.0 * torch.randn(M, C, generator=g_, dtype=torch.float64)).requires_grad_()
    gamma = (0.5 + torch.rand(C, generator=g_, dtype=torch.float64)).requires_grad_()
    beta = (0.3 * torch.randn(C, generator=g_, dtype=torch.float64)).requires_grad_()
    m = (3.0 + torch.randn(C, generator=g_, dtype=torch.float64)).requires_grad_()     # a leaf, so that "detached" is checked below
    s = 0.5 + 4.0 * torch.rand(C, generator=g_, dtype=torch.float64)
    s[0] = 0.0
    s.requires_grad_()
    res = torch.randn(M, C, generator=g_, dtype=torch.float64) if resid else None
    dz = torch.randn(M, C, generator=g_, dtype=torch.float64)
    for unbiased in (0, 1):
        z, xhat, mu, r, delta, m1, s1 = memory_bn(x, gamma, beta, m.detach(), s.detach(), rho, alpha, unbiased, res, relu)
        dx_a, dgamma_a, dbeta_a, dm, ds = torch.autograd.grad(z, [x, gamma, beta, m, s], dz, allow_unused=True)
        assert dm is None and ds is None
        g = dz * (z.detach() > 0) if relu else dz
        dx, dgamma, dbeta = closed_form_backward(g, xhat.detach(), gamma.detach(), r.detach(), delta.detach(), rho)
        for name, a, b in (("dx", dx, dx_a), ("dgamma", dgamma, dgamma_a), ("dbeta", dbeta, dbeta_a)):
            assert float((a - b).abs().max()) <= 1e-11 * (1.0 + float(b.abs().max())), (name, float((a - b).abs().max()))
        xd = x.detach()
        mu_b = xd.mean(0)
        v_b = xd.var(0, unbiased=False)
        assert torch.allclose(m1.detach(), (1 - alpha) * m.detach() + alpha * mu_b, rtol=0, atol=1e-14)
        want = xd.var(0, unbiased=True) if (unbiased and M > 1) else v_b          # M = 1: no division by M - 1 = 0
        assert bool(torch.isfinite(s1).all()) and torch.allclose(s1.detach(), (1 - alpha) * s.detach() + alpha * want, rtol=0, atol=1e-13)
        if rho == 1.0 and M > 1 and unbiased:    # nn.BatchNorm2d's training-mode rule, which DUA relies on
            bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=alpha).double()
            bn.running_mean.copy_(m.detach())
            bn.running_var.copy_(s.detach())
            with torch.no_grad():
                bn.weight.copy_(gamma)
                bn.bias.copy_(beta)
                ref = bn(xd)
            zz = ref + res if resid else ref
            assert float(((torch.relu(zz) if relu else zz) - z.detach()).abs().max()) <= 1e-12 * (1.0 + float(z.detach().abs().max()))
            assert torch.allclose(bn.running_mean, m1.detach(), rtol=0, atol=1e-13) and torch.allclose(bn.running_var, s1.detach(), rtol=0, atol=1e-13)


def test_a_stream_of_six_batches_is_the_unrolled_ema():
    C, a0, om, amin = 5, 0.1, 0.94, 0.005
    g_ = torch.Generator().manual_seed(3)
    xs = [2.0 + torch.randn(M, C, generator=g_, dtype=torch.float64) * (1.0 + 0.3 * i) for i, M in enumerate((1, 4, 2, 9, 1, 16))]
    gamma, beta = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    m0, s0 = torch.randn(C, generator=g_, dtype=torch.float64), 0.5 + torch.rand(C, generator=g_, dtype=torch.float64)
    m, s = m0, s0
    alphas = [momentum(a0, om, amin, t) for t in range(1, 7)]
    for x, a in zip(xs, alphas):
        z, _, mu, _, _, m_new, s_new = memory_bn(x, gamma, beta, m, s, a, a, 0)
        # rho = alpha (RoTTA): the layer normalises by exactly the updated estimate
        assert torch.allclose(mu, m_new, rtol=0, atol=1e-14)
        assert torch.allclose(z, (x - m_new) / torch.sqrt(s_new + EPS), rtol=0, atol=1e-12)
        m, s = m_new, s_new
    keep = [1.0] * 6
    for k in range(6):
        for j in range(k + 1, 6):
            keep[k] *= 1 - alphas[j]
    w0 = 1.0
    for a in alphas:
        w0 *= 1 - a
    m_unrolled = w0 * m0 + sum(alphas[k] * keep[k] * xs[k].mean(0) for k in range(6))
    s_unrolled = w0 * s0 + sum(alphas[k] * keep[k] * xs[k].var(0, unbiased=False) for k in range(6))
    assert torch.allclose(m, m_unrolled, rtol=0, atol=1e-13) and torch.allclose(s, s_unrolled, rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------ the GPU test's bar is reachable
def _within(a, b, name):
    b = b.double()
    err = (a.double() - b).abs()
    scale = float(b.abs().max())
    worst = float((err / (TOL * (1.0 + b.abs() + scale))).max())
    assert worst <= 1.0, f"{name}: fp32 ATen misses the GPU test's bar by a factor {worst:.2f}"
    return worst


def memory_bn_fp32(y, gamma, beta, m, s, rho, alpha, unbiased, resid, mask):
    """memory_bn with every wide operation in float32, in the manner csrc/stil_bnmemory.h prescribes: the batch statistics from sums
    about a pilot value (row 0) with the mean rounded to float32 at its full magnitude, the blends and r in double and rounded once,
    delta from the rounded mean and r, z = (y - mu) (gamma r) + beta in float32.  (A plain float32 memory_bn, whose batch mean sums
    values 50 standard deviations from zero, misses the bar on two of these inputs by factors 1.8 and 1.2: the reason the kernels
    shift their sums.)  -> (z, None, mu, r, delta, m', s'), float32"""
    M = y.shape[0]
    pilot = y[0]
    dl = y - pilot
    d = dl.mean(0)
    mean_b = pilot + d
    var_b = ((dl * dl).mean(0) - d * d).clamp_min(0.0)
    mu = (1 - rho) * m.double() + rho * mean_b.double()
    r = 1.0 / torch.sqrt((1 - rho) * s.double() + rho * var_b.double() + EPS)
    muf, rf = mu.float(), r.float()
    delta = ((muf.double() - mean_b.double()) * rf.double()).float()
    z = ((y - muf) * (gamma * rf) + beta + resid) * mask.float()
    c = M / (M - 1) if (unbiased and M > 1) else 1.0
    return (z, None, muf, rf, delta, ((1 - alpha) * m.double() + alpha * mean_b.double()).float(),
            ((1 - alpha) * s.double() + alpha * c * var_b.double()).float())


@pytest.mark.parametrize("M,C", SHAPES)
def test_fp32_aten_meets_the_gpu_tests_bar_on_its_inputs(M, C):
    """z, stats (mu, r, gamma r), delta, m', s' of the float32 restatement against the float64 one at close() / 2e-5, for every (rho,
    alpha) and both variance rules, on the layer inputs tests/test_gpu_bnmemory.py uses (the ReLU decisions are the float64 side's,
    as the GPU test hands the device's to its reference)."""
    c = layer_inputs(M, C)
    y32, y64 = c["y"], c["y"].double()
    worst = 0.0
    for rho, alpha in RHO_ALPHA:
        for unbiased in (0, 1):
            ref = memory_bn(y64, c["gamma"].double(), c["beta"].double(), c["rm"].double(), c["rv"].double(), rho, alpha, unbiased,
                            c["resid"].double(), True)
            got = memory_bn_fp32(y32, c["gamma"], c["beta"], c["rm"], c["rv"], rho, alpha, unbiased, c["resid"], ref[0] > 0)
            names = ("z", "xhat", "mu", "r", "delta", "m'", "s'")
            for i in (0, 2, 3, 4, 5, 6):
                assert got[i].dtype == torch.float32
                worst = max(worst, _within(got[i], ref[i], f"rho={rho} alpha={alpha} unbiased={unbiased} {names[i]}"))
            worst = max(worst, _within(c["gamma"] * got[3], c["gamma"].double() * ref[3], "gamma r"))
    print(f"M={M} C={C}: fp32 ATen uses at most {worst:.3f} of the bar")
