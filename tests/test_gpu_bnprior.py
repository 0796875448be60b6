"""Test-time BatchNorm with a source-statistics prior (Schneider et al., NeurIPS 2020): include/stil_bnprior.h, ops.bn_prior,
tta_bn_prior and tta_method "bn_adapt".

1. The four entry points against float64 (close() at TOL of test_gpu_ops): two-pass and tile paths, residual / resid_stats /
   z == NULL, the three relu modes, accumulate, gout; sentinels; repetition.  The ReLU mask of the reference is the device's z.
2. rho = 1 equals the existing entry points bit for bit (NULL running buffers), delta == 0.
3. Bad arguments are refused.
4. layer1 + layer2 under bn_prior: deferred / premasked blocks == plain blocks bit for bit, the epilogue's BatchNorm-backward sums
   to rounding (as without a prior), all close to float64 autograd.
5. TENT / EATA steps under a prior against the contract restated in float64 (oracle._bn replaced by the blended BatchNorm).
6. bn_adapt: predictions, nothing changes, no backward / optimiser call, freeze + inference_mode, fit.test.
7. Properties: call sequences, synchronising calls, tta_bn_prior = 0.0 is tta_bn_prior = None.
tests/test_bnprior_cpu.py holds the float64 restatement (blended_bn, closed_form_backward) and checks it against autograd."""
import contextlib
import math
import os
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_gpu_ops import TOL  # noqa: E402
from test_bnprior_cpu import EPS, blended_bn, closed_form_backward  # noqa: E402
import test_gpu_tta as T  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402

SENT = -7.25
MS = (1, 49, 1000, 12544)
CS = (4, 64, 260, 2048)
RHOS = (0.0, 0.2, 1.0)
# + one shape past 256 row tiles: the statistics take the two-launch (stage 1 + final) path there
SHAPES = [(M, C) for M in MS for C in CS] + [(64 * 257 + 3, 64)]


def _p(t):
    return None if t is None else t.data_ptr()


def close(a, b, tol=TOL, name=""):
    """close() of tests/test_gpu_ops.py, |a - b| <= tol (1 + |b| + max|b|), evaluated where b lives (the float64 references of the
    wide shapes stay on the device)"""
    b = b.detach().double()
    a = a.detach().to(b.device).double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = float(b.abs().max()) if b.numel() else 0.0
    err = (a - b).abs()
    assert bool((err <= tol * (1.0 + b.abs() + scale)).all()), f"{name}: max err {float(err.max()):.3e} (scale {scale:.3e})"


def _buf(shape_rows, C):
    """[rows + 1, C] filled with the sentinel: the entry point writes the first `rows` rows only"""
    return torch.full((shape_rows + 1, C), SENT, device="cuda")


class _Case:
    """One layer's tensors.  y = A W^T has |mean| / std = 50 per channel (a constant input column); the source variance is within
    a factor 1.5 of the batch's and running_var[0] = 0.  The source mean sits 0.1 to 0.3 batch standard deviations (std = 0.28)
    off the batch mean.  Both ends come from channel 0, where rstd reaches 1 / sqrt(eps) = 316 (rho = 0, or M = 1):
    * delta = (mu - mean_batch) rstd inherits the fp32 rounding of the batch mean or of mu (half an ulp of 14 = 4.8e-7) times
      316 = 1.5e-4; close() allows 2e-5 (1 + 2 |delta|), so |delta| >= 3.3, i.e. an offset >= 0.04 std;
    * the coefficient form of dx holds rho k3 delta and rho k3 xhat_i apart, which cancel to rho k3 (x_i - mean_batch) rstd: four
      fp32 roundings of size eps rho delta^2 / 2 of max|dx|, inside close() while |delta| < 40, i.e. an
      offset <= 0.55 std at M = 1, rho = 0.2."""

    def __init__(self, ops, L, M, C):
        g = torch.Generator().manual_seed(1000 * M + C)
        K = 32
        A = torch.randn(M, K, generator=g)
        W = torch.randn(C, K, generator=g) * 0.05
        std = 0.05 * math.sqrt(K - 1)
        A[:, 0] = 1000.0
        W[:, 0] = 0.05 * std * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)   # mean = +-50 std
        self.M, self.C, self.L = M, C, L
        self.T = L.gemm_nt_tile_rows(M, C, 0)
        self.ts = torch.empty(2 * ((M + self.T - 1) // self.T), C, device="cuda")
        self.y = ops.gemm_nt(A.cuda(), W.cuda(), M, C, K, colstats=self.ts)
        y64 = self.y.double()
        mean_b = y64.mean(0)
        off = std * (0.1 + 0.2 * torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
        self.rm = (mean_b.cpu() + off.double()).float().cuda()
        rv = std * std * (0.5 + torch.rand(C, generator=g))
        rv[0] = 0.0
        self.rv = rv.cuda()
        self.gamma = (0.5 + torch.rand(C, generator=g)).cuda()
        self.beta = (0.2 * torch.randn(C, generator=g)).cuda()
        self.resid = torch.randn(M, C, generator=g).cuda()
        self.rstats = torch.stack([torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g), 0.5 + torch.rand(C, generator=g),
                                   0.1 * torch.randn(C, generator=g)]).contiguous().cuda()
        self.dz_ops = (torch.randn(M, 16, generator=g).cuda(), (torch.randn(C, 16, generator=g) * 0.25).cuda())   # dz = A2 W2^T
        self.dinit = torch.randn(2, C, generator=g).cuda()
        self.ops = ops

    # ---- device
    def fwd(self, path, rho, resid=None, rstats=None, relu=0, want_z=True, legacy=False):
        """-> (z [M+1, C] or None, stats [5, C], delta [C + 4]); legacy: the existing entry point with NULL running buffers"""
        L, M, C = self.L, self.M, self.C
        z = _buf(M, C) if want_z else None
        stats, delta = _buf(4, C), torch.full((C + 4,), SENT, device="cuda")
        if path == "tiles":
            nb = L.bn_tiles_workspace_bytes(M, C, self.T)
            ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")
            if legacy:
                L.bn_train_fwd_tiles(_p(self.y), _p(self.ts), self.T, _p(self.gamma), _p(self.beta), None, None, None, _p(resid), _p(rstats), _p(z),
                                     _p(stats), M, C, relu, EPS, 0.1, _p(ws), nb, None)
            else:
                L.bn_prior_fwd_tiles(_p(self.y), _p(self.ts), self.T, _p(self.gamma), _p(self.beta), _p(self.rm), _p(self.rv), rho, _p(resid),
                                     _p(rstats), _p(z), _p(stats), _p(delta), M, C, relu, EPS, _p(ws), nb, None)
        else:
            nb = L.bn_workspace_bytes(M, C)
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            if legacy:
                L.bn_train_fwd(_p(self.y), _p(self.gamma), _p(self.beta), None, None, None, _p(resid), _p(z), _p(stats), M, C, relu, EPS, 0.1,
                               _p(ws), nb, None)
            else:
                L.bn_prior_fwd(_p(self.y), _p(self.gamma), _p(self.beta), _p(self.rm), _p(self.rv), rho, _p(resid), _p(z), _p(stats), _p(delta),
                               M, C, relu, EPS, _p(ws), nb, None)
        torch.cuda.synchronize()
        return z, stats, delta

    def grad(self, stats, mode, zmask):
        """dz [M, C] as the input-gradient GEMM of the layer's consumer leaves it, with the BatchNorm-backward tile sums of its
        epilogue (stil_gemm_nt bstats; mode 2: mask recomputed from y and stats, mode 0: dz masked by zmask, or no ReLU)"""
        M, C = self.M, self.C
        nt = (M + 63) // 64
        part = torch.empty(2 * nt, C, device="cuda")
        assert self.L.gemm_nt_bstats_ok(None, C, C, None, C, _p(zmask), C, _p(self.y))
        dz = self.ops.gemm_nt(self.dz_ops[0], self.dz_ops[1], M, C, 16, relu_mask=zmask, bstats=(self.y, stats, part, mode, 0))
        return dz, part, nt

    def bwd(self, path, rho, stats, delta, dz, z, relu, part=None, nt=0, gout=False, accumulate=0, legacy=False, ws_offset=0):
        """-> (dx [M+1, C], gout [M+1, C] or None, dgamma [C + 4], dbeta [C + 4]); ws_offset (two-pass): bytes the workspace pointer is
        moved past its 16-byte aligned start (4: the scalar final instead of the float4 one)"""
        L, M, C = self.L, self.M, self.C
        dx, go = _buf(M, C), (_buf(M, C) if gout else None)
        dga, dbe = torch.full((C + 4,), SENT, device="cuda"), torch.full((C + 4,), SENT, device="cuda")
        if accumulate:
            dga[:C], dbe[:C] = self.dinit[0], self.dinit[1]
        coef = torch.empty(3, C, device="cuda")
        if path == "tiles":
            nb = L.bn_bwd_tiles_workspace_bytes(nt, C)
            ws = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
            if legacy:
                L.bn_train_bwd_tiles(_p(dz), _p(z), _p(self.y), _p(self.gamma), _p(stats), _p(part), nt, _p(dx), _p(dga), _p(dbe), _p(coef), M, C,
                                     relu, accumulate, _p(ws), nb, None)
            else:
                L.bn_prior_bwd_tiles(_p(dz), _p(z), _p(self.y), _p(self.gamma), _p(stats), _p(delta), rho, _p(part), nt, _p(dx), _p(dga), _p(dbe),
                                     _p(coef), M, C, relu, accumulate, _p(ws), nb, None)
        else:
            nb = L.bn_workspace_bytes(M, C)
            ws = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
            wp = ws.data_ptr() + ws_offset
            assert wp % 16 == ws_offset, "the allocator's alignment decides which final runs"
            if legacy:
                L.bn_train_bwd(_p(dz), _p(z), _p(self.y), _p(self.gamma), _p(stats), _p(dx), _p(go), _p(dga), _p(dbe), _p(coef), M, C, relu,
                               accumulate, wp, nb, None)
            else:
                L.bn_prior_bwd(_p(dz), _p(z), _p(self.y), _p(self.gamma), _p(stats), _p(delta), rho, _p(dx), _p(go), _p(dga), _p(dbe), _p(coef),
                               M, C, relu, accumulate, wp, nb, None)
        torch.cuda.synchronize()
        return dx, go, dga, dbe

    # ---- float64 (ATen on the device: the same restatement tests/test_bnprior_cpu.py checks against autograd)
    def ref_fwd(self, rho, resid=None, rstats=None, relu=0, mask=None):
        r = None
        if resid is not None:
            r = resid.double()
            if rstats is not None:
                rs = rstats.double()
                r = (r - rs[0]) * rs[2] + rs[3]
        return blended_bn(self.y.double(), self.gamma.double(), self.beta.double(), self.rm.double(), self.rv.double(), rho, r, bool(relu), mask)


def _check_fwd(c, got, ref, label, want_z=True):
    z, stats, delta = got
    zr, _, mu, r, dl = ref
    M, C = c.M, c.C
    assert bool((stats[4] == SENT).all()) and bool((delta[C:] == SENT).all()), label
    close(stats[0], mu, name=label + " mean")
    close(stats[1], r, name=label + " rstd")
    close(stats[2], c.gamma.double() * r, name=label + " a")
    assert torch.equal(stats[3], c.beta), label
    close(delta[:C], dl, name=label + " delta")
    if want_z:
        assert bool((z[M] == SENT).all()), label
        close(z[:M], zr, name=label + " z")


def _same(a, b, label):
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None) == (v is None) and (u is None or torch.equal(u, v)), f"{label}: output {i} differs"


@pytest.fixture(scope="module")
def ops():
    from stil_tta_amd import ops as o
    return o


@pytest.fixture(scope="module")
def cases(ops):
    from stil_tta_amd._lib import lib
    cache = {}

    def get(M, C):
        if (M, C) not in cache:
            cache.clear()           # one layer's tensors at a time (the widest is 100 MB per tensor)
            cache[(M, C)] = _Case(ops, lib(), M, C)
        return cache[(M, C)]
    return get


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("M,C", SHAPES)
def test_entry_points_against_float64(cases, M, C, rho):
    c = cases(M, C)
    paths = ("tiles", "two_pass") if C % 64 == 0 else ("tiles",)
    for path in paths:
        # ---------------- forward: no residual + ReLU, residual (raw shortcut, tiles only) + ReLU, residual without ReLU, statistics only
        variants = [("plain", None, None, 1), ("resid", c.resid, None, 0), ("resid_relu", c.resid, None, 1)]
        if path == "tiles":
            variants.append(("resid_stats", c.resid, c.rstats, 1))
        fw = {}
        for name, resid, rstats, relu in variants:
            got = c.fwd(path, rho, resid, rstats, relu)
            _same(got, c.fwd(path, rho, resid, rstats, relu), f"{path} {name} repetition")
            mask = (got[0][:M] > 0) if relu else None
            ref = c.ref_fwd(rho, resid, rstats, relu, mask)
            _check_fwd(c, got, ref, f"{path} {name}")
            fw[name] = (got, ref)
        if path == "tiles":
            got = c.fwd(path, rho, want_z=False)
            _check_fwd(c, got, fw["plain"][1], "tiles statistics only", want_z=False)
            assert torch.equal(got[1], fw["plain"][0][1]) and torch.equal(got[2], fw["plain"][0][2])
        # ---------------- backward
        (zp, stats, delta), (_, xhat, _, r, dl) = fw["plain"]
        zr = fw["resid_relu"][0][0]
        gam = c.gamma.double()
        # (label, relu mode of the call, z of the call, mask of the reference, bstats mode, mask of the GEMM epilogue)
        modes = [("relu2", 2, None, zp[:M] > 0, 2, None), ("relu1", 1, zr, zr[:M] > 0, 0, zr[:M]), ("relu0", 0, None, None, 0, None)]
        for label, relu, zc, mask, bmode, zmask in modes:
            dz, part, nt = c.grad(stats, bmode, zmask)
            if path == "two_pass" and zmask is not None:
                dz = c.ops.gemm_nt(c.dz_ops[0], c.dz_ops[1], M, C, 16)      # the two-pass entry masks the raw gradient itself
            g = dz.double() * mask if mask is not None else dz.double()
            dxr, dgr, dbr = closed_form_backward(g, xhat, gam, r, dl, rho)
            for acc in (0, 1):
                for gout in ((False, True) if path == "two_pass" else (False,)):
                    kw = dict(part=part, nt=nt, gout=gout, accumulate=acc)
                    got = c.bwd(path, rho, stats, delta, dz, zc, relu, **kw)
                    _same(got, c.bwd(path, rho, stats, delta, dz, zc, relu, **kw), f"{path} {label} backward repetition")
                    dx, go, dga, dbe = got
                    tag = f"{path} {label} acc={acc} gout={gout}"
                    assert bool((dx[M] == SENT).all()) and bool((dga[C:] == SENT).all()) and bool((dbe[C:] == SENT).all()), tag
                    close(dx[:M], dxr, name=tag + " dx")
                    close(dga[:C], dgr + (c.dinit[0].double() if acc else 0.0), name=tag + " dgamma")
                    close(dbe[:C], dbr + (c.dinit[1].double() if acc else 0.0), name=tag + " dbeta")
                    if gout:
                        assert bool((go[M] == SENT).all()) and torch.equal(go[:M].double(), g), tag + " gout"


@pytest.mark.parametrize("M,C", [(49, 64), (1000, 64)])
def test_scalar_backward_final_against_float64(cases, M, C):
    """A two-pass backward whose workspace is not 16-byte aligned finishes its sums with the scalar final (8 lanes) instead of the
    float4 one (32 lanes): stil_bn_train_bwd and stil_bn_prior_bwd (rho = 0.2), aligned and 4 bytes off, against the float64
    reference and bar of test_entry_points_against_float64.  The two finals add in different orders: not bit-equal to each other."""
    c = cases(M, C)
    gam = c.gamma.double()
    dz = c.ops.gemm_nt(c.dz_ops[0], c.dz_ops[1], M, C, 16)
    for legacy, rho in ((True, 1.0), (False, 0.2)):
        zp, stats, delta = c.fwd("two_pass", rho, None, None, 1, legacy=legacy)
        zr = c.fwd("two_pass", rho, c.resid, None, 1, legacy=legacy)[0]
        _, xhat, _, r, dl = c.ref_fwd(rho, None, None, 1, zp[:M] > 0)
        for relu, zc, mask in ((2, None, zp[:M] > 0), (1, zr, zr[:M] > 0)):
            dxr, dgr, dbr = closed_form_backward(dz.double() * mask, xhat, gam, r, dl, rho)
            for acc in (0, 1):
                for off in (0, 4):
                    dx, _, dga, dbe = c.bwd("two_pass", rho, stats, delta, dz, zc, relu, accumulate=acc, legacy=legacy, ws_offset=off)
                    tag = f"{'train' if legacy else 'prior'} relu={relu} acc={acc} workspace+{off}"
                    assert bool((dx[M] == SENT).all()) and bool((dga[C:] == SENT).all()) and bool((dbe[C:] == SENT).all()), tag
                    close(dx[:M], dxr, name=tag + " dx")
                    close(dga[:C], dgr + (c.dinit[0].double() if acc else 0.0), name=tag + " dgamma")
                    close(dbe[:C], dbr + (c.dinit[1].double() if acc else 0.0), name=tag + " dbeta")


@pytest.mark.parametrize("M,C", SHAPES)
def test_rho_one_is_the_existing_entry_points_bit_for_bit(cases, M, C):
    c = cases(M, C)
    for path in (("tiles", "two_pass") if C % 64 == 0 else ("tiles",)):
        variants = [(None, None, 1), (c.resid, None, 0), (c.resid, None, 1)] + ([(c.resid, c.rstats, 1)] if path == "tiles" else [])
        for resid, rstats, relu in variants:
            new, old = c.fwd(path, 1.0, resid, rstats, relu), c.fwd(path, 1.0, resid, rstats, relu, legacy=True)
            _same(new[:2], old[:2], f"{path} forward")
            assert bool((new[2][:C] == 0).all()) and bool((new[2][C:] == SENT).all())
        if path == "tiles":
            new, old = c.fwd(path, 1.0, want_z=False), c.fwd(path, 1.0, want_z=False, legacy=True)
            _same(new[:2], old[:2], "statistics only")
            assert bool((new[2][:C] == 0).all())
        zp, stats, delta = c.fwd(path, 1.0, None, None, 1)
        zr = c.fwd(path, 1.0, c.resid, None, 1)[0]
        for relu, zc, bmode, zmask in ((2, None, 2, None), (1, zr, 0, zr[:M]), (0, None, 0, None)):
            dz, part, nt = c.grad(stats, bmode, zmask)
            for acc in (0, 1):
                for gout in ((False, True) if path == "two_pass" else (False,)):
                    kw = dict(part=part, nt=nt, gout=gout, accumulate=acc)
                    _same(c.bwd(path, 1.0, stats, delta, dz, zc, relu, **kw), c.bwd(path, 1.0, stats, delta, dz, zc, relu, legacy=True, **kw),
                          f"{path} backward relu={relu} acc={acc} gout={gout}")


def test_bad_arguments_are_refused(cases):
    from stil_tta_amd._lib import lib
    L = lib()
    D = L._dll
    M, C = 49, 64
    c = cases(M, C)
    z, stats, delta = _buf(M, C), _buf(4, C), torch.zeros(C, device="cuda")
    dx, dga, dbe, coef = _buf(M, C), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(3, C, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    nbf, nbt, nbb = L.bn_workspace_bytes(M, C), L.bn_tiles_workspace_bytes(M, C, c.T), L.bn_bwd_tiles_workspace_bytes(1, C)
    y, ts, ga, be, rm, rv = (_p(t) for t in (c.y, c.ts, c.gamma, c.beta, c.rm, c.rv))

    def fwd(x=y, rmean=rm, rho=0.5, C_=C, nb=nbf, zz=_p(z)):
        return D.stil_bn_prior_fwd(x, ga, be, rmean, rv, rho, None, zz, _p(stats), _p(delta), M, C_, 1, EPS, _p(ws), nb, None)

    def fwd_t(x=y, rvar=rv, rho=0.5, C_=C, nb=nbt, zz=_p(z), resid=None, rst=None, dl=_p(delta)):
        return D.stil_bn_prior_fwd_tiles(x, ts, c.T, ga, be, rm, rvar, rho, resid, rst, zz, _p(stats), dl, M, C_, 1, EPS, _p(ws), nb, None)

    def bwd(dz=y, dl=_p(delta), rho=0.5, C_=C, nb=nbf, relu=2, zz=None):
        return D.stil_bn_prior_bwd(dz, zz, y, ga, _p(stats), dl, rho, _p(dx), None, _p(dga), _p(dbe), _p(coef), M, C_, relu, 0, _p(ws), nb, None)

    def bwd_t(dz=y, dl=_p(delta), rho=0.5, C_=C, nb=nbb, relu=2, zz=None, part=ts, nt=1):
        return D.stil_bn_prior_bwd_tiles(dz, zz, y, ga, _p(stats), dl, rho, part, nt, _p(dx), _p(dga), _p(dbe), _p(coef), M, C_, relu, 0, _p(ws),
                                         nb, None)

    for fn in (fwd, fwd_t, bwd, bwd_t):
        assert fn() == 0, (fn.__name__, L.last_error())           # control: the arguments are good
        for rho in (-0.1, 1.5, float("nan"), float("inf")):
            assert fn(rho=rho) != 0 and "rho" in L.last_error(), (fn.__name__, rho)
        assert fn(nb=8) != 0 and "workspace" in L.last_error(), fn.__name__
    assert fwd(x=None) != 0 and "null" in L.last_error() and fwd(rmean=None) != 0 and fwd(zz=None) != 0
    assert fwd_t(x=None) != 0 and "null" in L.last_error() and fwd_t(rvar=None) != 0 and fwd_t(dl=None) != 0
    assert fwd_t(zz=None, resid=_p(c.resid)) != 0 and fwd_t(rst=_p(c.rstats)) != 0     # residual without z; resid_stats without resid
    assert fwd_t(zz=None) == 0                                                          # statistics only
    assert bwd(dz=None) != 0 and "null" in L.last_error() and bwd(dl=None) != 0 and bwd(relu=1) != 0 and bwd(relu=3) != 0
    assert bwd_t(dz=None) != 0 and "null" in L.last_error() and bwd_t(dl=None) != 0 and bwd_t(part=None) != 0 and bwd_t(relu=1) != 0
    assert bwd_t(nt=0) != 0
    assert fwd(C_=4) != 0 and "64" in L.last_error() and bwd(C_=260) != 0 and "64" in L.last_error()   # the two-pass entries need C % 64 == 0
    assert fwd_t(C_=6) != 0 and bwd_t(C_=6) != 0                                                       # the tile entries C % 4 == 0
    torch.cuda.synchronize()
    assert bool((z[M] == SENT).all()) and bool((dx[M] == SENT).all())


# ------------------------------------------------------------------------------------------ block level
def _blocks_f64(blocks, x_nchw, rho, masks):
    """layer1 + layer2 in float64 (CPU autograd) with the blended BatchNorm, on the device's ReLU decisions (masks: id(bn.weight)
    -> bool NCHW).  -> (output, leaves in blocks' parameter order)"""
    leaves = {id(p): p.detach().cpu().double().requires_grad_() for blk in blocks for p in blk.parameters()}

    def bn(mod, x, relu, resid=None):
        Nb, Cc, H, W = x.shape
        rows = x.permute(0, 2, 3, 1).reshape(-1, Cc)
        rr = None if resid is None else resid.permute(0, 2, 3, 1).reshape(-1, Cc)
        mk = masks[id(mod.weight)].permute(0, 2, 3, 1).reshape(-1, Cc) if relu else None
        z = blended_bn(rows, leaves[id(mod.weight)], leaves[id(mod.bias)], mod.running_mean.cpu().double(), mod.running_var.cpu().double(),
                       rho, rr, relu, mk)[0]
        return z.view(Nb, H, W, Cc).permute(0, 3, 1, 2)

    h = x_nchw
    for blk in blocks:
        idn = h
        if blk.downsample is not None:
            idn = bn(blk.downsample[1], F.conv2d(h, leaves[id(blk.downsample[0].weight)], stride=blk.downsample[0].stride), False)
        convs = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2)] + ([(blk.conv3, blk.bn3)] if hasattr(blk, "conv3") else [])
        for i, (cv, b) in enumerate(convs):
            last = i == len(convs) - 1
            h = bn(b, F.conv2d(h, leaves[id(cv.weight)], stride=cv.stride, padding=cv.padding), True, idn if last else None)
    return h, [leaves[id(p)] for blk in blocks for p in blk.parameters()]


@pytest.mark.parametrize("arch", ["resnet50", "resnet18"])
def test_blocks_under_a_prior_production_path_equals_the_plain_path_and_float64(ops, arch):
    """layer1 + layer2 (identity and downsample shortcuts, the stride-2 stage boundary) at Nb = 4 under ops.bn_prior, as
    test_premasked_residual_gradient_and_deferred_bn_equal_the_plain_blocks runs them without one.  Deferred BatchNorm and
    premasked gradients against the plain blocks: output and every gradient bit for bit.  With the BatchNorm-backward sums of
    the GEMM epilogues on top (the production path) the forward is still bit-identical; the gradients are the same sums added in
    another order -- per-tile fp32 sums combined in double instead of the reduction pass -- so, as in that test for the parent,
    they agree to 2e-5 of each tensor's scale and not to the bit.  Every path is within close() of float64 autograd of the
    blended BatchNorm on the device's ReLU decisions."""
    import test_gpu_step as S
    from stil_tta_amd.modules import ResNet
    Nb, N = 4, 12.0
    rho = Nb / (N + Nb)
    res, masks, keep = [], None, None
    for fused, bstat, trace in ((True, True, False), (False, False, False), (True, False, False), (True, True, True)):
        ops._BN_DEFER, ops._PREMASK, ops._BN_BWD_EPILOGUE = fused, fused, bstat
        try:
            torch.manual_seed(5)
            net = ResNet(arch).cuda()
            blocks = list(net.layer1) + list(net.layer2)
            g = torch.Generator().manual_seed(9)
            for blk in blocks:
                for mod in blk.modules():
                    if isinstance(mod, torch.nn.BatchNorm2d):
                        mod.running_mean.copy_(0.3 * torch.randn(mod.num_features, generator=g))
                        mod.running_var.copy_(0.5 + torch.rand(mod.num_features, generator=g))
                        mod.weight.data.copy_(0.5 + torch.rand(mod.num_features, generator=g))
                        mod.bias.data.copy_(0.2 * torch.randn(mod.num_features, generator=g))
            bufs0 = [b.clone() for blk in blocks for b in blk.buffers()]
            x = torch.randn(Nb, 12, 12, 64, generator=torch.Generator().manual_seed(1)).cuda().requires_grad_()
            with (S._trace_decisions() if trace else contextlib.nullcontext()) as tr:
                h = x
                with ops.frozen_bn_stats(), ops.bn_prior(N, Nb):
                    for blk in blocks:
                        h = blk.run(h, True)
                gy = torch.randn(h.shape, generator=torch.Generator().manual_seed(2)).cuda()
                h.backward(gy)
                torch.cuda.synchronize()
                if trace:
                    masks = {pid: (z.detach() > 0).permute(0, 3, 1, 2).cpu() for pid, z in tr["relu"].items()}
                    keep = (blocks, x, gy)
            ps = [p for blk in blocks for p in blk.parameters()]
            for b0, b1 in zip(bufs0, [b for blk in blocks for b in blk.buffers()]):
                assert torch.equal(b0, b1), "a running buffer was written under frozen_bn_stats + bn_prior"
            res.append([h.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in ps])
        finally:
            ops._BN_DEFER, ops._PREMASK, ops._BN_BWD_EPILOGUE = True, True, True
    prod, plain, nosums, traced = res
    assert len(prod) == len(plain) > 20
    for i, (u, v) in enumerate(zip(nosums, plain)):
        assert torch.equal(u, v), f"tensor {i}: deferred / premasked blocks differ from the plain ones (max |d| = {float((u - v).abs().max()):.3e})"
    for i, (u, v) in enumerate(zip(prod, traced)):
        assert torch.equal(u, v), f"tensor {i}: tracing the decisions changed the production path"
    assert torch.equal(prod[0], plain[0])
    worst = 0.0
    for i, (u, v) in enumerate(zip(prod[1:], plain[1:])):
        d = float((u - v).abs().max()) / (1e-30 + float(v.abs().max()))
        worst = max(worst, d)
        assert d <= 2e-5, f"gradient {i}: production path differs from the plain one by {d:.2e} of the tensor's scale"
    print(f"[{arch}] production vs plain gradients under a prior: worst |d| / max|g| = {worst:.2e}")
    blocks, x, gy = keep
    xin = x.detach().cpu().double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    out, leaves = _blocks_f64(blocks, xin, rho, masks)
    grads = torch.autograd.grad(out, [xin] + leaves, gy.cpu().double().permute(0, 3, 1, 2))
    for r in (prod, plain):
        close(r[0].permute(0, 3, 1, 2), out, name="blocks output")
        close(r[1].permute(0, 3, 1, 2), grads[0], name="blocks dx")
        for i, (u, v) in enumerate(zip(r[2:], grads[1:])):
            close(u, v, name=f"blocks parameter gradient {i}")


# ------------------------------------------------------------------------------------------ the steps, restated in float64
@contextlib.contextmanager
def blended_oracle(N, B):
    """oracle.stil_oracle._bn <- the blended BatchNorm at rho = B / (N + B) (N None: the batch statistics alone); no buffer written"""
    rho = 1.0 if N is None else B / (N + B)

    def bn(sd, name, x, train):
        assert train
        mu_b = x.mean((0, 2, 3))
        v_b = ((x - mu_b[None, :, None, None]) ** 2).mean((0, 2, 3))
        mu = (1 - rho) * sd[name + ".running_mean"] + rho * mu_b
        v = (1 - rho) * sd[name + ".running_var"] + rho * v_b
        xhat = (x - mu[None, :, None, None]) / torch.sqrt(v + 1e-5)[None, :, None, None]
        return xhat * sd[name + ".weight"][None, :, None, None] + sd[name + ".bias"][None, :, None, None]

    orig, O._bn = O._bn, bn
    try:
        yield
    finally:
        O._bn = orig


# (label, hparams, B, tta_params, batch seeds, state seed, N)
STEP = [
    ("dvm_b64_bn_online_n16", lambda: T.dvm_hp(64), 64, "bn", (201, 202), 11, 16.0),
    ("dvm_b8_norm_n64", lambda: T.dvm_hp(8), 8, "norm", (301,), 21, 64.0),
    ("cardiac_b32_bn_n16", lambda: T.cardiac_hp(32), 32, "bn", (401,), 31, 16.0),
]


@pytest.mark.parametrize("case", STEP, ids=[c[0] for c in STEP])
def test_tent_step_under_a_prior_matches_the_contract_restated_in_float64(case):
    """TENT's own bars (tests/test_gpu_tta.py): predictions 3e-5 scaled, every gradient of A at 3 e32 + 1e-4, Adam within
    2.2 lr step, everything outside A (running buffers included) bit-identical."""
    import test_gpu_step as S
    label, mk_hp, B, which, seeds, sseed, N = case
    hp = mk_hp()
    lr = 1e-3
    sd = T.initial_state(hp, sseed)
    m = T.make_model(hp, sd, tta=True, tta_method="tent", tta_params=which, tta_lr=lr, tta_bn_prior=N)
    m.freeze()
    keys = T.adapted_keys(m)
    opt, bad = {}, []
    for step, seed in enumerate(seeds, start=1):
        x, y = T.tta_batch(hp, B, seed)
        before = T.full_state(m)
        sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
        with S._trace_decisions() as trace:
            m.test_step(T.to_dev((x, y)), step - 1)
            torch.cuda.synchronize()
            decisions = S._device_decisions(m, trace)
        probs = m.last_tta["probs"].cpu().double()
        with blended_oracle(N, B):
            p64, g64, flips = T.tent_restated(sd_before, keys, x, hp, torch.float64, decisions)
            _, g64free, _ = T.tent_restated(sd_before, keys, x, hp, torch.float64)
            p32, g32, _ = T.tent_restated(sd_before, keys, x, hp, torch.float32)
        S._check_flips(flips)
        d = S._scaled(probs.numpy(), p64.numpy())
        print(f"[{label}] batch {step}: predictions scaled error {d:.2e} (fp32 restatement {S._scaled(p32.double().numpy(), p64.numpy()):.2e})")
        if d > 3e-5:
            bad.append((step, "predictions", d))
        gd = T.device_grads(m)
        ratios = []
        for k in keys:
            e32, err = T._rel(g32[k].double(), g64free[k]), T._rel(gd[k], g64[k])
            ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
            if err > 3 * e32 + 1e-4:
                bad.append((step, "grad " + k, err, e32))
        print(f"[{label}] batch {step}: gradient error / (3*e32 + 1e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
        sd32 = {k: v.clone() for k, v in sd_before.items()}
        O.adam_step(sd32, g32, opt, step, lr)
        after = T.full_state(m)
        aset = set(keys)
        for k, v in after.items():
            if k in aset:
                dev = float((v.cpu() - sd32[k]).abs().max())
                if dev > 2.2 * lr * step:
                    bad.append((step, "adam " + k, dev))
            elif not torch.equal(v, before[k]):
                bad.append((step, "changed " + k))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


def test_eata_step_under_a_prior_matches_the_contract_restated_in_float64():
    """One EATA batch (no running mean of predictions yet, no Fisher estimate) with N = 16, margins from the float64 pre-pass as in
    tests/test_gpu_eata.py; TENT's bars, and the selection equals the float64 one on every row."""
    import test_gpu_eata as E
    import test_gpu_step as S
    B, N, lr = 64, 16.0, 1e-3
    hp = T.dvm_hp(B)
    sd = E.scaled_state(hp, 11)
    m = T.make_model(hp, sd, tta=True, tta_method="eata", tta_params="bn", tta_lr=lr, tta_probs_momentum=E.MU, tta_bn_prior=N)
    m.freeze()
    keys = T.adapted_keys(m)
    x, y = T.tta_batch(hp, B, 201)
    sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
    m_in = torch.zeros(hp.num_classes)
    with blended_oracle(N, B):
        pre = E.eata_restated(sd_before, keys, x, hp, torch.float64, m_in, 0, E.MU)
    e0, dm = pre["margins"]
    m.hp.tta_e_margin, m.hp.tta_d_margin = e0, dm
    before = T.full_state(m)
    with S._trace_decisions() as trace:
        m.test_step(T.to_dev((x, y)), 0)
        torch.cuda.synchronize()
        decisions = S._device_decisions(m, trace)
    with blended_oracle(N, B):
        r64 = E.eata_restated(sd_before, keys, x, hp, torch.float64, m_in, 0, E.MU, margins=(e0, dm), decisions=decisions)
        r64free = E.eata_restated(sd_before, keys, x, hp, torch.float64, m_in, 0, E.MU, margins=(e0, dm))
        r32 = E.eata_restated(sd_before, keys, x, hp, torch.float32, m_in, 0, E.MU, margins=(e0, dm))
    S._check_flips(r64["flips"])
    eH = float((r32["H"].double() - r64free["H"]).abs().max())
    frac = pre["n"] / B
    print(f"E0 {e0:.4f} (half gap {pre['gaps']['H']:.2e}, fp32 restatement error on H {eH:.2e}), selected {pre['n']}/{B}")
    assert pre["gaps"]["H"] >= 100 * eH and 0.25 <= frac <= 0.75, "the margin is badly placed for this batch"
    lt = m.last_tta
    bad = []
    d = S._scaled(lt["probs"].cpu().double().numpy(), r64["p"].numpy())
    print(f"predictions scaled error {d:.2e}")
    if d > 3e-5:
        bad.append(("predictions", d))
    assert torch.equal(lt["selected"].cpu().bool(), r64["sel"]) and torch.equal(lt["reliable"].cpu().bool(), r64["rel"])
    assert int(lt["n_selected"]) == r64["n"]
    close(lt["loss_entropy"].view(1), r64["l_ent"].view(1), name="loss_entropy")
    gd = T.device_grads(m)
    ratios = []
    for k in keys:
        e32, err = T._rel(r32["g"][k].double(), r64free["g"][k]), T._rel(gd[k], r64["g"][k])
        ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
        if err > 3 * e32 + 1e-4:
            bad.append(("grad " + k, err, e32))
    print(f"gradient error / (3*e32 + 1e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
    sd32 = {k: v.clone() for k, v in sd_before.items()}
    O.adam_step(sd32, r32["g"], {}, 1, lr)
    aset = set(keys)
    for k, v in T.full_state(m).items():
        if k in aset:
            dev = float((v.cpu() - sd32[k]).abs().max())
            if dev > 2.2 * lr:
                bad.append(("adam " + k, dev))
        elif not torch.equal(v, before[k]):
            bad.append(("changed " + k,))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


# ------------------------------------------------------------------------------------------ bn_adapt
_BN_FWD = ("bn_train_fwd", "bn_train_fwd_tiles", "bn_prior_fwd", "bn_prior_fwd_tiles")
_BN_CALLS = ("bn_train_bwd", "bn_train_bwd_tiles", "bn_prior_bwd", "bn_prior_bwd_tiles", "wgrad_tn", "wgrad_tn_partial", "adam_step")


def _record(monkeypatch, names):
    """record the names of the C-ABI calls among `names`"""
    from stil_tta_amd._lib import lib
    L = lib()
    calls = []
    for name in names:
        orig = getattr(L, name)
        monkeypatch.setitem(L.__dict__, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    return calls


@pytest.mark.parametrize("label,B,N", [("batch_statistics", 32, None), ("n16", 32, 16.0), ("one_image_n16", 1, 16.0)])
def test_bn_adapt_predictions_against_float64_and_nothing_changes(label, B, N, monkeypatch):
    import test_gpu_step as S
    hp = T.dvm_hp(B)
    sd = T.initial_state(hp, 11)
    m = T.make_model(hp, sd, tta=True, tta_method="bn_adapt", tta_bn_prior=N, tta_episodic=True)
    calls = _record(monkeypatch, _BN_CALLS)
    x, y = T.tta_batch(hp, B, 201)
    before = T.full_state(m)
    with S._trace_decisions() as trace:
        p = m.test_step(T.to_dev((x, y)), 0)
        torch.cuda.synchronize()
        decisions = S._device_decisions(m, trace)
    m.reset_tta()
    assert calls == [], calls
    assert m._tent is None and set(m.last_tta) == {"y_hat_m", "probs"} and torch.equal(p, m.last_tta["probs"])
    after = T.full_state(m)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert bool(torch.isfinite(p).all())
    keys = T.adapted_keys(m)[:2]
    with blended_oracle(N, B):
        p64, _, flips = T.tent_restated(sd, keys, x, hp, torch.float64, decisions)
        p32, _, _ = T.tent_restated(sd, keys, x, hp, torch.float32)
    S._check_flips(flips)
    d = S._scaled(p.cpu().double().numpy(), p64.numpy())
    print(f"[{label}] predictions scaled error {d:.2e} (fp32 restatement {S._scaled(p32.double().numpy(), p64.numpy()):.2e})")
    assert d <= 3e-5
    close(torch.softmax(m.last_tta["y_hat_m"].double(), 1), p, name="probs is softmax(y_hat_m)")


def _small(method="tent", **tta):
    hp = T.dvm_hp(16, img_size=64)
    sd = T.initial_state(hp, 5)
    return hp, sd, (lambda: T.make_model(hp, sd, tta=True, tta_method=method, **tta))


def test_bn_adapt_freeze_inference_mode_and_fit_test(tmp_path):
    from stil_tta_amd import fit
    hp, sd, mk = _small("bn_adapt", tta_bn_prior=16.0)
    b = T.to_dev(T.tta_batch(hp, 16, 14))
    a, c = mk(), mk()
    a.freeze()
    with torch.inference_mode():
        pa = a.test_step(b, 0)
    pc = c.test_step(b, 0)
    assert torch.equal(pa, pc)
    off = T.make_model(hp, sd, tta=True)
    assert not torch.equal(off.test_step(b, 0), pc), "bn_adapt scores equal the eval-mode ones"
    sa, sc = T.full_state(a), T.full_state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert not any(q.requires_grad for q in a.parameters())
    # fit.test with a checkpoint: the scores of the loop below, short last batch included
    loader = [T.tta_batch(hp, 16, 20), T.tta_batch(hp, 16, 21), T.tta_batch(hp, 5, 22)]
    ck = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": {k: v.clone() for k, v in sd.items()}}, ck)
    f = mk()
    f.load_state_dict({k: v.cuda() for k, v in T.initial_state(hp, 77).items()})
    rf = fit.test(f, loader, ck)
    h = mk()
    h.freeze()
    h.acc_test.reset()
    h.auc_test.reset()
    for i, bt in enumerate(loader):
        h.test_step(T.to_dev(bt), i)
    rh = {k: float(v) for k, v in h.test_epoch_end().items()}
    assert rf.keys() == rh.keys() and all(rf[k] == rh[k] or (rf[k] != rf[k] and rh[k] != rh[k]) for k in rf), (rf, rh)
    sf, sh = T.full_state(f), T.full_state(h)
    for k in sf:
        assert torch.equal(sf[k], sh[k]), k
    ro = fit.test(T.make_model(hp, sd, tta=True), loader, ck)
    assert ro.keys() == rf.keys()


# ------------------------------------------------------------------------------------------ properties
def test_call_sequences_with_and_without_a_prior(monkeypatch):
    hp, sd, mk = _small()
    mp = _small(tta_bn_prior=16.0)[2]
    b = T.to_dev(T.tta_batch(hp, 16, 7))
    calls = _record(monkeypatch, _BN_FWD + _BN_CALLS)
    mk().test_step(b, 0)
    torch.cuda.synchronize()
    plain = list(calls)
    calls.clear()
    mp().test_step(b, 0)
    torch.cuda.synchronize()
    prior = list(calls)
    # no prior: the parent's sequence -- one BatchNorm forward per layer, their backwards, one Adam launch; no weight-gradient product
    assert not any(n.startswith("bn_prior_") or n.startswith("wgrad") for n in plain)
    nf, nbw = sum(n.startswith("bn_train_fwd") for n in plain), sum(n.startswith("bn_train_bwd") for n in plain)
    assert nf == nbw == 53 and plain.count("adam_step") >= 1
    assert all(n.startswith("bn_train_fwd") for n in plain[:nf]) and all(n.startswith("bn_train_bwd") for n in plain[nf:nf + nbw])
    # with a prior: the same sequence with every BatchNorm call replaced by its prior counterpart, none of the old ones left
    assert prior == [n.replace("bn_train_", "bn_prior_") for n in plain]


def test_prior_step_synchronises_no_more_than_a_tent_step():
    hp, sd, mk = _small()
    mp = _small(tta_bn_prior=16.0)[2]
    ma = _small("bn_adapt", tta_bn_prior=16.0)[2]
    batches = [T.to_dev(T.tta_batch(hp, 16, 30 + i)) for i in range(3)]
    t, p, a = mk(), mp(), ma()
    for mm in (t, p, a):
        mm.test_step(batches[0], 0)

    def count(mm):
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                for i, bt in enumerate(batches[1:]):
                    mm.test_step(bt, i + 1)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        return [str(w.message) for w in rec if "synchroniz" in str(w.message).lower()]

    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:      # control: the counter sees a device -> host read
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            float(t.last_tta["loss"])
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert any("synchroniz" in str(w.message).lower() for w in rec), "the sync counter sees nothing"
    wt, wp, wa = count(t), count(p), count(a)
    print(f"synchronising calls over two steps: tent {len(wt)}, tent + prior {len(wp)}, bn_adapt + prior {len(wa)}")
    assert len(wp) <= len(wt) and len(wa) <= len(wt), (wt, wp, wa)


def test_prior_zero_is_no_prior_bit_for_bit():
    hp, sd, mk = _small()
    mz = _small(tta_bn_prior=0.0)[2]
    a, z = mk(), mz()
    for i, seed in enumerate((11, 12)):
        b = T.to_dev(T.tta_batch(hp, 16, seed))
        pa, pz = a.test_step(b, i), z.test_step(b, i)
        torch.cuda.synchronize()
        assert torch.equal(pa, pz), f"batch {i}: predictions"
        ga, gz = T.device_grads(a), T.device_grads(z)
        for k in ga:
            assert torch.equal(ga[k], gz[k]), f"batch {i}: gradient {k}"
        sa, sz = T.full_state(a), T.full_state(z)
        for k in sa:
            assert torch.equal(sa[k], sz[k]), f"batch {i}: {k}"
    assert any(not torch.equal(sa[k], v.cuda()) for k, v in sd.items() if k in set(T.adapted_keys(a))), "nothing was adapted"
