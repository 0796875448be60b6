"""Test-time BatchNorm on a running estimate of the target statistics (RoTTA's robust BatchNorm, Yuan et al., CVPR 2023; DUA, Mirza
et al., CVPR 2022): csrc/stil_bnmemory.h, ops.bn_memory, tta.BnMemory, tta_bn_momentum and tta_method "dua".

1. The two entry points against float64 (close() at 2e-5, the bar of tests/test_gpu_bnprior.py): z, stats, delta, m', s'; two-pass
   and tile paths, residual / resid_stats / z == NULL, both variance rules (M = 1 with unbiased = 1 included), sentinels, repetition,
   the memory read bit-unchanged.  The ReLU mask of the reference is the device's z.
2. NULL outputs are stil_bn_prior_fwd(_tiles) bit for bit; rho = 1 gives stil_bn_train_fwd(_tiles)'s z / stats, delta = 0, and still
   updates the memory.
3. Bad arguments are refused with nothing written.
4. tent / sar / bn_adapt / dua steps against the contract restated in float64 on the oracle (oracle._bn replaced by the memory
   BatchNorm), TENT's bars; the memory after every step against the float64 update at close().
5. State rules and properties: reset, episodic, load_state_dict, freeze + inference_mode, fit.test with a ragged last batch,
   synchronising calls, no backward in dua, and every new key at its default leaves the call sequence of tent / bn_adapt alone.
tests/test_bnmemory_cpu.py holds the float64 restatement's own checks and shows the bar of 1. reachable in fp32 on these inputs."""
import contextlib
import os
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from bnmemory_cases import RHO_ALPHA, SHAPES, layer_inputs, memory_bn, momentum  # noqa: E402
from test_bnprior_cpu import EPS  # noqa: E402
import test_gpu_bnprior as P  # noqa: E402
import test_gpu_tta as T  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402

SENT = P.SENT
close, _p, _buf, _same = P.close, P._p, P._buf, P._same


class _Layer:
    """One layer's tensors on the device (bnmemory_cases.layer_inputs; y through the project's GEMM, whose epilogue leaves the tile
    statistics) and the calls."""

    def __init__(self, ops, L, M, C):
        c = layer_inputs(M, C)
        self.M, self.C, self.L = M, C, L
        self.T = L.gemm_nt_tile_rows(M, C, 0)
        self.ts = torch.empty(2 * ((M + self.T - 1) // self.T), C, device="cuda")
        self.y = ops.gemm_nt(c["A"].cuda(), c["W"].cuda(), M, C, c["K"], colstats=self.ts)
        self.rm, self.rv, self.gamma, self.beta, self.resid, self.rstats = (c[k].cuda() for k in ("rm", "rv", "gamma", "beta", "resid", "rstats"))
        self.rm0, self.rv0 = self.rm.clone(), self.rv.clone()

    def fwd(self, path, rho, alpha=0.5, unbiased=0, resid=None, rstats=None, relu=0, want_z=True, update=True, which="memory"):
        """-> (z [M+1, C] or None, stats [5, C], delta [C + 4], m' [C + 4], s' [C + 4]); which: "memory", or "prior" / "train": the
        existing entry points on the same arguments (train: NULL running buffers)"""
        L, M, C = self.L, self.M, self.C
        z = _buf(M, C) if want_z else None
        stats, delta = _buf(4, C), torch.full((C + 4,), SENT, device="cuda")
        mo, vo = torch.full((C + 4,), SENT, device="cuda"), torch.full((C + 4,), SENT, device="cuda")
        o1, o2 = (_p(mo), _p(vo)) if update else (None, None)
        if path == "tiles":
            nb = L.bn_tiles_workspace_bytes(M, C, self.T)
            ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")
            if which == "memory":
                L.bn_memory_fwd_tiles(_p(self.y), _p(self.ts), self.T, _p(self.gamma), _p(self.beta), _p(self.rm), _p(self.rv), o1, o2, alpha,
                                      unbiased, rho, _p(resid), _p(rstats), _p(z), _p(stats), _p(delta), M, C, relu, EPS, _p(ws), nb, None)
            elif which == "prior":
                L.bn_prior_fwd_tiles(_p(self.y), _p(self.ts), self.T, _p(self.gamma), _p(self.beta), _p(self.rm), _p(self.rv), rho, _p(resid),
                                     _p(rstats), _p(z), _p(stats), _p(delta), M, C, relu, EPS, _p(ws), nb, None)
            else:
                L.bn_train_fwd_tiles(_p(self.y), _p(self.ts), self.T, _p(self.gamma), _p(self.beta), None, None, None, _p(resid), _p(rstats), _p(z),
                                     _p(stats), M, C, relu, EPS, 0.1, _p(ws), nb, None)
        else:
            nb = L.bn_workspace_bytes(M, C)
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            if which == "memory":
                L.bn_memory_fwd(_p(self.y), _p(self.gamma), _p(self.beta), _p(self.rm), _p(self.rv), o1, o2, alpha, unbiased, rho, _p(resid),
                                _p(z), _p(stats), _p(delta), M, C, relu, EPS, _p(ws), nb, None)
            elif which == "prior":
                L.bn_prior_fwd(_p(self.y), _p(self.gamma), _p(self.beta), _p(self.rm), _p(self.rv), rho, _p(resid), _p(z), _p(stats), _p(delta),
                               M, C, relu, EPS, _p(ws), nb, None)
            else:
                L.bn_train_fwd(_p(self.y), _p(self.gamma), _p(self.beta), None, None, None, _p(resid), _p(z), _p(stats), M, C, relu, EPS, 0.1,
                               _p(ws), nb, None)
        torch.cuda.synchronize()
        assert torch.equal(self.rm, self.rm0) and torch.equal(self.rv, self.rv0), "the memory read was written"
        return z, stats, delta, mo, vo

    def ref(self, rho, alpha, unbiased, resid=None, rstats=None, relu=0, mask=None):
        r = None
        if resid is not None:
            r = resid.double()
            if rstats is not None:
                rs = rstats.double()
                r = (r - rs[0]) * rs[2] + rs[3]
        return memory_bn(self.y.double(), self.gamma.double(), self.beta.double(), self.rm.double(), self.rv.double(), rho, alpha, unbiased,
                         r, bool(relu), mask)


def _check(c, got, ref, label, want_z=True, updated=True):
    P._check_fwd(c, got[:3], ref[:5], label, want_z)
    mo, vo = got[3], got[4]
    C = c.C
    assert bool((mo[C:] == SENT).all()) and bool((vo[C:] == SENT).all()), label
    if updated:
        assert bool(torch.isfinite(mo[:C]).all()) and bool(torch.isfinite(vo[:C]).all()), label
        close(mo[:C], ref[5], name=label + " m'")
        close(vo[:C], ref[6], name=label + " s'")
    else:
        assert bool((mo == SENT).all()) and bool((vo == SENT).all()), label


@pytest.fixture(scope="module")
def layers():
    from stil_tta_amd import ops
    from stil_tta_amd._lib import lib
    cache = {}

    def get(M, C):
        if (M, C) not in cache:
            cache.clear()           # one layer's tensors at a time
            cache[(M, C)] = _Layer(ops, lib(), M, C)
        return cache[(M, C)]
    return get


def _paths(C):
    return ("tiles", "two_pass") if C % 64 == 0 else ("tiles",)


@pytest.mark.parametrize("M,C", SHAPES)
def test_entry_points_against_float64(layers, M, C):
    c = layers(M, C)
    for path in _paths(C):
        for rho, alpha in RHO_ALPHA:
            variants = [("plain", None, None, 1), ("resid_relu", c.resid, None, 1)]
            if path == "tiles":
                variants.append(("resid_stats", c.resid, c.rstats, 1))
            for name, resid, rstats, relu in variants:
                for unbiased in ((0, 1) if name == "plain" else (0,)):
                    label = f"{path} {name} rho={rho} alpha={alpha} unbiased={unbiased}"
                    got = c.fwd(path, rho, alpha, unbiased, resid, rstats, relu)
                    _same(got, c.fwd(path, rho, alpha, unbiased, resid, rstats, relu), label + " repetition")
                    _check(c, got, c.ref(rho, alpha, unbiased, resid, rstats, relu, got[0][:M] > 0), label)
                    if name == "plain" and unbiased == 0:
                        plain = got
            if path == "tiles":   # statistics only: the same statistics, delta and memory, no z
                got = c.fwd(path, rho, alpha, 0, want_z=False)
                _same(got[1:], plain[1:], f"{path} statistics only rho={rho}")


@pytest.mark.parametrize("M,C", SHAPES)
def test_null_outputs_are_the_prior_entry_points_bit_for_bit(layers, M, C):
    c = layers(M, C)
    for path in _paths(C):
        for rho in (0.0, 0.05, 1.0):
            variants = [(None, None, 1, True), (c.resid, None, 0, True)] + ([(c.resid, c.rstats, 1, True), (None, None, 0, False)] if path == "tiles" else [])
            for resid, rstats, relu, want_z in variants:
                new = c.fwd(path, rho, 0.3, 1, resid, rstats, relu, want_z, update=False)
                old = c.fwd(path, rho, 0.3, 1, resid, rstats, relu, want_z, which="prior")
                _same(new[:3], old[:3], f"{path} rho={rho}")
                assert bool((new[3] == SENT).all()) and bool((new[4] == SENT).all())


@pytest.mark.parametrize("M,C", SHAPES)
def test_rho_one_is_the_training_entry_points_bit_for_bit_and_still_updates(layers, M, C):
    c = layers(M, C)
    for path in _paths(C):
        variants = [(None, None, 1, True), (c.resid, None, 1, True)] + ([(c.resid, c.rstats, 1, True), (None, None, 0, False)] if path == "tiles" else [])
        for resid, rstats, relu, want_z in variants:
            for unbiased in (0, 1):
                new = c.fwd(path, 1.0, 0.1, unbiased, resid, rstats, relu, want_z)
                old = c.fwd(path, 1.0, 0.1, unbiased, resid, rstats, relu, want_z, which="train")
                _same(new[:2], old[:2], f"{path} rho=1 forward")
                assert bool((new[2][:C] == 0).all()) and bool((new[2][C:] == SENT).all())
                ref = c.ref(1.0, 0.1, unbiased)
                assert bool((new[3][C:] == SENT).all()) and bool((new[4][C:] == SENT).all())
                close(new[3][:C], ref[5], name=f"{path} rho=1 m'")
                close(new[4][:C], ref[6], name=f"{path} rho=1 s'")


def test_bad_arguments_are_refused_with_nothing_written(layers):
    from stil_tta_amd._lib import lib
    L = lib()
    D = L._dll
    M, C = 49, 64
    c = layers(M, C)
    z, stats, delta = _buf(M, C), _buf(4, C), torch.full((C,), SENT, device="cuda")
    mo, vo = torch.full((2 * C,), SENT, device="cuda"), torch.full((2 * C,), SENT, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    nbf, nbt = L.bn_workspace_bytes(M, C), L.bn_tiles_workspace_bytes(M, C, c.T)
    y, ts, ga, be, rm, rv = (_p(t) for t in (c.y, c.ts, c.gamma, c.beta, c.rm, c.rv))
    both = torch.cat([c.rm, c.rv])          # one allocation: [mean | var], to alias against

    def fwd(x=y, m=rm, v=rv, o1=_p(mo), o2=_p(vo), alpha=0.5, unb=0, rho=0.5, C_=C, nb=nbf, zz=_p(z)):
        return D.stil_bn_memory_fwd(x, ga, be, m, v, o1, o2, alpha, unb, rho, None, zz, _p(stats), _p(delta), M, C_, 1, EPS, _p(ws), nb, None)

    def fwd_t(x=y, m=rm, v=rv, o1=_p(mo), o2=_p(vo), alpha=0.5, unb=0, rho=0.5, C_=C, nb=nbt, zz=_p(z), resid=None, rst=None):
        return D.stil_bn_memory_fwd_tiles(x, ts, c.T, ga, be, m, v, o1, o2, alpha, unb, rho, resid, rst, zz, _p(stats), _p(delta), M, C_, 1, EPS,
                                          _p(ws), nb, None)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == SENT).all()) for t in (z, stats, delta, mo, vo))

    for fn in (fwd, fwd_t):
        for alpha in (-0.1, 1.5, float("nan"), float("inf")):
            assert fn(alpha=alpha) != 0 and "alpha" in L.last_error(), (fn.__name__, alpha)
            assert fn(alpha=alpha, o1=None, o2=None) != 0 and "alpha" in L.last_error()
        for rho in (-0.1, 1.5, float("nan"), float("inf")):
            assert fn(rho=rho) != 0 and "rho" in L.last_error(), (fn.__name__, rho)
        assert fn(unb=2) != 0 and "unbiased" in L.last_error()
        assert fn(o1=None) != 0 and "without the other" in L.last_error() and fn(o2=None) != 0 and "without the other" in L.last_error()
        bm, bv = _p(both), _p(both) + 4 * C
        for kw in (dict(o1=rm), dict(o2=rv), dict(o1=rv), dict(o2=rm), dict(o2=_p(mo)), dict(o1=_p(mo), o2=_p(mo) + 4 * (C - 1)),
                   dict(m=bm, v=bv, o1=bm + 4 * (C - 1), o2=_p(vo)), dict(m=bm, v=bv, o1=_p(mo), o2=bv - 4)):
            assert fn(**kw) != 0 and "alias" in L.last_error(), (fn.__name__, kw)
        assert fn(x=None) != 0 and "null" in L.last_error() and fn(m=None) != 0 and fn(v=None) != 0
        assert fn(nb=8) != 0 and "workspace" in L.last_error()
        assert untouched(), fn.__name__
    assert fwd(zz=None) != 0 and fwd(C_=4) != 0 and "64" in L.last_error()
    assert fwd_t(C_=6) != 0 and fwd_t(zz=None, resid=_p(c.resid)) != 0 and fwd_t(rst=_p(c.rstats)) != 0
    assert untouched()
    assert fwd() == 0 and fwd_t() == 0 and fwd_t(zz=None) == 0, L.last_error()        # control: the arguments are good
    torch.cuda.synchronize()
    assert bool((mo[:C] != SENT).all()) and bool((mo[C:] == SENT).all()) and bool((vo[C:] == SENT).all()) and bool((z[M] == SENT).all())


# ------------------------------------------------------------------------------------------ the steps, restated in float64
def _bn_names(m):
    return ["model.encoder_imaging." + n for n, mod in m.model.encoder_imaging.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)]


def memory_of(m, sd):
    """{oracle name of a BatchNorm layer: (mean, var)} (float64, CPU) of the estimate the next batch reads: the device's memory, or
    the running buffers of the state `sd` while none exists"""
    names = _bn_names(m)
    if m._bn_mem is None:
        return {n: (sd[n + ".running_mean"].cpu().double(), sd[n + ".running_var"].cpu().double()) for n in names}
    return {n: (a.cpu().double(), b.cpu().double()) for n, (a, b) in zip(names, m._bn_mem.state())}


@contextlib.contextmanager
def memory_oracle(mem, rho, alpha, unbiased=False, record=None):
    """oracle.stil_oracle._bn <- the BatchNorm of csrc/stil_bnmemory.h on the memory `mem`; record (a dict): <- {name: (m', s')}.
    No buffer of the state is read or written."""
    def bn(sd, name, x, train):
        assert train
        m_, s_ = (t.to(x.dtype) for t in mem[name])
        mu_b = x.mean((0, 2, 3))
        v_b = ((x - mu_b[None, :, None, None]) ** 2).mean((0, 2, 3))
        mu = (1 - rho) * m_ + rho * mu_b
        v = (1 - rho) * s_ + rho * v_b
        if record is not None:
            M = x.numel() // x.shape[1]
            c = M / (M - 1) if (unbiased and M > 1) else 1.0
            record[name] = (((1 - alpha) * m_ + alpha * mu_b).detach(), ((1 - alpha) * s_ + alpha * c * v_b).detach())
        xhat = (x - mu[None, :, None, None]) / torch.sqrt(v + 1e-5)[None, :, None, None]
        return xhat * sd[name + ".weight"][None, :, None, None] + sd[name + ".bias"][None, :, None, None]

    orig, O._bn = O._bn, bn
    try:
        yield
    finally:
        O._bn = orig


def _check_memory(m, record, label):
    got = memory_of(m, None)
    assert set(got) == set(record) and len(got) >= 20
    for n in got:
        close(got[n][0], record[n][0], name=f"{label} memory mean {n}")
        close(got[n][1], record[n][1], name=f"{label} memory var {n}")


def _state_dict_unchanged(m, before, keys, label):
    aset = set(keys)
    for k, v in m.state_dict().items():
        if k not in aset:
            assert torch.equal(v, before[k]), f"{label}: {k} changed"


def _hp(B):
    return T.dvm_hp(B, img_size=64)


LR = 1e-3


@pytest.mark.parametrize("label,B,N,alpha,seeds", [("b1_online", 1, None, 0.05, (41, 42, 43, 44)), ("b8_n16", 8, 16.0, 0.05, (51, 52))])
def test_tent_step_on_the_memory_matches_the_contract_restated_in_float64(label, B, N, alpha, seeds):
    """TENT's bars (tests/test_gpu_tta.py): predictions 3e-5 scaled, every gradient of A at 3 e32 + 1e-4, Adam within 2.2 lr step,
    everything outside A (running buffers included) bit-identical; the memory after each batch at close() of the float64 update."""
    import test_gpu_step as S
    hp = _hp(B)
    sd = T.initial_state(hp, 5)
    m = T.make_model(hp, sd, tta=True, tta_method="tent", tta_lr=LR, tta_bn_momentum=alpha, tta_bn_prior=N)
    m.freeze()
    keys = T.adapted_keys(m)
    rho = alpha if N is None else B / (N + B)
    opt, bad = {}, []
    for step, seed in enumerate(seeds, start=1):
        x, y = T.tta_batch(hp, B, seed)
        before = T.full_state(m)
        sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
        mem_before = memory_of(m, sd_before)
        with S._trace_decisions() as trace:
            m.test_step(T.to_dev((x, y)), step - 1)
            torch.cuda.synchronize()
            decisions = S._device_decisions(m, trace)
        assert m._bn_mem.t == step and m._bn_mem.alpha == alpha
        probs = m.last_tta["probs"].cpu().double()
        rec = {}
        with memory_oracle(mem_before, rho, alpha, record=rec):
            p64, g64, flips = T.tent_restated(sd_before, keys, x, hp, torch.float64, decisions)
        with memory_oracle(mem_before, rho, alpha):
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
        O.adam_step(sd32, g32, opt, step, LR)
        aset = set(keys)
        for k, v in T.full_state(m).items():
            if k in aset:
                dev = float((v.cpu() - sd32[k]).abs().max())
                if dev > 2.2 * LR * step:
                    bad.append((step, "adam " + k, dev))
            elif not torch.equal(v, before[k]):
                bad.append((step, "changed " + k))
        _check_memory(m, rec, f"[{label}] batch {step}")
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


def _record_args(monkeypatch, names):
    """record (name, args) of the C-ABI calls among `names`"""
    from stil_tta_amd._lib import lib
    L = lib()
    calls = []
    for name in names:
        orig = getattr(L, name)
        monkeypatch.setitem(L.__dict__, name, lambda *a, _o=orig, _n=name, **k: (calls.append((_n, a)), _o(*a, **k))[1])
    return calls


def _mem_ptrs(call):
    """-> (mean, var, mean_out, var_out) pointers of a recorded stil_bn_memory_fwd(_tiles) call"""
    name, a = call
    return a[5:9] if name.endswith("_tiles") else a[3:7]


def test_sar_step_on_the_memory_both_passes_read_one_estimate_and_it_moves_once(monkeypatch):
    """B = 4, one batch, a margin that keeps every row (the selection is tests/test_gpu_sar.py's subject).  Both passes read the same
    front buffers, the first alone writes; the memory after the step is ONE update by the first pass's statistics.  Predictions (first
    pass; float64 on its own decisions: the step's trace ends holding the second pass's) at 3e-5 scaled; the second pass's gradients, at
    the device's own perturbed A and on its decisions, at 3 e32 + 1e-4; Adam within 2.2 lr."""
    import test_gpu_sar as R
    import test_gpu_step as S
    B, alpha, e0 = 4, 0.05, 6.0
    hp = _hp(B)
    sd = T.initial_state(hp, 5)
    m = T.make_model(hp, sd, tta=True, tta_method="sar", tta_lr=LR, tta_bn_momentum=alpha, tta_e_margin=e0, tta_sar_reset=False)
    m.freeze()
    keys = T.adapted_keys(m)
    x, y = T.tta_batch(hp, B, 61)
    before = T.full_state(m)
    sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
    mem_before = memory_of(m, sd_before)
    calls = _record_args(monkeypatch, ("bn_memory_fwd", "bn_memory_fwd_tiles"))
    with S._trace_decisions() as trace:
        m.test_step(T.to_dev((x, y)), 0)
        torch.cuda.synchronize()
        dec2 = S._device_decisions(m, trace)
    assert len(calls) == 106
    for first, second in zip(calls[:53], calls[53:]):
        a, b = _mem_ptrs(first), _mem_ptrs(second)
        assert a[0] == b[0] and a[1] == b[1], "the second pass read another estimate"
        assert a[2] is not None and a[3] is not None and b[2] is None and b[3] is None, "the first pass alone writes the update"
    assert m._bn_mem.t == 1
    lt, st = m.last_tta, m._tent
    rec = {}
    with memory_oracle(mem_before, alpha, alpha, record=rec):
        r1 = R.sar_pass(sd_before, keys, x, hp, torch.float64, e0)
    assert r1["n"] == B and int(lt["n_first"]) == B
    d = S._scaled(lt["probs"].cpu().double().numpy(), r1["p"].numpy())
    print(f"predictions scaled error {d:.2e}")
    assert d <= 3e-5
    _check_memory(m, rec, "sar")
    e_dev = dict(zip(keys, [v.cpu() for v in st._compact_views(st.e)]))
    sd_pert = R.perturbed(sd_before, e_dev)
    sel1 = lt["selected_first"].cpu().bool()
    with memory_oracle(mem_before, alpha, alpha):
        r2 = R.sar_pass(sd_pert, keys, x, hp, torch.float64, e0, prior=sel1, decisions=dec2)
        r2free = R.sar_pass(sd_pert, keys, x, hp, torch.float64, e0, prior=sel1)
        r2_32 = R.sar_pass(sd_pert, keys, x, hp, torch.float32, e0, prior=sel1)
    S._check_flips(r2["flips"])
    assert r2["n"] == B and int(lt["n_selected"]) == B
    gd, bad, ratios = T.device_grads(m), [], []
    for k in keys:
        e32, err = T._rel(r2_32["g"][k].double(), r2free["g"][k]), T._rel(gd[k], r2["g"][k])
        ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
        if err > 3 * e32 + 1e-4:
            bad.append(("grad (pass 2) " + k, err, e32))
    print(f"pass 2 gradient error / (3*e32 + 1e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
    sd32 = {k: v.clone() for k, v in sd_before.items()}
    O.adam_step(sd32, r2_32["g"], {}, 1, LR)
    aset = set(keys)
    for k, v in T.full_state(m).items():
        if k in aset:
            if float((v.cpu() - sd32[k]).abs().max()) > 2.2 * LR:
                bad.append(("adam " + k,))
        elif not torch.equal(v, before[k]):
            bad.append(("changed " + k,))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


_BWD_CALLS = ("bn_train_bwd", "bn_train_bwd_tiles", "bn_prior_bwd", "bn_prior_bwd_tiles", "wgrad_tn", "wgrad_tn_partial", "adam_step")
_BN_FWD = ("bn_train_fwd", "bn_train_fwd_tiles", "bn_prior_fwd", "bn_prior_fwd_tiles", "bn_memory_fwd", "bn_memory_fwd_tiles")


def test_bn_adapt_on_the_memory_four_single_images(monkeypatch):
    import test_gpu_step as S
    B, alpha = 1, 0.05
    hp = _hp(B)
    sd = T.initial_state(hp, 5)
    m = T.make_model(hp, sd, tta=True, tta_method="bn_adapt", tta_bn_momentum=alpha)
    calls = P._record(monkeypatch, _BWD_CALLS)
    keys = T.adapted_keys(m)[:2]
    before = T.full_state(m)
    for step, seed in enumerate((71, 72, 73, 74), start=1):
        x, y = T.tta_batch(hp, B, seed)
        mem_before = memory_of(m, sd)
        with S._trace_decisions() as trace:
            p = m.test_step(T.to_dev((x, y)), step - 1)
            torch.cuda.synchronize()
            decisions = S._device_decisions(m, trace)
        assert m._tent is None and m._bn_mem.t == step and set(m.last_tta) == {"y_hat_m", "probs"}
        rec = {}
        with memory_oracle(mem_before, alpha, alpha, record=rec):
            p64, _, flips = T.tent_restated(sd, keys, x, hp, torch.float64, decisions)
        S._check_flips(flips)
        d = S._scaled(p.cpu().double().numpy(), p64.numpy())
        print(f"bn_adapt batch {step}: predictions scaled error {d:.2e}")
        assert d <= 3e-5
        _check_memory(m, rec, f"bn_adapt batch {step}")
    assert calls == [], calls
    after = T.full_state(m)
    for k in before:
        assert torch.equal(before[k], after[k]), k


def test_dua_three_single_samples_with_the_schedule(monkeypatch):
    """B = 1, V = 8, 0.1 / 0.94 / 0.005: per sample the views are rebuilt from last_tta["draws"], the memory after the sample is the
    float64 update (rho = 1, alpha_t, unbiased variance) by the statistics of encoder_imaging on those views at close(), and the scores
    are eval-mode BatchNorm on the device's memory at 3e-5 scaled.  No backward, weight-gradient or Adam call; no TentState; the
    state_dict, running buffers included, never changes."""
    import test_gpu_step as S
    from stil_tta_amd import tta
    B, V = 1, 8
    hp = _hp(B)
    sd = T.initial_state(hp, 5)
    m = T.make_model(hp, sd, tta=True, tta_method="dua", tta_views=V, tta_bn_momentum=0.1, tta_bn_momentum_decay=0.94, tta_bn_momentum_min=0.005)
    m.freeze()
    calls = P._record(monkeypatch, _BWD_CALLS)
    keys = T.adapted_keys(m)[:2]
    before = T.full_state(m)
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for t, seed in enumerate((81, 82, 83), start=1):
        x, y = T.tta_batch(hp, B, seed)
        mem_before = memory_of(m, sd)
        with S._trace_decisions() as trace, torch.inference_mode():
            p = m.test_step(T.to_dev((x, y)), t - 1)
            torch.cuda.synchronize()
            decisions = S._device_decisions(m, trace)
        lt = m.last_tta
        a = momentum(0.1, 0.94, 0.005, t)
        assert set(lt) == {"y_hat_m", "probs", "alpha", "draws"} and lt["alpha"] == a and m._bn_mem.t == t and m._tent is None
        views, tab, draws = tta.make_views(m, T.to_dev((x, y))[0], lt["draws"])
        assert draws is lt["draws"] and tuple(views.shape) == (B * V, 3, 64, 64) and tuple(tab.shape)[0] == B * V
        assert torch.equal(views, tta.make_views(m, T.to_dev((x, y))[0], lt["draws"])[0]), "the views do not rebuild bit for bit"
        rec = {}
        with memory_oracle(mem_before, 1.0, a, unbiased=True, record=rec), torch.no_grad():
            O.resnet_forward(sd64, "model.encoder_imaging.", views.cpu().double(), hp.model, True)
        _check_memory(m, rec, f"dua sample {t}")
        with memory_oracle(memory_of(m, None), 0.0, a):
            p64, _, flips = T.tent_restated(sd, keys, x, hp, torch.float64, decisions)
        S._check_flips(flips)
        d = S._scaled(p.cpu().double().numpy(), p64.numpy())
        print(f"dua sample {t}: alpha {a:.5f}, predictions scaled error {d:.2e}")
        assert d <= 3e-5
        close(torch.softmax(lt["y_hat_m"].double(), 1), p, name="probs is softmax(y_hat_m)")
    assert calls == [], calls
    after = T.full_state(m)
    for k in before:
        assert torch.equal(before[k], after[k]), k


# ------------------------------------------------------------------------------------------ state rules and properties
def _small(method="tent", **tta):
    hp = T.dvm_hp(16, img_size=64)
    sd = T.initial_state(hp, 5)
    return hp, sd, (lambda: T.make_model(hp, sd, tta=True, tta_method=method, **tta))


def _source_memory(m):
    return all(torch.equal(a, mod.running_mean) and torch.equal(b, mod.running_var) for (a, b), mod in zip(m._bn_mem.state(), m._bn_mem.layers))


def test_reset_episodic_and_load_state_dict():
    hp, sd, mk = _small(tta_bn_momentum=0.1, tta_bn_momentum_decay=0.9)
    b1, b2 = (T.to_dev(T.tta_batch(hp, 16, s)) for s in (11, 12))
    m = mk()
    assert m._bn_mem is None
    p1 = m.test_step(b1, 0).clone()
    m.test_step(b2, 1)
    assert m._bn_mem.t == 2 and not _source_memory(m)
    m.reset_tta()
    assert m._bn_mem.t == 0 and _source_memory(m)
    assert torch.equal(m.test_step(b1, 0), p1), "after reset_tta the first batch does not repeat"
    # episodic: every batch starts from the checkpoint's statistics and alpha_1
    e, f = _small(tta_bn_momentum=0.1, tta_bn_momentum_decay=0.9, tta_episodic=True)[2](), mk()
    e.test_step(b1, 0)
    assert torch.equal(e.test_step(b2, 1), f.test_step(b2, 0)) and e._bn_mem.t == 1 and e._bn_mem.alpha == f._bn_mem.alpha
    # load_state_dict drops the state
    m.load_state_dict({k: v.cuda() for k, v in sd.items()})
    assert m._bn_mem is None and m._tent is None
    for mm in (m, e, f):
        for k, v in mm.state_dict().items():
            if "running_" in k or "num_batches_tracked" in k:
                assert torch.equal(v.cpu(), sd[k]), k


def test_freeze_inference_mode_and_fit_test_with_a_ragged_last_batch(tmp_path):
    from stil_tta_amd import fit
    hp, sd, mk = _small(tta_bn_momentum=0.05, tta_bn_prior=16.0)
    b = T.to_dev(T.tta_batch(hp, 16, 14))
    a, c = mk(), mk()
    a.freeze()
    with torch.inference_mode():
        pa = a.test_step(b, 0)
    assert torch.equal(pa, c.test_step(b, 0))
    assert all(torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) for u, v in zip(a._bn_mem.state(), c._bn_mem.state()))
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
    assert f._bn_mem.t == h._bn_mem.t == 3
    assert all(torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) for u, v in zip(f._bn_mem.state(), h._bn_mem.state()))
    plain = _small(tta_bn_prior=16.0)[2]()     # the same stream on the checkpoint's statistics: the memory must show from batch 2 on
    for i, bt in enumerate(loader):
        plain.test_step(T.to_dev(bt), i)
    assert not torch.equal(h.last_tta["probs"], plain.last_tta["probs"]), "the memory changed nothing over a stream"


def test_memory_steps_synchronise_no_more_than_the_same_steps_without():
    hp, sd, mk = _small()
    variants = {"tent": mk, "tent + memory": _small(tta_bn_momentum=0.05)[2], "bn_adapt": _small("bn_adapt")[2],
                "bn_adapt + memory": _small("bn_adapt", tta_bn_momentum=0.05)[2]}   # dua's views upload their draws: test_gpu_margent's subject
    batches = [T.to_dev(T.tta_batch(hp, 16, 30 + i)) for i in range(3)]
    counts = {}
    for name, make in variants.items():
        mm = make()
        mm.test_step(batches[0], 0)
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
        counts[name] = [str(w.message) for w in rec if "synchroniz" in str(w.message).lower()]
        if name == "tent":   # control: the counter sees a device -> host read
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                torch.cuda.set_sync_debug_mode("warn")
                try:
                    float(mm.last_tta["loss"])
                finally:
                    torch.cuda.set_sync_debug_mode("default")
            assert any("synchroniz" in str(w.message).lower() for w in rec), "the sync counter sees nothing"
    print("synchronising calls over two steps: " + ", ".join(f"{k} {len(v)}" for k, v in counts.items()))
    for name in ("tent", "bn_adapt"):
        assert len(counts[name + " + memory"]) <= len(counts[name]), (name, counts[name + " + memory"], counts[name])


@pytest.mark.parametrize("method", ["tent", "bn_adapt"])
def test_defaults_leave_the_call_sequence_and_the_results_alone(method, monkeypatch):
    """Every new key at its default: no memory is created, no stil_bn_memory_* call runs, the BatchNorm call sequence is the one
    tests/test_gpu_bnprior.py pins for the parent, and spelling the defaults out changes no bit over two batches."""
    hp, sd, mk = _small(method)
    spelled = _small(method, tta_bn_momentum=None, tta_bn_momentum_decay=1.0, tta_bn_momentum_min=0.0)[2]
    a, s = mk(), spelled()
    calls = P._record(monkeypatch, _BN_FWD + _BWD_CALLS)
    for i, seed in enumerate((11, 12)):
        b = T.to_dev(T.tta_batch(hp, 16, seed))
        calls.clear()
        pa = a.test_step(b, i)
        torch.cuda.synchronize()
        seq = list(calls)
        ps = s.test_step(b, i)
        torch.cuda.synchronize()
        assert torch.equal(pa, ps) and a._bn_mem is None and s._bn_mem is None
        assert not any(n.startswith("bn_memory_") or n.startswith("bn_prior_") or n.startswith("wgrad") for n in seq)
        nf, nbw = sum(n.startswith("bn_train_fwd") for n in seq), sum(n.startswith("bn_train_bwd") for n in seq)
        assert nf == 53 and all(n.startswith("bn_train_fwd") for n in seq[:nf])
        if method == "tent":
            assert nbw == 53 and all(n.startswith("bn_train_bwd") for n in seq[nf:nf + nbw]) and seq.count("adam_step") >= 1
        else:
            assert seq[nf:] == []
    sa, ss = T.full_state(a), T.full_state(s)
    for k in sa:
        assert torch.equal(sa[k], ss[k]), k


def test_call_sequence_with_the_memory(monkeypatch):
    """With tta_bn_momentum the sequence is the parent's with every BatchNorm forward replaced by its memory counterpart; the backward
    is the prior's, unchanged."""
    hp, sd, mk = _small()
    mm = _small(tta_bn_momentum=0.05)[2]
    b = T.to_dev(T.tta_batch(hp, 16, 7))
    calls = P._record(monkeypatch, _BN_FWD + _BWD_CALLS)
    mk().test_step(b, 0)
    torch.cuda.synchronize()
    plain = list(calls)
    calls.clear()
    mm().test_step(b, 0)
    torch.cuda.synchronize()
    assert list(calls) == [n.replace("bn_train_fwd", "bn_memory_fwd").replace("bn_train_bwd", "bn_prior_bwd") for n in plain]
