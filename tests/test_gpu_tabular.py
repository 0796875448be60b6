"""stil_tab_embed_fwd / _bwd, stil_saint_embed_fwd / _bwd and stil_colmlp_fwd / _bwd called through the C ABI with raw addresses
on every case of tests/tabular_cases.py, against the float64 definitions there, with the suite's `close()` at `TOL`
(tests/test_tabular_cases_cpu.py shows that fp32 in the kernels' own summation order meets it on every case, and that it rejects
what a subtly wrong kernel would produce).

Every output buffer is longer than what may be written and holds a sentinel there; whatever may not be read holds NaN (table
rows no sample selects, the other family's columns of x, the other family's gradient tokens); every call is made twice on
fresh buffers and must repeat bit for bit; every backward runs with accumulate 0 (on sentinel-filled gradients: it must
overwrite all it owns) and 1 (on random gradients: prefill + gradient, rows without a sample bit-equal to the prefill).

Only arguments the entry points accept and the kernels can follow are passed here: every code lies in its column's range.
The refusals are tested on the host (test_tabular_cases_cpu.py), where a missed one cannot store anywhere."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tabular_cases as T  # noqa: E402
from tabular_cases import NAN, SENT  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402  (the suite's tolerance and comparison, unchanged)

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def L():
    from stil_tta_amd._lib import lib
    return lib()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nTABULAR_DEVICE worst error / allowance:", {f: f"{r:.3f} ({n})" for f, (r, n) in sorted(WORST.items())})


def _st():
    from stil_tta_amd.ops import _stream
    return _stream()


def P(t):
    return None if t is None else t.data_ptr()


_KEEP = []


def dev(t):
    """a contiguous CUDA copy that stays alive until the test ends (the entry points take raw addresses)"""
    _KEEP.append(t.cuda().contiguous())
    return _KEEP[-1]


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    _KEEP.clear()


class Guarded:
    """a device buffer that starts with `t` and goes on with `extra` sentinel elements nothing may write"""

    def __init__(self, t, extra):
        self.n = t.numel()
        flat = torch.full((self.n + extra,), SENT, dtype=torch.float32)
        flat[:self.n] = t.flatten()
        self.buf = dev(flat)
        self.view = self.buf[:self.n].view(t.shape)

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.n:] == SENT).all())


def filled(shape, value=SENT):
    return torch.full(tuple(shape), value, dtype=torch.float32)


def check(family, name, got, ref):
    close(got, ref, name=f"{family}/{name}")
    WORST[family] = max(WORST.get(family, (0.0, "")), (T.ratio(got, ref, TOL), name))


def poisoned(t, keep_cols):
    """x with NaN in every column but keep_cols"""
    out = filled(t.shape, NAN)
    out[:, keep_cols] = t[:, keep_cols]
    return out


def poisoned_rows(emb, rows):
    out = emb.clone()
    out[rows] = NAN
    return out


def prefills(x, names, shapes, acc):
    """accumulate = 1: the case's random prefill; accumulate = 0: sentinels, which the kernel has to overwrite"""
    return {k: (x["pre_" + k].clone() if acc else filled(shapes[k])) for k in names}


def expected(ref, pre, acc):
    return pre.double() + ref if acc else ref


# ====================================================================================================================
# stil_tab_embed_fwd / stil_tab_embed_bwd
# ====================================================================================================================
def _tab_fwd(L, c, x, emb):
    T_ = len(c.cards) + c.ncon + 1
    h = Guarded(filled((c.B, T_, c.D)), c.D)
    L.tab_embed_fwd(P(dev(x["x"])), P(dev(x["offs"])) if c.cards else None, P(dev(emb)) if c.cards else None,
                    P(dev(x["con_w"])) if c.ncon else None, P(dev(x["con_b"])) if c.ncon else None, P(dev(x["cls"])), P(dev(x["colemb"])),
                    h.ptr(), c.B, len(c.cards) + c.ncon, len(c.cards), c.D, _st())
    torch.cuda.synchronize()
    assert h.intact()
    return h.view.cpu()


def _tab_bwd(L, c, x, acc):
    ncat, ncols = len(c.cards), len(c.cards) + c.ncon
    names = [k for k in T.TAB_GRADS if k[2:] in x]
    shapes = {k: x[k[2:]].shape for k in names}
    pre = prefills(x, names, shapes, acc)
    bufs = {k: Guarded(pre[k], c.D if k in ("d_emb", "d_colemb") else 7) for k in names}
    if not c.ncon:                                     # cat-only: live buffers the kernel has no business with
        bufs["d_con_w"], bufs["d_con_b"] = Guarded(filled((0,)), c.D + 7), Guarded(filled((0,)), c.D + 7)
    nb = L.tab_embed_bwd_workspace_bytes(ncols, c.D)
    ws = Guarded(filled((nb // 4,), 0.5), 64)
    L.tab_embed_bwd(P(dev(x["g"])), P(dev(x["x"])), P(dev(x["offs"])) if ncat else None, P(dev(x["rowcol"])) if ncat else None,
                    x["emb"].shape[0] if ncat else 0, bufs["d_emb"].ptr() if ncat else None, bufs["d_con_w"].ptr(), bufs["d_con_b"].ptr(),
                    bufs["d_cls"].ptr(), bufs["d_colemb"].ptr(), c.B, ncols, ncat, c.D, acc, ws.ptr(), nb, _st())
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.intact(), f"{c.name}: a write past {k}"
    assert ws.intact(), f"{c.name}: a write past the workspace"
    return {k: bufs[k].view.cpu() for k in names}, pre


@pytest.mark.parametrize("name", [c.name for c in T.TAB_CASES])
def test_tab_embed_against_float64(L, name):
    c = T.BY_NAME["tab", name]
    x, ref = T.tab_inputs(c), T.tab_reference(c)
    ncat = len(c.cards)
    dead = T.undrawn_rows(x, False) if ncat else []
    emb = poisoned_rows(x["emb"], dead) if ncat else None
    h = _tab_fwd(L, c, x, emb)
    assert torch.equal(h, _tab_fwd(L, c, x, emb))
    assert bool(torch.isfinite(h).all())
    check("tab", f"{name}/h", h, ref["out"])
    assert torch.equal(h[:, 0], (x["cls"] + x["colemb"][0]).expand(c.B, c.D))                      # one fp32 add
    if ncat:
        assert torch.equal(h[:, 1:1 + ncat], x["emb"][T.table_index(x, False)] + x["colemb"][1:1 + ncat])
    for acc in T.accumulates("tab", name):
        got, pre = _tab_bwd(L, c, x, acc)
        again, _ = _tab_bwd(L, c, x, acc)
        for k in got:
            assert torch.equal(got[k], again[k]), (name, k, acc)
            check("tab", f"{name}/{k}/acc{acc}", got[k], expected(ref[k], pre[k], acc))
        if ncat and dead:
            assert torch.equal(got["d_emb"][dead], pre["d_emb"][dead] if acc else torch.zeros(len(dead), c.D))


# ====================================================================================================================
# stil_saint_embed_fwd / stil_saint_embed_bwd
# ====================================================================================================================
def _saint_fwd(L, c, x, xx, emb, out=None):
    ncat, nfeats = len(c.cards), len(c.cards) + c.ncon + 1
    out = out or Guarded(filled((c.B, nfeats, c.d)), c.d)
    L.saint_embed_fwd(P(dev(xx)), P(dev(x["cat_cols"])) if ncat else None, P(dev(x["offs"])), P(dev(emb)), P(dev(x["pos"])), out.ptr(),
                      c.B, ncat + c.ncon, ncat, nfeats, c.d, _st())
    torch.cuda.synchronize()
    assert out.intact()
    return out.view.cpu()


def _saint_bwd(L, c, x, xx, g, acc):
    ncat, nfeats = len(c.cards), len(c.cards) + c.ncon + 1
    pre = prefills(x, ("d_emb", "d_pos"), {"d_emb": x["emb"].shape, "d_pos": x["pos"].shape}, acc)
    bufs = {k: Guarded(pre[k], c.d) for k in pre}
    L.saint_embed_bwd(P(dev(g)), P(dev(xx)), P(dev(x["cat_cols"])) if ncat else None, P(dev(x["offs"])), P(dev(x["rowcol"])), x["emb"].shape[0],
                      bufs["d_emb"].ptr(), bufs["d_pos"].ptr(), c.B, ncat + c.ncon, ncat, nfeats, c.d, acc, _st())
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.intact(), f"{c.name}: a write past {k}"
    return {k: b.view.cpu() for k, b in bufs.items()}, pre


@pytest.mark.parametrize("name", [c.name for c in T.SAINT_CASES])
def test_saint_embed_against_float64(L, name):
    c = T.BY_NAME["saint", name]
    x, ref = T.saint_inputs(c), T.saint_reference(c)
    ncat = len(c.cards)
    dead = T.undrawn_rows(x, True)
    xx = poisoned(x["x"], x["cat_cols"].long())                            # the continuous columns hold NaN
    emb = poisoned_rows(x["emb"], dead)
    out = _saint_fwd(L, c, x, xx, emb)
    assert torch.equal(out, _saint_fwd(L, c, x, xx, emb))
    assert bool((out[:, ncat + 1:] == SENT).all()), "the continuous tokens are the column MLP's"
    tok = out[:, :ncat + 1]
    assert bool(torch.isfinite(tok).all())
    check("saint", f"{name}/out", tok, ref["out"])
    assert torch.equal(tok, x["emb"][T.table_index(x, True)] + x["pos"][:ncat + 1])               # one fp32 add
    g = x["g"].clone()
    g[:, ncat + 1:] = NAN                                                  # the continuous tokens' gradient rows hold NaN
    for acc in T.accumulates("saint", name):
        got, pre = _saint_bwd(L, c, x, xx, g, acc)
        again, _ = _saint_bwd(L, c, x, xx, g, acc)
        for k in got:
            assert torch.equal(got[k], again[k]), (name, k, acc)
        check("saint", f"{name}/d_emb/acc{acc}", got["d_emb"], expected(ref["d_emb"], pre["d_emb"], acc))
        check("saint", f"{name}/d_pos/acc{acc}", got["d_pos"][:ncat + 1], expected(ref["d_pos"][:ncat + 1], pre["d_pos"][:ncat + 1], acc))
        assert torch.equal(got["d_pos"][ncat + 1:], pre["d_pos"][ncat + 1:]), "d_pos rows of the continuous tokens are not this kernel's"
        if dead:
            assert torch.equal(got["d_emb"][dead], pre["d_emb"][dead] if acc else torch.zeros(len(dead), c.d))


# ====================================================================================================================
# stil_colmlp_fwd / stil_colmlp_bwd
# ====================================================================================================================
def scattered(tensors, key, extra=5):
    """each tensor in a Guarded buffer of its own, allocated in a shuffled order with spacers between -> in the given order"""
    order = torch.randperm(len(tensors), generator=T.gen(5, key, len(tensors))).tolist()
    out = [None] * len(tensors)
    for n, i in enumerate(order):
        out[i] = Guarded(tensors[i], extra)
        dev(filled((17 + 64 * (n % 3),), NAN))
    return out


def table(bufs):
    return dev(torch.tensor([b.ptr() for b in bufs], dtype=torch.int64))


def _params(c, x):
    """[w1_0, b1_0, W2_0, b2_0, w1_1, ...] as the tables list them"""
    return [x[k][j] for j in range(c.ncon) for k in T.MLP_PARAMS]


def _mlp_fwd(L, c, x, xx, out=None):
    nfeats = c.ncat + c.ncon + 1
    out = out or Guarded(filled((c.B, nfeats, c.d)), c.d)
    par = scattered(_params(c, x), 1)
    L.colmlp_fwd(P(dev(xx)), P(dev(x["con_cols"])), P(table(par)), out.ptr(), c.B, c.ncat + c.ncon, c.ncon, nfeats, c.ncat + 1, c.hid, c.d, _st())
    torch.cuda.synchronize()
    assert out.intact() and all(b.intact() for b in par)
    return out.view.cpu()


def _mlp_bwd(L, c, x, xx, g, acc):
    nfeats = c.ncat + c.ncon + 1
    pre = [x["pre_d_" + k][j].clone() if acc else filled(x[k][j].shape) for j in range(c.ncon) for k in T.MLP_PARAMS]
    par, grads = scattered(_params(c, x), 2), scattered(pre, 3)
    L.colmlp_bwd(P(dev(g)), P(dev(xx)), P(dev(x["con_cols"])), P(table(par)), P(table(grads)), c.B, c.ncat + c.ncon, c.ncon, nfeats, c.ncat + 1,
                 c.hid, c.d, acc, _st())
    torch.cuda.synchronize()
    assert all(b.intact() for b in grads), f"{c.name}: a write past a gradient"
    return [b.view.cpu() for b in grads], pre


@pytest.mark.parametrize("name", [c.name for c in T.MLP_CASES])
def test_colmlp_against_float64(L, name):
    c = T.BY_NAME["mlp", name]
    x, ref = T.mlp_inputs(c), T.mlp_reference(c)
    tok0 = c.ncat + 1
    xx = poisoned(x["x"], x["con_cols"].long())                            # the categorical columns hold NaN
    out = _mlp_fwd(L, c, x, xx)
    assert torch.equal(out, _mlp_fwd(L, c, x, xx))
    assert bool((out[:, :tok0] == SENT).all()), "the CLS and categorical tokens are the embedding's"
    assert bool(torch.isfinite(out[:, tok0:]).all())
    check("mlp", f"{name}/out", out[:, tok0:], ref["out"])
    if not c.bwd:
        return                                                             # the backward refuses this shape: test_tabular_cases_cpu.py
    g = x["g"].clone()
    g[:, :tok0] = NAN
    for acc in T.accumulates("mlp", name):
        got, pre = _mlp_bwd(L, c, x, xx, g, acc)
        again, _ = _mlp_bwd(L, c, x, xx, g, acc)
        for n, (a, b, q) in enumerate(zip(got, again, pre)):
            j, k = divmod(n, 4)
            assert torch.equal(a, b), (name, j, k, acc)
            check("mlp", f"{name}/d_{T.MLP_PARAMS[k]}[{j}]/acc{acc}", a, expected(ref["d_" + T.MLP_PARAMS[k]][j], q, acc))
    if c.edges:                                                            # zero pre-activation and dead unit: no gradient at all
        got, _ = _mlp_bwd(L, c, x, xx, g, 0)
        zero = T.mlp_manual_grads(c, x)
        assert float(zero["d_w1"][0][1]) == 0.0 and float(got[0][1]) == 0.0 and float(got[1][1]) == 0.0          # dead for every sample
        if c.B == 1:
            assert float(got[0][0]) == 0.0 and float(got[1][0]) == 0.0                                           # pre-activation exactly 0


def test_colmlp_follows_its_pointer_tables(L):
    """parameters and gradients at shuffled places of two arenas with gaps between: the kernel follows the tables (no slab
    assumed), reads no gap (NaN) and writes none (sentinel)"""
    c = T.BY_NAME["mlp", "model_B12"]
    x, ref = T.mlp_inputs(c), T.mlp_reference(c)
    tensors = _params(c, x)
    order = torch.randperm(len(tensors), generator=T.gen(6)).tolist()
    offs, end = {}, 3
    for i in order:                                                        # a different gap before each, 4-byte aligned only
        offs[i] = end
        end += tensors[i].numel() + 1 + 2 * (i % 5)
    arena, garena = filled((end,), NAN), filled((end,))
    for i, t in enumerate(tensors):
        arena[offs[i]:offs[i] + t.numel()] = t.flatten()
    arena, garena = dev(arena), dev(garena)
    addr = lambda a: dev(torch.tensor([a.data_ptr() + 4 * offs[i] for i in range(len(tensors))], dtype=torch.int64))
    out = Guarded(filled((c.B, c.ncat + c.ncon + 1, c.d)), c.d)
    args = (c.B, c.ncat + c.ncon, c.ncon, c.ncat + c.ncon + 1, c.ncat + 1, c.hid, c.d)
    L.colmlp_fwd(P(dev(x["x"])), P(dev(x["con_cols"])), P(addr(arena)), out.ptr(), *args, _st())
    L.colmlp_bwd(P(dev(x["g"])), P(dev(x["x"])), P(dev(x["con_cols"])), P(addr(arena)), P(addr(garena)), *args, 0, _st())
    torch.cuda.synchronize()
    check("mlp", "tables/out", out.view[:, c.ncat + 1:], ref["out"])
    got, mask = garena.cpu(), torch.ones(end, dtype=torch.bool)
    for i, t in enumerate(tensors):
        j, k = divmod(i, 4)
        check("mlp", f"tables/d_{T.MLP_PARAMS[k]}[{j}]", got[offs[i]:offs[i] + t.numel()].view(t.shape), ref["d_" + T.MLP_PARAMS[k]][j])
        mask[offs[i]:offs[i] + t.numel()] = False
    assert bool((got[mask] == SENT).all()) and int(mask.sum()) > len(tensors)


# ====================================================================================================================
# both forwards on one token buffer
# ====================================================================================================================
@pytest.mark.parametrize("name,hid", T.OWNERSHIP)
def test_each_forward_stays_inside_its_own_tokens(L, name, hid):
    c, m, x = T.ownership_inputs(name, hid)
    ref = T.ownership_reference(name, hid)
    ncat, nfeats = len(c.cards), len(c.cards) + c.ncon + 1
    alone = _saint_fwd(L, c, x, x["x"], x["emb"])
    assert bool((alone[:, ncat + 1:] == SENT).all())
    alone = _mlp_fwd(L, m, x, x["x"])
    assert bool((alone[:, :ncat + 1] == SENT).all())
    for first in (0, 1):                                                   # in either order
        out = Guarded(filled((c.B, nfeats, c.d)), c.d)
        for step in (first, 1 - first):
            (_mlp_fwd(L, m, x, x["x"], out) if step else _saint_fwd(L, c, x, x["x"], x["emb"], out))
        check("saint", f"{name}/both forwards", out.view.cpu(), ref)
