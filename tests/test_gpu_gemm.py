"""Every instantiation of the NT GEMM and of the weight gradient (csrc/gemm.hip) through the C ABI -- `stil_gemm_nt`,
`stil_wgrad_tn`, `stil_wgrad_tn_partial` with an explicit `tune`, explicit leading dimensions and an explicit workspace --
against the float64 definitions of tests/gemm_cases.py on the same fp32 inputs.

What one case checks:
  * `stil_gemm_nt_config` / `stil_wgrad_config` on the real operands name the kernel the table claims (the coverage of the
    module rests on the tables: tests/test_gemm_cases_cpu.py proves on the host that they reach every instantiation);
  * every output (C, `pre`, `colstats`, `bstats`, dW, the slab partials) against float64 within FACTOR = 4 x the error fp32 ATen
    makes on the inputs of the case's family (gemm_cases.bounds(), capped at 2e-5; DESIGN.md section 2 records the figures); the
    split-precision kernels by the rule of test_gemm_nt_split_precision_mode_...: relative L2 within 1.25 x the fp32-exact kernel's;
  * whatever must not be read holds NaN: the gaps of every padded leading dimension, rows past M, the float before an offset
    operand, the margins of every buffer, the unread row of an a_bn / x_bn statistics block, the slabs of a split workspace;
  * whatever must not be written holds a sentinel that is compared bit for bit afterwards: the gaps of ldc, rows the output map
    skips, statistics tiles before bs_tile0 and after the last tile, the margins (dW is [N, Kdst]: a column at or past Kdst would
    land in the next row and fail the comparison);
  * split-K: the ticket words are zero after the launch and a second launch with the same workspace gives the same bits; an empty
    weight-gradient slab holds exact zeros.
Each comparison prints its figure (`GEMM_ERR ...`) before it asserts."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = G.MARGIN
SENT_BITS = torch.tensor(G.SENT).view(torch.int32).item()


@pytest.fixture(scope="module")
def L():
    from stil_tta_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def bounds():
    b = G.bounds()
    print("GEMM_YARDSTICK", {f: f"{e:.3e}" for f, e in G.aten_errors().items()}, "bounds", {f: f"{v:.3e}" for f, v in b.items()})
    return b


def _st():
    from stil_tta_amd.ops import _stream
    return _stream()


class Buf:
    """a [rows, cols] operand with row stride ld inside a flat device buffer: MARGIN floats, `off` floats, the rows (and `extra`
    rows more), MARGIN floats -- all `fill` except the [rows, cols] values"""

    def __init__(self, rows, cols, ld, off=0, fill=G.NAN, extra=2, values=None):
        self.rows, self.cols, self.ld, self.start = rows, cols, ld, MARGIN + off
        self.flat = torch.full((2 * MARGIN + off + (rows + extra) * ld,), fill, dtype=torch.float32, device="cuda")
        assert self.flat.data_ptr() % 256 == 0
        self.view = torch.as_strided(self.flat, (rows, cols), (ld, 1), self.start)
        if values is not None:
            self.view.copy_(values)
        self.ptr = self.flat.data_ptr() + 4 * self.start

    def index(self, rows=None):
        """flat positions of the [rows, cols] elements (rows: a LongTensor of row numbers, default all)"""
        r = torch.arange(self.rows) if rows is None else rows
        return (self.start + r[:, None] * self.ld + torch.arange(self.cols)[None, :]).reshape(-1).cuda()

    def untouched_except(self, idx=None):
        keep = torch.ones(self.flat.numel(), dtype=torch.bool, device="cuda")
        if idx is not None:
            keep[idx] = False
        return bool((self.flat.view(torch.int32)[keep] == SENT_BITS).all())


def vec_in(v):
    return Buf(1, v.numel(), v.numel(), values=v[None, :])


def scattered(t, rowmap, out_rows):
    """a [M, N] tensor in GEMM-row order placed at its output rows; every other row NaN"""
    full = torch.full((out_rows, t.shape[1]), G.NAN)
    full[rowmap] = t
    return full


def run_nt(L, c, x, tune=None, repeat=True):
    """launches the case -> {"C", "pre", "colstats", "bstats"} on the CPU in GEMM-row order, after the sentinel / ticket checks"""
    g, e = c.g, c.epi
    tune = c.tune if tune is None else tune
    rowmap, out_rows = G.row_map(c)
    A = Buf(c.nb * g.H * g.W, c.C, c.lda, off=int("A" in c.off), values=x["A"].reshape(-1, c.C))
    W = Buf(c.N, c.K, c.ldb, off=int("W" in c.off), values=x["W"])
    C = Buf(out_rows, c.N, c.ldc, off=int("C" in c.off), fill=G.SENT)
    vecs = {n: (vec_in(x[n]) if n in e else None) for n in ("bias", "sub", "scale", "shift", "scale_var")}
    resid = Buf(out_rows, c.N, c.ldr, values=scattered(x["resid"], rowmap, out_rows)) if "resid" in e else None
    mask = Buf(out_rows, c.N, c.ldm, values=scattered(x["relu_mask"], rowmap, out_rows)) if "relu_mask" in e else None
    pre = Buf(out_rows, c.N, c.ldc, fill=G.SENT) if "pre" in e else None
    a_bn = Buf(4, c.C, c.C, values=x["a_bn"]) if "a_bn" in e else None
    nst, nbt = 2 * G.cdiv(c.M, G.nt_stat_rows(c)), 2 * G.cdiv(c.M, 64)
    cst = Buf(nst, c.N, c.N, fill=G.SENT) if "colstats" in e else None
    bs_y = Buf(out_rows, c.N, c.ldc, values=scattered(x["bs_y"], rowmap, out_rows)) if "bstats" in e else None
    bs_st = Buf(4, c.N, c.N, values=x["bs_stats"]) if "bstats" in e else None
    bst = Buf(2 * c.bs_tile0 + nbt, c.N, c.N, fill=G.SENT) if "bstats" in e else None
    P = lambda b: None if b is None else b.ptr
    cfg = L.gemm_nt_config(A.ptr, W.ptr, c.M, c.N, c.K, c.lda, c.ldb, c.C, g.KH, g.KW, int(G.is_plain(g)), int("a_bn" in e), tune)
    assert cfg == c.code or tune != c.tune, f"{c.name}: the launch takes {cfg}, the table says {c.code}"
    ws, ws_ptr, ws_bytes = None, None, 0
    old = L.gemm_nt_force_splits(c.force or 0)
    try:
        if c.force is not None:
            ws_bytes = L.gemm_nt_split_workspace_bytes(c.M, c.N, c.K, tune)
            assert ws_bytes == 16384 + G.cdiv(c.M, 64) * G.cdiv(c.N, 64) * c.splits * 16384
            ws = torch.full((2 * MARGIN + ws_bytes // 4,), G.NAN, dtype=torch.float32, device="cuda")   # the slabs hold NaN: written before read
            ws[:MARGIN] = G.SENT
            ws[-MARGIN:] = G.SENT
            ws[MARGIN:MARGIN + 4096].view(torch.int32).zero_()                                            # the tickets, zeroed ONCE
            ws_ptr = ws.data_ptr() + 4 * MARGIN
            assert ws_ptr % 256 == 0

        def launch():
            L.gemm_nt(A.ptr, W.ptr, C.ptr, c.M, c.N, c.K, c.lda, c.ldb, c.ldc, g.H, g.W, c.C, g.OH, g.OW, g.KH, g.KW, g.stride, g.pad_y, g.pad_x,
                      g.mode, g.os, g.opy, g.opx, g.oOH, g.oOW, P(vecs["bias"]), P(vecs["sub"]), P(vecs["scale"]), P(vecs["shift"]), P(resid), c.ldr,
                      P(pre), c.act, c.alpha, P(cst), P(a_bn), P(mask), c.ldm, P(bs_y), P(bs_st), P(bst), c.bs_relu, c.bs_tile0,
                      P(vecs["scale_var"]), c.var_eps, ws_ptr, ws_bytes, tune, _st())
            torch.cuda.synchronize()
        launch()
        outs = [b for b in (C, pre, cst, bst) if b is not None]
        first = [b.flat.clone() for b in outs]
        if ws is not None:
            assert bool((ws[MARGIN:MARGIN + 4096].view(torch.int32) == 0).all()), "split-K left a ticket word non-zero"
            assert bool((ws[:MARGIN].view(torch.int32) == SENT_BITS).all() and (ws[-MARGIN:].view(torch.int32) == SENT_BITS).all()), "wrote past the split workspace"
            if repeat:
                launch()
                assert all(torch.equal(b.flat.view(torch.int32), f.view(torch.int32)) for b, f in zip(outs, first)), \
                    "a second launch with the same split workspace gave other bits"
                assert bool((ws[MARGIN:MARGIN + 4096].view(torch.int32) == 0).all())
    finally:
        L.gemm_nt_force_splits(old)
    rm = rowmap.cuda()
    got = {"C": C.view[rm].cpu()}
    assert C.untouched_except(C.index(rowmap)), "C written outside its [rows, N] elements (ldc gap, a skipped row or a margin)"
    if pre is not None:
        got["pre"] = pre.view[rm].cpu()
        assert pre.untouched_except(pre.index(rowmap)), "pre written outside its [rows, N] elements"
    if cst is not None:
        got["colstats"] = cst.view.cpu()
        assert cst.untouched_except(cst.index()), "colstats written past its last tile"
    if bst is not None:
        got["bstats"] = bst.view[2 * c.bs_tile0:].cpu()
        assert bst.untouched_except(bst.index(torch.arange(2 * c.bs_tile0, 2 * c.bs_tile0 + nbt))), "bstats written before bs_tile0 or past the last tile"
    return got


@pytest.mark.parametrize("name", [c.name for c in G.NT_CASES])
def test_gemm_nt_instantiations_against_float64(L, bounds, name):
    c = G.NT_BY_NAME[name]
    x, ref = G.reference(c)
    got = run_nt(L, c, x)
    if name in G.B3_CASES:      # split precision: relative L2 from float64 within 1.25 x the fp32-exact kernel's on the same operands
        e3 = G.rel_l2(got["C"], ref["C"])
        e32 = G.rel_l2(run_nt(L, c, x, tune=c.tune - 100000)["C"], ref["C"])
        print(f"GEMM_ERR b3 {c.name} {G.nt_kernel(c.code)} rel-L2 {e3:.3e} fp32-exact {e32:.3e}")
        assert e3 <= 1.25 * e32 + 1e-8 and e3 < 5e-7, f"split precision {e3:.2e} from float64, fp32-exact chain {e32:.2e}"
        G.check_nt(c, got, ref, bounds[c.family])          # printed only: the rule above is the B3 kernels' bound
        assert not any(bool(torch.isnan(v).any()) for v in got.values())
        return
    bad = G.check_nt(c, got, ref, bounds[c.family])
    assert not bad, f"{c.name} ({G.nt_kernel(c.code)}): beyond {bounds[c.family]:.3e} of float64: {bad}"


@pytest.mark.parametrize("a,b,what", G.NT_EXACT, ids=[f"{a}-{b}" for a, b, _ in G.NT_EXACT])
def test_documented_exact_relations_hold_bit_for_bit(L, a, b, what):
    """two instantiations documented to share their k order and sums, on the same operands: C and `pre` bit for bit (the tile
    statistics too between the two epilogues of the 64x64 tile; the lean kernel's agree to rounding and are checked against
    float64 above).  In addition to the float64 comparison of each, not in place of it."""
    ca, cb = G.NT_BY_NAME[a], G.NT_BY_NAME[b]
    assert ca.base == cb.base and ca.tune != cb.tune
    x, _ = G.reference(ca)
    ga, gb = run_nt(L, ca, x, repeat=False), run_nt(L, cb, x, repeat=False)
    keys = [k for k in ga if k != "colstats" or "epilogue" in what]
    for k in keys:
        assert torch.equal(ga[k].view(torch.int32), gb[k].view(torch.int32)), f"{what}: {k} of {a} and {b} differ"


def run_wg(L, c, x):
    g = c.g
    dY = Buf(c.M, c.N, c.ldy, off=int("dY" in c.off), values=x["dY"])
    X = Buf(c.nb * g.H * g.W, c.C, c.ldx, off=int("X" in c.off), values=x["X"].reshape(-1, c.C))
    xbn = Buf(4, c.C, c.C, values=x["x_bn"]) if c.x_bn else None
    dW = Buf(c.N, c.Kdst, c.Kdst, fill=G.SENT, extra=0)
    if c.accumulate:
        dW.view.copy_(x["init"])
    old = L.wgrad_force_splits(c.force)
    try:
        assert L.wgrad_splits(c.M, c.N, c.K, c.tune) == c.splits
        nbytes = L.wgrad_workspace_bytes(c.M, c.N, c.K, c.tune)
        assert nbytes == c.splits * c.N * c.K * 4
        ws = Buf(c.splits, c.N * c.K, c.N * c.K, off=int("ws" in c.off), extra=0)       # NaN: every slab is written before it is read
        ws.flat[:MARGIN] = G.SENT
        ws.flat[-MARGIN:] = G.SENT
        assert L.wgrad_config(dY.ptr, X.ptr, c.M, c.N, c.K, c.ldy, c.ldx, c.C, g.KH, g.KW, int(c.x_bn), ws.ptr, c.tune) == c.code
        geo = (g.H, g.W, c.C, g.OH, g.OW, g.KH, g.KW, g.stride, g.pad_y)
        if c.partial:
            L.wgrad_tn_partial(dY.ptr, X.ptr, c.M, c.N, c.K, c.ldy, c.ldx, *geo, None if xbn is None else xbn.ptr, ws.ptr, nbytes, c.tune, _st())
        else:
            L.wgrad_tn(dY.ptr, X.ptr, dW.ptr, c.M, c.N, c.K, c.ldy, c.ldx, *geo, c.Kdst, c.accumulate, None if xbn is None else xbn.ptr,
                       ws.ptr, nbytes, c.tune, _st())
        torch.cuda.synchronize()
    finally:
        L.wgrad_force_splits(old)
    slabs = ws.view.cpu().view(c.splits, c.N, c.K)
    for z, (b, e) in enumerate(G.wg_slabs(c)):
        if b == e:
            assert bool((slabs[z].view(torch.int32) == 0).all()), f"slab {z} owns no rows and must hold exact zeros"
    assert bool((ws.flat[:MARGIN].view(torch.int32) == SENT_BITS).all() and (ws.flat[-MARGIN:].view(torch.int32) == SENT_BITS).all()), "wrote past the workspace"
    if c.partial:
        assert dW.untouched_except(None), "stil_wgrad_tn_partial wrote a destination"
        return {"P": slabs.double().sum(0)}
    assert dW.untouched_except(dW.index()), "dW written outside its [N, Kdst] elements"
    return {"dW": dW.view.cpu()}


@pytest.mark.parametrize("name", [c.name for c in G.WG_CASES])
def test_wgrad_instantiations_against_float64(L, bounds, name):
    c = G.WG_BY_NAME[name]
    x, ref = G.reference(c)
    got = run_wg(L, c, x)
    bad = G.check_wg(c, got, ref, bounds["wgrad"], keys=tuple(got))
    assert not bad, f"{c.name} ({G.wg_kernel(c.code)}): beyond {bounds['wgrad']:.3e} of float64: {bad}"


def test_the_tables_cover_every_reachable_instantiation():
    """the condition tests/test_gemm_cases_cpu.py proves on the host, restated where the launches happen (each case above asserts
    its own CONFIG code on the real operands)"""
    assert G.nt_coverage_gaps(G.NT_CASES) == [] and G.wg_coverage_gaps(G.WG_CASES) == []
