"""The case tables of tests/gemm_cases.py on the host: every case's CONFIG code from `stil_gemm_nt_config` / `stil_wgrad_config`,
its splits, slabs and column panels from the library's own queries, the coverage condition (every reachable instantiation in
every orientation) and that the condition can fail, the argument checks that refuse before any launch, and the yardsticks of
tests/test_gpu_gemm.py: fp32 ATen through the same check functions.  No GPU: the queries make no GPU call and only refused
argument combinations are passed to the entry points, with addresses nothing dereferences."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as G  # noqa: E402

BASE = 1 << 20                     # a fake, 256-byte aligned address


def fake(off=0):
    return ctypes.c_void_p(BASE + 4 * off)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as E
    E.build()
    from stil_tta_amd._lib import lib
    return lib()


def nt_config(L, c):
    g = c.g
    return L.gemm_nt_config(fake("A" in c.off), fake("W" in c.off), c.M, c.N, c.K, c.lda, c.ldb, c.C, g.KH, g.KW, int(G.is_plain(g)),
                            int("a_bn" in c.epi), c.tune)


def wg_config(L, c):
    g = c.g
    return L.wgrad_config(fake("dY" in c.off), fake("X" in c.off), c.M, c.N, c.K, c.ldy, c.ldx, c.C, g.KH, g.KW, int(c.x_bn),
                          fake("ws" in c.off), c.tune)


def test_every_case_reports_the_code_its_table_names(L):
    got = {c.name: nt_config(L, c) for c in G.NT_CASES}
    assert got == {c.name: c.code for c in G.NT_CASES}
    got = {c.name: wg_config(L, c) for c in G.WG_CASES}
    assert got == {c.name: c.code for c in G.WG_CASES}
    # every code of the tables is one the launchers can reach, and the reachable set is the size the launchers spell out
    assert {G.nt_kernel(c.code) for c in G.NT_CASES} <= set(G.NT_KERNELS) and len(G.NT_KERNELS) == 60 and len(G.NT_REACHABLE) == 60
    assert {G.wg_kernel(c.code) for c in G.WG_CASES} <= set(G.WG_KERNELS) and len(G.WG_KERNELS) == 9
    # the queries refuse what the entry points refuse
    assert L.wgrad_config(fake(1), fake(), 32, 8, 8, 8, 8, 8, 1, 1, 1, fake(), 0) < 0          # x_bn without 16-byte operands
    assert L.wgrad_config(fake(), fake(), 32, 8, 8, 8, 8, 8, 1, 1, 0, fake(), 21) < 0         # a tile the weight gradient does not have


def test_splits_slabs_and_panels_are_what_the_cases_claim(L):
    for c in G.NT_CASES:
        assert L.gemm_nt_panel(c.M, c.N, c.K) == c.panel, c.name
        if c.force is None:
            assert c.splits == 1
            continue
        old = L.gemm_nt_force_splits(c.force)
        try:
            nbytes = L.gemm_nt_split_workspace_bytes(c.M, c.N, c.K, c.tune)
        finally:
            L.gemm_nt_force_splits(old)
        tiles = G.cdiv(c.M, 64) * G.cdiv(c.N, 64)
        assert c.splits > 1 and nbytes == 16384 + tiles * c.splits * 4096 * 4, (c.name, nbytes)
    assert L.gemm_nt_force_splits(0) == 0
    assert sum(c.panel > 0 for c in G.NT_CASES) >= 2 and G.NT_BY_NAME["big_wide544_colstats"].panel == 4
    assert 1024 * 544 * 4 > 2 << 20 and G.NT_BY_NAME["narrow_no_panel"].panel == 0
    for c in G.WG_CASES:
        old = L.wgrad_force_splits(c.force)
        try:
            assert L.wgrad_splits(c.M, c.N, c.K, c.tune) == c.splits, c.name
            assert L.wgrad_workspace_bytes(c.M, c.N, c.K, c.tune) == c.splits * c.N * c.K * 4
        finally:
            L.wgrad_force_splits(old)
    assert L.wgrad_force_splits(0) == 0


def test_slice_and_slab_arithmetic_of_the_forced_splits():
    """kpt in gemm_nt_kernel: ceil(k-tiles / slices) rounded up to whole 64-product chains; m_per_split in wgrad_tn_impl"""
    s = {n: G.nt_slices(G.NT_BY_NAME[n])[0] for n in G.NT_BY_NAME if G.NT_BY_NAME[n].splits > 1}
    assert s["split544_force2"] == [(0, 10), (10, 17)] and s["split544_force3"] == [(0, 6), (6, 12), (12, 17)]
    assert s["split544_force7"] == [(0, 4), (4, 8), (8, 12), (12, 16), (16, 17), (17, 17), (17, 17)]
    assert s["split544_force8"] == s["split544_force7"] + [(17, 17)]
    assert s["split544_bk16_force7"] == [(0, 8), (8, 16), (16, 24), (24, 32), (32, 34), (34, 34), (34, 34)]
    assert s["split286_scalar_force2"] == [(0, 12), (12, 18)] and s["split286_scalar_force3"] == [(0, 8), (8, 16), (16, 18)]
    assert s["split272_abn_force3"] == [(0, 8), (8, 16), (16, 17)]
    for n, sl in s.items():
        lens = [e - b for b, e in sl]
        assert sum(lens) == sl[-1][1] and lens[0] > 0, n
        if "force" in n:
            assert min(v for v in lens if v) < lens[0], f"{n}: no short last slice"
    sl, per_tap = G.nt_slices(G.NT_BY_NAME["split_conv48_force2"])
    assert sl == [(0, 16), (16, 27)] and per_tap == 3 and 16 % per_tap != 0            # the boundary falls inside tap 5
    w = {c.name: G.wg_slabs(c) for c in G.WG_CASES}
    assert w["slab100_force5"] == [(0, 32), (32, 64), (64, 96), (96, 100), (128, 128)]
    assert w["slab100_force6"] == w["slab100_force5"] + [(160, 160)] and 16 * 2 * (6 - 1) >= 100
    assert w["slab100_force2"] == [(0, 64), (64, 100)] and w["slab9_force5"] == [(0, 9)]
    assert w["slab_policy5"] == [(0, 272), (272, 544), (544, 816), (816, 1088), (1088, 1300)]
    assert w["slab_grid3x3_force2"] == [(0, 32), (32, 45)] and 32 % 9 != 0               # slab 1 starts inside an image


def test_every_reachable_instantiation_is_covered_in_every_orientation():
    assert G.nt_coverage_gaps(G.NT_CASES) == []
    assert G.wg_coverage_gaps(G.WG_CASES) == []
    # the check can fail: without the ragged cases it reports gaps, and it names a kernel nothing launches
    dull = [c for c in G.NT_CASES if not ({"M%tile", "N%tile", "Ktail"} & G.nt_tags(c))]
    gaps = G.nt_coverage_gaps(dull)
    assert len(gaps) > 50 and any(t == "M%tile" for _, t in gaps) and any(t == "reached" for _, t in gaps)
    assert ("shape", "M=1") in G.nt_coverage_gaps([c for c in G.NT_CASES if c.M > 1])
    assert ("gather", "dgrad2") in G.nt_coverage_gaps([c for c in G.NT_CASES if c.geom != "dgrad2"])
    wgaps = G.wg_coverage_gaps([c for c in G.WG_CASES if c.M % 16 == 0 or c.N % 64 == 0])
    assert any(t == "M%16" for _, t in wgaps)
    assert ("slabs", "empty slab") in G.wg_coverage_gaps([c for c in G.WG_CASES if not c.force])
    assert ("wgrad_reduce_kernel", "taps>1") in G.wg_coverage_gaps([c for c in G.WG_CASES if "ws" not in c.off])
    # epilogue: every operand singly and all together on each of the five tile / epilogue forms; statistics on the tiles that admit them
    for tile in ("11w", "11s", "12", "21", "22"):
        names = {c.name for c in G.NT_CASES if c.name.startswith(f"epi{tile}_")}
        assert len(names) == 13, (tile, sorted(names))
        assert f"colstats{tile}" in G.NT_BY_NAME
    assert {c.bs_relu for c in G.NT_CASES if "bstats" in c.epi} == {0, 2} and any(c.bs_tile0 > 0 for c in G.NT_CASES if "bstats" in c.epi)
    for c in G.NT_CASES:
        assert c.ldr != c.ldc and c.ldm != c.ldc
    # under a split: scalar loads, a_bn, colstats, bstats, a convolution; forced 2, 3, 7, 8 and the policy
    split = [c for c in G.NT_CASES if c.splits > 1]
    assert {c.force for c in split} >= {0, 2, 3, 7, 8}
    assert any(not G.nt_decode(c.code).vec for c in split) and any("a_bn" in c.epi for c in split) and any("colstats" in c.epi for c in split)
    assert any("bstats" in c.epi for c in split) and any(c.geom != "plain" for c in split)


def _gemm_nt(L, M, N, K, geom, tune, a_bn=None, bstats=None, A=None):
    """stil_gemm_nt on fake addresses: only for argument combinations the entry point refuses before its first launch"""
    bs = (fake(), fake(), fake(), 0, 0) if bstats else (None, None, None, 0, 0)
    L.gemm_nt(A or fake(), fake(), fake(), M, N, K, geom[2], K, N, *geom, 1, 0, 0, geom[3], geom[4], None, None, None, None, None, 0, None, 0,
              1.0, None, a_bn, None, 0, *bs, None, 0.0, None, 0, tune, None)


def test_argument_checks_refuse_before_any_launch(L):
    plain = lambda C: (1, 1, C, 1, 1, 1, 1, 1, 0, 0, 0)
    with pytest.raises(RuntimeError, match="bstats needs"):
        _gemm_nt(L, 128, 64, 48, plain(48), 21, bstats=True)                          # bstats on a 128-row tile
    with pytest.raises(RuntimeError, match="bstats needs"):
        _gemm_nt(L, 128, 64, 48, plain(48), 10011, bstats=True)                       # ... and on the scalar epilogue
    with pytest.raises(RuntimeError, match="a_bn runs 64x64"):
        _gemm_nt(L, 128, 64, 40, plain(40), 0, a_bn=fake())                           # a_bn with Cin % 16 != 0
    with pytest.raises(RuntimeError, match="a_bn runs 64x64"):
        _gemm_nt(L, 128, 64, 48, plain(48), 21, a_bn=fake())                          # a_bn on another tile
    with pytest.raises(RuntimeError, match="a_bn runs 64x64"):
        _gemm_nt(L, 128, 64, 48, plain(48), 0, a_bn=fake(), A=fake(1))                # a_bn without 16-byte operands
    with pytest.raises(RuntimeError, match=r"Cin % 16 == 0"):
        _gemm_nt(L, 50, 64, 9 * 8, (5, 5, 8, 5, 5, 3, 3, 1, 1, 1, 0), 0)              # implicit-GEMM convolution with Cin % 16 != 0
    wg = lambda dY, ws_bytes, x_bn: L.wgrad_tn(dY, fake(), fake(), 100, 36, 40, 36, 40, 1, 1, 40, 1, 1, 1, 1, 1, 0, 40, 0, x_bn,
                                                        fake(), ws_bytes, 0, None)
    with pytest.raises(RuntimeError, match="x_bn needs 16-byte"):
        wg(fake(1), 1 << 20, fake())                                                  # x_bn without vector operands
    with pytest.raises(RuntimeError, match="workspace too small"):
        wg(fake(), 36 * 40 * 4 - 4, None)                                             # a short workspace
    old = L.wgrad_force_splits(5)
    try:
        with pytest.raises(RuntimeError, match="workspace too small"):
            wg(fake(), 4 * 36 * 40 * 4, None)                                         # ... four slabs where five are forced
        with pytest.raises(RuntimeError, match="workspace too small"):
            L.wgrad_tn_partial(fake(), fake(), 100, 36, 40, 36, 40, 1, 1, 40, 1, 1, 1, 1, 1, 0, None, fake(), 4 * 36 * 40 * 4, 0, None)
    finally:
        L.wgrad_force_splits(old)


# fp32 ATen against float64 per family, as measured when the tables were written, on two hosts (ATen's blocked sums depend on the
# thread count and the vector width: 3.52 / 4.38 / 3.71 / 5.73 / 3.82 / 3.02 e-7 on one, 3.52 / 3.63 / 2.79 / 3.58 / 3.82 / 6.28 e-7 on
# the other; recorded: their geometric means).  The bounds of the GPU module come from the figures measured at run time; these
# records only catch a drift of the yardstick itself, beyond the factor DRIFT either way.
RECORDED = {"plain": 3.52e-7, "gather": 3.99e-7, "split": 3.22e-7, "stats": 4.53e-7, "backward": 3.82e-7, "wgrad": 4.35e-7}
DRIFT = 3.0


def test_fp32_aten_passes_the_checks_of_the_gpu_module_and_the_yardsticks_hold():
    errs, bounds = G.aten_errors(), G.bounds()
    print("GEMM_YARDSTICK fp32 ATen vs float64:", {f: f"{e:.3e}" for f, e in errs.items()}, "kernel bounds:", {f: f"{b:.3e}" for f, b in bounds.items()})
    for f in G.FAMILIES:
        assert 0.0 < errs[f] < G.TOL, (f, errs[f])                       # no input here is ill-conditioned beyond the suite's tolerance
        assert bounds[f] == min(G.TOL, G.FACTOR * errs[f])
        assert RECORDED[f] / DRIFT <= errs[f] <= RECORDED[f] * DRIFT, f"the {f} yardstick drifted: {errs[f]:.3e}, recorded {RECORDED[f]:.3e}"
    # ATen itself through check_nt / check_wg on the same inputs: it passes its own family's bound (FACTOR >= 1), every output is there
    for c in G.NT_CASES:
        x, r64 = G.reference(c)
        r32 = G.nt_eval(c, x, torch.float32)
        assert set(r32) == set(r64) == {"C"} | ({"pre", "colstats", "bstats"} & set(c.epi))
        assert G.check_nt(c, r32, r64, bounds[c.family], tag="GEMM_ATEN") == [], c.name
    for c in G.WG_CASES:
        x, r64 = G.reference(c)
        assert G.check_wg(c, G.wg_eval(c, x, torch.float32), r64, bounds["wgrad"], keys=("dW", "P"), tag="GEMM_ATEN") == [], c.name
    # and the check functions can fail: a product with one k dropped is beyond every bound
    c = G.NT_BY_NAME["twin160_acc1_bkd0"]
    x, r64 = G.reference(c)
    x2 = dict(x, W=x["W"].clone())
    x2["W"][:, -1] = 0
    assert G.check_nt(c, G.nt_eval(c, x2, torch.float64), r64, bounds["plain"], tag="GEMM_SELFTEST") != []
    nan = {k: torch.full_like(v, G.NAN) for k, v in r64.items()}
    assert G.check_nt(c, nan, r64, bounds["plain"], tag="GEMM_SELFTEST") != []
