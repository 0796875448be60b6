"""The cases of tests/tabular_cases.py on the host: what the list reaches (computed from the case data), that fp32 with the
kernels' own summation order meets the suite's tolerance against the float64 definitions on every case (no ill-conditioned
input), that the comparison rejects what a subtly wrong kernel would produce, and the argument checks of the six entry points
and of SaintEmbedColMlpFn, which refuse before any launch.  No GPU: only refused argument combinations are passed to the entry
points, with addresses nothing dereferences -- which is why these live here and not in the GPU module, where a missed refusal
would be a wild store."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tabular_cases as T  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402  (the suite's tolerance and comparison, unchanged)

BASE = 1 << 20


def fake(off=0):
    return ctypes.c_void_p(BASE + 4 * off)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as E
    E.build()
    from stil_tta_amd._lib import lib
    return lib()


def rejected(a, b, name=""):
    try:
        close(a, b, name=name)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------- coverage
def test_the_case_list_reaches_every_property_by_construction():
    assert T.coverage_gaps() == []
    assert {T.mlp_ne(c) for c in T.MLP_CASES if c.bwd} == set(range(1, T.MAXE + 1))
    assert {(c.d, c.hid) for c in T.MLP_CASES} >= {(32, 100), (16, 256), (256, 16), (40, 100), (33, 7), (1, 1), (64, 200)}
    assert [c.name for c in T.MLP_CASES if not c.bwd] == ["fwd_only_64x200"] and 64 * 200 > T.MAXE * T.BLOCK
    assert {c.B for c in T.MLP_CASES if (c.d, c.hid) == (32, 100)} == {1, 12, 257}
    assert {c.D for c in T.TAB_CASES} == {1, 48, 64, 260, 512} and {c.B for c in T.TAB_CASES} == {1, 9, 300}
    assert {(len(c.cards), c.d, c.B) for c in T.SAINT_CASES} == {(n, d, B) for n in (0, 1, 5) for d in (8, 32, 72) for B in (1, 12, 257)}
    assert len(T.RUNS) == 2 * sum(len(cs) for cs in T.CASES.values()) == 2 * len(T.BY_NAME)
    # the check can fail: each property goes missing with the cases that carry it
    drop = lambda pred: [r for r in T.RUNS if not pred(r[0], T.BY_NAME[r[0], r[1]], r[2])]
    assert ("mlp", "ne=7") in T.coverage_gaps(drop(lambda f, c, a: f == "mlp" and T.mlp_ne(c) == 7))
    assert ("mlp", "ne=16 with d=256") in T.coverage_gaps(drop(lambda f, c, a: f == "mlp" and c.d == 256))
    assert ("mlp", "ne=16 with hid=256") in T.coverage_gaps(drop(lambda f, c, a: f == "mlp" and c.hid == 256))
    assert ("mlp", "ragged last group") in T.coverage_gaps(drop(lambda f, c, a: f == "mlp" and (c.d, c.hid) == (40, 100)))
    assert ("tab", "D>256") in T.coverage_gaps(drop(lambda f, c, a: f == "tab" and c.D > 256))
    assert ("tab", "partial last 64-thread block") in T.coverage_gaps(drop(lambda f, c, a: f == "tab" and c.D == 260))
    assert ("saint", "d>64") in T.coverage_gaps(drop(lambda f, c, a: f == "saint" and c.d == 72))
    assert ("tab", "layout con") in T.coverage_gaps(drop(lambda f, c, a: f == "tab" and not c.cards))
    assert ("saint", "ncat=0") in T.coverage_gaps(drop(lambda f, c, a: f == "saint" and not c.cards))
    assert ("saint", "accumulate=1") in T.coverage_gaps(drop(lambda f, c, a: f == "saint" and a == 1 and c.B == 12))
    assert ("mlp", "B=1") in T.coverage_gaps(drop(lambda f, c, a: f == "mlp" and c.B == 1))


def test_the_input_edges_are_in_the_data():
    for c in T.TAB_CASES:
        x = T.tab_inputs(c)
        ncat = len(c.cards)
        if c.ncon:
            assert float(x["x"][0, ncat]) == 0.0                                           # an exact zero continuous value
        if ncat:
            code = x["x"][:, :ncat].long()
            assert 1 in c.cards and any(card >= 4 for card in c.cards) and 3 in c.cards
            assert int(code.min()) >= 0 and bool((code < torch.tensor(c.cards)).all())     # never a code outside its column
            hole = next(j for j, card in enumerate(c.cards) if card >= 4)
            assert int(x["offs"][hole]) + 2 in T.undrawn_rows(x, False)                    # a row no sample draws
            same = c.cards.index(3)
            assert code[:, same].unique().tolist() == [1]                                  # every sample on one code
    for c in T.SAINT_CASES:
        x = T.saint_inputs(c)
        ncat = len(c.cards)
        code = x["x"][:, x["cat_cols"].long()].long()
        assert x["pos"].shape[0] >= ncat + 1 and x["emb"].shape[0] == 1 + sum(c.cards)
        assert not ncat or (int(code.min()) >= 0 and bool((code < torch.tensor(c.cards)).all()))
        if ncat:
            hole = next(j for j, card in enumerate(c.cards) if card >= 4)
            assert int(x["offs"][1 + hole]) + 2 in T.undrawn_rows(x, True)
            cols = sorted(x["cat_cols"].tolist() + x["con_cols"].tolist())
            assert cols == list(range(ncat + c.ncon)) and x["cat_cols"].tolist() != list(range(ncat))   # interleaved
        if ncat == 5:
            assert code[:, c.cards.index(3)].unique().tolist() == [1] and 1 in c.cards
    assert T.interleave(4, 3) == ([1, 2, 4, 6], [0, 3, 5])
    for c in T.MLP_CASES:
        x = T.mlp_inputs(c)
        if c.edges:
            zero, dead, live = T.relu_units(c, x)
            assert zero >= 1 and dead >= 1 and live >= 1, c.name
        # the written-out float64 gradients are the autograd ones: exactly-zero pre-activations get gradient 0, as ATen's do
        ref, man = T.mlp_reference(c), T.mlp_manual_grads(c, x)
        for name, a, b in T.pairs(man, ref):
            assert T.ratio(a, b, TOL) < 1e-6, (c.name, name)


# ------------------------------------------------------------------------------------------------------------ yardstick
# fp32 in the kernels' order against float64, worst error over close()'s allowance per family, as measured when the cases
# were written (DESIGN.md section 2 quotes them).  They only catch a drift of the yardstick itself; the bound is TOL.
RECORDED = {"tab": 0.026, "saint": 0.019, "mlp": 0.022}
DRIFT = 3.0


def test_fp32_in_batch_order_meets_the_tolerance_on_every_case():
    worst = {}
    for f, cases in T.CASES.items():
        worst[f] = (0.0, "")
        for c in cases:
            got, ref = T.SEQ32[f](c), T.REFERENCE[f](c)
            for name, a, b in T.pairs(got, ref):
                if name != "out" and not getattr(c, "bwd", True):
                    continue
                close(a, b, name=f"{f}/{c.name}/{name}")              # a failure here: change the case, never the tolerance
                worst[f] = max(worst[f], (T.ratio(a, b, TOL), f"{c.name}/{name}"))
            assert set(got) == set(ref), (f, c.name)
    print("TABULAR_YARDSTICK fp32 in batch order vs float64, worst error / allowance:", {f: f"{r:.3f} ({n})" for f, (r, n) in worst.items()})
    for f, (r, _) in worst.items():
        assert 0.0 < r < 1.0
        assert RECORDED[f] / DRIFT <= r <= RECORDED[f] * DRIFT, f"the {f} yardstick drifted: {r:.4f}, recorded {RECORDED[f]:.4f}"


# --------------------------------------------------------------------------------------------------- the check can fail
@pytest.mark.parametrize("family,bug", [("tab", "row_dropped"), ("saint", "row_dropped"), ("tab", "offsets_swapped"), ("saint", "offsets_swapped"),
                                        ("mlp", "relu_ge"), ("mlp", "tok0_off_by_one")])
def test_a_subtly_wrong_kernel_is_rejected(family, bug):
    caught, tried = [], 0
    for c in T.CASES[family]:
        bad, ref = T.broken(family, c, bug), T.REFERENCE[family](c)
        if bad is None:
            continue
        tried += 1
        if any(rejected(a, b) for _, a, b in T.pairs(bad, ref)):
            caught.append(c.name)
    assert tried and caught, (family, bug)
    if bug == "relu_ge":
        assert set(caught) == {c.name for c in T.MLP_CASES if c.bwd and c.edges}    # exactly the cases that hold a zero pre-activation
    else:
        assert len(caught) == tried                                               # these defects show on every case they apply to


@pytest.mark.parametrize("family", list(T.CASES))
def test_an_ignored_accumulate_flag_is_rejected(family):
    for c in T.CASES[family]:
        if not getattr(c, "bwd", True):
            continue
        x, ref = T.INPUTS[family](c), T.REFERENCE[family](c)
        grads = {k: v for k, v in ref.items() if k != "out"}
        # accumulate = 1 asked, the kernel overwrote: every gradient misses its prefill
        assert all(rejected(a, b) for _, a, b in T.pairs(grads, grads, pre=x)), c.name
        # accumulate = 0 asked, the kernel added to what was there
        added = {k: ([p.double() + t for p, t in zip(x["pre_" + k], v)] if isinstance(v, list) else x["pre_" + k].double() + v) for k, v in grads.items()}
        assert all(rejected(a, b) for _, a, b in T.pairs(added, grads)), c.name


# ------------------------------------------------------------------------------------------------------------- refusals
def _tab_bwd(L, ncat, ncon, D=8, rowcol=True, offs=True, d_emb=True, d_con_w=True, d_con_b=True, ws_short=0):
    ncols = ncat + ncon
    nb = L.tab_embed_bwd_workspace_bytes(ncols, D)
    assert nb == 2 * (ncols + 1) * D * 4
    f = lambda on: fake() if on else None
    L.tab_embed_bwd(fake(), fake(), f(offs), f(rowcol), 3 * ncat, f(d_emb), f(d_con_w), f(d_con_b), fake(), fake(), 4, ncols, ncat, D, 1,
                    fake(), nb - ws_short, None)


def test_argument_checks_refuse_before_any_launch(L):
    """every call below would launch with wild addresses if its check were missing or came after a launch; on a host without
    a device that shows as a launch error in place of the entry point's own message"""
    for kw in (dict(d_con_w=False), dict(d_con_b=False)):
        with pytest.raises(RuntimeError, match="stil_tab_embed_bwd: null continuous pointers"):
            _tab_bwd(L, 2, 1, **kw)
        with pytest.raises(RuntimeError, match="stil_tab_embed_bwd: null continuous pointers"):
            _tab_bwd(L, 0, 2, **kw)
    for kw in (dict(rowcol=False), dict(offs=False), dict(d_emb=False)):
        with pytest.raises(RuntimeError, match="stil_tab_embed_bwd: null categorical pointers"):
            _tab_bwd(L, 2, 1, **kw)
        with pytest.raises(RuntimeError, match="stil_tab_embed_bwd: null categorical pointers"):
            _tab_bwd(L, 2, 0, d_con_w=False, d_con_b=False, **kw)              # cat-only: the continuous pointers may be NULL
    with pytest.raises(RuntimeError, match="stil_tab_embed_bwd: workspace too small"):
        _tab_bwd(L, 2, 1, ws_short=4)
    with pytest.raises(RuntimeError, match="stil_tab_embed_bwd: null pointer"):
        L.tab_embed_bwd(fake(), fake(), fake(), fake(), 6, fake(), fake(), fake(), None, fake(), 4, 3, 2, 8, 0, fake(), 1 << 20, None)
    with pytest.raises(RuntimeError, match="stil_tab_embed_fwd: null pointer"):
        L.tab_embed_fwd(fake(), fake(), fake(), None, fake(), fake(), fake(), fake(), 4, 3, 2, 8, None)
    with pytest.raises(RuntimeError, match="stil_saint_embed_bwd: null pointer"):
        L.saint_embed_bwd(fake(), fake(), None, fake(), fake(), 7, fake(), fake(), 4, 5, 2, 6, 8, 1, None)      # NULL cat_cols, ncat = 2
    with pytest.raises(RuntimeError, match="stil_saint_embed_fwd: null pointer"):
        L.saint_embed_fwd(fake(), None, fake(), fake(), fake(), fake(), 4, 5, 2, 6, 8, None)
    mlp_bwd = lambda d, hid, ncon=2: L.colmlp_bwd(fake(), fake(), fake(), fake(), fake(), 4, 5, ncon, 6, 3, hid, d, 1, None)
    mlp_fwd = lambda d, hid, ncon=2: L.colmlp_fwd(fake(), fake(), fake(), fake(), 4, 5, ncon, 6, 3, hid, d, None)
    for d, hid in ((32, 129), (1, 257), (257, 1)):                 # d * hid > 4096, hid > 256, d > 256: each bound on its own
        with pytest.raises(RuntimeError, match=rf"stil_colmlp_bwd: hidden {hid} x dim {d} too large"):
            mlp_bwd(d, hid)
    with pytest.raises(RuntimeError, match="stil_colmlp_bwd: hidden 200 x dim 64 too large"):
        mlp_bwd(64, 200)                                           # the forward-only case of the GPU module
    with pytest.raises(RuntimeError, match="stil_colmlp_fwd: hidden 128 x dim 128 does not fit LDS"):
        mlp_fwd(128, 128)
    assert (64 * 200 + 2 * 200 + 64) * 4 <= 60 * 1024 < (128 * 128 + 2 * 128 + 128) * 4      # ... which the forward does take
    with pytest.raises(RuntimeError, match="stil_colmlp_fwd: bad arguments"):
        mlp_fwd(32, 100, ncon=0)
    with pytest.raises(RuntimeError, match="stil_colmlp_bwd: bad arguments"):
        mlp_bwd(32, 100, ncon=0)


def test_saint_embedding_refuses_a_positional_table_without_a_row_per_token(monkeypatch):
    """pos_encodings has ncat + ncon rows, the kernels touch rows 0..ncat: with no continuous column that is one row too many"""
    from stil_tta_amd import ops

    def touched():
        raise AssertionError("lib() was reached: the refusal has to come before any launch")

    monkeypatch.setattr(ops, "lib", touched)
    ncat, d = 3, 8
    meta = dict(ncat=ncat, ncon=0, hid=100, cat_cols=None, con_cols=None, offs=None, rowcol=None)
    for device in ("cpu", "meta"):
        x, emb, pos = (torch.zeros(s, device=device) for s in ((4, ncat), (7, d), (ncat, d)))
        with pytest.raises(RuntimeError, match=rf"pos has {ncat} rows.*ncat \+ 1 = {ncat + 1}"):
            ops.SaintEmbedColMlpFn.apply(x, emb, pos, meta)
    # one more row passes this check and stops at the next one (these are no device tensors), still before lib()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.SaintEmbedColMlpFn.apply(torch.zeros(4, ncat), torch.zeros(7, d), torch.zeros(ncat + 1, d), meta)
