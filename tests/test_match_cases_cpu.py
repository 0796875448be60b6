"""CPU side of tests/test_gpu_match_kernels.py.  Conditioning: on every float case of tests/match_cases.py, fp32 ATen on the CPU
passes the very checks the GPU test applies to the kernels (the `check_*` functions of that module) against the float64
reference, and every float64 reference is finite.  Planted truths: top-1 leads top-2 and every maximum keeps off its threshold
by MIN_GAP in float64, planted ties are bit-equal in fp32, the entries at fp32(th) are edges and their neighbours below are
not.  Reach: both inf0 branches, a class without a bank entry, an edge with p < 1e-7, a gradient that is not zero, and the
widths 255 / 256 / 257 all occur.  Refusals: the four entry points turn down bad arguments before any launch -- only refused
argument combinations are passed, with addresses nothing dereferences, which is why they live here and not in the GPU module."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cases as M  # noqa: E402
import test_gpu_match_kernels as GM  # noqa: E402

BASE = 1 << 20


def fake(off=0):
    return ctypes.c_void_p(BASE + 4 * off)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as E
    E.build()
    from stil_tta_amd._lib import lib
    return lib()


def _finite(ref, keys):
    return all(bool(torch.isfinite(ref[k]).all()) for k in keys)


def _gap(p):
    t = p.double().topk(min(2, p.shape[1]), 1)[0]
    return t[:, 0] - t[:, 1] if p.shape[1] > 1 else torch.ones(len(p), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------------------
# stil_contrast_graph
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inv_rows", M.CONTRAST_INV_ROWS)
@pytest.mark.parametrize("rows,N", M.CONTRAST_TABLE)
def test_fp32_aten_meets_the_contrast_checks(rows, N, inv_rows):
    c = M.contrast_case(rows, N)
    inv = 1.0 / rows if inv_rows is None else inv_rows
    r64 = M.contrast_reference(c["S"], c["Q"], c["th"], inv, torch.float64)
    assert _finite(r64, ("row_loss", "dS"))
    GM.check_contrast(M.contrast_reference(c["S"], c["Q"], c["th"], inv, torch.float32), r64)
    assert float(r64["row_loss"].min()) >= -2e-7, "-sum(w log(p + 1e-7)) with p <= 1"


@pytest.mark.parametrize("rows,N", M.CONTRAST_TABLE)
def test_contrast_rows_hold_what_they_are_named_for(rows, N):
    c = M.contrast_case(rows, N)
    S, Q, th = c["S"], c["Q"], M.f32(c["th"])
    assert float(S.min()) >= -5.0 and float(S.max()) <= 5.0 and float(Q.min()) >= 0.0 and float(Q.max()) <= 1.0
    assert torch.equal(c["edges"], Q.double() >= th), "fp32 and float64 agree on the edges once the threshold is the fp32 one"
    assert bool(c["edges"][c["at_th"]].all()) and not bool(c["edges"][c["below"]].any())
    off = ~(c["at_th"] | c["below"])
    assert bool(((Q.double() - th).abs()[off] >= 0.04).all()), "no other entry comes near the threshold"
    p = M.contrast_reference(S, Q, c["th"], 1.0, torch.float64)["p"]
    for r, kind in enumerate(c["kinds"]):
        d = r % N
        assert float(Q[r, d]) == 1.0 and bool(c["edges"][r, d])
        e = c["edges"][r]
        if kind == "diag":
            assert int(e.sum()) == 1
        elif kind == "all":
            assert bool(e.all())
        elif kind == "th" and N >= 2:
            assert int(c["at_th"][r].sum()) >= 1 and (N < 3 or int(c["below"][r].sum()) >= 1)
            assert bool((Q[r][c["at_th"][r]] == np.float32(c["th"])).all()) and bool((Q[r][c["below"][r]] < np.float32(c["th"])).all())
            assert float(np.float32(c["th"])) != c["th"], "the double 0.7 is not the fp32 one: a float64 compare against it would differ"
            assert not bool((Q[r][c["at_th"][r]].double() >= c["th"]).any()), "... and would drop exactly the planted edges"
        elif kind == "sat":
            assert sorted(set(S[r].tolist())) == ([-5.0, 5.0] if N > 1 else [5.0]) and int((S[r] == 5.0).sum()) == 1
        elif kind == "eps":
            assert int(e.sum()) == M.EPS_ROW_EDGES + 1 and bool((S[r][e] == -5.0).all()) and bool((S[r][~e] == 5.0).all())
            assert 0.0 < float(p[r][e].max()) < M.f32(M.EPS_CONTRAST), "p < 1e-7 on every edge: the epsilon decides the value"


def test_contrast_table_reaches_what_it_names():
    ns = {N for _, N in M.CONTRAST_TABLE}
    assert {1, 2, 255, 256, 257} <= ns and max(ns) == 2597 and {r for r, _ in M.CONTRAST_TABLE} == {1, 3, 37}
    assert all(r == 37 for r, N in M.CONTRAST_TABLE if N == 2597) and all(r * N <= 37 * 2597 for r, N in M.CONTRAST_TABLE)
    kinds = {k for rows, N in M.CONTRAST_TABLE for k in M.contrast_kinds(rows, N)}
    assert kinds == {"rand", "diag", "all", "th", "sat", "eps"}
    assert {N for rows, N in M.CONTRAST_TABLE if "th" in M.contrast_kinds(rows, N)} >= {255, 256, 257, 2597}
    rows, N, th = M.CONTRAST_NO_EDGE
    assert th > 1.0 and not bool((M.contrast_case(rows, N)["Q"] >= th).any())


# ---------------------------------------------------------------------------------------------------------------------
# stil_simmatch_unfold
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_smooth", M.UNFOLD_CS)
@pytest.mark.parametrize("R,N,K", M.UNFOLD_TABLE)
def test_fp32_aten_meets_the_unfold_checks(R, N, K, c_smooth):
    tpo, probs, labels = M.unfold_case(R, N, K)
    r64 = M.unfold_reference(tpo, probs, labels, c_smooth, torch.float64)
    assert _finite(r64, ("teacher", "pseudo"))
    GM.check_unfold(M.unfold_reference(tpo, probs, labels, c_smooth, torch.float32), r64)
    assert float((r64["teacher"].sum(1) - 1.0).abs().max()) < 1e-12 and float((r64["pseudo"].sum(1) - 1.0).abs().max()) < 1e-6
    if c_smooth >= 1.0:
        assert torch.equal(r64["pseudo"], probs.double())


def test_unfold_labels_are_in_range_and_leave_a_class_empty():
    for R, N, K in M.UNFOLD_TABLE:
        tpo, probs, labels = M.unfold_case(R, N, K)
        assert labels.dtype == torch.int64 and labels.shape == (N,) and int(labels.min()) >= 0 and int(labels.max()) == K - 1
        agg = M.unfold_reference(tpo, probs, labels, 0.0, torch.float64)["agg"]
        if K > 1:
            assert bool((agg[:, 0] == 0).all()) and 0 not in labels.tolist(), "a class without a bank entry: its agg is 0"
    assert len(set(M.unfold_case(*M.UNFOLD_ONE_CLASS)[2].tolist())) == 1 and M.UNFOLD_ONE_CLASS in M.UNFOLD_TABLE
    assert {255, 256, 257} <= {N for _, N, _ in M.UNFOLD_TABLE} and any(K > 256 for _, _, K in M.UNFOLD_TABLE) and any(K == 1000 for _, _, K in M.UNFOLD_TABLE)
    assert {0.0, 1.0} <= set(M.UNFOLD_CS) and any(0.0 < c < 1.0 for c in M.UNFOLD_CS)


# ---------------------------------------------------------------------------------------------------------------------
# stil_freematch_update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", M.UPDATE_MOMENTA)
@pytest.mark.parametrize("R,K", M.UPDATE_TABLE)
def test_fp32_aten_meets_the_update_checks_and_rows_are_unambiguous(R, K, momentum):
    c = M.update_case(R, K, momentum)
    r64, r32 = M.update_run_reference(c, torch.float64), M.update_run_reference(c, torch.float32)
    assert len(r64) == M.UPDATE_CALLS == 2
    sides = set()
    for (probs, top, ties), a, b in zip(c["calls"], r32, r64):
        assert _finite(b, ("p_model", "label_hist", "time_p", "thr"))
        GM.check_update(a, b)
        assert torch.equal(a["mask"], b["mask"]), "fp32 and float64 select the same rows"
        tie_rows = [t for t, _, _ in ties]
        keep = torch.tensor([r not in tie_rows for r in range(R)])
        assert bool((_gap(probs)[keep] >= M.MIN_GAP).all()) and torch.equal(probs.argmax(1)[keep], top[keep])
        assert tie_rows == M.update_tie_rows(R, K)
        for t, c0, c1 in ties:
            row = probs[t]
            assert c0 < c1 and int(top[t]) == c0 and float(row[c0]) == float(row[c1]) == float(row.max()), "a tie is exact in fp32"
            rest = row.double().clone()
            rest[[c0, c1]] = 0
            assert float(row.double().max() - rest.max()) >= M.MIN_GAP
        if M.update_at_threshold(R, momentum):
            assert bool((b["mx"] == b["thr"]).all()) and bool((b["mask"] == 1).all()), "ON the threshold, in float64 too"
        else:
            assert bool(((b["mx"] - b["thr"]).abs() >= M.MIN_GAP).all())
        sides |= set(b["mask"].tolist())
        if M.f32(momentum) == 1.0:
            assert all(torch.equal(b[k], c[k].double()) for k in ("p_model", "label_hist", "time_p"))
    if R >= 40:
        assert sides == {0.0, 1.0}, "rows on both sides of the threshold"
    assert K == 1 or not torch.equal(c["calls"][0][0], c["calls"][1][0])
    assert (M.f32(momentum) == 1.0 or K == 1 or not torch.equal(r64[0]["p_model"], r64[1]["p_model"]))


def test_update_table_reaches_what_it_names():
    assert {255, 256, 257} <= {R for R, _ in M.UPDATE_TABLE} and {1, 2} <= {R for R, _ in M.UPDATE_TABLE}
    assert {1, 2, 286, 1000} <= {K for _, K in M.UPDATE_TABLE} and set(M.UPDATE_MOMENTA) == {0.999, 0.0, 1.0}
    assert any(M.update_tie_rows(R, K) for R, K in M.UPDATE_TABLE) and len(M.update_tie_rows(300, 286)) == 3
    assert any(M.update_at_threshold(R, m) for R, _ in M.UPDATE_TABLE for m in M.UPDATE_MOMENTA)


# ---------------------------------------------------------------------------------------------------------------------
# stil_freematch_entropy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", M.ENTROPY_MASKS)
@pytest.mark.parametrize("R,K", M.ENTROPY_TABLE)
def test_fp32_aten_meets_the_entropy_checks(R, K, kind):
    c, mask = M.entropy_case(R, K), M.entropy_mask(R, kind)
    r64 = M.entropy_reference(c, mask, torch.float64)
    assert _finite(r64, ("loss", "dz"))
    sel = mask != 0
    grad = M.entropy_has_gradient(c, mask)
    GM.check_entropy(M.entropy_reference(c, mask, torch.float32), r64, grad)
    assert bool((r64["dz"][~sel] == 0).all())
    if kind == "empty":
        assert not bool(sel.any()) and float(r64["loss"]) == 0.0 and not grad
        return
    assert grad == (int(sel.sum()) >= 2 and K >= 2), "every case with two selected rows and two classes predicts two classes"
    if grad:
        assert float(r64["dz"].abs().max()) >= M.ENTROPY_MIN_GRAD, f"a vacuous gradient check: max |dz| = {float(r64['dz'].abs().max()):.3e}"
    else:
        assert float(r64["dz"].abs().max()) <= 1e-12, "one predicted class: the loss is constant"
    if K >= 3:
        assert float(c["label_hist"][c["zero_class"]]) == 0.0 and float(r64["a"][c["zero_class"]]) == 0.0, "inf0(1 / label_hist)"
        assert int((c["label_hist"] == 0).sum()) == 1
    if K > int(sel.sum()) or K == 3:
        assert bool((r64["hist"] == 0).any()), "inf0(1 / hist): a class no selected row predicts"
    if K == 3:
        assert float(r64["hist"][2]) == 0.0


@pytest.mark.parametrize("R,K", M.ENTROPY_TABLE)
def test_entropy_rows_are_unambiguous_and_the_tie_is_exact(R, K):
    c = M.entropy_case(R, K)
    p32, p64 = c["z"].softmax(1), c["z"].double().softmax(1)
    assert torch.equal(p32.argmax(1), c["top"]), "argmax(softmax) in fp32 ATen is the planted column (first index on the tie)"
    keep = torch.ones(R, dtype=torch.bool)
    if c["tie"] is not None:
        keep[M.ENTROPY_TIE_ROW] = False
        c0, c1 = c["tie"]
        z, p = c["z"][M.ENTROPY_TIE_ROW], p32[M.ENTROPY_TIE_ROW]
        assert c0 < c1 and float(z[c0]) == float(z[c1]) == float(z.max()) and float(p[c0]) == float(p[c1]) == float(p.max()), "a tie is exact in fp32"
        rest = p64[M.ENTROPY_TIE_ROW].clone()
        rest[[c0, c1]] = 0
        assert float(p64[M.ENTROPY_TIE_ROW].max() - rest.max()) >= M.MIN_GAP
        assert all(float(M.entropy_mask(R, k)[M.ENTROPY_TIE_ROW]) != 0 for k in M.ENTROPY_MASKS if k != "empty"), "the tie row is selected"
    assert (c["tie"] is not None) == (R > M.ENTROPY_TIE_ROW and K >= 2)
    assert bool((_gap(p64)[keep] >= M.MIN_GAP).all()) and torch.equal(p64.argmax(1)[keep], c["top"][keep])


def test_entropy_table_and_masks_reach_what_they_name():
    assert {255, 256, 257} <= {R for R, _ in M.ENTROPY_TABLE} and any(K > 256 for _, K in M.ENTROPY_TABLE) and any(K == 1000 for _, K in M.ENTROPY_TABLE)
    assert {1, 2} <= {R for R, _ in M.ENTROPY_TABLE} and {1, 2, 3} <= {K for _, K in M.ENTROPY_TABLE}
    odd = M.entropy_mask(257, "odd")
    assert set(odd.tolist()) == {0.5, -1.0, 0.0} and torch.equal(odd != 0, odd.bool())
    mixed = M.entropy_mask(257, "mixed")
    assert 0 < float(mixed.sum()) < 257 and float(M.entropy_mask(257, "full").sum()) == 257 and float(M.entropy_mask(257, "empty").abs().sum()) == 0
    grads = [(R, K, k) for R, K in M.ENTROPY_TABLE for k in M.ENTROPY_MASKS if M.entropy_has_gradient(M.entropy_case(R, K), M.entropy_mask(R, k))]
    assert {(300, 286), (513, 65), (40, 1000), (2, 2), (257, 3)} <= {(R, K) for R, K, _ in grads}
    # the K = 3 tie row: its second column is class 2, which no row predicts -- a last-index argmax would change hist there
    assert M.entropy_case(257, 3)["tie"] == (1, 2)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: every call below fails the entry point's STIL_REQUIRE on the host; none reaches a launch
# ---------------------------------------------------------------------------------------------------------------------
def _refused(call, name):
    with pytest.raises(RuntimeError, match=f"{name}: bad arguments"):
        call()


def test_contrast_graph_refuses_before_any_launch(L):
    def call(S=True, Q=True, rl=True, dS=True, lds=8, ldq=8, ldd=8, rows=2, N=8):
        f = lambda on, off: fake(off) if on else None
        return lambda: L.contrast_graph(f(S, 0), lds, f(Q, 64), ldq, 0.7, f(rl, 128), f(dS, 192), ldd, rows, N, 0.5, None)
    for kw in (dict(S=False), dict(Q=False), dict(rl=False), dict(rows=0), dict(rows=-1), dict(N=0), dict(N=-3), dict(lds=7), dict(ldq=7), dict(ldd=7),
               dict(ldd=0), dict(lds=0, ldq=0)):
        _refused(call(**kw), "stil_contrast_graph")
    # ldd < N without dS is no refusal (ldd is not looked at): that call launches, so it is made on the GPU only
    # (tests/test_gpu_match_kernels.py passes ldd = 0 with dS = NULL); here the other checks still refuse it
    _refused(call(dS=False, ldd=0, rows=0), "stil_contrast_graph")


def test_simmatch_unfold_refuses_before_any_launch(L):
    def call(tpo=True, probs=True, labels=True, teacher=True, rows=2, N=8, K=3):
        f = lambda on, off: fake(off) if on else None
        return lambda: L.simmatch_unfold(f(tpo, 0), f(probs, 64), f(labels, 128), f(teacher, 192), None, rows, N, K, 0.9, None)
    for kw in (dict(tpo=False), dict(probs=False), dict(labels=False), dict(teacher=False), dict(rows=0), dict(rows=-2), dict(N=0), dict(N=-1), dict(K=0), dict(K=-1)):
        _refused(call(**kw), "stil_simmatch_unfold")


def test_freematch_update_refuses_before_any_launch(L):
    names = ("probs", "p_model", "label_hist", "time_p", "mask", "onehot", "idx", "scratch")

    def call(rows=4, K=3, null=None):
        p = [None if n == null else fake(64 * i) for i, n in enumerate(names)]
        return lambda: L.freematch_update(p[0], rows, K, p[1], p[2], p[3], 0.999, p[4], p[5], p[6], p[7], None)
    for n in names:
        _refused(call(null=n), "stil_freematch_update")
    for kw in (dict(rows=0), dict(rows=-1), dict(K=0), dict(K=-1)):
        _refused(call(**kw), "stil_freematch_update")


def test_freematch_entropy_refuses_before_any_launch(L):
    names = ("logits", "mask", "p_model", "label_hist", "loss", "dlogits", "P", "pred", "vec")

    def call(rows=4, K=3, null=None):
        p = [None if n == null else fake(64 * i) for i, n in enumerate(names)]
        return lambda: L.freematch_entropy(p[0], p[1], rows, K, p[2], p[3], p[4], p[5], p[6], p[7], p[8], None)
    for n in names:
        _refused(call(null=n), "stil_freematch_entropy")
    for kw in (dict(rows=0), dict(rows=-1), dict(K=0), dict(K=-1)):
        _refused(call(**kw), "stil_freematch_entropy")
