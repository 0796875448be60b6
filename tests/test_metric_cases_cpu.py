"""The cases of tests/metric_cases.py on the host: the references agree with ATen where ATen speaks (top-1 with argmax, NaN rows
included; binary accuracy with `p > thr`) and with scikit-learn's roc_auc_score on every AUROC case whose classes have both
sides; oracle/metrics_oracle.py agrees with them; the tables hold what they name and `coverage_gaps()` can fail.  The NaN rows
of the top-k table are the ones the rule `beat = (v > st) | (v == st & j < t)` -- the kernel's and the oracle's before NaN was
ranked -- gets wrong: `test_the_unranked_nan_rule_fails_exactly_the_nan_rows` says which."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metric_cases as M  # noqa: E402

from oracle import metrics_oracle as MO  # noqa: E402


def _f64_area(u2, n_pos, n_neg):
    return u2 / (2.0 * n_pos * n_neg) if n_pos and n_neg else 0.0


# ------------------------------------------------------------------------------------------------ ATen and scikit-learn
def test_top1_reference_is_atens_argmax_nan_rows_included():
    rows = 0
    for c in M.TOPK_TABLE:
        s, y = M.topk_case(c)
        valid = (y >= 0) & (y < c.K)
        am = s[:, :c.K].argmax(1)
        assert torch.equal(M.topk_reference(s, y, c.K, 1), valid & (am == y)), c.name
        assert bool(M.topk_reference(s, y, c.K, c.K)[valid].all()) and not bool(M.topk_reference(s, y, c.K, c.K)[~valid].any()), c.name
        rows += len(y)
    assert rows > 2000
    nan = M.NAN
    three = torch.tensor([[nan, nan, nan]] * 3)
    assert int(three.argmax(1)[0]) == 0 and M.topk_reference(three, torch.arange(3), 3, 1).tolist() == [True, False, False]
    mixed = torch.tensor([[0.1, nan, 0.3]] * 3)
    assert int(mixed.argmax(1)[0]) == 1 and M.topk_reference(mixed, torch.arange(3), 3, 1).tolist() == [False, True, False]
    assert M.topk_reference(mixed, torch.arange(3), 3, 2).tolist() == [False, True, True]


def test_topk_reference_is_atens_topk_where_the_kth_score_is_untied():
    """torch.topk promises no order among equal scores: compared on the rows whose k-th and (k+1)-th sorted scores differ"""
    seen = 0
    for c in M.TOPK_TABLE:
        s, y = M.topk_case(c)
        s = s[:, :c.K]
        for k in M.topk_ks(c):
            if k >= c.K:
                continue
            top = torch.sort(s, dim=1, descending=True, stable=True).values
            a, b = top[:, k - 1], top[:, k]
            untied = ~((a == b) | (a.isnan() & b.isnan()))
            valid = (y >= 0) & (y < c.K)
            member = (torch.topk(s, k, dim=1).indices == y[:, None]).any(1)
            assert torch.equal(M.topk_reference(s, y, c.K, k)[untied], (valid & member)[untied]), (c.name, k)
            seen += int(untied.sum())
    assert seen > 1000


def test_binary_reference_is_atens_comparison():
    for c in M.BINARY_TABLE:
        p, y = M.binary_case(c)
        ref = M.binary_reference(p.numpy(), y.numpy(), c.thr)
        assert np.array_equal(ref, ((p > c.thr) == (y == 1)).numpy()), c
        nan = torch.isnan(p).numpy()
        assert np.array_equal(ref[nan], (y != 1).numpy()[nan]), "a NaN score predicts 0"


def test_auroc_reference_against_sklearn():
    """order is all the area depends on: a column with infinities (which scikit-learn refuses) is replaced by its dense ranks"""
    from sklearn.metrics import roc_auc_score
    classes = 0
    for c in M.AUROC_TABLE:
        s, y = M.auroc_case(c)
        s, y = s.numpy()[:, :c.K], y.numpy()
        assert not np.isnan(s).any()
        per, macro, u2, n_pos, n_neg = M.auroc_expected(c)
        pos = M.positives(y, c.K)
        for k in range(c.K):
            if not (n_pos[k] and n_neg[k]):
                assert per[k] == 0
                continue
            col = s[:, k].astype(np.float64)
            if not np.isfinite(col).all():
                col = np.unique(s[:, k], return_inverse=True)[1].astype(np.float64)
            assert abs(_f64_area(u2[k], n_pos[k], n_neg[k]) - roc_auc_score(pos[:, k], col)) < 1e-12, (M.auroc_id(c), k)
            classes += 1
    assert classes > 150


def test_auroc_reference_mirrors_under_negation():
    """U2(s) + U2(-s) = 2 n_pos n_neg: every pair is counted once, whatever its sign, zero or infinity"""
    for c in M.AUROC_TABLE:
        s, y = M.auroc_case(c)
        _, _, u2, n_pos, n_neg = M.auroc_expected(c)
        _, _, m2, _, _ = M.auroc_reference(-s.numpy()[:, :c.K], y.numpy(), c.K)
        assert [a + b for a, b in zip(u2, m2)] == [2 * p * n for p, n in zip(n_pos, n_neg)], M.auroc_id(c)


# ---------------------------------------------------------------------------------------------------------- the oracle
def _oracle_topk_hits(s, y, K, k):
    valid = ((y >= 0) & (y < K)).numpy()
    return round(MO.topk_accuracy(s.numpy()[valid][:, :K], y.numpy()[valid], k) * int(valid.sum())) if valid.any() else 0


@pytest.mark.parametrize("name", [c.name for c in M.TOPK_TABLE])
def test_oracle_topk_agrees_with_the_reference(name):
    """on every case, the NaN rows included (fails on the unranked rule for every `nan_*` case)"""
    c = M.TOPK_BY_NAME[name]
    s, y = M.topk_case(c)
    for k in M.topk_ks(c):
        assert _oracle_topk_hits(s, y, c.K, k) == int(M.topk_reference(s, y, c.K, k).sum()), (name, k)


def test_oracle_binary_and_auroc_agree_with_the_references():
    for c in M.BINARY_TABLE:
        p, y = M.binary_case(c)
        assert MO.binary_accuracy(p.numpy(), y.numpy(), c.thr) == float(M.binary_reference(p.numpy(), y.numpy(), c.thr).mean()), c
    for c in M.AUROC_TABLE:
        s, y = M.auroc_case(c)
        s, y = s.numpy()[:, :c.K], y.numpy()
        per, macro, u2, n_pos, n_neg = M.auroc_expected(c)
        if c.K == 1:
            got = np.array([MO.binary_auroc(s[:, 0], y == 1)])
        else:
            got = MO.multiclass_auroc(s, y)[1]
        assert got.tolist() == [_f64_area(*t) for t in zip(u2, n_pos, n_neg)], M.auroc_id(c)
        assert np.array_equal(got.astype(np.float32), per), M.auroc_id(c)


def test_the_unranked_nan_rule_fails_exactly_the_nan_rows():
    """`topk_parent_rule` is the expression before NaN was ranked.  It equals the reference on every NaN-free row of the table and
    differs on NaN rows only; on those it never misses a hit, it invents them: "all" (every target but 0), "below_target",
    "around_target", a NaN target behind another NaN -- and at k = 1 also "above_target", where ATen's argmax is the NaN."""
    wrong = {}
    for c in M.TOPK_TABLE:
        s, y = M.topk_case(c)
        has_nan = torch.isnan(s[:, :c.K]).any(1)
        for k in M.topk_ks(c):
            ref, old = M.topk_reference(s, y, c.K, k), M.topk_parent_rule(s.numpy(), y.numpy(), c.K, k)
            assert torch.equal(ref[~has_nan], old[~has_nan]), (c.name, k)
            assert not bool((ref & ~old).any()), "the unranked rule only ever adds hits"
            if c.name.startswith("nan"):
                for (_, t, place), bad in zip(M.nan_rows(c.K), (ref != old).tolist()):
                    if bad:
                        wrong.setdefault(place, set()).add(k)
    print("TOPK_NAN_ROWS the unranked rule gets wrong, by placement and k:", {p: sorted(ks) for p, ks in sorted(wrong.items())})
    assert 1 in wrong["all"] and 1 in wrong["below_target"] and 1 in wrong["above_target"] and 1 in wrong["around_target"]
    assert 2 in wrong["around_target"] and "at_target" not in wrong and "nan_target_first" not in wrong
    assert 1 in wrong["nan_target_second"] and 2 in wrong["nan_target_third"]
    for c in M.TOPK_NAN:
        s, y = M.topk_case(c)
        assert not torch.equal(M.topk_reference(s, y, c.K, 1), M.topk_parent_rule(s.numpy(), y.numpy(), c.K, 1)), c.name


# ------------------------------------------------------------------------------------------- the tables hold what they name
def test_the_tables_hold_what_they_name():
    T = M.AUROC_TABLE
    assert {(c.N, c.K) for c in T} >= {(N, K) for N in M.AUROC_NS for K in M.AUROC_KS}
    assert {(c.kind, c.layout) for c in T} == {(k, l) for k in M.AUROC_KINDS for l in M.AUROC_LAYOUTS}
    assert M.AUROC_WIDE in T and M.auroc_case(M.AUROC_WIDE)[0].shape == (300, 289) and bool(M.auroc_case(M.AUROC_WIDE)[0][:, 286:].isnan().all())
    assert len({M.auroc_id(c) for c in T}) == len(T)
    both_zeros_both_sides = 0
    for c in T:
        s, y = M.auroc_case(c)
        s, y = s.numpy()[:, :c.K], y.numpy()
        _, _, _, n_pos, n_neg = M.auroc_expected(c)
        hi, one = (2, 0) if c.K == 1 else (c.K, 0)
        if c.layout == "one_pos":
            assert n_pos[one] == 1 and n_neg[one] == c.N - 1
        elif c.layout == "one_neg":
            assert n_neg[one] == 1 and n_pos[one] == c.N - 1
        elif c.layout == "absent":
            assert n_pos[-1] == 0
        elif c.layout == "one_class":
            assert n_pos[-1] == c.N and n_neg[-1] == 0
        elif c.layout == "bad_labels":
            assert c.N < 12 or ({-1, hi, 2 ** 40} <= set(y.tolist()) and sum(n_pos) < c.N)
        else:
            assert int(y.min()) >= 0 and int(y.max()) < hi
        if c.kind == "softmax":
            assert s.min() >= 0 and s.max() <= 1
        elif c.kind == "logits" and c.N >= 63:
            assert s.min() < -1 and s.max() > 1
        elif c.kind == "tied" and c.N >= 2:
            assert (np.signbit(s) & (s == 0)).any() and (~np.signbit(s) & (s == 0)).any() and (c.N < 255 or len(np.unique(s)) < s.size // 2)
        elif c.kind == "two":
            assert set(np.unique(s).tolist()) <= {-1.0, 1.0}
        elif c.kind == "const":
            assert len(np.unique(s)) == 1
        elif c.kind == "specials" and c.N >= 255:
            assert set(M.SPECIALS) <= set(s.flatten().tolist()) and (np.signbit(s) & (s == 0)).any()
            pos = M.positives(y, c.K)
            for k in range(c.K):
                z, neg0 = s[:, k] == 0, np.signbit(s[:, k])
                sides = [bool((z & sg & side).any()) for sg in (neg0, ~neg0) for side in (pos[:, k], ~pos[:, k])]
                both_zeros_both_sides += all(sides)
                assert all(sides) or n_pos[k] < 2 or n_neg[k] < 2, (M.auroc_id(c), k)
    assert both_zeros_both_sides >= 10
    # top-k
    assert {(c.K, c.N) for c in M.TOPK_GRID} == {(K, N) for K in M.TOPK_KS for N in M.TOPK_NS}
    assert all(M.topk_ks(c) == tuple(dict.fromkeys((1, 2, 5, c.K))) for c in M.TOPK_TABLE)
    for c in M.TOPK_GRID:
        s, y = M.topk_case(c)
        assert s.shape == (c.N, c.K) and int(y.min()) >= 0 and int(y.max()) < c.K and torch.equal(s, torch.round(s * 10) / 10)
    assert bool((M.topk_case(M.TOPK_BY_NAME["grid_K286_N257"])[0] < 0).any())
    s, y = M.topk_case(M.TOPK_BY_NAME["ties"])
    for (r, t, (where, what)), row, tt in zip(M.tie_rows(), s, y):
        a, b = [int(i) for i in torch.nonzero(row == row.max()).flatten()]
        assert ((b - a) % M.WAVE == 0) == (where == "lane") and int(tt) == {"first": a, "second": b, "neither": b + 1}[what]
    s, y = M.topk_case(M.TOPK_BY_NAME["zeros"])
    assert bool(((s == 0).sum(1) == 2).all()) and bool((torch.signbit(s) & (s == 0)).sum(1).eq(1).all()) and bool((s.max(1).values == 0).all())
    s, y = M.topk_case(M.TOPK_BY_NAME["infs"])
    assert bool((s == M.INF).any()) and bool((s == -M.INF).any()) and bool((s[torch.arange(len(y)), y] == -M.INF).any())
    s, y = M.topk_case(M.TOPK_BY_NAME["bad_targets"])
    assert {-1, 5, 2 ** 40, -2 ** 63} <= set(y.tolist()) and int(((y >= 0) & (y < 5)).sum()) == 5
    for name, fill in (("ld_nan", None), ("ld_inf", M.INF)):
        c = M.TOPK_BY_NAME[name]
        pad = M.topk_case(c)[0][:, c.K:]
        assert pad.shape[1] == M.TOPK_PAD == 5 and bool(pad.isnan().all() if fill is None else (pad == fill).all())
    for c in M.TOPK_NAN:
        rows = M.nan_rows(c.K)
        assert {p for _, _, p in rows} >= set(M.NAN_PLACEMENTS)
        for r, t, place in rows:
            n = torch.isnan(r)
            want = {"all": bool(n.all()), "at_target": bool(n[t]) and int(n.sum()) == 1, "below_target": bool(n[:t].any()) and not bool(n[t:].any()),
                    "above_target": bool(n[t + 1:].any()) and not bool(n[:t + 1].any()),
                    "around_target": bool(n[:t].any()) and bool(n[t + 1:].any()) and not bool(n[t])}.get(place, bool(n[t]) and int(n.sum()) == 3)
            assert want, (c.name, t, place)
        assert c.K <= M.WAVE or any(t >= M.WAVE for _, t, _ in rows)
    # binary
    assert {(c.N, c.thr) for c in M.BINARY_TABLE} == {(N, t) for N in M.BINARY_NS for t in M.BINARY_THRS}
    for c in M.BINARY_TABLE:
        p, y = M.binary_case(c)
        assert float(p[0]) == c.thr
        if c.N >= 63:
            bits = lambda v: np.float32(v).view(np.int32).item()
            got = {(bits(a), int(b)) for a, b in zip(p.numpy(), y.numpy())}
            assert {(bits(v), l) for v in M.binary_planted(c.thr) for l in M.BINARY_LABELS} <= got, c
            plain = ~np.isin(p.numpy().view(np.int32), [bits(v) for v in M.binary_planted(c.thr)])
            assert (p.numpy()[plain] > c.thr).any() and (p.numpy()[plain] < c.thr).any()
    up, down = M.binary_planted(0.0)[1:3]
    assert up == M.SUB and down == -M.SUB


def test_coverage_gaps_is_empty_and_can_fail():
    assert M.coverage_gaps() == []
    A, T, B = M.AUROC_TABLE, M.TOPK_TABLE, M.BINARY_TABLE
    assert ("auroc", "second trip of the scan") in M.coverage_gaps(auroc=[c for c in A if c.N <= M.SCAN_TRIP])
    assert ("auroc", "a scan of full trips only") in M.coverage_gaps(auroc=[c for c in A if c.N != 2048])
    assert ("auroc", "two-valued column beyond one trip") in M.coverage_gaps(auroc=[c for c in A if c.kind != "two" or c.N <= M.SCAN_TRIP])
    assert ("auroc", "ld > K") in M.coverage_gaps(auroc=[c for c in A if not c.pad])
    assert ("auroc", "kind specials") in M.coverage_gaps(auroc=[c for c in A if c.kind != "specials"])
    assert ("auroc", "layout bad_labels") in M.coverage_gaps(auroc=[c for c in A if c.layout != "bad_labels"])
    assert ("topk", "second trip of the K loop") in M.coverage_gaps(topk=[c for c in T if c.K <= M.WAVE])
    one_row = [c for c in T if c.N == 1]
    assert {("topk", "row not in wave 0 of its block"), ("topk", "partial last block"), ("topk", "more than one block")} <= set(M.coverage_gaps(topk=one_row))
    assert ("topk", "partial last block") in M.coverage_gaps(topk=[c for c in M.TOPK_GRID if c.N in (1, 3, 4)])
    assert ("topk", "ld > K") in M.coverage_gaps(topk=[c for c in T if not c.pad])
    no_ties = M.coverage_gaps(topk=[c for c in T if c.name != "ties"])
    assert {("topk", "tie within a lane"), ("topk", "tie across lanes"), ("topk", "tie target second")} <= set(no_ties)
    assert ("topk", "tie within a lane") in M.coverage_gaps(ties=[w for _, _, w in M.tie_rows() if w[0] != "lane"])
    assert ("topk", "tie across lanes") in M.coverage_gaps(ties=[w for _, _, w in M.tie_rows() if w[0] != "lanes"])
    assert ("binary", "partial last block") in M.coverage_gaps(binary=[c for c in B if c.N <= M.BIN_BLOCK])
    assert ("binary", "row not in wave 0 of its block") in M.coverage_gaps(binary=[c for c in B if c.N <= M.WAVE])
    assert ("binary", "a full block") in M.coverage_gaps(binary=[c for c in B if c.N != 256])


def test_the_nan_column_case_differs_in_one_column_only():
    dirty, clean, y = M.auroc_nan_column_case()
    n = torch.isnan(dirty)
    assert bool(n[:, M.AUROC_NAN_COLUMN].any()) and not bool(n[:, [0, 2]].any()) and not bool(torch.isnan(clean).any())
    assert torch.equal(dirty[~n], clean[~n]) and dirty.shape == M.AUROC_NAN_SHAPE
