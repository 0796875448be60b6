"""CPU side of LAME test-time adaptation (tests/test_gpu_lame.py; Boudiaf et al., CVPR 2022; definition as recalled: unpinned): the
registration and the hparams rules; the conditions on the inputs the GPU tests use, checked on the float64 restatement of
tests/lame_cases.py -- no neighbour decision hangs on a d2 gap below 1e-9 (exact ties, which the tie rule decides, apart), no energy
ratio lies within 5 % of tol, so the device's stopping step is decided with margin, every row of Y sums to 1 and the energy does not
rise from step 2 on -- and the reason the method exists, in float64: on a class-ordered batch whose logits are right on half the rows,
the correction along the features' neighbour graph recovers nearly all of them."""
import os
import sys

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import lame_cases as C  # noqa: E402

KEYS = ("tta_lame_affinity", "tta_lame_knn", "tta_lame_lambda", "tta_lame_steps", "tta_lame_tol")
DEFAULTS = ("knn", 5, 1.0, 100, 1e-8)


def _model(**over):
    from stil_tta_amd import STiLModel
    d = dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False)
    d.update(over)
    return STiLModel(d)


def _checked(**over):
    """the hparams of _model(**over) through tta.check_hparams alone: what the constructor runs, without building the backbone"""
    from stil_tta_amd import tta
    from stil_tta_amd.stil_model import _as_namespace
    hp = _as_namespace(dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False, **over))
    tta.check_hparams(hp)
    return hp


# ------------------------------------------------------------------------------------------ registration
def test_lame_is_registered_with_its_keys_and_defaults():
    from stil_tta_amd import tta
    m = _model(tta=True, tta_method="lame")
    assert m._tta_on() and not _model(tta=False, tta_method="lame")._tta_on()
    assert tuple(getattr(m.hp, k) for k in KEYS) == DEFAULTS
    assert "lame" in tta.METHODS and tta.STEPS["lame"] is tta.lame_step and callable(tta.lame_correct)
    assert tta.LAME_AFFINITIES == C.KINDS and tta.LAME_MAX_ROWS == 2048
    assert m._tent is None and m._bn_mem is None and m.last_tta == {}
    assert tuple(getattr(_model().hp, k) for k in KEYS) == DEFAULTS   # the keys exist whatever the method
    # the BatchNorm knobs compose (the paper's LAME on adapted statistics); episodic acts on the memory only
    hp = _model(tta=True, tta_method="lame", tta_bn_prior=16, tta_bn_momentum=0.05, tta_episodic=True).hp
    assert (hp.tta_bn_prior, hp.tta_bn_momentum, hp.tta_episodic) == (16, 0.05, True)


def test_lame_refuses_the_fusion_set_and_saint():
    with pytest.raises(ValueError, match="fusion"):
        _model(tta=True, tta_method="lame", tta_params="fusion")
    with pytest.raises(NotImplementedError):
        _model(tta=True, tta_method="lame", tabular_encoder="saint")
    with pytest.raises(NotImplementedError):
        _model(tta_method="lame", algorithm_name="STiL_SAINT")
    with pytest.raises(ValueError, match="tta_method"):
        _model(tta=True, tta_method="LAME")


@pytest.mark.parametrize("method", [None, "tent", "lame"])
def test_lame_keys_are_checked_whatever_the_method(method):
    nan, inf = float("nan"), float("inf")
    bad = dict(tta_lame_affinity=("linear", "KNN", "", None, 0, 1.0, True, ("knn",)),
               tta_lame_knn=(0, -1, 5.0, "5", None, True, inf, nan),
               tta_lame_lambda=(-1.0, -1e-9, inf, -inf, nan, "1", None, True),
               tta_lame_steps=(0, -3, 100.0, "100", None, True, inf, nan),
               tta_lame_tol=(-1e-8, -1.0, inf, nan, "1e-8", None, False))
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=key):
                _checked(tta=True, tta_method=method, **{key: v})
        with pytest.raises(ValueError, match=key):   # the model's constructor is where the check runs
            _model(tta=True, tta_method=method, **{key: values[0]})
    ok = _model(tta=True, tta_method=method, tta_lame_affinity="rbf", tta_lame_knn=1, tta_lame_lambda=0, tta_lame_steps=1, tta_lame_tol=0).hp
    assert tuple(getattr(ok, k) for k in KEYS) == ("rbf", 1, 0, 1, 0)
    assert _checked(tta=True, tta_method=method, tta_lame_knn=10 ** 6, tta_lame_lambda=2.5).tta_lame_lambda == 2.5


def test_lame_correct_has_no_cpu_path_and_names_its_bound():
    from stil_tta_amd import tta
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tta.lame_correct(torch.zeros(4, 3), torch.zeros(4, 8))


# ------------------------------------------------------------------------------------------ the cases cover what the issue lists
def test_the_cases_cover_every_shape_k_kind_lambda_and_stopping_mode():
    aff, rws = C.affinity_cases(), C.rows_cases()
    assert len(set(aff)) == len(aff) and len(set(rws)) == len(rws)
    assert set(C.SEEDS) <= set(rws)
    for rows, K, D in C.SHAPES:
        ks = C.ks_of(rows)
        assert {1, 5} <= set(ks) and max(ks) > rows and (rows < 2 or rows - 1 in ks)
        mine = [c for c in aff if c[:3] == (rows, D, "plain")]
        assert {(c[3], c[4]) for c in mine} == {(k, kind) for k in ks for kind in C.KINDS}
        mine = [c for c in rws if c[:4] == (rows, K, D, "plain")]
        assert {(c[6], c[7], c[8]) for c in mine} == {(lam,) + stop for lam in C.LAMS for stop in C.STOPS}
        assert {c[5] for c in mine} == set(C.KINDS) and len({c[4] for c in mine}) >= min(3, len(ks))
    for fkind in C.FKINDS[1:]:
        assert {c[:2] for c in aff if c[2] == fkind} == {(r, d) for r, _, d in C.SPECIAL}
        assert {c[:3] for c in rws if c[3] == fkind} == set(C.SPECIAL)
        assert {(c[7], c[8]) for c in rws if c[3] == fkind} == set(C.STOPS)
    assert {c[4] for c in rws} >= {1, 5} and any(c[4] == c[0] - 1 for c in rws) and any(c[4] > c[0] for c in rws)


# ------------------------------------------------------------------------------------------ conditioning of the cases
@pytest.mark.parametrize("rows,D,fkind", sorted({c[:3] for c in C.affinity_cases()}))
def test_no_neighbour_decision_hangs_on_a_small_gap(rows, D, fkind):
    """exact ties exist in the tied kind (duplicated rows: the tie rule is the point), in the zero kind (d2 = 2 exactly from the zero
    row to everyone) and in the nan kind (every NaN orders as +inf); they are decided by the lower index, not by rounding"""
    for k in C.ks_of(rows):
        F, ref = C.affinity_case(rows, D, fkind, k, "knn")
        C.check_gaps(F, fkind, k)
        kp = min(k, rows - 1)
        nbr = ref["nbr"]
        assert bool((nbr[:, :kp] >= 0).all()) and bool((nbr[:, :kp] < rows).all()) and bool((nbr[:, kp:] == -1).all())
        assert all(len(set(r[:kp].tolist())) == kp and i not in r[:kp].tolist() for i, r in enumerate(nbr))
    if fkind == "tied" and rows >= 4:
        F, ref = C.affinity_case(rows, D, fkind, 5, "knn")
        assert torch.equal(F[0], F[1]) and int(ref["nbr"][0, 0]) == 1 and int(ref["nbr"][1, 0]) == 0
        d2 = ref["d2"]
        assert bool((d2[4:, 0] == d2[4:, 1]).all()), "duplicated rows must be equally far from everyone, bit for bit"
        lists = ref["nbr"][4:, : min(5, rows - 1)].tolist()
        assert all(r.index(0) + 1 == r.index(1) for r in lists if 0 in r and 1 in r), "a tie goes to the lower index"


@pytest.mark.parametrize("case", C.rows_cases(), ids=lambda c: "-".join(map(str, c)))
def test_the_iteration_is_well_conditioned(case):
    rows, K, D, fkind, k, kind, lam, tol, max_steps = case
    Z, F, ref = C.rows_case(*case)
    C.check_gaps(F, fkind, k)
    steps, e = ref["steps"], ref["energy"]
    assert 1 <= steps <= max_steps and e.numel() == steps
    if tol == 0:
        assert steps == max_steps
    if fkind == "nan":   # only the neighbour lists of the finite rows, the range and termination are asserted on this kind
        assert steps == max_steps
        return
    assert C.band_clear(ref["ratios"], tol), f"an energy ratio within {C.BAND:.0%} of tol: {ref['ratios']}"
    assert bool(torch.isfinite(ref["Y"]).all()) and float((ref["Y"].sum(1) - 1).abs().max()) <= 1e-12
    assert bool((e[2:] <= e[1:-1]).all()), f"the energy rises: {e.tolist()}"
    if lam == 0 or rows == 1:
        assert steps == (2 if tol > 0 else max_steps) and float((ref["Y"] - ref["p"]).abs().max()) <= (K + 1) * 1e-10
    if K == 1:
        assert bool((ref["Y"] == 1).all())
    assert torch.equal(ref["A"], ref["A"].T) and float(ref["A"].diagonal().abs().max()) == 0


def test_without_neighbours_the_scores_are_the_softmax_and_two_steps_run():
    Z, F = C.inputs(1, 3, 8, "plain")
    r = C.lame_ref64(Z, F, 5, "rbf", 1.0, 100, 1e-8)
    assert r["steps"] == 2 and float(r["A"].abs().max()) == 0 and bool((r["nbr"] == -1).all()) and float(r["dk"][0]) == 0
    assert float((r["Y"] - torch.softmax(Z.double(), 1)).abs().max()) <= 4e-10   # softmax(log(p + 1e-10)) = (p + 1e-10) / (1 + K 1e-10)
    assert r["energy"][0] == r["energy"][1]


# ------------------------------------------------------------------------------------------ the reason the method exists
def test_the_correction_recovers_a_class_ordered_batch_in_float64():
    c = C.PROPERTY
    Z, F, y, ref = C.property_ref()
    assert Z.shape == (48, 8) and F.shape == (48, 32) and len(set(y.tolist())) == 3 and y.tolist() == sorted(y.tolist(), key=y.tolist().index)
    raw = float((Z.argmax(1) == y).float().mean())
    acc = float((ref["Y"].argmax(1) == y).float().mean())
    print(f"raw accuracy {raw:.3f}, corrected {acc:.3f}, steps {ref['steps']}")
    assert 0.35 <= raw <= 0.65, raw
    assert acc - raw >= 0.3 and acc >= 0.94, (raw, acc)
    assert 2 <= ref["steps"] < c["max_steps"] and C.band_clear(ref["ratios"], c["tol"])
    top = ref["Y"].topk(2, dim=1).values
    assert int(((top[:, 0] - top[:, 1]) <= C.MARGIN).sum()) <= C.MAX_EXCLUDED
