"""The shifted test stream (stil_tta_amd/shift.py, csrc/shift.hip) as far as it can be checked without a GPU:

1. ShiftSpec / resolve refuse what they must; the wrappers refuse bad tensors before any launch.
2. Every stil_shift_* entry point refuses bad arguments through the C ABI without a device.
3. TableStats.from_table against numpy; class_ordered; IndexLoader(order=...).
4. The MODEL's statistics (tests/shift_cases.py): the normals' mean and variance, the impulse and missing fractions.
5. The GPU bar is well-posed: the definitions evaluated in float32 numpy stay within a quarter of close(TOL) of the float64 model
   on every arithmetic case tests/test_gpu_shift.py runs (worst values printed; DESIGN.md section 19 records them)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import shift_cases as SC  # noqa: E402
from test_gpu_ops import TOL  # noqa: E402


def _stats():
    from stil_tta_amd.shift import TableStats
    return TableStats(*SC.table_stats(9, 4))


# ------------------------------------------------------------------------------------------ 1. validation on the host
def test_the_shift_names_and_severity_tables():
    from stil_tta_amd import shift as S
    assert S.IMAGE_SHIFTS == ("gaussian_noise", "impulse_noise", "contrast", "brightness", "gaussian_blur", "pixelate")
    assert S.TABULAR_SHIFTS == ("tab_noise", "tab_missing", "tab_cat_flip")
    assert set(S.SEVERITY) == set(S.IMAGE_SHIFTS + S.TABULAR_SHIFTS) and all(len(v) == 5 for v in S.SEVERITY.values())
    assert S.SEVERITY["gaussian_noise"] == (0.08, 0.12, 0.18, 0.26, 0.38) and S.SEVERITY["impulse_noise"] == (0.03, 0.06, 0.09, 0.17, 0.27)
    assert S.SEVERITY["contrast"] == (0.4, 0.3, 0.2, 0.1, 0.05) and S.SEVERITY["brightness"] == (0.1, 0.2, 0.3, 0.4, 0.5)
    assert S.SEVERITY["gaussian_blur"] == (1, 2, 3, 4, 6) and S.SEVERITY["pixelate"] == (2, 3, 4, 6, 8)
    assert S.SEVERITY["tab_noise"] == (0.1, 0.25, 0.5, 1, 2) and S.SEVERITY["tab_missing"] == (0.1, 0.2, 0.3, 0.5, 0.7)
    assert S.SEVERITY["tab_cat_flip"] == (0.05, 0.1, 0.2, 0.3, 0.5)
    assert S.resolve(("contrast", 5)) == ("contrast", 0.05) and S.resolve(("contrast", 0.5)) == ("contrast", 0.5)
    assert S.resolve(("pixelate", 1)) == ("pixelate", 2.0) and S.resolve(("pixelate", 1.0)) == ("pixelate", 1.0)
    assert S.resolve(("brightness", -0.25)) == ("brightness", -0.25)


def test_shift_spec_refuses_what_it_must():
    from stil_tta_amd.shift import ShiftSpec
    st = _stats()
    ok = ShiftSpec(image=("gaussian_noise", 3), tabular=("tab_missing", 0.2), seed=7, columns=[0, 8], stats=st)
    assert ok.image == ("gaussian_noise", 0.18) and ok.tabular == ("tab_missing", 0.2) and ok.col_on.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1]
    assert ShiftSpec().image is None and ShiftSpec().tabular is None and ShiftSpec(clip=None).clip is None
    bad = [
        dict(image=("fog", 1)), dict(tabular=("gaussian_noise", 1), stats=st), dict(image=("tab_noise", 1)),           # unknown names
        dict(image=("contrast", 0)), dict(image=("contrast", 6)), dict(tabular=("tab_noise", 0), stats=st),              # severity 0 or 6
        dict(image=("contrast", True)), dict(image=("pixelate", False)), dict(image=("contrast", "3")),                  # a bool as a level
        dict(image=("gaussian_noise", -0.1)), dict(image=("gaussian_blur", -1.0)), dict(tabular=("tab_noise", -1.0), stats=st),
        dict(image=("impulse_noise", 1.5)), dict(tabular=("tab_missing", 1.01), stats=st), dict(tabular=("tab_cat_flip", 2.0), stats=st),
        dict(image=("pixelate", 0.0)), dict(image=("pixelate", 0.5)), dict(image=("pixelate", 2.5)),                     # s < 1, s not whole
        dict(image=("gaussian_noise", float("nan"))), dict(image=("brightness", float("inf"))),
        dict(tabular=("tab_noise", 1)),                                                                                 # no stats
        dict(tabular=("tab_noise", 1), stats=st, columns=[9]), dict(tabular=("tab_noise", 1), stats=st, columns=[-1]),   # columns out of range
        dict(columns=[0]), dict(image=("contrast",)), dict(image="contrast"), dict(seed=-1), dict(seed=True),
        dict(image=("impulse_noise", 1), clip=None), dict(clip=(1.0, 0.0)), dict(stats=object()),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ShiftSpec(**kw)


def test_wrappers_refuse_bad_tensors_before_any_launch():
    from stil_tta_amd import shift as S
    img = torch.zeros(2, 3, 4, 4)
    for fn, arg in ((S.gaussian_noise, 0.1), (S.impulse_noise, 0.1), (S.contrast, 0.5), (S.brightness, 0.1), (S.pixelate, 2), (S.gaussian_blur, 1.0)):
        for bad in (img.double(), img[0], img[:0], img.permute(0, 1, 3, 2), "x"):
            with pytest.raises(ValueError):
                fn(bad, arg)
        with pytest.raises(RuntimeError, match="no CPU fallback"):     # a valid call: only the device is missing
            fn(img, arg)
    for fn, arg in ((S.brightness, 0.1), (S.gaussian_blur, 1.0)):
        with pytest.raises(ValueError, match="3 channels"):
            fn(torch.zeros(2, 1, 4, 4), arg)
    for fn, arg in ((S.gaussian_noise, -1.0), (S.impulse_noise, 1.5), (S.contrast, -0.5), (S.brightness, math.nan), (S.pixelate, 0), (S.pixelate, 1.5)):
        with pytest.raises(ValueError):
            fn(img, arg)
    with pytest.raises(ValueError, match="negative"):
        S.gaussian_noise(img, 0.1, offset=-1)
    with pytest.raises(ValueError, match="finite"):
        S.impulse_noise(img, 0.1, clip=None)
    st = _stats()
    tab = torch.zeros(5, 9)
    for bad in (tab.double(), tab[:, :8], tab[:0], tab.t().contiguous().t(), None):
        with pytest.raises(ValueError):
            S.tab_shift(bad, st, "tab_noise", 1.0)
    for name, s in (("tab_noise", -1.0), ("tab_missing", 1.5), ("tab_flip", 0.1)):
        with pytest.raises(ValueError):
            S.tab_shift(tab, st, name, s)
    with pytest.raises(ValueError, match="TableStats"):
        S.tab_shift(tab, None, "tab_noise", 1.0)
    with pytest.raises(ValueError, match="col_on"):
        S.tab_shift(tab, st, "tab_noise", 1.0, col_on=torch.ones(8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.tab_shift(tab, st, "tab_noise", 1.0)
    assert [S.blur_ksize(s, 64, 64) for s in S.SEVERITY["gaussian_blur"]] == [9, 17, 25, 33, 49]
    assert S.blur_ksize(8.0, 64, 64) == 63 and S.blur_ksize(6.0, 5, 7) == 9 and S.blur_ksize(1.0, 1, 9) == 1 and S.blur_ksize(0.0, 8, 8) == 1
    s = S.ShiftStream(S.ShiftSpec())
    for bad in ("x", (torch.zeros(1),), ([torch.zeros(1)], 0)):
        with pytest.raises(ValueError):
            s(bad)
    b = ([torch.zeros(2, 3, 4, 4), torch.zeros(2, 9), "kept"], torch.zeros(2), "also kept")
    o = s(b)                                  # an empty spec launches nothing: the structure and the counters are all there is to see
    assert type(o) is tuple and type(o[0]) is list and o[0][0] is b[0][0] and o[0][1] is b[0][1] and o[0][2] == "kept" and o[2] == "also kept"
    assert (s.image_drawn, s.table_drawn) == (96, 18)


def test_fit_test_shifts_refuses_bad_protocols_and_shift_tables_before_touching_the_model():
    from stil_tta_amd import fit
    from stil_tta_amd.shift import ShiftSpec
    spec = ShiftSpec(image=("contrast", 2))
    for shifts, protocol in (({"a": spec}, "episodic"), ({}, "reset"), ({"mean": spec}, "reset"), ({"a": ("contrast", 2)}, "continual")):
        with pytest.raises(ValueError):
            fit.test_shifts(None, [], shifts, protocol=protocol)      # model None: anything past the checks would fail otherwise


# ------------------------------------------------------------------------------------------ 2. the C ABI without a device
def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from stil_tta_amd._lib import lib
    L = lib()
    P, Q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20)        # never dereferenced: the checks run before any launch
    inf = math.inf
    with pytest.raises(RuntimeError, match="null pointer or empty"):
        L.shift_noise(None, Q, 16, 0, 0.1, 0.0, 1.0, 1, 0, None)
    with pytest.raises(RuntimeError, match="null pointer or empty"):
        L.shift_noise(P, None, 16, 0, 0.1, 0.0, 1.0, 1, 0, None)
    for n in (0, -4):
        with pytest.raises(RuntimeError, match="null pointer or empty"):
            L.shift_noise(P, Q, n, 0, 0.1, 0.0, 1.0, 1, 0, None)
    with pytest.raises(RuntimeError, match="overlaps"):
        L.shift_noise(P, P, 16, 0, 0.1, 0.0, 1.0, 1, 0, None)
    with pytest.raises(RuntimeError, match="overlaps"):
        L.shift_noise(P, ctypes.c_void_p((1 << 20) + 32), 16, 0, 0.1, 0.0, 1.0, 1, 0, None)
    for kind in (-1, 2):
        with pytest.raises(RuntimeError, match="kind"):
            L.shift_noise(P, Q, 16, kind, 0.1, 0.0, 1.0, 1, 0, None)
    for kind, s in ((0, -0.1), (0, math.nan), (0, inf), (1, 1.5), (1, -0.5)):
        with pytest.raises(RuntimeError, match="strength"):
            L.shift_noise(P, Q, 16, kind, s, 0.0, 1.0, 1, 0, None)
    for lo, hi in ((1.0, 0.0), (math.nan, 1.0), (0.0, math.nan)):
        with pytest.raises(RuntimeError, match="clip range"):
            L.shift_noise(P, Q, 16, 0, 0.1, lo, hi, 1, 0, None)

    W = ctypes.c_void_p(3 << 20)
    for x, o, ws in ((None, Q, W), (P, None, W), (P, Q, None)):
        with pytest.raises(RuntimeError, match="null pointer or empty"):
            L.shift_contrast(x, o, 2, 3, 16, 0.5, 0.0, 1.0, ws, None)
    for B, C, HW in ((0, 3, 16), (-1, 3, 16), (2, 0, 16), (2, 3, 0)):
        with pytest.raises(RuntimeError, match="null pointer or empty"):
            L.shift_contrast(P, Q, B, C, HW, 0.5, 0.0, 1.0, W, None)
    with pytest.raises(RuntimeError, match="overlaps"):
        L.shift_contrast(P, P, 2, 3, 16, 0.5, 0.0, 1.0, W, None)
    for f in (-0.5, math.nan, inf):
        with pytest.raises(RuntimeError, match="factor"):
            L.shift_contrast(P, Q, 2, 3, 16, f, 0.0, 1.0, W, None)
    with pytest.raises(RuntimeError, match="clip range"):
        L.shift_contrast(P, Q, 2, 3, 16, 0.5, 1.0, 0.0, W, None)

    for x, o in ((None, Q), (P, None)):
        with pytest.raises(RuntimeError, match="null pointer or empty"):
            L.shift_brightness(x, o, 2, 3, 16, 0.1, 0.0, 1.0, None)
    for B, HW in ((0, 16), (2, 0)):
        with pytest.raises(RuntimeError, match="null pointer or empty"):
            L.shift_brightness(P, Q, B, 3, HW, 0.1, 0.0, 1.0, None)
    for C in (1, 2, 4):
        with pytest.raises(RuntimeError, match="3 channels"):
            L.shift_brightness(P, Q, 2, C, 16, 0.1, 0.0, 1.0, None)
    with pytest.raises(RuntimeError, match="overlaps"):
        L.shift_brightness(P, P, 2, 3, 16, 0.1, 0.0, 1.0, None)
    for d in (math.nan, inf, -inf):
        with pytest.raises(RuntimeError, match="delta"):
            L.shift_brightness(P, Q, 2, 3, 16, d, 0.0, 1.0, None)
    with pytest.raises(RuntimeError, match="clip range"):
        L.shift_brightness(P, Q, 2, 3, 16, 0.1, math.nan, 1.0, None)

    for x, o in ((None, Q), (P, None)):
        with pytest.raises(RuntimeError, match="null pointer or empty"):
            L.shift_pixelate(x, o, 2, 3, 4, 4, 2, None)
    for B, C, H, Wd in ((0, 3, 4, 4), (2, 0, 4, 4), (2, 3, 0, 4), (2, 3, 4, -1)):
        with pytest.raises(RuntimeError, match="null pointer or empty"):
            L.shift_pixelate(P, Q, B, C, H, Wd, 2, None)
    for s in (0, -2):
        with pytest.raises(RuntimeError, match="at least 1"):
            L.shift_pixelate(P, Q, 2, 3, 4, 4, s, None)
    with pytest.raises(RuntimeError, match="overlaps"):
        L.shift_pixelate(P, P, 2, 3, 4, 4, 2, None)

    CL, ON, SD, FI = (ctypes.c_void_p(k << 20) for k in (4, 5, 6, 7))
    for x, o, on, sd, fi in ((None, Q, ON, SD, FI), (P, None, ON, SD, FI), (P, Q, None, SD, FI), (P, Q, ON, None, FI), (P, Q, ON, SD, None)):
        with pytest.raises(RuntimeError, match="null pointer or empty"):
            L.shift_tab(x, o, 4, 9, 4, CL, on, sd, fi, 0, 0.5, 1, 0, None)
    for B, n in ((0, 9), (-3, 9), (4, 0)):
        with pytest.raises(RuntimeError, match="null pointer or empty"):
            L.shift_tab(P, Q, B, n, 0, CL, ON, SD, FI, 0, 0.5, 1, 0, None)
    for num_cat, cl in ((-1, CL), (10, CL), (4, None)):
        with pytest.raises(RuntimeError, match="num_cat"):
            L.shift_tab(P, Q, 4, 9, num_cat, cl, ON, SD, FI, 0, 0.5, 1, 0, None)
    with pytest.raises(RuntimeError, match="overlaps"):
        L.shift_tab(P, P, 4, 9, 4, CL, ON, SD, FI, 0, 0.5, 1, 0, None)
    for kind in (-1, 3):
        with pytest.raises(RuntimeError, match="kind"):
            L.shift_tab(P, Q, 4, 9, 4, CL, ON, SD, FI, kind, 0.5, 1, 0, None)
    for kind, s in ((0, -1.0), (0, math.nan), (1, 1.5), (2, 1.5), (2, -0.1)):
        with pytest.raises(RuntimeError, match="strength"):
            L.shift_tab(P, Q, 4, 9, 4, CL, ON, SD, FI, kind, s, 1, 0, None)
    assert L.version() == 106


# ------------------------------------------------------------------------------------------ 3. host-side pieces
def test_table_stats_from_table_against_numpy():
    from stil_tta_amd.shift import TableStats
    g = np.random.default_rng(5)
    field_lengths = [3, 1, 4, 1, 1, 2]                     # the reference's list: lengths in column order of the ORIGINAL table
    cat = [3, 4, 2]
    N = 200
    t = np.concatenate([np.stack([g.integers(0, n, N) for n in cat], 1).astype(np.float32), g.normal(size=(N, 3)).astype(np.float32) * 5 + 2], 1)
    t[:, 2] = np.tile([0, 1], N // 2)                      # a tie between codes 0 and 1: the smallest wins
    t[:, 1] = 3.0
    st = TableStats.from_table(torch.from_numpy(t), field_lengths)
    assert st.num_cat == 3 and st.n_cols == 6 and st.cat_len.dtype == torch.int32 and st.cat_len.tolist() == cat
    d = t.astype(np.float64)
    assert np.array_equal(st.col_std.numpy(), d.std(axis=0).astype(np.float32)) and float(st.col_std[1]) == 0.0
    assert np.array_equal(st.col_fill.numpy()[3:], d.mean(axis=0).astype(np.float32)[3:])
    counts0 = np.bincount(t[:, 0].astype(int), minlength=3)
    assert st.col_fill.tolist()[:3] == [float(np.flatnonzero(counts0 == counts0.max())[0]), 3.0, 0.0]
    e = TableStats([3, 4], [1, 1, 0.5], [0, 1, 2.5])       # from explicit vectors
    assert (e.num_cat, e.n_cols) == (2, 3) and e.col_fill.dtype == torch.float32
    bad_code = t.copy()
    bad_code[0, 0] = 3.0
    frac = t.copy()
    frac[0, 0] = 0.5
    for args in ((bad_code, field_lengths), (frac, field_lengths), (t[:, :5], field_lengths), (t[0], field_lengths)):
        with pytest.raises(ValueError):
            TableStats.from_table(torch.from_numpy(np.ascontiguousarray(args[0])), args[1])
    for args in (([0], [1, 1], [0, 0]), ([2], [1, -1], [0, 0]), ([2], [1, 1], [0]), ([2, 2, 2], [1, 1], [0, 0]), ([], [], []), ([2], [1, math.nan], [0, 0])):
        with pytest.raises(ValueError):
            TableStats(*args)


def test_class_ordered_is_a_stable_seeded_permutation_sorted_by_class():
    from stil_tta_amd.shift import class_ordered
    g = torch.Generator().manual_seed(3)
    y = torch.randint(0, 7, (300,), generator=g) * 3 - 4        # labels need not be 0..K-1
    o = class_ordered(y, seed=1)
    assert o.dtype == torch.int64 and sorted(o.tolist()) == list(range(300))
    ys = y[o].tolist()
    blocks = [ys[0]] + [b for a, b in zip(ys, ys[1:]) if a != b]
    assert len(blocks) == len(set(blocks)) == len(set(y.tolist())), "a class shows up in two places"
    for c in set(ys):
        idx = [int(i) for i in o if int(y[i]) == c]
        assert idx == sorted(idx), "not stable within a class"
    assert torch.equal(o, class_ordered(y.numpy(), seed=1))
    orders = {tuple(y[class_ordered(y, seed=s)].unique_consecutive().tolist()) for s in range(8)}
    assert len(orders) > 1, "the seed does not move the class order"


class _Rows:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __call__(self, idx):
        return idx.clone()


def test_index_loader_takes_an_order_and_is_unchanged_without_one():
    from stil_tta_amd.augment import IndexLoader
    from stil_tta_amd.shift import class_ordered
    n = 23
    order = class_ordered(torch.arange(n) % 4, seed=2)
    ld = IndexLoader(_Rows(n), 5, shuffle=True, seed=9, order=order)
    for _ in range(2):                                                     # every epoch, whatever `shuffle` says
        got = list(ld)
        assert len(got) == len(ld) == 5 and [len(b) for b in got] == [5, 5, 5, 5, 3] and torch.equal(torch.cat(got), order)
    assert torch.equal(torch.cat(list(IndexLoader(_Rows(n), 5, drop_last=True, order=order))), order[:20])
    assert torch.equal(torch.cat(list(IndexLoader(_Rows(n), 4, order=order, rank=1, world=2))), torch.cat([order, order[:1]])[1::2])
    for bad in (order[:-1], order.float(), order.view(1, -1), order + 1, order - 1):
        with pytest.raises(ValueError):
            IndexLoader(_Rows(n), 5, order=bad)
    # without an order: arange, or the permutations of a generator seeded with `seed`, one per epoch
    assert torch.equal(torch.cat(list(IndexLoader(_Rows(n), 5, shuffle=False))), torch.arange(n))
    ld, g = IndexLoader(_Rows(n), 5, shuffle=True, seed=9), torch.Generator().manual_seed(9)
    for _ in range(2):
        assert torch.equal(torch.cat(list(ld)), torch.randperm(n, generator=g))
    assert ld.order is None


# ------------------------------------------------------------------------------------------ 4. the model's statistics
def test_model_moments_over_2_to_the_20_draws():
    N = 1 << 20
    for seed in (SC.SEED, 0, 7):
        g = SC.gauss(seed, SC.counters(0, N))
        mean, var = float(g.mean()), float(g.var())
        print(f"seed {seed}: normals mean {mean:+.2e} (bar {5 / math.sqrt(N):.2e}), variance {var:.5f} (bar 1 +- {5 * math.sqrt(2 / N):.2e})")
        assert abs(mean) <= 5 / math.sqrt(N) and abs(var - 1) <= 5 * math.sqrt(2 / N)
        assert np.isfinite(g).all() and float(np.abs(g).max()) <= math.sqrt(48 * math.log(2)) + 1e-12
        x = np.full(N, 0.5, dtype=np.float32)
        for amount in (0.03, 0.27):
            out = SC.noise_model(x, 1, amount, 0.0, 1.0, seed, 0)
            lo, hi = float((out == 0).mean()), float((out == 1).mean())
            se_half, se = math.sqrt(amount / 2 * (1 - amount / 2) / N), math.sqrt(amount * (1 - amount) / N)
            print(f"seed {seed}: impulse {amount}: fraction lo {lo:.5f}, hi {hi:.5f}")
            assert abs(lo - amount / 2) <= 5 * se_half and abs(hi - amount / 2) <= 5 * se_half and abs(lo + hi - amount) <= 5 * se
        t = np.zeros((N // 8, 8), dtype=np.float32)
        for rate in (0.1, 0.7):
            out = SC.tab_model(t, 0, [], np.ones(8), np.ones(8), np.full(8, 9.0), 1, rate, seed, 0)
            frac = float((out == 9).mean())
            print(f"seed {seed}: missing {rate}: fraction {frac:.5f}")
            assert abs(frac - SC.f32(rate)) <= 5 * math.sqrt(rate * (1 - rate) / N)
        cat = np.zeros((N // 8, 8), dtype=np.float32)
        out = SC.tab_model(cat, 8, [5] * 8, np.ones(8), np.ones(8), np.zeros(8), 2, 0.5, seed, 0)
        assert out.max() == 4 and out.min() == 0 and (out == np.floor(out)).all()
        frac = float((out != 0).mean())              # a flip draws code 0 one time in five
        assert abs(frac - 0.5 * 0.8) <= 5 * math.sqrt(0.4 * 0.6 / N)


def test_the_pair_rule_and_the_counters_of_the_model():
    e = SC.counters(2 ** 32 - 5, 12)
    assert int(e[-1]) == 2 ** 32 + 6 and e.dtype == np.uint64
    g = SC.gauss(SC.SEED, e)
    for k in range(0, 11):                            # the two members of a pair lie on one circle: same rho
        if int(e[k]) % 2 == 0:
            j = int(e[k]) >> 1
            u1 = (int(SC.r24(SC.SEED, np.array([2 * j], dtype=np.uint64))[0]) + 1) * 2.0 ** -24
            assert abs(g[k] ** 2 + g[k + 1] ** 2 - (-2 * math.log(u1))) < 1e-12
    # cutting the stream anywhere changes nothing
    whole = SC.noise_model(np.zeros(12, np.float32), 0, 1.0, -SC.INF, SC.INF, 3, 5)
    parts = np.concatenate([SC.noise_model(np.zeros(5, np.float32), 0, 1.0, -SC.INF, SC.INF, 3, 5),
                            SC.noise_model(np.zeros(7, np.float32), 0, 1.0, -SC.INF, SC.INF, 3, 10)])
    assert np.array_equal(whole, parts)
    # the hash is the one of csrc/augment.hip: a value worked out by hand in Python integers
    def h(seed, ctr):
        M = 2 ** 64 - 1
        z = (seed + 0x9E3779B97F4A7C15 * (ctr + 1)) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        return (z >> 16) & 0xFFFFFFFF
    for seed, ctr in ((0, 0), (2024, 12345), (2 ** 63 + 11, 2 ** 40 + 3)):
        assert int(SC.aug_hash(seed, np.array([ctr], dtype=np.uint64))[0]) == h(seed, ctr)


# ------------------------------------------------------------------------------------------ 5. the GPU bar is well-posed
def test_float32_numpy_stays_within_a_quarter_of_tol_of_the_float64_model():
    worst, worst_abs = {}, {}
    for kind, label, fn in SC.arithmetic_cases():
        b, a = fn(np.float64), fn(np.float32)
        assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape and np.isfinite(b).all(), (kind, label)
        scale = float(np.abs(b).max())
        err = np.abs(a.astype(np.float64) - b)
        ratio = float((err / (TOL * (1.0 + np.abs(b) + scale))).max())
        worst[kind] = max(worst.get(kind, 0.0), ratio)
        worst_abs[kind] = max(worst_abs.get(kind, 0.0), float(err.max()))
        assert ratio <= 0.25, (kind, label, ratio)
    g64, g32 = SC.gauss(SC.SEED, SC.counters(0, 1 << 20)), SC.gauss(SC.SEED, SC.counters(0, 1 << 20), np.float32)
    gerr = float(np.abs(g32.astype(np.float64) - g64).max())
    print(f"normals: worst absolute float32 error {gerr:.2e}")
    for kind in worst:
        print(f"{kind}: worst float32 error {worst_abs[kind]:.2e} absolute, {worst[kind]:.3f} of close(TOL={TOL})")
    assert set(worst) == {"gaussian_noise", "contrast", "brightness", "pixelate", "tab_noise"}
    assert gerr <= 5e-6
