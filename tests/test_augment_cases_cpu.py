"""CPU side of tests/test_gpu_augment_kernels.py.  Conditioning: over every float case of tests/augment_cases.py the fp32
restatement of each kernel passes, against the float64 reference, the very check the GPU test applies (`augment_cases.check`);
its largest error is the constant E_* written there (measured here, printed with -s), the GPU allowance is 4 times that and stays
below 1e-4.  Reach: the tables hold the pixel counts, box kinds, sigmas, angles, sectors and planted pixels they name; every
clamped box lies inside its image; the narrow rotations reach taps several periods outside the image on both sides.  Refusals:
the seven entry points of csrc/augment.hip turn down bad arguments before any launch -- only refused argument combinations are
passed, with addresses nothing dereferences, which is why they live here and not in the GPU module."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_cases as A  # noqa: E402

BASE = 1 << 20


def fake(off=0):
    return ctypes.c_void_p(BASE + 256 * off)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as E
    E.build()
    from stil_tta_amd._lib import lib
    return lib()


# ---------------------------------------------------------------------------------------------------------------------
# the float cases: (kind, what, fp32 restatement, float64 reference) of every case the GPU module runs
# ---------------------------------------------------------------------------------------------------------------------
def _gray_mean_cases():
    for H, W in A.GM_SHAPES:
        for fmt in A.FMTS:
            img = A.gm_image(fmt, H, W)
            for br in (None, np.array(A.GM_BRIGHTNESS, dtype=np.float32)):
                yield (fmt, H, W, br is not None), A.gray_mean_restate(img, br), A.gray_mean_reference(img, br)


def _resize_cases():
    for H, W in A.RS_SOURCES:
        for P in A.RS_PS:
            for fmt in A.FMTS:
                img, boxes = A.resize_source(fmt, H, W), A.resize_boxes(H, W)
                for flip in (None, np.ones(6, np.uint8)):
                    yield (fmt, H, W, P, flip is not None), A.resize_restate(img, boxes, P, flip), A.resize_reference(img, boxes, P, flip)
    H, W, P = A.RS_BAD_SHAPE
    bad = np.array(A.RS_BAD_BOXES, dtype=np.int32)
    for fmt in A.FMTS:
        img = A.image(fmt, len(bad), H, W, 32)
        yield (fmt, "bad boxes"), A.resize_restate(img, bad, P), A.resize_reference(img, bad, P)


def _colour_cases():
    for H, W, P in A.RS_JITTER_SHAPES:
        for fmt in A.FMTS:
            img, boxes = A.resize_source(fmt, H, W)[:3], A.resize_boxes(H, W)[[0, 4, 5]]
            for jit in A.RS_JITTERS + ((A.IDENTITY_JITTER,) * 3,):
                jit = np.array(jit, dtype=np.float32)
                gm = A.jitter_gmean(img, jit)
                flip = np.array([0, 1, 0], np.uint8)
                yield (fmt, H, W, P, jit.tolist()), A.resize_restate(img, boxes, P, flip, jit, gm), A.resize_reference(img, boxes, P, flip, jit, gm)


def _blur_cases():
    for H, W, k in A.BL_GEOMS:
        for fmt in A.FMTS:
            img = A.image(fmt, 3, H, W, 33)
            for sigma in A.BL_SIGMAS:
                yield (fmt, H, W, k, sigma), A.blur_restate(img, sigma, k), A.blur_reference(img, sigma, k)


def _rotate_cases():
    for H, W in A.RT_SHAPES:
        for fmt in A.FMTS:
            img = A.image(fmt, 3, H, W, 34)
            for ang in A.RT_ANGLES:
                yield (fmt, H, W, ang), A.rotate_restate(img, ang), A.rotate_reference(img, ang)


def _hue_cases():
    for H, W in A.HUE_SHAPES:
        img = A.hue_image(H, W)
        for hue, gr in A.HUE_CALLS:
            yield (H, W, hue, gr), A.hue_restate(img, hue, gr), A.hue_reference(img, hue, gr)


FLOAT_KINDS = {"gray_mean": (_gray_mean_cases, "E_GRAY_MEAN"), "resize": (_resize_cases, "E_RESIZE"), "colour": (_colour_cases, "E_COLOUR"),
               "blur": (_blur_cases, "E_BLUR"), "rotate": (_rotate_cases, "E_ROTATE"), "hue": (_hue_cases, "E_HUE")}


@pytest.mark.parametrize("kind", sorted(FLOAT_KINDS))
def test_measured_errors_are_the_constants(kind):
    """the fp32 restatement meets the GPU check on every case; its largest error is the constant (within a factor 2 below it:
    a constant may be rounded up, not inflated); 4 times the constant is the allowance and stays under the cap"""
    cases, name = FLOAT_KINDS[kind]
    E = getattr(A, name)
    worst, where, n = 0.0, None, 0
    for what, restated, ref in cases():
        assert ref.dtype == np.float64 and restated.dtype == np.float32 and bool(np.isfinite(ref).all())
        err = A.check(kind, restated, ref, what)
        n += 1
        if err > worst:
            worst, where = err, what
    print(f"{kind}: measured {worst:.3e} at {where} over {n} cases; {name} = {E:.3e}; allowance {A.TOL[kind]:.3e}")
    assert 0.5 * E <= worst <= E, f"{name} = {E:.3e} but the measured error is {worst:.3e} (at {where})"
    assert A.TOL[kind] == A.ALLOW * E and A.ALLOW == 4.0
    assert A.TOL[kind] < A.CAP == 1e-4, "a case that needs more is badly conditioned: change the case, not the bound"
    assert A.CAP < 1.0 / 255.0 / 10, "one mis-indexed uint8 pixel is far outside every allowance"


# ---------------------------------------------------------------------------------------------------------------------
# the tables hold what they name
# ---------------------------------------------------------------------------------------------------------------------
def test_tab_cases_are_well_formed_and_reach_past_one_wave():
    assert {n for _, n, _, _ in A.TAB_TABLE} == {1, 63, 64, 65, 200} and {B for B, _, _, _ in A.TAB_TABLE} == {1, 5}
    assert {N for _, _, N, _ in A.TAB_TABLE} == {1, 37}
    assert A.tab_ks(1) == [0, 1] and A.tab_ks(63) == [0, 1, 63] and A.tab_ks(64) == [0, 1, 64] and A.tab_ks(65) == [0, 1, 64, 65]
    assert A.tab_ks(200) == [0, 1, 64, 65, 200]
    assert any(k > 64 for _, _, _, k in A.TAB_TABLE) and any(k == n > 64 for _, n, _, k in A.TAB_TABLE)
    for B, n, N, k in A.TAB_TABLE:
        c = A.tab_case(B, n, N, k)
        assert c["idx"].shape == c["pos"].shape == (B, k) and c["idx"].dtype == c["pos"].dtype == np.int32
        assert all(len(set(r.tolist())) == k for r in c["idx"]), "the columns of one row are distinct (the contract)"
        assert k == 0 or (0 <= c["idx"].min() and c["idx"].max() < n and 0 <= c["pos"].min() and c["pos"].max() < N)
        m = c["marginal"]
        assert m.shape == (n, N) and len(np.unique(m)) == n * N and np.array_equal(np.floor(m / 1000), np.arange(n)[:, None].repeat(N, 1))
        assert np.array_equal(m - 1000 * np.floor(m / 1000), np.arange(N)[None, :].repeat(n, 0) + 0.5), "entry (c, r) encodes c and r"
        ref = A.tab_reference(c)
        assert int((ref != c["clean"]).sum()) == B * k and bool((c["clean"] < 0).all()) and bool((m > 0).all())
        assert k < n or bool((ref > 0).all()), "k == n_cols: every entry comes from the table"


def test_gray_mean_cases_reach_the_launch_edges_and_the_clamp():
    assert [H * W for H, W in A.GM_SHAPES] == [1, 15, 255, 256, 257, 1000]
    assert A.GM_BRIGHTNESS == (0.0, 0.4, 1.8) and np.array_equal(A.gm_jitter()[:, 1:], np.full((3, 3), A.GM_JUNK, np.float32))
    big = A.gm_image("f32", 25, 40)
    assert float(big.min()) < 0.0 and float(big.max()) > 1.0, "a float source outside [0, 1]"
    u8 = A.gm_image("u8", 25, 40)
    assert float((A.src64(u8) * 1.8).max()) > 1.0, "brightness 1.8 makes the clamp active"
    ref = A.gray_mean_reference(u8, np.array(A.GM_BRIGHTNESS, np.float32))
    assert ref[0] == 0.0 and 0.1 < ref[1] < ref[2] < 1.0
    assert not np.array_equal(A.gray_mean_reference(big), A.gray_mean_reference(np.clip(big, 0.2, 0.8)))


def test_resize_boxes_are_what_they_are_named_for():
    assert sorted(P * P for P in A.RS_PS) == [1, 225, 256, 289]
    for H, W in A.RS_SOURCES:
        bx = A.resize_boxes(H, W)
        assert len(bx) == len(A.RS_BOX_NAMES) == 6
        for b in bx:
            t, l, h, w = (int(v) for v in b)
            assert t >= 0 and l >= 0 and h >= 1 and w >= 1 and t + h <= H and l + w <= W
            assert A.clamp_box(b, H, W) == (t, l, h, w), "the clamp is the identity on a valid box"
        assert tuple(bx[0]) == (0, 0, H, W) and tuple(bx[1]) == (H - 1, W - 1, 1, 1) and bx[2][3] == 1 and bx[2][2] == H and bx[3][2] == 1 and bx[3][3] == W
        assert bx[4][0] + bx[4][2] == H and bx[4][1] + bx[4][3] == W
        t, l, h, w = (int(v) for v in bx[5])
        if H >= 3:
            assert t >= 1 and t + h < H and h < min(p for p in A.RS_PS if p > 1), "interior and upsampled"
        if W >= 3:
            assert l >= 1 and l + w < W and w < min(p for p in A.RS_PS if p > 1)
        for fmt in A.FMTS:
            s = A.src64(A.resize_source(fmt, H, W))[5]
            inside = np.zeros((H, W), bool)
            inside[t:t + h, l:l + w] = True
            assert bool((s[:, inside] == 1.0).all()) and bool((s[:, ~inside] == 0.0).all())
            # a neighbour read from outside the crop would show: the reference of that box is full scale everywhere
            assert float(np.abs(A.resize_reference(A.resize_source(fmt, H, W)[5:], bx[5:], 17) - 1.0).max()) < 1e-12
    assert any(H >= 3 and W >= 3 for H, W in A.RS_SOURCES)


def test_bad_boxes_are_bad_and_clamp_into_the_image():
    H, W, _ = A.RS_BAD_SHAPE
    kinds = set()
    for b in A.RS_BAD_BOXES:
        t, l, h, w = b
        assert not (t >= 0 and l >= 0 and h > 0 and w > 0 and t + h <= H and l + w <= W), b
        kinds |= {"negative"} if t < 0 or l < 0 else set()
        kinds |= {"empty"} if h <= 0 or w <= 0 else set()
        kinds |= {"past the border"} if 0 <= t < H and 0 <= l < W and (t + h > H or l + w > W) else set()
        kinds |= {"top at H"} if t == H else set()
        kinds |= {"top beyond H"} if t > H else set()
        kinds |= {"left at W"} if l == W else set()
        ct, cl, ch, cw = A.clamp_box(b, H, W)
        assert 0 <= ct < H and 0 <= cl < W and ch >= 1 and cw >= 1 and ct + ch <= H and cl + cw <= W, (b, (ct, cl, ch, cw))
    assert kinds == {"negative", "empty", "past the border", "top at H", "top beyond H", "left at W"}
    assert len(A.RS_BAD_BOXES) % 3 == 0


def test_jitter_batches_hold_each_factor_alone_and_all_at_once():
    rows = [r for batch in A.RS_JITTERS for r in batch]
    for col in range(3):
        for v in (0.0, 1.8):
            want = list(A.IDENTITY_JITTER)
            want[col] = v
            assert tuple(want) in rows, want
    assert any(all(r[i] != A.IDENTITY_JITTER[i] for i in range(4)) and r[3] == 1.0 for r in rows), "all four at once, gray = 1"
    assert all(len({tuple(r) for r in batch}) == 3 for batch in A.RS_JITTERS), "every sample of a batch has its own factors"


def test_blur_cases_reach_the_largest_radius_underflow_and_a_flat_kernel():
    assert {k for _, _, k in A.BL_GEOMS} == {3, 29, 63}
    assert any(k // 2 == H - 1 < W - 1 for H, W, k in A.BL_GEOMS) and any(k // 2 == W - 1 < H - 1 for H, W, k in A.BL_GEOMS)
    assert all(k // 2 < min(H, W) for H, W, k in A.BL_GEOMS) and (32, 33, 63) in A.BL_GEOMS
    assert {H * W for H, W, _ in A.BL_GEOMS} >= {255, 256, 172} and {s for t in A.BL_SIGMAS for s in t} == {-1.0, 0.0, 0.05, 0.1, 0.9, 2.0, 50.0}
    for k in (3, 29, 63):
        w = A.blur_weights(k, 0.05, np.float32)
        assert w[k // 2] == 1.0 and float(np.abs(w).sum()) == 1.0, "sigma 0.05: the side weights underflow to 0, the row stays finite"
        assert float(A.blur_weights(k, 0.1, np.float32)[k // 2 + 1]) > 0.0, "sigma 0.1: they do not"
        flat = A.blur_weights(k, 50.0, np.float64)
        assert float(flat.min() / flat.max()) > 0.8
        for s in (-1.0, 0.0):
            assert np.array_equal(A.blur_weights(k, s, np.float32), (np.arange(k) == k // 2).astype(np.float32))
    u8 = A.image("u8", 3, 15, 40, 33)
    got = A.blur_restate(u8, (0.05, -1.0, 0.0), 29)
    assert np.array_equal(got, A.raw32(u8) * A.INV255), "a copy of a uint8 source is v * fp32(1 / 255), exactly"


def test_rotations_of_narrow_images_reach_taps_periods_outside_on_both_sides():
    assert set(A.RT_ANGLE_SET) == {a for t in A.RT_ANGLES for a in t} and len(A.RT_ANGLE_SET) == 11
    for (H, W), axis in (((2, 50), 1), ((50, 2), 0)):
        for ang in (90.0, -90.0):
            flx, fly, _, _ = A.rotate_taps(H, W, ang)
            i, n = (fly, H) if axis == 1 else (flx, W)
            period = 2 * n - 2
            assert n == 2 and period == 2
            assert int(i.min()) < -period and int(i.max()) + 1 >= n + period, "more than one period outside, on both sides"
            assert int(np.fmod(i.min(), period)) <= 0 and int(i.min()) % period >= 0, "C's % is negative there, Python's is not"
    for H, W in ((1, 1), (1, 7), (7, 1)):
        for ang in A.RT_ANGLE_SET:
            flx, fly, _, _ = A.rotate_taps(H, W, ang)
            i, n = (fly, H) if H == 1 else (flx, W)
            assert n == 1 and bool((A.reflect101(i, n) == 0).all()) and bool((A.reflect101(i + 1, n) == 0).all())
        # without the n == 1 rule the period is 0: the one-wide cases exist to take that rule with taps off pixel 0
        flx, fly, _, _ = A.rotate_taps(H, W, 45.0)
        assert (H * W == 1) or int(np.abs(fly if H == 1 else flx).max()) >= 1
    assert {H * W for H, W in A.RT_SHAPES} >= {1, 7, 100, 255, 256, 258, 1961}
    img = A.image("u8", 3, 15, 17, 34)
    assert np.array_equal(A.rotate_restate(img, (0.0, 0.0, 0.0)), A.raw32(img) * A.INV255), "angle 0 copies: v * fp32(1 / 255)"


def test_hue_cases_reach_every_sector_the_wrap_and_the_planted_pixels():
    sectors, wrapped_below, wrapped_above = set(), False, False
    for H, W in A.HUE_SHAPES:
        img = A.hue_image(H, W)
        for hue, _ in A.HUE_CALLS:
            for b in range(3):
                if hue is not None and hue[b] != 0.0:
                    _, i, moved = A.hue_steps(img[b].astype(np.float64), hue[b])
                    sectors |= set(np.unique(i).tolist())
                    wrapped_below |= bool((moved < 0).any())
                    wrapped_above |= bool((moved >= 1).any())
    assert sectors == {0, 1, 2, 3, 4, 5} and wrapped_below and wrapped_above
    assert {h for hue, _ in A.HUE_CALLS if hue for h in hue} == set(A.HUE_SET)
    assert any(hue is None and gr is not None for hue, gr in A.HUE_CALLS) and any(gr is None for _, gr in A.HUE_CALLS)
    assert {g for _, gr in A.HUE_CALLS if gr for g in gr} == {0.0, 1.0}
    assert any(hue and gr and any(h == 0.0 and g == 0.0 for h, g in zip(hue, gr)) for hue, gr in A.HUE_CALLS)
    P = A.HUE_PLANTS
    assert (0.0, 0.0, 0.0) in P and (1.0, 1.0, 1.0) in P and any(p[0] == p[1] == p[2] and 0 < p[0] < 1 for p in P)
    assert {(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)} <= set(P)
    ties = [p for p in P if sorted(p)[1] == sorted(p)[2] != sorted(p)[0]]
    assert len(ties) >= 3 and {tuple(np.argsort(p)[:1]) for p in ties} == {(0,), (1,), (2,)}, "each pair of channels ties at the top"
    # primaries and secondaries shifted by half a turn land on a sector boundary: h * 6 is an integer up to its rounding, so
    # fp32 and float64 may pick different sectors there -- and must still agree on the colour
    sides = set()
    for p in P[3:9]:
        x = np.array(p, dtype=np.float64).reshape(3, 1)
        _, _, moved = A.hue_steps(x, 0.5)
        h6 = float(moved[0] * 6)
        assert abs(h6 - round(h6)) < 1e-12, p
        sides.add(h6 < round(h6))
    assert sides == {True, False}, "some land a rounding below the boundary, some on it"
    img = A.hue_image(20, 24)
    assert all(tuple(img[0, :, 0, p].tolist()) == tuple(np.float32(P[p]).tolist()) for p in range(len(P)))
    assert tuple(A.hue_image(1, 1)[1, :, 0, 0].tolist()) == P[4] and [H * W for H, W in A.HUE_SHAPES] == [1, 255, 256, 480]
    grey = A.hue_reference(img, (0.07, 0.07, 0.07), None)[0, :, 0, 0]
    assert tuple(grey.tolist()) == tuple(float(np.float32(v)) for v in P[0]), "a grey pixel does not move"


def test_part_b_tables_hold_what_they_name():
    assert [H * W for H, W in A.ALB_NPIX] == [1, 3, 4, 5, 1023, 1024, 1025] and all(n % 4 == 0 for n in A.ALB_MISALIGNED)
    assert A.ALB_WG == ((256, 256), (5, 5)) and -(-((256 * 256 + 3) // 4) // 256) >= 64 and -(-((5 * 5 + 3) // 4) // 256) == 1
    assert {W for _, W in A.ALB_BLUR_TILE} == {31, 32, 33} and {H for H, _ in A.ALB_BLUR_TILE} == {15, 16, 17}
    assert all(min(H, W) < 29 // 2 for H, W in A.ALB_BLUR_SHORT)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: every call below fails the entry point's STIL_REQUIRE on the host; none reaches a launch
# ---------------------------------------------------------------------------------------------------------------------
def _refused(call, match):
    with pytest.raises(RuntimeError, match=match):
        call()


def _f(on, off):
    return fake(off) if on else None


SOURCES = (dict(u8=True, f32=True), dict(u8=False, f32=False))       # both source pointers set / neither
SHAPES = tuple({n: v} for n in ("B", "H", "W") for v in (0, -1))


def test_tab_corrupt_refuses_before_any_launch(L):
    def call(clean=True, marginal=True, idx=True, pos=True, out=True, B=2, n_cols=8, n_rows=5, k=3):
        return lambda: L.tab_corrupt(_f(clean, 0), _f(marginal, 1), _f(idx, 2), _f(pos, 3), _f(out, 4), B, n_cols, n_rows, k, None)
    for kw in (dict(clean=False), dict(marginal=False), dict(out=False), dict(B=0), dict(B=-1), dict(n_cols=0, k=0), dict(n_cols=-1, k=0),
               dict(n_rows=0), dict(n_rows=-2)):
        _refused(call(**kw), "stil_tab_corrupt: null pointer or empty shape")
    for kw in (dict(k=-1), dict(k=9), dict(k=9, n_cols=8), dict(idx=False), dict(pos=False), dict(idx=False, pos=False, k=1), dict(k=8, pos=False)):
        _refused(call(**kw), "stil_tab_corrupt: k=-?[0-9]+ outside .* or missing draws")


def test_gray_mean_refuses_before_any_launch(L):
    def call(u8=True, f32=False, gmean=True, B=2, H=4, W=5):
        return lambda: L.aug_gray_mean(_f(u8, 0), _f(f32, 1), None, _f(gmean, 2), B, H, W, 1.0, None)
    for kw in SOURCES + (dict(gmean=False),) + SHAPES:
        _refused(call(**kw), "stil_aug_gray_mean: bad arguments")


def test_resize_refuses_before_any_launch(L):
    def call(u8=False, f32=True, box=True, jitter=False, gmean=False, out=True, B=2, H=4, W=5, P=3):
        return lambda: L.aug_resize(_f(u8, 0), _f(f32, 1), _f(box, 2), None, _f(jitter, 3), _f(gmean, 4), _f(out, 5), B, H, W, P, 1.0, None)
    for kw in SOURCES:
        _refused(call(**kw), "stil_aug_resize: exactly one of src_u8 / src_f32")
    for kw in (dict(box=False), dict(out=False), dict(P=0), dict(P=-1)) + SHAPES:
        _refused(call(**kw), "stil_aug_resize: null pointer or empty shape")
    _refused(call(jitter=True), "stil_aug_resize: colour jitter needs gmean")
    _refused(call(jitter=True, u8=True, f32=False), "stil_aug_resize: colour jitter needs gmean")


def test_blur_refuses_before_any_launch(L):
    def call(u8=True, f32=False, sigma=True, tmp=True, out=True, B=2, H=40, W=40, ksize=29):
        return lambda: L.aug_blur(_f(u8, 0), _f(f32, 1), _f(sigma, 2), _f(tmp, 3), _f(out, 4), B, H, W, ksize, 1.0, None)
    for kw in SOURCES + (dict(sigma=False), dict(tmp=False), dict(out=False), dict(B=0), dict(B=-1)):
        _refused(call(**kw), "stil_aug_blur: bad arguments")
    for kw in (dict(ksize=4), dict(ksize=28), dict(ksize=1), dict(ksize=65), dict(ksize=-3), dict(ksize=0),
               dict(H=14), dict(W=14), dict(H=14, W=14), dict(ksize=63, H=31), dict(ksize=63, W=31), dict(ksize=3, H=1), dict(ksize=3, W=1),
               dict(H=0), dict(H=-1), dict(W=0), dict(W=-1)):
        _refused(call(**kw), "stil_aug_blur: kernel size -?[0-9]+ must be odd")


def test_rotate_refuses_before_any_launch(L):
    def call(u8=True, f32=False, angle=True, out=True, B=2, H=4, W=5):
        return lambda: L.aug_rotate(_f(u8, 0), _f(f32, 1), _f(angle, 2), _f(out, 3), B, H, W, 1.0, None)
    for kw in SOURCES + (dict(angle=False), dict(out=False)) + SHAPES:
        _refused(call(**kw), "stil_aug_rotate: bad arguments")


def test_hue_refuses_before_any_launch(L):
    def call(img=True, hue=True, gray=True, B=2, H=4, W=5):
        return lambda: L.aug_hue(_f(img, 0), _f(hue, 1), _f(gray, 2), B, H, W, None)
    for kw in (dict(img=False), dict(hue=False, gray=False), dict(img=False, hue=False)) + SHAPES:
        _refused(call(**kw), "stil_aug_hue: bad arguments")
