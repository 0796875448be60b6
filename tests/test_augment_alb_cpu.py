"""The albumentations branch of the input pipeline without a GPU (stil_tta_amd/augment.py, augmentation_speedup=True): the
policy table against utils/utils.py:46-256, the statistics of the host draws, the loaders' selection of the branch, the input
formats it refuses, and the argument checks of the stil_alb_* entry points."""
import os
import sys
from itertools import permutations

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

R = (0.75, 4.0 / 3.0)


def _cj(a, hue, p):
    return ("cj", dict(brightness=a, contrast=a, saturation=a, hue=hue, p=p))


FLIP, GRAY, TT = ("flip", dict(p=0.5)), ("gray", dict(p=0.2)), ("to_tensor", {})
EXPECTED = {
    ("contrastive", True): [_cj(0.8, 0.2, 0.8), GRAY, ("blur", dict(k=29, sigma=(0.1, 2.0), p=0.5)), ("rrc", dict(scale=(0.08, 1.0), ratio=R)), FLIP, TT],
    ("contrastive", False): [FLIP, ("rotate", dict(limit=45.0, p=0.5)), _cj(0.5, 0.2, 0.5), ("rrc", dict(scale=(0.2, 1.0), ratio=R)), TT],
    ("hard_eval", True): [_cj(0.8, 0.2, 0.8), GRAY, ("blur", dict(k=29, sigma=(0.1, 2.0), p=0.5)), ("rrc", dict(scale=(0.6, 1.0), ratio=R)), FLIP, TT],
    ("hard_eval", False): [FLIP, ("rotate", dict(limit=45.0, p=0.5)), _cj(0.5, 0.2, 0.5), ("rrc", dict(scale=(0.6, 1.0), ratio=R)), TT],
    ("soft_eval", True): [FLIP, ("rotate", dict(limit=20.0, p=0.5)), _cj(0.25, 0.2, 0.5), ("rrc", dict(scale=(0.8, 1.0), ratio=R)), TT],
    ("soft_eval", False): [FLIP, ("rotate", dict(limit=20.0, p=0.5)), _cj(0.25, 0.2, 0.5), ("rrc", dict(scale=(0.8, 1.0), ratio=R)), TT],
    ("weak", True): [("rrc", dict(scale=(0.2, 1.0), ratio=R)), FLIP, TT],
    ("weak", False): [("rrc", dict(scale=(0.2, 1.0), ratio=R)), FLIP, TT],
    ("strong", True): [("rrc", dict(scale=(0.2, 1.0), ratio=R)), FLIP, _cj(0.4, 0.1, 0.8), GRAY, ("blur", dict(k=19, sigma=(0.1, 2.0), p=0.5)), TT],
    ("strong", False): [("rrc", dict(scale=(0.2, 1.0), ratio=R)), FLIP, _cj(0.4, 0.1, 0.8), ("blur", dict(k=19, sigma=(0.1, 2.0), p=0.5)), TT],
    ("default", True): [("resize", {}), TT],
    ("default", False): [("resize", {}), TT],
}


@pytest.mark.parametrize("kind,dvm", sorted(EXPECTED))
def test_alb_policy_equals_the_reference_table(kind, dvm):
    from stil_tta_amd.augment import _alb_policy
    got = _alb_policy(kind, dvm, 0.08)
    exp = EXPECTED[(kind, dvm)]
    assert [n for n, _ in got] == [n for n, _ in exp]
    for (n, g), (_, e) in zip(got, exp):
        assert g.keys() == e.keys(), n
        for k in e:
            assert np.allclose(g[k], e[k], rtol=0, atol=1e-12), (n, k, g[k], e[k])


def test_alb_policy_crop_scale_lower_reaches_the_dvm_contrastive_crop_only():
    from stil_tta_amd.augment import _alb_policy
    assert dict(_alb_policy("contrastive", True, 0.3))["rrc"]["scale"] == (0.3, 1.0)
    assert dict(_alb_policy("hard_eval", True, 0.3))["rrc"]["scale"] == (0.6, 1.0)
    assert dict(_alb_policy("contrastive", False, 0.3))["rrc"]["scale"] == (0.2, 1.0)
    with pytest.raises(ValueError, match="unknown transform family"):
        _alb_policy("mixup", True)


B_STAT = 20000


@pytest.mark.parametrize("kind,dvm", [("contrastive", True), ("contrastive", False), ("soft_eval", True), ("strong", True), ("strong", False),
                                      ("hard_eval", False)])
def test_alb_draw_statistics(kind, dvm):
    from stil_tta_amd.augment import ImageAugmenter, _alb_policy
    rate = 0.95
    aug = ImageAugmenter(64, "dvm" if dvm else "CAD", rate, seed=5, kind=kind, augmentation_speedup=True)
    H, W = 96, 80
    d = aug.draw(B_STAT, H, W)
    stages = dict(_alb_policy(kind, dvm))
    a = d["aug"]
    assert abs(a.mean() - rate) < 0.01
    cj = stages["cj"]
    on = d["cj_on"].astype(bool)
    assert not on[~a].any()
    assert abs(on.mean() - cj["p"] * rate) < 0.01
    f = d["factors"][on]
    for i, k in enumerate(("brightness", "contrast", "saturation")):
        assert f[:, i].min() >= max(0.0, 1 - cj[k]) and f[:, i].max() <= 1 + cj[k]
    assert np.abs(f[:, 3]).max() <= cj["hue"] and np.abs(f[:, 3]).max() > 0.9 * cj["hue"]   # hue shifts: hue=0.2 where the reference leaves it default
    assert (d["factors"][~on] == [1, 1, 1, 0]).all()
    orders = [tuple(o) for o in d["order"][on]]
    freq = {p: orders.count(p) / len(orders) for p in permutations(range(4))}
    assert len(freq) == 24 and all(abs(v - 1 / 24) < 0.005 for v in freq.values()), freq
    if "rotate" in stages:
        r = d["rot_on"].astype(bool)
        assert abs(r.mean() - 0.5 * rate) < 0.01
        assert np.abs(d["angle"][r]).max() <= stages["rotate"]["limit"] and (d["angle"][~r] == 0).all()
        assert abs(d["flip_first"].mean() - 0.5 * rate) < 0.01 and not d["flip"].any()      # the flip precedes the rotation
    else:
        assert abs(d["flip"].mean() - 0.5 * rate) < 0.01 and not d["flip_first"].any()
    if "gray" in stages:
        assert abs(d["gray_on"].mean() - 0.2 * rate) < 0.01
    if "blur" in stages:
        s = d["sigma"]
        assert abs((s > 0).mean() - 0.5 * rate) < 0.01 and s[s > 0].min() >= 0.1 and s.max() <= 2.0
    bx = d["boxes"]
    t, l, h, w = bx.T.astype(np.int64)
    assert (t >= 0).all() and (l >= 0).all() and (h > 0).all() and (w > 0).all() and (t + h <= H).all() and (l + w <= W).all()
    assert (bx[~a] == [0, 0, H, W]).all()
    lo = stages["rrc"]["scale"][0]
    h, w = h[a], w[a]     # w, h are the rounded sqrt(area * ratio), sqrt(area / ratio): bounds widen by half a pixel
    assert ((h + 0.5) * (w + 0.5) >= lo * H * W).all() and (h * w <= H * W).all()
    assert ((w + 0.5) / (h - 0.5) >= 0.75).all() and ((w - 0.5) / (h + 0.5) <= 4 / 3).all()


def test_alb_draws_of_the_default_mode_are_unchanged():
    from stil_tta_amd.augment import ImageAugmenter
    a = ImageAugmenter(64, "dvm", 0.95, seed=3).draw(16, 96, 80)
    assert set(a) == {"boxes", "flip", "aug", "jitter", "sigma"}


def _hp(**kw):
    d = dict(algorithm_name="STiL", img_size=32, target="dvm", corruption_rate=0.3, batch_size=16, unlabelled_ratio=3, seed=1)
    d.update(kw)
    return d


def _data(N, fmt):
    g = torch.Generator().manual_seed(0)
    if fmt == "u8":
        im = torch.randint(0, 256, (N, 40, 36, 3), generator=g, dtype=torch.uint8)
    elif fmt == "f32hwc":
        im = torch.rand(N, 40, 36, 3, generator=g)
    else:
        im = torch.rand(N, 3, 40, 36, generator=g)
    return im, torch.randn(N, 6, generator=g), torch.randint(0, 2, (N,), generator=g)


@pytest.mark.parametrize("algo", ["STiL", "CoMatch", "SimMatch"])
def test_semisl_loaders_select_the_albumentations_branch(algo):
    from stil_tta_amd.augment import semisl_loaders
    for key, fmt in ((True, "u8"), (False, "u8"), (None, "f32chw")):
        hp = _hp(algorithm_name=algo)
        if key is not None:
            hp["augmentation_speedup"] = key
        ld = semisl_loaders(hp, _data(8, fmt), _data(24, fmt), device="cpu")
        for part in ("l", "u"):
            b = ld[part].builder
            augs = [getattr(b, n) for n in ("augment", "weak", "strong") if hasattr(b, n)]
            assert augs and all(a.alb == bool(key) for a in augs), (algo, key, part)
    hp = _hp(algorithm_name=algo, augmentation_speedup=True, target="CAD")
    ld = semisl_loaders(hp, _data(8, "f32hwc"), _data(24, "f32hwc"), device="cpu")
    assert ld["l"].builder.images.shape[-1] == 3


def test_float_chw_is_refused_in_albumentations_mode_only():
    from stil_tta_amd.augment import ContrastiveBatchBuilder, EvalTrainBatchBuilder, StrongWeakBatchBuilder
    im, tab, y = _data(8, "f32chw")
    for cls in (ContrastiveBatchBuilder, EvalTrainBatchBuilder, StrongWeakBatchBuilder):
        with pytest.raises(ValueError, match="float CHW"):
            cls(im, tab, y, 32, target="CAD", device="cpu", augmentation_speedup=True)
        cls(im, tab, y, 32, target="CAD", device="cpu")     # the default mode keeps taking it
    with pytest.raises(ValueError, match="HWC"):
        ContrastiveBatchBuilder(im.double().permute(0, 2, 3, 1), tab, y, 32, device="cpu", augmentation_speedup=True)


def test_rotation_matrix_matches_the_restatement():
    import alb_restate as RS
    from stil_tta_amd.augment import alb_rotation_matrix
    ang = np.array([0.0, 17.3, -44.9, 90.0, 1e-7])
    M = alb_rotation_matrix(ang, 37, 52)
    for i, a in enumerate(ang):
        assert np.array_equal(M[i], RS.rotation_matrix(float(a), 37, 52))
    assert np.allclose(M[0], [1, 0, 0, 0, 1, 0], atol=1e-15)


def test_restatement_identities():
    import alb_restate as RS
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    f = rng.random((9, 11, 3), dtype=np.float32)
    for img in (u8, f):
        assert RS.color_jitter(img, [0, 1, 2, 3], [1.0, 1.0, 1.0, 0.0]) is img
        assert np.array_equal(RS.rotate(img, 0.0), img)
        assert np.array_equal(RS.resize_crop(img, (0, 0, 9, 9), 9), img[:, :9])
        assert np.array_equal(RS.gaussian_blur(img, 29, 0.0), img)
    assert np.array_equal(RS.to_tensor(u8), (u8.transpose(2, 0, 1) / 255.0).astype(np.float32))
    # hue of a grey pixel is undefined: a pure grey image comes back unchanged
    g = np.full((2, 2, 3), 77, np.uint8)
    assert np.array_equal(RS.hue(g, 0.13), g)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    import ctypes
    from stil_tta_amd._lib import lib
    L = lib()
    P = ctypes.c_void_p(64)        # never dereferenced: the checks run before any launch
    with pytest.raises(RuntimeError, match="null image pointer"):
        L.alb_color(None, None, None, None, 2, 8, 8, P, P, P, P, P, 0, None)
    with pytest.raises(RuntimeError, match="null image pointer"):
        L.alb_color(P, None, None, None, 2, 8, 8, P, P, P, P, P, 0, None)
    with pytest.raises(RuntimeError, match="wg_per_image"):
        L.alb_color(P, None, P, None, 2, 8, 8, P, P, P, P, P, 65, None)
    for k in (0, -3, 4, 28):
        with pytest.raises(RuntimeError, match="must be odd, positive"):
            L.alb_blur(P, None, ctypes.c_void_p(128), None, 2, 8, 8, P, k, None)
    with pytest.raises(RuntimeError, match="null image pointer"):
        L.alb_blur(None, P, None, None, 2, 8, 8, P, 29, None)
    for p in (0, -1):
        with pytest.raises(RuntimeError, match="must be positive"):
            L.alb_resize(P, None, None, None, ctypes.c_void_p(128), 2, 8, 8, P, None, p, None)
    with pytest.raises(RuntimeError, match="null image pointer"):
        L.alb_resize(P, None, ctypes.c_void_p(128), None, ctypes.c_void_p(256), 2, 8, 8, P, None, 4, None)
    with pytest.raises(RuntimeError, match="null image pointer"):
        L.alb_rotate(None, None, P, None, 2, 8, 8, P, P, None, None)
    with pytest.raises(RuntimeError, match="in place"):
        L.alb_rotate(P, None, P, None, 2, 8, 8, P, P, None, None)
    with pytest.raises(RuntimeError, match="null image pointer"):
        L.alb_to_tensor(None, None, P, 2, 8, 8, None)
    assert L.version() == 106


def test_crop_box_outside_the_image_is_refused_on_the_host():
    from stil_tta_amd.augment import alb_resize
    src = torch.zeros(2, 10, 12, 3, dtype=torch.uint8)
    for bad in ([[0, 0, 10, 12], [5, 0, 6, 12]], [[0, 0, 10, 12], [0, -1, 4, 4]], [[0, 0, 0, 12], [0, 0, 10, 12]]):
        with pytest.raises(ValueError, match="crop box outside"):
            alb_resize(src, bad, 8)
    with pytest.raises(ValueError, match="must be positive"):
        alb_resize(src, [[0, 0, 10, 12]] * 2, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        alb_resize(src, [[0, 0, 10, 12], [9, 11, 1, 1]], 8)       # valid boxes: only the device is missing
