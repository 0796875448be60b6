"""The albumentations branch of the device input pipeline (csrc/augment_alb.hip, augment.py with augmentation_speedup=True)
against the numpy restatement of its pixel definitions (tests/alb_restate.py): bit-exact for uint8 images, within 2e-6 for
float32 ones, plus the builders end to end.  The reflect-101 border, the hue shift and the random ColorJitter order are each
checked by a case that the torchvision-branch kernels would fail."""
import os
import sys
from itertools import permutations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alb_restate as RS  # noqa: E402

pytestmark = pytest.mark.gpu


def _u8(rng, *shape):
    return rng.integers(0, 256, shape, dtype=np.uint8)


def _f32(rng, *shape):
    return rng.random(shape, dtype=np.float32)


def _gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _eq(got, ref, fl, tol=2e-6):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    if fl:
        err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
        assert err <= tol, err
    else:
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize("H,W", [(96, 96), (61, 75)])      # 4-pixel vector path / per-pixel path
def test_color_u8_brightness_contrast_all_orders_bit_exact(H, W):
    """Brightness and contrast LUTs over all 24 orders and factors {0.2, 0.7, 1.0, 1.8}, bit for bit; the integer grey sum
    makes one workgroup per image and several per image give identical bits."""
    from stil_tta_amd.augment import alb_color
    rng = np.random.default_rng(1)
    fs = [0.2, 0.7, 1.0, 1.8]
    orders = list(permutations(range(4)))
    combos = [(o, fb, fc) for o in orders for fb in fs for fc in fs][::2]         # 192 images: every order, every factor
    B = len(combos)
    img = _u8(rng, B, H, W, 3)
    order = np.array([c[0] for c in combos], np.int32)
    fac = np.array([[c[1], c[2], 1.0, 0.0] for c in combos])
    on, off = np.ones(B, np.uint8), np.zeros(B, np.uint8)
    src = _gpu(img)
    outs = [alb_color(src, order, fac, on, off, wg_per_image=w).cpu() for w in (1, 7, 0)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    got = outs[0].numpy()
    for b in range(B):
        _eq(got[b], RS.color_jitter(img[b], order[b], fac[b]), False)
    assert torch.equal(src.cpu(), torch.from_numpy(img))                          # src -> dst leaves the source alone


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_color_full_chain_with_hue_saturation_gray(dtype):
    from stil_tta_amd.augment import alb_color
    rng = np.random.default_rng(2)
    B, H, W = 48, 50, 70
    fl = dtype == "f32"
    img = _f32(rng, B, H, W, 3) if fl else _u8(rng, B, H, W, 3)
    img[0, :, :10] = img[0, :, :1]                                           # grey pixels (undefined hue)
    order = np.argsort(rng.random((B, 4)), 1).astype(np.int32)
    fac = np.concatenate([rng.uniform(0.2, 1.8, (B, 3)), rng.uniform(-0.2, 0.2, (B, 1))], 1)
    fac[1] = [1.0, 1.0, 1.0, 0.0]                                             # identity factors
    fac[2, 3] = 0.5                                                           # half a turn
    fac[3] = [0.0, 0.0, 0.0, -0.5]                                            # zero factors
    cj_on = (rng.random(B) < 0.8).astype(np.uint8)
    cj_on[:4] = 1
    gray_on = (rng.random(B) < 0.3).astype(np.uint8)
    x = _gpu(img)
    got = alb_color(x, order, fac, cj_on, gray_on).cpu().numpy()
    for b in range(B):
        ref = RS.color_jitter(img[b], order[b], fac[b]) if cj_on[b] else img[b]
        ref = RS.to_gray(ref) if gray_on[b] else ref
        _eq(got[b], ref, fl)
        if not cj_on[b] and not gray_on[b]:
            assert np.array_equal(got[b], img[b])
    assert np.array_equal(got[1], RS.to_gray(img[1]) if gray_on[1] else img[1])
    # in place gives the same bits; the hue shift is real (the torchvision branch never shifts hue in these views)
    alb_color(x, order, fac, cj_on, gray_on, out=x)
    assert np.array_equal(x.cpu().numpy(), got)
    only_hue = np.tile(np.array([[1.0, 1.0, 1.0, 0.15]]), (B, 1))
    h = alb_color(_gpu(img), order, only_hue, np.ones(B, np.uint8), np.zeros(B, np.uint8)).cpu().numpy()
    assert np.abs(h[5].astype(np.float64) - img[5]).max() > (0.05 if fl else 10)
    _eq(h[5], RS.hue(img[5], 0.15), fl)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_blur_reflect101_borders(dtype):
    from stil_tta_amd.augment import alb_blur
    rng = np.random.default_rng(3)
    fl = dtype == "f32"
    for k, (H, W) in ((29, (40, 45)), (19, (23, 66)), (29, (9, 13))):        # every pixel within the radius of a border
        B = 5
        img = _f32(rng, B, H, W, 3) if fl else _u8(rng, B, H, W, 3)
        sigma = np.array([0.1, 0.8, 2.0, 0.0, 1.37])
        got = alb_blur(_gpu(img), sigma, k).cpu().numpy()
        for b in range(B):
            ref = RS.gaussian_blur(img[b], k, float(sigma[b]))
            _eq(got[b], ref, fl, 1e-6)
        assert np.array_equal(got[3], img[3])                                  # sigma 0: a copy
        # cv2's BORDER_REFLECT (the edge pixel repeated) gives a different picture within the radius of the border
        rep = RS.gaussian_blur_border(img[2], k, 2.0, edge_repeat=True)
        assert np.abs(rep[:, :k // 2].astype(np.float64) - got[2][:, :k // 2]).max() > (1e-3 if fl else 0)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_resize_crop_flip_and_to_tensor(dtype):
    from stil_tta_amd.augment import alb_resize, alb_to_tensor, rrc_boxes
    rng = np.random.default_rng(4)
    fl = dtype == "f32"
    B, H, W, P = 8, 57, 43, 32
    img = _f32(rng, B, H, W, 3) if fl else _u8(rng, B, H, W, 3)
    boxes = rrc_boxes(H, W, B, scale=(0.08, 1.0), rng=rng)
    boxes[0] = [0, 0, H, W]                # A.Resize
    boxes[1] = [5, 7, 1, 1]                # one-pixel box
    boxes[2] = [3, 2, 10, 12]              # upsampling
    boxes[3] = [H - 1, W - 1, 1, 1]        # last pixel
    flip = (rng.random(B) < 0.5).astype(np.uint8)
    flip[2] = 1
    x = _gpu(img)
    hwc = alb_resize(x, boxes, P, flip, final=False).cpu().numpy()
    chw = alb_resize(x, boxes, P, flip, final=True).cpu().numpy()
    for b in range(B):
        ref = RS.resize_crop(img[b], boxes[b], P, bool(flip[b]))
        _eq(hwc[b], ref, fl, 1e-6)
        _eq(chw[b], RS.to_tensor(hwc[b]), False)           # the fused tensor is to_tensor of the stage's image, bit for bit
    assert (chw[1] == chw[1][:, :1, :1]).all()
    tt = alb_to_tensor(x).cpu().numpy()
    for b in range(B):
        _eq(tt[b], RS.to_tensor(img[b]), False)
    odd = img[:, :13, :11]                                 # 143 pixels: the per-pixel path
    _eq(alb_to_tensor(_gpu(odd)).cpu().numpy()[3], RS.to_tensor(odd[3]), False)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_rotate_quantised_reflect101(dtype):
    from stil_tta_amd.augment import alb_rotate
    rng = np.random.default_rng(5)
    fl = dtype == "f32"
    B, H, W = 6, 37, 52
    img = _f32(rng, B, H, W, 3) if fl else _u8(rng, B, H, W, 3)
    angle = np.array([0.0, 45.0, -44.9, 17.3, 90.0, 12.0])
    on = np.array([1, 1, 1, 1, 1, 0], np.uint8)
    ff = np.array([0, 0, 1, 0, 1, 1], np.uint8)
    got = alb_rotate(_gpu(img), angle, on, ff).cpu().numpy()
    for b in range(B):
        ref = RS.rotate(img[b], float(angle[b]), bool(ff[b])) if on[b] else (img[b][:, ::-1] if ff[b] else img[b])
        _eq(got[b], ref, fl, 1e-6)
    assert np.array_equal(got[0], img[0])                  # angle 0: an exact copy
    assert np.array_equal(got[5], img[5][:, ::-1])         # off: the flip alone


FAMILIES = [(k, t) for k in ("contrastive", "hard_eval", "soft_eval", "weak", "strong", "default") for t in ("dvm", "CAD")]


@pytest.mark.parametrize("kind,target", FAMILIES)
def test_family_chain_equals_the_restated_chain(kind, target):
    from stil_tta_amd.augment import ImageAugmenter, _alb_policy
    rng = np.random.default_rng(6)
    fl = target != "dvm"
    B, H, W, P = 10, 48, 40, 32
    img = _f32(rng, B, H, W, 3) if fl else _u8(rng, B, H, W, 3)
    aug = ImageAugmenter(P, target, 0.9, seed=11, kind=kind, augmentation_speedup=True)
    d = aug.draw(B, H, W)
    names = [n for n, _ in _alb_policy(kind, not fl)]
    for b in (0, 1):                                          # every stage of the family applied to two images of the batch
        if "cj" in names:
            d["cj_on"][b], d["factors"][b], d["order"][b] = 1, [1.3, 0.6, 1.4, 0.1 - 0.2 * b], [3, 1, 0, 2] if b else [1, 2, 3, 0]
        if "gray" in names:
            d["gray_on"][b] = b
        if "rotate" in names:
            d["rot_on"][b], d["angle"][b] = 1, 30.0 - 50.0 * b
        if "blur" in names:
            d["sigma"][b] = 1.5
    view, orig = aug(_gpu(img), d)
    view, orig = view.cpu().numpy(), orig.cpu().numpy()
    stages = _alb_policy(kind, not fl)
    for b in range(B):
        _eq(view[b], RS.apply_chain(img[b], stages, d, b, P), fl)
        _eq(orig[b], RS.apply_chain(img[b], _alb_policy("default", not fl), d, b, P), fl)
    again, _ = aug(_gpu(img), d, want_orig=False)
    assert np.array_equal(again.cpu().numpy(), view)           # same draws, same bits


def _stil_step(builder_l, builder_u, fl_cols):
    from stil_tta_amd import STiLModel
    from stil_tta_amd.driver import train_step
    from stil_tta_amd.flat import StilAdam
    g = torch.Generator().manual_seed(4)
    bl, bu = builder_l(torch.tensor([0, 5])), builder_u(torch.randperm(40, generator=g)[:14])
    im, tab, y, orig, ident = bu
    assert im[1].shape == (14, 3, 64, 64) and orig.shape == (14, 3, 64, 64) and im[1].dtype == torch.float32
    assert float(im[1].min()) >= 0.0 and float(im[1].max()) <= 1.0 and float(orig.max()) <= 1.0
    torch.manual_seed(0)
    m = STiLModel(dict(model="resnet18", embedding_dim=512, field_lengths=fl_cols, num_classes=5, start_epoch=0, batch_size=16, th1=0.3, img_size=64))
    m.setup_device("cuda"); m.train(); m.current_epoch = 1
    m.prototypes.copy_(F.normalize(torch.randn(5, 128, generator=g)).cuda())
    return train_step(m, StilAdam(m.flat, lr=1e-3), {"l": bl, "u": bu})


def _table(N, g):
    return torch.cat([torch.randint(0, 3, (N, 1), generator=g).float(), torch.randint(0, 4, (N, 1), generator=g).float(), torch.randn(N, 3, generator=g)], 1)


@pytest.mark.parametrize("target", ["dvm", "CAD"])
def test_contrastive_builder_feeds_a_stil_step(target):
    from stil_tta_amd.augment import ContrastiveBatchBuilder
    g = torch.Generator().manual_seed(4)
    N = 48
    imgs = torch.randint(0, 256, (N, 80, 72, 3), generator=g, dtype=torch.uint8) if target == "dvm" else torch.rand(N, 80, 72, 3, generator=g)
    table, labels = _table(N, g), torch.randint(0, 5, (N,), generator=g)
    kw = dict(augmentation_speedup=True)
    lab = ContrastiveBatchBuilder(imgs[:8], table[:8], labels[:8], 64, target, 0.3, 0.95, labelled=True, **kw)
    unl = ContrastiveBatchBuilder(imgs[8:], table[8:], labels[8:], 64, target, 0.3, 0.95, labelled=False, **kw)
    loss = _stil_step(lab, unl, [3, 4] + [1] * 3)
    assert bool(torch.isfinite(loss))


def test_match_builders_feed_a_comatch_step():
    from stil_tta_amd import CoMatch
    from stil_tta_amd.augment import EvalTrainBatchBuilder, StrongWeakBatchBuilder
    from stil_tta_amd.driver import train_step
    from stil_tta_amd.flat import StilAdam
    g = torch.Generator().manual_seed(4)
    N, fl = 48, [3, 4] + [1] * 8
    imgs = torch.randint(0, 256, (N, 80, 72, 3), generator=g, dtype=torch.uint8)
    table = torch.cat([torch.randint(0, 3, (N, 1), generator=g).float(), torch.randint(0, 4, (N, 1), generator=g).float(), torch.randn(N, 8, generator=g)], 1)
    labels = torch.randint(0, 2, (N,), generator=g)
    lab = EvalTrainBatchBuilder(imgs[:8], table[:8], labels[:8], 64, "dvm", 0.3, 0.8, augmentation_speedup=True)
    unl = StrongWeakBatchBuilder(imgs[8:], table[8:], labels[8:], 64, "dvm", 0.3, two_strong=True, augmentation_speedup=True)
    (x_l, t_l), y_l, idx = lab(torch.tensor([0, 5]))
    views, y_u = unl(torch.randperm(40, generator=g)[:14])
    assert x_l.shape == (2, 3, 64, 64) and len(views) == 3 and all(v[0].shape == (14, 3, 64, 64) for v in views)
    assert all(float(v[0].min()) >= 0.0 and float(v[0].max()) <= 1.0 for v in views)
    assert not torch.equal(views[1][0], views[2][0])
    torch.manual_seed(0)
    m = CoMatch(dict(model="resnet18", embedding_dim=512, field_lengths=fl, num_classes=2, start_epoch=0, batch_size=16, img_size=64, K=40,
                     co_threshold=0.5, contrast_th=0.5))
    m.setup_device("cuda"); m.train(); m.current_epoch = 1
    loss = train_step(m, StilAdam(m.flat, lr=1e-3), {"l": ((x_l, t_l), y_l, idx), "u": (views, y_u)})
    assert bool(torch.isfinite(loss))


@pytest.mark.parametrize("algo,target", [("STiL", "dvm"), ("CoMatch", "CAD")])
def test_semisl_loaders_with_the_key_yield_float_batches(algo, target):
    from stil_tta_amd.augment import semisl_loaders
    g = torch.Generator().manual_seed(7)

    def data(N):
        im = torch.randint(0, 256, (N, 50, 46, 3), generator=g, dtype=torch.uint8) if target == "dvm" else torch.rand(N, 50, 46, 3, generator=g)
        return im, _table(N, g), torch.randint(0, 2, (N,), generator=g)
    hp = dict(algorithm_name=algo, img_size=32, target=target, corruption_rate=0.3, batch_size=16, unlabelled_ratio=3, seed=1,
              augmentation_speedup=True)
    ld = semisl_loaders(hp, data(12), data(40))
    lb, ub = next(iter(ld["l"])), next(iter(ld["u"]))
    if algo == "STiL":
        ims = [lb[0][1], lb[3], ub[0][1], ub[3]]
        assert lb[0][1].shape == (4, 3, 32, 32) and ub[0][1].shape == (12, 3, 32, 32)
    else:
        ims = [lb[0][0]] + [v[0] for v in ub[0]]
        assert lb[0][0].shape == (4, 3, 32, 32) and len(ub[0]) == 3 and ub[0][0][0].shape == (12, 3, 32, 32)
    for x in ims:
        assert x.dtype == torch.float32 and float(x.min()) >= 0.0 and float(x.max()) <= 1.0
