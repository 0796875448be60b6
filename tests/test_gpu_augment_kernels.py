"""The twelve entry points of the input pipeline, called through the C ABI with raw addresses at the cases of
tests/augment_cases.py.

Part A, csrc/augment.hip (stil_tab_corrupt, stil_aug_gray_mean, stil_aug_resize, stil_aug_blur, stil_aug_rotate, stil_aug_hue):
compared with the float64 references there (`augment_cases.check`: 4 times the error the fp32 restatement makes on the same
cases, which tests/test_augment_cases_cpu.py measures and caps at 1e-4), stil_tab_corrupt exactly.  Every call runs uint8 HWC
and float CHW sources where the kernel takes both, writes into sentinel-filled outputs between guard elements, leaves its
inputs bit-identical, repeats bit for bit, and gives sample b of a batch of 3 the bits of a batch of 1 holding that sample.
Part B, csrc/augment_alb.hip (stil_alb_color, stil_alb_blur, stil_alb_resize, stil_alb_rotate, stil_alb_to_tensor): the
geometry tests/test_gpu_augment_alb.py leaves out, against tests/alb_restate.py under that module's `_eq` (bit for bit for
uint8, its float tolerances for float32)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alb_restate as RS  # noqa: E402
import augment_cases as A  # noqa: E402
from test_gpu_augment_alb import _eq  # noqa: E402
from test_gpu_entry_points import SENT, P, _release_operands, _st, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu

GUARD = 64                       # guard elements before and after every output
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from stil_tta_amd._lib import lib
    return lib()


def up(a):
    """a numpy array (or None) -> a CUDA copy kept alive until the test ends"""
    return None if a is None else dev(torch.tensor(np.asarray(a)))


def guarded(shape, dtype=torch.float32, fill=SENT):
    """-> (buffer, view): a sentinel-filled view of `shape` with GUARD sentinel elements on either side"""
    n = int(np.prod(shape))
    buf = dev(torch.full((n + 2 * GUARD,), fill, dtype=dtype))
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_hold(buf, fill=SENT):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def untouched(t, a):
    return t is None or same_bits(t.cpu().numpy(), np.asarray(a))


def src_of(img):
    """-> (device tensor, src_u8 address, src_f32 address)"""
    t = up(img)
    return (t, P(t), None) if A.is_u8(img) else (t, None, P(t))


def f32a(v):
    return None if v is None else np.asarray(v, dtype=np.float32)


def batch_rules(run, B, *per_sample):
    """run(rows) -> the output of the call on samples `rows` (checked for guards and untouched inputs inside).  Applies the rules
    every part-A case carries: a second call gives the same bits, and sample b of the batch gives the bits of a batch of 1."""
    out = run(slice(0, B))
    assert same_bits(out, run(slice(0, B))), "a second identical call differs"
    if B > 1:
        for b in range(B):
            assert same_bits(out[b:b + 1], run(slice(b, b + 1))), f"sample {b} of the batch differs from a batch of 1 holding it"
    return out


# =====================================================================================================================
# part A: stil_tab_corrupt
# =====================================================================================================================
def _tab(L, c, rows, n, N, k):
    clean, marg = up(c["clean"][rows]), up(c["marginal"])
    idx, pos = (up(c["idx"][rows]), up(c["pos"][rows])) if k else (None, None)      # k == 0: NULL draws
    Bs = clean.shape[0]
    buf, out = guarded((Bs, n))
    L.tab_corrupt(P(clean), P(marg), P(idx), P(pos), P(out), Bs, n, N, k, _st())
    torch.cuda.synchronize()
    assert guards_hold(buf), "a write outside the output"
    assert untouched(clean, c["clean"][rows]) and untouched(marg, c["marginal"]), "an input changed"
    assert k == 0 or (untouched(idx, c["idx"][rows]) and untouched(pos, c["pos"][rows])), "a draw changed"
    return out.cpu().numpy()


@pytest.mark.parametrize("n_cols", A.TAB_NCOLS)
def test_tab_corrupt_copies_and_scatters_exactly(L, n_cols):
    for B, n, N, k in A.TAB_TABLE:
        if n != n_cols:
            continue
        c = A.tab_case(B, n, N, k)
        out = batch_rules(lambda rows: _tab(L, c, rows, n, N, k), B)
        ref = A.tab_reference(c)
        assert same_bits(out, ref), (B, n, N, k, np.argwhere(out != ref)[:5].tolist())
        if k == 0:
            assert same_bits(out, c["clean"])


# =====================================================================================================================
# part A: stil_aug_gray_mean
# =====================================================================================================================
def _gray_mean(L, img, jitter, rows):
    img = img[rows]
    jitter = None if jitter is None else jitter[rows]
    H, W = A.hw(img)
    t, pu, pf = src_of(img)
    jd = up(jitter)
    buf, out = guarded((len(img),))
    L.aug_gray_mean(pu, pf, P(jd), P(out), len(img), H, W, A.scale_of(img), _st())
    torch.cuda.synchronize()
    assert guards_hold(buf) and untouched(t, img) and untouched(jd, jitter)
    return out.cpu().numpy()


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("H,W", A.GM_SHAPES)
def test_gray_mean_against_float64(L, H, W, fmt):
    img = A.gm_image(fmt, H, W)
    plain = batch_rules(lambda rows: _gray_mean(L, img, None, rows), 3)
    A.check("gray_mean", plain, A.gray_mean_reference(img), "jitter NULL")
    jit = A.gm_jitter()
    out = batch_rules(lambda rows: _gray_mean(L, img, jit, rows), 3)
    A.check("gray_mean", out, A.gray_mean_reference(img, jit[:, 0]), "brightness 0 / 0.4 / 1.8")
    assert float(out[0]) == 0.0, "brightness 0: the mean of a black image"
    ones = jit.copy()
    ones[:, 0] = 1.0
    assert same_bits(_gray_mean(L, img, ones, slice(0, 3)), plain), "brightness 1 is the NULL jitter"


# =====================================================================================================================
# part A: stil_aug_resize
# =====================================================================================================================
def _resize(L, img, boxes, Pn, flip=None, jitter=None, gmean=None, nan_margin=False):
    """-> [B, 3, P, P] on the host.  nan_margin (float sources): the image lies between NaN margins, so a read outside it
    poisons the output"""
    H, W = A.hw(img)
    B = len(img)
    if nan_margin:
        n = img.size
        sb = dev(torch.full((n + 2 * GUARD,), NAN))
        sb[GUARD:GUARD + n] = torch.tensor(img).flatten().cuda()
        t, pu, pf = sb, None, sb[GUARD:].data_ptr()
        before = sb.cpu().numpy()
    else:
        t, pu, pf = src_of(img)
        before = img
    bd, fd, jd, gd = up(np.asarray(boxes, dtype=np.int32)), up(flip), up(f32a(jitter)), up(f32a(gmean))
    buf, out = guarded((B, 3, Pn, Pn))
    L.aug_resize(pu, pf, P(bd), P(fd), P(jd), P(gd), P(out), B, H, W, Pn, A.scale_of(img), _st())
    torch.cuda.synchronize()
    assert guards_hold(buf), "a write outside the output"
    assert untouched(t, before) and untouched(bd, np.asarray(boxes, dtype=np.int32)) and untouched(fd, flip), "an input changed"
    assert untouched(jd, f32a(jitter)) and untouched(gd, f32a(gmean)), "an input changed"
    got = out.cpu().numpy()
    assert bool((got != SENT).all()), "an output pixel was not written"
    return got


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("Pn", A.RS_PS)
@pytest.mark.parametrize("H,W", A.RS_SOURCES)
def test_resize_crop_flip_against_float64(L, H, W, Pn, fmt):
    src, boxes = A.resize_source(fmt, H, W), A.resize_boxes(H, W)
    for lo in (0, 3):                                             # two batches of 3 over the six boxes
        img, bx = src[lo:lo + 3], boxes[lo:lo + 3]
        out = batch_rules(lambda rows: _resize(L, img[rows], bx[rows], Pn), 3)
        A.check("resize", out, A.resize_reference(img, bx, Pn), f"boxes {A.RS_BOX_NAMES[lo:lo + 3]}")
        assert same_bits(out, _resize(L, img, bx, Pn, np.zeros(3, np.uint8))), "flip NULL differs from flip = 0"
        mirrored = _resize(L, img, bx, Pn, np.ones(3, np.uint8))
        assert same_bits(mirrored, out[:, :, :, ::-1]), "flip = 1 is not the mirror image of flip = 0"
        mixed = _resize(L, img, bx, Pn, np.array([0, 1, 0], np.uint8))
        assert same_bits(mixed[0], out[0]) and same_bits(mixed[1], mirrored[1]) and same_bits(mixed[2], out[2]), "flip is per sample"
        A.check("resize", mirrored, A.resize_reference(img, bx, Pn, np.ones(3, np.uint8)), "flipped")
    if H >= 3 and W >= 3:
        assert float(np.abs(out[2] - 1.0).max()) <= A.TOL["resize"], "the interior box of a full-scale patch: a read outside the crop shows"


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("H,W,Pn", A.RS_JITTER_SHAPES)
def test_resize_colour_jitter_against_float64(L, H, W, Pn, fmt):
    img, bx = A.resize_source(fmt, H, W)[:3], A.resize_boxes(H, W)[[0, 4, 5]]
    plain = _resize(L, img, bx, Pn)
    ident = np.array([A.IDENTITY_JITTER] * 3, np.float32)
    assert same_bits(_resize(L, img, bx, Pn, None, ident, A.jitter_gmean(img, ident)), plain), "(1, 1, 1, 0) differs from a NULL jitter"
    flip = np.array([0, 1, 0], np.uint8)
    for batch in A.RS_JITTERS:
        jit = np.array(batch, np.float32)
        gm = A.jitter_gmean(img, jit)
        out = batch_rules(lambda rows: _resize(L, img[rows], bx[rows], Pn, flip[rows], jit[rows], gm[rows]), 3)
        A.check("colour", out, A.resize_reference(img, bx, Pn, flip, jit, gm), batch)
        unflipped = _resize(L, img, bx, Pn, None, jit, gm)
        assert same_bits(out[1], unflipped[1, :, :, ::-1]) and same_bits(out[0], unflipped[0])
        for b in range(3):
            if batch[b][3] != 0.0:
                assert same_bits(out[b, 0], out[b, 1]) and same_bits(out[b, 0], out[b, 2]), "gray = 1: three equal channels"
        # the constant as the host gets it: stil_aug_gray_mean on the device, handed to the resize as it is
        gdev = _gray_mean(L, img, jit, slice(0, 3))
        A.check("colour", _resize(L, img, bx, Pn, flip, jit, gdev), A.resize_reference(img, bx, Pn, flip, jit, gdev), "gmean from the device")


@pytest.mark.parametrize("fmt", A.FMTS)
def test_resize_clamps_bad_device_boxes_into_the_image(L, fmt):
    """boxes that already live on the device skip the host check: the kernel clamps them (augment_cases.clamp_box restates
    the clamp), through the C ABI and through resize_crop with a CUDA tensor of boxes"""
    from stil_tta_amd.augment import resize_crop
    H, W, Pn = A.RS_BAD_SHAPE
    bad = np.array(A.RS_BAD_BOXES, dtype=np.int32)
    clamped = np.array([A.clamp_box(b, H, W) for b in bad], dtype=np.int32)
    img = A.image(fmt, len(bad), H, W, 32)
    ref = A.resize_reference(img, clamped, Pn)
    outs = []
    for lo in range(0, len(bad), 3):
        rows = slice(lo, lo + 3)
        out = batch_rules(lambda r: _resize(L, img[rows][r], bad[rows][r], Pn, nan_margin=fmt == "f32"), 3)
        A.check("resize", out, ref[rows], f"bad boxes {bad[rows].tolist()}")
        assert same_bits(out, _resize(L, img[rows], clamped[rows], Pn)), "a bad box differs from its clamped box"
        outs.append(out)
    srcd = up(img)
    got = resize_crop(srcd, dev(torch.tensor(bad)), Pn)
    torch.cuda.synchronize()
    assert same_bits(got.cpu().numpy(), np.concatenate(outs)), "resize_crop with device boxes differs from the C ABI"
    with pytest.raises(ValueError, match="crop box outside"):
        resize_crop(srcd, bad, Pn)                                 # the same boxes from the host are refused before the upload


# =====================================================================================================================
# part A: stil_aug_blur
# =====================================================================================================================
def _blur(L, img, sigma, k):
    H, W = A.hw(img)
    B = len(img)
    t, pu, pf = src_of(img)
    sd = up(f32a(sigma))
    tbuf, tmp = guarded((B, 3, H, W))
    buf, out = guarded((B, 3, H, W))
    L.aug_blur(pu, pf, P(sd), P(tmp), P(out), B, H, W, k, A.scale_of(img), _st())
    torch.cuda.synchronize()
    assert guards_hold(buf) and guards_hold(tbuf), "a write outside the output or the workspace"
    assert untouched(t, img) and untouched(sd, f32a(sigma)), "an input changed"
    return out.cpu().numpy()


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("H,W,k", A.BL_GEOMS)
def test_blur_against_float64(L, H, W, k, fmt):
    img = A.image(fmt, 3, H, W, 33)
    copy = A.raw32(img) * A.INV255 if fmt == "u8" else img           # sigma <= 0: v * fp32(1 / 255) / the same bits
    for sigma in A.BL_SIGMAS:
        sg = np.array(sigma, np.float32)
        out = batch_rules(lambda rows: _blur(L, img[rows], sg[rows], k), 3)
        A.check("blur", out, A.blur_reference(img, sg, k), f"sigma {sigma}")
        for b, s in enumerate(sigma):
            if s <= 0:
                assert same_bits(out[b], copy[b]), f"sigma {s} must copy"
            if s == 0.05:
                assert bool(np.isfinite(out[b]).all()) and A.max_err(out[b], A.src64(img)[b]) <= A.TOL["blur"], "underflowing side weights: the source"


# =====================================================================================================================
# part A: stil_aug_rotate
# =====================================================================================================================
def _rotate(L, img, angle):
    H, W = A.hw(img)
    B = len(img)
    t, pu, pf = src_of(img)
    ad = up(f32a(angle))
    buf, out = guarded((B, 3, H, W))
    L.aug_rotate(pu, pf, P(ad), P(out), B, H, W, A.scale_of(img), _st())
    torch.cuda.synchronize()
    assert guards_hold(buf), "a write outside the output"
    assert untouched(t, img) and untouched(ad, f32a(angle)), "an input changed"
    return out.cpu().numpy()


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("H,W", A.RT_SHAPES)
def test_rotate_against_float64(L, H, W, fmt):
    img = A.image(fmt, 3, H, W, 34)
    copy = A.raw32(img) * A.INV255 if fmt == "u8" else img
    for angles in A.RT_ANGLES:
        ang = np.array(angles, np.float32)
        out = batch_rules(lambda rows: _rotate(L, img[rows], ang[rows]), 3)
        A.check("rotate", out, A.rotate_reference(img, ang), f"angles {angles}")
        for b, a in enumerate(angles):
            if a == 0.0:
                assert same_bits(out[b], copy[b]), "angle 0 must copy"
    if H == W:
        r90 = _rotate(L, img, np.full(3, 90.0, np.float32))
        assert A.max_err(r90, np.rot90(A.src64(img), 1, axes=(2, 3))) <= A.TOL["rotate"], "90 degrees on a square: counter-clockwise"


# =====================================================================================================================
# part A: stil_aug_hue
# =====================================================================================================================
def _hue(L, img, hue, gr):
    B, _, H, W = img.shape
    buf, x = guarded((B, 3, H, W))
    x.copy_(torch.tensor(img))
    hd, gd = up(f32a(hue)), up(f32a(gr))
    L.aug_hue(P(x), P(hd), P(gd), B, H, W, _st())
    torch.cuda.synchronize()
    assert guards_hold(buf), "a write outside the image"
    assert untouched(hd, f32a(hue)) and untouched(gd, f32a(gr)), "an input changed"
    return x.cpu().numpy()


@pytest.mark.parametrize("H,W", A.HUE_SHAPES)
def test_hue_against_float64(L, H, W):
    img = A.hue_image(H, W)
    for hue, gr in A.HUE_CALLS:
        h, g = f32a(hue), f32a(gr)
        out = batch_rules(lambda rows: _hue(L, img[rows], None if h is None else h[rows], None if g is None else g[rows]), 3)
        A.check("hue", out, A.hue_reference(img, hue, gr), f"hue {hue} gray {gr}")
        for b in range(3):
            off = (hue is None or hue[b] == 0.0) and (gr is None or gr[b] == 0.0)
            if off:
                assert same_bits(out[b], img[b]), "hue 0 and gray 0: the sample keeps its bits"
            if gr is not None and gr[b] != 0.0:
                assert same_bits(out[b, 0], out[b, 1]) and same_bits(out[b, 0], out[b, 2])
            if hue is not None and hue[b] != 0.0 and (gr is None or gr[b] == 0.0):
                grey = np.flatnonzero((img[b, 0] == img[b, 1]).ravel() & (img[b, 1] == img[b, 2]).ravel())
                assert same_bits(out[b].reshape(3, -1)[:, grey], img[b].reshape(3, -1)[:, grey]), "grey, black and white pixels do not move"


# =====================================================================================================================
# part B: csrc/augment_alb.hip against tests/alb_restate.py
# =====================================================================================================================
def _typed(t, u8):
    """(uint8 address, float32 address) of an image tensor"""
    return (P(t), None) if u8 else (None, P(t))


def _offset_image(img, off):
    """a CUDA copy of `img` that starts `off` elements into its buffer (off = 1: a misaligned base address)"""
    flat = torch.tensor(img).flatten()
    buf = dev(torch.zeros(flat.numel() + off, dtype=flat.dtype))
    buf[off:] = flat.cuda()
    return buf[off:].view(*img.shape)


def _alb_color(L, img, draws, wg=0, off=0, in_place=False):
    order, fac, cj, gr = draws
    B, H, W, _ = img.shape
    u8 = A.is_u8(img)
    src = _offset_image(img, off)
    dst = src if in_place else _offset_image(np.full_like(img, 7), off)
    od, fd, cd, gd = up(order), up(fac), up(cj), up(gr)
    gpart = dev(torch.zeros(B, 64, dtype=torch.float64))
    L.alb_color(*_typed(src, u8), *_typed(dst, u8), B, H, W, P(od), P(fd), P(cd), P(gd), P(gpart), wg, _st())
    torch.cuda.synchronize()
    assert in_place or untouched(src, img), "the source changed"
    return dst.cpu().numpy()


def _color_ref(img, draws):
    order, fac, cj, gr = draws
    out = []
    for b in range(len(img)):
        r = RS.color_jitter(img[b], order[b], fac[b]) if cj[b] else img[b]
        out.append(RS.to_gray(r) if gr[b] else r)
    return np.stack(out)


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("H,W", A.ALB_NPIX)
def test_alb_color_at_the_pixel_count_edges_and_in_place(L, H, W, fmt):
    img, draws = A.alb_image(fmt, 3, H, W), A.alb_color_draws(3, H, W)
    out = _alb_color(L, img, draws)
    _eq(out, _color_ref(img, draws), fmt == "f32")
    assert same_bits(out[1], img[1]), "a sample with both ops off is copied"
    assert same_bits(_alb_color(L, img, draws, in_place=True), out), "in place differs"       # per pixel wherever H * W % 4 != 0
    if fmt == "u8":
        assert same_bits(_alb_color(L, img, draws, wg=64), out), "wg_per_image = 64 is clipped to the groups the image fills"


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("n", A.ALB_MISALIGNED)
def test_alb_color_and_to_tensor_from_a_misaligned_base_take_the_per_pixel_path(L, n, fmt):
    img, draws = A.alb_image(fmt, 2, 2, n // 2), A.alb_color_draws(2, n)
    draws[2][:] = 1                                                # the colour ops run on both samples
    aligned = _alb_color(L, img, draws)
    for in_place in (False, True):
        got = _alb_color(L, img, draws, off=1, in_place=in_place)
        assert same_bits(got, aligned), "a base address 1 element into its buffer differs from the aligned call"
    _eq(aligned, _color_ref(img, draws), fmt == "f32")
    tt = _alb_to_tensor(L, img)
    assert same_bits(_alb_to_tensor(L, img, off=1), tt), "to_tensor from and into misaligned buffers differs"
    for b in range(2):
        _eq(tt[b], RS.to_tensor(img[b]), False)


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("H,W", A.ALB_WG)
def test_alb_color_with_64_workgroups_per_image(L, H, W, fmt):
    img, draws = A.alb_image(fmt, 1, H, W), A.alb_color_draws(1, H, W)
    one, many = _alb_color(L, img, draws, wg=1), _alb_color(L, img, draws, wg=64)
    if fmt == "u8":
        assert same_bits(one, many), "the integer grey sum does not depend on the split over workgroups"
    _eq(many, _color_ref(img, draws), fmt == "f32")
    _eq(one, _color_ref(img, draws), fmt == "f32")


def _alb_to_tensor(L, img, off=0):
    B, H, W, _ = img.shape
    src = _offset_image(img, off)
    obuf = dev(torch.full((B * 3 * H * W + off + GUARD,), SENT))
    out = obuf[off:off + B * 3 * H * W].view(B, 3, H, W)
    L.alb_to_tensor(*_typed(src, A.is_u8(img)), P(out), B, H, W, _st())
    torch.cuda.synchronize()
    assert bool((obuf[:off] == SENT).all()) and bool((obuf[off + B * 3 * H * W:] == SENT).all()) and untouched(src, img)
    return out.cpu().numpy()


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("H,W", A.ALB_NPIX)
def test_alb_to_tensor_at_the_pixel_count_edges(L, H, W, fmt):
    img = A.alb_image(fmt, 3, H, W)
    out = _alb_to_tensor(L, img)
    for b in range(3):
        _eq(out[b], RS.to_tensor(img[b]), False)


def _alb_blur(L, img, sigma, k):
    B, H, W, _ = img.shape
    u8 = A.is_u8(img)
    src, sd = up(img), up(np.asarray(sigma, dtype=np.float64))
    dst = dev(torch.full(img.shape, 7, dtype=src.dtype))
    L.alb_blur(*_typed(src, u8), *_typed(dst, u8), B, H, W, P(sd), k, _st())
    torch.cuda.synchronize()
    assert untouched(src, img)
    return dst.cpu().numpy()


def _alb_blur_case(L, fmt, H, W, k, sigma=(0.8, 2.0, 0.0)):
    img = A.alb_image(fmt, 3, H, W, k)
    out = _alb_blur(L, img, sigma, k)
    for b in range(3):
        _eq(out[b], RS.gaussian_blur(img[b], k, float(sigma[b])), fmt == "f32", 1e-6)
    assert same_bits(out[2], img[2]), "sigma 0 copies"
    return img, out


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("H,W", A.ALB_BLUR_TILE)
def test_alb_blur_at_the_tile_edges(L, H, W, fmt):
    for k in A.ALB_BLUR_KS:
        _alb_blur_case(L, fmt, H, W, k)
    img = A.alb_image(fmt, 3, H, W, 1)
    assert same_bits(_alb_blur(L, img, (0.8, 2.0, 0.0), 1), img), "ksize 1 is an exact copy"


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("H,W", A.ALB_BLUR_SHORT)
def test_alb_blur_on_images_shorter_than_the_radius(L, H, W, fmt):
    img, out = _alb_blur_case(L, fmt, H, W, 29)
    if H * W == 1:
        _eq(out, img, fmt == "f32", 1e-6)                          # one pixel: every tap is that pixel


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("Pn", A.ALB_RESIZE_PS)
@pytest.mark.parametrize("H,W", A.ALB_RESIZE_SOURCES)
def test_alb_resize_of_one_pixel_wide_sources_both_outputs(L, H, W, Pn, fmt):
    img = A.alb_image(fmt, 3, H, W, Pn)
    boxes = np.array([[0, 0, H, W], [H - 1, W - 1, 1, 1], [H // 2, W // 2, H - H // 2, W - W // 2]], dtype=np.int32)
    flip = np.array([0, 1, 1], np.uint8)
    u8 = A.is_u8(img)
    src, bd, fd = up(img), up(boxes), up(flip)
    hwc = dev(torch.full((3, Pn, Pn, 3), 7, dtype=src.dtype))
    cbuf, chw = guarded((3, 3, Pn, Pn))
    L.alb_resize(*_typed(src, u8), *_typed(hwc, u8), None, 3, H, W, P(bd), P(fd), Pn, _st())
    L.alb_resize(*_typed(src, u8), None, None, P(chw), 3, H, W, P(bd), P(fd), Pn, _st())
    torch.cuda.synchronize()
    assert guards_hold(cbuf) and untouched(src, img) and untouched(bd, boxes)
    hwc, chw = hwc.cpu().numpy(), chw.cpu().numpy()
    for b in range(3):
        _eq(hwc[b], RS.resize_crop(img[b], boxes[b], Pn, bool(flip[b])), fmt == "f32", 1e-6)
        _eq(chw[b], RS.to_tensor(hwc[b]), False)                   # the fused tensor is to_tensor of the stage's image


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("H,W", A.ALB_ROT_SHAPES)
def test_alb_rotate_of_narrow_images_with_and_without_flip_first(L, H, W, fmt):
    from stil_tta_amd.augment import alb_rotation_matrix
    angle = np.array(A.ALB_ROT_ANGLES * 2 + (33.0,))
    n = len(A.ALB_ROT_ANGLES)
    ff = np.array([0] * n + [1] * n + [1], np.uint8)
    on = np.array([1] * (2 * n) + [0], np.uint8)                    # the last sample: on = 0 together with flip_first
    B = len(angle)
    img = A.alb_image(fmt, B, H, W)
    u8 = A.is_u8(img)
    src, md, od, fd = up(img), up(alb_rotation_matrix(angle, H, W)), up(on), up(ff)
    dst = dev(torch.full(img.shape, 7, dtype=src.dtype))
    L.alb_rotate(*_typed(src, u8), *_typed(dst, u8), B, H, W, P(md), P(od), P(fd), _st())
    torch.cuda.synchronize()
    assert untouched(src, img)
    got = dst.cpu().numpy()
    for b in range(B):
        ref = RS.rotate(img[b], float(angle[b]), bool(ff[b])) if on[b] else img[b][:, ::-1]
        _eq(got[b], ref, fmt == "f32", 1e-6)
    assert same_bits(got[0], img[0]) and same_bits(got[n], img[n][:, ::-1]) and same_bits(got[-1], img[-1][:, ::-1])
    plain = dev(torch.full(img.shape, 7, dtype=src.dtype))
    L.alb_rotate(*_typed(src, u8), *_typed(plain, u8), B, H, W, P(md), P(od), None, _st())
    torch.cuda.synchronize()
    assert same_bits(plain.cpu().numpy()[:n], got[:n]) and same_bits(plain.cpu().numpy()[-1], img[-1]), "flip_first NULL is no flip"
