"""The shifted test stream on the device (csrc/shift.hip, stil_tta_amd/shift.py) against the definitions of tests/shift_cases.py:
the arithmetic kinds by close() at TOL of test_gpu_ops against float64, the selection kinds (impulse, missing, categorical flip)
bit for bit; the stream property (any cut of the stream gives the same bits) for the kernels and for ShiftStream; fit.test(shift=)
and fit.test_shifts under both protocols.  tests/test_shift_cpu.py checks on the CPU that float32 meets a quarter of these bars."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import shift_cases as SC  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402

INF = math.inf


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def unaligned(t):
    """a contiguous copy of t that starts 4 bytes past a 16-byte boundary: the 4-byte path of every kernel"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("offset", SC.NOISE_OFFSETS)
@pytest.mark.parametrize("shape", SC.NOISE_SHAPES, ids=str)
def test_noise_against_the_model(shape, offset):
    from stil_tta_amd import shift as S
    x = SC.image_input(shape)
    xd = dev(x)
    for clip in ((0.0, 1.0), None):
        lo, hi = clip or (-INF, INF)
        out = S.gaussian_noise(xd, SC.NOISE_STRENGTH[0], SC.SEED, offset, clip)
        close(out, t64(SC.noise_model(x, 0, SC.NOISE_STRENGTH[0], lo, hi, SC.SEED, offset)), name=f"gaussian {shape} @ {offset} clip {clip}")
        assert torch.equal(out, S.gaussian_noise(xd, SC.NOISE_STRENGTH[0], SC.SEED, offset, clip)), "not bit-identical on repetition"
        assert torch.equal(out, S.gaussian_noise(unaligned(xd), SC.NOISE_STRENGTH[0], SC.SEED, offset, clip)), "the 4-byte path gives other bits"
        if clip is None:
            assert float((out - xd).abs().max()) > 0.0
    for amount in (SC.NOISE_STRENGTH[1], 0.03, 1.0):
        for clip in ((0.0, 1.0), (-2.0, 3.5)):
            out = S.impulse_noise(xd, amount, SC.SEED, offset, clip)
            assert torch.equal(out.cpu(), torch.from_numpy(SC.noise_model(x, 1, amount, clip[0], clip[1], SC.SEED, offset))), (amount, clip)
            assert torch.equal(out, S.impulse_noise(xd, amount, SC.SEED, offset, clip))
            assert torch.equal(out, S.impulse_noise(unaligned(xd), amount, SC.SEED, offset, clip))
    other = S.gaussian_noise(xd, SC.NOISE_STRENGTH[0], SC.SEED + 1, offset, None)
    assert not torch.equal(other, S.gaussian_noise(xd, SC.NOISE_STRENGTH[0], SC.SEED, offset, None)), "the seed does not reach the kernel"


@pytest.mark.parametrize("offset", SC.NOISE_OFFSETS)
@pytest.mark.parametrize("sample", [(3, 5, 7), (3, 16, 16), (1, 1, 1), (3, 4, 1)], ids=str)
def test_one_call_on_three_samples_is_a_call_on_one_then_on_two(sample, offset):
    """105 elements per sample: the cut falls on an odd element and off a 16-byte boundary, so the parts take the 4-byte path and,
    at an even offset, split a pair of normals between them; 768 and 12: the whole and both parts take the 16-byte path; 1: one
    element per call"""
    from stil_tta_amd import shift as S
    xd = dev(SC.image_input((3,) + sample, seed=1))
    n1 = xd[0].numel()
    for fn, strength, clip in ((S.gaussian_noise, 0.38, (0.0, 1.0)), (S.gaussian_noise, 0.38, None), (S.impulse_noise, 0.27, (0.0, 1.0))):
        whole = fn(xd, strength, SC.SEED, offset, clip)
        parts = torch.cat([fn(xd[:1], strength, SC.SEED, offset, clip), fn(xd[1:], strength, SC.SEED, offset + n1, clip)])
        assert torch.equal(whole, parts), (fn.__name__, clip)


def test_noise_of_strength_zero_without_clipping_is_a_copy():
    from stil_tta_amd import shift as S
    from stil_tta_amd._lib import lib
    for shape in SC.NOISE_SHAPES:
        x = dev(SC.image_input(shape) * 8 - 4)
        assert torch.equal(S.gaussian_noise(x, 0.0, SC.SEED, 1, None), x)
        out = torch.full_like(x, SC.SENT)
        lib().shift_noise(x.data_ptr(), out.data_ptr(), x.numel(), 1, 0.0, -INF, INF, SC.SEED, 1, None)
        assert torch.equal(out, x)


# ------------------------------------------------------------------------------------------ contrast
@pytest.mark.parametrize("HW", SC.CONTRAST_HW)
def test_contrast_against_float64(HW):
    from stil_tta_amd import shift as S
    x = SC.contrast_input(HW)
    B, C = SC.CONTRAST_BC
    xd = dev(x).view(B, C, HW, 1)
    for factor in SC.CONTRAST_FACTORS + (0.0, 7.5):
        ref, m = SC.contrast_model(x, factor, 0.0, 1.0)
        out, mean = S.contrast(xd, factor, return_mean=True)
        close(out.view(B, C, HW), t64(ref), name=f"contrast HW {HW} factor {factor}")
        close(mean, t64(m), name=f"plane means HW {HW}")
        assert float((mean.cpu() - torch.from_numpy(m)).abs().max()) <= 2.0 ** -24, "the mean is more than an ulp from the float64 mean"
        assert torch.equal(out[0, 1], xd[0, 1]), f"a constant plane came back changed at factor {factor}"
        out2, mean2 = S.contrast(unaligned(xd), factor, return_mean=True)
        assert torch.equal(out, out2) and torch.equal(mean, mean2), "the 4-byte path gives other bits"
        assert torch.equal(out, S.contrast(xd, factor))
    ref, _ = SC.contrast_model(x * 4 - 2, 1.5, -INF, INF)
    close(S.contrast(dev(x * 4 - 2).view(B, C, HW, 1), 1.5, clip=None).view(B, C, HW), t64(ref), name="contrast without clipping")


# ------------------------------------------------------------------------------------------ brightness
@pytest.mark.parametrize("HW", [37, 40])     # the 4-byte and the 16-byte path
def test_brightness_against_float64_at_its_edges(HW):
    from stil_tta_amd import shift as S
    x = SC.brightness_input(HW)
    xd = dev(x).view(2, 3, HW, 1)
    for delta in SC.BRIGHT_DELTAS + (0.0, -0.25):
        for clip in ((0.0, 1.0), None):
            lo, hi = clip or (-INF, INF)
            out = S.brightness(xd, delta, clip)
            close(out.view(2, 3, HW), t64(SC.brightness_model(x, delta, lo, hi)), name=f"brightness delta {delta} clip {clip}")
            o = out.view(2, 3, HW).cpu()
            vprime = float(np.minimum(np.float32(0) + np.float32(delta), np.float32(hi)))
            assert o[0, :, 2].tolist() == [vprime] * 3 and o[1, :, 1].tolist() == [vprime] * 3, "V <= 0: every channel becomes V'"
            assert o[0, 0, 4] == o[0, 1, 4] == o[0, 2, 4], "r = g = b stays grey"
            if clip is not None and delta > 0:
                assert float(o[0, 0, 6]) == 1.0 and float(o.max()) <= 1.0, "V + delta is capped at hi"
            assert torch.equal(out, S.brightness(unaligned(xd), delta, clip)) and torch.equal(out, S.brightness(xd, delta, clip))


# ------------------------------------------------------------------------------------------ pixelate
@pytest.mark.parametrize("image", SC.PIX_IMAGES, ids=str)
@pytest.mark.parametrize("s", SC.PIX_SIDES)
def test_pixelate_against_float64(s, image):
    from stil_tta_amd import shift as S
    H, W = image
    x = SC.image_input(SC.PIX_BC + (H, W))
    xd = dev(x)
    out = S.pixelate(xd, s)
    close(out, t64(SC.pixelate_model(x, s)), name=f"pixelate {H}x{W} s {s}")
    assert torch.equal(out, S.pixelate(xd, s)) and torch.equal(out, S.pixelate(unaligned(xd), s))
    if s == 1:
        assert torch.equal(out, xd), "s = 1 is a copy"
    if s >= max(H, W):
        flat = out.view(*SC.PIX_BC, H * W)
        assert torch.equal(flat, flat[:, :, :1].expand_as(flat)), "one block per plane"
        close(flat[:, :, 0], t64(x.astype(np.float64).mean(axis=(2, 3))), name="plane mean")


# ------------------------------------------------------------------------------------------ tabular
@pytest.mark.parametrize("B", SC.TAB_BATCHES)
@pytest.mark.parametrize("layout", SC.TAB_LAYOUTS, ids=str)
def test_tabular_shifts_against_the_model(layout, B):
    from stil_tta_amd import shift as S
    n_cols, num_cat = layout
    cat_len, std, fill = SC.table_stats(n_cols, num_cat)
    st = S.TableStats(cat_len, std, fill)
    x = SC.table_input(B, n_cols, num_cat)
    xd = dev(x)
    names = {0: "tab_noise", 1: "tab_missing", 2: "tab_cat_flip"}
    for cname, on in SC.table_columns(n_cols).items():
        ond = dev(on)
        for kind, name in names.items():
            for strength in (SC.TAB_STRENGTH[kind], 0.0, 1.0):
                for offset in (3, 2 ** 32 - 5):
                    out = S.tab_shift(xd, st, name, strength, SC.SEED, offset, ond)
                    ref = SC.tab_model(x, num_cat, cat_len, on, std, fill, kind, strength, SC.SEED, offset)
                    what = f"{name} {layout} B {B} columns {cname} strength {strength} @ {offset}"
                    if kind == 0:
                        close(out, t64(ref), name=what)
                    else:
                        assert torch.equal(out.cpu(), torch.from_numpy(ref)), what
                    assert torch.equal(out, S.tab_shift(xd, st, name, strength, SC.SEED, offset, ond)), what
                    o = out.cpu()
                    if cname == "none" or strength == 0.0:
                        assert torch.equal(out, xd), what + ": not a copy"
                    if kind == 2:
                        assert torch.equal(o[:, num_cat:], torch.from_numpy(x[:, num_cat:])), what
                        for c in range(num_cat):
                            assert bool(((o[:, c] >= 0) & (o[:, c] < int(cat_len[c])) & (o[:, c] == o[:, c].floor())).all()), what
                    if kind == 1 and strength == 1.0:
                        assert torch.equal(o[:, on.astype(bool)], torch.from_numpy(fill)[on.astype(bool)].expand(B, -1)), what
                    if kind == 0:
                        assert torch.equal(o[:, :num_cat], torch.from_numpy(x[:, :num_cat])), what + ": a categorical column moved"
    assert torch.equal(S.tab_shift(xd, st, "tab_missing", 0.3, SC.SEED, 3), S.tab_shift(xd, st, "tab_missing", 0.3, SC.SEED, 3, dev(np.ones(n_cols, np.uint8))))
    if num_cat < n_cols and B > 1:
        moved = S.tab_shift(xd, st, "tab_noise", 1.0, SC.SEED, 3)
        assert torch.equal(moved[:, -1], xd[:, -1]), "a column of deviation 0 moved"
        assert not torch.equal(moved[:, num_cat], xd[:, num_cat])


@pytest.mark.parametrize("layout", SC.TAB_LAYOUTS, ids=str)
def test_a_table_of_257_rows_is_one_row_then_256(layout):
    from stil_tta_amd import shift as S
    n_cols, num_cat = layout
    st = S.TableStats(*SC.table_stats(n_cols, num_cat))
    xd = dev(SC.table_input(257, n_cols, num_cat))
    for name, strength in (("tab_noise", 2.0), ("tab_missing", 0.3), ("tab_cat_flip", 0.5)):
        for offset in (0, 1, 2 ** 32 - 5):
            whole = S.tab_shift(xd, st, name, strength, SC.SEED, offset)
            parts = torch.cat([S.tab_shift(xd[:1], st, name, strength, SC.SEED, offset), S.tab_shift(xd[1:], st, name, strength, SC.SEED, offset + n_cols)])
            assert torch.equal(whole, parts), (name, offset)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_out_untouched():
    from stil_tta_amd._lib import lib
    D = lib()._dll
    x = torch.rand(2, 3, 4, 4, device="cuda")
    out = torch.full_like(x, SC.SENT)
    ws = torch.full((6,), SC.SENT, device="cuda")
    t = torch.rand(4, 9, device="cuda")
    tout = torch.full_like(t, SC.SENT)
    cl = torch.tensor([3, 1, 4, 5], dtype=torch.int32, device="cuda")
    on = torch.ones(9, dtype=torch.uint8, device="cuda")
    v = torch.ones(9, device="cuda")
    X, O, T, TO = x.data_ptr(), out.data_ptr(), t.data_ptr(), tout.data_ptr()
    bad = [
        D.stil_shift_noise(X, O, 96, 2, 0.1, 0, 1, 1, 0, None), D.stil_shift_noise(X, O, 96, 0, -0.1, 0, 1, 1, 0, None),
        D.stil_shift_noise(X, O, 96, 1, 1.5, 0, 1, 1, 0, None), D.stil_shift_noise(X, O, 96, 0, 0.1, 1, 0, 1, 0, None),
        D.stil_shift_noise(X, O, 0, 0, 0.1, 0, 1, 1, 0, None), D.stil_shift_noise(None, O, 96, 0, 0.1, 0, 1, 1, 0, None),
        D.stil_shift_contrast(X, O, 2, 3, 16, -1.0, 0, 1, ws.data_ptr(), None), D.stil_shift_contrast(X, O, 2, 3, 16, 0.5, 0, 1, None, None),
        D.stil_shift_contrast(X, O, 0, 3, 16, 0.5, 0, 1, ws.data_ptr(), None),
        D.stil_shift_brightness(X, O, 2, 1, 48, 0.1, 0, 1, None), D.stil_shift_brightness(X, O, 2, 4, 12, 0.1, 0, 1, None),
        D.stil_shift_brightness(X, O, 2, 3, 16, math.nan, 0, 1, None),
        D.stil_shift_pixelate(X, O, 2, 3, 4, 4, 0, None), D.stil_shift_pixelate(X, O, 2, 3, 0, 4, 2, None),
        D.stil_shift_tab(T, TO, 4, 9, 10, cl.data_ptr(), on.data_ptr(), v.data_ptr(), v.data_ptr(), 0, 0.5, 1, 0, None),
        D.stil_shift_tab(T, TO, 4, 9, 4, None, on.data_ptr(), v.data_ptr(), v.data_ptr(), 2, 0.5, 1, 0, None),
        D.stil_shift_tab(T, TO, 4, 9, 4, cl.data_ptr(), on.data_ptr(), v.data_ptr(), v.data_ptr(), 3, 0.5, 1, 0, None),
        D.stil_shift_tab(T, TO, 4, 9, 4, cl.data_ptr(), on.data_ptr(), v.data_ptr(), v.data_ptr(), 1, 1.5, 1, 0, None),
        D.stil_shift_tab(T, TO, 0, 9, 4, cl.data_ptr(), on.data_ptr(), v.data_ptr(), v.data_ptr(), 1, 0.5, 1, 0, None),
    ]
    x0 = x.clone()
    inplace = [D.stil_shift_noise(X, X, 96, 0, 0.1, 0, 1, 1, 0, None), D.stil_shift_contrast(X, X, 2, 3, 16, 0.5, 0, 1, ws.data_ptr(), None),
               D.stil_shift_brightness(X, X, 2, 3, 16, 0.1, 0, 1, None), D.stil_shift_pixelate(X, X, 2, 3, 4, 4, 2, None),
               D.stil_shift_noise(X, X + 64, 80, 0, 0.1, 0, 1, 1, 0, None),
               D.stil_shift_tab(T, T, 4, 9, 4, cl.data_ptr(), on.data_ptr(), v.data_ptr(), v.data_ptr(), 1, 0.5, 1, 0, None)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad + inplace), (bad, inplace)
    assert bool((out == SC.SENT).all() and (tout == SC.SENT).all() and (ws == SC.SENT).all()) and torch.equal(x, x0)


# ------------------------------------------------------------------------------------------ the stream
def _stream_specs(seed=5):
    from stil_tta_amd import shift as S
    st = S.TableStats(*SC.table_stats(9, 4))
    return [S.ShiftSpec(image=("gaussian_noise", 5), tabular=("tab_noise", 5), seed=seed, stats=st),
            S.ShiftSpec(image=("impulse_noise", 5), tabular=("tab_cat_flip", 5), seed=seed, stats=st, columns=[0, 2]),
            S.ShiftSpec(image=("contrast", 3), tabular=("tab_missing", 3), seed=seed, stats=st),
            S.ShiftSpec(image=("brightness", 3), seed=seed), S.ShiftSpec(image=("gaussian_blur", 2), seed=seed),
            S.ShiftSpec(image=("pixelate", 2), seed=seed), S.ShiftSpec(tabular=("tab_noise", 0.5), seed=seed, stats=st, clip=None)]


def _run_stream(spec, img, tab, y, cuts):
    from stil_tta_amd.shift import ShiftStream
    s = ShiftStream(spec)
    imgs, tabs, at = [], [], 0
    for n in cuts:
        out = s(([img[at:at + n], tab[at:at + n], "extra"], y[at:at + n], at))
        assert type(out) is tuple and type(out[0]) is list and out[0][2] == "extra" and out[1] is not None and out[2] == at
        assert torch.equal(out[1], y[at:at + n])
        imgs.append(out[0][0])
        tabs.append(out[0][1])
        at += n
    assert (s.image_drawn, s.table_drawn) == (img.numel(), tab.numel())
    return torch.cat(imgs), torch.cat(tabs)


def test_shift_stream_yields_the_same_samples_however_it_is_cut():
    img = dev(SC.image_input((32, 3, 9, 9), seed=2))          # 243 elements per sample: a cut after 5 samples is odd
    tab = dev(SC.table_input(32, 9, 4, seed=2))
    y = torch.arange(32, device="cuda")
    for spec, other in zip(_stream_specs(5), _stream_specs(6)):
        a_img, a_tab = _run_stream(spec, img, tab, y, (16, 16))
        for cuts in ((8, 8, 8, 8), (5, 27), (32,)):
            b_img, b_tab = _run_stream(spec, img, tab, y, cuts)
            assert torch.equal(a_img, b_img) and torch.equal(a_tab, b_tab), (spec, cuts)
        if spec.image is None:
            assert torch.equal(a_img, img)
        else:
            assert not torch.equal(a_img, img), spec
        if spec.tabular is None:
            assert torch.equal(a_tab, tab)
        else:
            assert not torch.equal(a_tab, tab), spec
        o_img, o_tab = _run_stream(other, img, tab, y, (16, 16))
        if spec.image is not None and spec.image[0] in ("gaussian_noise", "impulse_noise"):
            assert not torch.equal(a_img, o_img), "another seed gives the same images"
        if spec.tabular is not None:
            assert not torch.equal(a_tab, o_tab), "another seed gives the same tables"
    # the two streams of a spec: image elements under seed 2 s, table cells under 2 s + 1, both from counter 0
    spec = _stream_specs(5)[0]
    a_img, a_tab = _run_stream(spec, img, tab, y, (16, 16))
    close(a_img, t64(SC.noise_model(img.cpu().numpy(), 0, 0.38, 0.0, 1.0, 10, 0)), name="stream image")
    cat_len, std, fill = SC.table_stats(9, 4)
    close(a_tab, t64(SC.tab_model(tab.cpu().numpy(), 4, cat_len, np.ones(9), std, fill, 0, 2.0, 11, 0)), name="stream table")


def test_shifted_loader_starts_a_fresh_stream_per_pass():
    from stil_tta_amd.shift import ShiftedLoader
    img, tab = SC.image_input((8, 3, 9, 9), seed=3), SC.table_input(8, 9, 4, seed=3)
    loader = [([torch.from_numpy(img[i:i + 4]), torch.from_numpy(tab[i:i + 4])], torch.arange(i, i + 4)) for i in (0, 4)]
    sl = ShiftedLoader(loader, _stream_specs(5)[0], "cuda")
    one, two = list(sl), list(sl)
    assert len(sl) == 2 and len(one) == 2
    for a, b in zip(one, two):
        assert a[0][0].is_cuda and a[1].is_cuda and torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][1], b[0][1]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------ fit.test / fit.test_shifts
def _fit_setup(tmp_path, n_batches=2):
    import test_gpu_tta as T
    from stil_tta_amd import shift as S
    from stil_tta_amd.modules import split_field_lengths
    hp, sd, mk = T._small()
    loader = [T.tta_batch(hp, 16, 40 + i) for i in range(n_batches)]
    ck = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": {k: v.clone() for k, v in sd.items()}}, ck)
    cat, con = split_field_lengths(hp.field_lengths)
    st = S.TableStats(cat, [1.0] * (len(cat) + len(con)), [0.0] * (len(cat) + len(con)))
    first = S.ShiftSpec(image=("gaussian_noise", 3), tabular=("tab_noise", 3), seed=1, stats=st)
    second = S.ShiftSpec(image=("contrast", 4), tabular=("tab_missing", 2), seed=2, stats=st)
    return T, hp, sd, mk, loader, ck, first, second


def _same_metrics(a, b):
    return a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def _record(model):
    """wrap model.test_step: keep what every call received, and the adapted set A as it stood when the call came in"""
    seen, entering = [], []
    orig = model.test_step
    keys = model.tta_param_names()

    def test_step(batch, i=None):
        seen.append((batch[0][0].clone(), batch[0][1].clone(), batch[1].clone()))
        sd = model.state_dict()
        entering.append({k: sd[k].detach().clone() for k in keys})
        return orig(batch, i)
    model.test_step = test_step
    return seen, entering


def test_fit_test_without_a_shift_is_the_existing_path(tmp_path):
    from stil_tta_amd import fit
    T, hp, sd, mk, loader, ck, first, second = _fit_setup(tmp_path)
    a = mk()
    ra = fit.test(a, loader, ck, shift=None)
    h = mk()
    h.freeze()
    h.acc_test.reset()
    h.auc_test.reset()
    for i, bt in enumerate(loader):
        h.test_step(T.to_dev(bt), i)
    rh = {k: float(v) for k, v in h.test_epoch_end().items()}
    assert _same_metrics(ra, rh), (ra, rh)
    sa, sh = T.full_state(a), T.full_state(h)
    for k in sa:
        assert torch.equal(sa[k], sh[k]), k


def test_fit_test_with_a_shift_feeds_test_step_the_shifted_stream(tmp_path):
    from stil_tta_amd import fit
    from stil_tta_amd.shift import ShiftedLoader, ShiftStream
    T, hp, sd, mk, loader, ck, first, second = _fit_setup(tmp_path)
    a = mk()
    seen, _ = _record(a)
    ra = fit.test(a, loader, ck, shift=first)
    s = ShiftStream(first)
    want = [s(T.to_dev(bt)) for bt in loader]
    assert len(seen) == len(want) == 2
    for (img, tab, y), w in zip(seen, want):
        assert torch.equal(img, w[0][0]) and torch.equal(tab, w[0][1]) and torch.equal(y, w[1])
        assert not torch.equal(img, T.to_dev(loader[0])[0][0])
    for (img, tab, y), w in zip(seen, ShiftedLoader(loader, first, "cuda")):
        assert torch.equal(img, w[0][0]) and torch.equal(tab, w[0][1])
    assert set(ra) == {"test.acc", "test.auc"}


@pytest.mark.parametrize("protocol", ["reset", "continual"])
def test_fit_test_shifts_under_both_protocols(tmp_path, protocol):
    from stil_tta_amd import fit
    T, hp, sd, mk, loader, ck, first, second = _fit_setup(tmp_path)
    m = mk()
    seen, entering = _record(m)
    res = fit.test_shifts(m, loader, {"noise": first, "contrast+missing": second}, ck, protocol=protocol)
    assert list(res) == ["noise", "contrast+missing", "mean"] and len(seen) == 4
    for k in res["noise"]:
        a, b, mean = res["noise"][k], res["contrast+missing"][k], res["mean"][k]
        assert mean == (a + b) / 2 or (mean != mean and (a != a or b != b)), (k, a, b, mean)
    src = {k: v.cuda() for k, v in sd.items()}
    for k, v in entering[0].items():
        assert torch.equal(v, src[k]), k
    assert any(not torch.equal(v, src[k]) for k, v in entering[1].items()), "the first batch adapted nothing"
    f = mk()
    f_seen, _ = _record(f)
    alone = fit.test(f, loader, ck, shift=second)
    for a, b in zip(seen[2:], f_seen):                      # the second shift's stream starts afresh under either protocol
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    if protocol == "reset":
        for k, v in entering[2].items():
            assert torch.equal(v, src[k]), k
        assert _same_metrics(res["contrast+missing"], alone), (res["contrast+missing"], alone)
        sa, sf = T.full_state(m), T.full_state(f)
        for k in sa:
            assert torch.equal(sa[k], sf[k]), k
    else:
        assert any(not torch.equal(v, src[k]) for k, v in entering[2].items()), "continual: the second shift started from the source values"
        sa, sf = T.full_state(m), T.full_state(f)
        assert any(not torch.equal(sa[k], sf[k]) for k in m.tta_param_names())
    with pytest.raises(ValueError):
        fit.test_shifts(m, loader, {"noise": first}, protocol="episodic")
    with pytest.raises(ValueError):
        fit.test_shifts(m, loader, {"mean": first})
    with pytest.raises(ValueError):
        fit.test_shifts(m, loader, {})
