"""The four kernels that carry the unsupervised loss of the Match baselines (csrc/loss.hip: stil_contrast_graph,
stil_simmatch_unfold, stil_freematch_update, stil_freematch_entropy), called through the C ABI at the cases of
tests/match_cases.py and compared with the float64 references there, never with another kernel of the library.

Floats: the suite's `close()` at `TOL` for row_loss and the loss scalars, `rel_close` for everything whose magnitude is far below
1 (dS, dz, teacher, pseudo, p_model, label_hist, time_p); tests/test_match_cases_cpu.py asserts on the CPU that fp32 ATen meets
the same checks (the `check_*` functions below) on the same inputs, so a kernel that misses one is wrong, not unlucky.
Exact: argmax, one-hot, masks (planted, tie rows and the row ON its threshold included), zeros where the definition has zeros,
NULL optional outputs and padded leading dimensions against the plain call bit for bit, a second call bit for bit, sentinels
round every output, inputs untouched."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cases as M  # noqa: E402
from test_gpu_entry_points import NAN, SENT, TOL, P, _release_operands, _st, close, dev, out_strided, rel_close, strided  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ISENT = -5


@pytest.fixture(scope="module")
def ops():
    from stil_tta_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from stil_tta_amd._lib import lib
    return lib()


def sent(*shape, dtype=torch.float32, fill=SENT):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def bits(t):
    """the raw words of a float tensor on the host: equality of these is bit-for-bit equality (NaN and -0.0 included)"""
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# the float checks, shared with the CPU test (which feeds them fp32 ATen instead of the kernel)
# ---------------------------------------------------------------------------------------------------------------------
def check_contrast(out, ref):
    """N = 1: p = 1 whatever S holds, so dS is identically zero and float64 autograd leaves only its rounding noise: close()
    there (as for a constant entropy loss below), rel_close() at every other width"""
    close(out["row_loss"], ref["row_loss"], name="row_loss")
    if out.get("dS") is not None:
        if ref["dS"].shape[1] == 1:
            close(out["dS"], ref["dS"], name="dS (one column: constant loss)")
        else:
            rel_close(out["dS"], ref["dS"], "dS")


def check_unfold(out, ref):
    rel_close(out["teacher"], ref["teacher"], "teacher")
    if out.get("pseudo") is not None:
        rel_close(out["pseudo"], ref["pseudo"], "pseudo")


def check_update(out, ref):
    for k in ("p_model", "label_hist", "time_p"):
        rel_close(out[k], ref[k], k)


def check_entropy(out, ref, has_gradient):
    """dz is identically zero in float64 where the selected rows predict one class: close() there, rel_close() elsewhere"""
    close(out["loss"], ref["loss"], name="entropy loss")
    if has_gradient:
        rel_close(out["dz"], ref["dz"], "dz")
    else:
        close(out["dz"], ref["dz"], name="dz (constant loss)")


# =====================================================================================================================
# stil_contrast_graph
# =====================================================================================================================
def _contrast(L, c, th, inv_rows, pad=0, want_dS=True):
    """-> (row_loss [rows], dS [rows, N] or None) on the host, after the sentinel and input checks of one launch"""
    rows, N = c["rows"], c["N"]
    if pad:
        Sb, Sv = strided(c["S"], pad)
        Qb, Qv = strided(c["Q"], pad)
    else:
        Sb = Sv = dev(c["S"])
        Qb = Qv = dev(c["Q"])
    S0, Q0 = bits(Sb), bits(Qb)
    rl = sent(rows + 1)
    ldd = N + pad if want_dS else 0                     # ldd is not looked at without dS
    db = sent(rows + 1, N + pad) if want_dS else None
    L.contrast_graph(P(Sv), N + pad, P(Qv), N + pad, th, P(rl), P(db), ldd, rows, N, inv_rows, _st())
    torch.cuda.synchronize()
    assert float(rl[rows]) == SENT, "row_loss: a write past the last row"
    assert torch.equal(bits(Sb), S0) and torch.equal(bits(Qb), Q0), "an input changed"
    if db is None:
        return rl[:rows].cpu(), None
    assert bool((db[rows] == SENT).all()) and bool((db[:, N:] == SENT).all()), "dS: a write into the padding or past the last row"
    return rl[:rows].cpu(), db[:rows, :N].cpu()


@pytest.mark.parametrize("inv_rows", M.CONTRAST_INV_ROWS)
@pytest.mark.parametrize("rows,N", M.CONTRAST_TABLE)
def test_contrast_graph_against_float64(L, rows, N, inv_rows):
    c = M.contrast_case(rows, N)
    inv = 1.0 / rows if inv_rows is None else inv_rows
    rl, dS = _contrast(L, c, c["th"], inv)
    check_contrast({"row_loss": rl, "dS": dS}, M.contrast_reference(c["S"], c["Q"], c["th"], inv, torch.float64))
    rl2, dS2 = _contrast(L, c, c["th"], inv)
    assert same_bits(rl, rl2) and same_bits(dS, dS2), "a second identical call differs"
    rl3, none = _contrast(L, c, c["th"], inv, want_dS=False)
    assert none is None and same_bits(rl, rl3), "dS = NULL changes row_loss"
    rl4, dS4 = _contrast(L, c, c["th"], inv, pad=M.PAD)
    assert same_bits(rl, rl4) and same_bits(dS, dS4), "lds = ldq = ldd = N + 3 changes the result"
    rl5, _ = _contrast(L, c, c["th"], inv, pad=M.PAD, want_dS=False)
    assert same_bits(rl, rl5)


def test_contrast_graph_row_without_an_edge_gives_zero(L):
    """present behaviour, pinned: with no Q >= threshold in a row (a threshold above 1, or a diagonal that is not 1) the
    kernel returns row_loss = 0 and dS = 0 where the reference's 0 / 0 gives NaN"""
    rows, N, th = M.CONTRAST_NO_EDGE
    c = M.contrast_case(rows, N)
    assert not bool((c["Q"] >= th).any())
    rl, dS = _contrast(L, c, th, 1.0 / rows)
    assert bool((rl == 0).all()) and bool((dS == 0).all())


def test_contrast_graph_fn_scales_by_the_upstream_gradient(L, ops):
    rows, N = 3, 257
    c = M.contrast_case(rows, N)
    Sd, Qd = dev(c["S"]).requires_grad_(), dev(c["Q"])
    loss = ops.ContrastGraphFn.apply(Sd, Qd, c["th"])
    (3.0 * loss).backward()
    ref = M.contrast_reference(c["S"], c["Q"], c["th"], 1.0 / rows, torch.float64)
    close(loss, ref["mean"], name="loss")
    rel_close(Sd.grad, 3.0 * ref["dS"], "dS under an upstream gradient of 3")
    _, dS = _contrast(L, c, c["th"], 1.0 / rows)
    scaled = sent(rows * N + 1)
    L.scale_dev(P(dev(dS)), P(dev(torch.tensor([3.0]))), 1.0, P(scaled), rows * N, _st())
    torch.cuda.synchronize()
    assert float(scaled[rows * N]) == SENT and same_bits(Sd.grad.flatten(), scaled[:rows * N]), "the gradient is not scale_dev(dS, 3)"
    assert not same_bits(Sd.grad, dS)


# =====================================================================================================================
# stil_simmatch_unfold
# =====================================================================================================================
def _margins(rows, cols):
    """a sentinel buffer of rows + 2 PAD rows and its inner [rows, cols] view: the kernel writes the view only"""
    buf = sent(rows + 2 * M.PAD, cols)
    return buf, buf[M.PAD:M.PAD + rows]


def _margins_hold(buf, rows):
    return bool((buf[:M.PAD] == SENT).all()) and bool((buf[M.PAD + rows:] == SENT).all())


def _unfold(L, tpo, probs, labels, c_smooth, want_pseudo=True):
    R, N = tpo.shape
    K = probs.shape[1]
    td, pd, ld = dev(tpo), dev(probs), dev(labels)
    tb, tv = _margins(R, N)
    pb, pv = _margins(R, K) if want_pseudo else (None, None)
    L.simmatch_unfold(P(td), P(pd), P(ld), P(tv), P(pv), R, N, K, c_smooth, _st())
    torch.cuda.synchronize()
    assert _margins_hold(tb, R) and (pb is None or _margins_hold(pb, R)), "a write outside the output"
    assert same_bits(td, tpo) and same_bits(pd, probs) and torch.equal(ld.cpu(), labels), "an input changed"
    return tv.cpu(), None if pv is None else pv.cpu()


@pytest.mark.parametrize("c_smooth", M.UNFOLD_CS)
@pytest.mark.parametrize("R,N,K", M.UNFOLD_TABLE)
def test_simmatch_unfold_against_float64(L, R, N, K, c_smooth):
    tpo, probs, labels = M.unfold_case(R, N, K)
    assert int(labels.min()) >= 0 and int(labels.max()) < K, "an out-of-range label is an out-of-bounds read: never launched"
    teacher, pseudo = _unfold(L, tpo, probs, labels, c_smooth)
    ref = M.unfold_reference(tpo, probs, labels, c_smooth, torch.float64)
    check_unfold({"teacher": teacher, "pseudo": pseudo}, ref)
    assert float((teacher.double().sum(1) - 1.0).abs().max()) <= TOL and float((pseudo.double().sum(1) - 1.0).abs().max()) <= TOL
    if c_smooth >= 1.0:
        assert same_bits(pseudo, probs), "c_smooth = 1: the pseudo-label is the class probability itself"
    if c_smooth == 0.0 and K > 1:
        assert bool((pseudo[:, 0] == 0).all()), "a class without a bank entry aggregates nothing"
    t2, p2 = _unfold(L, tpo, probs, labels, c_smooth)
    assert same_bits(teacher, t2) and same_bits(pseudo, p2), "a second identical call differs"
    t3, none = _unfold(L, tpo, probs, labels, c_smooth, want_pseudo=False)
    assert none is None and same_bits(teacher, t3), "pseudo = NULL changes teacher"


# =====================================================================================================================
# stil_freematch_update
# =====================================================================================================================
def _state(c):
    """the three state vectors inside sentinel margins -> (buffers, views)"""
    bufs, views = [], []
    for k in ("p_model", "label_hist", "time_p"):
        n = c[k].numel()
        b = sent(n + 2)
        b[1:n + 1] = c[k].cuda()
        bufs.append(b); views.append(b[1:n + 1])
    return bufs, views


def _update(L, probs, views, momentum):
    R, K = probs.shape
    pd = dev(probs)
    mask, onehot, idx, scratch = sent(R + 1), sent(R + 1, K), sent(R + 1, dtype=torch.int32, fill=ISENT), sent(R + 1)
    L.freematch_update(P(pd), R, K, P(views[0]), P(views[1]), P(views[2]), momentum, P(mask), P(onehot), P(idx), P(scratch), _st())
    torch.cuda.synchronize()
    assert float(mask[R]) == SENT and bool((onehot[R] == SENT).all()) and int(idx[R]) == ISENT and float(scratch[R]) == SENT, "a write past the last row"
    assert same_bits(pd, probs), "an input changed"
    return {"mask": mask[:R].cpu(), "onehot": onehot[:R].cpu(), "idx": idx[:R].cpu(), "p_model": views[0].cpu(), "label_hist": views[1].cpu(),
            "time_p": views[2].cpu()}


@pytest.mark.parametrize("momentum", M.UPDATE_MOMENTA)
@pytest.mark.parametrize("R,K", M.UPDATE_TABLE)
def test_freematch_update_two_calls_against_float64(L, R, K, momentum):
    c = M.update_case(R, K, momentum)
    refs = M.update_run_reference(c, torch.float64)
    bufs, views = _state(c)
    first = None
    for call, ((probs, top, ties), ref) in enumerate(zip(c["calls"], refs)):
        before = [v.cpu() for v in views]
        out = _update(L, probs, views, momentum)        # in place: the second call starts from what the first one left
        first = first or out
        assert all(float(b[0]) == SENT and float(b[-1]) == SENT for b in bufs), "a write outside the state"
        assert torch.equal(out["idx"].long(), top), (call, out["idx"].tolist(), top.tolist())
        assert torch.equal(out["onehot"], F.one_hot(top, K).float()) and bool((out["onehot"].sum(1) == 1).all())
        for t, c0, c1 in ties:
            assert float(probs[t, c0]) == float(probs[t, c1]) == float(probs[t].max()) and int(out["idx"][t]) == c0 < c1, "the first maximum wins"
        check_update(out, ref)
        assert torch.equal(out["mask"], ref["mask"]), (call, torch.nonzero(out["mask"] != ref["mask"]).flatten().tolist())
        if momentum == 1.0:
            assert all(same_bits(out[k], b) for k, b in zip(("p_model", "label_hist", "time_p"), before)), "momentum 1 moves the state"
        if M.update_at_threshold(R, momentum):
            i = int(out["idx"][0])
            assert same_bits(out["time_p"], probs[0, i:i + 1]) and float(out["p_model"][i] / out["p_model"].max()) == 1.0
            assert float(out["mask"][0]) == 1.0, "a row ON its threshold is selected: >=, not >"
    _, views2 = _state(c)
    again = _update(L, c["calls"][0][0], views2, momentum)
    assert all(same_bits(first[k], again[k]) for k in first), "the first call, repeated from the same state, differs"


# =====================================================================================================================
# stil_freematch_entropy
# =====================================================================================================================
def _entropy(L, c, mask):
    R, K = c["R"], c["K"]
    zd, md, pmd, lhd = dev(c["z"]), dev(mask), dev(c["p_model"]), dev(c["label_hist"])
    loss, dz, Ps, pred, vec = sent(2), sent(R + 1, K), sent(R + 1, K), sent(R + 1, dtype=torch.int32, fill=ISENT), sent(4 * K + 1)
    L.freematch_entropy(P(zd), P(md), R, K, P(pmd), P(lhd), P(loss), P(dz), P(Ps), P(pred), P(vec), _st())
    torch.cuda.synchronize()
    assert float(loss[1]) == SENT and bool((dz[R] == SENT).all()) and bool((Ps[R] == SENT).all()) and int(pred[R]) == ISENT and float(vec[4 * K]) == SENT, \
        "a write past an output or a scratch buffer"
    assert same_bits(zd, c["z"]) and same_bits(md, mask) and same_bits(pmd, c["p_model"]) and same_bits(lhd, c["label_hist"]), "an input changed"
    return {"loss": loss[0].cpu(), "dz": dz[:R].cpu(), "pred": pred[:R].cpu()}


@pytest.mark.parametrize("kind", M.ENTROPY_MASKS)
@pytest.mark.parametrize("R,K", M.ENTROPY_TABLE)
def test_freematch_entropy_against_float64(L, R, K, kind):
    c, mask = M.entropy_case(R, K), M.entropy_mask(R, kind)
    sel = mask != 0
    out = _entropy(L, c, mask)
    if not bool(sel.any()):
        assert float(out["loss"]) == 0.0 and bool((out["dz"] == 0).all()), "an empty mask: loss 0 and dz 0, exactly"
    else:
        check_entropy(out, M.entropy_reference(c, mask, torch.float64), M.entropy_has_gradient(c, mask))
        assert torch.equal(out["pred"][sel].long(), c["top"][sel]) and bool((out["pred"][~sel] == -1).all()), "the first maximum wins"
        assert bool((out["dz"][~sel] == 0).all()), "a row outside the mask has a gradient"
    again = _entropy(L, c, mask)
    assert same_bits(out["loss"], again["loss"]) and same_bits(out["dz"], again["dz"]), "a second identical call differs"


def test_freematch_entropy_fn_scales_by_the_upstream_gradient(L, ops):
    R, K = 257, 3
    c, mask = M.entropy_case(R, K), M.entropy_mask(R, "mixed")
    zd = dev(c["z"]).requires_grad_()
    loss = ops.FreeMatchEntropyFn.apply(zd, dev(mask), dev(c["p_model"]), dev(c["label_hist"]))
    (3.0 * loss).backward()
    ref = M.entropy_reference(c, mask, torch.float64)
    close(loss, ref["loss"], name="loss")
    rel_close(zd.grad, 3.0 * ref["dz"], "dz under an upstream gradient of 3")
    dz = _entropy(L, c, mask)["dz"]
    scaled = sent(R * K + 1)
    L.scale_dev(P(dev(dz)), P(dev(torch.tensor([3.0]))), 1.0, P(scaled), R * K, _st())
    torch.cuda.synchronize()
    assert float(scaled[R * K]) == SENT and same_bits(zd.grad.flatten(), scaled[:R * K]), "the gradient is not scale_dev(dz, 3)"
    assert not same_bits(zd.grad, dz)
