"""RoTTA test-time adaptation (Yuan, Xie, Li, CVPR 2023, "Robust Test-Time Adaptation in Dynamic Scenarios"; definition as
recalled: unpinned) in STiLModel.test_step, on top of TENT (tests/test_gpu_tta.py) and the BatchNorm memory (tests/test_gpu_bnmemory.py).

1. stil_rotta_bank_update against the walk restated in tests/rotta_cases.py: every decision and count exactly, unc and p under close()
   at TOL, lse / p / H stil_entropy_rows' bits, sentinels, repetition, one call against one call per sample, a one-class stream.
2. stil_rotta_bank_store: a bit-exact gather on the scalar and the vector path, misaligned bases, untouched slots.
3. stil_rotta_rows against float64 autograd; an empty bank; grad_scale; empty slots.
4. stil_rotta_exchange and stil_rotta_teacher against float64: inactive, padding and out-of-range chunks untouched.
5. Every entry point refuses bad arguments with nothing written.
6. The step against RoTTA restated in float64 on the oracle, on the device's ReLU / max-pool decisions, two consecutive batches.
7. The properties of the step.
tests/test_rotta_cpu.py checks on the CPU that the inputs of checks 1 and 3 are well-conditioned."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import rotta_cases as C  # noqa: E402
from rotta_cases import f32  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
import test_gpu_bnmemory as BM  # noqa: E402
import test_gpu_eata as E  # noqa: E402
import test_gpu_shot as G  # noqa: E402
import test_gpu_tta as T  # noqa: E402

SENTINEL = -7.25
ISENT = -77
BANK_KEYS = ("label", "unc", "age", "occ", "n")


# ------------------------------------------------------------------------------------------ check 1: the bank's bookkeeping
def _bank_dev(bank, N, K):
    """the bank on the device, one sentinel past every vector"""
    out = {}
    for k, size in (("label", N), ("unc", N), ("age", N), ("occ", K), ("n", 1)):
        t = torch.full((size + 1,), SENTINEL if k == "unc" else ISENT, dtype=torch.float32 if k == "unc" else torch.int32)
        t[:size] = torch.from_numpy(np.asarray(bank[k]))
        out[k] = t.cuda()
    return out


def _run_update(L, zb, ld, B, K, N, dev_bank, lt=C.LAMBDA_T, lu=C.LAMBDA_U):
    """one call on the rows [0, B) of zb (stride ld); dev_bank is moved in place.  -> the outputs on the CPU, sentinels included"""
    full = lambda shape, dtype=torch.float32: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")  # noqa: E731
    ifull = lambda shape, dtype=torch.int32: torch.full(shape, ISENT % 256 if dtype == torch.uint8 else ISENT, dtype=dtype, device="cuda")  # noqa: E731
    o = dict(lse=full((B + 1,), torch.float64), p=full((B + 1, ld)), H=full((B + 1,)), yhat=ifull((B + 1,)), owner=ifull((N + 1,)),
             accepted=ifull((B + 1,), torch.uint8), slot_of=ifull((B + 1,)), counts=ifull((5,)))
    q = {k: v.data_ptr() for k, v in o.items()}
    b = {k: v.data_ptr() for k, v in dev_bank.items()}
    L.rotta_bank_update(zb.data_ptr(), ld, B, K, N, f32(lt), f32(lu), b["label"], b["unc"], b["age"], b["occ"], b["n"], q["owner"], q["lse"],
                        q["p"], ld, q["H"], q["yhat"], q["accepted"], q["slot_of"], q["counts"], None)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in o.items()}
    out.update({k: v.cpu() for k, v in dev_bank.items()})
    return out


def _check_update(a, ref, N, K, B, ld):
    """a: _run_update's outputs; ref: bank_walk's dict (plus lse, p, H, yhat)"""
    for k, size in (("label", N), ("age", N), ("occ", K), ("n", 1), ("owner", N), ("slot_of", B), ("counts", 4)):
        assert np.array_equal(a[k][:size].numpy(), ref[k]), (k, a[k][:size].tolist(), ref[k].tolist())
        assert int(a[k][size]) == ISENT, f"{k}: the entry past the end was written"
    assert np.array_equal(a["accepted"][:B].numpy(), ref["accepted"]) and int(a["accepted"][B]) == ISENT % 256
    assert torch.equal(a["yhat"][:B], ref["yhat"]) and int(a["yhat"][B]) == ISENT
    close(a["unc"][:N], torch.from_numpy(ref["unc"]), name="unc")
    close(a["p"][:B, :K], ref["p"], name="p")
    close(a["lse"][:B], ref["lse"], name="lse")
    close(a["H"][:B], ref["H"], name="H")
    assert float(a["unc"][N]) == SENTINEL and float(a["lse"][B]) == SENTINEL and float(a["H"][B]) == SENTINEL
    assert bool((a["p"][B] == SENTINEL).all()) and (ld == K or bool((a["p"][:, K:] == SENTINEL).all()))
    n = int(a["n"][0])
    assert bool((a["label"][:n] >= 0).all()) and bool((a["label"][n:N] == -1).all()), "the filled slots are not the prefix"
    # a slot an accepted sample took holds that sample's entropy, bit for bit
    for s, b in enumerate(a["owner"][:N].tolist()):
        if b >= 0:
            assert float(a["unc"][s]) == float(a["H"][b]) and int(a["label"][s]) == int(a["yhat"][b])


@pytest.mark.parametrize("N,K,B,start", C.update_cases())
def test_bank_update_against_the_restatement(N, K, B, start):
    from stil_tta_amd._lib import lib
    L = lib()
    z, bank, ref = C.update_case(N, K, B, start)
    for pad in (0, 3):
        ld = K + pad
        zb = G._padded(z, B, K, pad)
        a, b = (_run_update(L, zb, ld, B, K, N, _bank_dev(bank, N, K)) for _ in range(2))
        for k in a:
            assert torch.equal(a[k], b[k]), f"{k}: not bit-identical on repetition"
        _check_update(a, ref, N, K, B, ld)
        t = G._run_entropy(L, zb, ld, B, K, 1.0)
        assert torch.equal(a["lse"][:B], t["lse"]) and torch.equal(a["H"][:B], t["H"]) and torch.equal(a["p"][:B, :K], t["p"])


@pytest.mark.parametrize("N,K,B,start", [c for c in C.update_cases() if c[2] > 1 and c[0] > 1])
def test_one_call_equals_one_call_per_sample(N, K, B, start):
    from stil_tta_amd._lib import lib
    L = lib()
    z, bank, ref = C.update_case(N, K, B, start)
    zb = G._padded(z, B, K, 3)
    whole = _run_update(L, zb, K + 3, B, K, N, _bank_dev(bank, N, K))
    dev = _bank_dev(bank, N, K)
    acc, slots = [], []
    for b in range(B):
        one = _run_update(L, zb[b:], K + 3, 1, K, N, dev)
        acc.append(int(one["accepted"][0]))
        slots.append(int(one["slot_of"][0]))
        assert one["owner"][:N].tolist() == [0 if s == slots[-1] else -1 for s in range(N)]
        assert one["counts"][:4].tolist()[0] == acc[-1] and one["counts"][:4].tolist()[2:] == [int(one["n"][0]), 0]
        assert torch.equal(one["lse"][:1], whole["lse"][b:b + 1]) and torch.equal(one["p"][0, :K], whole["p"][b, :K])
    assert acc == whole["accepted"][:B].tolist() and slots == whole["slot_of"][:B].tolist()
    for k in BANK_KEYS:
        assert torch.equal(one[k], whole[k]), f"{k}: B calls on one sample each differ from one call on B samples"


def test_a_one_class_stream_is_held_to_its_share():
    from stil_tta_amd._lib import lib
    L = lib()
    N, K, B, c = 8, 5, 70, 2
    z = C.one_class_stream(B, K, c)
    bank = C.start_bank(N, K, "empty", 0)
    _, _, H, yhat = C.rows_ref(z)
    assert bool((yhat == c).all())
    ref = C.bank_walk(H.numpy(), yhat.numpy(), N, K, bank)
    a = _run_update(L, z.cuda(), K, B, K, N, _bank_dev(bank, N, K))
    assert a["occ"][:K].tolist() == ref["occ"].tolist() == [0, 0, 2, 0, 0] and int(a["n"][0]) == 2
    assert a["label"][:N].tolist() == [c, c] + [-1] * (N - 2)
    if ref["margin"] >= C.MIN_MARGIN:
        assert np.array_equal(a["slot_of"][:B].numpy(), ref["slot_of"]) and np.array_equal(a["age"][:N].numpy(), ref["age"])
    # an age at the top of its range stays there
    bank = C.start_bank(N, K, "full", 1)
    bank["age"][:] = C.INT_MAX - 1
    a = _run_update(L, z.cuda()[:3].contiguous(), K, 3, K, N, _bank_dev(bank, N, K), lt=0.0, lu=0.0)   # lambdas 0: nothing is accepted
    assert a["counts"][:4].tolist() == [0, 0, N, 0] and bool((a["age"][:N] == C.INT_MAX).all())


# ------------------------------------------------------------------------------------------ check 2: the gather
@pytest.mark.parametrize("shape,tabw,off", [((3, 5, 7), 1, 0), ((3, 5, 7), 17, 0), ((3, 16, 16), 1, 0), ((3, 16, 16), 17, 0), ((3, 16, 16), 16, 0),
                                           ((3, 16, 16), 16, 1), ((3, 40, 40), 4, 0)])
def test_bank_store_is_a_bit_exact_gather(shape, tabw, off):
    """3x5x7 floats: the scalar path; 3x16x16: the vector path; 3x40x40 = 4800 floats: a second, ragged chunk; off = 1: every base
    one float off its 16-byte boundary, which sends an otherwise vector-sized row down the scalar path."""
    from stil_tta_amd._lib import lib
    L = lib()
    N, B = 6, 5
    F = int(np.prod(shape))
    g = torch.Generator().manual_seed(F + tabw)

    def buf(rows, width, fill=None):
        t = torch.randn(off + rows * width + 1, generator=g) if fill is None else torch.full((off + rows * width + 1,), fill)
        t[-1] = SENTINEL
        return t.cuda()

    x_img, x_tab = buf(B, F), buf(B, tabw)
    bank_img, bank_tab = buf(N, F, 0.5), buf(N, tabw, 0.5)
    owner = torch.tensor([3, -1, 0, 4, -1, 7, ISENT], dtype=torch.int32).cuda()   # 7 >= B: out of range, the slot is left alone
    before_img, before_tab = bank_img.clone(), bank_tab.clone()
    ptr = lambda t: t.data_ptr() + 4 * off  # noqa: E731
    L.rotta_bank_store(ptr(x_img), ptr(x_tab), owner.data_ptr(), N, B, F, tabw, ptr(bank_img), ptr(bank_tab), None)
    torch.cuda.synchronize()
    for got, before, src, w in ((bank_img, before_img, x_img, F), (bank_tab, before_tab, x_tab, tabw)):
        got, before, src = got.cpu(), before.cpu(), src.cpu()
        for s, o in enumerate(owner[:N].tolist()):
            want = src[off + o * w: off + (o + 1) * w] if 0 <= o < B else before[off + s * w: off + (s + 1) * w]
            assert torch.equal(got[off + s * w: off + (s + 1) * w], want), f"slot {s} (owner {o}), width {w}"
        assert float(got[-1]) == SENTINEL and torch.equal(got[:off], before[:off])
    assert float(x_img[-1]) == SENTINEL and float(x_tab[-1]) == SENTINEL


# ------------------------------------------------------------------------------------------ check 3: the loss on the bank
def _run_rows(L, zs, zt, label, age, rows, K, pad, gs=1.0, gate=True):
    ld = K + pad
    full = lambda shape, dtype=torch.float32: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")  # noqa: E731
    o = dict(ce=full((rows + 1,)), w=full((rows + 1,)), dZ=full((rows + 1, ld)), counts=torch.full((5,), ISENT, dtype=torch.int32, device="cuda"),
             loss=full((2,)), ws=full((4 * rows + 1,), torch.float64), gate=torch.full((4,), 9, dtype=torch.uint8, device="cuda"))
    active = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()
    q = {k: v.data_ptr() for k, v in o.items()}
    zsb, ztb = G._padded(zs, rows, K, pad), G._padded(zt, rows, K, pad)
    lab, ag = label.cuda(), age.cuda()
    L.rotta_rows(zsb.data_ptr(), ld, ztb.data_ptr(), ld, lab.data_ptr(), ag.data_ptr(), rows, K, gs, q["ce"], q["w"], q["dZ"], ld, q["counts"],
                 q["loss"], active.data_ptr() if gate else None, q["gate"] if gate else None, 3 if gate else 0, q["ws"], None)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize("rows,K,ages", C.loss_cases())
def test_rotta_rows_against_float64(rows, K, ages):
    from stil_tta_amd._lib import lib
    L = lib()
    zs, zt, label, age = C.loss_input(rows, K, ages)
    ref = C.loss_ref64(rows, K, ages)
    gs = f32(0.37)
    for pad in (0, 3):
        a, b = (_run_rows(L, zs, zt, label, age, rows, K, pad, gs) for _ in range(2))
        for k in a:
            if k != "ws":
                assert torch.equal(a[k], b[k]), f"{k}: not bit-identical on repetition"
        assert a["counts"].tolist() == [ref["n"], rows, 0, 0, ISENT]
        close(a["loss"][:1], ref["loss"].view(1), name="loss")
        close(a["ce"][:rows], ref["ce"], name="ce")
        close(a["w"][:rows], ref["w"], name="w")
        close(a["dZ"][:rows, :K], ref["grad"] * gs, name="dZ")
        one = _run_rows(L, zs, zt, label, age, rows, K, pad, 1.0)
        close(one["dZ"][:rows, :K], ref["grad"], name="dZ at grad_scale 1")
        assert torch.equal(one["loss"], a["loss"]) and torch.equal(one["w"], a["w"])
        assert bool((a["dZ"][:rows, :K][label < 0] == 0).all()) and bool((a["w"][:rows][label < 0] == 0).all()), "an empty slot has a gradient"
        assert float(a["ce"][rows]) == SENTINEL and float(a["w"][rows]) == SENTINEL and float(a["loss"][1]) == SENTINEL
        assert bool((a["dZ"][rows] == SENTINEL).all()) and (pad == 0 or bool((a["dZ"][:, K:] == SENTINEL).all()))
        assert float(a["ws"][4 * rows]) == SENTINEL
        assert a["gate"].tolist() == [1, 0, 1, 9], "the gate is active and n > 0"
        if ages == "huge":
            assert float(a["loss"][0]) == 0.0 and bool((a["dZ"][:rows, :K] == 0).all()) and bool((a["w"][:rows] == 0).all())
        no_gate = _run_rows(L, zs, zt, label, age, rows, K, pad, gs, gate=False)
        assert no_gate["gate"].tolist() == [9, 9, 9, 9] and torch.equal(no_gate["dZ"], a["dZ"])


def test_rotta_rows_on_an_empty_bank():
    from stil_tta_amd._lib import lib
    L = lib()
    rows, K = 5, 7
    zs, zt, label, age = C.loss_input(rows, K, "mixed")
    a = _run_rows(L, zs, zt, torch.full_like(label, -1), age, rows, K, 3)
    assert a["counts"].tolist() == [0, rows, 0, 0, ISENT] and float(a["loss"][0]) == 0.0
    assert bool((a["dZ"][:rows, :K] == 0).all()) and bool((a["dZ"][:, K:] == SENTINEL).all())
    assert a["gate"].tolist() == [0, 0, 0, 9], "an empty bank leaves the gate open"


# ------------------------------------------------------------------------------------------ check 4: the teacher over A
def _slab():
    n, params, _, theta0, _ = E.slab_input()
    c2t = torch.tensor(E.C2T, dtype=torch.int32).cuda()
    act = torch.tensor(E.ACTIVE, dtype=torch.uint8).cuda()
    ach = torch.tensor(E.ACHUNKS, dtype=torch.int32).cuda()
    return n, params, theta0, c2t, act, ach


def test_exchange_and_teacher_against_float64():
    from stil_tta_amd._lib import lib
    L = lib()
    n, params, teacher, c2t, act, ach = _slab()
    tail = (ach.data_ptr(), len(E.ACHUNKS), c2t.data_ptr(), act.data_ptr(), len(E.ACTIVE), n)
    live_of = {ch: j for j, ch in enumerate(E.ACHUNKS) if ch in E.LIVE}
    chunk = lambda t, i: t[i * 1024:(i + 1) * 1024]  # noqa: E731
    P, Tt = params.cuda(), teacher.cuda()
    L.rotta_exchange(P.data_ptr(), Tt.data_ptr(), *tail, None)
    torch.cuda.synchronize()
    p1, t1 = P.cpu(), Tt.cpu()
    for ch in range(len(E.C2T) + 1):       # the last is the sentinel chunk past the slab
        want = chunk(teacher, live_of[ch]) if ch in live_of else chunk(params, ch)
        assert torch.equal(chunk(p1, ch), want), f"exchange: slab chunk {ch}"
    for j, ch in enumerate(E.ACHUNKS):
        want = chunk(params, ch) if ch in live_of else chunk(teacher, j)
        assert torch.equal(chunk(t1, j), want), f"exchange: teacher chunk {j}"
    assert not torch.equal(p1, params)
    L.rotta_exchange(P.data_ptr(), Tt.data_ptr(), *tail, None)
    torch.cuda.synchronize()
    assert torch.equal(P.cpu(), params) and torch.equal(Tt.cpu(), teacher), "swapping twice is not the identity"
    for nu in (0.0, 1.0, 0.001, 0.3):
        outs = []
        for _ in range(2):
            P, Tt = params.cuda(), teacher.cuda()
            L.rotta_teacher(P.data_ptr(), Tt.data_ptr(), *tail, f32(nu), None)
            torch.cuda.synchronize()
            assert torch.equal(P.cpu(), params), "the teacher's average wrote A"
            outs.append(Tt.cpu())
        assert torch.equal(outs[0], outs[1])
        for j, ch in enumerate(E.ACHUNKS):
            want = C.teacher_ref(chunk(teacher, j), chunk(params, ch), nu) if ch in live_of else chunk(teacher, j)
            assert torch.equal(chunk(outs[0], j), want), f"nu {nu}: teacher chunk {j} (slab chunk {ch})"
        if nu == 0.0:
            assert torch.equal(outs[0], teacher)
        if nu == 1.0:
            assert all(torch.equal(chunk(outs[0], j), chunk(params, ch)) for ch, j in live_of.items())
    # a closed gate (every tensor inactive) moves nothing
    P, Tt = params.cuda(), teacher.cuda()
    closed = torch.zeros(len(E.ACTIVE), dtype=torch.uint8).cuda()
    L.rotta_teacher(P.data_ptr(), Tt.data_ptr(), *tail[:3], closed.data_ptr(), *tail[4:], 0.5, None)
    L.rotta_exchange(P.data_ptr(), Tt.data_ptr(), *tail[:3], closed.data_ptr(), *tail[4:], None)
    L.rotta_exchange(P.data_ptr(), Tt.data_ptr(), tail[0], 0, *tail[2:], None)
    torch.cuda.synchronize()
    assert torch.equal(P.cpu(), params) and torch.equal(Tt.cpu(), teacher)


# ------------------------------------------------------------------------------------------ check 5: bad arguments
def test_entry_points_reject_bad_arguments_with_nothing_written():
    from stil_tta_amd._lib import lib
    L = lib()
    D = L._dll
    c32, lng, nan, inf = ctypes.c_float, ctypes.c_long, float("nan"), float("inf")
    B, K, N, F, W = 4, 8, 4, 48, 5
    dev = "cuda"
    shapes = dict(z=(B, K), zt=(N, K), p=(B, K), dz=(N, K), label=(N,), unc=(N,), age=(N,), occ=(K,), n=(1,), owner=(N,), lse=(B,), H=(B,), yhat=(B,),
                  accepted=(B,), slot_of=(B,), counts=(4,), ce=(N,), w=(N,), loss=(1,), ws=(4 * N,), x_img=(B, F), x_tab=(B, W), bank_img=(N, F),
                  bank_tab=(N, W), active=(3,), gate=(3,))
    ints = ("label", "age", "occ", "n", "owner", "yhat", "slot_of", "counts")
    dtypes = dict(lse=torch.float64, ws=torch.float64, accepted=torch.uint8, active=torch.uint8, gate=torch.uint8, **{k: torch.int32 for k in ints})
    ptr = {k: torch.full(s, 1, dtype=dtypes.get(k, torch.float32), device=dev) for k, s in shapes.items()}
    ptr["owner"].copy_(torch.tensor([0, 1, 2, 3]))
    ptr["n"].fill_(N)
    ptr["occ"].zero_()
    ptr["occ"][1] = N
    before = {k: v.clone() for k, v in ptr.items()}

    def q(null):
        return {k: (None if k in null else v.data_ptr()) for k, v in ptr.items()}

    def upd(ld=K, B_=B, K_=K, N_=N, lt=1.0, lu=1.0, ldp=K, null=()):
        a = q(null)
        return D.stil_rotta_bank_update(a["z"], ld, B_, K_, N_, c32(lt), c32(lu), a["label"], a["unc"], a["age"], a["occ"], a["n"], a["owner"],
                                        a["lse"], a["p"], ldp, a["H"], a["yhat"], a["accepted"], a["slot_of"], a["counts"], None)

    refused = [upd(null=(k,)) for k in ("z", "label", "unc", "age", "occ", "n", "owner", "lse", "p", "H", "yhat", "accepted", "slot_of", "counts")]
    refused += [upd(B_=0), upd(B_=-1), upd(K_=0), upd(K_=-2), upd(N_=0), upd(N_=-4), upd(ld=K - 1), upd(ldp=K - 1), upd(N_=4097), upd(K_=65537, ld=65537, ldp=65537)]
    refused += [upd(lt=v) for v in (-1.0, -1e-9, inf, nan)] + [upd(lu=v) for v in (-1.0, -1e-9, inf, nan)]
    assert all(rc < 0 for rc in refused), refused
    assert b"stil_rotta_bank_update" in D.stil_last_error()

    def store(N_=N, B_=B, F_=F, W_=W, null=()):
        a = q(null)
        return D.stil_rotta_bank_store(a["x_img"], a["x_tab"], a["owner"], N_, B_, lng(F_), W_, a["bank_img"], a["bank_tab"], None)

    refused = [store(null=(k,)) for k in ("x_img", "x_tab", "owner", "bank_img", "bank_tab")]
    refused += [store(N_=0), store(N_=-1), store(N_=4097), store(B_=0), store(B_=-3), store(F_=0), store(F_=-48), store(W_=0), store(W_=-5)]
    assert all(rc < 0 for rc in refused), refused
    assert b"stil_rotta_bank_store" in D.stil_last_error()

    def rows(lds=K, ldt=K, R=N, K_=K, gs=1.0, ldd=K, nt=3, null=()):
        a = q(null)
        return D.stil_rotta_rows(a["zt"], lds, a["z"], ldt, a["label"], a["age"], R, K_, c32(gs), a["ce"], a["w"], a["dz"], ldd, a["counts"],
                                 a["loss"], a["active"], a["gate"], nt, a["ws"], None)

    refused = [rows(null=(k,)) for k in ("zt", "z", "label", "age", "ce", "w", "dz", "counts", "loss", "ws", "active", "gate")]
    refused += [rows(R=0), rows(R=-1), rows(K_=0), rows(K_=-1), rows(lds=K - 1), rows(ldt=K - 1), rows(ldd=K - 1), rows(nt=-1)]
    refused += [rows(gs=v) for v in (inf, -inf, nan)]
    assert all(rc < 0 for rc in refused), refused
    assert b"stil_rotta_rows" in D.stil_last_error()
    # the teacher's two entry points
    n, params, teacher, c2t, act, ach = _slab()
    P, Tt = params.cuda(), teacher.cuda()
    tail = (ach.data_ptr(), len(E.ACHUNKS), c2t.data_ptr(), act.data_ptr(), len(E.ACTIVE))

    def ex(p=P.data_ptr(), t=Tt.data_ptr(), tail_=tail, n_=n):
        return D.stil_rotta_exchange(p, t, *tail_, lng(n_), None)

    def te(p=P.data_ptr(), t=Tt.data_ptr(), tail_=tail, n_=n, nu=0.3):
        return D.stil_rotta_teacher(p, t, *tail_, lng(n_), c32(nu), None)

    for fn, name in ((ex, b"stil_rotta_exchange"), (te, b"stil_rotta_teacher")):
        refused = [fn(p=None), fn(t=None), fn(tail_=(None,) + tail[1:]), fn(tail_=tail[:2] + (None,) + tail[3:]), fn(tail_=tail[:3] + (None, tail[4]))]
        refused += [fn(n_=n + 5), fn(n_=-1024), fn(tail_=(tail[0], -1) + tail[2:]), fn(tail_=tail[:4] + (-1,)), fn(p=P.data_ptr() + 4), fn(t=Tt.data_ptr() + 4)]
        if fn is te:
            refused += [te(nu=v) for v in (-0.01, 1.01, inf, -inf, nan)]
        assert all(rc < 0 for rc in refused), (name, refused)
        assert name in D.stil_last_error()
    torch.cuda.synchronize()
    for k, v in ptr.items():
        assert torch.equal(v, before[k]), f"a refused call wrote {k}"
    assert torch.equal(P.cpu(), params) and torch.equal(Tt.cpu(), teacher), "a refused call wrote the slab"
    # and the calls they are variations of are accepted
    assert upd() == 0 and upd(lt=0.0, lu=0.0) == 0 and store() == 0 and rows() == 0 and rows(nt=0, null=("active", "gate")) == 0 and rows(gs=0.0) == 0
    assert ex() == 0 and ex() == 0 and te() == 0 and te(nu=0.0) == 0 and te(nu=1.0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ check 6: the step, restated
STEP_LR, STEP_NU, STEP_ALPHA, STEP_N = 1e-3, 0.3, 0.05, 8


def _step_hp(B):
    return O.default_hparams(batch_size=B, model="resnet18", embedding_dim=512, img_size=64, num_classes=5)


def _teacher_of(m):
    """{state_dict name of a member of A: the teacher's value} (CPU copies)"""
    return {k: v.cpu().clone() for k, v in zip(m.tta_param_names(), m._tent._compact_views(m._tent.teacher))}


def _bank_of(st, N, K):
    if st is None or st.bank_img is None:
        return C.start_bank(N, K, "empty", 0), None, None
    return ({k: getattr(st, k).cpu().numpy().copy() for k in BANK_KEYS}, st.bank_img.cpu().clone(), st.bank_tab.cpu().clone())


def _oracle_out_m(sd, keys, x_img, x_tab, hp, dtype, mem, rho, alpha, record=None, decisions=None, grad=False):
    """out_m of the oracle on a copy of `sd` in `dtype`, its BatchNorm the memory's at share rho -> (out_m, state, flips)"""
    s = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    if grad:
        for k in keys:
            s[k].requires_grad_(True)
    ctx = O.force_decisions(*decisions) if decisions is not None else contextlib.nullcontext()
    with BM.memory_oracle(mem, rho, alpha, record=record), ctx as d:
        out = O.backbone_forward_all(s, "model.", x_img.to(dtype), x_tab.to(dtype), hp, train=True, masks=None)[0]
    flips = {t: v for t, v in d.get("flips", {}).items() if v[0]} if d is not None else {}
    return out, s, flips


def _student(sd, keys, views, tab, hp, dtype, mem, zt_bank, label, age, decisions=None):
    out, s, flips = _oracle_out_m(sd, keys, views, tab, hp, dtype, mem, 0.0, 0.0, decisions=decisions, grad=True)
    r = C.rotta_forward(out, zt_bank.to(dtype), label, age)
    g = torch.autograd.grad(r["loss"], [s[k] for k in keys]) if r["n"] > 0 else [torch.zeros_like(s[k]) for k in keys]
    return dict(loss=r["loss"].detach(), w=r["w"], g=dict(zip(keys, [t.detach() for t in g])), flips=flips)


def test_rotta_step_matches_rotta_restated_in_float64():
    """Two consecutive batches of 16 on a ResNet-18 at 64 px, K = 5, a bank of 8: the second adapts on a bank the first filled, and
    its teacher has moved (nu = 0.3, so that a teacher that failed to move shows).  Bars are TENT's (tests/test_gpu_tta.py): the
    teacher's scores <= 3e-5 scaled, every gradient of A <= 3 e32 + 1e-4 -- the backward at rho = 0 on the memory -- A after Adam
    within 2.2 lr step of the fp32 restatement, everything outside A bit-identical; the bank's bookkeeping is the float64 walk's
    exactly, the bank's samples are the batch's bit for bit, the memory and the teacher at close()."""
    import test_gpu_step as S
    from stil_tta_amd import tta
    B, N = 16, STEP_N
    hp = _step_hp(B)
    K = hp.num_classes
    sd = G.parity_state(hp, 41, G.HEAD_SCALE)
    m = T.make_model(hp, sd, tta=True, tta_method="rotta", tta_lr=STEP_LR, tta_bn_momentum=STEP_ALPHA, tta_rotta_capacity=N, tta_rotta_nu=STEP_NU)
    m.freeze()
    keys = T.adapted_keys(m)
    assert len(keys) == 40
    opt, bad = {}, []
    for step, seed in enumerate((701, 702), start=1):
        x, y = T.tta_batch(hp, B, seed)
        before = T.full_state(m)
        sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
        mem_before = BM.memory_of(m, sd_before)
        teacher_before = _teacher_of(m) if m._tent is not None else {k: sd_before[k].clone() for k in keys}
        bank_before, img_before, tab_before = _bank_of(m._tent, N, K)
        with S._trace_decisions() as trace:
            scores = m.test_step(T.to_dev((x, y)), step - 1)
            torch.cuda.synchronize()
            decisions = S._device_decisions(m, trace)
        lt, st = m.last_tta, m._tent
        assert m._bn_mem.t == step
        # (2) the teacher on the clean batch, the one forward that writes the memory
        sd_teacher = dict(sd_before, **teacher_before)
        rec = {}
        zt64, _, _ = _oracle_out_m(sd_teacher, keys, x[0], x[1], hp, torch.float64, mem_before, STEP_ALPHA, STEP_ALPHA, record=rec)
        zt64 = zt64.detach()
        p64 = torch.softmax(zt64, dim=1)
        d = S._scaled(lt["probs"].cpu().double().numpy(), p64.numpy())
        print(f"[rotta] batch {step}: teacher scores scaled error {d:.2e}")
        if d > 3e-5:
            bad.append((step, "predictions", d))
        close(lt["probs_bank"], torch.softmax(lt["y_hat_m"].double(), dim=1), name="probs_bank against softmax(y_hat_m)")
        assert torch.equal(scores, m._task_scores(lt["probs"]))
        BM._check_memory(m, rec, f"[rotta] batch {step}")
        # (3) the bank: the float64 walk on the float64 teacher's entropies
        top2 = zt64.topk(2, dim=1).values
        assert float((top2[:, 0] - top2[:, 1]).min()) >= 1e-3, "a pseudo-label hangs on a tie: choose another seed"
        H64 = -(p64 * torch.log_softmax(zt64, dim=1)).sum(dim=1)
        walk = C.bank_walk(H64.numpy(), zt64.argmax(dim=1).numpy(), N, K, bank_before, f32(m.hp.tta_rotta_lambda_t), f32(m.hp.tta_rotta_lambda_u))
        print(f"[rotta] batch {step}: smallest margin of the bank's decisions {walk['margin']:.3e}; accepted {walk['counts'].tolist()}")
        assert walk["margin"] >= C.MIN_MARGIN, f"batch {step}: the oracle's margin {walk['margin']:.2e} makes the bank ill-posed: choose another seed"
        for k, got in (("label", st.label), ("age", st.age), ("occ", st.occ), ("n", st.n), ("owner", st.owner), ("accepted", lt["accepted"]),
                       ("slot_of", lt["slot_of"])):
            if not np.array_equal(got.cpu().numpy(), walk[k]):
                bad.append((step, "bank " + k, got.cpu().tolist(), walk[k].tolist()))
        assert int(lt["n_bank"]) == int(walk["n"][0]) and torch.equal(lt["bank_label"], st.label) and torch.equal(lt["bank_age"], st.age)
        close(st.unc, torch.from_numpy(walk["unc"]), name="unc")
        img = torch.zeros((N,) + tuple(x[0].shape[1:])) if img_before is None else img_before
        tab = torch.zeros((N,) + tuple(x[1].shape[1:])) if tab_before is None else tab_before
        for s_, o in enumerate(walk["owner"]):
            if o >= 0:
                img[s_], tab[s_] = x[0][o], x[1][o]
        assert torch.equal(st.bank_img.cpu(), img) and torch.equal(st.bank_tab.cpu(), tab), "the bank's samples are not the batch's"
        # (4) the teacher on the bank, on the committed memory alone
        ztb64 = _oracle_out_m(sd_teacher, keys, img, tab, hp, torch.float64, rec, 0.0, 0.0)[0].detach()
        # (5) the student on the device's own views of the bank
        views, vtab, _ = tta.make_views(m, (st.bank_img, st.bank_tab), draws=lt["draws"])
        views, vtab = views.cpu(), vtab.cpu()
        assert torch.equal(vtab, tab) and not torch.equal(views, img)
        label, age = torch.from_numpy(walk["label"]), torch.from_numpy(walk["age"])
        r64 = _student(sd_before, keys, views, vtab, hp, torch.float64, rec, ztb64, label, age, decisions)
        r64free = _student(sd_before, keys, views, vtab, hp, torch.float64, rec, ztb64, label, age)
        r32 = _student(sd_before, keys, views, vtab, hp, torch.float32, rec, ztb64, label, age)
        S._check_flips(r64["flips"])
        close(lt["loss"].view(1), r64["loss"].view(1), name="loss")
        close(lt["weight"], r64["w"], name="weight")
        gd = T.device_grads(m)
        ratios = []
        for k in keys:
            e32, err = T._rel(r32["g"][k].double(), r64free["g"][k]), T._rel(gd[k], r64["g"][k])
            ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
            if err > 3 * e32 + 1e-4:
                bad.append((step, "grad " + k, err, e32))
        print(f"[rotta] batch {step}: gradient error / (3*e32 + 1e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
        # (6) Adam over A (fp32 oracle, its own moments), (7) the teacher's average of the device's A
        sd32 = {k: v.clone() for k, v in sd_before.items()}
        O.adam_step(sd32, r32["g"], opt, step, STEP_LR)
        after, aset = T.full_state(m), set(keys)
        for k, v in after.items():
            if k in aset:
                dev = float((v.cpu() - sd32[k]).abs().max())
                if dev > 2.2 * STEP_LR * step:
                    bad.append((step, "adam " + k, dev))
            elif not torch.equal(v, before[k]):
                bad.append((step, "changed " + k))
        assert any(not torch.equal(after[k], before[k]) for k in keys), "the step adapted nothing"
        teacher_after = _teacher_of(m)
        for k in keys:
            want = C.teacher_ref(teacher_before[k], after[k].cpu(), STEP_NU)
            if not torch.equal(teacher_after[k], want):
                bad.append((step, "teacher " + k, float((teacher_after[k] - want).abs().max())))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


# ------------------------------------------------------------------------------------------ check 7: properties
def _small(which="bn", method="rotta", **tta):
    hp = T.dvm_hp(16, img_size=64)
    sd = T.initial_state(hp, 5)
    tta.setdefault("tta_bn_momentum", 0.05)
    tta.setdefault("tta_rotta_capacity", 8)
    return hp, sd, (lambda: T.make_model(hp, sd, tta=True, tta_method=method, tta_params=which, **tta))


def _A(m):
    return {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}


def _bank_state(st):
    return {k: getattr(st, k).clone() for k in BANK_KEYS + ("owner", "bank_img", "bank_tab", "teacher")}


def test_frozen_teacher_and_student_report_bn_adapts_scores_bit_for_bit():
    """tta_rotta_nu 0 with tta_lr 0: the teacher stays at the source, so batch after batch the reported scores are those of bn_adapt
    under the same tta_bn_momentum, bit for bit -- the bank fills beside them and changes nothing that is reported."""
    hp, sd, mk = _small(tta_rotta_nu=0, tta_lr=0.0)
    _, _, mkb = _small(method="bn_adapt")
    r, b = mk(), mkb()
    A0 = _A(r)
    for i, seed in enumerate((11, 12, 13)):
        batch = T.to_dev(T.tta_batch(hp, 16, seed))
        pr, pb = r.test_step(batch, i), b.test_step(batch, i)
        assert torch.equal(r.last_tta["y_hat_m"], b.last_tta["y_hat_m"]), f"batch {i}: the logits differ"
        assert torch.equal(pr, pb) and torch.equal(r.last_tta["probs"], b.last_tta["probs"]), f"batch {i}: the scores differ"
        for (m1, v1), (m2, v2) in zip(r._bn_mem.state(), b._bn_mem.state()):
            assert torch.equal(m1, m2) and torch.equal(v1, v2)
    assert int(r.last_tta["n_bank"]) >= 1 and r._bn_mem.t == 3
    for k, v in A0.items():
        assert torch.equal(r.state_dict()[k], v), k
    assert torch.equal(r._tent.teacher, r._tent.theta0)


def test_the_bank_carries_over_and_reset_and_episodes_empty_it():
    hp, sd, mk = _small()
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, 11)), T.to_dev(T.tta_batch(hp, 16, 12))
    o = mk()
    A0 = _A(o)
    src_mem = [(a.clone(), b.clone()) for a, b in tta_memory(o)]
    o.test_step(b1, 0)
    n1, lab1 = int(o.last_tta["n_bank"]), o._tent.label.clone()
    assert n1 >= 1 and int((lab1 >= 0).sum()) == n1 and bool((o._tent.age[:n1] >= 1).all())
    assert bool((o._tent.bank_img[:n1] != 0).any()) and bool((o._tent.bank_img[n1:] == 0).all())
    r2 = o.test_step(b2, 1).clone()
    assert int(o._tent.steps.max()) == 2 and not torch.equal(o._tent.teacher, o._tent.theta0), "the teacher never moved"
    o.reset_tta()
    st = o._tent
    for k, v in A0.items():
        assert torch.equal(o.state_dict()[k], v), k
    assert bool((st.label == -1).all()) and int(st.n) == 0 and not bool(st.occ.any()) and not bool(st.age.any())
    assert not bool(st.bank_img.any()) and not bool(st.bank_tab.any()) and torch.equal(st.teacher, st.theta0) and int(st.steps.max()) == 0
    for (a, b), (sa, sb) in zip(o._bn_mem.state(), src_mem):
        assert torch.equal(a, sa) and torch.equal(b, sb)
    # episodic: every batch starts from the source, an empty bank, the source teacher and the checkpoint's statistics
    _, _, mke = _small(tta_episodic=True)
    e, f = mke(), mk()
    e.test_step(b1, 0)
    p2, q2 = e.test_step(b2, 1).clone(), f.test_step(b2, 0).clone()
    assert torch.equal(p2, q2) and not torch.equal(p2, r2), "episodic batch 2 is not a first batch, or nothing carries over online"
    for k in BANK_KEYS + ("bank_tab",):
        assert torch.equal(getattr(e._tent, k), getattr(f._tent, k)), k
    assert int(e.last_tta["n_bank"]) <= 16 and e._bn_mem.t == 1


def tta_memory(m):
    from stil_tta_amd import tta
    with torch.inference_mode(False):
        m.setup_device()
        return tta._memory(m).state()


def test_nothing_outside_a_the_teacher_and_the_bank_is_written():
    hp, sd, mk = _small("norm")
    m = mk()
    before = T.full_state(m)
    keys = set(T.adapted_keys(m))
    for i, seed in enumerate((11, 12)):
        m.test_step(T.to_dev(T.tta_batch(hp, 16, seed)), i)
    torch.cuda.synchronize()
    after = T.full_state(m)
    for k, v in after.items():
        if k not in keys:
            assert torch.equal(v, before[k]), f"{k} changed"      # training slabs, BatchNorm buffers, prototypes, the checkpoint's teacher
    assert any(not torch.equal(after[k], before[k]) for k in keys), "the RoTTA step adapted nothing"
    lt = m.last_tta
    for k in ("loss", "y_hat_m", "probs", "probs_bank", "accepted", "slot_of", "n_bank", "bank_label", "bank_age", "weight"):
        assert lt[k].is_cuda, k
    assert lt["probs"].shape == (16, hp.num_classes) and lt["weight"].shape == (8,) and lt["bank_label"].shape == (8,) and isinstance(lt["draws"], dict)


def test_freeze_inference_mode_and_load_state_dict():
    hp, sd, mk = _small()
    b = T.to_dev(T.tta_batch(hp, 16, 14))
    a, c = mk(), mk()
    a.freeze()
    c.freeze()
    with torch.inference_mode():
        pa = a.test_step(b, 0)
    pc = c.test_step(b, 0)
    assert torch.equal(pa, pc)
    sa, sc = T.full_state(a), T.full_state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    ba, bc = _bank_state(a._tent), _bank_state(c._tent)
    for k in ba:
        assert torch.equal(ba[k], bc[k]), k
    assert any(not torch.equal(sa[k], v) for k, v in T.full_state(mk()).items() if k in set(T.adapted_keys(a)))
    assert not any(q.requires_grad for q in a.parameters())
    a.load_state_dict({k: v.cuda() for k, v in T.initial_state(hp, 77).items()})
    assert a._tent is None and a._bn_mem is None, "load_state_dict kept the adaptation state"
    a.test_step(b, 0)
    assert a._tent.bank_img is not None and a._bn_mem.t == 1


def test_fit_test_and_a_ragged_last_batch(tmp_path):
    from stil_tta_amd import fit
    hp, sd, mk = _small()
    loader = [T.tta_batch(hp, 16, 20), T.tta_batch(hp, 16, 21), T.tta_batch(hp, 5, 22)]
    ck = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": {k: v.clone() for k, v in sd.items()}}, ck)
    a = mk()
    ra = fit.test(a, loader, ck)
    h = mk()
    h.freeze()
    h.acc_test.reset()
    h.auc_test.reset()
    for i, bt in enumerate(loader):
        h.test_step(T.to_dev(bt), i)
    rh = {k: float(v) for k, v in h.test_epoch_end().items()}
    assert ra.keys() == rh.keys() and all(ra[k] == rh[k] or (ra[k] != ra[k] and rh[k] != rh[k]) for k in ra), (ra, rh)
    ba, bh = _bank_state(a._tent), _bank_state(h._tent)
    for k in ba:
        assert torch.equal(ba[k], bh[k]), k
    assert a.last_tta["probs"].shape == (5, hp.num_classes) and a.last_tta["accepted"].shape == (5,) and int(a._tent.steps.max()) == 3
