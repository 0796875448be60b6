"""LAME test-time adaptation (Boudiaf, Mueller, Ben Ayed, Bertinetto, CVPR 2022, "Parameter-free Online Test-time Adaptation";
definition as recalled: unpinned) in STiLModel.test_step, beside bn_adapt (tests/test_gpu_bnprior.py, tests/test_gpu_bnmemory.py).

1. stil_lame_affinity against the float64 restatement of tests/lame_cases.py on every case: nbr exactly, wts and dk under close() at
   TOL, ldf = D and D + 3 (the padding holds NaN: it must not be read), sentinels, repetition.
2. stil_lame_rows against the restatement: steps exactly, Y and energy[:steps] under close() at TOL, energy[steps:] untouched, p and
   lse stil_entropy_rows' bits, ld = K and K + 3, sentinels, repetition; lambda 0, K 1, tol 0.
3. Both entries refuse every bad argument with nothing written.
4. The step on the small model of tests/test_gpu_tta.py.
5. The property on the device: the class-ordered batch of tests/test_lame_cpu.py.
tests/test_lame_cpu.py checks on the CPU that the inputs of checks 1, 2 and 5 are well-conditioned."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import lame_cases as C  # noqa: E402
from lame_cases import f32  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402
import test_gpu_shot as G  # noqa: E402
import test_gpu_tta as T  # noqa: E402

SENTINEL = -7.25
ISENT = -77
NAN = float("nan")


def _ids(c):
    return "-".join(map(str, c))


# ------------------------------------------------------------------------------------------ check 1: the affinity
def _run_affinity(L, F, rows, D, pad, k, kind):
    """one call on the rows [0, rows) of the features (stride D + pad, the padding and the row past the end hold NaN) -> the outputs on
    the CPU, sentinels included"""
    ldf = D + pad
    Fb = torch.full((rows + 1, ldf), NAN, dtype=torch.float32)
    Fb[:rows, :D] = F
    Fb = Fb.cuda()
    n_ws = rows * (1 + min(k, rows))
    o = dict(nbr=torch.full((rows + 1, k), ISENT, dtype=torch.int32, device="cuda"), wts=torch.full((rows + 1, k), SENTINEL, device="cuda"),
             dk=torch.full((rows + 1,), SENTINEL, dtype=torch.float64, device="cuda"),
             ws=torch.full((n_ws + 1,), SENTINEL, dtype=torch.float64, device="cuda"))
    L.lame_affinity(Fb.data_ptr(), ldf, rows, D, k, C.KINDS.index(kind), o["nbr"].data_ptr(), o["wts"].data_ptr(), o["dk"].data_ptr(),
                    o["ws"].data_ptr(), None)
    torch.cuda.synchronize()
    return {k_: v.cpu() for k_, v in o.items()}


@pytest.mark.parametrize("case", C.affinity_cases(), ids=_ids)
def test_affinity_against_the_restatement(case):
    from stil_tta_amd._lib import lib
    L = lib()
    rows, D, fkind, k, kind = case
    F, ref = C.affinity_case(*case)
    kp = min(k, rows - 1)
    for pad in (0, 3):
        a, b = (_run_affinity(L, F, rows, D, pad, k, kind) for _ in range(2))
        for key in ("nbr", "wts", "dk"):
            assert torch.equal(a[key].view(torch.uint8), b[key].view(torch.uint8)), f"{key}: not bit-identical on repetition"
        # sentinels: the row past the end, the element past every vector; the padding of the lists holds -1 and 0
        assert bool((a["nbr"][rows] == ISENT).all()) and bool((a["wts"][rows] == SENTINEL).all())
        assert float(a["dk"][rows]) == SENTINEL and float(a["ws"][-1]) == SENTINEL
        nbr, wts, dk = a["nbr"][:rows], a["wts"][:rows], a["dk"][:rows]
        assert bool((nbr[:, kp:] == -1).all()) and bool((wts[:, kp:] == 0).all())
        # every index written is in range, no row lists itself or anyone twice: whatever the features hold
        assert bool((nbr[:, :kp] >= 0).all()) and bool((nbr[:, :kp] < rows).all())
        assert all(len(set(r[:kp].tolist())) == kp and i not in r[:kp].tolist() for i, r in enumerate(nbr))
        if fkind == "nan":   # only the lists of the rows whose own features are finite are asserted
            finite = torch.isfinite(F).all(dim=1)
            assert int(finite.sum()) == rows - 1
            assert torch.equal(nbr[finite], ref["nbr"][finite]), "the neighbours of a finite row"
            continue
        assert torch.equal(nbr, ref["nbr"]), f"neighbours differ in rows {(nbr != ref['nbr']).any(dim=1).nonzero().flatten().tolist()[:8]}"
        close(wts, ref["wts"], name="wts")
        close(dk, ref["dk"], name="dk")
        if kind == "knn":
            assert bool((wts[:, :kp] == 1).all())


# ------------------------------------------------------------------------------------------ check 2: the correction
def _run_rows(L, Z, rows, K, pad, nbr, wts, lam, max_steps, tol):
    """one call on the rows [0, rows) of the logits (stride K + pad) under the restatement's own neighbours and float32 weights -> the
    outputs on the CPU, sentinels included"""
    ld = K + pad
    k = nbr.shape[1]
    zb = G._padded(Z, rows, K, pad)
    full = lambda shape, dtype=torch.float32: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")  # noqa: E731
    n_ws = 2 * rows * rows + 3 * rows * K + 3 * rows + 2
    o = dict(lse=full((rows + 1,), torch.float64), p=full((rows + 1, ld)), Y=full((rows + 1, ld)), energy=full((max_steps + 1,), torch.float64),
             steps=torch.full((2,), ISENT, dtype=torch.int32, device="cuda"), ws=full((n_ws + 1,), torch.float64))
    nb, wt = nbr.int().contiguous().cuda(), wts.float().contiguous().cuda()
    L.lame_rows(zb.data_ptr(), ld, rows, K, nb.data_ptr(), wt.data_ptr(), k, f32(lam), max_steps, f32(tol), o["lse"].data_ptr(), o["p"].data_ptr(),
                ld, o["Y"].data_ptr(), ld, o["energy"].data_ptr(), o["steps"].data_ptr(), o["ws"].data_ptr(), None)
    torch.cuda.synchronize()
    out = {k_: v.cpu() for k_, v in o.items()}
    out["entropy"] = G._run_entropy(L, zb, ld, rows, K, 1.0)
    return out


@pytest.mark.parametrize("case", C.rows_cases(), ids=_ids)
def test_rows_against_the_restatement(case):
    from stil_tta_amd._lib import lib
    L = lib()
    rows, K, D, fkind, k, kind, lam, tol, max_steps = case
    Z, F, ref = C.rows_case(*case)
    for pad in (0, 3):
        a, b = (_run_rows(L, Z, rows, K, pad, ref["nbr"], ref["wts"], lam, max_steps, tol) for _ in range(2))
        for key in ("lse", "p", "Y", "energy", "steps"):
            assert torch.equal(a[key].view(torch.uint8), b[key].view(torch.uint8)), f"{key}: not bit-identical on repetition"
        # sentinels: padding columns, the row past the end, the element past every vector
        assert bool((a["p"][rows] == SENTINEL).all()) and bool((a["Y"][rows] == SENTINEL).all()) and float(a["lse"][rows]) == SENTINEL
        assert pad == 0 or (bool((a["p"][:, K:] == SENTINEL).all()) and bool((a["Y"][:, K:] == SENTINEL).all()))
        assert int(a["steps"][1]) == ISENT and float(a["ws"][-1]) == SENTINEL
        # p and lse are stil_entropy_rows' bits
        assert torch.equal(a["lse"][:rows], a["entropy"]["lse"]) and torch.equal(a["p"][:rows, :K], a["entropy"]["p"])
        steps = int(a["steps"][0])
        print(f"steps {steps} (restatement {ref['steps']})")
        assert steps == ref["steps"], (steps, ref["steps"])
        assert bool((a["energy"][steps:] == SENTINEL).all()), "energy was written from `steps` on"
        if tol == 0:
            assert steps == max_steps
        Y = a["Y"][:rows, :K]
        if not bool(torch.isfinite(ref["Y"]).all()):   # the nan kind under rbf weights: termination is all that is asserted
            assert fkind == "nan" and steps == max_steps
            continue
        close(Y, ref["Y"], name="Y")
        close(a["energy"][:steps], ref["energy"], name="energy")
        close(a["p"][:rows, :K], ref["p"], name="p")
        close(a["lse"][:rows], ref["lse"], name="lse")
        if lam == 0:
            close(Y, ref["p"], name="Y at lambda 0 against p")
        if K == 1:
            assert bool((Y == 1).all())


# ------------------------------------------------------------------------------------------ check 3: refusals
def test_entry_points_reject_bad_arguments_with_nothing_written():
    from stil_tta_amd._lib import lib
    L = lib()
    D_ = L._dll
    c32, nan, inf = ctypes.c_float, float("nan"), float("inf")
    R, K, D, k, S = 6, 5, 8, 3, 4
    shapes = dict(F=(R, D), nbr=(R, k), wts=(R, k), dk=(R,), ws=(2 * R * R + 3 * R * K + 3 * R + 2,), Z=(R, K), lse=(R,), p=(R, K), Y=(R, K), energy=(S,),
                  steps=(1,))
    dtypes = dict(nbr=torch.int32, steps=torch.int32, dk=torch.float64, ws=torch.float64, lse=torch.float64, energy=torch.float64)
    ptr = {n: torch.full(s, 1, dtype=dtypes.get(n, torch.float32), device="cuda") for n, s in shapes.items()}
    before = {n: v.clone() for n, v in ptr.items()}

    def q(null):
        return {n: (None if n in null else v.data_ptr()) for n, v in ptr.items()}

    def aff(ldf=D, R_=R, D_dim=D, k_=k, kind=0, null=()):
        a = q(null)
        return D_.stil_lame_affinity(a["F"], ldf, R_, D_dim, k_, kind, a["nbr"], a["wts"], a["dk"], a["ws"], None)

    refused = [aff(null=(n,)) for n in ("F", "nbr", "wts", "dk", "ws")]
    refused += [aff(R_=0), aff(R_=-1), aff(D_dim=0), aff(D_dim=-8), aff(k_=0), aff(k_=-1), aff(R_=2049), aff(ldf=D - 1), aff(kind=2), aff(kind=-1)]
    assert all(rc < 0 for rc in refused), refused
    assert b"stil_lame_affinity" in D_.stil_last_error()

    def rows(ld=K, R_=R, K_=K, k_=k, lam=1.0, steps=S, tol=1e-8, ldp=K, ldy=K, null=()):
        a = q(null)
        return D_.stil_lame_rows(a["Z"], ld, R_, K_, a["nbr"], a["wts"], k_, c32(lam), steps, c32(tol), a["lse"], a["p"], ldp, a["Y"], ldy,
                                 a["energy"], a["steps"], a["ws"], None)

    refused = [rows(null=(n,)) for n in ("Z", "nbr", "wts", "lse", "p", "Y", "energy", "steps", "ws")]
    refused += [rows(R_=0), rows(R_=-1), rows(K_=0), rows(K_=-5), rows(k_=0), rows(k_=-3), rows(R_=2049), rows(ld=K - 1), rows(ldp=K - 1), rows(ldy=K - 1)]
    refused += [rows(lam=v) for v in (-1.0, -1e-9, inf, -inf, nan)] + [rows(tol=v) for v in (-1e-8, -1.0, inf, -inf, nan)]
    refused += [rows(steps=0), rows(steps=-1)]
    assert all(rc < 0 for rc in refused), refused
    assert b"stil_lame_rows" in D_.stil_last_error()
    torch.cuda.synchronize()
    for n, v in ptr.items():
        assert torch.equal(v, before[n]), f"a refused call wrote {n}"
    # and the calls they are variations of are accepted
    assert aff() == 0 and aff(kind=1) == 0 and aff(k_=1) == 0 and rows() == 0 and rows(lam=0.0, tol=0.0, steps=1) == 0
    torch.cuda.synchronize()
    from stil_tta_amd import tta
    with pytest.raises(ValueError, match=str(tta.LAME_MAX_ROWS)):
        tta.lame_correct(torch.zeros(tta.LAME_MAX_ROWS + 1, 3, device="cuda"), torch.zeros(tta.LAME_MAX_ROWS + 1, 4, device="cuda"))
    for bad in (dict(kind="linear"), dict(k=0), dict(k=2.0), dict(max_steps=0), dict(k=True)):
        with pytest.raises(ValueError):
            tta.lame_correct(torch.zeros(4, 3, device="cuda"), torch.zeros(4, 4, device="cuda"), **bad)
    with pytest.raises(RuntimeError, match="lambda"):
        tta.lame_correct(torch.zeros(4, 3, device="cuda"), torch.zeros(4, 4, device="cuda"), lam=-1.0)


# ------------------------------------------------------------------------------------------ check 4: the step
STEP_SEED = 7


def _small(method="lame", hp_fn=T.dvm_hp, **tta):
    hp = hp_fn(16, img_size=64)
    sd = T.initial_state(hp, 5)
    return hp, sd, (lambda: T.make_model(hp, sd, tta=True, tta_method=method, **tta))


def _restated(m, **over):
    """lame_ref64 on the device's own logits and features under the model's hparams"""
    hp = m.hp
    kw = dict(k=hp.tta_lame_knn, kind=hp.tta_lame_affinity, lam=hp.tta_lame_lambda, max_steps=hp.tta_lame_steps, tol=hp.tta_lame_tol)
    kw.update(over)
    z, f = m.last_tta["y_hat_m"].cpu(), m.last_tta["features"].cpu()
    C.check_gaps(f, "plain", kw["k"])   # the comparison below is only as good as the neighbour decisions are clear
    return C.lame_ref64(z, f, **kw)


@pytest.mark.parametrize("over", [dict(), dict(tta_lame_affinity="rbf", tta_lame_knn=3, tta_lame_lambda=2.5, tta_lame_tol=0.0, tta_lame_steps=7)],
                         ids=["defaults", "rbf-7-steps"])
def test_the_steps_scores_are_the_restatement_on_its_own_logits_and_features(over):
    hp, sd, mk = _small(**over)
    m = mk()
    batch = T.to_dev(T.tta_batch(hp, 16, STEP_SEED))
    out = m.test_step(batch, 0)
    torch.cuda.synchronize()
    lt = m.last_tta
    assert set(lt) == {"y_hat_m", "probs", "probs_raw", "features", "neighbours", "steps", "energy"} and all(v.is_cuda for v in lt.values())
    K, Dm = hp.num_classes, 3 * hp.multimodal_embedding_dim
    assert lt["features"].shape == (16, Dm) and lt["probs"].shape == (16, K) and lt["neighbours"].shape == (16, m.hp.tta_lame_knn)
    ref = _restated(m)
    steps = int(lt["steps"][0])
    print(f"steps {steps} (restatement {ref['steps']}); ratios {['%.3e' % r for r in ref['ratios'][-3:]]}")
    assert C.band_clear(ref["ratios"], m.hp.tta_lame_tol), "the stopping step of this batch is not decided with margin: pick another STEP_SEED"
    assert steps == ref["steps"] and torch.equal(lt["neighbours"].cpu(), ref["nbr"])
    close(lt["probs"], ref["Y"], name="probs")
    close(lt["energy"][:steps], ref["energy"], name="energy")
    assert bool(torch.isnan(lt["energy"][steps:]).all())
    assert torch.equal(out, lt["probs"]) and not torch.equal(lt["probs"], lt["probs_raw"])
    # the features are the multimodal classifier's own input: the logits follow from them
    with torch.no_grad():
        cl = m.model.classifier_multimodal
        z = lt["features"].double() @ cl.weight.double().T + cl.bias.double()
    close(lt["y_hat_m"], z, name="logits from the features")


def test_raw_scores_are_the_plain_steps_bit_for_bit():
    hp, sd, mk = _small()
    plain = T.make_model(hp, sd, tta=False)
    m = mk()
    for i, seed in enumerate((11, 12)):
        batch = T.to_dev(T.tta_batch(hp, 16, seed))
        pm, pp = m.test_step(batch, i), plain.test_step(batch, i)
        assert torch.equal(m.last_tta["probs_raw"], pp), f"batch {i}: probs_raw is not the plain test_step's scores"
        assert not torch.equal(pm, pp)
    assert m._bn_mem is None and m._tent is None


@pytest.mark.parametrize("knobs", [dict(tta_bn_prior=16), dict(tta_bn_momentum=0.05)], ids=["prior", "memory"])
def test_raw_scores_are_bn_adapts_bit_for_bit_under_the_batchnorm_knobs(knobs):
    """the paper's LAME on adapted statistics: the forward is bn_adapt_step's, batch after batch, the memory included"""
    hp, _, mkl = _small(**knobs)
    _, _, mkb = _small(method="bn_adapt", **knobs)
    a, b = mkl(), mkb()
    for i, seed in enumerate((11, 12, 13)):
        batch = T.to_dev(T.tta_batch(hp, 16, seed))
        a.test_step(batch, i)
        pb = b.test_step(batch, i)
        assert torch.equal(a.last_tta["y_hat_m"], b.last_tta["y_hat_m"]), (knobs, i)
        assert torch.equal(a.last_tta["probs_raw"], pb) and torch.equal(a.last_tta["probs_raw"], b.last_tta["probs"]), (knobs, i)
    if "tta_bn_momentum" in knobs:
        assert a._bn_mem.t == 3
        for (m1, v1), (m2, v2) in zip(a._bn_mem.state(), b._bn_mem.state()):
            assert torch.equal(m1, m2) and torch.equal(v1, v2)
        a.reset_tta()
        assert a._bn_mem.t == 0
    assert a._tent is None


def test_nothing_of_the_model_is_written():
    for knobs in (dict(), dict(tta_bn_momentum=0.05, tta_bn_prior=16, tta_episodic=True)):
        hp, sd, mk = _small(**knobs)
        m = mk()
        before = T.full_state(m)
        for i, seed in enumerate((11, 12, 13)):
            m.test_step(T.to_dev(T.tta_batch(hp, 16, seed)), i)
        torch.cuda.synchronize()
        after = T.full_state(m)
        assert before.keys() == after.keys()
        for key in before:
            assert torch.equal(before[key], after[key]), f"{knobs}: the step wrote {key}"
        assert m._tent is None


def test_freeze_inference_mode_metrics_binary_and_one_row():
    hp, sd, mk = _small()
    b = T.to_dev(T.tta_batch(hp, 16, 14))
    a, c = mk(), mk()
    a.freeze()
    with torch.inference_mode():
        pa = a.test_step(([b[0][0].clone(), b[0][1].clone()], b[1].clone()), 0)
    fed = []
    for name in ("acc_test", "auc_test"):
        metric = getattr(c, name)
        setattr(c, name, lambda p, y, _m=metric, _n=name: (fed.append((_n, p)), _m(p, y))[1])
    pc = c.test_step(b, 0)
    assert torch.equal(pa, pc)
    assert [n for n, _ in fed] == ["acc_test", "auc_test"] and all(torch.equal(p, c.last_tta["probs"]) for _, p in fed), "the metrics are fed Y"
    assert not torch.equal(c.last_tta["probs"], c.last_tta["probs_raw"])
    assert not any(q.requires_grad for q in a.parameters())
    # one row: no neighbour, the scores are softmax(log(p + 1e-10)) after two steps
    one = ([b[0][0][:1].contiguous(), b[0][1][:1].contiguous()], b[1][:1].contiguous())
    p1 = c.test_step(one, 1)
    assert p1.shape == (1, hp.num_classes) and int(c.last_tta["steps"][0]) == 2 and bool((c.last_tta["neighbours"] == -1).all())
    close(p1, c.last_tta["probs_raw"], name="one row")
    # the binary task reports column 1 of Y
    hp2, sd2, mk2 = _small(hp_fn=T.cardiac_hp)
    m2 = mk2()
    p2 = m2.test_step(T.to_dev(T.tta_batch(hp2, 16, 15)), 0)
    assert hp2.num_classes == 2 and p2.shape == (16,) and torch.equal(p2, m2.last_tta["probs"][:, 1])
    # a batch above the bound is refused before its forward, naming the bound
    from stil_tta_amd import tta
    big = ([torch.zeros(tta.LAME_MAX_ROWS + 1, 3, 8, 8, device="cuda"), torch.zeros(tta.LAME_MAX_ROWS + 1, b[0][1].shape[1], device="cuda")],
           torch.zeros(tta.LAME_MAX_ROWS + 1, dtype=torch.long, device="cuda"))
    with pytest.raises(ValueError, match=str(tta.LAME_MAX_ROWS)):
        c.test_step(big, 2)


def test_fit_test_and_test_shifts_take_the_lame_path(tmp_path):
    """fit.test and fit.test_shifts reach the step through STEPS alone: their metrics are those of the batches run by hand"""
    from stil_tta_amd import fit
    from stil_tta_amd.shift import ShiftSpec
    hp, sd, mk = _small()
    loader = [T.tta_batch(hp, 16, 20 + i) for i in range(2)]
    ck = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": {k: v.clone() for k, v in sd.items()}}, ck)
    a = mk()
    ra = fit.test(a, loader, ck)
    assert set(a.last_tta) >= {"probs", "probs_raw", "neighbours", "steps", "energy"}
    h = mk()
    h.freeze()
    for i, bt in enumerate(loader):
        h.test_step(T.to_dev(bt), i)
    rh = {k: float(v) for k, v in h.test_epoch_end().items()}
    assert ra.keys() == rh.keys() and all(ra[k] == rh[k] or (ra[k] != ra[k] and rh[k] != rh[k]) for k in ra), (ra, rh)
    off = T.make_model(hp, sd, tta=False)
    ro = fit.test(off, loader, ck)
    assert ro.keys() == ra.keys()
    table = fit.test_shifts(a, loader, {"clean": ShiftSpec(), "noise": ShiftSpec(image=("gaussian_noise", 3))}, ck, protocol="reset")
    assert set(table) == {"clean", "noise", "mean"} and all(table["clean"][k] == ra[k] or ra[k] != ra[k] for k in ra)


# ------------------------------------------------------------------------------------------ check 5: the property, on the device
def test_the_property_on_the_device():
    from stil_tta_amd import tta
    c = C.PROPERTY
    Z, F, y, ref = C.property_ref()
    Y, p, info = tta.lame_correct(Z.cuda(), F.cuda(), c["k"], c["kind"], c["lam"], c["max_steps"], c["tol"])
    torch.cuda.synchronize()
    Y = Y.cpu()
    top = ref["Y"].topk(2, dim=1).values
    decided = (top[:, 0] - top[:, 1]) > C.MARGIN
    assert int((~decided).sum()) <= C.MAX_EXCLUDED
    assert torch.equal(Y.argmax(1)[decided], ref["Y"].argmax(1)[decided])
    assert int(info["steps"][0]) == ref["steps"] and torch.equal(info["nbr"].cpu(), ref["nbr"])
    close(Y, ref["Y"], name="Y")
    raw, acc = float((p.cpu().argmax(1) == y).float().mean()), float((Y.argmax(1) == y).float().mean())
    print(f"raw accuracy {raw:.3f}, corrected {acc:.3f}, steps {int(info['steps'][0])}")
    assert acc - raw >= 0.3
