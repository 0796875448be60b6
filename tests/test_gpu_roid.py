"""ROID test-time adaptation (Marsden, Doebler, Yang, WACV 2024, "Universal Test-time Adaptation through Weight Ensembling,
Diversity Weighting, and Prior Correction"; definition as recalled: unpinned) in STiLModel.test_step, on top of TENT
(tests/test_gpu_tta.py).

1. stil_roid_rows against float64 autograd on every case of tests/roid_cases.py: ld = K and K + 3, sentinels, repetition; keep and
   counts exactly, everything else under close() at TOL; lse, p, H are stil_entropy_rows' bits; the degenerate rule; K = 1.
2. stil_roid_ensemble against float64: inactive, padding and out-of-range chunks untouched; momentum 1 and 0.
3. Both entry points refuse bad arguments with nothing written.
4. The step against ROID restated here in float64 on the oracle, on the device's ReLU / max-pool decisions.
5. The properties of the step.
tests/test_roid_cpu.py checks on the CPU that the inputs of check 1 are well-conditioned (no selection hangs on a margin below 5e-5
and fp32 ATen meets the same bars)."""
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

import roid_cases as C  # noqa: E402
from roid_cases import f32  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
import test_gpu_eata as E  # noqa: E402
import test_gpu_shot as G  # noqa: E402
import test_gpu_tta as T  # noqa: E402

SENTINEL = -7.25
ROW_FLOATS = ("H", "cos", "slr", "dn", "cn", "w")


# ------------------------------------------------------------------------------------------ check 1: the row loss
def _padded(z, rows, K, pad):
    zb = torch.full((rows + 1, K + pad), SENTINEL, dtype=torch.float32)
    zb[:rows, :K] = z
    return zb.cuda()


def _run_roid(L, zb, ld, rows, K, ema, gs=1.0, correct=1, tau=C.TAU, clip=C.CLIP, eps=C.EPS, momentum=C.MOMENTUM):
    dev = "cuda"
    full = lambda shape, dtype=torch.float32: torch.full(shape, SENTINEL, dtype=dtype, device=dev)  # noqa: E731
    o = dict(lse=full((rows + 1,), torch.float64), p=full((rows + 1, ld)), scores=full((rows + 1, ld)), dZ=full((rows + 1, ld)),
             keep=torch.full((rows + 1,), 77, dtype=torch.uint8, device=dev), pbar=full((K + 1,)), prior=full((K + 1,)),
             counts=torch.full((5,), -9, dtype=torch.int32, device=dev), loss=full((2,)),
             ws=full((4 * rows + 2 * K + 1,), torch.float64))   # not cleared: written before it is read
    for k in ROW_FLOATS:
        o[k] = full((rows + 1,))
    e = torch.full((K + 1,), SENTINEL, dtype=torch.float32)
    e[:K] = ema
    o["ema"] = e.cuda()
    q = {k: v.data_ptr() for k, v in o.items()}
    L.roid_rows(zb.data_ptr(), ld, rows, K, q["ema"], tau, clip, eps, momentum, gs, correct, q["lse"], q["p"], ld, q["H"], q["cos"], q["slr"],
                q["dn"], q["cn"], q["w"], q["keep"], q["pbar"], q["prior"], q["scores"] if correct else None, ld, q["dZ"], ld, q["counts"],
                q["loss"], q["ws"], None)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize("rows,K,kind,ema_kind", C.roid_cases())
def test_roid_rows_against_float64(rows, K, kind, ema_kind):
    from stil_tta_amd._lib import lib
    L = lib()
    z, ema = C.roid_input(rows, K, kind), C.roid_ema(K, ema_kind)
    ref = C.roid_ref64(rows, K, kind, ema_kind)
    gs = f32(0.37)
    args = [f32(v) for v in (C.TAU, C.CLIP, C.EPS, C.MOMENTUM)]
    for pad in (0, 3):
        ld = K + pad
        zb = _padded(z, rows, K, pad)
        a, b = (_run_roid(L, zb, ld, rows, K, ema, gs, 1, *args) for _ in range(2))
        for k in a:
            if k != "ws":
                assert torch.equal(a[k], b[k]), f"{k}: not bit-identical on repetition"
        # sentinels: padding columns, the row past the end, the element past every vector
        for k in ("p", "scores", "dZ"):
            assert bool((a[k][rows] == SENTINEL).all()), k
            if pad:
                assert bool((a[k][:, K:] == SENTINEL).all()), k
        for k in ROW_FLOATS + ("lse",):
            assert float(a[k][rows]) == SENTINEL, k
        assert int(a["keep"][rows]) == 77 and int(a["counts"][4]) == -9 and float(a["loss"][1]) == SENTINEL
        assert float(a["pbar"][K]) == SENTINEL and float(a["prior"][K]) == SENTINEL and float(a["ema"][K]) == SENTINEL
        assert float(a["ws"][4 * rows + 2 * K]) == SENTINEL
        # the decisions, exactly
        assert torch.equal(a["keep"][:rows].bool(), ref["keep"]), "keep"
        assert torch.equal(a["counts"][:4], ref["counts"]), (a["counts"], ref["counts"])
        # everything else under close() at TOL
        close(a["lse"][:rows], ref["lse"], name="lse")
        close(a["p"][:rows, :K], ref["probs"], name="probs")
        for k in ROW_FLOATS:
            close(a[k][:rows], ref[k], name=k)
        close(a["pbar"][:K], ref["pbar"], name="pbar")
        close(a["prior"][:K], ref["prior"], name="prior")
        close(a["ema"][:K], ref["ema"], name="ema after the call")
        close(a["loss"][:1], ref["loss"].view(1), name="loss")
        close(a["dZ"][:rows, :K], ref["grad"] * gs, name="dZ")
        close(a["scores"][:rows, :K], ref["scores"], name="scores")
        close(a["scores"][:rows, :K].double().sum(1), torch.ones(rows, dtype=torch.float64), name="rows of scores sum to 1")
        assert bool((a["dZ"][:rows, :K][~ref["keep"]] == 0).all()), "a row that is not kept has a gradient"
        if rows == 1 or K == 1 or kind == "tied":
            assert a["counts"][2:4].tolist() == [1, 1] and bool((a["w"][:rows] == 1).all()) and bool(a["keep"][:rows].all())
            assert bool((a["dn"][:rows] == 0).all()) and bool((a["cn"][:rows] == 0).all())
        if K == 1:
            assert bool((a["dZ"][:rows, :K] == 0).all())
        # the tie to TENT's kernel: lse, p and H bit for bit
        t = G._run_entropy(L, zb, ld, rows, K, gs)
        assert torch.equal(a["lse"][:rows], t["lse"]) and torch.equal(a["H"][:rows], t["H"]) and torch.equal(a["p"][:rows, :K], t["p"])
        # correct = 0: scores (NULL here) and nothing else changes; prior is still written when given
        c = _run_roid(L, zb, ld, rows, K, ema, gs, 0, *args)
        assert bool((c["scores"] == SENTINEL).all())
        for k in a:
            if k not in ("ws", "scores"):
                assert torch.equal(c[k], a[k]), k


# ------------------------------------------------------------------------------------------ check 2: the ensemble
def _slab():
    n, params, _, theta0, _ = E.slab_input()
    c2t = torch.tensor(E.C2T, dtype=torch.int32).cuda()
    act = torch.tensor(E.ACTIVE, dtype=torch.uint8).cuda()
    ach = torch.tensor(E.ACHUNKS, dtype=torch.int32).cuda()
    return n, params, theta0, c2t, act, ach


def _ensemble(L, params, theta0, c2t, act, ach, n, m, na=None):
    P, T0 = params.cuda(), theta0.cuda()
    L.roid_ensemble(P.data_ptr(), T0.data_ptr(), ach.data_ptr(), len(E.ACHUNKS) if na is None else na, c2t.data_ptr(), act.data_ptr(),
                    len(E.ACTIVE), n, m, None)
    torch.cuda.synchronize()
    assert torch.equal(T0.cpu(), theta0)
    return P.cpu()


def test_roid_ensemble_against_float64():
    from stil_tta_amd._lib import lib
    L = lib()
    n, params, theta0, c2t, act, ach = _slab()
    live_of = {ch: j for j, ch in enumerate(E.ACHUNKS) if ch in E.LIVE}
    for m in (0.99, 0.5, f32(1.0 / 3.0)):
        a, b = (_ensemble(L, params, theta0, c2t, act, ach, n, f32(m)) for _ in range(2))
        assert torch.equal(a, b), "not bit-identical on repetition"
        for ch in range(len(E.C2T) + 1):       # the last is the sentinel chunk past the slab
            s = slice(ch * 1024, (ch + 1) * 1024)
            if ch in live_of:
                j = live_of[ch]
                want = C.ensemble_ref(params[s], theta0[j * 1024:(j + 1) * 1024], m)
                assert torch.equal(a[s], want), f"momentum {m}: chunk {ch} is not the float64 combination rounded once"
                assert not torch.equal(a[s], params[s])
            else:
                assert torch.equal(a[s], params[s]), f"momentum {m}: chunk {ch} outside A changed"
    assert torch.equal(_ensemble(L, params, theta0, c2t, act, ach, n, 1.0), params), "momentum 1 is not the identity bit for bit"
    z = _ensemble(L, params, theta0, c2t, act, ach, n, 0.0)
    for ch in range(len(E.C2T) + 1):
        s = slice(ch * 1024, (ch + 1) * 1024)
        want = theta0[live_of[ch] * 1024:(live_of[ch] + 1) * 1024] if ch in live_of else params[s]
        assert torch.equal(z[s], want), f"momentum 0: chunk {ch}"
    assert torch.equal(_ensemble(L, params, theta0, c2t, act, ach, n, 0.5, na=0), params), "an empty list of chunks wrote something"


# ------------------------------------------------------------------------------------------ check 3: bad arguments
def test_entry_points_reject_bad_arguments_with_nothing_written():
    from stil_tta_amd._lib import lib
    L = lib()
    fn, fe = L._dll.stil_roid_rows, L._dll.stil_roid_ensemble
    R, K = 4, 8
    dev = "cuda"
    names = ("z", "ema", "lse", "p", "H", "cos", "slr", "dn", "cn", "w", "keep", "pbar", "prior", "scores", "dz", "counts", "loss", "ws")
    shapes = dict(z=(R, K), p=(R, K), scores=(R, K), dz=(R, K), ema=(K,), pbar=(K,), prior=(K,), counts=(4,), loss=(1,), ws=(4 * R + 2 * K,))
    dtypes = dict(lse=torch.float64, ws=torch.float64, keep=torch.uint8, counts=torch.int32)
    ptr = {k: torch.full(shapes.get(k, (R,)), 3, dtype=dtypes.get(k, torch.float32), device=dev) for k in names}
    ptr["ema"].fill_(1.0 / K)
    before = {k: v.clone() for k, v in ptr.items()}
    c32, nan, inf = ctypes.c_float, float("nan"), float("inf")

    def call(ld=K, rows=R, K_=K, ldp=K, lds=K, ldd=K, tau=1.0 / 3.0, clip=0.99, eps=1e-5, mom=0.9, gs=1.0, correct=1, null=()):
        q = {k: (None if k in null else v.data_ptr()) for k, v in ptr.items()}
        return fn(q["z"], ld, rows, K_, q["ema"], c32(tau), c32(clip), c32(eps), c32(mom), c32(gs), correct, q["lse"], q["p"], ldp, q["H"],
                  q["cos"], q["slr"], q["dn"], q["cn"], q["w"], q["keep"], q["pbar"], q["prior"], q["scores"], lds, q["dz"], ldd, q["counts"],
                  q["loss"], q["ws"], None)

    refused = [call(null=(k,)) for k in names]
    refused += [call(rows=0), call(rows=-1), call(K_=0), call(K_=-3), call(ld=K - 1), call(ldp=K - 1), call(lds=K - 1), call(ldd=K - 1)]
    refused += [call(tau=v) for v in (0.0, -1.0, inf, nan)] + [call(eps=v) for v in (0.0, -1e-5, inf, nan)]
    refused += [call(clip=v) for v in (0.0, 1.0, 1.5, -0.5, inf, nan)] + [call(mom=v) for v in (-0.01, 1.01, inf, nan)]
    refused += [call(gs=v) for v in (inf, -inf, nan)] + [call(correct=2), call(correct=-1)]
    assert all(rc < 0 for rc in refused), refused
    assert b"stil_roid_rows" in L._dll.stil_last_error()
    # the ensemble
    n, params, theta0, c2t, act, ach = _slab()
    P, T0 = params.cuda(), theta0.cuda()
    tail = (ach.data_ptr(), len(E.ACHUNKS), c2t.data_ptr(), act.data_ptr(), len(E.ACTIVE))
    lng = ctypes.c_long

    def ens(p=P.data_ptr(), t0=T0.data_ptr(), tail_=tail, n_=n, m=0.99):
        return fe(p, t0, *tail_, lng(n_), c32(m), None)

    refused = [ens(p=None), ens(t0=None), ens(tail_=(None,) + tail[1:]), ens(tail_=tail[:2] + (None,) + tail[3:]), ens(tail_=tail[:3] + (None, tail[4]))]
    refused += [ens(n_=n + 5), ens(n_=-1024), ens(tail_=(tail[0], -1) + tail[2:]), ens(tail_=tail[:4] + (-1,)), ens(p=P.data_ptr() + 4), ens(t0=T0.data_ptr() + 4)]
    refused += [ens(m=v) for v in (-0.01, 1.01, inf, -inf, nan)]
    assert all(rc < 0 for rc in refused), refused
    assert b"stil_roid_ensemble" in L._dll.stil_last_error()
    torch.cuda.synchronize()
    for k, v in ptr.items():
        assert torch.equal(v, before[k]), f"a refused call wrote {k}"
    assert torch.equal(P.cpu(), params) and torch.equal(T0.cpu(), theta0), "a refused call wrote the slab"
    # and the calls they are variations of are accepted: scores, prior optional without the correction
    assert call() == 0 and call(correct=0, null=("scores", "prior"), lds=0) == 0 and call(mom=0.0) == 0 and call(mom=1.0) == 0 and call(gs=0.0) == 0
    assert ens() == 0 and ens(m=0.0) == 0 and ens(m=1.0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ check 4: the step, restated
def hyper(hp):
    """the scalars of the row loss as the float32 the C ABI receives"""
    return dict(tau=f32(hp.tta_roid_temperature), clip=f32(hp.tta_roid_clip), eps=f32(hp.tta_roid_eps), momentum=f32(hp.tta_probs_momentum))


def roid_restated(sd, keys, x, hp, dtype, ema, hyp, decisions=None):
    """ROID's adapting pass on one batch, on a deep copy of the state (the oracle updates running statistics in place): out_m of
    O.backbone_forward_all(train=True, masks=None), roid_cases.roid_forward against the running mean `ema`, autograd w.r.t. A.
    -> roid_forward's dict (loss detached) plus g {key: gradient} and flips"""
    s = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k in keys:
        s[k].requires_grad_(True)
    ctx = O.force_decisions(*decisions) if decisions is not None else contextlib.nullcontext()
    with ctx as d:
        out_m = O.backbone_forward_all(s, "model.", x[0].to(dtype), x[1].to(dtype), hp, train=True, masks=None)[0]
        out = C.roid_forward(out_m, ema.to(dtype), hyp["tau"], hyp["clip"], hyp["eps"], hyp["momentum"])
        g = torch.autograd.grad(out["loss"], [s[k] for k in keys])
    out["loss"] = out["loss"].detach()
    out["g"] = dict(zip(keys, [t.detach() for t in g]))
    out["flips"] = {t: v for t, v in d.get("flips", {}).items() if v[0]} if d is not None else {}
    return out


def ensemble_state(sd, source, keys, momentum):
    """the fp32 weight ensembling of the restated step, in place: sd[k] <- m sd[k] + (1 - m) source[k] over A, rounded once"""
    for k in keys:
        sd[k] = C.ensemble_ref(sd[k], source[k], momentum)


# (label, hparams, B, tta_params, batch seeds (online), state seed, head scale): tests/test_gpu_shot.py's protocol and states.  The
# batch seeds were chosen on the CPU (the float64 oracle, online through its own fp32 Adam and ensembling steps) so that the smallest
# margin |dn_r - mean dn| of every batch is >= 1e-3: the mask is then the same on any correct evaluation
PARITY = [
    ("dvm64_b16_x8", lambda: T.dvm_hp(16, img_size=64), 16, "bn", (501, 502), 41, G.HEAD_SCALE),
    ("cardiac64_b16_norm", lambda: T.cardiac_hp(16, img_size=64), 16, "norm", (601,), 51, None),
]
PARITY_LR = 1e-3
MIN_MARGIN = 1e-3


@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_roid_step_matches_roid_restated_in_float64(case):
    """Bars are TENT's (tests/test_gpu_tta.py): raw predictions <= 3e-5 scaled, every gradient of A <= 3 e32 + 1e-4, A after Adam AND
    the ensembling within 2.2 lr step of the fp32 restatement, everything outside A bit-identical; kept is the oracle's mask."""
    import test_gpu_step as S
    label, mk_hp, B, which, seeds, sseed, head = case
    hp = mk_hp()
    lr = PARITY_LR
    sd = G.parity_state(hp, sseed, head)
    m = T.make_model(hp, sd, tta=True, tta_method="roid", tta_params=which, tta_lr=lr)
    m.freeze()
    hyp, src_m = hyper(m.hp), m.hp.tta_roid_src_momentum
    assert (m.hp.tta_roid_temperature, src_m, m.hp.tta_roid_clip, m.hp.tta_roid_eps, m.hp.tta_probs_momentum) == (1.0 / 3.0, 0.99, 0.99, 1e-5, 0.9)
    keys = T.adapted_keys(m)
    assert len(keys) == (106 if which == "bn" else 106 + 2 * (1 + 4 * 2) + 2 * 2)
    K = hp.num_classes
    source = {k: v.clone() for k, v in sd.items() if k in set(keys)}
    opt = {}
    bad = []
    for step, seed in enumerate(seeds, start=1):
        x, y = T.tta_batch(hp, B, seed)
        before = T.full_state(m)
        sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
        ema_before = m._tent.ema.cpu().clone() if m._tent is not None else torch.full((K,), 1.0 / K, dtype=torch.float32)
        with S._trace_decisions() as trace:
            scores = m.test_step(T.to_dev((x, y)), step - 1)
            torch.cuda.synchronize()
            decisions = S._device_decisions(m, trace)
        lt = m.last_tta
        r64 = roid_restated(sd_before, keys, x, hp, torch.float64, ema_before, hyp, decisions)
        r64free = roid_restated(sd_before, keys, x, hp, torch.float64, ema_before, hyp)
        r32 = roid_restated(sd_before, keys, x, hp, torch.float32, ema_before, hyp)
        S._check_flips(r64["flips"])
        d = S._scaled(lt["probs_raw"].cpu().double().numpy(), r64["probs"].numpy())
        print(f"[{label}] batch {step}: raw predictions scaled error {d:.2e}; flips {({t: v[0] for t, v in r64['flips'].items()})}")
        print(f"[{label}] batch {step}: smallest margin |dn_r - mean dn| of the float64 oracle {r64['margin']:.3e} (free decisions "
              f"{r64free['margin']:.3e}); kept {int(r64['counts'][0])} of {B}; fp32 oracle's mask equal: {torch.equal(r32['keep'], r64['keep'])}")
        if d > 3e-5:
            bad.append((step, "predictions", d))
        assert r64["margin"] >= MIN_MARGIN, f"batch {step}: the oracle's margin {r64['margin']:.2e} makes the mask ill-posed: choose another seed"
        if not torch.equal(lt["kept"].cpu().bool(), r64["keep"]):
            bad.append((step, "kept", lt["kept"].cpu().tolist(), r64["keep"].tolist()))
        if int(lt["n_kept"]) != int(r64["counts"][0]):
            bad.append((step, "n_kept", int(lt["n_kept"])))
        for name, got, want in (("loss", lt["loss"].view(1), r64["loss"].view(1)), ("weight", lt["weight"], r64["w"]),
                                ("marginal", lt["marginal"], r64["pbar"]), ("prior", lt["prior"], r64["prior"]), ("probs", lt["probs"], r64["scores"])):
            got, want = got.cpu().double(), want.double()
            ratio = float(((got - want).abs() / (TOL * (1.0 + want.abs() + want.abs().max()))).max())
            print(f"[{label}] batch {step}: {name} error / close() bound {ratio:.3f}")
        # the reported scores are the correction of the device's own raw scores; the marginal their mean; the running mean moved
        praw = lt["probs_raw"].cpu().double()
        close(lt["probs_raw"], torch.softmax(lt["y_hat_m"].double(), dim=1), name="probs_raw against softmax(y_hat_m)")
        close(lt["marginal"], praw.mean(0), name="marginal against the mean of probs_raw")
        sc = praw * lt["prior"].cpu().double()[None, :]
        close(lt["probs"], sc / sc.sum(1, keepdim=True), name="probs against the correction of probs_raw")
        close(m._tent.ema, f32(0.9) * ema_before.double() + (1.0 - f32(0.9)) * praw.mean(0), name="running mean")
        assert torch.equal(scores, m._task_scores(lt["probs"]))
        gd = T.device_grads(m)
        ratios = []
        for k in keys:
            e32 = T._rel(r32["g"][k].double(), r64free["g"][k])
            err = T._rel(gd[k], r64["g"][k])
            ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
            if err > 3 * e32 + 1e-4:
                bad.append((step, "grad " + k, err, e32))
        print(f"[{label}] batch {step}: gradient error / (3*e32 + 1e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
        # Adam over A (fp32 oracle, its own moments) from the same parameters, then the ensembling with the source values
        sd32 = {k: v.clone() for k, v in sd_before.items()}
        O.adam_step(sd32, r32["g"], opt, step, lr)
        ensemble_state(sd32, source, keys, src_m)
        after = T.full_state(m)
        aset = set(keys)
        worst_adam = 0.0
        for k, v in after.items():
            if k in aset:
                dev = float((v.cpu() - sd32[k]).abs().max())
                worst_adam = max(worst_adam, dev / (2.2 * lr * step))
                if dev > 2.2 * lr * step:
                    bad.append((step, "adam " + k, dev))
            elif not torch.equal(v, before[k]):
                bad.append((step, "changed " + k))
        print(f"[{label}] batch {step}: deviation of A after Adam and ensembling / (2.2 lr step), worst: {worst_adam:.3f}")
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


# ------------------------------------------------------------------------------------------ check 5: properties
def _small(which="bn", method="roid", **tta):
    hp = T.dvm_hp(16, img_size=64)
    sd = T.initial_state(hp, 5)
    return hp, sd, (lambda: T.make_model(hp, sd, tta=True, tta_method=method, tta_params=which, **tta))


def _A(m):
    return {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}


def test_source_momentum_zero_returns_a_to_the_source_after_every_batch():
    hp, sd, mk = _small(tta_roid_src_momentum=0.0)
    m = mk()
    A0 = _A(m)
    K = hp.num_classes
    for i, seed in enumerate((11, 12)):
        b = T.to_dev(T.tta_batch(hp, 16, seed))
        ema_before = m._tent.ema.clone() if m._tent is not None else torch.full((K,), 1.0 / K, device="cuda")
        m.test_step(b, i)
        torch.cuda.synchronize()
        for k, v in A0.items():
            assert torch.equal(m.state_dict()[k], v), f"batch {i}: {k} is not its source value"
        assert int(m._tent.steps.max()) == i + 1 and bool((m._tent.exp_avg != 0).any()), "Adam did not run"
        # the scores still come from roid_loss: the same logits through the entry point give last_tta's bits
        from stil_tta_amd import tta
        z = m.last_tta["y_hat_m"].clone().requires_grad_(True)
        loss, scores, info = tta.roid_loss(z, ema_before, m.hp.tta_roid_temperature, 0.99, 1e-5, 0.9, True)
        assert torch.equal(scores, m.last_tta["probs"]) and torch.equal(info["probs"], m.last_tta["probs_raw"])
        assert torch.equal(loss.detach(), m.last_tta["loss"]) and torch.equal(info["keep"], m.last_tta["kept"])
        assert torch.equal(ema_before, m._tent.ema), "the replayed call moves the copy of the running mean to the state's value"
        assert not torch.equal(m.last_tta["probs"], m.last_tta["probs_raw"])
    # and with the default momentum A moves
    _, _, mk1 = _small()
    o = mk1()
    o.test_step(T.to_dev(T.tta_batch(hp, 16, 11)), 0)
    assert any(not torch.equal(o.state_dict()[k], v) for k, v in A0.items()), "the ROID step adapted nothing"


def test_ensembling_pulls_a_towards_the_source_by_the_stated_fraction():
    """A after a step at momentum 0.5 is, chunk for chunk, the ensemble of A after the same step at momentum 1 (no pull)."""
    hp, sd, mk1 = _small(tta_roid_src_momentum=1.0)
    _, _, mkh = _small(tta_roid_src_momentum=0.5)
    b = T.to_dev(T.tta_batch(hp, 16, 11))
    a, h = mk1(), mkh()
    A0 = _A(a)
    a.test_step(b, 0)
    h.test_step(b, 0)
    A1, Ah = _A(a), _A(h)
    assert any(not torch.equal(A1[k], A0[k]) for k in A0)
    for k in A0:
        assert torch.equal(Ah[k].cpu(), C.ensemble_ref(A1[k].cpu(), A0[k].cpu(), 0.5)), k
    # momentum 1 is TENT's bookkeeping with another loss: the scores and moments of both models agree, only A differs
    assert torch.equal(a.last_tta["probs"], h.last_tta["probs"]) and torch.equal(a._tent.exp_avg, h._tent.exp_avg)


def test_without_the_prior_correction_the_scores_are_the_raw_ones():
    hp, sd, mk = _small(tta_roid_prior_correction=False)
    _, _, mkc = _small()
    b = T.to_dev(T.tta_batch(hp, 16, 11))
    m, c = mk(), mkc()
    p, pc = m.test_step(b, 0), c.test_step(b, 0)
    lt = m.last_tta
    assert torch.equal(lt["probs"], lt["probs_raw"]) and torch.equal(p, m._task_scores(lt["probs_raw"]))
    close(lt["probs_raw"], torch.softmax(lt["y_hat_m"].double(), dim=1), name="probs_raw")
    # the correction is forward only: the same raw scores, loss and A with and without it, other reported scores
    assert torch.equal(lt["probs_raw"], c.last_tta["probs_raw"]) and torch.equal(lt["loss"], c.last_tta["loss"])
    assert torch.equal(lt["prior"], c.last_tta["prior"])
    for k, v in _A(m).items():
        assert torch.equal(v, c.state_dict()[k]), k
    assert not torch.equal(p, pc)
    close(c.last_tta["probs"].double().sum(1), torch.ones(16, dtype=torch.float64), name="rows of the corrected scores")


def test_episodic_mode_and_reset():
    hp, sd, mk = _small(tta_episodic=True)
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, 11)), T.to_dev(T.tta_batch(hp, 16, 12))
    K = hp.num_classes
    uniform = torch.full((K,), 1.0 / K, device="cuda")
    m = mk()
    m.test_step(b1, 0)
    assert not torch.equal(m._tent.ema, uniform)
    p2 = m.test_step(b2, 1).clone()
    s2, e2 = T.full_state(m), m._tent.ema.clone()
    f = mk()
    q2 = f.test_step(b2, 0).clone()
    t2 = T.full_state(f)
    assert torch.equal(p2, q2) and torch.equal(e2, f._tent.ema)
    for k in s2:
        assert torch.equal(s2[k], t2[k]), k
    # online: batch 2 sees batch 1's adaptation and running mean; reset_tta() restores A and the running mean bit for bit
    _, _, mk_on = _small()
    o = mk_on()
    A0 = _A(o)
    o.test_step(b1, 0)
    r2 = o.test_step(b2, 1).clone()
    assert not torch.equal(r2, q2), "online batch 2 equals the episodic one: nothing carried over"
    o.reset_tta()
    for k, v in A0.items():
        assert torch.equal(o.state_dict()[k], v), k
    assert torch.equal(o._tent.ema, uniform) and int(o._tent.steps.max()) == 0
    _, _, mk_f = _small()
    fresh = mk_f()
    assert torch.equal(o.test_step(b2, 2), fresh.test_step(b2, 0)), "after reset_tta() the next batch starts from the source, fresh moments, 1 / K"


@pytest.mark.parametrize("which", ["bn", "norm"])
def test_roid_step_issues_no_weight_gradient_product(which, monkeypatch):
    from stil_tta_amd._lib import lib
    hp, sd, mk = _small(which)
    m = mk()
    L = lib()
    calls = []
    for name in ("wgrad_tn", "wgrad_tn_partial"):
        orig = getattr(L, name)
        monkeypatch.setitem(L.__dict__, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    A0 = _A(m)
    m.test_step(T.to_dev(T.tta_batch(hp, 16, 7)), 0)
    torch.cuda.synchronize()
    assert calls == [], f"{len(calls)} weight-gradient launches in a ROID step"
    assert any(not torch.equal(m.state_dict()[k], v) for k, v in A0.items()), "the ROID step adapted nothing"


def test_freeze_and_inference_mode():
    hp, sd, mk = _small()
    b = T.to_dev(T.tta_batch(hp, 16, 14))
    a, c = mk(), mk()
    a.freeze()
    c.freeze()
    with torch.inference_mode():
        pa = a.test_step(b, 0)
    pc = c.test_step(b, 0)
    assert torch.equal(pa, pc) and torch.equal(a._tent.ema, c._tent.ema)
    sa, sc = T.full_state(a), T.full_state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert any(not torch.equal(sa[k], v) for k, v in T.full_state(mk()).items() if k in set(T.adapted_keys(a)))
    assert not any(q.requires_grad for q in a.parameters()) and not any(q.requires_grad for q in c.parameters())


def test_bn_prior_and_bn_momentum_compose():
    hp, sd, mk = _small(tta_bn_prior=16, tta_bn_momentum=0.1)
    _, _, mk0 = _small()
    b = T.to_dev(T.tta_batch(hp, 16, 11))
    m, o = mk(), mk0()
    p, q = m.test_step(b, 0), o.test_step(b, 0)
    assert m._bn_mem is not None and m._bn_mem.t == 1 and o._bn_mem is None
    assert bool(torch.isfinite(p).all()) and not torch.equal(p, q), "the BatchNorm prior and memory changed nothing"


def test_ragged_last_batch():
    hp, sd, mk = _small()
    m = mk()
    m.test_step(T.to_dev(T.tta_batch(hp, 16, 11)), 0)
    A1 = _A(m)
    p = m.test_step(T.to_dev(T.tta_batch(hp, 5, 12)), 1)
    torch.cuda.synchronize()
    lt = m.last_tta
    K = hp.num_classes
    assert p.shape == (5, K) and lt["probs"].shape == (5, K) and lt["probs_raw"].shape == (5, K)
    assert lt["marginal"].shape == (K,) and lt["prior"].shape == (K,) and lt["kept"].shape == (5,) and lt["weight"].shape == (5,)
    for k in ("loss", "probs", "probs_raw", "weight", "marginal", "prior"):
        assert lt[k].is_cuda and bool(torch.isfinite(lt[k]).all()), k
    assert 1 <= int(lt["n_kept"]) == int(lt["kept"].sum()) <= 5
    close(lt["marginal"], lt["probs_raw"].double().mean(0), name="marginal against the mean of probs_raw")
    close(lt["probs"].double().sum(1), torch.ones(5, dtype=torch.float64), name="rows of the scores")
    assert int(m._tent.steps.max()) == 2
    assert any(not torch.equal(m.state_dict()[k], v) for k, v in A1.items()), "the short batch adapted nothing"
    # one row: both ranges degenerate, the row is kept with weight 1
    m.test_step(T.to_dev(T.tta_batch(hp, 1, 13)), 2)
    assert int(m.last_tta["n_kept"]) == 1 and float(m.last_tta["weight"][0]) == 1.0


def test_fit_test_and_test_shifts_take_the_adapting_path(tmp_path):
    from stil_tta_amd import fit
    hp, sd, mk = _small()
    loader = [T.tta_batch(hp, 16, 20 + i) for i in range(3)]
    ck = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": {k: v.clone() for k, v in sd.items()}}, ck)
    a = mk()
    a.test_step(T.to_dev(loader[0]), 0)          # adaptation state from an earlier run: the checkpoint load must discard it
    a.load_state_dict({k: v.cuda() for k, v in T.initial_state(hp, 77).items()})
    assert a._tent is None
    ra = fit.test(a, loader, ck)
    h = mk()
    h.freeze()
    h.acc_test.reset()
    h.auc_test.reset()
    for i, bt in enumerate(loader):
        h.test_step(T.to_dev(bt), i)
    rh = {k: float(v) for k, v in h.test_epoch_end().items()}
    assert ra.keys() == rh.keys() and all(ra[k] == rh[k] or (ra[k] != ra[k] and rh[k] != rh[k]) for k in ra), (ra, rh)
    sa, sh = T.full_state(a), T.full_state(h)
    for k in sa:
        assert torch.equal(sa[k], sh[k]), k
    assert torch.equal(a._tent.ema, h._tent.ema)
    off = T.make_model(hp, sd, tta=True)
    fit.test(off, loader, ck)
    so = T.full_state(off)
    assert any(not torch.equal(so[k], sa[k]) for k in T.adapted_keys(a)), "fit.test with ROID left A where the run without TTA leaves it"
    # fit.test_shifts: "reset" starts every shift from the source model and 1 / K, "continual" carries A and the running mean over
    from stil_tta_amd import shift as SH
    from stil_tta_amd.modules import split_field_lengths
    cat, con = split_field_lengths(hp.field_lengths)
    stats = SH.TableStats(cat, [1.0] * (len(cat) + len(con)), [0.0] * (len(cat) + len(con)))
    shifts = {"noise": SH.ShiftSpec(image=("gaussian_noise", 3), tabular=("tab_noise", 3), seed=1, stats=stats),
              "contrast": SH.ShiftSpec(image=("contrast", 4), tabular=("tab_missing", 2), seed=2, stats=stats)}
    r, c = mk(), mk()
    res_r = fit.test_shifts(r, loader[:2], shifts, ck, protocol="reset")
    res_c = fit.test_shifts(c, loader[:2], shifts, ck, protocol="continual")
    assert list(res_r) == list(res_c) == ["noise", "contrast", "mean"]
    alone = mk()
    fit.test(alone, loader[:2], ck, shift=shifts["contrast"])
    sr, sc_, sl = T.full_state(r), T.full_state(c), T.full_state(alone)
    for k in sr:
        assert torch.equal(sr[k], sl[k]), k
    assert torch.equal(r._tent.ema, alone._tent.ema) and not torch.equal(c._tent.ema, alone._tent.ema)
    assert any(not torch.equal(sc_[k], sl[k]) for k in T.adapted_keys(c)), "continual: the second shift started from the source values"
    assert int(r._tent.steps.max()) == 2 and int(c._tent.steps.max()) == 4
