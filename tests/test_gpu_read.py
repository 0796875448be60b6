"""READ test-time adaptation (Yang et al., ICLR 2024, "Test-time Adaptation against Multi-modal Reliability Bias") in
STiLModel.test_step: the encoders frozen, the last fusion layer's Q/K/V projection adapted under a confidence-aware loss with a
batch-balance term, on top of TENT (tests/test_gpu_tta.py) and SHOT-IM (tests/test_gpu_shot.py).

1. stil_read_rows against float64 autograd (close() at TOL of test_gpu_ops), ld = K + 3 views, sentinels, repetition; lse and p
   are stil_entropy_rows' bits, pbar and out[2] stil_infomax_rows'; yhat exact; p = NULL and dZ = NULL.
2. Bad arguments are refused with nothing written.
3. The step against READ restated here in float64 on the oracle, on the device's yhat.
4. The backward stays out of the encoders.
5. First-batch scores are test_step's without adaptation.
6. tta_div_weight = 0.
7. Episodic mode, reset_tta(), freeze() + torch.inference_mode(), fit.test.
tests/test_read_cpu.py checks on the CPU that the inputs used here are well-conditioned (fp32 ATen and the fp32 oracle meet the
same bars, yhat is unambiguous and rows lie on both sides of gamma)."""
import ctypes
import functools
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_gpu_ops import close  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
import test_gpu_tta as T  # noqa: E402
from test_gpu_shot import f32, parity_state  # noqa: E402

SENTINEL = -7.25
KINDS = T.ENT_KINDS + ("near_gamma",)
LAMBDAS = (0.0, 1.0)
EPS = 1e-5
GAMMA = math.exp(-1.0)


# ------------------------------------------------------------------------------------------ check 1: the entry point
def read_cases():
    return [(r, k, kind, lam) for r in T.ENT_ROWS for k in T.ENT_K for kind in KINDS for lam in LAMBDAS]


def read_input(rows, K, kind, gamma=GAMMA):
    """float32 logits [rows, K]: T.entropy_input's three kinds, and near_gamma: one logit above K - 1 equal ones (zeros), placed
    so that the row's confidence runs from 0.5 gamma (row 0) to 1.5 gamma (the last row), clamped into (1 / K, 1): rows on both
    sides of the sign change of ln(gamma / c).  K = 1 has the one confidence 1."""
    if kind in T.ENT_KINDS:
        return T.entropy_input(rows, K, kind)
    z = torch.zeros(rows, K, dtype=torch.float64)
    if K > 1:
        c = gamma * torch.linspace(0.5, 1.5, rows, dtype=torch.float64)
        c = c.clamp(1.0 / K + 0.02 * (1.0 - 1.0 / K), 0.98)
        r = torch.arange(rows)
        z[r, (7 * r) % K] = torch.log(c * (K - 1) / (1.0 - c))
    return z.float()


def first_max(x):
    """the first maximum of every row (torch.argmax promises no order among ties)"""
    K = x.shape[1]
    idx = torch.arange(K).expand_as(x)
    return torch.where(x == x.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, K)).min(dim=1).values


def read_loss(out_m, gamma, lam, eps, yhat=None):
    """READ's loss of logits as csrc/stil_read.h states it, yhat (the first maximum when not given) held fixed.
    -> (loss, mean f, D, log p, f, c, mean prediction, yhat)"""
    logp = torch.log_softmax(out_m, dim=1)
    p = logp.exp()
    if yhat is None:
        yhat = first_max(out_m.detach())
    lc = logp.gather(1, yhat.view(-1, 1).long()).squeeze(1)
    c = lc.exp()
    f = c * (1.0 + math.log(gamma) - lc)
    pbar = p.mean(dim=0)
    D = (pbar * torch.log(pbar + eps)).sum()
    conf = f.mean()
    return conf + lam * D, conf, D, logp, f, c, pbar, yhat


def read_ref(z, gamma, lam, eps, dtype):
    """The loss with autograd in `dtype`: -> dict(loss, conf_loss, D, grad, probs, f, conf, lse, pbar, yhat)."""
    x = z.detach().to(dtype).clone().requires_grad_(True)
    loss, cl, D, logp, f, c, pbar, yhat = read_loss(x, gamma, lam, eps)
    (g,) = torch.autograd.grad(loss, [x])
    return dict(loss=loss.detach(), conf_loss=cl.detach(), D=D.detach(), grad=g, probs=logp.exp().detach(), f=f.detach(),
                conf=c.detach(), lse=torch.logsumexp(x.detach(), dim=1), pbar=pbar.detach(), yhat=yhat)


@functools.lru_cache(maxsize=None)
def read_ref64(rows, K, kind, lam):
    """the float64 reference of one case, computed once (read-only), at the gamma, weight and eps the kernel receives"""
    return read_ref(read_input(rows, K, kind), f32(GAMMA), f32(lam), f32(EPS), torch.float64)


def _run_read(L, zb, ld, rows, K, gs, gamma, lam, eps, p=True, dz=True):
    dev = "cuda"
    o = dict(lse=torch.full((rows + 1,), SENTINEL, dtype=torch.float64, device=dev), p=torch.full((rows + 1, ld), SENTINEL, device=dev),
             yhat=torch.full((rows + 1,), -7, dtype=torch.int32, device=dev), conf=torch.full((rows + 1,), SENTINEL, device=dev),
             f=torch.full((rows + 1,), SENTINEL, device=dev), pbar=torch.full((K + 1,), SENTINEL, device=dev),
             dZ=torch.full((rows + 1, ld), SENTINEL, device=dev), out=torch.full((4,), SENTINEL, device=dev),
             ws=torch.full((2 * K + 1,), SENTINEL, dtype=torch.float64, device=dev))   # not cleared: written before it is read
    L.read_rows(zb.data_ptr(), ld, rows, K, gs, gamma, lam, eps, o["lse"].data_ptr(), o["p"].data_ptr() if p else None, ld,
                o["yhat"].data_ptr(), o["conf"].data_ptr(), o["f"].data_ptr(), o["pbar"].data_ptr(), o["dZ"].data_ptr() if dz else None, ld,
                o["out"].data_ptr(), o["ws"].data_ptr(), None)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _run_infomax(L, zb, ld, rows, K, gs, lam, eps):
    lse = torch.empty(rows, dtype=torch.float64, device="cuda")
    H, pbar, out = torch.empty(rows, device="cuda"), torch.empty(K, device="cuda"), torch.empty(3, device="cuda")
    ws = torch.empty(2 * K + rows, dtype=torch.float64, device="cuda")
    L.infomax_rows(zb.data_ptr(), ld, rows, K, gs, lam, eps, lse.data_ptr(), None, ld, H.data_ptr(), pbar.data_ptr(), None, ld,
                   out.data_ptr(), ws.data_ptr(), None)
    torch.cuda.synchronize()
    return dict(pbar=pbar.cpu(), out=out.cpu())


def _padded(z, rows, K, pad):
    zb = torch.full((rows + 1, K + pad), SENTINEL, dtype=torch.float32)
    zb[:rows, :K] = z
    return zb.cuda()


@pytest.mark.parametrize("rows,K,kind,lam", read_cases())
def test_read_rows_against_float64(rows, K, kind, lam):
    from stil_tta_amd._lib import lib
    L = lib()
    z = read_input(rows, K, kind)
    ref = read_ref64(rows, K, kind, lam)
    gs, g32, lam32, eps32 = f32(1.0 / rows), f32(GAMMA), f32(lam), f32(EPS)
    for pad in (0, 3):
        ld = K + pad
        zb = _padded(z, rows, K, pad)
        a, b = (_run_read(L, zb, ld, rows, K, gs, g32, lam32, eps32) for _ in range(2))
        for k in a:
            if k != "ws":
                assert torch.equal(a[k], b[k]), f"{k}: not bit-identical on repetition"
        # sentinels: padding columns, the row past the end, the element past every vector
        assert bool((a["p"][rows] == SENTINEL).all() and (a["dZ"][rows] == SENTINEL).all())
        assert float(a["lse"][rows]) == SENTINEL and float(a["conf"][rows]) == SENTINEL and float(a["f"][rows]) == SENTINEL
        assert int(a["yhat"][rows]) == -7 and float(a["pbar"][K]) == SENTINEL
        assert float(a["out"][3]) == SENTINEL and float(a["ws"][2 * K]) == SENTINEL
        if pad:
            assert bool((a["p"][:, K:] == SENTINEL).all() and (a["dZ"][:, K:] == SENTINEL).all())
        # yhat is exact (the first maximum; `tied`: 0), and conf is that entry of p
        assert torch.equal(a["yhat"][:rows].long(), ref["yhat"]), "yhat"
        if kind == "tied":
            assert bool((a["yhat"][:rows] == 0).all())
        assert torch.equal(a["conf"][:rows], a["p"][:rows, :K].gather(1, ref["yhat"].view(-1, 1)).squeeze(1)), "conf is not p[r, yhat[r]]"
        close(a["lse"][:rows], ref["lse"], name="lse")
        close(a["p"][:rows, :K], ref["probs"], name="probs")
        close(a["conf"][:rows], ref["conf"], name="conf")
        close(a["f"][:rows], ref["f"], name="f")
        close(a["pbar"][:K], ref["pbar"], name="pbar")
        close(a["dZ"][:rows, :K], ref["grad"] * (gs * rows), name="dZ")   # grad_scale as the float32 the kernel receives
        close(a["out"][0:1], ref["loss"].view(1), name="out[0]")
        close(a["out"][1:2], ref["conf_loss"].view(1), name="out[1]")
        close(a["out"][2:3], ref["D"].view(1), name="out[2]")
        if K == 1:
            assert bool((a["dZ"][:rows, :K] == 0).all()) and bool((a["conf"][:rows] == 1).all())
        # ties to the two kernels it is built on: lse, p of stil_entropy_rows; pbar, D of stil_infomax_rows, bit for bit
        t = _run_entropy(L, zb, ld, rows, K, gs)
        assert torch.equal(a["lse"][:rows], t["lse"]) and torch.equal(a["p"][:rows, :K], t["p"])
        s = _run_infomax(L, zb, ld, rows, K, gs, lam32, eps32)
        assert torch.equal(a["pbar"][:K], s["pbar"]) and torch.equal(a["out"][2:3], s["out"][2:3])
    # p == NULL, dZ == NULL: the other outputs are unchanged
    for no_p, no_dz in ((True, False), (False, True), (True, True)):
        c = _run_read(L, zb, ld, rows, K, gs, g32, lam32, eps32, p=not no_p, dz=not no_dz)
        for k in ("lse", "p", "yhat", "conf", "f", "pbar", "dZ", "out"):
            if (k == "p" and no_p) or (k == "dZ" and no_dz):
                assert bool((c[k] == SENTINEL).all()), (no_p, no_dz, k)
            else:
                assert torch.equal(c[k], a[k]), (no_p, no_dz, k)


def _run_entropy(L, zb, ld, rows, K, gs):
    lse = torch.empty(rows, dtype=torch.float64, device="cuda")
    p, dZ = torch.empty(rows, ld, device="cuda"), torch.empty(rows, ld, device="cuda")
    H, mean = torch.empty(rows, device="cuda"), torch.empty(1, device="cuda")
    L.entropy_rows(zb.data_ptr(), ld, rows, K, gs, lse.data_ptr(), p.data_ptr(), ld, H.data_ptr(), dZ.data_ptr(), ld, mean.data_ptr(), None)
    torch.cuda.synchronize()
    return dict(lse=lse.cpu(), p=p.cpu()[:, :K])


# ------------------------------------------------------------------------------------------ check 2: bad arguments
def test_read_rows_rejects_bad_arguments_with_nothing_written():
    from stil_tta_amd._lib import lib
    fn = lib()._dll.stil_read_rows
    rows, K = 4, 8
    z = torch.zeros(rows, K, device="cuda")

    def fresh():
        return dict(lse=torch.full((rows,), SENTINEL, dtype=torch.float64, device="cuda"), p=torch.full((rows, K), SENTINEL, device="cuda"),
                    yhat=torch.full((rows,), -7, dtype=torch.int32, device="cuda"), conf=torch.full((rows,), SENTINEL, device="cuda"),
                    f=torch.full((rows,), SENTINEL, device="cuda"), pbar=torch.full((K,), SENTINEL, device="cuda"),
                    dz=torch.full((rows, K), SENTINEL, device="cuda"), out=torch.full((3,), SENTINEL, device="cuda"),
                    ws=torch.full((2 * K,), SENTINEL, dtype=torch.float64, device="cuda"))

    def call(o, ld=K, rows=rows, K=K, ldp=K, ldd=K, gamma=GAMMA, lam=1.0, eps=EPS, null=()):
        q = {k: (None if k in null else v.data_ptr()) for k, v in o.items()}
        c32 = ctypes.c_float
        return fn(None if "z" in null else z.data_ptr(), ld, rows, K, c32(0.25), c32(gamma), c32(lam), c32(eps), q["lse"], q["p"], ldp,
                  q["yhat"], q["conf"], q["f"], q["pbar"], q["dz"], ldd, q["out"], q["ws"], None)

    def untouched(o):
        torch.cuda.synchronize()
        return all(bool((v == (-7 if k == "yhat" else SENTINEL)).all()) for k, v in o.items())

    bad = [dict(null=(k,)) for k in ("z", "lse", "yhat", "conf", "f", "pbar", "out", "ws")]
    bad += [dict(rows=0), dict(rows=-1), dict(K=0), dict(K=-3), dict(ld=K - 1), dict(ldp=K - 1), dict(ldd=K - 1)]
    bad += [dict(gamma=g) for g in (0.0, -0.1, 1.0000001, 2.0, float("inf"), float("-inf"), float("nan"))]
    bad += [dict(eps=e) for e in (0.0, -1e-5, float("inf"), float("nan"))]
    bad += [dict(lam=w) for w in (-0.5, float("inf"), float("-inf"), float("nan"))]
    for kw in bad:
        o = fresh()
        assert call(o, **kw) < 0, kw
        assert untouched(o), f"{kw}: refused, yet something was written"
    for kw in (dict(), dict(null=("p",)), dict(null=("dz",)), dict(null=("p", "dz"), ldp=0, ldd=0), dict(gamma=1.0), dict(lam=0.0)):
        o = fresh()
        assert call(o, **kw) == 0, kw
        torch.cuda.synchronize()
        assert bool((o["out"] != SENTINEL).all())


# ------------------------------------------------------------------------------------------ check 3: the step, restated
def read_restated(sd, keys, x, hp, dtype, gamma, lam, eps, yhat=None):
    """READ on one batch, on a copy of the state: out_m of O.backbone_forward_all(train=False) (eval-mode BatchNorm, no MI-layer
    dropout), read_loss with yhat given (None: its own first maximum), autograd w.r.t. the two tensors of A.  No ReLU or max-pool
    lies between A and the loss, so there are no decisions to force.
    -> dict(p, g {key: gradient}, out_m, conf, l_conf, D, pbar, yhat)"""
    s = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k in keys:
        s[k].requires_grad_(True)
    out_m = O.backbone_forward_all(s, "model.", x[0].to(dtype), x[1].to(dtype), hp, train=False, masks=None)[0]
    loss, cl, D, logp, _, c, pbar, yhat = read_loss(out_m, gamma, lam, eps, yhat)
    g = torch.autograd.grad(loss, [s[k] for k in keys])
    return dict(p=logp.exp().detach(), g=dict(zip(keys, [t.detach() for t in g])), out_m=out_m.detach(), conf=c.detach(),
                l_conf=cl.detach(), D=D.detach(), pbar=pbar.detach(), yhat=yhat)


def fusion_keys(hp):
    last = hp.multimodal_transformer_num_layers - 1
    return [f"model.transformer.{last}.attn.qkv.weight", f"model.transformer.{last}.attn.qkv.bias"]


def case_gamma(gamma):
    return GAMMA if gamma is None else gamma


# (label, hparams, B, batch seeds (online), state seed, head scale, tta_read_gamma).  Random states predict one class with confidence
# >= 0.96, which never reaches the c < gamma branch: every case scales the multimodal head down; K = 2 has c >= 0.5 > 1/e, so the
# cardiac case sets a gamma above its confidences' median (tests/test_read_cpu.py holds both).
PARITY = [
    ("dvm64_b16", lambda: T.dvm_hp(16, img_size=64), 16, (7, 11), 5, 0.25, None),
    ("dvm64_b16_two_layers", lambda: T.dvm_hp(16, img_size=64, multimodal_transformer_num_layers=2), 16, (7,), 5, 0.25, 0.343),
    ("cardiac64_b16", lambda: T.cardiac_hp(16, img_size=64), 16, (7,), 5, 0.25, 0.57),
]
PARITY_LR = 1e-4    # READ's published rate (as recalled); at 1e-3 one step moves every confidence of the next batch below 1/e


def read_model(hp, sd, **tta):
    kw = dict(tta=True, tta_method="read", tta_params="fusion")
    kw.update(tta)
    return T.make_model(hp, sd, **kw)


@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_read_step_matches_read_restated_in_float64(case):
    """Bars are TENT's (tests/test_gpu_tta.py): predictions <= 3e-5 scaled, each gradient of A <= 3 e32 + 1e-4, Adam within
    2.2 lr step, everything outside A bit-identical (with two fusion layers: layer 0 too); the float64 restatement takes the
    device's yhat, which must be its own."""
    from test_gpu_step import _scaled
    label, mk_hp, B, seeds, sseed, head, gamma = case
    hp = mk_hp()
    lr = PARITY_LR
    sd = parity_state(hp, sseed, head)
    m = read_model(hp, sd, tta_lr=lr, tta_read_gamma=gamma)
    m.freeze()
    lam, eps, gam = m.hp.tta_div_weight, m.hp.tta_div_eps, case_gamma(gamma)
    assert (lam, eps) == (1.0, 1e-5)
    keys = T.adapted_keys(m)
    assert keys == fusion_keys(hp)
    opt = {}
    bad = []
    for step, seed in enumerate(seeds, start=1):
        x, y = T.tta_batch(hp, B, seed)
        before = T.full_state(m)
        sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
        m.test_step(T.to_dev((x, y)), step - 1)
        torch.cuda.synchronize()
        lt = m.last_tta
        probs = lt["probs"].cpu().double()
        yhat = lt["yhat"].cpu().long()
        r64 = read_restated(sd_before, keys, x, hp, torch.float64, gam, lam, eps, yhat)
        r32 = read_restated(sd_before, keys, x, hp, torch.float32, gam, lam, eps)
        assert torch.equal(yhat, first_max(r64["out_m"])), "the device's yhat is not float64's"
        d = _scaled(probs.numpy(), r64["p"].numpy())
        below = int((r64["conf"] < gam).sum())
        print(f"[{label}] batch {step}: predictions scaled error {d:.2e}; {below} rows below gamma, {B - below} above")
        if d > 3e-5:
            bad.append((step, "predictions", d))
        close(lt["loss_confidence"].view(1), r64["l_conf"].view(1), name="loss_confidence")
        close(lt["loss_balance"].view(1), r64["D"].view(1), name="loss_balance")
        close(lt["loss"].view(1), (r64["l_conf"] + lam * r64["D"]).view(1), name="loss")
        close(lt["marginal"], r64["pbar"], name="marginal")
        close(lt["conf"], r64["conf"], name="conf")
        close(lt["probs"], torch.softmax(lt["y_hat_m"].double(), dim=1), name="probs against softmax(y_hat_m)")
        gd = T.device_grads(m)
        ratios = []
        for k in keys:
            e32 = T._rel(r32["g"][k].double(), r64["g"][k])
            err = T._rel(gd[k], r64["g"][k])
            ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
            if err > 3 * e32 + 1e-4:
                bad.append((step, "grad " + k, err, e32))
        print(f"[{label}] batch {step}: gradient error / (3*e32 + 1e-4): {ratios}")
        # Adam over A (fp32 oracle, its own moments) from the same parameters
        sd32 = {k: v.clone() for k, v in sd_before.items()}
        O.adam_step(sd32, r32["g"], opt, step, lr)
        after = T.full_state(m)
        aset = set(keys)
        worst_adam = 0.0
        for k, v in after.items():
            if k in aset:
                dev = float((v.cpu() - sd32[k]).abs().max())
                worst_adam = max(worst_adam, dev / (2.2 * lr * step))
                if dev > 2.2 * lr * step:
                    bad.append((step, "adam " + k, dev))
                if torch.equal(v, before[k]):
                    bad.append((step, "unchanged " + k))
            elif not torch.equal(v, before[k]):
                bad.append((step, "changed " + k))
        print(f"[{label}] batch {step}: Adam deviation / (2.2 lr step), worst: {worst_adam:.3f}")
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


# ------------------------------------------------------------------------------------------ check 4: the backward's reach
def _small(**tta):
    hp = T.dvm_hp(16, img_size=64)
    sd = parity_state(hp, 5, 0.25)
    return hp, sd, (lambda: read_model(hp, sd, **tta))


def test_read_backward_stays_out_of_the_encoders(monkeypatch):
    """One step on the small model: no BatchNorm, max-pool or tabular-embedding backward runs; the attention backward runs for
    ONE attention layer, i.e. once for each of the fusion layer's three windows (image, table, shared token: stil_attention_bwd is
    a per-window entry point), never for the tabular encoder's four blocks; the weight gradient of qkv is a product."""
    from stil_tta_amd._lib import lib
    hp, sd, mk = _small()
    m = mk()
    L = lib()
    calls = []
    never = ("bn_train_bwd", "bn_train_bwd_tiles", "bn_prior_bwd", "bn_prior_bwd_tiles", "maxpool3x3s2_bwd", "tab_embed_bwd")
    for name in never + ("attention_bwd", "wgrad_tn", "wgrad_tn_partial"):
        orig = getattr(L, name)
        monkeypatch.setitem(L.__dict__, name, lambda *a, _o=orig, _n=name, **k: (calls.append((_n, a)), _o(*a, **k))[1])
    A0 = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    m.test_step(T.to_dev(T.tta_batch(hp, 16, 7)), 0)
    torch.cuda.synchronize()
    names = [n for n, _ in calls]
    for name in never:
        assert names.count(name) == 0, f"{name} ran {names.count(name)} times in a READ step"
    Ni, Nt = (64 // 32) ** 2, len(hp.field_lengths)
    T_ = 1 + Ni + Nt
    windows = sorted(a[9:13] for n, a in calls if n == "attention_bwd")   # (q_off, Sq, kv_off, Skv) of stil_attention_bwd
    assert windows == sorted([(1, Ni, 1, Ni), (1 + Ni, Nt, 1 + Ni, Nt), (0, 1, 0, T_)]), \
        f"the attention backward must run once, over the three windows of the one fusion layer: {windows}"
    assert names.count("wgrad_tn") + names.count("wgrad_tn_partial") >= 1
    assert all(not torch.equal(m.state_dict()[k], v) for k, v in A0.items()), "the READ step left a tensor of A unchanged"


# ------------------------------------------------------------------------------------------ check 5: the first batch's scores
def test_first_batch_scores_are_test_steps_without_adaptation():
    """The logits are bit for bit those of the model without adaptation: up to them the forward makes the launches test_step makes.
    One launch differs, the softmax: the scores here are the p of stil_read_rows (formed in double and rounded once, stil_entropy_rows'
    bits), test_step's come from stil_row_softmax_fwd; that comparison is held at _scaled <= 3e-5."""
    from test_gpu_step import _scaled
    hp, sd, mk = _small()
    b = T.to_dev(T.tta_batch(hp, 16, 7))
    a, off = mk(), T.make_model(hp, sd, tta=False)
    pa, po = a.test_step(b, 0), off.test_step(b, 0)
    with torch.no_grad():
        zo = off.model.forward((b[0][0], b[0][1]), train=False)[0]
    torch.cuda.synchronize()
    za = a.last_tta["y_hat_m"]
    d = _scaled(pa.cpu().numpy(), po.cpu().numpy())
    print(f"logits: max difference {float((za - zo).abs().max()):.3e}; scores: scaled difference {d:.2e}")
    assert torch.equal(za, zo), f"logits: max difference {float((za - zo).abs().max()):.3e}"
    assert d <= 3e-5
    assert torch.equal(a.last_tta["probs"], pa)
    p2 = a.test_step(b, 1)
    assert not torch.equal(p2, po), "the second batch shows no adaptation"


# ------------------------------------------------------------------------------------------ check 6: tta_div_weight = 0
def test_zero_div_weight_is_the_confidence_loss_alone():
    hp, sd, mk0 = _small(tta_div_weight=0.0)
    _, _, mk1 = _small()
    b = T.to_dev(T.tta_batch(hp, 16, 7))
    z, w = mk0(), mk1()
    z.test_step(b, 0)
    w.test_step(b, 0)
    torch.cuda.synchronize()
    lz, lw = z.last_tta, w.last_tta
    assert torch.equal(lz["loss"], lz["loss_confidence"])
    assert torch.equal(lz["loss_balance"], lw["loss_balance"]) and bool(torch.isfinite(lz["loss_balance"])) and float(lz["loss_balance"]) < 0
    assert torch.equal(lz["loss_confidence"], lw["loss_confidence"]) and not torch.equal(lw["loss"], lw["loss_confidence"])
    ka = T.adapted_keys(z)
    assert any(not torch.equal(z.state_dict()[k], w.state_dict()[k]) for k in ka), "the balance term moved nothing"


# ------------------------------------------------------------------------------------------ check 7: inherited properties
def _adapt_state(m):
    st = m._tent
    out = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    out.update({"#tta_exp_avg": st.exp_avg.clone(), "#tta_exp_avg_sq": st.exp_avg_sq.clone(), "#tta_steps": st.steps.clone()})
    return out


def test_episodic_mode_and_reset():
    hp, sd, mk = _small(tta_episodic=True)
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, 11)), T.to_dev(T.tta_batch(hp, 16, 12))
    m = mk()
    m.test_step(b1, 0)
    p2 = m.test_step(b2, 1).clone()
    s2, a2 = T.full_state(m), _adapt_state(m)
    f = mk()
    q2 = f.test_step(b2, 0).clone()
    t2, c2 = T.full_state(f), _adapt_state(f)
    assert torch.equal(p2, q2)
    for k in s2:
        assert torch.equal(s2[k], t2[k]), k
    for k in a2:
        assert torch.equal(a2[k], c2[k]), k
    # online: batch 2 sees batch 1's adaptation; reset_tta() restores A bit for bit and clears the moments
    _, _, mk_on = _small()
    o = mk_on()
    A0 = {k: v.clone() for k, v in o.state_dict().items() if k in set(T.adapted_keys(o))}
    o.test_step(b1, 0)
    r2 = o.test_step(b2, 1).clone()
    assert not torch.equal(r2, q2), "online batch 2 equals the episodic one: nothing carried over"
    o.reset_tta()
    for k, v in A0.items():
        assert torch.equal(o.state_dict()[k], v), k
    st = o._tent
    assert not bool(st.exp_avg.any()) and not bool(st.exp_avg_sq.any()) and not bool(st.steps.any())
    assert torch.equal(o.test_step(b2, 2), q2), "after reset_tta() the next batch starts from the source values and fresh moments"


def test_freeze_and_inference_mode():
    hp, sd, mk = _small()
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, 14)), T.to_dev(T.tta_batch(hp, 16, 15))
    a, c = mk(), mk()
    a.freeze()
    c.freeze()
    with torch.inference_mode():
        a.test_step(b1, 0)
        pa = a.test_step(b2, 1)
    c.test_step(b1, 0)
    pc = c.test_step(b2, 1)
    assert torch.equal(pa, pc)
    sa, sc = T.full_state(a), T.full_state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert all(not torch.equal(sa[k], v) for k, v in T.full_state(mk()).items() if k in set(T.adapted_keys(a)))
    assert not any(q.requires_grad for q in a.parameters()) and not any(q.requires_grad for q in c.parameters())
    # reset_tta() after freeze() and inside inference_mode restores A bit for bit
    src = {k: v for k, v in T.full_state(mk()).items() if k in set(T.adapted_keys(a))}
    with torch.inference_mode():
        a.reset_tta()
    for k, v in src.items():
        assert torch.equal(a.state_dict()[k], v), k


def test_fit_test_takes_the_adapting_path(tmp_path):
    from stil_tta_amd import fit
    hp, sd, mk = _small()
    loader = [T.tta_batch(hp, 16, 20 + i) for i in range(3)]
    ck = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": {k: v.clone() for k, v in sd.items()}}, ck)
    a = mk()
    a.test_step(T.to_dev(loader[0]), 0)          # adaptation state from an earlier run: the checkpoint load must discard it
    a.load_state_dict({k: v.cuda() for k, v in T.initial_state(hp, 77).items()})
    assert a._tent is None
    a.test_step(T.to_dev(loader[1]), 0)
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
    off = T.make_model(hp, sd, tta=True)
    fit.test(off, loader, ck)
    so = T.full_state(off)
    assert all(not torch.equal(so[k], sa[k]) for k in T.adapted_keys(a)), "fit.test with READ left A where the run without TTA leaves it"
