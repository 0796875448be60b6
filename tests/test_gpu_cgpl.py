"""CGPL test-time adaptation in STiLModel.test_step: STiL's own unlabelled-data branch (consensus-guided pseudo-labels over the
three classifier heads, prototype-guided label smoothing, one soft cross-entropy per head; models/Disentangle/STiLModel.py:255-303
with use_ema False, restated in oracle/stil_oracle.py's training_step) run on the test batch, on top of TENT (tests/test_gpu_tta.py).

1. stil_cgpl_rows against float64 autograd (close() at TOL of test_gpu_ops), ld = K + 3 views, sentinels, repetition; lse3[0] and p
   are stil_entropy_rows' bits; flags, counts and gate exact; p = NULL, each dZ = NULL, rate = 1 with feat = NULL.
2. Bad arguments are refused with nothing written.
3. The step against the method restated here in float64 on the oracle, on the device's ReLU / max-pool decisions and coins; the
   device's cases and mask1 are float64's own.  Also under tta_bn_prior and under tta_bn_momentum.
4. No weight-gradient product; first-batch logits and scores are tent's; a threshold of 1 moves nothing; a rate of 1 never runs
   the projector; the coins; episodic mode, reset_tta(), freeze() + torch.inference_mode(), fit.test.
tests/test_cgpl_cpu.py checks on the CPU that the inputs used here are well-conditioned (fp32 ATen and the fp32 oracle meet the same
bars, every decision is unambiguous) and pins the restatement below to oracle.stil_oracle.training_step."""
import contextlib
import ctypes
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_gpu_ops import close  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
from oracle import make_golden as MG  # noqa: E402
import test_gpu_tta as T  # noqa: E402

SENTINEL = -7.25
ROWS = (1, 7, 512)
KS = (1, 2, 3, 286, 1000, 5000)
KINDS = ("agree", "mi", "mt", "none", "cycle", "near_th", "tied")
RATES = (1.0, 0.8)
TEMP = 0.1
ACTIVE = (1, 0, 1, 1, 0)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------ the method, restated
def first_max(x):
    """the first maximum of every row (torch.argmax promises no order among ties)"""
    K = x.shape[1]
    idx = torch.arange(K).expand_as(x)
    return torch.where(x == x.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, K)).min(dim=1).values


def cgpl_terms(zm, zi, zt, feat, protos, coin, rate, T, th):
    """csrc/stil_cgpl.h restated in the dtype of the logits: the pseudo-label and every decision carry no gradient.
    -> dict(loss, losses [m, i, t], ce [3 x rows], logp, q, q0, pred, conf, mask1, case (1..4), w [3 x rows bool], tops)"""
    logp = [torch.log_softmax(z, dim=1) for z in (zm, zi, zt)]
    with torch.no_grad():
        a, b, d = tops = [first_max(z) for z in (zm, zi, zt)]
        c1 = (a == b) & (a == d)
        c2 = (a == b) & (a != d)
        c3 = (a == d) & (a != b)
        c4 = ~(c1 | c2 | c3)
        mean = torch.where(c1[:, None], (zm + zi + zt) / 3.0, torch.where(c2[:, None], (zm + zi) / 2.0, torch.where(c3[:, None], (zm + zt) / 2.0, zm)))
        q0 = torch.softmax(mean, dim=1)
        pm = logp[0].exp()
        if rate < 1.0:
            tp = torch.softmax(feat @ protos.t() / T, dim=1)
            q, pred = rate * q0 + (1.0 - rate) * tp, rate * pm + (1.0 - rate) * tp
        else:
            q, pred = q0, pm
        conf = pred.max(dim=1).values
        mask1 = conf >= th
        heads_or_tails = coin.bool()
        w = [mask1 & c1, mask1 & (c1 | c3 | (c4 & heads_or_tails)), mask1 & (c1 | c2 | (c4 & ~heads_or_tails))]
    ce = [-(q * lp).sum(dim=1) for lp in logp]
    rows = zm.shape[0]
    losses = [(c * wh.to(c.dtype)).sum() / rows for c, wh in zip(ce, w)]
    return dict(loss=losses[0] + losses[1] + losses[2], losses=losses, ce=ce, logp=logp, q=q, q0=q0, pred=pred, conf=conf, mask1=mask1,
                case=(1 * c1 + 2 * c2 + 3 * c3 + 4 * c4), w=w, tops=tops)


def cgpl_ref(inp, dtype):
    """The loss of the inputs `inp` (cgpl_input) with autograd in `dtype`, at the float32 rate, T and th the kernel receives.
    -> dict(lse3 [3, rows], p, q, conf, ce3 [3, rows], dz [3 x (rows, K)], out [4], flags [rows, 4], counts [5], case, mask1, tops)"""
    zs = [inp[k].detach().to(dtype).clone().requires_grad_(True) for k in ("zm", "zi", "zt")]
    t = cgpl_terms(*zs, inp["feat"].to(dtype), inp["protos"].to(dtype), inp["coin"], inp["rate"], inp["T"], inp["th"])
    dz = torch.autograd.grad(t["loss"], zs)
    rows = zs[0].shape[0]
    flags = torch.stack((t["case"], t["mask1"].long(), t["mask1"].long(), torch.zeros(rows, dtype=torch.long)), dim=1).to(torch.uint8)
    counts = torch.tensor([int(t["mask1"].sum())] + [int((t["case"] == c).sum()) for c in (1, 2, 3, 4)], dtype=torch.int32)
    return dict(lse3=torch.stack([torch.logsumexp(z.detach(), dim=1) for z in zs]), p=t["logp"][0].exp().detach(), q=t["q"],
                conf=t["conf"], ce3=torch.stack([c.detach() for c in t["ce"]]), dz=list(dz),
                out=torch.stack([t["loss"].detach()] + [x.detach() for x in t["losses"]]), flags=flags, counts=counts, case=t["case"],
                mask1=t["mask1"], tops=t["tops"])


# ------------------------------------------------------------------------------------------ check 1: the entry point
def cgpl_cases():
    return [(r, k, kind, rate) for r in ROWS for k in KS for kind in KINDS for rate in RATES]


def _place_threshold(conf):
    """a threshold in the widest gap of the middle half of the sorted confidences (as oracle/make_golden.py's build_case places
    th1); with one row, or rows that all share one confidence, half the smallest: every row is kept"""
    c = conf.double().sort().values
    n = c.numel()
    lo = n // 4
    if n >= 4:
        gaps = c[lo + 1: n - lo + 1] - c[lo: n - lo]
        if gaps.numel() and float(gaps.max()) > 1e-6 * float(c.max()):
            j = int(gaps.argmax()) + lo
            return float((c[j] + c[j + 1]) / 2)
    return 0.5 * float(c.min())


@functools.lru_cache(maxsize=None)
def cgpl_input(rows, K, kind, rate):
    """The inputs of one case (read-only): float32 logits zm, zi, zt [rows, K], feat [rows, Dp] and protos [K, Dp] (unit rows), one
    coin per row, and rate, T, th as the float32 values the kernel receives.
    Every kind but `tied`: logits uniform in +-1 with one logit raised by 4 per head, so each head has one clear top class.
      agree / mi / mt / none: the three tops coincide / multimodal = imaging / multimodal = tabular / the multimodal top stands alone;
      cycle: the four of them in turn over the rows.  (K = 1 is case 1 throughout.)
      near_th: all three heads share zm = one logit above K - 1 zeros and every prototype is the same vector (tp uniform), placed so
               that conf sweeps from 0.5 th to 1.5 th over the rows (clamped into (1 / K, 1); a row that would land on th itself is
               moved to 1.005 th).
      tied: every logit 3.5: every top is class 0.
    th: near_th fixes it (0.4; K = 2: 0.7); otherwise it lies in the widest gap of the middle half of the float64 confidences."""
    g = torch.Generator().manual_seed(7919 * rows + 13 * K + 101 * KINDS.index(kind) + int(10 * rate))
    Dp = 70 if K <= 3 else 19
    rate32, T32 = f32(rate), f32(TEMP)
    feat = F.normalize(torch.randn(rows, Dp, generator=g, dtype=torch.float64), dim=1).float()
    protos = F.normalize(torch.randn(K, Dp, generator=g, dtype=torch.float64), dim=1).float()
    coin = (torch.rand(rows, generator=g) >= 0.5).to(torch.uint8)
    r = torch.arange(rows)
    th = None
    if kind == "tied":
        zm = zi = zt = torch.full((rows, K), 3.5, dtype=torch.float32)
    elif kind == "near_th":
        th = f32(0.7 if K == 2 else 0.4)
        protos = protos[:1].expand(K, Dp).contiguous()
        z = torch.zeros(rows, K, dtype=torch.float64)
        if K > 1:
            s = torch.linspace(0.5, 1.5, rows, dtype=torch.float64)
            s = torch.where((s - 1.0).abs() < 0.005, torch.full_like(s, 1.005), s)
            c = ((th * s - (1.0 - rate32) / K) / rate32).clamp(1.0 / K + 0.02 * (1.0 - 1.0 / K), 0.98)   # softmax(zm)'s largest entry
            z[r, (7 * r) % K] = torch.log(c * (K - 1) / (1.0 - c))
        zm = zi = zt = z.float()
    else:
        which = {"agree": 1, "mi": 2, "mt": 3, "none": 4}.get(kind)
        case = torch.full((rows,), which) if which else (r % 4) + 1
        top_m = (7 * r) % K
        other = (top_m + 1 + (3 * r) % max(K - 1, 1)) % K     # != top_m whenever K > 1
        top_i = torch.where((case == 1) | (case == 2), top_m, other)
        top_t = torch.where((case == 1) | (case == 3), top_m, other)
        zm, zi, zt = ((torch.rand(rows, K, generator=g, dtype=torch.float64) * 2.0 - 1.0) for _ in range(3))
        for z, top in ((zm, top_m), (zi, top_i), (zt, top_t)):
            z[r, top] += 4.0
        zm, zi, zt = zm.float(), zi.float(), zt.float()
    inp = dict(zm=zm, zi=zi, zt=zt, feat=feat, protos=protos, coin=coin, rate=rate32, T=T32, th=0.0)
    if th is None:
        th = f32(_place_threshold(cgpl_ref(inp, torch.float64)["conf"]))
    inp["th"] = th
    return inp


@functools.lru_cache(maxsize=None)
def cgpl_ref64(rows, K, kind, rate):
    """the float64 reference of one case, computed once (read-only)"""
    return cgpl_ref(cgpl_input(rows, K, kind, rate), torch.float64)


def _padded(z, pad, fill=SENTINEL):
    rows, K = z.shape
    zb = torch.full((rows + 1, K + pad), fill, dtype=torch.float32)
    zb[:rows, :K] = z
    return zb.cuda()


def _fresh(rows, K, ld, smooth):
    dev = "cuda"
    return dict(lse3=torch.full((3 * rows + 1,), SENTINEL, dtype=torch.float64, device=dev), p=torch.full((rows + 1, ld), SENTINEL, device=dev),
                q=torch.full((rows + 1, ld), SENTINEL, device=dev), conf=torch.full((rows + 1,), SENTINEL, device=dev),
                flags=torch.full((rows + 1, 4), 77, dtype=torch.uint8, device=dev), ce3=torch.full((3 * rows + 1,), SENTINEL, device=dev),
                dzm=torch.full((rows + 1, ld), SENTINEL, device=dev), dzi=torch.full((rows + 1, ld), SENTINEL, device=dev),
                dzt=torch.full((rows + 1, ld), SENTINEL, device=dev), counts=torch.full((6,), -7, dtype=torch.int32, device=dev),
                out=torch.full((5,), SENTINEL, device=dev), gate=torch.full((len(ACTIVE) + 1,), 77, dtype=torch.uint8, device=dev),
                ws=torch.full(((rows * K if smooth else 0) + 1,), SENTINEL, dtype=torch.float64, device=dev))   # not cleared: written before it is read


def _run_cgpl(L, d, rows, K, ld, gs, null=()):
    """one call on the device inputs d (padded logits, feat, protos, coin, active, and the float32 scalars); `null`: outputs (or
    "feat": feat, protos and ws) passed as NULL"""
    smooth = d["rate"] < 1.0
    o = _fresh(rows, K, ld, smooth)
    q = {k: (None if k in null else v.data_ptr()) for k, v in o.items()}
    nofeat = "feat" in null
    L.cgpl_rows(d["zm"].data_ptr(), d["zi"].data_ptr(), d["zt"].data_ptr(), ld, None if nofeat else d["feat"].data_ptr(),
                None if nofeat else d["protos"].data_ptr(), d["coin"].data_ptr(), rows, K, d["feat"].shape[1], d["T"], d["rate"], d["th"], gs,
                q["lse3"], q["p"], q["q"], ld, q["conf"], q["flags"], q["ce3"], q["dzm"], q["dzi"], q["dzt"], ld, q["counts"], q["out"],
                d["active"].data_ptr(), q["gate"], len(ACTIVE), None if (nofeat or not smooth) else q["ws"], None)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _run_entropy(L, zb, ld, rows, K, gs):
    lse = torch.empty(rows, dtype=torch.float64, device="cuda")
    p, dZ = torch.empty(rows, ld, device="cuda"), torch.empty(rows, ld, device="cuda")
    H, mean = torch.empty(rows, device="cuda"), torch.empty(1, device="cuda")
    L.entropy_rows(zb.data_ptr(), ld, rows, K, gs, lse.data_ptr(), p.data_ptr(), ld, H.data_ptr(), dZ.data_ptr(), ld, mean.data_ptr(), None)
    torch.cuda.synchronize()
    return dict(lse=lse.cpu(), p=p.cpu()[:, :K])


@pytest.mark.parametrize("rows,K,kind,rate", cgpl_cases())
def test_cgpl_rows_against_float64(rows, K, kind, rate):
    from stil_tta_amd._lib import lib
    L = lib()
    inp = cgpl_input(rows, K, kind, rate)
    ref = cgpl_ref64(rows, K, kind, rate)
    gs = f32(1.0 / rows)
    smooth = inp["rate"] < 1.0
    active = torch.tensor(ACTIVE, dtype=torch.uint8)
    for pad in (0, 3):
        ld = K + pad
        d = dict(inp, zm=_padded(inp["zm"], pad), zi=_padded(inp["zi"], pad), zt=_padded(inp["zt"], pad), feat=inp["feat"].cuda(),
                 protos=inp["protos"].cuda(), coin=inp["coin"].cuda(), active=active.cuda())
        a, b = (_run_cgpl(L, d, rows, K, ld, gs) for _ in range(2))
        for k in a:
            if k != "ws":
                assert torch.equal(a[k], b[k]), f"{k}: not bit-identical on repetition"
        # sentinels: padding columns, the row past the end, the element past every vector
        for k in ("p", "q", "dzm", "dzi", "dzt"):
            assert bool((a[k][rows] == SENTINEL).all()), k
            if pad:
                assert bool((a[k][:, K:] == SENTINEL).all()), k
        assert float(a["lse3"][3 * rows]) == SENTINEL and float(a["ce3"][3 * rows]) == SENTINEL and float(a["conf"][rows]) == SENTINEL
        assert bool((a["flags"][rows] == 77).all()) and int(a["counts"][5]) == -7 and float(a["out"][4]) == SENTINEL
        assert int(a["gate"][len(ACTIVE)]) == 77 and float(a["ws"][-1]) == SENTINEL
        # decisions are exact
        assert torch.equal(a["flags"][:rows], ref["flags"]), "flags"
        assert torch.equal(a["counts"][:5], ref["counts"]), (a["counts"], ref["counts"])
        assert torch.equal(a["gate"][:len(ACTIVE)], active * int(int(ref["counts"][0]) > 0)), "gate"
        if kind == "tied" or K == 1:
            assert bool((a["flags"][:rows, 0] == 1).all())
        close(a["lse3"][:3 * rows].view(3, rows), ref["lse3"], name="lse3")
        close(a["p"][:rows, :K], ref["p"], name="p")
        close(a["q"][:rows, :K], ref["q"], name="q")
        close(a["conf"][:rows], ref["conf"], name="conf")
        close(a["ce3"][:3 * rows].view(3, rows), ref["ce3"], name="ce3")
        for k, g in zip(("dzm", "dzi", "dzt"), ref["dz"]):
            close(a[k][:rows, :K], g * (gs * rows), name=k)   # grad_scale as the float32 the kernel receives
        close(a["out"][:4], ref["out"], name="out")
        # lse3[0] and p are stil_entropy_rows' on Zm, bit for bit
        t = _run_entropy(L, d["zm"], ld, rows, K, gs)
        assert torch.equal(a["lse3"][:rows], t["lse"]) and torch.equal(a["p"][:rows, :K], t["p"])
    # a NULL optional output (and, at rate 1, NULL feat, protos and ws) leaves the others as they are: on the ld = K + 3 view
    for null in (("p",), ("dzm",), ("dzi",), ("dzt",), ("p", "dzm", "dzi", "dzt")) + ((("feat",),) if not smooth else ()):
        c = _run_cgpl(L, d, rows, K, ld, gs, null=null)
        for k in a:
            if k in null:
                assert bool((c[k] == SENTINEL).all()), (null, k)
            elif k != "ws":
                assert torch.equal(c[k], a[k]), (null, k)


# ------------------------------------------------------------------------------------------ check 2: bad arguments
def test_cgpl_rows_rejects_bad_arguments_with_nothing_written():
    from stil_tta_amd._lib import lib
    fn = lib()._dll.stil_cgpl_rows
    rows, K, Dp = 4, 8, 5
    ins = dict(zm=torch.zeros(rows, K, device="cuda"), zi=torch.zeros(rows, K, device="cuda"), zt=torch.zeros(rows, K, device="cuda"),
               feat=torch.zeros(rows, Dp, device="cuda"), protos=torch.zeros(K, Dp, device="cuda"),
               coin=torch.zeros(rows, dtype=torch.uint8, device="cuda"), active=torch.ones(3, dtype=torch.uint8, device="cuda"))
    fill = dict(flags=77, gate=77, counts=-7)

    def fresh():
        o = _fresh(rows - 1, K, K, True)    # one row more than rows - 1: exactly the shapes of the call
        o["lse3"], o["ce3"] = o["lse3"].new_full((3 * rows,), SENTINEL), o["ce3"].new_full((3 * rows,), SENTINEL)
        o["ws"], o["gate"] = o["ws"].new_full((rows * K,), SENTINEL), o["gate"].new_full((3,), 77)
        return o

    def call(o, ld=K, rows=rows, K=K, Dp=Dp, ldp=K, ldd=K, T=0.1, rate=0.8, nt=3, null=()):
        q = {k: (None if k in null else v.data_ptr()) for k, v in {**ins, **o}.items()}
        c32 = ctypes.c_float
        return fn(q["zm"], q["zi"], q["zt"], ld, q["feat"], q["protos"], q["coin"], rows, K, Dp, c32(T), c32(rate), c32(0.1), c32(0.25),
                  q["lse3"], q["p"], q["q"], ldp, q["conf"], q["flags"], q["ce3"], q["dzm"], q["dzi"], q["dzt"], ldd, q["counts"], q["out"],
                  q["active"], q["gate"], nt, q["ws"], None)

    def untouched(o):
        torch.cuda.synchronize()
        return all(bool((v == fill.get(k, SENTINEL)).all()) for k, v in o.items())

    bad = [dict(null=(k,)) for k in ("zm", "zi", "zt", "coin", "lse3", "q", "conf", "flags", "ce3", "counts", "out", "active", "gate")]
    bad += [dict(null=(k,)) for k in ("feat", "protos", "ws")]                        # rate < 1 needs all three
    bad += [dict(rows=0), dict(rows=-1), dict(K=0), dict(K=-3), dict(Dp=0), dict(Dp=-1), dict(ld=K - 1), dict(ldp=K - 1), dict(ldd=K - 1)]
    bad += [dict(rate=v) for v in (-0.1, 1.0000001, 2.0, float("inf"), float("-inf"), float("nan"))]
    bad += [dict(T=v) for v in (0.0, -0.1, float("inf"), float("nan"))]
    bad += [dict(nt=-1), dict(rate=1.0, Dp=0)]
    for kw in bad:
        o = fresh()
        assert call(o, **kw) < 0, kw
        assert untouched(o), f"{kw}: refused, yet something was written"
    good = [dict(), dict(null=("p",)), dict(null=("dzm",)), dict(null=("dzi", "dzt")), dict(null=("dzm", "dzi", "dzt"), ldd=0), dict(rate=0.0),
            dict(rate=1.0, null=("feat", "protos", "ws")), dict(rate=1.0, T=0.0), dict(nt=0, null=("active", "gate"))]
    for kw in good:
        o = fresh()
        assert call(o, **kw) == 0, kw
        torch.cuda.synchronize()
        assert bool((o["out"][:4] != SENTINEL).all()) and bool((o["counts"][:5] != -7).all())


# ------------------------------------------------------------------------------------------ check 3: the step, restated
def cgpl_restated(sd, keys, x, hp, dtype, coin, rate, th, decisions=None):
    """The method on one batch, on a deep copy of the state (the oracle updates running statistics in place): all ten outputs of
    O.backbone_forward_all(train=True, masks=None), the normalised multimodal projection of cat(e_si, e_c, e_st) without gradient,
    cgpl_terms with the state's prototypes and temperature, autograd w.r.t. A.
    -> dict(p, g {key: gradient}, flips, terms (cgpl_terms' dict, detached), out_m, out_i, out_t)"""
    s = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k in keys:
        s[k].requires_grad_(True)
    ctx = O.force_decisions(*decisions) if decisions is not None else contextlib.nullcontext()
    with ctx as d:
        zm, zi, zt, si_e, _, _, st_e, _, _, xc = O.backbone_forward_all(s, "model.", x[0].to(dtype), x[1].to(dtype), hp, train=True, masks=None)
        with torch.no_grad():
            feat = F.normalize(O._head(s, "projector_multimodal.", torch.cat((si_e, xc, st_e), dim=1)))
        t = cgpl_terms(zm, zi, zt, feat, s["prototypes"], coin, rate, hp.temperature, th)
        g = torch.autograd.grad(t["loss"], [s[k] for k in keys], allow_unused=True) if keys else ()
    flips = {tag: v for tag, v in d.get("flips", {}).items() if v[0]} if d is not None else {}
    g = {k: (torch.zeros_like(s[k]) if u is None else u.detach()) for k, u in zip(keys, g)}
    terms = {k: ([u.detach() for u in v] if isinstance(v, list) else v.detach()) for k, v in t.items()}
    return dict(p=terms["logp"][0].exp(), g=g, flips=flips, terms=terms, out_m=zm.detach(), out_i=zi.detach(), out_t=zt.detach())


@functools.lru_cache(maxsize=None)
def step_case(name, sseed, bseed):
    """One step case (read-only): the shapes of oracle/make_golden.py's case `name` (64 px, B = 16), a randomised state with unit
    random prototypes, the three heads coupled by craft_heads and their biases re-centred on the student's own train-mode logits of
    the batch `bseed` (use_ema False: craft_heads then centres on the student), and tta_pl_threshold in the widest gap of the middle
    half of the sorted float64 confidences.  -> (hp, state, B, threshold)"""
    over, B, epoch, _, _ = MG.CASES[name]
    hp = O.default_hparams(**over)
    sd = MG.randomize_state(O.init_state(hp, seed=sseed), seed=sseed + 1)
    g = torch.Generator().manual_seed(7)
    sd["prototypes"] = F.normalize(torch.randn(hp.num_classes, hp.projection_dim, generator=g))
    student = O.default_hparams(**{**over, "use_ema": False})
    batch = O.synthetic_batch(hp, B, seed=bseed)
    sd = MG.craft_heads(sd, batch, student, epoch, torch.zeros(B - max(B // 8, 1), dtype=torch.bool))
    x, _ = T.tta_batch(hp, B, bseed)
    conf = cgpl_restated(sd, [], x, hp, torch.float64, torch.zeros(B, dtype=torch.uint8), hp.rate_pseudo, 0.0)["terms"]["conf"]
    return hp, sd, B, _place_threshold(conf)


# (label, make_golden case, tta_params, batch seeds (online), state seed).  The batch seeds are chosen so that the conditions of
# tests/test_cgpl_cpu.py hold: build_case's own batch (seed 2022) has a row whose two largest imaging logits lie within 30 fp32
# errors of each other
STEP = [
    ("dvm64_b16_bn_online", "dvm_r50_pseudo", "bn", (2032, 2033), 1234),
    ("dvm64_b16_norm", "dvm_r50_pseudo", "norm", (2032,), 1234),
    ("cardiac64_b16_bn", "cardiac_r50", "bn", (2032,), 1234),
]
STEP_LR = 1e-3


def cgpl_model(hp, sd, th, **tta):
    kw = dict(tta=True, tta_method="cgpl", tta_pl_threshold=th)
    kw.update(tta)
    return T.make_model(hp, sd, **kw)


def check_steps(label, m, hp, B, seeds, lr, oracle=None):
    """The device's steps on the batches `seeds` against the float64 restatement.  Bars are TENT's (tests/test_gpu_tta.py):
    predictions <= 3e-5 scaled, each gradient of A <= 3 e32 + 1e-4, Adam within 2.2 lr step, everything outside A bit-identical;
    the restatement takes the device's coins, and the device's cases and mask1 must be float64's own.
    oracle(m, state before the batch) -> a factory of context managers under which the oracle's BatchNorm follows the device's rule.
    -> [per batch: dict(terms of float64, grads of the device, worst margins)]"""
    import test_gpu_step as S
    from stil_tta_amd import tta
    keys = T.adapted_keys(m)
    rate, th = tta.cgpl_rate(m.hp), tta.cgpl_threshold(m.hp)
    opt, bad, seen = {}, [], []
    for step, seed in enumerate(seeds, start=1):
        x, y = T.tta_batch(hp, B, seed)
        before = T.full_state(m)
        sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
        scope = oracle(m, sd_before) if oracle is not None else contextlib.nullcontext
        with S._trace_decisions() as trace:
            m.test_step(T.to_dev((x, y)), step - 1)
            torch.cuda.synchronize()
            decisions = S._device_decisions(m, trace)
        lt = m.last_tta
        coin = lt["coin"].cpu()
        with scope():
            r64 = cgpl_restated(sd_before, keys, x, hp, torch.float64, coin, rate, th, decisions)
        with scope():
            r64free = cgpl_restated(sd_before, keys, x, hp, torch.float64, coin, rate, th)
        with scope():
            r32 = cgpl_restated(sd_before, keys, x, hp, torch.float32, coin, rate, th)
        S._check_flips(r64["flips"])
        t64 = r64["terms"]
        flags = lt["flags"].cpu()
        assert torch.equal(flags[:, 0].long(), t64["case"]), f"[{label}] batch {step}: the device's cases are not float64's"
        assert torch.equal(flags[:, 1].bool(), t64["mask1"]), f"[{label}] batch {step}: the device's mask1 is not float64's"
        n = int(t64["mask1"].sum())
        assert torch.equal(lt["counts"].cpu(), torch.tensor([n] + [int((t64["case"] == c).sum()) for c in (1, 2, 3, 4)], dtype=torch.int32))
        d = S._scaled(lt["probs"].cpu().double().numpy(), r64["p"].numpy())
        print(f"[{label}] batch {step}: predictions scaled error {d:.2e}; cases {lt['counts'].cpu().tolist()[1:]}, n = {n}; "
              f"flips {({tag: v[0] for tag, v in r64['flips'].items()})}")
        if d > 3e-5:
            bad.append((step, "predictions", d))
        # the three heads' logits, by the rule of test_gpu_step._fwd_check: the crafted, batch-centred heads carry large cancelling
        # terms, and the fp32 oracle's own logits lie up to 6e-5 (scaled) from float64 here, so a logit that misses 3e-5 must be as
        # close to float64 as the fp32 oracle is (3 e32 + 1e-5) and inside 1e-4
        for k, o in (("y_hat_m", "out_m"), ("y_hat_i", "out_i"), ("y_hat_t", "out_t")):
            e = S._scaled(lt[k].cpu().double().numpy(), r64[o].numpy())
            e32 = S._scaled(r32[o].double().numpy(), r64free[o].numpy())
            if e > 3e-5 and not (e <= 1e-4 and e <= 3 * e32 + 1e-5):
                bad.append((step, k, e, e32))
        close(lt["pseudo_label"], t64["q"], name="pseudo_label")
        close(lt["conf"], t64["conf"], name="conf")
        close(lt["loss"].view(1), t64["loss"].view(1), name="loss")
        for k, v in zip(("loss_m", "loss_i", "loss_t"), t64["losses"]):
            close(lt[k].view(1), v.view(1), name=k)
        close(lt["probs"], torch.softmax(lt["y_hat_m"].double(), dim=1), name="probs against softmax(y_hat_m)")
        gd = T.device_grads(m)
        ratios = []
        for k in keys:
            e32 = T._rel(r32["g"][k].double(), r64free["g"][k])
            err = T._rel(gd[k], r64["g"][k])
            ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
            if err > 3 * e32 + 1e-4:
                bad.append((step, "grad " + k, err, e32))
        print(f"[{label}] batch {step}: gradient error / (3*e32 + 1e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
        sd32 = {k: v.clone() for k, v in sd_before.items()}
        if n > 0:
            O.adam_step(sd32, r32["g"], opt, step, lr)    # fp32 oracle, its own moments, from the same parameters
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
        print(f"[{label}] batch {step}: predictions / 3e-5 = {d / 3e-5:.3f}; worst gradient ratio {max(r[0] for r in ratios):.3f}; "
              f"Adam deviation / (2.2 lr step) {worst_adam:.3f}")
        seen.append(dict(terms=t64, grads=gd, n=n))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"
    return seen


@pytest.mark.parametrize("case", STEP, ids=[c[0] for c in STEP])
def test_cgpl_step_matches_the_method_restated_in_float64(case):
    label, name, which, seeds, sseed = case
    hp, sd, B, th = step_case(name, sseed, seeds[0])
    m = cgpl_model(hp, sd, th, tta_params=which, tta_lr=STEP_LR)
    m.freeze()
    keys = T.adapted_keys(m)
    assert len(keys) == (106 if which == "bn" else 106 + 2 * (1 + 4 * 2) + 2 * 2)
    seen = check_steps(label, m, hp, B, seeds, STEP_LR)
    first = seen[0]
    assert first["n"] > 0 and any(not torch.equal(m.state_dict()[k].cpu(), sd[k]) for k in keys), "the step adapted nothing"
    if which == "norm":
        # a row whose tabular head disagrees with the other two (case 2_i) and passes the threshold teaches the tabular head: its
        # gradient reaches the tabular encoder's LayerNorm affines through out_t
        t = first["terms"]
        assert bool(((t["case"] == 2) & t["mask1"]).any()), "no selected case-2_i row on this batch"
        tab = [k for k in keys if k.startswith("model.encoder_tabular.")]
        assert len(tab) == 2 * (1 + 4 * 2)
        for k in tab:
            assert float(first["grads"][k].abs().max()) > 0, f"{k}: no gradient reached the tabular encoder"


def _threshold_under(scope, hp, sd, B, seed):
    """step_case's threshold again, for a BatchNorm rule that moves the confidences: the widest gap of the middle half of the float64
    confidences of the batch under the oracle scope `scope`"""
    x, _ = T.tta_batch(hp, B, seed)
    with scope():
        conf = cgpl_restated(sd, [], x, hp, torch.float64, torch.zeros(B, dtype=torch.uint8), hp.rate_pseudo, 0.0)["terms"]["conf"]
    return _place_threshold(conf)


def test_cgpl_step_under_a_batchnorm_prior_matches_the_restatement():
    from test_gpu_bnprior import blended_oracle
    label, name, which, seeds, sseed = STEP[0]
    hp, sd, B, _ = step_case(name, sseed, seeds[0])
    N = 16.0
    th = _threshold_under(lambda: blended_oracle(N, B), hp, sd, B, seeds[0])
    m = cgpl_model(hp, sd, th, tta_lr=STEP_LR, tta_bn_prior=N)
    m.freeze()
    seen = check_steps("prior_n16", m, hp, B, seeds[:1], STEP_LR, oracle=lambda m_, sd_: (lambda: blended_oracle(N, B)))
    assert 0 < seen[0]["n"] < B


def test_cgpl_step_on_the_batchnorm_memory_matches_the_restatement():
    from test_gpu_bnmemory import memory_oracle, memory_of
    label, name, which, seeds, sseed = STEP[0]
    hp, sd, B, _ = step_case(name, sseed, seeds[0])
    alpha = 0.05
    m = cgpl_model(hp, sd, 0.0, tta_lr=STEP_LR, tta_bn_momentum=alpha)
    m.freeze()

    def oracle(m_, sd_before):
        mem = memory_of(m_, sd_before)
        return lambda: memory_oracle(mem, alpha, alpha)

    m.hp.tta_pl_threshold = _threshold_under(oracle(m, sd), hp, sd, B, seeds[0])
    seen = check_steps("memory_a0.05", m, hp, B, seeds[:1], STEP_LR, oracle=oracle)
    assert 0 < seen[0]["n"] < B and m._bn_mem.t == 1


# ------------------------------------------------------------------------------------------ check 4: properties
def _small(**tta):
    label, name, which, seeds, sseed = STEP[0]
    hp, sd, B, th = step_case(name, sseed, seeds[0])
    return hp, sd, seeds[0], (lambda **more: cgpl_model(hp, sd, th, **{**tta, **more}))


@pytest.mark.parametrize("which", ["bn", "norm"])
def test_cgpl_step_issues_no_weight_gradient_product(which, monkeypatch):
    from stil_tta_amd._lib import lib
    hp, sd, seed, mk = _small(tta_params=which)
    m = mk()
    L = lib()
    calls = []
    for name in ("wgrad_tn", "wgrad_tn_partial", "cgpl_rows", "cgpl_pgls", "ce_soft_fwd"):
        if "stil_" + name not in L.protos:
            continue
        orig = getattr(L, name)
        monkeypatch.setitem(L.__dict__, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    A0 = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    m.test_step(T.to_dev(T.tta_batch(hp, 16, seed)), 0)
    torch.cuda.synchronize()
    assert calls == ["cgpl_rows"], f"a step makes one loss call and no weight-gradient product: {calls}"
    assert any(not torch.equal(m.state_dict()[k], v) for k, v in A0.items()), "the step adapted nothing"


def test_first_batch_logits_and_scores_are_tents():
    hp, sd, seed, mk = _small()
    b = T.to_dev(T.tta_batch(hp, 16, seed))
    a, t = mk(), T.make_model(hp, sd, tta=True, tta_method="tent")
    pa, pt = a.test_step(b, 0), t.test_step(b, 0)
    torch.cuda.synchronize()
    assert torch.equal(a.last_tta["y_hat_m"], t.last_tta["y_hat_m"]) and torch.equal(a.last_tta["probs"], t.last_tta["probs"])
    assert torch.equal(pa, pt) and torch.equal(a.last_tta["probs"], pa)
    assert set(a.last_tta) == {"loss", "loss_m", "loss_i", "loss_t", "y_hat_m", "y_hat_i", "y_hat_t", "probs", "pseudo_label", "conf", "flags",
                               "coin", "counts"}
    assert all(v.is_cuda for v in a.last_tta.values())
    assert not torch.equal(a.test_step(b, 1), t.test_step(b, 1)), "the second batch shows the same adaptation as tent's"


def _adapt_state(m):
    st = m._tent
    out = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    out.update({"#tta_exp_avg": st.exp_avg.clone(), "#tta_exp_avg_sq": st.exp_avg_sq.clone(), "#tta_steps": st.steps.clone()})
    return out


def test_a_threshold_of_one_selects_nothing_and_moves_nothing():
    hp, sd, seed, mk = _small()
    b = T.to_dev(T.tta_batch(hp, 16, seed))
    m = mk(tta_pl_threshold=1.0)
    m.setup_device()
    src = {k: v.clone() for k, v in m.state_dict().items()}
    m.test_step(b, 0)
    torch.cuda.synchronize()
    lt = m.last_tta
    assert int(lt["counts"][0]) == 0 and int(lt["counts"][1:].sum()) == 16 and not bool(lt["flags"][:, 1].any())
    assert float(lt["loss"]) == 0.0 and float(lt["loss_m"]) == 0.0 and float(lt["loss_i"]) == 0.0 and float(lt["loss_t"]) == 0.0
    st = m._tent
    assert not bool(st.gate.any()) and not bool(st.grads.any())
    assert not bool(st.exp_avg.any()) and not bool(st.exp_avg_sq.any()) and not bool(st.steps.any())
    for k, v in m.state_dict().items():
        assert torch.equal(v, src[k]), k
    # the same model at its own threshold does move
    w = mk()
    w.test_step(b, 0)
    assert int(w.last_tta["counts"][0]) > 0 and bool(w._tent.steps.any()) and torch.equal(w._tent.gate, w._tent.active)


def test_a_rate_of_one_never_runs_the_projector(monkeypatch):
    hp, sd, seed, mk = _small()
    b = T.to_dev(T.tta_batch(hp, 16, seed))
    calls = []
    for rate, want in ((None, 1), (1.0, 0), (0.0, 1)):
        m = mk(tta_pl_rate=rate)
        orig = m.project_3features
        monkeypatch.setattr(m, "project_3features", lambda *a, _o=orig, **k: (calls.append(rate), _o(*a, **k))[1])
        m.test_step(b, 0)
        torch.cuda.synchronize()
        assert calls.count(rate) == want, (rate, calls)
        assert bool(torch.isfinite(m.last_tta["loss"]))
    # rate 1: the pseudo-label is the consensus softmax alone, the confidence the multimodal one
    lt = m.last_tta   # rate 0.0: the prototype classifier alone
    one = mk(tta_pl_rate=1.0)
    one.test_step(b, 0)
    l1 = one.last_tta
    assert torch.equal(l1["conf"], l1["probs"].max(dim=1).values)
    assert not torch.equal(l1["pseudo_label"], lt["pseudo_label"])


def test_the_same_seed_gives_the_same_coins():
    hp, sd, seed, mk = _small()
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, seed)), T.to_dev(T.tta_batch(hp, 16, seed + 1))

    def coins(m, n=3):
        out = []
        for i in range(n):
            m.test_step(b1 if i % 2 == 0 else b2, i)
            out.append(m.last_tta["coin"].clone())
        return out

    a, c, other = coins(mk()), coins(mk()), coins(mk(tta_pl_seed=7))
    assert all(torch.equal(u, v) for u, v in zip(a, c))
    assert a[0].dtype == torch.uint8 and tuple(a[0].shape) == (16,) and bool((a[0] <= 1).all())
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2]), "every batch draws fresh coins"
    assert not torch.equal(a[0], other[0])
    assert 0 < int(torch.stack(a).sum()) < 48
    # the counter runs on through reset_tta() and episodes; a new state restarts it
    m = mk(tta_episodic=True)
    e = coins(m, 2)
    assert torch.equal(e[0], a[0]) and torch.equal(e[1], a[1])
    m.reset_tta()
    m.test_step(b1, 2)
    assert torch.equal(m.last_tta["coin"], a[2])
    m.load_state_dict({k: v.cuda() for k, v in sd.items()})
    assert m._tent is None
    m.test_step(b1, 0)
    assert torch.equal(m.last_tta["coin"], a[0])


def test_episodic_mode_and_reset():
    hp, sd, seed, mk = _small(tta_episodic=True)
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, seed)), T.to_dev(T.tta_batch(hp, 16, seed + 1))
    m = mk()
    m.test_step(b1, 0)
    m.test_step(b2, 1)
    p3 = m.test_step(b1, 2).clone()
    f = mk()
    q3 = f.test_step(b1, 0).clone()
    assert torch.equal(p3, q3), "an episode starts from the source values whatever came before"
    # the coins differ between the two (third draw against first), so A after the update may differ; everything outside A may not
    s3, t3 = T.full_state(m), T.full_state(f)
    aset = set(T.adapted_keys(m))
    for k in s3:
        if k not in aset:
            assert torch.equal(s3[k], t3[k]), k
    assert torch.equal(m._tent.steps, f._tent.steps)
    # online: batch 2 sees batch 1's adaptation; reset_tta() restores A bit for bit and clears the moments
    _, _, _, mk_on = _small()
    o = mk_on()
    A0 = {k: v.clone() for k, v in o.state_dict().items() if k in aset}
    o.test_step(b1, 0)
    r2 = o.test_step(b1, 1).clone()
    assert not torch.equal(r2, q3), "the online second batch equals the episodic one: nothing carried over"
    o.reset_tta()
    for k, v in A0.items():
        assert torch.equal(o.state_dict()[k], v), k
    st = o._tent
    assert not bool(st.exp_avg.any()) and not bool(st.exp_avg_sq.any()) and not bool(st.steps.any())
    assert int(st.coin_step) == 2
    assert torch.equal(o.test_step(b1, 2), q3), "after reset_tta() the next batch starts from the source values and fresh moments"


def test_freeze_and_inference_mode():
    hp, sd, seed, mk = _small()
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, seed)), T.to_dev(T.tta_batch(hp, 16, seed + 1))
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
    for k, v in _adapt_state(a).items():
        assert torch.equal(v, _adapt_state(c)[k]), k
    assert any(not torch.equal(sa[k], v) for k, v in T.full_state(mk()).items() if k in set(T.adapted_keys(a)))
    assert not any(q.requires_grad for q in a.parameters()) and not any(q.requires_grad for q in c.parameters())
    # reset_tta() after freeze() and inside inference_mode restores A bit for bit
    src = {k: v for k, v in T.full_state(mk()).items() if k in set(T.adapted_keys(a))}
    with torch.inference_mode():
        a.reset_tta()
    for k, v in src.items():
        assert torch.equal(a.state_dict()[k], v), k


def test_fit_test_takes_the_adapting_path(tmp_path):
    from stil_tta_amd import fit
    hp, sd, seed, mk = _small()
    loader = [T.tta_batch(hp, 16, seed + i) for i in range(3)]
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
    assert any(not torch.equal(so[k], sa[k]) for k in T.adapted_keys(a)), "fit.test with cgpl left A where the run without TTA leaves it"
