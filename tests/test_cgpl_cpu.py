"""CPU side of CGPL test-time adaptation (tests/test_gpu_cgpl.py): the hparams rules; the restatement of csrc/stil_cgpl.h pinned to
oracle.stil_oracle.training_step (itself pinned against the reference); its closed-form gradient against float64 autograd; and the
conditions on the inputs the GPU tests use -- fp32 ATen and the fp32 oracle meet the GPU bars against float64 there and every
decision (the three tops, conf against th) is unambiguous, so a kernel or step that misses them is wrong, not unlucky."""
import os
import sys

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import test_gpu_cgpl as G  # noqa: E402
import test_gpu_tta as T  # noqa: E402
from oracle import make_golden as MG  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402

EPS32 = float(torch.finfo(torch.float32).eps)


def _model(**over):
    from stil_tta_amd import STiLModel
    d = dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False)
    d.update(over)
    return STiLModel(d)


def _cgpl(**over):
    return _model(**{**dict(tta=True, tta_method="cgpl"), **over})


# ------------------------------------------------------------------------------------------ keys, defaults, refusals
def test_cgpl_keys_and_defaults():
    from stil_tta_amd import tta
    m = _cgpl()
    assert m._tta_on() and not _cgpl(tta=False)._tta_on()
    hp = m.hp
    assert (hp.tta_pl_threshold, hp.tta_pl_rate, hp.tta_pl_seed) == (None, None, 2025)
    assert (hp.tta_lr, hp.tta_episodic, hp.tta_params, hp.tta_bn_prior, hp.tta_bn_momentum) == (1e-3, False, "bn", None, None)
    d = _model().hp
    assert (d.tta_pl_threshold, d.tta_pl_rate, d.tta_pl_seed) == (None, None, 2025)
    assert tta.cgpl_threshold(hp) == hp.th1 and tta.cgpl_rate(hp) == hp.rate_pseudo
    o = _cgpl(tta_pl_threshold=0.3, tta_pl_rate=1, tta_pl_seed=0, th1=0.7, rate_pseudo=0.5).hp
    assert tta.cgpl_threshold(o) == 0.3 and tta.cgpl_rate(o) == 1.0 and o.tta_pl_seed == 0
    p = _cgpl(th1=0.7, rate_pseudo=0.5).hp
    assert tta.cgpl_threshold(p) == 0.7 and tta.cgpl_rate(p) == 0.5
    assert _cgpl(tta_pl_rate=0).hp.tta_pl_rate == 0 and _cgpl(tta_pl_threshold=0).hp.tta_pl_threshold == 0
    assert m._tent is None and m.last_tta == {}


def test_cgpl_is_a_registered_method_and_the_adapted_sets_are_tents():
    from stil_tta_amd import tta
    assert "cgpl" in tta.METHODS and tta.STEPS["cgpl"] is tta.cgpl_step and callable(tta.cgpl_loss)
    assert tta.PARAMS == ("bn", "norm", "fusion")
    assert issubclass(tta.CgplState, tta.TentState)
    for which in ("bn", "norm"):
        assert _cgpl(tta_params=which).tta_param_names() == _model(tta=True, tta_method="tent", tta_params=which).tta_param_names()
    assert len(_cgpl().tta_param_names()) == 106


def test_cgpl_composes_with_the_batchnorm_prior_the_memory_and_da():
    assert _cgpl(tta_bn_prior=16).hp.tta_bn_prior == 16 and _cgpl(tta_bn_momentum=0.05).hp.tta_bn_momentum == 0.05
    assert _cgpl(tta_bn_prior=16, tta_bn_momentum=0.05, tta_episodic=True)._tta_on()
    assert _cgpl(DA=True)._tta_on()     # not applied at test time, and not refused


def test_fusion_and_saint_stay_refused():
    with pytest.raises(ValueError, match="read"):
        _cgpl(tta_params="fusion")
    with pytest.raises(ValueError):
        _cgpl(tta_params="all")
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="CGPL")
    with pytest.raises(NotImplementedError):
        _cgpl(tabular_encoder="saint")
    with pytest.raises(NotImplementedError):
        _model(tta_method="cgpl", algorithm_name="STiL_SAINT")


def test_bad_pseudo_label_keys_are_refused_whatever_the_method():
    for method in (None, "tent", "cgpl"):
        for bad in (-0.1, float("inf"), float("nan"), "0.5", True, False):
            with pytest.raises(ValueError, match="tta_pl_threshold"):
                _model(tta=True, tta_method=method, tta_pl_threshold=bad)
        for bad in (-0.1, 1.0000001, 2, float("inf"), float("nan"), "0.5", True, False):
            with pytest.raises(ValueError, match="tta_pl_rate"):
                _model(tta=True, tta_method=method, tta_pl_rate=bad)
        for bad in (-1, 1.5, True, None, "7"):
            with pytest.raises(ValueError, match="tta_pl_seed"):
                _model(tta=True, tta_method=method, tta_pl_seed=bad)
        ok = _model(tta=True, tta_method=method, tta_pl_threshold=2.0, tta_pl_rate=0.25, tta_pl_seed=2 ** 40).hp
        assert (ok.tta_pl_threshold, ok.tta_pl_rate, ok.tta_pl_seed) == (2.0, 0.25, 2 ** 40)


# ------------------------------------------------------------------------------------------ pinned to the oracle
def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


@pytest.mark.parametrize("name", ["dvm_r50_pseudo", "cardiac_r50"])
def test_the_restatement_reproduces_the_oracles_training_step(name):
    """On cat(l, u) of a synthetic batch with use_ema False (the pseudo-labels come from the student's own detached outputs), DA False,
    current_epoch > start_epoch and an injected mask_random: cgpl_terms on the oracle's float64 logits, projection and prototypes of
    the rows [B_l:] reproduces pseudo_label, pseudo_label_orig, the cases, mask1 and the three unlabelled losses of
    O.training_step to 1e-12 relative, decisions exactly."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    over, B, epoch, _, _ = MG.CASES[name]
    hp = O.default_hparams(**{**over, "use_ema": False, "DA": False})
    assert epoch > hp.start_epoch and not hp.use_ema and not hp.DA
    sd = MG.randomize_state(O.init_state(hp, seed=1234), seed=99)
    g = torch.Generator().manual_seed(7)
    sd["prototypes"] = torch.nn.functional.normalize(torch.randn(hp.num_classes, hp.projection_dim, generator=g))
    batch = O.synthetic_batch(hp, B, seed=2022)
    B_l = len(batch["l"][2])
    B_u = B - B_l
    mr = torch.rand(B_u, generator=torch.Generator().manual_seed(11)).ge(0.5)
    sd = MG.craft_heads(sd, batch, hp, epoch, mr)
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    b64 = {k: ([v[0][0].double(), v[0][1].double()], [v[1][0].double(), v[1][1].double()], v[2], v[3], v[4]) for k, v in batch.items()}
    with torch.no_grad():
        pre = O.training_step({k: v.clone() for k, v in sd64.items()}, b64, hp, epoch, mr, None)
        hp.th1 = G._place_threshold(pre["prediction"].max(dim=1).values)    # `prediction` does not depend on th1: a mixed mask1
        o = O.training_step({k: v.clone() for k, v in sd64.items()}, b64, hp, epoch, mr, None)
    assert o["y_hat_m"].dtype == torch.float64 and o["pseudo_label"].dtype == torch.float64
    t = G.cgpl_terms(o["y_hat_m"][B_l:], o["y_hat_i"][B_l:], o["y_hat_t"][B_l:], o["feat_m"][B_l:], sd64["prototypes"], mr, hp.rate_pseudo,
                     hp.temperature, hp.th1)
    for c, key in ((1, "case1"), (2, "case2_i"), (3, "case2_t"), (4, "case3")):
        assert torch.equal(t["case"] == c, o[key]), key
    assert torch.equal(t["mask1"], o["mask1"])
    present = [int((t["case"] == c).sum()) for c in (1, 2, 3, 4)]
    print(f"[{name}] cases {present}, mask1 {int(t['mask1'].sum())} of {B_u}")
    assert sum(1 for n in present if n) >= 3 and 0 < int(t["mask1"].sum()) < B_u, "the pin is vacuous on this batch"
    worst = {"pseudo_label": _rel(t["q"], o["pseudo_label"]), "pseudo_label_orig": _rel(t["q0"], o["pseudo_label_orig"]),
             "prediction": _rel(t["pred"], o["prediction"])}
    for k, v in zip(("loss_m_u", "loss_i_u", "loss_t_u"), t["losses"]):
        assert float(o[k]) > 0, k
        worst[k] = abs(float(v) - float(o[k])) / abs(float(o[k]))
    print(f"[{name}] relative differences: {worst}")
    assert all(v <= 1e-12 for v in worst.values()), worst
    # the whole-model restatement the GPU tests use makes the oracle's forward on the same rows
    x = [torch.cat((batch["l"][0][1], batch["u"][0][1])), torch.cat((batch["l"][1][1], batch["u"][1][1]))]
    r = G.cgpl_restated(sd, [], x, hp, torch.float64, torch.zeros(B, dtype=torch.uint8), hp.rate_pseudo, hp.th1)
    assert torch.equal(r["out_m"], o["y_hat_m"]) and torch.equal(r["out_i"], o["y_hat_i"]) and torch.equal(r["out_t"], o["y_hat_t"])
    assert _rel(r["terms"]["q"][B_l:], o["pseudo_label"]) <= 1e-12 and torch.equal(r["terms"]["mask1"][B_l:], o["mask1"])


# ------------------------------------------------------------------------------------------ the closed form
@pytest.mark.parametrize("rows,K", [(5, 2), (7, 3), (8, 13)])
@pytest.mark.parametrize("rate", [1.0, 0.8, 0.0])
def test_closed_form_gradient_is_float64_autograd(rows, K, rate):
    """dZ_h of csrc/stil_cgpl.h, restated in float64, is the autograd gradient of grad_scale rows out[0] with q held constant, on
    rows that show all four cases and both sides of the threshold."""
    inp = G.cgpl_input(rows, K, "cycle", rate)
    ref = G.cgpl_ref(inp, torch.float64)
    assert sorted(set(ref["case"].tolist())) == [1, 2, 3, 4]
    assert 0 < int(ref["mask1"].sum()) < rows
    gs = 0.37
    zs = [inp[k].double() for k in ("zm", "zi", "zt")]
    t = G.cgpl_terms(*zs, inp["feat"].double(), inp["protos"].double(), inp["coin"], inp["rate"], inp["T"], inp["th"])
    for h in range(3):
        dz = gs * t["w"][h][:, None].double() * (torch.softmax(zs[h], dim=1) - t["q"])
        want = ref["dz"][h] * gs * rows
        assert float((dz - want).abs().max()) <= 1e-13 * (1.0 + float(want.abs().max())), h
        assert bool((want.abs().sum(dim=1) > 0).equal(t["w"][h])), "exactly the rows of w_h carry a gradient"
    assert any(bool(w.any()) for w in t["w"])
    assert abs(float(sum(t["losses"])) - float(ref["out"][0])) <= 1e-14
    if rate == 1.0:
        assert torch.equal(t["q"], t["q0"]) and torch.equal(t["conf"], t["logp"][0].exp().max(dim=1).values)


# ------------------------------------------------------------------------------------------ reachability of the kernel bar
@pytest.mark.parametrize("rows,K,kind,rate", G.cgpl_cases())
def test_fp32_aten_cgpl_meets_tol_on_well_posed_inputs(rows, K, kind, rate):
    """fp32 ATen meets every bar of test_cgpl_rows_against_float64 on its inputs with the same decisions, and in float64 every
    |conf - th| and every top-1 gap is at least 100 times the row's fp32 error."""
    inp = G.cgpl_input(rows, K, kind, rate)
    r64 = G.cgpl_ref64(rows, K, kind, rate)
    r32 = G.cgpl_ref(inp, torch.float32)
    # the kinds are what they say
    case = r64["case"]
    want = {"agree": {1}, "mi": {2}, "mt": {3}, "none": {4}, "tied": {1}, "near_th": {1}}.get(kind)
    if K == 1:
        want = {1}
    if want is not None:
        assert set(case.tolist()) == want, (kind, set(case.tolist()))
    elif rows >= 4:
        assert set(case.tolist()) == {1, 2, 3, 4}
    if kind == "tied":
        assert all(bool((t == 0).all()) for t in r64["tops"])
    if kind == "near_th" and K > 1 and rows >= 7:
        assert 4 * int(r64["mask1"].sum()) >= rows and 4 * int((~r64["mask1"]).sum()) >= rows
    if kind not in ("near_th", "tied") and K > 1 and rows >= 7:
        assert 0 < int(r64["mask1"].sum()) < rows
    # decisions: unambiguous in float64, and fp32's own
    conf_err = torch.maximum((r32["conf"].double() - r64["conf"]).abs(), EPS32 * r64["conf"])   # at least one rounding of conf itself
    margin = float(((r64["conf"] - inp["th"]).abs() / conf_err).min())
    assert margin >= 100.0, f"|conf - th| is only {margin:.1f} times the fp32 error"
    if kind != "tied" and K > 1:
        for z in (inp["zm"], inp["zi"], inp["zt"]):
            top2 = z.double().topk(2, dim=1).values
            gap = top2[:, 0] - top2[:, 1]
            assert float((gap / (EPS32 * z.double().abs().max(dim=1).values.clamp_min(1.0))).min()) >= 100.0
    assert torch.equal(r32["flags"], r64["flags"]) and torch.equal(r32["counts"], r64["counts"])
    assert all(torch.equal(a, b) for a, b in zip(r32["tops"], r64["tops"]))
    worst = 0.0
    for k in ("lse3", "p", "q", "conf", "ce3", "out"):
        assert bool(torch.isfinite(r64[k]).all()), k
        close(r32[k], r64[k], TOL, name=k)
    for h in range(3):
        a, b = r32["dz"][h].double(), r64["dz"][h]
        worst = max(worst, float(((a - b).abs() / (TOL * (1.0 + b.abs() + float(b.abs().max())))).max()))
        close(a, b, TOL, name=f"dz[{h}]")
    print(f"rows {rows} K {K} {kind} rate {rate}: |conf - th| / fp32 error {margin:.2e}; fp32 dZ error / bar {worst:.3f}")


# ------------------------------------------------------------------------------------------ reachability of the step bars
@pytest.mark.parametrize("case", G.STEP, ids=[c[0] for c in G.STEP])
def test_step_cases_are_well_posed_and_the_fp32_oracle_meets_the_bars(case):
    """On every batch of every step case, on the float64 oracle: the device's bars are reachable (the fp32 restatement's predictions
    are within _scaled <= 3e-5 of float64) and no decision is a near-tie (the gap between the two largest logits of every head and row,
    and every |conf - th|, is at least 100 times the fp32 oracle's error there).  On the batch the case is built on: DVM shows each of
    the four cases, cardiac at least three, and mask1 holds between a quarter and three quarters of the rows.  The online batches are
    reached by the fp32 oracle's own Adam steps (the GPU test reaches them by the device's)."""
    from test_gpu_step import _scaled
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    label, name, which, seeds, sseed = case
    hp, sd, B, th = G.step_case(name, sseed, seeds[0])
    sd = {k: v.clone() for k, v in sd.items()}
    keys = _cgpl(**{**vars(hp), "tta_params": which}).tta_param_names()
    rate = hp.rate_pseudo
    coin = torch.zeros(B, dtype=torch.uint8)
    opt = {}
    for step, seed in enumerate(seeds, start=1):
        x, _ = T.tta_batch(hp, B, seed)
        last = step == len(seeds)
        r32 = G.cgpl_restated(sd, [] if last else keys, x, hp, torch.float32, coin, rate, th)
        r64 = G.cgpl_restated(sd, [], x, hp, torch.float64, coin, rate, th)
        t32, t64 = r32["terms"], r64["terms"]
        d = _scaled(r32["p"].double().numpy(), r64["p"].numpy())
        ratios = []
        for k in ("out_m", "out_i", "out_t"):
            top2 = r64[k].topk(2, dim=1).values
            err = (r32[k].double() - r64[k]).abs().max(dim=1).values.clamp_min(1e-300)
            ratios.append(float(((top2[:, 0] - top2[:, 1]) / err).min()))
        cerr = (t32["conf"].double() - t64["conf"]).abs().clamp_min(1e-300)
        cratio = float(((t64["conf"] - th).abs() / cerr).min())
        present = [int((t64["case"] == c).sum()) for c in (1, 2, 3, 4)]
        n = int(t64["mask1"].sum())
        print(f"[{label}] batch {step}: cases {present}, mask1 {n} of {B} at th {th:.4f} (conf {float(t64['conf'].min()):.3f} .. "
              f"{float(t64['conf'].max()):.3f}); fp32 oracle predictions scaled error {d:.2e}; smallest top-1 gap / logit error per head "
              f"{[f'{r:.1e}' for r in ratios]}; smallest |conf - th| / error {cratio:.1e}")
        assert d <= 3e-5
        assert min(ratios) >= 100.0 and cratio >= 100.0
        assert torch.equal(t32["case"], t64["case"]) and torch.equal(t32["mask1"], t64["mask1"])
        if step == 1:
            assert sum(1 for c in present if c) >= (4 if hp.num_classes > 2 else 3), present
            assert B <= 4 * n <= 3 * B, n
            if which == "norm":
                assert bool(((t64["case"] == 2) & t64["mask1"]).any()), "the norm case needs a selected case-2_i row"
        if not last and n > 0:
            O.adam_step(sd, r32["g"], opt, step, G.STEP_LR)


def test_the_two_composed_cases_are_well_posed():
    """The smoke cases under tta_bn_prior = 16 and under tta_bn_momentum = 0.05 (first batch: the memory is the checkpoint's
    statistics), each at the threshold the GPU test places for it: mask1 is mixed and every decision is at least 100 fp32-oracle
    errors wide."""
    from test_gpu_bnmemory import memory_oracle
    from test_gpu_bnprior import blended_oracle
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    label, name, which, seeds, sseed = G.STEP[0]
    hp, sd, B, _ = G.step_case(name, sseed, seeds[0])
    mem = {k[:-len(".running_mean")]: (sd[k].double(), sd[k.replace("running_mean", "running_var")].double())
           for k in sd if k.startswith("model.encoder_imaging.") and k.endswith("running_mean")}
    coin = torch.zeros(B, dtype=torch.uint8)
    x, _ = T.tta_batch(hp, B, seeds[0])
    for what, scope in (("prior", lambda: blended_oracle(16.0, B)), ("memory", lambda: memory_oracle(mem, 0.05, 0.05))):
        th = G._threshold_under(scope, hp, sd, B, seeds[0])
        with scope():
            r32 = G.cgpl_restated(sd, [], x, hp, torch.float32, coin, hp.rate_pseudo, th)
            r64 = G.cgpl_restated(sd, [], x, hp, torch.float64, coin, hp.rate_pseudo, th)
        ratios = []
        for k in ("out_m", "out_i", "out_t"):
            top2 = r64[k].topk(2, dim=1).values
            err = (r32[k].double() - r64[k]).abs().max(dim=1).values.clamp_min(1e-300)
            ratios.append(float(((top2[:, 0] - top2[:, 1]) / err).min()))
        t32, t64 = r32["terms"], r64["terms"]
        cratio = float(((t64["conf"] - th).abs() / (t32["conf"].double() - t64["conf"]).abs().clamp_min(1e-300)).min())
        n = int(t64["mask1"].sum())
        print(f"[{what}] th {th:.4f}: mask1 {n} of {B}; smallest top-1 gap / logit error per head {[f'{r:.1e}' for r in ratios]}; "
              f"smallest |conf - th| / error {cratio:.1e}")
        assert 0 < n < B and min(ratios) >= 100.0 and cratio >= 100.0
        assert torch.equal(t32["case"], t64["case"]) and torch.equal(t32["mask1"], t64["mask1"])
