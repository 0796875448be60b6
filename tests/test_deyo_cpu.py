"""CPU side of DeYO test-time adaptation (tests/test_gpu_deyo.py): the hparams rules, the float64 references the GPU tests use
(the row contract, and the shuffle as a torch index gather against a plain loop), and the conditions on the GPU tests' inputs --
every selection decision is far from its threshold and fp32 ATen meets the GPU bars against float64 there, so a kernel or step
that misses them is wrong, not unlucky."""
import math
import os
import sys

import numpy as np
import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import test_gpu_deyo as D  # noqa: E402
import test_gpu_eata as E  # noqa: E402
import test_gpu_tta as T  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402


def _model(**over):
    from stil_tta_amd import STiLModel
    d = dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False)
    d.update(over)
    return STiLModel(d)


def test_deyo_keys_and_defaults():
    from stil_tta_amd import tta
    assert "deyo" in tta.METHODS
    m = _model(tta=True, tta_method="deyo")
    assert m._tta_on() and not _model(tta=False, tta_method="deyo")._tta_on()
    hp = m.hp
    assert (hp.tta_patch_grid, hp.tta_ent_margin, hp.tta_plpd_margin, hp.tta_reweight_ent, hp.tta_reweight_plpd, hp.tta_shuffle_seed) == \
        (4, None, 0.2, 1.0, 1.0, 2024)
    assert (hp.tta_e_margin, hp.tta_lr, hp.tta_episodic, hp.tta_params) == (None, 1e-3, False, "bn")
    assert len(m.tta_param_names()) == 106
    assert hp.img_size % hp.tta_patch_grid == 0


def test_check_hparams_accepts_and_rejects():
    import copy
    from stil_tta_amd import tta
    base = _model(tta=True, tta_method="deyo", tta_patch_grid=8, tta_ent_margin=2, tta_plpd_margin=-2.0, tta_reweight_ent=0.0, tta_shuffle_seed=0)
    assert (base.hp.tta_patch_grid, base.hp.tta_ent_margin, base.hp.tta_plpd_margin, base.hp.tta_reweight_ent, base.hp.tta_shuffle_seed) == (8, 2, -2.0, 0.0, 0)

    def check(method="deyo", **kw):
        hp = copy.copy(base.hp)
        hp.tta_method = method
        for k, v in kw.items():
            setattr(hp, k, v)
        tta.check_hparams(hp)
    for kw in (dict(tta_patch_grid=1), dict(tta_patch_grid=base.hp.img_size), dict(tta_ent_margin=0.0), dict(tta_ent_margin=None), dict(tta_plpd_margin=0),
               dict(tta_reweight_ent=0.0, tta_reweight_plpd=0), dict(tta_reweight_plpd=3.5), dict(tta_shuffle_seed=2 ** 40)):
        check(**kw)
    for method in ("deyo", "tent", None):               # the keys are checked whatever the method
        for kw in (dict(tta_patch_grid=0), dict(tta_patch_grid=-4), dict(tta_patch_grid=4.0), dict(tta_patch_grid=True), dict(tta_patch_grid="4"),
                   dict(tta_patch_grid=5), dict(tta_patch_grid=4, img_size=126),
                   dict(tta_ent_margin=float("nan")), dict(tta_ent_margin="1"), dict(tta_ent_margin=True),
                   dict(tta_plpd_margin=None), dict(tta_plpd_margin=float("inf")), dict(tta_plpd_margin="0.2"),
                   dict(tta_reweight_ent=-1.0), dict(tta_reweight_ent=float("inf")), dict(tta_reweight_ent=None), dict(tta_reweight_plpd=-0.5),
                   dict(tta_reweight_plpd=float("nan")), dict(tta_reweight_plpd=False),
                   dict(tta_shuffle_seed=-1), dict(tta_shuffle_seed=1.5), dict(tta_shuffle_seed=True), dict(tta_shuffle_seed=None)):
            with pytest.raises(ValueError):
                check(method, **kw)
    with pytest.raises(ValueError):
        check("DeYO")
    with pytest.raises(ValueError):                     # through the constructor too
        _model(tta=True, tta_method="deyo", tta_patch_grid=5)
    with pytest.raises(NotImplementedError):
        _model(tta=True, tta_method="deyo", tabular_encoder="saint")
    with pytest.raises(NotImplementedError):
        _model(tta_method="deyo", algorithm_name="STiL_SAINT")


def test_draw_perm_gives_permutations_and_follows_its_generator():
    from stil_tta_amd import tta
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    p1, p2 = tta.draw_perm(a, 6, 4), tta.draw_perm(a, 6, 4)
    assert p1.dtype == np.int32 and p1.shape == (6, 16)
    for p in (p1, p2):
        assert np.array_equal(np.sort(p, axis=1), np.tile(np.arange(16), (6, 1)))
    assert not np.array_equal(p1, p2) and len({tuple(r) for r in p1}) > 1
    assert np.array_equal(tta.draw_perm(b, 6, 4), p1)
    assert np.array_equal(tta.draw_perm(a, 3, 1), np.zeros((3, 1), dtype=np.int32))


@pytest.mark.parametrize("B,C,H,W,grid", D.SHUFFLE_CASES)
def test_the_gather_restatement_of_the_shuffle_is_the_plain_loop(B, C, H, W, grid):
    x, perm = D.shuffle_input(B, C, H, W, grid)
    assert all(sorted(r.tolist()) == list(range(grid * grid)) for r in perm)
    bad = perm.clone()
    bad[:, 0], bad[:, -1] = -1, grid * grid
    ph, pw = H // grid, W // grid
    for pm in (perm, bad):
        ref = torch.empty_like(x)
        for b in range(B):
            for s in range(grid * grid):
                q = int(pm[b, s])
                q = q if 0 <= q < grid * grid else s
                ref[b, :, (s // grid) * ph:(s // grid + 1) * ph, (s % grid) * pw:(s % grid + 1) * pw] = \
                    x[b, :, (q // grid) * ph:(q // grid + 1) * ph, (q % grid) * pw:(q % grid + 1) * pw]
        assert torch.equal(D.shuffle_ref(x, grid, pm), ref)
    # a permutation moves every value once: the sorted pixels of each channel are the source's
    out = D.shuffle_ref(x, grid, perm)
    assert torch.equal(out.flatten(2).sort(dim=2).values, x.flatten(2).sort(dim=2).values)
    # both kernel paths are covered: 16-byte pieces need pw % 4 == 0
    assert {(W // g) % 4 == 0 for _, _, _, W, g in D.SHUFFLE_CASES} == {True, False}


@pytest.mark.parametrize("rows,K,variant", D.deyo_cases())
def test_row_kernel_inputs_are_far_from_every_threshold_and_fp32_aten_meets_tol(rows, K, variant):
    """No row has |H - tau_ent| below 1e-3 (K == 1: H = 0 = tau_ent exactly, in every precision), no reliable row has
    |PLPD - tau_plpd| below 1e-3, no row's first maximum is within 1e-3 of another logit unless it is an exact tie; the variants
    hold what they are named for."""
    z, zs, tau_ent, tau_plpd, e0 = D.deyo_input(rows, K, variant)
    gs = 0.75
    r64 = D.deyo_ref(z, zs, tau_ent, tau_plpd, e0, D.A_ENT, D.A_PLPD, torch.float64, gs)
    r32 = D.deyo_ref(z, zs, tau_ent, tau_plpd, e0, D.A_ENT, D.A_PLPD, torch.float32, gs)
    if K == 1:
        assert tau_ent == 0.0 and bool((r64["H"] == 0).all()) and bool((r32["H"] == 0).all())
    else:
        assert float((r64["H"] - tau_ent).abs().min()) >= 1e-3
    if r64["n_rel"]:
        assert float((r64["plpd"] - tau_plpd).abs()[r64["rel"]].min()) >= 1e-3
    top = z.max(dim=1, keepdim=True).values
    near = ((z - top).abs() < 1e-3) & (z != top)
    assert not bool(near.any())
    assert bool((z.gather(1, r64["yhat"][:, None]) == top).all())
    if K == 1 or variant == "none_reliable":
        assert r64["n"] == 0 and r64["n_rel"] == 0
    elif variant == "plpd_fails":
        assert r64["n"] == 0 and r64["n_rel"] > 0
    elif variant == "tied":
        ties = (z == top).sum(dim=1)
        assert bool((ties[0::2] == min(K, 2)).all())
        if K > 2:                                      # the double peak is reliable and selected by its FIRST maximum only
            assert bool(r64["sel"][0::2].all()) and not bool(r64["sel"][1::2].any())
            second = torch.where(z == top, torch.arange(K)[None, :], -1).max(dim=1).values
            d2 = torch.softmax(z.double(), 1).gather(1, second[:, None])[:, 0] - torch.softmax(zs.double(), 1).gather(1, second[:, None])[:, 0]
            assert bool((d2[0::2] < tau_plpd - 1e-3).all()), "the other maximum would be selected too"
    elif rows >= 7:
        sel, rel = r64["sel"], r64["rel"]
        assert bool(sel.any()) and bool((~rel).any()) and bool((rel & ~sel).any())
    assert torch.equal(r32["sel"], r64["sel"]) and torch.equal(r32["rel"], r64["rel"]) and torch.equal(r32["yhat"], r64["yhat"])
    for k in ("lse", "probs", "H", "plpd", "w", "loss", "grad"):
        assert bool(torch.isfinite(r64[k]).all()), k
        a, b = (r[k].view(-1) if r[k].ndim == 0 else r[k] for r in (r32, r64))
        close(a, b, TOL, name=k)


def test_entropy_only_contract_is_eatas_with_an_invalid_mean():
    """The float64 references agree on what the GPU test asks of the kernels bit for bit."""
    for rows, K in ((7, 286), (512, 2)):
        z, zs, tau_ent, _, _ = D.deyo_input(rows, K, "mixed")
        d = D.deyo_ref(z, zs, tau_ent, -2.0, tau_ent, 1.0, 0.0, torch.float64, 0.75)
        e = E.eata_ref(z, tau_ent, E.D_MARGIN, E.MU, torch.zeros(K), 0, torch.float64, 0.75)
        assert torch.equal(d["sel"], e["sel"]) and d["n"] == e["n"] and d["n"] > 0
        close(d["loss"].view(1), e["loss"].view(1), 1e-12, name="loss")
        close(d["grad"], e["grad"], 1e-12, name="grad")


@pytest.mark.parametrize("case", D.PARITY, ids=[c[0] for c in D.PARITY])
def test_parity_batches_are_well_conditioned(case):
    """The step test's margins sit in gaps whose half-width is >= 100 x the fp32 restatement's error on H (resp. the PLPD of the
    reliable rows, the only ones it decides), the PLPD filter has both outcomes on the reliable rows, and the fp32 selection is
    the float64 one.  The online batches are reached by the fp32 restatement's own Adam steps (the GPU test reaches them by
    the device's); the permutations are those of a generator seeded as the model's."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from stil_tta_amd import STiLModel, tta
    label, mk_hp, B, which, seeds, sseed = case
    hp = mk_hp()
    lr = 1e-3
    sd = E.scaled_state(hp, sseed)
    d = dict(vars(hp))
    d.update(tta=True, tta_method="deyo", tta_params=which)
    keys = STiLModel(d).tta_param_names()
    rng = np.random.default_rng(D.SHUFFLE_SEED)
    opt = {}
    kw = dict(a_ent=D.A_ENT, a_plpd=D.A_PLPD)
    for step, seed in enumerate(seeds, start=1):
        x, _ = T.tta_batch(hp, B, seed)
        perm = tta.draw_perm(rng, B, D.GRID)
        pre = D.deyo_restated(sd, keys, x, perm, hp, torch.float64, **kw)
        r32 = D.deyo_restated(sd, keys, x, perm, hp, torch.float32, margins=pre["margins"], **kw)
        eH = float((r32["H"].double() - pre["H"]).abs().max())
        ed = float((r32["plpd"].double() - pre["plpd"]).abs()[pre["rel"]].max())
        print(f"[{label}] batch {step}: margins {pre['margins']}, half gaps H {pre['gaps']['H']:.3e} plpd {pre['gaps']['plpd']:.3e}; "
              f"fp32 error H {eH:.2e} plpd {ed:.2e}; reliable {int(pre['rel'].sum())} selected {pre['n']}/{B}; "
              f"plpd in [{float(pre['plpd'].min()):.3f}, {float(pre['plpd'].max()):.3f}]")
        assert pre["gaps"]["H"] >= 100 * eH, (pre["gaps"]["H"], eH)
        assert pre["gaps"]["plpd"] >= 100 * ed, (pre["gaps"]["plpd"], ed)
        assert bool((pre["rel"] & ~pre["sel"]).any()) and bool(pre["sel"].any()), "the PLPD filter has one outcome only on the reliable rows"
        assert torch.equal(r32["sel"], pre["sel"]) and torch.equal(r32["rel"], pre["rel"]) and torch.equal(r32["yhat"], pre["yhat"])
        if step < len(seeds):
            O.adam_step(sd, r32["g"], opt, step, lr)
