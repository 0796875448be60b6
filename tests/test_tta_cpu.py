"""CPU side of test-time adaptation (TENT in STiLModel.test_step, tests/test_gpu_tta.py): the hparams rules, the adapted set,
and the conditions on the inputs the GPU tests use -- fp32 ATen meets the GPU bars against float64 there, so a kernel or step
that misses them is wrong, not unlucky."""
import json
import os
import sys

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import test_gpu_tta as T  # noqa: E402
from test_gpu_ops import TOL, close  # noqa: E402

GOLD = os.path.join(TESTS, "golden")


def _model(**over):
    from stil_tta_amd import STiLModel
    d = dict(field_lengths=[10, 20, 30, 40] + [1] * 13, use_ema=False)
    d.update(over)
    return STiLModel(d)


def test_shipped_config_leaves_adaptation_off():
    from stil_tta_amd.stil_model import _as_namespace
    with open(os.path.join(GOLD, "hparams_config_dvm_STiL.json")) as f:
        hp = _as_namespace(json.load(f)["hparams"])
    assert hp.tta is True and hp.tta_method is None
    assert (hp.tta_lr, hp.tta_episodic, hp.tta_params) == (1e-3, False, "bn")
    m = _model(**{k: v for k, v in vars(hp).items() if k in ("tta", "num_classes", "img_size", "model")})
    assert not m._tta_on()
    assert _model(tta=True, tta_method="tent")._tta_on()
    assert not _model(tta=False, tta_method="tent")._tta_on()


def test_unknown_method_or_params_and_saint_are_refused():
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="memo")
    with pytest.raises(ValueError):
        _model(tta=True, tta_method="tent", tta_params="all")
    with pytest.raises(NotImplementedError):
        _model(tta=True, tta_method="tent", tabular_encoder="saint")
    with pytest.raises(NotImplementedError):
        _model(tta_method="tent", algorithm_name="STiL_SAINT")


def test_adapted_set_names():
    m = _model(tta=True, tta_method="tent")
    bn = m.tta_param_names()
    assert len(bn) == 106 and len(set(bn)) == 106
    bns = {n for n, mod in m.model.encoder_imaging.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)}
    assert len(bns) == 53 and any("downsample" in n for n in bns)
    assert set(bn) == {f"model.encoder_imaging.{n}.{w}" for n in bns for w in ("weight", "bias")}
    sd = m.state_dict()
    assert all(n in sd for n in bn)
    norm = _model(tta=True, tta_method="tent", tta_params="norm").tta_param_names()
    lns = [f"model.encoder_tabular.norm.{w}" for w in ("weight", "bias")]
    for i in range(4):
        lns += [f"model.encoder_tabular.transformer_blocks.{i}.norm{j}.{w}" for j in (1, 2) for w in ("weight", "bias")]
    lns += [f"model.transformer.0.norm{j}.{w}" for j in (1, 2) for w in ("weight", "bias")]
    assert norm[:106] == bn and sorted(norm[106:]) == sorted(lns)


@pytest.mark.parametrize("rows,K,kind", T.entropy_cases())
def test_fp32_aten_entropy_meets_tol(rows, K, kind):
    z = T.entropy_input(rows, K, kind)
    r64, r32 = T.entropy_ref(z, torch.float64), T.entropy_ref(z, torch.float32)
    for k in ("loss", "grad", "probs"):
        assert bool(torch.isfinite(r64[k]).all()), k
        close(r32[k].view(-1) if k == "loss" else r32[k], r64[k].view(-1) if k == "loss" else r64[k], TOL, name=k)


@pytest.mark.parametrize("case", T.PARITY, ids=[c[0] for c in T.PARITY])
def test_fp32_oracle_tta_predictions_meet_the_bar(case):
    """The parity test's predictions bar (_scaled <= 3e-5 against float64) is reachable: the fp32 oracle meets it on the
    initial state of every case and every batch seed."""
    from test_gpu_step import _scaled
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    label, mk_hp, B, which, seeds, sseed = case
    hp = mk_hp()
    sd = T.initial_state(hp, sseed)
    keys = [k for k in sd if k.startswith("model.encoder_imaging.") and (k.endswith(".weight") or k.endswith(".bias"))
            and k.replace("weight", "running_var").replace("bias", "running_var") in sd][:2]
    for seed in seeds:
        x, _ = T.tta_batch(hp, B, seed)
        p32, _, _ = T.tent_restated(sd, keys, x, hp, torch.float32)
        p64, _, _ = T.tent_restated(sd, keys, x, hp, torch.float64)
        d = _scaled(p32.numpy(), p64.numpy())
        print(f"[{label}] seed {seed}: fp32 oracle predictions scaled error {d:.2e}")
        assert d <= 3e-5
