"""The launch choice of the public step API (driver.choose_launch / make_step) without a GPU: which per-GPU shapes replay a
captured hipGraph under launch="auto", and the refusals (several ranks, a model that cannot be captured)."""
import multiprocessing as mp
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_choose_launch_auto_eager_graph():
    from stil_tta_amd.driver import choose_launch
    assert choose_launch("auto", 16, 128, True, 1) == "graph"            # cardiac share of 16 samples per GPU: launch-bound
    assert choose_launch("auto", 256, 224, True, 1) == "eager"           # B = 256 at 224 px: GPU-bound
    assert choose_launch("auto", 32, 224, True, 1) == "eager"            # replays slower than it runs eagerly
    assert choose_launch("auto", 16, 128, True, 2) == "eager"            # several ranks: collectives are not captured
    assert choose_launch("auto", 16, 128, False, 1) == "eager"           # the model declares no capture_key / capture_state
    assert choose_launch("eager", 16, 128, True, 1) == "eager"
    assert choose_launch("graph", 256, 224, True, 1) == "graph"
    with pytest.raises(ValueError, match="one rank"):
        choose_launch("graph", 16, 128, True, 2)
    with pytest.raises(ValueError, match="capture_key"):
        choose_launch("graph", 16, 128, False, 1)
    with pytest.raises(ValueError, match="launch must be one of"):
        choose_launch("graphs", 16, 128, True, 1)


def test_batch_geometry_of_both_batch_layouts():
    from stil_tta_amd.driver import batch_geometry, synthetic_batch
    assert batch_geometry(synthetic_batch([3, 4, 1, 1], 5, 16, 64)) == (16, 64)
    im, tab = torch.zeros(2, 3, 96, 96), torch.zeros(2, 4)
    u = [(torch.zeros(14, 3, 96, 96), torch.zeros(14, 4)) for _ in range(3)]
    assert batch_geometry({"l": ((im, tab), torch.zeros(2), torch.arange(2)), "u": (u, torch.zeros(14))}) == (16, 96)


def test_models_declare_what_a_capture_bakes_in():
    from stil_tta_amd import STiLModel
    from stil_tta_amd.driver import is_capturable
    from stil_tta_amd.match import CoMatch
    from oracle import match_oracle as XO
    m = STiLModel(dict(model="resnet18", embedding_dim=512, field_lengths=[3, 4, 1], num_classes=5, start_epoch=1, batch_size=16))
    assert is_capturable(m) and not is_capturable(object())
    m.current_epoch = 1
    k1 = m.capture_key()
    m.current_epoch = 2
    assert m.capture_key() != k1                                         # the pseudo-label terms join the loss
    hp = XO.default_hparams(model="resnet18", embedding_dim=512, img_size=64, field_lengths=[3, 4, 1], num_classes=5, batch_size=16,
                            K=40, start_epoch=5)
    c = CoMatch(dict(vars(hp)))
    keys = []
    for e in (0, 1, 2):
        c.current_epoch = e
        keys.append(c.capture_key())
    assert len(set(keys)) == 3                                           # min(epoch + 1, lam_c) is a host constant of the loss


def _graph_at_world2(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from stil_tta_amd import STiLModel
    from stil_tta_amd.driver import init_distributed, make_step, synthetic_batch
    init_distributed(backend="gloo", timeout_s=60)
    m = STiLModel(dict(model="resnet18", embedding_dim=512, field_lengths=[3, 4, 1], num_classes=5, batch_size=16))
    batch = synthetic_batch([3, 4, 1], 5, 16, 64)
    msg = ""
    try:
        make_step(m, None, batch, launch="graph")
    except ValueError as e:
        msg = str(e)
    eager = make_step(m, None, batch, launch="auto").launch
    q.put((rank, (msg, eager)))
    dist.barrier()
    dist.destroy_process_group()


def test_make_step_graph_refuses_two_ranks_gloo():
    from test_product_cpu import _run_ranks
    res = _run_ranks(_graph_at_world2)
    for rank in (0, 1):
        msg, eager = res[rank]
        assert "one rank" in msg and "world size 2" in msg, msg
        assert eager == "eager"
