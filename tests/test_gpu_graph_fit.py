"""fit(launch="graph") against fit(launch="eager"): two epochs under the cosine scheduler (a new learning rate, so a re-capture,
every epoch), a ragged last batch (run eagerly between replays), validation and a best checkpoint -- the same run, bit for bit."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_fit import _Val, _data, _model  # noqa: E402


class _Ragged:
    """DataLoader(drop_last=False) stand-in: the last batch is shorter."""

    def __init__(self, img, tab, y, bs, labelled):
        self.img, self.tab, self.y, self.bs, self.lab = img, tab, y, bs, labelled

    def __len__(self):
        return (len(self.y) + self.bs - 1) // self.bs

    def __iter__(self):
        for i in range(len(self)):
            s = slice(i * self.bs, min((i + 1) * self.bs, len(self.y)))
            n = s.stop - s.start
            yield ([torch.zeros(n), self.img[s]], [self.tab[s], self.tab[s]], self.y[s], self.img[s], torch.full((n,), self.lab, dtype=torch.bool))


def _run(tmp, launch):
    from stil_tta_amd import fit as F
    li, lt, ly = _data(8, 1)
    ui, ut, uy = _data(56, 2)
    vi, vt, vy = _data(40, 3)
    loaders = {"l": _Ragged(li, lt, ly, 2, True), "u": _Ragged(ui, ut, uy, 15, False)}   # 4 steps; the 4th has 11 unlabelled samples
    m = _model(scheduler="cosine", dataset_length=4)
    m.setup_device("cuda")
    m.prototypes.copy_(torch.nn.functional.normalize(torch.randn(3, 128, generator=torch.Generator().manual_seed(5))).cuda())
    out = F.fit(m, loaders, _Val(vi, vt, vy, 16), max_epochs=2, eval_metric="acc", logdir=str(tmp), verbose=False, launch=launch)
    return m, out


def test_fit_graph_equals_fit_eager(tmp_path):
    me, oe = _run(tmp_path / "eager", "eager")
    mg, og = _run(tmp_path / "graph", "graph")
    assert oe["launch"] == "eager" and og["launch"] == "graph"
    for k in ("best_score", "best_epoch", "lr_by_epoch", "callback_metrics", "global_step", "epochs_run"):
        assert oe[k] == og[k], (k, oe[k], og[k])
    assert oe["lr_by_epoch"][0] != oe["lr_by_epoch"][1]
    for k in me.logged:                       # train losses of the last step, the epoch's train accuracy / AUROC
        assert torch.equal(torch.as_tensor(me.logged[k]), torch.as_tensor(mg.logged[k])), k
    assert "eval.train.auc" in mg.logged
    ce = torch.load(oe["checkpoint"], map_location="cpu", weights_only=False)
    cg = torch.load(og["checkpoint"], map_location="cpu", weights_only=False)
    assert ce["epoch"] == cg["epoch"] and ce["global_step"] == cg["global_step"]
    for k in ce["state_dict"]:
        assert torch.equal(ce["state_dict"][k], cg["state_dict"][k]), k
    se, sg = ce["optimizer_states"][0], cg["optimizer_states"][0]
    assert se["param_groups"] == sg["param_groups"] and set(se["state"]) == set(sg["state"])
    for pid in se["state"]:
        for f in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(se["state"][pid][f], sg["state"][pid][f]), (pid, f)
