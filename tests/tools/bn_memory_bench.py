"""Time STiLModel.test_step on the BatchNorm memory (tta_bn_momentum, tta_method "dua") against the steps it stands beside, from
a given source tree (the branch or a checkout of its parent: --root), one JSON line per run.  Tool, not a test.

  python tests/tools/bn_memory_bench.py --root ../parent --label parent --mode tent_prior --B 256
  python tests/tools/bn_memory_bench.py --root . --label branch --mode tent_memory --B 256
  python tests/tools/bn_memory_bench.py --root . --label branch --mode dua --B 1 --V 64
  python tests/tools/bn_memory_bench.py --root . --label branch --mode bn_adapt --B 65
  python tests/tools/bn_memory_bench.py --summarize runs.jsonl --bench bench_runs.txt --out profiles/bn_memory_step.json

tent_prior: tent + tta_bn_prior 16 (both trees); tent_memory: tent + tta_bn_momentum 0.05 (RoTTA's rule); dua: the published
setting 0.1 / 0.94 / 0.005 on --V views; bn_adapt: the forward-only baseline, to set beside dua on the same number of rows (B V + B).
--cardiac: K = 2, 26 + 49 columns.  Run parent and branch alternating in one call per shape, three runs each; wall clock over --iters
steps between two device synchronisations, after --warmup steps; --summarize reports per tree / mode / shape the median, the runs and
their spread."""
import argparse
import json
import os
import statistics
import sys
import time

MODES = {"tent_prior": dict(tta_method="tent", tta_bn_prior=16.0), "tent_memory": dict(tta_method="tent", tta_bn_momentum=0.05),
         "tent_memory_prior": dict(tta_method="tent", tta_bn_momentum=0.05, tta_bn_prior=16.0),
         "bn_adapt": dict(tta_method="bn_adapt"), "bn_adapt_memory": dict(tta_method="bn_adapt", tta_bn_momentum=0.05),
         "dua": dict(tta_method="dua", tta_bn_momentum=0.1, tta_bn_momentum_decay=0.94, tta_bn_momentum_min=0.005)}


def run(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    from stil_tta_amd import STiLModel
    from stil_tta_amd.driver import synthetic_batch
    ncat, ncon, classes = (26, 49, 2) if a.cardiac else (16, 48, 286)
    fl = ([4] if a.cardiac else [8]) * ncat + [1] * ncon
    hp = dict(field_lengths=fl, num_classes=classes, img_size=a.img, batch_size=a.B, mi_dropout=False, tta=True)
    if a.cardiac:
        hp.update(target="CAD")
    hp.update(MODES[a.mode])
    if a.mode == "dua":
        hp.update(tta_views=a.V)
    torch.manual_seed(0)
    m = STiLModel(hp)
    m.setup_device("cuda")
    m.freeze()
    batch = synthetic_batch(fl, classes, max(a.B, 2), a.img, seed=1, device="cuda")   # it splits its rows into two halves
    x = [torch.cat((batch["l"][0][1], batch["u"][0][1]))[:a.B].contiguous(), torch.cat((batch["l"][1][1], batch["u"][1][1]))[:a.B].contiguous()]
    y = torch.cat((batch["l"][2], batch["u"][2]))[:a.B].contiguous()
    assert x[0].shape[0] == a.B, x[0].shape
    for _ in range(a.warmup):
        m.test_step((x, y), 0)
    torch.cuda.synchronize()
    reps = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for _ in range(a.iters):
            m.test_step((x, y), 0)
        torch.cuda.synchronize()
        reps.append((time.perf_counter() - t0) * 1e3 / a.iters)
    print(json.dumps(dict(tree=a.label or root, mode=a.mode, B=a.B, V=a.V if a.mode == "dua" else 1, img=a.img, cardiac=a.cardiac,
                          ms_per_step=statistics.median(reps), ms_reps=reps, iters=a.iters)), flush=True)


def summarize(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from stil_tta_amd._lib import source_hash
    runs = [json.loads(l) for l in open(a.summarize) if l.strip().startswith("{")]
    groups = {}
    for r in runs:
        key = f"{r['tree']}:{r['mode']}:{'cardiac' if r['cardiac'] else 'dvm'}:B{r['B']}{'xV%d' % r['V'] if r['V'] > 1 else ''}x{r['img']}px"
        groups.setdefault(key, []).append(r["ms_per_step"])
    res = {k: dict(median_ms=statistics.median(v), runs_ms=v, spread_ms=max(v) - min(v)) for k, v in sorted(groups.items())}
    out = dict(source_hash=source_hash(), what="test_step under the modes of tests/tools/bn_memory_bench.py, parent vs branch, alternating runs in "
                                               "one call per shape on one GPU; wall clock per step", timings=res)
    if a.bench:
        b = {}
        for l in open(a.bench):
            l = l.strip()
            if l.startswith(("parent ", "branch ")):
                tree, js = l.split(" ", 1)
                b.setdefault(tree, []).append(json.loads(js)["ms_per_step"])
        out["bench_py_ms_per_step"] = {t: dict(median=statistics.median(v), runs=v, spread=max(v) - min(v)) for t, v in b.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=".")
    ap.add_argument("--label", default="")
    ap.add_argument("--mode", choices=list(MODES), default="tent_memory")
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--V", type=int, default=64, help="dua: views per sample")
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--cardiac", action="store_true")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--bench", default=None, help="with --summarize: lines 'parent|branch <bench.py JSON>'")
    ap.add_argument("--out", default="profiles/bn_memory_step.json")
    a = ap.parse_args()
    summarize(a) if a.summarize else run(a)
