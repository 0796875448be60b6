"""Time STiLModel.test_step with TENT, TENT under a source-statistics prior (tta_bn_prior), the forward-only "bn_adapt" baseline
(with and without the prior) and plain eval-mode test_step, from a given source tree (the branch or a checkout of its parent:
--root), one JSON line per run.  Tool, not a test.

  python tests/tools/bn_prior_bench.py --root . --mode tent_prior --B 256 --img 224 --ncat 16 --ncon 48
  python tests/tools/bn_prior_bench.py --summarize runs.jsonl --bench bench_runs.txt --out profiles/bn_prior_step.json

--mode tent and plain run on the parent too; the other three need tta_bn_prior / "bn_adapt"."""
import argparse
import json
import os
import statistics
import sys
import time

MODES = {"plain": dict(tta_method=None), "tent": dict(tta_method="tent"), "tent_prior": dict(tta_method="tent", tta_bn_prior=16.0),
         "bn_adapt": dict(tta_method="bn_adapt"), "bn_adapt_prior": dict(tta_method="bn_adapt", tta_bn_prior=16.0)}


def run(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    from stil_tta_amd import STiLModel
    from stil_tta_amd.driver import synthetic_batch
    fl = [8] * a.ncat + [1] * a.ncon
    hp = dict(field_lengths=fl, num_classes=a.classes, img_size=a.img, batch_size=a.B, mi_dropout=False, tta=True, tta_params="bn")
    hp.update(MODES[a.mode])
    torch.manual_seed(0)
    m = STiLModel(hp)
    m.setup_device("cuda")
    m.freeze()
    batch = synthetic_batch(fl, a.classes, a.B, a.img, seed=1, device="cuda")
    x = [torch.cat((batch["l"][0][1], batch["u"][0][1])), torch.cat((batch["l"][1][1], batch["u"][1][1]))]
    y = torch.cat((batch["l"][2], batch["u"][2]))
    step = lambda: m.test_step((x, y), 0)   # noqa: E731
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    reps = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for _ in range(a.iters):
            step()
        torch.cuda.synchronize()
        reps.append((time.perf_counter() - t0) * 1e3 / a.iters)
    print(json.dumps(dict(tree=a.label or root, mode=a.mode, B=a.B, img=a.img, cols=a.ncat + a.ncon, classes=a.classes,
                          ms_per_step=statistics.median(reps), ms_reps=reps, iters=a.iters)), flush=True)


def summarize(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from stil_tta_amd._lib import source_hash
    runs = [json.loads(l) for l in open(a.summarize) if l.strip().startswith("{")]
    groups = {}
    for r in runs:
        groups.setdefault(f"{r['tree']}:{r['mode']}:B{r['B']}x{r['img']}px", []).append(r["ms_per_step"])
    res = {k: dict(median_ms=statistics.median(v), runs_ms=v, spread_ms=max(v) - min(v)) for k, v in sorted(groups.items())}
    out = dict(source_hash=source_hash(), what="test_step: plain, TENT, TENT + tta_bn_prior 16, bn_adapt, bn_adapt + tta_bn_prior 16; parent vs "
                                               "branch, alternating runs in one call per shape on one GPU (tests/tools/bn_prior_bench.py)",
               timings=res)
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
    ap.add_argument("--mode", choices=sorted(MODES), default="tent_prior")
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--ncat", type=int, default=16)
    ap.add_argument("--ncon", type=int, default=48)
    ap.add_argument("--classes", type=int, default=286)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--bench", default=None, help="with --summarize: lines 'parent|branch <bench.py JSON>'")
    ap.add_argument("--out", default="profiles/bn_prior_step.json")
    a = ap.parse_args()
    summarize(a) if a.summarize else run(a)
