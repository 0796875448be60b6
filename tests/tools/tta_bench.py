"""Time STiLModel.test_step under every test-time adaptation mode, plain test_step and the training step, from a given source
tree (the branch or a checkout of its parent: --root), one JSON line per run.  Tool, not a test.

  python tests/tools/tta_bench.py --root . --mode eata_fisher --B 256 --img 224 --ncat 16 --ncon 48
  python tests/tools/tta_bench.py --summarize runs.jsonl --bench bench_runs.txt --kernel-stats run_kernel_stats.csv --out profiles/tta_step.json

--mode test / plain: test_step as the reference (no adaptation); train: one training step (zero_grad -> training_step ->
backward -> Adam, driver.train_step); the others are the rows of MODES.  EATA's margins are set so that every row is selected
(the full backward); eata_fisher runs with an estimate from two batches."""
import argparse
import json
import math
import os
import statistics
import sys
import time

MODES = {"test": {}, "plain": {}, "train": dict(mi_dropout=True),
         "tent": dict(tta_method="tent"), "tent_prior": dict(tta_method="tent", tta_bn_prior=16.0),
         "bn_adapt": dict(tta_method="bn_adapt"), "bn_adapt_prior": dict(tta_method="bn_adapt", tta_bn_prior=16.0),
         "eata": dict(tta_method="eata"), "eata_fisher": dict(tta_method="eata")}


def run(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    from stil_tta_amd import STiLModel
    from stil_tta_amd.driver import synthetic_batch, train_step
    from stil_tta_amd.flat import StilAdam
    fl = [8] * a.ncat + [1] * a.ncon
    hp = dict(field_lengths=fl, num_classes=a.classes, img_size=a.img, batch_size=a.B, mi_dropout=False, tta=True, tta_params=a.params)
    hp.update(MODES[a.mode])
    if hp.get("tta_method") == "eata":
        hp.update(tta_e_margin=2.0 * math.log(a.classes), tta_d_margin=2.0)
    torch.manual_seed(0)
    m = STiLModel(hp)
    m.setup_device("cuda")
    batch = synthetic_batch(fl, a.classes, a.B, a.img, seed=1, device="cuda")
    if a.mode == "train":
        m.train()
        opt = StilAdam(m.flat, lr=1e-4)
        step = lambda: train_step(m, opt, batch)   # noqa: E731
    else:
        m.freeze()
        x = [torch.cat((batch["l"][0][1], batch["u"][0][1])), torch.cat((batch["l"][1][1], batch["u"][1][1]))]
        y = torch.cat((batch["l"][2], batch["u"][2]))
        if a.mode == "eata_fisher":
            m.estimate_tta_fisher([(x, y), (x, y)])
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
    out = dict(tree=a.label or root, mode=a.mode, params=a.params if hp.get("tta_method") in ("tent", "eata") else None, B=a.B,
               img=a.img, cols=a.ncat + a.ncon, classes=a.classes, ms_per_step=statistics.median(reps), ms_reps=reps, iters=a.iters)
    if hp.get("tta_method") == "eata":
        out["n_selected"] = int(m.last_tta["n_selected"])
    print(json.dumps(out), flush=True)


def summarize(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from stil_tta_amd._lib import source_hash
    runs = [json.loads(l) for l in open(a.summarize) if l.strip().startswith("{")]
    groups = {}
    for r in runs:
        key = f"{r['tree']}:{r['mode']}{'/' + r['params'] if r.get('params') else ''}:B{r['B']}x{r['img']}px"
        groups.setdefault(key, []).append(r["ms_per_step"])
    res = {k: dict(median_ms=statistics.median(v), runs_ms=v, spread_ms=max(v) - min(v)) for k, v in sorted(groups.items())}
    out = dict(source_hash=source_hash(), what="test_step under the modes of tests/tools/tta_bench.py (plain, TENT, EATA, bn_adapt; with / without "
                                               "tta_bn_prior 16 or a Fisher estimate) and the training step, parent vs branch, alternating runs "
                                               "in one call per shape on one GPU", timings=res)
    if a.bench:
        b = {}
        for l in open(a.bench):
            l = l.strip()
            if l.startswith(("parent ", "branch ")):
                tree, js = l.split(" ", 1)
                b.setdefault(tree, []).append(json.loads(js)["ms_per_step"])
        out["bench_py_ms_per_step"] = {t: dict(median=statistics.median(v), runs=v, spread=max(v) - min(v)) for t, v in b.items()}
    if a.kernel_stats:   # rocprofv3 --kernel-trace --stats of adapting steps: the launches adaptation adds, and the Adam step EATA gates
        import csv
        rows = [r for r in csv.DictReader(open(a.kernel_stats)) if any(t in r["Name"] for t in ("eata_", "adam_", "tta_entropy"))]
        out["added_launches"] = [dict(name=r["Name"].split("(")[0], calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3) for r in rows]
    bs = [k for k in res if k.startswith("branch:tent/bn:B256x224")]
    ps = [k for k in res if k.startswith("parent:train:B256x224")]
    if bs and ps:
        out["tta_over_parent_train_step_B256_224"] = res[bs[0]]["median_ms"] / res[ps[0]]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=".")
    ap.add_argument("--label", default="")
    ap.add_argument("--mode", choices=list(MODES), default="tent")
    ap.add_argument("--params", choices=["bn", "norm"], default="bn")
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
    ap.add_argument("--kernel-stats", default=None, help="with --summarize: a rocprofv3 *_kernel_stats.csv of adapting steps")
    ap.add_argument("--out", default="profiles/tta_step.json")
    a = ap.parse_args()
    summarize(a) if a.summarize else run(a)
