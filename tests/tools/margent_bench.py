"""Time STiLModel.test_step under tta_method "marginal_entropy" (B samples x V views) and under "tent" over the same number of
rows, from a given source tree (the branch or a checkout of its parent: --root), one JSON line per run.  Tool, not a test;
tests/tools/tta_bench.py times the other modes.

  python tests/tools/margent_bench.py --root . --label branch --mode marginal_entropy --B 1 --V 32
  python tests/tools/margent_bench.py --root ../parent --label parent --mode tent --B 32
  python tests/tools/margent_bench.py --summarize runs.jsonl --bench bench_runs.txt --kernel-stats run_kernel_stats.csv --out profiles/margent_step.json

Run parent and branch alternating in one call per shape, three runs each; --summarize reports the median and the spread of
each group and the cost of a marginal_entropy step as a multiple of the tent step over the same B x V rows."""
import argparse
import json
import os
import statistics
import sys
import time


def run(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    from stil_tta_amd import STiLModel
    from stil_tta_amd.driver import synthetic_batch
    fl = [8] * a.ncat + [1] * a.ncon
    hp = dict(field_lengths=fl, num_classes=a.classes, img_size=a.img, batch_size=a.B, mi_dropout=False, tta=True, tta_params=a.params,
              tta_method=a.mode, tta_bn_prior=a.prior)
    if a.mode == "marginal_entropy":
        hp.update(tta_views=a.V, tta_episodic=a.episodic)
    torch.manual_seed(0)
    m = STiLModel(hp)
    m.setup_device("cuda")
    m.freeze()
    n = max(a.B, 2)   # synthetic_batch splits its rows into a labelled and an unlabelled half
    batch = synthetic_batch(fl, a.classes, n, a.img, seed=1, device="cuda")
    x = [torch.cat((batch["l"][0][1], batch["u"][0][1]))[:a.B].contiguous(), torch.cat((batch["l"][1][1], batch["u"][1][1]))[:a.B].contiguous()]
    y = torch.cat((batch["l"][2], batch["u"][2]))[:a.B].contiguous()
    assert x[0].shape[0] == a.B, x[0].shape
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
    V = a.V if a.mode == "marginal_entropy" else 1
    print(json.dumps(dict(tree=a.label or root, mode=a.mode, params=a.params, B=a.B, V=V, rows=a.B * V, img=a.img, cols=a.ncat + a.ncon,
                          classes=a.classes, prior=a.prior, ms_per_step=statistics.median(reps), ms_reps=reps, iters=a.iters)), flush=True)


def summarize(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from stil_tta_amd._lib import source_hash
    runs = [json.loads(l) for l in open(a.summarize) if l.strip().startswith("{")]
    groups = {}
    for r in runs:
        groups.setdefault(f"{r['tree']}:{r['mode']}/{r['params']}:B{r['B']}xV{r['V']}x{r['img']}px", []).append(r["ms_per_step"])
    res = {k: dict(median_ms=statistics.median(v), runs_ms=v, spread_ms=max(v) - min(v)) for k, v in sorted(groups.items())}
    out = dict(source_hash=source_hash(), what="test_step under tta_method marginal_entropy (B samples x V views) and tent over the same "
                                               "number of rows, parent vs branch, alternating runs in one call per shape on one GPU",
               timings=res)
    tent = {r["rows"]: f"branch:tent/{r['params']}:B{r['B']}xV1x{r['img']}px" for r in runs if r["tree"] == "branch" and r["mode"] == "tent"}
    mult = {}
    for r in runs:
        if r["tree"] == "branch" and r["mode"] == "marginal_entropy" and r["rows"] in tent:
            k = f"branch:marginal_entropy/{r['params']}:B{r['B']}xV{r['V']}x{r['img']}px"
            mult[k] = res[k]["median_ms"] / res[tent[r["rows"]]]["median_ms"]
    out["marginal_entropy_over_tent_same_rows"] = mult
    if a.bench:
        b = {}
        for l in open(a.bench):
            l = l.strip()
            if l.startswith(("parent ", "branch ")):
                tree, js = l.split(" ", 1)
                b.setdefault(tree, []).append(json.loads(js)["ms_per_step"])
        out["bench_py_ms_per_step"] = {t: dict(median=statistics.median(v), runs=v, spread=max(v) - min(v)) for t, v in b.items()}
    if a.kernel_stats:   # rocprofv3 --kernel-trace --stats of a few steps: the launches the method adds
        import csv
        rows = [r for r in csv.DictReader(open(a.kernel_stats)) if "margent_" in r["Name"]]
        out["added_launches"] = [dict(name=r["Name"].split("(")[0], calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3) for r in rows]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=".")
    ap.add_argument("--label", default="")
    ap.add_argument("--mode", choices=["tent", "marginal_entropy"], default="marginal_entropy")
    ap.add_argument("--params", choices=["bn", "norm"], default="bn")
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--prior", type=float, default=16.0)
    ap.add_argument("--episodic", action="store_true")
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--ncat", type=int, default=16)
    ap.add_argument("--ncon", type=int, default=48)
    ap.add_argument("--classes", type=int, default=286)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--bench", default=None, help="with --summarize: lines 'parent|branch <bench.py JSON>'")
    ap.add_argument("--kernel-stats", default=None, help="with --summarize: a rocprofv3 *_kernel_stats.csv of a few steps")
    ap.add_argument("--out", default="profiles/margent_step.json")
    a = ap.parse_args()
    summarize(a) if a.summarize else run(a)
