"""Time STiLModel.test_step under tta_method "sar" and "tent" from a given source tree (the branch, or a checkout of its parent for
"tent": --root), one JSON line per run; tests/tools/tta_bench.py has no "sar" mode.  Tool, not a test.

  python tests/tools/sar_bench.py --root . --label branch --mode sar --B 256 --img 224 --ncat 16 --ncon 48
  python tests/tools/sar_bench.py --summarize runs.jsonl --bench bench_runs.txt --out profiles/sar_step.json

"sar" runs with a margin above ln K, so every row is selected in both passes (the full backward twice), and with a recovery
threshold far below any loss, so the recover launch runs and never fires."""
import argparse
import json
import math
import os
import statistics
import sys
import time

MODES = {"tent": dict(tta_method="tent"), "sar": dict(tta_method="sar", tta_sar_rho=0.05, tta_sar_reset=1e-6)}


def run(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    from stil_tta_amd import STiLModel
    from stil_tta_amd.driver import synthetic_batch
    fl = [8] * a.ncat + [1] * a.ncon
    hp = dict(field_lengths=fl, num_classes=a.classes, img_size=a.img, batch_size=a.B, mi_dropout=False, tta=True, tta_params="bn")
    hp.update(MODES[a.mode])
    if a.mode == "sar":
        hp.update(tta_e_margin=2.0 * math.log(a.classes))
    torch.manual_seed(0)
    m = STiLModel(hp)
    m.setup_device("cuda")
    m.freeze()
    batch = synthetic_batch(fl, a.classes, a.B, a.img, seed=1, device="cuda")
    x = [torch.cat((batch["l"][0][1], batch["u"][0][1])), torch.cat((batch["l"][1][1], batch["u"][1][1]))]
    y = torch.cat((batch["l"][2], batch["u"][2]))
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
    out = dict(tree=a.label or root, mode=a.mode, B=a.B, img=a.img, cols=a.ncat + a.ncon, classes=a.classes,
               ms_per_step=statistics.median(reps), ms_reps=reps, iters=a.iters)
    if a.mode == "sar":
        lt = m.last_tta
        out.update(n_first=int(lt["n_first"]), n_selected=int(lt["n_selected"]), recovered=int(lt["recovered"]))
    print(json.dumps(out), flush=True)


def summarize(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from stil_tta_amd._lib import source_hash
    runs = [json.loads(l) for l in open(a.summarize) if l.strip().startswith("{")]
    groups, meta = {}, {}
    for r in runs:
        key = f"{r['tree']}:{r['mode']}:B{r['B']}x{r['img']}px/{r['cols']}cols"
        groups.setdefault(key, []).append(r["ms_per_step"])
        if r["mode"] == "sar":
            meta[key] = dict(n_first=r["n_first"], n_selected=r["n_selected"], recovered=r["recovered"])
    res = {k: dict(median_ms=statistics.median(v), runs_ms=v, spread_ms=max(v) - min(v), **meta.get(k, {})) for k, v in sorted(groups.items())}
    out = dict(source_hash=source_hash(), what="test_step under tta_method tent (parent and branch) and sar (branch, every row selected in both passes, "
                                               "the recover launch running without firing), alternating runs in one call per shape on one GPU", timings=res)
    for k in res:
        if k.startswith("branch:sar:"):
            shape = k.split(":", 2)[2]
            t = res.get(f"branch:tent:{shape}")
            if t:
                out.setdefault("sar_over_tent", {})[shape] = res[k]["median_ms"] / t["median_ms"]
                out.setdefault("sar_minus_two_tent_ms", {})[shape] = res[k]["median_ms"] - 2 * t["median_ms"]
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
    ap.add_argument("--mode", choices=list(MODES), default="sar")
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
    ap.add_argument("--out", default="profiles/sar_step.json")
    a = ap.parse_args()
    summarize(a) if a.summarize else run(a)
