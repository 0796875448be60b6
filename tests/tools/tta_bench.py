"""Time STiLModel.test_step under every test-time adaptation mode, plain test_step and the training step, from a given source
tree (the branch or a checkout of its parent: --root), one JSON line per run.  Tool, not a test.

  python tests/tools/tta_bench.py --root . --label branch --mode eata_fisher --B 256 --img 224 --ncat 16 --ncon 48
  python tests/tools/tta_bench.py --root ../parent --label parent --mode marginal_entropy --B 1 --V 32
  python tests/tools/tta_bench.py --summarize runs.jsonl --bench bench_runs.txt --kernel-stats run_kernel_stats.csv --out profiles/tta_step.json

--mode test / plain: test_step as the reference (no adaptation); train: one training step (zero_grad -> training_step ->
backward -> Adam, driver.train_step); the others are the rows of MODES.  The margins of EATA, DeYO and SAR are set so that every
row is selected (the full backward; SAR's twice); eata_fisher runs with an estimate from two batches; sar runs with a recovery
threshold far below any loss, so the recover launch runs and never fires; marginal_entropy runs B samples x --V views under
--prior (MEMO's own shape, B = 1 with 32 views and a prior of 16, is its default).  Run parent and branch alternating in one
call per shape, three runs each; --summarize reports per tree / mode / shape the median, the runs and their spread, the counts
the step left in last_tta, and the step as a multiple of the same tree's tent step over the same number of rows."""
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
         "eata": dict(tta_method="eata"), "eata_fisher": dict(tta_method="eata"), "shot_im": dict(tta_method="shot_im"),
         "marginal_entropy": dict(tta_method="marginal_entropy"), "deyo": dict(tta_method="deyo"),
         "sar": dict(tta_method="sar", tta_sar_rho=0.05, tta_sar_reset=1e-6)}
COUNTS = ("n_selected", "n_first", "n_reliable", "recovered")   # what a step leaves in last_tta beside its tensors


def run(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    from stil_tta_amd import STiLModel
    from stil_tta_amd.driver import synthetic_batch, train_step
    from stil_tta_amd.flat import StilAdam
    fl = [8] * a.ncat + [1] * a.ncon
    memo = a.mode == "marginal_entropy"
    B = a.B if a.B is not None else 1 if memo else 256
    hp = dict(field_lengths=fl, num_classes=a.classes, img_size=a.img, batch_size=B, mi_dropout=False, tta=True, tta_params=a.params)
    hp.update(MODES[a.mode])
    method = hp.get("tta_method")
    if method in ("eata", "deyo", "sar"):
        hp.update(tta_e_margin=2.0 * math.log(a.classes), tta_d_margin=2.0, tta_ent_margin=2.0 * math.log(a.classes), tta_plpd_margin=-2.0)
    if memo:
        hp.update(tta_views=a.V, tta_episodic=a.episodic, tta_bn_prior=16.0)
    if a.prior is not None:
        hp.update(tta_bn_prior=a.prior)
    torch.manual_seed(0)
    m = STiLModel(hp)
    m.setup_device("cuda")
    batch = synthetic_batch(fl, a.classes, max(B, 2), a.img, seed=1, device="cuda")   # it splits its rows into two halves
    if a.mode == "train":
        m.train()
        opt = StilAdam(m.flat, lr=1e-4)
        step = lambda: train_step(m, opt, batch)   # noqa: E731
    else:
        m.freeze()
        x = [torch.cat((batch["l"][0][1], batch["u"][0][1]))[:B].contiguous(), torch.cat((batch["l"][1][1], batch["u"][1][1]))[:B].contiguous()]
        y = torch.cat((batch["l"][2], batch["u"][2]))[:B].contiguous()
        assert x[0].shape[0] == B, x[0].shape
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
    out = dict(tree=a.label or root, mode=a.mode, params=a.params if method not in (None, "bn_adapt") else None, B=B,
               V=a.V if memo else 1, img=a.img, cols=a.ncat + a.ncon, classes=a.classes, prior=hp.get("tta_bn_prior"),
               ms_per_step=statistics.median(reps), ms_reps=reps, iters=a.iters,
               counts={k: int(m.last_tta[k]) for k in COUNTS if k in m.last_tta})
    print(json.dumps(out), flush=True)


def summarize(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from stil_tta_amd._lib import source_hash
    runs = [json.loads(l) for l in open(a.summarize) if l.strip().startswith("{")]
    groups, tent = {}, {}
    for r in runs:
        V = r.get("V", 1)
        key = f"{r['tree']}:{r['mode']}{'/' + r['params'] if r.get('params') else ''}:B{r['B']}{f'xV{V}' if V > 1 else ''}x{r['img']}px"
        like = (r["tree"], r["B"] * V, r["img"], r.get("params") or "bn")   # the tent run this one is a multiple of
        g = groups.setdefault(key, dict(ms=[], counts=r.get("counts", {}), like=like))
        g["ms"].append(r["ms_per_step"])
        if r["mode"] == "tent":
            tent[like] = key
    res = {k: dict(median_ms=statistics.median(g["ms"]), runs_ms=g["ms"], spread_ms=max(g["ms"]) - min(g["ms"]), **g["counts"])
           for k, g in sorted(groups.items())}
    for k, g in groups.items():
        if g["like"] in tent:
            res[k]["over_tent"] = res[k]["median_ms"] / res[tent[g["like"]]]["median_ms"]
    out = dict(source_hash=source_hash(), what="test_step under the modes of tests/tools/tta_bench.py (plain, bn_adapt, TENT, EATA, SHOT-IM, "
                                               "marginal entropy, DeYO, SAR; with / without tta_bn_prior or a Fisher estimate) and the training "
                                               "step, parent vs branch, alternating runs in one call per shape on one GPU; over_tent: the step as "
                                               "a multiple of the same tree's tent step over the same number of rows", timings=res)
    if a.bench:
        b = {}
        for l in open(a.bench):
            l = l.strip()
            if l.startswith(("parent ", "branch ")):
                tree, js = l.split(" ", 1)
                b.setdefault(tree, []).append(json.loads(js)["ms_per_step"])
        out["bench_py_ms_per_step"] = {t: dict(median=statistics.median(v), runs=v, spread=max(v) - min(v)) for t, v in b.items()}
    if a.kernel_stats:   # rocprofv3 --kernel-trace --stats of adapting steps: the launches adaptation adds, and the Adam step it gates
        import csv
        rows = [r for r in csv.DictReader(open(a.kernel_stats)) if any(t in r["Name"] for t in ("tta_", "eata_", "infomax_", "margent_", "deyo_", "patch_shuffle", "sar_", "adam_"))]
        out["added_launches"] = [dict(name=r["Name"].split("(")[0], calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3) for r in rows]
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
    ap.add_argument("--B", type=int, default=None, help="default: 256; marginal_entropy: 1")
    ap.add_argument("--V", type=int, default=32, help="marginal_entropy: views per sample")
    ap.add_argument("--prior", type=float, default=None, help="tta_bn_prior, over the mode's own (marginal_entropy: 16)")
    ap.add_argument("--episodic", action="store_true", help="marginal_entropy: tta_episodic")
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
