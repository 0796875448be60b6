"""Time STiLModel.test_step under tta_method "deyo" against "tent" on the same build, batch and GPU (alternating groups of
steps in one process), and stil_patch_shuffle by itself (HIP events; bytes read + written per second).  Tool, not a test;
tests/tools/tta_bench.py and tests/tools/margent_bench.py time the other modes.

  python tests/tools/deyo_bench.py --B 256 --img 224 --out profiles/deyo_step.json
  python tests/tools/deyo_bench.py --bench bench_runs.txt --out profiles/deyo_step.json     # adds lines 'parent|branch <bench.py JSON>'"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from stil_tta_amd import STiLModel, tta
    from stil_tta_amd._lib import source_hash
    from stil_tta_amd.driver import synthetic_batch
    fl = [8] * a.ncat + [1] * a.ncon
    batch = synthetic_batch(fl, a.classes, a.B, a.img, seed=1, device="cuda")
    x = [torch.cat((batch["l"][0][1], batch["u"][0][1])).contiguous(), torch.cat((batch["l"][1][1], batch["u"][1][1])).contiguous()]
    y = torch.cat((batch["l"][2], batch["u"][2])).contiguous()
    models = {}
    for mode in ("tent", "deyo"):
        torch.manual_seed(0)
        m = STiLModel(dict(field_lengths=fl, num_classes=a.classes, img_size=a.img, batch_size=a.B, mi_dropout=False, tta=True, tta_params=a.params,
                           tta_method=mode, tta_patch_grid=a.grid))
        m.setup_device("cuda")
        m.freeze()
        models[mode] = m
    times = {k: [] for k in models}
    for k, m in models.items():
        for _ in range(a.warmup):
            m.test_step((x, y), 0)
    torch.cuda.synchronize()
    for _ in range(a.reps):                              # alternating groups
        for k, m in models.items():
            t0 = time.perf_counter()
            for _ in range(a.iters):
                m.test_step((x, y), 0)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
    res = {k: dict(median_ms=statistics.median(v), runs_ms=v, spread_ms=max(v) - min(v)) for k, v in times.items()}
    # the shuffle by itself: 2 x B C H W x 4 bytes moved per call
    img = x[0]
    perm = torch.as_tensor(tta.draw_perm(np.random.default_rng(0), a.B, a.grid)).cuda()
    for _ in range(3):
        tta.patch_shuffle(img, a.grid, perm)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(a.reps):
        s.record()
        for _ in range(20):
            tta.patch_shuffle(img, a.grid, perm)
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) * 1e3 / 20)
    nbytes = 2 * img.numel() * 4
    out = dict(source_hash=source_hash(), what="test_step under tta_method deyo against tent, alternating groups on one build and one GPU; "
                                               "stil_patch_shuffle by itself (allocation of its output included)",
               shape=dict(B=a.B, img=a.img, cols=a.ncat + a.ncon, classes=a.classes, params=a.params, grid=a.grid, iters=a.iters),
               step_ms=res, deyo_minus_tent_ms=res["deyo"]["median_ms"] - res["tent"]["median_ms"],
               deyo_over_tent=res["deyo"]["median_ms"] / res["tent"]["median_ms"],
               patch_shuffle=dict(bytes_per_call=nbytes, us_per_call=statistics.median(us), runs_us=us,
                                  tb_per_s=nbytes / (statistics.median(us) * 1e-6) / 1e12))
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
    ap.add_argument("--params", choices=["bn", "norm"], default="bn")
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--ncat", type=int, default=16)
    ap.add_argument("--ncon", type=int, default=48)
    ap.add_argument("--classes", type=int, default=286)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bench", default=None, help="lines 'parent|branch <bench.py JSON>' of alternating bench.py runs")
    ap.add_argument("--out", default="profiles/deyo_step.json")
    main(ap.parse_args())
