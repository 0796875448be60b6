"""Time STiLModel.test_step under tta_method "lame" with the harness of tests/tools/tta_bench.py, whose own modes (plain, bn_adapt,
...) it passes through unchanged, one JSON line per run (one process per run); --summarize writes profiles/lame_step.json.  lame runs
at its defaults (knn, 5 neighbours, at most 100 steps, tol 1e-8: 3 + 2 + 101 launches enqueued per batch, those after the stopping
rule has fired return at once); lame_rbf is the same step under the rbf affinity.  Tool, not a test; a record, not a pass/fail
criterion.

  python tests/tools/lame_bench.py --mode plain --B 16 --img 224 >> runs.jsonl
  python tests/tools/lame_bench.py --mode bn_adapt --B 16 --img 224 >> runs.jsonl
  python tests/tools/lame_bench.py --mode lame --B 16 --img 224 >> runs.jsonl
  python tests/tools/lame_bench.py --summarize runs.jsonl --out profiles/lame_step.json"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import tta_bench as B  # noqa: E402

B.MODES["lame"] = dict(tta_method="lame")
B.MODES["lame_rbf"] = dict(tta_method="lame", tta_lame_affinity="rbf")


def summarize(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from stil_tta_amd._lib import source_hash
    runs = [json.loads(l) for l in open(a.summarize) if l.strip().startswith("{")]
    groups = {}
    for r in runs:
        groups.setdefault((r["B"], r["img"], r["cols"], r["classes"]), {}).setdefault(r["mode"], []).append(r)
    res = {}
    for (Bn, img, cols, K), modes in sorted(groups.items()):
        plain = statistics.median(r["ms_per_step"] for r in modes["plain"]) if "plain" in modes else None
        for mode, rs in sorted(modes.items()):
            ms = [r["ms_per_step"] for r in rs]
            e = dict(median_ms=statistics.median(ms), runs_ms=ms, reps_ms=[r["ms_reps"] for r in rs], iters=rs[0]["iters"])
            if plain:
                e["over_plain"] = e["median_ms"] / plain
            res[f"{mode}:B{Bn}x{img}px,{cols}cols,K{K}"] = e
    out = dict(source_hash=source_hash(), what="test_step under tta_method lame (defaults: knn, 5 neighbours, at most 100 steps, tol 1e-8; lame_rbf: "
               "the rbf affinity) beside bn_adapt and the plain test_step, tests/tools/lame_bench.py on one GPU, this tree only, one process per "
               "run; runs_ms: one figure per run, the median of its repetitions (reps_ms) of `iters` steps, host clock around steps that end in "
               "a device synchronise; over_plain: the step as a multiple of the plain step on the same rows.  A record, not a pass/fail "
               "criterion: no speed claim is made", timings=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=".")
    ap.add_argument("--label", default="")
    ap.add_argument("--mode", choices=list(B.MODES), default="lame")
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--ncat", type=int, default=16)
    ap.add_argument("--ncon", type=int, default=48)
    ap.add_argument("--classes", type=int, default=286)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--params", choices=["bn", "norm"], default="bn")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--out", default="profiles/lame_step.json")
    a = ap.parse_args()
    if a.summarize:
        summarize(a)
    else:
        a.V, a.prior, a.episodic = 32, None, False
        B.run(a)
