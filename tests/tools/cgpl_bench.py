"""Time STiLModel.test_step under tta_method "cgpl" with the harness of tests/tools/tta_bench.py, whose own modes (tent, plain, ...)
it passes through unchanged, one JSON line per run; --summarize writes profiles/cgpl_step.json.  The threshold is 0, so every row is
learned from and the Adam step always runs; cgpl_rate1 is the same step at tta_pl_rate 1 (no projector, no prototypes).  Tool, not a
test; a record, not a pass/fail criterion.

  python tests/tools/cgpl_bench.py --mode tent --B 16 --img 224 >> runs.jsonl
  python tests/tools/cgpl_bench.py --mode cgpl --B 16 --img 224 >> runs.jsonl
  python tests/tools/cgpl_bench.py --summarize runs.jsonl --out profiles/cgpl_step.json"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import tta_bench as B  # noqa: E402

B.MODES["cgpl"] = dict(tta_method="cgpl", tta_pl_threshold=0.0)
B.MODES["cgpl_rate1"] = dict(tta_method="cgpl", tta_pl_threshold=0.0, tta_pl_rate=1.0)


def summarize(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from stil_tta_amd._lib import source_hash
    runs = [json.loads(l) for l in open(a.summarize) if l.strip().startswith("{")]
    groups = {}
    for r in runs:   # a mode is named with its adapted set: tent/bn, cgpl/norm, plain
        name = r["mode"] + ("/" + r["params"] if r.get("params") else "")
        groups.setdefault((r["B"], r["img"], r["cols"], r["classes"]), {}).setdefault(name, []).append(r)
    res = {}
    for (Bn, img, cols, K), modes in sorted(groups.items()):
        tents = {n.split("/")[1]: statistics.median(r["ms_per_step"] for r in rs) for n, rs in modes.items() if n.startswith("tent/")}
        for mode, rs in sorted(modes.items()):
            ms = [r["ms_per_step"] for r in rs]
            e = dict(median_ms=statistics.median(ms), runs_ms=ms, reps_ms=[r["ms_reps"] for r in rs], iters=rs[0]["iters"])
            tent = tents.get(mode.split("/")[1] if "/" in mode else "bn")
            if tent:
                e["over_tent"] = e["median_ms"] / tent
            res[f"{mode}:B{Bn}x{img}px,{cols}cols,K{K}"] = e
    out = dict(source_hash=source_hash(), what="test_step under tta_method cgpl (tta_params bn, threshold 0: every row selected; cgpl_rate1: "
               "tta_pl_rate 1) beside tent (bn) and the plain test_step, tests/tools/cgpl_bench.py on one GPU, this tree only; runs_ms: one "
               "figure per run, the median of its repetitions (reps_ms) of `iters` steps; over_tent: the step as a multiple of the tent step "
               "on the same rows and adapted set (plain: of tent/bn).  A record, not a pass/fail criterion: no speed claim is made", timings=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=".")
    ap.add_argument("--label", default="")
    ap.add_argument("--mode", choices=list(B.MODES), default="cgpl")
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
    ap.add_argument("--out", default="profiles/cgpl_step.json")
    a = ap.parse_args()
    if a.summarize:
        summarize(a)
    else:
        a.V, a.prior, a.episodic = 32, None, False
        B.run(a)
