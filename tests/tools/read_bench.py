"""Time STiLModel.test_step under tta_method "read" (tta_params "fusion") with the harness of tests/tools/tta_bench.py, whose own
modes (tent, plain, ...) it passes through unchanged, one JSON line per run; --summarize writes profiles/read_step.json.  Tool, not a
test; a record, not a pass/fail criterion.

  python tests/tools/read_bench.py --mode tent --B 256 --img 224 >> runs.jsonl
  python tests/tools/read_bench.py --mode read --B 256 --img 224 >> runs.jsonl
  python tests/tools/read_bench.py --summarize runs.jsonl --out profiles/read_step.json"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import tta_bench as B  # noqa: E402

B.MODES["read"] = dict(tta_method="read", tta_params="fusion")


def summarize(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from stil_tta_amd._lib import source_hash
    runs = [json.loads(l) for l in open(a.summarize) if l.strip().startswith("{")]
    groups = {}
    for r in runs:
        groups.setdefault((r["B"], r["img"], r["cols"], r["classes"]), {}).setdefault(r["mode"], []).append(r)
    res = {}
    for (Bn, img, cols, K), modes in sorted(groups.items()):
        tent = statistics.median(r["ms_per_step"] for r in modes["tent"]) if "tent" in modes else None
        for mode, rs in sorted(modes.items()):
            ms = [r["ms_per_step"] for r in rs]
            e = dict(median_ms=statistics.median(ms), runs_ms=ms, reps_ms=[r["ms_reps"] for r in rs], iters=rs[0]["iters"])
            if tent:
                e["over_tent"] = e["median_ms"] / tent
            res[f"{mode}:B{Bn}x{img}px,{cols}cols,K{K}"] = e
    out = dict(source_hash=source_hash(), what="test_step under tta_method read (tta_params fusion) beside tent (bn) and the plain test_step, "
               "tests/tools/read_bench.py on one GPU, this tree only; runs_ms: one figure per run, the median of its repetitions (reps_ms) of "
               "`iters` steps; over_tent: the step as a multiple of the tent step on the same rows.  A record, not a pass/fail criterion: "
               "no speed claim is made", timings=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=".")
    ap.add_argument("--label", default="")
    ap.add_argument("--mode", choices=list(B.MODES), default="read")
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--ncat", type=int, default=16)
    ap.add_argument("--ncon", type=int, default=48)
    ap.add_argument("--classes", type=int, default=286)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--out", default="profiles/read_step.json")
    a = ap.parse_args()
    if a.summarize:
        summarize(a)
    else:
        a.params, a.V, a.prior, a.episodic = ("fusion" if a.mode == "read" else "bn"), 32, None, False
        B.run(a)
