"""Times the device input pipeline's two branches in one process: ContrastiveBatchBuilder with augmentation_speedup=False
(torchvision branch) and =True (albumentations branch) on a uint8 DVM-like shard resident in HBM, at the bench shape (256 per
batch, 224x224 sources, P = 224) and at 128 px.  The branches alternate batch by batch within each round, so both see the
same machine state.  Writes profiles/r06_alb_pipeline.json (OUT=... to change).

    python tests/tools/alb_pipeline_bench.py [--rounds 5] [--batches 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def alg_bytes(B, S, P, alb):
    """Bytes one batch must move at least.  Both: the gathered uint8 rows (read + write), the unaugmented resize's read of the
    source, two float [B,3,P,P] outputs.  torchvision branch: the crop / blur / grey-mean kernels read the source twice more.
    albumentations branch: ColorJitter reads the source twice (grey sum, chain) and writes it, the blur reads and writes it,
    the crop reads it."""
    src, out = B * S * S * 3, B * 3 * P * P * 4
    return (3 + (2 if not alb else 6)) * src + 2 * out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the pipeline bench needs a GPU (no CPU timing is reported)"
    from stil_tta_amd.augment import ContrastiveBatchBuilder
    from stil_tta_amd._lib import source_hash
    dev, N, B, ncols = "cuda", 1024, 256, 64
    res = dict(metric="device input pipeline, ContrastiveBatchBuilder (labelled + unlabelled split 1:7), both branches in one process",
               source_hash=source_hash(), batch=B, shapes=[])
    for S in (224, 128):
        g = torch.Generator().manual_seed(99)
        images = torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8, generator=g)
        table, labels = torch.randn(N, ncols, generator=g), torch.randint(0, 2, (N,), generator=g)
        Bl = B // 8
        builders = {}
        for alb in (False, True):
            lab = ContrastiveBatchBuilder(images, table, labels, S, "dvm", labelled=True, device=dev, seed=2022, augmentation_speedup=alb)
            unl = ContrastiveBatchBuilder(images, table, labels, S, "dvm", labelled=False, device=dev, seed=2122, augmentation_speedup=alb)
            builders[alb] = (lab, unl)
        idx = [(torch.randint(0, N, (Bl,), generator=g), torch.randint(0, N, (B - Bl,), generator=g)) for _ in range(a.batches)]
        times = {False: [], True: []}
        for alb in (False, True):       # warm-up: code objects, allocator
            for il, iu in idx[:2]:
                builders[alb][0](il), builders[alb][1](iu)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for alb in (False, True):
                lab, unl = builders[alb]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for il, iu in idx:
                    lab(il), unl(iu)
                torch.cuda.synchronize()
                times[alb].append((time.perf_counter() - t0) / a.batches)
        row = dict(source=f"uint8 {S}x{S}x3", P=S)
        for alb, name in ((False, "torchvision"), (True, "albumentations")):
            t = sorted(times[alb])
            med = t[len(t) // 2]
            alg = alg_bytes(B, S, S, alb)
            row[name] = dict(ms_per_batch=round(med * 1e3, 3), ms_min=round(t[0] * 1e3, 3), ms_max=round(t[-1] * 1e3, 3),
                             samples_per_s=round(B / med, 1), algorithmic_bytes_per_batch=alg, gbps=round(alg / med / 1e9, 1))
        row["albumentations_over_torchvision"] = round(row["albumentations"]["ms_per_batch"] / row["torchvision"]["ms_per_batch"], 3)
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    res["note"] = ("medians over rounds of the mean over batches; host time included (draws on the host, uploads of the draws, "
                   "launches): what a training loop pays per batch.  Targets: albumentations <= 2x torchvision per batch and "
                   ">= 21k samples/s at 224 px.")
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r06_alb_pipeline.json"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
