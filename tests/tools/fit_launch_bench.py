"""Steps per second of fit(limit_train_batches=N), eager against replayed (fit(launch="eager" | "graph")), on synthetic data held
in host memory (fit's own prefetcher copies every batch to the device):
  cardiac  -- configs/config_cardiac_STiL.yaml's step: 26 categorical + 49 continuous columns, K = 2, 128 px, 16 samples per GPU;
  dvm_b32  -- the DVM STiL step at 224 px, 32 samples per GPU (16 categorical + 48 continuous columns, K = 286).
Each run: one warm-up epoch (captures, allocator, lazy setup), then `--epochs` timed epochs of N steps (every epoch re-captures
under the anneal scheduler: a new learning rate).  Prints and appends one JSON line per (workload, launch) to --out.
  python tests/tools/fit_launch_bench.py --steps 30 --epochs 2 --out profiles/fit_launch.jsonl"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

WORKLOADS = {
    "cardiac": dict(B=16, img=128, ncat=26, card=4, ncon=49, K=2,
                    extra=dict(target="CAD", th1=0.85, beta=1.0, gamma=1.0, rate_pseudo=0.95, ema_momentum=0.4, lr_eval=1e-3)),
    "dvm_b32": dict(B=32, img=224, ncat=16, card=8, ncon=48, K=286, extra={}),
}


class _Loader:
    """`n` batches of one part (labelled or not) in the reference's layout, from one pool of host tensors."""

    def __init__(self, img, tab, y, bs, n, labelled):
        self.img, self.tab, self.y, self.bs, self.n, self.lab = img, tab, y, bs, n, labelled

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            s = slice((i * self.bs) % (len(self.y) - self.bs + 1), (i * self.bs) % (len(self.y) - self.bs + 1) + self.bs)
            yield ([torch.zeros(self.bs), self.img[s]], [self.tab[s], self.tab[s]], self.y[s], self.img[s],
                   torch.full((self.bs,), self.lab, dtype=torch.bool))


def run(name, launch, steps, epochs):
    from stil_tta_amd import STiLModel
    from stil_tta_amd import fit as F
    w = WORKLOADS[name]
    fl = [w["card"]] * w["ncat"] + [1] * w["ncon"]
    g = torch.Generator().manual_seed(7)
    B, P, K = w["B"], w["img"], w["K"]
    B_l = max(B // 8, 1)
    pool = 4 * B
    img = torch.rand(pool, 3, P, P, generator=g).pin_memory()
    cols = [torch.randint(0, w["card"], (pool, 1), generator=g).float() for _ in range(w["ncat"])] + [torch.randn(pool, w["ncon"], generator=g)]
    tab = torch.cat(cols, 1).pin_memory()
    y = torch.randint(0, K, (pool,), generator=g)
    loaders = {"l": _Loader(img, tab, y, B_l, steps, True), "u": _Loader(img, tab, y, B - B_l, steps, False)}
    torch.manual_seed(2022)
    m = STiLModel(dict(field_lengths=fl, num_classes=K, img_size=P, batch_size=B, start_epoch=0, max_epochs=100, warmup_epochs=1,
                       **w["extra"]))
    m.setup_device("cuda")
    m.prototypes.copy_(torch.nn.functional.normalize(torch.randn(K, 128, generator=g)).cuda())
    # every class must receive a confident sample per epoch (STiLModel.py:412): keep the pseudo-label path off, time the step
    m.hp.start_epoch = 10 ** 6
    m.training_epoch_end = lambda *_: None
    out = F.fit(m, loaders, None, max_epochs=1, limit_train_batches=steps, verbose=False, launch=launch)   # warm-up epoch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = F.fit(m, loaders, None, max_epochs=1 + epochs, limit_train_batches=steps, verbose=False, launch=launch, resume_from=None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = out["global_step"]
    return dict(tool="fit_launch_bench", workload=name, launch=out["launch"], batch=B, img=P, steps=n, seconds=round(dt, 4),
                steps_per_s=round(n / dt, 3), ms_per_step=round(1000 * dt / n, 3),
                note="fit() wall time incl. per-epoch re-capture (new learning rate), prefetch from pinned host memory; no validation")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cardiac,dvm_b32")
    ap.add_argument("--steps", type=int, default=30, help="training steps per epoch (limit_train_batches)")
    ap.add_argument("--epochs", type=int, default=2, help="timed epochs")
    ap.add_argument("--out", default=None, help="append the JSON lines here (e.g. profiles/fit_launch.jsonl)")
    a = ap.parse_args()
    for name in a.workloads.split(","):
        for launch in ("eager", "graph"):
            r = run(name, launch, a.steps, a.epochs)
            line = json.dumps(r)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
