"""Device-side evaluation metrics with the torchmetrics==0.11.0 call surface the reference uses
(`metric(preds, target)`, `.compute()`, `.reset()`; models/Disentangle/STiLModel.py:122-145, 360-363, 458-463, 529-545).

Accuracy keeps two int64 counters on the device (hits, samples); AUROC keeps the epoch's scores and computes the exact
(thresholds=None) area with integer rank statistics in `stil_auroc`.  Under data parallelism `.compute()` reduces the
counters / gathers the scores over the process group (torchmetrics' sync-on-compute); it reaches the collectives before it
decides anything, so a rank that received no rows takes part and an error is raised on every rank or on none.  Scores are
converted with `.to(float32)`, targets with `.to(int64)`.  No host sync until `.compute()` is read.  There is no CPU path: the kernels live in libstil_hip.so.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.distributed as dist

from ._lib import lib
from .ops import _p, _stream, _ws


def _dist_on() -> bool:
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def _here() -> torch.device:
    """the device of a rank that holds no tensor yet"""
    return torch.device("cuda", torch.cuda.current_device())


def _prep(preds: torch.Tensor, target: torch.Tensor):
    if not preds.is_cuda:
        raise RuntimeError("stil_tta_amd.metrics needs CUDA(HIP) tensors: there is no CPU fallback")
    return preds.detach().to(torch.float32).contiguous(), target.detach().to(device=preds.device, dtype=torch.int64).contiguous()


class Accuracy:
    """torchmetrics.Accuracy(task='multiclass', top_k=k, num_classes=K) (micro average) or task='binary' (threshold 0.5)."""

    def __init__(self, task: str = "multiclass", num_classes: Optional[int] = None, top_k: int = 1, threshold: float = 0.5):
        assert task in ("binary", "multiclass")
        self.task, self.num_classes, self.top_k, self.threshold = task, num_classes, int(top_k), float(threshold)
        self.counts: Optional[torch.Tensor] = None

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        p, y = _prep(preds, target)
        if self.counts is None:
            self.counts = torch.zeros(2, dtype=torch.int64, device=p.device)
        if self.task == "binary":
            if p.dim() != 1 or p.shape[0] != y.shape[0]:
                raise RuntimeError(f"binary accuracy expects preds [N] and target [N], got {tuple(p.shape)} / {tuple(y.shape)}")
            lib().metric_binary(_p(p), _p(y), p.shape[0], self.threshold, _p(self.counts), _stream())
        else:
            if p.dim() != 2 or p.shape[0] != y.shape[0]:
                raise RuntimeError(f"multiclass accuracy expects preds [N, K] and target [N], got {tuple(p.shape)} / {tuple(y.shape)}")
            lib().metric_topk(_p(p), p.shape[1], _p(y), p.shape[0], p.shape[1], self.top_k, _p(self.counts), _stream())

    __call__ = update

    def compute(self) -> torch.Tensor:
        if _dist_on():   # the collective first: a rank that saw no batch joins with zero counters (its peers are waiting in all_reduce)
            c = torch.zeros(2, dtype=torch.int64, device=_here()) if self.counts is None else self.counts.clone()
            dist.all_reduce(c, op=dist.ReduceOp.SUM)
        elif self.counts is None:
            raise RuntimeError("Accuracy.compute() before any update")
        else:
            c = self.counts
        return c[0].to(torch.float32) / c[1].to(torch.float32)

    def reset(self) -> None:
        if self.counts is not None:
            self.counts.zero_()

    def state_tensors(self, device=None) -> List[torch.Tensor]:
        """The device counters an update writes, created (zero) on `device` if no update has happened yet."""
        if self.counts is None and device is not None:
            self.counts = torch.zeros(2, dtype=torch.int64, device=device)
        return [] if self.counts is None else [self.counts]


_NO_ROWS = "AUROC.compute(): no rows arrived since the last reset() (no update, or only zero-row updates)"


class AUROC:
    """torchmetrics.AUROC(task='binary') / (task='multiclass', num_classes=K, average='macro'), exact mode."""

    def __init__(self, task: str = "multiclass", num_classes: Optional[int] = None):
        assert task in ("binary", "multiclass")
        self.task, self.num_classes = task, num_classes
        self.preds: List[torch.Tensor] = []
        self.target: List[torch.Tensor] = []
        self.per_class: Optional[torch.Tensor] = None
        self.store = None   # reserve(): (scores [capacity, K], targets [capacity], int64 row count, int32 overflow flag) on the device

    def reserve(self, capacity: int, device, K: Optional[int] = None) -> None:
        """Preallocate room for `capacity` rows: updates then append on the device at a device-held row count
        (stil_rows_append), which a captured hipGraph can replay; compute() raises if more rows arrived than fit.
        Without a reservation the scores are kept in a Python list, as before."""
        K = 1 if self.task == "binary" else int(self.num_classes if K is None else K)
        capacity = int(capacity)
        if capacity <= 0:
            raise ValueError("AUROC.reserve: capacity must be positive")
        if self.preds:
            raise RuntimeError("AUROC.reserve: scores are already accumulated in the list; reset() first")
        self.store = (torch.empty((capacity, K), dtype=torch.float32, device=device), torch.empty((capacity,), dtype=torch.int64, device=device),
                      torch.zeros(1, dtype=torch.int64, device=device), torch.zeros(1, dtype=torch.int32, device=device))

    @property
    def reserved(self) -> bool:
        return self.store is not None

    def state_tensors(self) -> List[torch.Tensor]:
        """The device tensors an update writes (a captured step's warm-up snapshot restores them)."""
        return [] if self.store is None else list(self.store)

    def has_updates(self) -> bool:
        """Did anything arrive since the last reset()?  (Reads the device row count when reserved: one host sync.)"""
        return bool(self.preds) or (self.store is not None and int(self.store[2].item()) > 0)

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        p, y = _prep(preds, target)
        if self.task == "binary":
            p = p.reshape(-1, 1)
        elif p.dim() != 2 or (self.num_classes is not None and p.shape[1] != self.num_classes):
            raise RuntimeError(f"multiclass AUROC expects preds [N, {self.num_classes}], got {tuple(p.shape)}")
        if p.shape[0] != y.shape[0]:
            raise RuntimeError("AUROC: preds / target length mismatch")
        if self.store is not None:
            sc, st, cnt, ovf = self.store
            if p.shape[1] != sc.shape[1]:
                raise RuntimeError(f"AUROC: {p.shape[1]} score columns for a store reserved with {sc.shape[1]}")
            if p.shape[0] > 0:
                lib().rows_append(_p(p), _p(y), p.shape[0], p.shape[1], _p(sc), _p(st), sc.shape[0], _p(cnt), _p(ovf), _stream())
            return
        self.preds.append(p)
        self.target.append(y)

    __call__ = update

    def _local(self):
        """-> (scores [n, K], targets [n], error or None) of this rank; n = 0 (and K = 0 where the width is not known yet) on a
        rank nothing arrived at.  An overflowed reservation is reported, not raised: compute() raises after the collectives."""
        if self.store is None:
            if self.preds:
                return torch.cat(self.preds), torch.cat(self.target), None
            if not _dist_on():
                raise RuntimeError(_NO_ROWS)
            K = 1 if self.task == "binary" else int(self.num_classes or 0)
            return torch.empty((0, K), dtype=torch.float32, device=_here()), torch.empty((0,), dtype=torch.int64, device=_here()), None
        sc, st, cnt, ovf = self.store
        n, full = int(cnt.item()), int(ovf.item())
        if full or n > sc.shape[0]:
            return sc[:0], st[:0], f"AUROC: {n} rows arrived for a reservation of {sc.shape[0]} (AUROC.reserve)"
        return sc[:n], st[:n], None

    def _gathered(self):
        """Every rank's rows in rank order.  The first collective carries (rows, columns, overflowed) of each rank, so a rank
        without rows takes part like any other, learns the width from its peers, and every rank sees the same global state
        before anything is raised."""
        p, y, err = self._local()
        if not _dist_on():
            if err:
                raise RuntimeError(err)
            return p, y
        head = torch.tensor([p.shape[0], p.shape[1], 1 if err else 0], dtype=torch.int64, device=p.device)
        heads = [torch.zeros_like(head) for _ in range(dist.get_world_size())]
        dist.all_gather(heads, head)
        heads = [[int(v) for v in h.tolist()] for h in heads]
        if any(h[2] for h in heads):
            raise RuntimeError(err or f"AUROC: the reservation of rank {[h[2] for h in heads].index(1)} overflowed (AUROC.reserve)")
        sizes, K = [h[0] for h in heads], max(h[1] for h in heads)
        if any(h[0] and h[1] != K for h in heads):
            raise RuntimeError(f"AUROC: the ranks hold scores of different widths {[h[1] for h in heads]}")
        nmax = max(sizes)
        if nmax == 0:
            return p.new_empty((0, K)), y
        pp = torch.zeros((nmax, K), dtype=p.dtype, device=p.device)
        yy = torch.zeros((nmax,), dtype=y.dtype, device=p.device)
        if p.shape[0]:
            pp[: p.shape[0]], yy[: y.shape[0]] = p, y
        ps = [torch.empty_like(pp) for _ in sizes]
        ys = [torch.empty_like(yy) for _ in sizes]
        dist.all_gather(ps, pp)
        dist.all_gather(ys, yy)
        return torch.cat([t[:n] for t, n in zip(ps, sizes)]), torch.cat([t[:n] for t, n in zip(ys, sizes)])

    def compute(self) -> torch.Tensor:
        p, y = self._gathered()   # before any decision: under data parallelism every rank has to reach the collectives
        N, K = p.shape
        if N == 0:
            raise RuntimeError(_NO_ROWS)
        nb = lib().auroc_workspace_bytes(N, K)
        if nb == 0:
            raise RuntimeError(f"AUROC: {N} x {K} scores exceed the 2^31-element limit")
        ws = _ws.get(nb, p.device)
        per = torch.empty(K, dtype=torch.float32, device=p.device)
        macro = torch.empty(1, dtype=torch.float32, device=p.device)
        lib().auroc(_p(p), K, _p(y), N, K, _p(per), _p(macro), _p(ws), nb, _stream())
        self.per_class = per
        return macro[0]

    def reset(self) -> None:
        self.preds, self.target = [], []
        if self.store is not None:
            self.store[2].zero_()
            self.store[3].zero_()
