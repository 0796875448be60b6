"""Golden fixtures under tests/golden/ within the repository's limit of 1 MiB per committed file.

A fixture whose compressed form fits is one ordinary NAME.npz.  A larger one is written as numbered shards NAME.0.npz,
NAME.1.npz, ... (an array too large for one shard is cut along its first axis into members KEY@partI) and `load` reads
either form back as one mapping with the arrays bit for bit as they were saved."""
from __future__ import annotations

import io
import os
import zlib

import numpy as np

LIMIT = 1 << 20            # bytes per committed file
_BUDGET = 900_000          # estimated compressed bytes per shard: headroom for the zip records of every member
_PIECE = _BUDGET // 2      # arrays whose compressed estimate exceeds this are cut along their first axis
_SPLIT = "@part"


class Fixture(dict):
    """dict of arrays with the `files` list of an np.load result."""

    @property
    def files(self):
        return list(self)


def _estimate(a: np.ndarray) -> int:
    buf = io.BytesIO()
    np.save(buf, a, allow_pickle=False)
    return len(zlib.compress(buf.getvalue(), 6)) + 200


def _shards(path: str):
    base = path[:-len(".npz")]
    out, i = [], 0
    while os.path.exists(f"{base}.{i}.npz"):
        out.append(f"{base}.{i}.npz")
        i += 1
    return out


def save(path: str, fx) -> list:
    """Write the mapping `fx` (name -> array) as PATH (NAME.npz) or as its shards; returns the files written."""
    assert path.endswith(".npz"), path
    pieces = []
    for k, v in fx.items():
        assert _SPLIT not in k, k
        v = np.asarray(v)
        est = _estimate(v)
        if est > _PIECE and v.ndim >= 1 and v.shape[0] > 1:
            parts = np.array_split(v, min(v.shape[0], -(-est // _PIECE)))
            pieces += [(f"{k}{_SPLIT}{i}", p, _estimate(p)) for i, p in enumerate(parts)]
        else:
            pieces.append((k, v, est))
    groups, cur, size = [], {}, 0
    for k, v, est in pieces:
        if cur and size + est > _BUDGET:
            groups.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += est
    groups.append(cur)
    for f in _shards(path) + ([path] if os.path.exists(path) else []):
        os.remove(f)
    base = path[:-len(".npz")]
    files = [path] if len(groups) == 1 else [f"{base}.{i}.npz" for i in range(len(groups))]
    for f, g in zip(files, groups):
        np.savez_compressed(f, **g)
        assert os.path.getsize(f) < LIMIT, (f, os.path.getsize(f))
    return files


def load(path: str) -> Fixture:
    """PATH (NAME.npz) or, where it was sharded, NAME.0.npz, NAME.1.npz, ... as one mapping."""
    files = [path] if os.path.exists(path) else _shards(path)
    if not files:
        raise FileNotFoundError(path)
    out, cut = Fixture(), {}
    for f in files:
        with np.load(f) as z:
            for k in z.files:
                if _SPLIT in k:
                    name, i = k.rsplit(_SPLIT, 1)
                    out.setdefault(name, None)
                    cut.setdefault(name, {})[int(i)] = z[k]
                else:
                    out[k] = z[k]
    for name, parts in cut.items():
        out[name] = np.concatenate([parts[i] for i in range(len(parts))])
    return out
