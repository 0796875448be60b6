"""CPU side of tests/test_gpu_entry_points.py: every row-loss input chosen there is well-conditioned -- fp32 ATen on the CPU
stays within the suite's `close()` at `TOL` of the float64 reference the GPU tests compare with.  A kernel that misses `TOL`
on one of these inputs is therefore wrong, not unlucky: the list of ill-conditioned exceptions is empty.
The Python models of the device-state kernels are exercised here too, so that a mistake in a model shows without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_entry_points as EP  # noqa: E402


def _cases():
    return [pytest.param(fn, args, id=f"{name}-{'-'.join(str(a) for a in args)}") for name, fn, args in EP.row_loss_cases()]


@pytest.mark.parametrize("fn,args", _cases())
def test_fp32_aten_meets_tol_on_every_row_loss_input(fn, args):
    _, ref = fn(*args)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert r64.keys() == r32.keys()
    for k in r64:
        assert bool(torch.isfinite(r64[k]).all()), f"{k}: the float64 reference is not finite"
        if fn is EP.case_l2norm and args[0] >= 13:
            EP.close_rows(r32[k], r64[k], EP.L2_SPECIAL, k)
        else:
            EP.close(r32[k], r64[k], name=k)


def test_ring_model_covers_the_required_states():
    for name, (Q, D, steps) in EP.RING_SCENARIOS.items():
        assert len(steps) >= 12
        for mode in (0, 1):
            m = EP.RingModel(Q, D)
            base = 1.0
            for setp, n in steps:
                assert 0 < n and (mode == 0 or n <= Q)
                if setp is not None:
                    m.ptr = setp
                rows = (base + np.arange(n * D, dtype=np.float64)).astype(np.float32).reshape(n, D)
                base += n * D
                before = m.slots.copy()
                p = m.ptr % Q
                m.enqueue(rows, mode, 1, 1)
                written = min(n, Q - p) if mode == 0 else n
                assert int((m.slots != before).any(1).sum()) == written      # distinct values: every written slot changes
                assert 0 <= m.ptr < Q and m.count <= Q
            assert {"n == Q", "ends at the ring end", "negative pointer", "pointer >= Q", "count saturated",
                    "truncated" if mode == 0 else "wrapped mid-batch"} <= m.events, (name, mode, m.events)
    assert any(n * D > 1024 * 256 for Q, D, steps in EP.RING_SCENARIOS.values() for _, n in steps)
    assert any(D == 1 for _, D, _ in EP.RING_SCENARIOS.values()) and any(D % 4 for _, D, _ in EP.RING_SCENARIOS.values())


def test_draw_model_draws_distinct_columns():
    idx, pos = EP._draw_model(8, 64, 1000, 64, 2022, 12345)
    assert bool((np.sort(idx, 1) == np.arange(64)[None]).all()) and pos.min() >= 0 and pos.max() < 1000
    idx2, _ = EP._draw_model(8, 64, 1000, 64, 2022, 12345 + 8 * 2 * 64)
    assert not np.array_equal(idx, idx2)
