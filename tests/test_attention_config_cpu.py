"""`stil_attention_config` on the host: the kernel codes tests/test_gpu_attention.py relies on, refusal exactly where the entry
points refuse, and the set of shapes the forward takes and the backward refuses.  No GPU: the query makes no GPU call, and an
entry point refuses a shape that fits no kernel before its first one (only refused shapes are passed to the entry points
here, with addresses nothing dereferences)."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as A  # noqa: E402

LDS = 160 * 1024
FAKE = ctypes.c_void_p(4096)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as G
    G.build()
    from stil_tta_amd._lib import lib
    return lib()


def valu_bytes(Sq, Skv, d, bwd):
    """LDS of the VALU kernels as csrc/transformer.hip lays it out: Q [Sq][d], K/V [Skv][d + 4], P [Sq][Skv] forward; dO/Q and
    V/K [max(Sq, Skv)][d + 4] plus dS and the dropped probabilities [Sq][Skv] backward"""
    if bwd:
        return 4 * (2 * max(Sq, Skv) * (d + 4) + 2 * Sq * Skv)
    return 4 * (Sq * d + Skv * (d + 4) + Sq * Skv)


def mfma_bytes(Sq, Skv, d, bwd):
    """LDS of the matrix-pipe kernels: windows padded to 16, row strides == 20 (mod 32) (pad), == 16 (mod 64) (padT) or d + 4"""
    up16 = lambda n: (n + 15) // 16 * 16
    pad = lambda n: (n + 4 - 20 + 31) // 32 * 32 + 20
    padT = lambda n: (n - 16 + 63) // 64 * 64 + 16
    SqP, SkP = up16(Sq), up16(Skv)
    if bwd:
        return 4 * (SqP * max(pad(d), padT(d)) + SkP * max(d + 4, padT(d)) + SqP * pad(SkP))
    return 4 * (SqP * (d + 4) + SkP * pad(d) + SqP * pad(SkP))


def fits_some_kernel(Sq, Skv, d, bwd):
    """the documented limits: 160 KiB of LDS for the VALU kernel, or -- head dim a multiple of 16 and at most 4096 float4 per
    prefetched operand -- for the matrix-pipe kernel"""
    mfma = d % 16 == 0 and mfma_bytes(Sq, Skv, d, bwd) <= LDS and (max(Sq, Skv) + 15) // 16 * 16 * (d // 4) <= 4096
    return mfma or valu_bytes(Sq, Skv, d, bwd) <= LDS


def test_the_cases_of_the_gpu_test_map_to_their_kernels(L):
    codes = {c[:3]: (L.attention_config(*c[:3], 0), L.attention_config(*c[:3], 1)) for c in A.CASES}
    assert codes == {c[:3]: c[5:] for c in A.CASES}
    assert A.coverage_gaps(codes) == [], "a kernel is no longer reached by a ragged square, Sq < Skv and Sq > Skv"
    assert len(A.coverage_gaps({k: v for k, v in codes.items() if k[0] == k[1]})) > 0    # the check can fail
    for Sq, Skv, d in A.REFUSED_BWD:
        assert L.attention_config(Sq, Skv, d, 0) == 0 and L.attention_config(Sq, Skv, d, 1) < 0
    # the issue's arithmetic for the tightest case: 159744 of 163840 bytes
    assert mfma_bytes(125, 128, 64, True) == 159744 and L.attention_config(125, 128, 64, 1) == 2


def _refuses(L, Sq, Skv, d, bwd, match):
    T = max(Sq, Skv, 1) + 8
    with pytest.raises(RuntimeError, match=match):
        if bwd:
            L.attention_bwd(FAKE, FAKE, FAKE, None, FAKE, 1, T, 1, d, 0, Sq, 0, Skv, 1.0, 0.0, None)
        else:
            L.attention_fwd(FAKE, FAKE, FAKE, None, 1, T, 1, d, 0, Sq, 0, Skv, 1.0, 0.0, None)


def test_config_is_negative_exactly_where_the_entry_points_refuse(L):
    n_refused = 0
    for d in (4, 12, 16, 20, 32, 48, 64, 80, 96, 112, 128, 144, 256):
        for Sq, Skv in [(n, n) for n in range(1, 200, 3)] + [(n, 300 - n) for n in range(10, 300, 20)] + [(1, 2000), (2000, 1), (300, 300)]:
            for bwd in (0, 1):
                code = L.attention_config(Sq, Skv, d, bwd)
                assert code in (0, 1, 2) or code < 0
                assert (code >= 0) == fits_some_kernel(Sq, Skv, d, bwd), (Sq, Skv, d, bwd, code)
                if code > 0:
                    assert d % 16 == 0
                if code < 0:                    # the entry point says so itself, on the host, before any launch
                    _refuses(L, Sq, Skv, d, bwd, "LDS")
                    n_refused += 1
    assert n_refused > 100
    for Sq, Skv, d, match in [(8, 8, 0, "multiple of 4"), (8, 8, -16, "multiple of 4"), (8, 8, 18, "multiple of 4"),
                              (0, 8, 16, "window"), (8, 0, 16, "window"), (-3, 8, 16, "window")]:
        for bwd in (0, 1):
            assert L.attention_config(Sq, Skv, d, bwd) < 0
            _refuses(L, Sq, Skv, d, bwd, match)


# squares n x n up to 192 that the forward takes and the backward refuses, per head dim (both ends included)
FWD_ONLY = {16: (177, 185), 32: (129, 171), 64: (129, 146), 128: (97, 110)}    # above the span neither runs, below it both


def test_the_shapes_forward_takes_and_backward_refuses_are_pinned(L):
    for d, span in FWD_ONLY.items():
        got = [n for n in range(1, 193) if L.attention_config(n, n, d, 0) >= 0 and L.attention_config(n, n, d, 1) < 0]
        assert got == list(range(span[0], span[1] + 1)), (d, got[:1], got[-1:])
        assert [n for n in range(1, 193) if L.attention_config(n, n, d, 0) < 0] == list(range(span[1] + 1, 193))


def test_fp32_aten_meets_the_caps_on_every_input_of_the_gpu_test():
    """the yardstick of tests/test_gpu_attention.py: fp32 ATen against float64 on the same inputs, per output kind.  It is
    non-zero and below test_attention's tolerances (no input here is ill-conditioned beyond them); the kernels' bound is 4 x it"""
    errs, bounds = A.aten_errors(), A.bounds()
    print("fp32 ATen vs float64:", errs, "kernel bounds:", bounds)
    for kind in A.KINDS:
        for key, e in errs[kind].items():
            assert 0.0 < e < A.CAP[key], (kind, key, e)
            assert bounds[kind][key] == min(A.CAP[key], A.FACTOR * e)
            assert bounds[kind][key] <= min(A.CAP[key], A.FACTOR * max(errs[k][key] for k in A.KINDS))   # never wider than one bound over all inputs
