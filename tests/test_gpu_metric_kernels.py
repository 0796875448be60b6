"""The metric kernels (csrc/metrics.hip: stil_metric_topk, stil_metric_binary, stil_auroc, stil_auroc_workspace_bytes) called
through the C ABI at the cases of tests/metric_cases.py, and stil_tta_amd/metrics.py on top of them -- alone and on two ranks.

Every expectation is exact: the counters are integers, and the AUROC values are compared as fp32 bit patterns with the
pair-counting reference (the kernel's arithmetic is integer up to one float64 division and one rounding, which the reference
repeats: there is no tolerance in this module).  Every call runs twice with equal bits, every output sits between sentinels,
the inputs are compared with what was uploaded.  NaN among AUROC scores is out of contract (include/stil_hip.h);
`test_auroc_nan_in_one_column_leaves_the_other_classes_alone` holds the little that is pinned about it."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metric_cases as M  # noqa: E402
from test_gpu_entry_points import SENT, P, _release_operands, _st, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISENT = -5
GUARD = 64                      # bytes behind the AUROC workspace
SHARDS = (37, 5)                # rows of rank 0 and rank 1


@pytest.fixture(scope="module")
def L():
    from stil_tta_amd._lib import lib
    return lib()


def f32bits(t):
    """the raw words of an fp32 tensor / array on the host: equal words are equal bits, -0.0 and NaN included"""
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t, dtype=np.float32)
    return a.view(np.int32).tolist()


def same_input(d, host):
    return torch.equal(d.cpu().view(torch.int32) if d.dtype == torch.float32 else d.cpu(), host.view(torch.int32) if host.dtype == torch.float32 else host)


# =====================================================================================================================
# counters
# =====================================================================================================================
def _counters(hits=0, total=0):
    """[ISENT, hits, total, ISENT] int64 -> (buffer, the two counters in the middle)"""
    buf = torch.tensor([ISENT, hits, total, ISENT], dtype=torch.int64, device="cuda")
    return buf, buf[1:3]


def _read(buf):
    torch.cuda.synchronize()
    b = buf.cpu().tolist()
    assert b[0] == ISENT and b[3] == ISENT, "a counter's neighbour changed"
    return b[1:3]


def _topk(L, s, y, K, k, into=None):
    sd, yd = dev(s), dev(y)
    buf, cnt = into or _counters()
    L.metric_topk(P(sd), s.shape[1], P(yd), s.shape[0], K, k, P(cnt), _st())
    got = _read(buf)
    assert same_input(sd, s) and same_input(yd, y), "an input changed"
    return got


def _binary(L, p, y, thr, into=None):
    pd, yd = dev(p), dev(y)
    buf, cnt = into or _counters()
    L.metric_binary(P(pd), P(yd), p.shape[0], thr, P(cnt), _st())
    got = _read(buf)
    assert same_input(pd, p) and same_input(yd, y), "an input changed"
    return got


@pytest.mark.parametrize("name", [c.name for c in M.TOPK_TABLE])
def test_topk_counters_equal_the_sorted_position(L, name):
    c = M.TOPK_BY_NAME[name]
    s, y = M.topk_case(c)
    for k in M.topk_ks(c):
        want = [int(M.topk_reference(s, y, c.K, k).sum()), s.shape[0]]
        got = _topk(L, s, y, c.K, k)
        print(f"TOPK {name} k={k}: got {got} want {want}")
        assert got == want, (name, k)
        assert _topk(L, s, y, c.K, k) == got, "a second identical call differs"
    if c.pad:
        assert _topk(L, s[:, :c.K].contiguous(), y, c.K, 1) == _topk(L, s, y, c.K, 1), "ld = K + 5 changes the count"


@pytest.mark.parametrize("name", [c.name for c in M.TOPK_NAN])
def test_topk_nan_rows_one_by_one(L, name):
    """each NaN row alone (N = 1), so that a miss names its placement"""
    c = M.TOPK_BY_NAME[name]
    for r, t, place in M.nan_rows(c.K):
        s, y = r[None].contiguous(), torch.tensor([t])
        for k in M.topk_ks(c):
            assert _topk(L, s, y, c.K, k) == [int(M.topk_reference(s, y, c.K, k)[0]), 1], (name, t, place, k)


@pytest.mark.parametrize("case", M.BINARY_TABLE, ids=lambda c: f"N{c.N}_thr{c.thr}")
def test_binary_counters_equal_the_comparison(L, case):
    p, y = M.binary_case(case)
    want = [int(M.binary_reference(p.numpy(), y.numpy(), case.thr).sum()), case.N]
    got = _binary(L, p, y, case.thr)
    print(f"BINARY {case}: got {got} want {want}")
    assert got == want
    assert _binary(L, p, y, case.thr) == got, "a second identical call differs"


def test_counters_add_over_calls_and_an_empty_call_leaves_them(L):
    cases = [M.TOPK_BY_NAME[n] for n in ("grid_K65_N257", "nan_K65", "bad_targets")]
    for k in (1, 5):
        into, want = _counters(7, 11), [7, 11]
        for c in cases:      # K differs from call to call: the counters do not care
            s, y = M.topk_case(c)
            want = [want[0] + int(M.topk_reference(s, y, c.K, k).sum()), want[1] + s.shape[0]]
            assert _topk(L, s, y, c.K, k, into=into) == want
        assert _topk(L, s[:0].contiguous(), y[:0].contiguous(), c.K, k, into=into) == want, "N = 0 moved a counter"
    into, want = _counters(3, 4), [3, 4]
    for c in (M.Binary(257, 0.5), M.Binary(64, 0.0), M.Binary(513, 0.5)):
        p, y = M.binary_case(c)
        want = [want[0] + int(M.binary_reference(p.numpy(), y.numpy(), c.thr).sum()), want[1] + c.N]
        assert _binary(L, p, y, c.thr, into=into) == want
    assert _binary(L, p[:0].contiguous(), y[:0].contiguous(), 0.5, into=into) == want, "N = 0 moved a counter"
    s, y = M.topk_case(M.TOPK_BY_NAME["bad_targets"])             # [9, 5]: every call below is refused on the host
    sd, yd, cnt = dev(s), dev(y), into[1]
    for ld, N, k in ((4, 9, 1), (5, 9, 0), (5, -1, 1)):           # ld < K, k < 1, N < 0
        with pytest.raises(RuntimeError, match="stil_metric_topk"):
            L.metric_topk(P(sd), ld, P(yd), N, 5, k, P(cnt), _st())
        assert "stil_metric_topk" in L.last_error()
    with pytest.raises(RuntimeError, match="stil_metric_binary"):
        L.metric_binary(P(dev(p)), P(dev(y)), -1, 0.5, P(cnt), _st())
    assert _read(into[0]) == want, "a refused call moved a counter"


# =====================================================================================================================
# stil_auroc
# =====================================================================================================================
def _auroc(L, s, y, K, short=0, ws_null=False, ld=None, expect_ok=True):
    """one call on [N, ld] scores -> (per-class words, macro word); outputs between sentinels, the workspace exactly
    stil_auroc_workspace_bytes long (minus `short`) with GUARD bytes behind it"""
    N = s.shape[0]
    ld = s.shape[1] if ld is None else ld
    nb = L.auroc_workspace_bytes(N, K)
    assert nb > 0 and nb % 256 == 0
    sd, yd = dev(s), dev(y)
    ws = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    per, macro = torch.full((K + 2,), SENT, device="cuda"), torch.full((3,), SENT, device="cuda")
    args = (P(sd), ld, P(yd), N, K, P(per[1:]), P(macro[1:]), None if ws_null else P(ws), nb - short, _st())
    if not expect_ok:
        with pytest.raises(RuntimeError, match="stil_auroc"):
            L.auroc(*args)
        assert "stil_auroc" in L.last_error()
    else:
        L.auroc(*args)
    torch.cuda.synchronize()
    assert float(per[0]) == SENT and float(per[K + 1]) == SENT, "a write beside per[K]"
    assert float(macro[0]) == SENT and float(macro[2]) == SENT, "a write beside macro"
    assert bool((ws[nb:] == 0xA5).all()), "a write behind the workspace"
    assert same_input(sd, s) and same_input(yd, y), "an input changed"
    if not expect_ok:
        assert bool((per == SENT).all()) and bool((macro == SENT).all()), "a refused call wrote an output"
        return None
    return f32bits(per[1:K + 1]), f32bits(macro[1:2])


@pytest.mark.parametrize("case", M.AUROC_TABLE, ids=M.auroc_id)
def test_auroc_equals_the_pair_count_bit_for_bit(L, case):
    s, y = M.auroc_case(case)
    per, macro, u2, n_pos, n_neg = M.auroc_expected(case)
    got_per, got_macro = _auroc(L, s, y, case.K)
    bad = [k for k in range(case.K) if got_per[k] != f32bits(per)[k]]
    print(f"AUROC {M.auroc_id(case)}: macro word {got_macro[0]:#x} want {f32bits([macro])[0]:#x}; classes that differ: {bad[:8]}")
    assert not bad, [(k, np.array(got_per[k], dtype=np.int32).view(np.float32).item(), float(per[k]), u2[k], n_pos[k], n_neg[k]) for k in bad[:8]]
    assert got_macro == f32bits([macro])
    assert _auroc(L, s, y, case.K) == (got_per, got_macro), "a second identical call differs"
    if case.pad:
        assert _auroc(L, s[:, :case.K].contiguous(), y, case.K) == (got_per, got_macro), "ld = K + 3 changes the result"


def test_auroc_workspace_bound_and_refusals(L):
    case = M.Auroc(257, 3, "tied", "random", 0)
    s, y = M.auroc_case(case)
    per, macro, *_ = M.auroc_expected(case)
    assert _auroc(L, s, y, 3) == (f32bits(per), f32bits([macro])), "at exactly stil_auroc_workspace_bytes"
    _auroc(L, s, y, 3, short=1, expect_ok=False)
    assert "workspace" in L.last_error()
    _auroc(L, s, y, 3, ws_null=True, expect_ok=False)
    _auroc(L, s, y, 3, ld=2, expect_ok=False)                      # ld < K
    for N, K, ld in ((257, 0, 3), (257, -1, 3), (0, 3, 3), (-1, 3, 3)):
        out = torch.full((8,), SENT, device="cuda")
        with pytest.raises(RuntimeError, match="stil_auroc: bad shape"):
            L.auroc(P(dev(s)), ld, P(dev(y)), N, K, P(out[1:]), P(out[6:]), P(out), 1 << 20, _st())
        assert "stil_auroc" in L.last_error() and bool((out == SENT).all())
    assert L.auroc_workspace_bytes(0, 3) == 0 and L.auroc_workspace_bytes(3, 0) == 0 and L.auroc_workspace_bytes(-1, 3) == 0
    assert L.auroc_workspace_bytes(1 << 16, 1 << 15) == 0 and L.auroc_workspace_bytes((1 << 16) - 1, 1 << 15) > 0      # N K = 2^31 is the limit
    sizes = [L.auroc_workspace_bytes(N, 3) for N in (1, 64, 257, 1025, 3073)]
    assert sizes == sorted(sizes) and all(b >= 3 * N * (4 + 4 + 1 + 1 + 4) for b, N in zip(sizes, (1, 64, 257, 1025, 3073)))


def test_auroc_nan_in_one_column_leaves_the_other_classes_alone(L):
    """out of contract, pinned only: the call returns, the NaN-free classes have the bits they have without the NaNs (every
    class is sorted and ranked in a segment of its own), the sentinels stand (checked in _auroc)"""
    dirty, clean, y = M.auroc_nan_column_case()
    K, col = dirty.shape[1], M.AUROC_NAN_COLUMN
    want = f32bits(M.auroc_reference(clean.numpy(), y.numpy(), K)[0])
    got_clean, _ = _auroc(L, clean, y, K)
    got_dirty, _ = _auroc(L, dirty, y, K)
    assert got_clean == want
    assert [w for k, w in enumerate(got_dirty) if k != col] == [w for k, w in enumerate(want) if k != col]


# =====================================================================================================================
# stil_tta_amd/metrics.py
# =====================================================================================================================
def _module_inputs():
    """-> (logits [300, 5] float64 signed tenths, labels [300]); every dtype below is a rounding of these"""
    g = M.gen(300, 5, 113)
    z = torch.round(torch.randn(300, 5, generator=g, dtype=torch.float64) * 2.0 * 1000.0) / 1000.0
    return z, torch.randint(0, 5, (300,), generator=g)


def _ratio(hits, n):
    """hits / n as Accuracy.compute() takes it: one fp32 division on the device"""
    return torch.tensor([hits], dtype=torch.float32, device="cuda") / torch.tensor([n], dtype=torch.float32, device="cuda")


def _expect_multiclass(z32, y, k):
    hits = int(M.topk_reference(z32, y, z32.shape[1], k).sum())
    per, macro, *_ = M.auroc_reference(z32.numpy(), y.numpy(), z32.shape[1])
    return hits, per, macro


@pytest.mark.parametrize("tdtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64, torch.float32])
def test_metrics_module_converts_to_fp32_then_counts(dtype, tdtype):
    """the documented conversion: scores .to(float32), targets .to(int64); fp16 / bf16 roundings collide, so ties are plenty"""
    from stil_tta_amd.metrics import AUROC, Accuracy
    z, y = _module_inputs()
    zc = z.to(dtype)
    z32 = zc.to(torch.float32)
    assert dtype in (torch.float32, torch.float64) or len(z32.unique()) < len(z.unique())
    for k in (1, 2):
        hits, per, macro = _expect_multiclass(z32, y, k)
        acc, auc = Accuracy("multiclass", 5, top_k=k), AUROC("multiclass", 5)
        for a, b in ((0, 100), (100, 100), (100, 300)):           # the middle update has no row
            acc(zc[a:b].cuda(), y[a:b].to(tdtype).cuda())
            auc(zc[a:b].cuda(), y[a:b].to(tdtype).cuda())
        assert acc.counts.cpu().tolist() == [hits, 300]
        assert f32bits(acc.compute()[None]) == f32bits(_ratio(hits, 300))
        assert f32bits(auc.compute()[None]) == f32bits([macro]) and f32bits(auc.per_class) == f32bits(per)
    # binary: column 0 as the score, threshold 0 and 0.5; bool targets
    p32 = z32[:, 0].contiguous()
    yb = y == 1
    for thr in (0.0, 0.5):
        acc = Accuracy("binary", threshold=thr)
        acc(zc.cuda()[:, 0], yb.cuda())                            # a non-contiguous column slice, bool targets
        want = int(M.binary_reference(p32.numpy(), yb.numpy().astype(np.int64), thr).sum())
        assert acc.counts.cpu().tolist() == [want, 300]
    auc = AUROC("binary")
    auc(zc.cuda()[:, 0], yb.cuda())
    per, macro, *_ = M.auroc_reference(p32.numpy()[:, None], yb.numpy().astype(np.int64), 1)
    assert f32bits(auc.compute()[None]) == f32bits([macro]) == f32bits(per)


def test_metrics_module_on_a_column_slice_of_a_wider_matrix():
    from stil_tta_amd.metrics import AUROC, Accuracy
    z, y = _module_inputs()
    wide = torch.cat([torch.full((300, 2), float("inf"), dtype=torch.float64), z, torch.full((300, 2), float("nan"), dtype=torch.float64)], 1).to(torch.float32).cuda()
    view = wide[:, 2:7]
    assert not view.is_contiguous()
    hits, per, macro = _expect_multiclass(z.to(torch.float32), y, 1)
    acc, auc = Accuracy("multiclass", 5), AUROC("multiclass", 5)
    acc(view, y.cuda()); auc(view, y.cuda())
    assert acc.counts.cpu().tolist() == [hits, 300]
    assert f32bits(auc.compute()[None]) == f32bits([macro]) and f32bits(auc.per_class) == f32bits(per)


@pytest.mark.parametrize("reserved", [False, True])
def test_a_zero_row_update_alone_says_that_no_rows_arrived(reserved):
    from stil_tta_amd.metrics import AUROC
    for task, K in (("multiclass", 5), ("binary", 1)):
        auc = AUROC(task, num_classes=K)
        if reserved:
            auc.reserve(16, "cuda")
        empty = torch.zeros((0, K) if K > 1 else (0,), device="cuda")
        auc(empty, torch.zeros(0, dtype=torch.int64, device="cuda"))
        with pytest.raises(RuntimeError, match="no rows arrived"):
            auc.compute()
        z, y = _module_inputs()
        s = z[:9].float() if K > 1 else z[:9, 0].float()
        auc(s.cuda(), (y[:9] % 2).cuda())
        auc(empty, torch.zeros(0, dtype=torch.int64, device="cuda"))
        per, macro, *_ = M.auroc_reference(s.reshape(9, -1).numpy(), (y[:9] % 2).numpy(), K)
        assert f32bits(auc.compute()[None]) == f32bits([macro]) and f32bits(auc.per_class) == f32bits(per)
        auc.reset()
        with pytest.raises(RuntimeError, match="no rows arrived"):
            auc.compute()


# =====================================================================================================================
# two ranks (gloo, sharing the one GPU): the all-reduce of Accuracy.compute, the ragged gather of AUROC.compute
# =====================================================================================================================
def _rank_inputs():
    """-> (scores [42, 5] signed tenths, labels [42], binary scores [42], binary labels [42]); rank 0 takes the first 37 rows"""
    g = M.gen(sum(SHARDS), 5, 127)
    z = (torch.round(torch.randn(sum(SHARDS), 5, generator=g) * 10.0) / 10.0).to(torch.float32)
    y = torch.randint(0, 5, (sum(SHARDS),), generator=g)
    return z, y, z[:, 0].contiguous(), (y == 1).to(torch.int64)


def _feed(rows, reserved, empty_rank1=False, rank=0):
    """the four metrics over this process's rows, in two updates -> dict of host results"""
    from stil_tta_amd.metrics import AUROC, Accuracy
    z, y, zb, yb = (t[rows] for t in _rank_inputs())
    acc, acc5, accb = Accuracy("multiclass", 5), Accuracy("multiclass", 5, top_k=2), Accuracy("binary", threshold=0.0)
    auc, aucb = AUROC("multiclass", 5), AUROC("binary")
    if reserved:
        auc.reserve(64, "cuda"); aucb.reserve(64, "cuda")
    half = len(z) // 2
    for sl in ([] if (empty_rank1 and rank == 1) else [slice(0, half), slice(half, len(z))]):
        zd, yd, zbd, ybd = z[sl].cuda(), y[sl].cuda(), zb[sl].cuda(), yb[sl].cuda()
        acc(zd, yd); acc5(zd, yd); accb(zbd, ybd); auc(zd, yd); aucb(zbd, ybd)
    out = dict(acc=acc.compute(), acc5=acc5.compute(), accb=accb.compute(), auc=auc.compute(), aucb=aucb.compute())
    out.update(per=auc.per_class, perb=aucb.per_class)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().reshape(-1) for k, v in out.items()}


def _metrics_worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      STIL_DIST_BACKEND="gloo", STIL_DIST_TIMEOUT_S="120")
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from stil_tta_amd.driver import init_distributed
    init_distributed()
    rows = slice(0, SHARDS[0]) if rank == 0 else slice(SHARDS[0], sum(SHARDS))
    out = {}
    for reserved in (False, True):
        out[f"ragged_{int(reserved)}"] = _feed(rows, reserved, rank=rank)
        out[f"empty_{int(reserved)}"] = _feed(rows, reserved, empty_rank1=True, rank=rank)
    # nothing anywhere: every rank gets the error, after the size gather (no rank is left waiting in a collective)
    from stil_tta_amd.metrics import AUROC
    try:
        AUROC("multiclass", 5).compute()
        out["nothing"] = "no error"
    except RuntimeError as e:
        out["nothing"] = str(e)
    torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_metrics_equal_one_process_on_the_concatenation():
    """ragged shards (37 and 5 rows), list mode and reserved mode: both ranks hold, bit for bit, what one process computes on
    the rank-ordered concatenation; with rank 1 holding no rows, what rank 0's rows alone give -- and rank 1 takes part in the
    collectives instead of raising while rank 0 waits."""
    from test_gpu_dp import _run_pair
    with tempfile.TemporaryDirectory() as td:
        r0, r1 = _run_pair(_metrics_worker, td)
    whole, first = _feed(slice(0, sum(SHARDS)), False), _feed(slice(0, SHARDS[0]), False)
    z, y, zb, yb = _rank_inputs()
    for ref, n in ((whole, sum(SHARDS)), (first, SHARDS[0])):     # the single process itself against the references
        per, macro, *_ = M.auroc_reference(z[:n].numpy(), y[:n].numpy(), 5)
        assert f32bits(ref["auc"]) == f32bits([macro]) and f32bits(ref["per"]) == f32bits(per)
        hits = int(M.topk_reference(z[:n], y[:n], 5, 1).sum())
        assert f32bits(ref["acc"]) == f32bits(_ratio(hits, n))
    for reserved in (0, 1):
        for key, ref in ((f"ragged_{reserved}", whole), (f"empty_{reserved}", first)):
            for r in (r0, r1):
                assert {k: f32bits(v) for k, v in r[key].items()} == {k: f32bits(v) for k, v in ref.items()}, (key, reserved)
    assert "no rows arrived" in r0["nothing"] and "no rows arrived" in r1["nothing"]
