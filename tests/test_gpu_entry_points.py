"""Direct tests of the C-ABI entry points that the operator suite reaches only through whole steps (include/stil_hip.h):
every test calls the entry point (through `_lib.lib()` or its `ops` wrapper) and compares with a reference written here in
float64 or integer arithmetic -- a Python model for the device-state kernels (exact), the torch expression in float64 for the
row kernels (the suite's `close()` at `TOL`), never another kernel of the library unless bit-equality with that kernel is the
claim under test (stil_queue_mean == stil_colsum).  Inputs come from seeded generators; the shapes are the edges the golden
steps never visit (K = 1 / 2, K above one block's width, `ld > K` views, half-full and wrapping rings, an overflowing store).

Every "bad argument" case below is rejected by the entry point's STIL_REQUIRE on the host before any launch; stray writes are
detected with sentinel-filled buffers, unread rows hold NaN.  tests/test_entry_point_inputs_cpu.py checks on the CPU that fp32
ATen meets `TOL` against the same float64 references on every row-loss input chosen here (no ill-conditioned case)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_ops import TOL, close  # noqa: E402  (the suite's tolerance and comparison, unchanged)

pytestmark = pytest.mark.gpu

SENT = -777.0
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from stil_tta_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from stil_tta_amd._lib import lib
    return lib()


def _st():
    from stil_tta_amd.ops import _stream
    return _stream()


def P(t):
    return None if t is None else t.data_ptr()


_KEEP = []


def dev(t):
    """a contiguous CUDA copy that stays alive until the test ends: the entry points take raw addresses, and a temporary freed
    right after its address was read would hand the same memory to the next operand"""
    _KEEP.append(t.cuda().contiguous())
    return _KEEP[-1]


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    _KEEP.clear()


def gen(*key):
    g = torch.Generator()
    g.manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) % (2 ** 31))
    return g


def strided(t, pad=3, fill=NAN):
    """[rows, K] -> a CUDA view with leading dimension K + pad whose padding holds `fill` (NaN: a read past K poisons the row)."""
    rows, K = t.shape
    buf = torch.full((rows, K + pad), fill, dtype=t.dtype)
    buf[:, :K] = t
    buf = buf.cuda()
    return buf, buf[:, :K]


def out_strided(rows, K, pad=3):
    buf = torch.full((rows, K + pad), SENT, device="cuda")
    return buf, buf[:, :K]


def rel_close(a, b, name):
    """|a - b| <= TOL * max|b|: for rows whose magnitude is far below 1, where close()'s `1 +` term would accept anything"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert err <= TOL * scale, f"{name}: max err {err:.3e} (scale {scale:.3e})"


# =====================================================================================================================
# device state (csrc/state.hip): exact comparisons with a Python model
# =====================================================================================================================
class RingModel:
    """The ring of include/stil_hip.h in numpy: bank as [Q, D] slots, an integer pointer, an integer count."""

    def __init__(self, Q, D, ptr=0, count=0):
        self.Q, self.D, self.ptr, self.count = Q, D, ptr, count
        self.slots = np.full((Q, D), SENT, dtype=np.float32)
        self.events = set()

    def enqueue(self, rows, mode, advance, with_count):
        Q, n = self.Q, rows.shape[0]
        p = self.ptr % Q                      # Python's %: already in [0, Q)
        m = min(n, Q - p) if mode == 0 else n
        self.slots[(p + np.arange(m)) % Q] = rows[:m]
        if self.ptr < 0:
            self.events.add("negative pointer")
        if self.ptr >= Q:
            self.events.add("pointer >= Q")
        if n == Q:
            self.events.add("n == Q")
        if p + n == Q:
            self.events.add("ends at the ring end")
        if p + n > Q:
            self.events.add("truncated" if mode == 0 else "wrapped mid-batch")
        if advance:
            self.ptr = (p + m) % Q
            if with_count:
                if self.count + m >= Q:
                    self.events.add("count saturated")
                self.count = min(self.count + m, Q)

    def bank(self, layout):
        return self.slots.T.copy() if layout else self.slots.copy()


# (Q, D, [(pointer to set before the call or None, n), ...]): >= 12 enqueues each
RING_SCENARIOS = {
    "Q40_D5": (40, 5, [(None, 7), (None, 40), (10, 30), (35, 9), (-3, 2), (85, 4), (None, 1), (None, 13), (None, 17), (None, 11),
                       (39, 1), (None, 40), (None, 6)]),
    "Q64_D1": (64, 1, [(None, 5), (None, 64), (60, 4), (60, 10), (-1, 3), (64 * 3 + 2, 7), (None, 1), (None, 33), (None, 31),
                       (None, 64), (63, 1), (None, 20)]),
    # n * D = 2050 * 130 = 266500 > 1024 blocks x 256 threads: the grid-stride loop takes a second trip
    "Q2100_D130": (2100, 130, [(None, 2050), (None, 2100), (100, 2000), (2000, 500), (-2105, 10), (4300, 50), (None, 1), (None, 700),
                               (None, 1400), (None, 2100), (2099, 1), (None, 2050)]),
}


@pytest.mark.parametrize("with_count", [0, 1])
@pytest.mark.parametrize("advance", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("scenario", sorted(RING_SCENARIOS))
def test_ring_enqueue_matches_python_ring(L, scenario, layout, mode, advance, with_count):
    """stil_ring_enqueue against RingModel after EVERY enqueue: the whole bank (sentinel-filled: a stray write shows), the
    pointer and the count.  advance = 0 must leave pointer and count alone (match.py / mmatch.py write two banks at one
    position that way)."""
    Q, D, steps = RING_SCENARIOS[scenario]
    assert len(steps) >= 12
    model = RingModel(Q, D)
    bank = torch.full((D, Q) if layout else (Q, D), SENT, device="cuda")
    ptr = torch.zeros(1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    base = 1.0
    for i, (setp, n) in enumerate(steps):
        if setp is not None:
            ptr.fill_(setp)
            model.ptr = setp
        rows = (base + np.arange(n * D, dtype=np.float64)).astype(np.float32).reshape(n, D)   # distinct, exact in fp32
        base += n * D
        assert base < 2 ** 24
        r = torch.from_numpy(rows).cuda()
        L.ring_enqueue(P(bank), P(r), n, D, Q, layout, mode, P(ptr), P(cnt) if with_count else None, advance, _st())
        model.enqueue(rows, mode, advance, with_count)
        torch.cuda.synchronize()
        assert torch.equal(bank.cpu(), torch.from_numpy(model.bank(layout))), f"bank differs after enqueue {i} (n={n}, set pointer {setp})"
        assert int(ptr.item()) == model.ptr, f"pointer {int(ptr.item())} != {model.ptr} after enqueue {i}"
        assert int(cnt.item()) == model.count, f"count {int(cnt.item())} != {model.count} after enqueue {i}"
    need = {"n == Q", "ends at the ring end", "negative pointer", "pointer >= Q", "truncated" if mode == 0 else "wrapped mid-batch"}
    if advance and with_count:
        need.add("count saturated")
    assert need <= model.events, f"the sequence missed {need - model.events}"
    if not (advance and with_count):
        assert model.count == 0


def test_ring_enqueue_rejects_bad_arguments_before_any_write(L):
    Q, D = 16, 3
    bank = torch.full((Q, D), SENT, device="cuda")
    rows = torch.ones(Q + 1, D, device="cuda")
    ptr = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):
        L.ring_enqueue(P(bank), P(rows), Q + 1, D, Q, 0, 1, P(ptr), None, 1, _st())     # wrapping more rows than slots
    with pytest.raises(RuntimeError):
        L.ring_enqueue(P(bank), P(rows), 4, D, Q, 2, 0, P(ptr), None, 1, _st())         # layout 2
    with pytest.raises(RuntimeError):
        L.ring_enqueue(P(bank), P(rows), 4, D, Q, 0, 0, None, None, 1, _st())           # null pointer to the position
    torch.cuda.synchronize()
    assert bool((bank == SENT).all()) and int(ptr.item()) == 0


QM_L = 1152
QM_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1151, QM_L)


@pytest.mark.parametrize("K", [1, 2, 5, 64, 65, 286, 300])
def test_queue_mean_is_colsum_bit_for_bit_and_the_float64_mean(L, ops, K):
    """state.hip: "the bits of stil_colsum with M = r and scale = 1 / r".  Rows at and beyond `count` hold NaN (and so do guard
    rows beyond L): reading one row too many fails.  colsum gets the same fp32 scale the kernel forms, (float)(1.0 / (double)M),
    so the comparison pins the association of the sums and not a rounding of the scale."""
    base = torch.randn(QM_L + 8, K, generator=gen(K, 3)) + 0.25
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    for count in QM_COUNTS:
        q = base.clone()
        q[count:] = NAN
        qd = q.cuda()
        cnt.fill_(count)
        out = torch.full((K,), SENT, device="cuda")
        L.queue_mean(P(qd), QM_L, K, P(cnt), P(out), _st())
        ref = torch.full((K,), SENT, device="cuda")
        ops.colsum(qd, ref, count, K, scale=float(np.float32(1.0 / count)))
        torch.cuda.synchronize()
        assert torch.equal(out, ref), f"count={count}: queue_mean differs from colsum by {float((out - ref).abs().max()):.3e}"
        close(out, q[:count].double().mean(0), name=f"queue_mean count={count} K={K}")


def test_queue_mean_clamps_the_count(L):
    K = 37
    q = torch.randn(QM_L + 8, K, generator=gen(5))
    q[QM_L:] = NAN                                      # guard rows: a kernel that trusts count > L reads NaN, not foreign memory
    qd = q.cuda()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    outs = {}
    for count in (0, -1, -(2 ** 40), QM_L, QM_L + 1, 2 ** 40):
        cnt.fill_(count)
        out = torch.full((K,), SENT, device="cuda")
        L.queue_mean(P(qd), QM_L, K, P(cnt), P(out), _st())
        outs[count] = out.cpu()
    for count in (0, -1, -(2 ** 40)):
        assert torch.equal(outs[count], torch.zeros(K)), count
    close(outs[QM_L], q[:QM_L].double().mean(0), name="full queue")
    assert torch.equal(outs[QM_L + 1], outs[QM_L]) and torch.equal(outs[2 ** 40], outs[QM_L])


# (K, capacity, batch sizes): a batch that straddles the capacity, then batches that start past it
ROWS_APPEND_SCENARIOS = {
    "K1": (1, 50, [7, 20, 1, 15, 12, 4, 1]),
    "K286": (286, 50, [7, 20, 1, 15, 12, 4, 1]),
    "K286_grid_stride": (286, 1500, [1000, 300, 400, 10]),      # 1000 x 286 elements: more than one trip of the copy loop
}


@pytest.mark.parametrize("scenario", sorted(ROWS_APPEND_SCENARIOS))
def test_rows_append_matches_python_store(L, scenario):
    K, cap, batches = ROWS_APPEND_SCENARIOS[scenario]
    sc = torch.full((cap, K), SENT, device="cuda")
    tg = torch.full((cap,), -5, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    m_sc, m_tg, m_cnt, m_ovf = np.full((cap, K), SENT, np.float32), np.full((cap,), -5, np.int64), 0, 0
    base, straddled, past = 1.0, False, False
    for i, n in enumerate(batches):
        src = (base + np.arange(n * K, dtype=np.float64)).astype(np.float32).reshape(n, K)
        tgt = (1000 * (i + 1) + np.arange(n)).astype(np.int64)
        base += n * K
        assert base < 2 ** 24
        L.rows_append(P(dev(torch.from_numpy(src))), P(dev(torch.from_numpy(tgt))), n, K, P(sc), P(tg), cap, P(cnt), P(ovf), _st())
        fit = max(0, min(n, cap - m_cnt))
        straddled |= 0 < fit < n
        past |= m_cnt >= cap
        m_sc[m_cnt:m_cnt + fit], m_tg[m_cnt:m_cnt + fit] = src[:fit], tgt[:fit]
        m_cnt += n
        m_ovf = 1 if m_cnt > cap else m_ovf
        torch.cuda.synchronize()
        assert torch.equal(sc.cpu(), torch.from_numpy(m_sc)), f"scores differ after batch {i} (n={n})"
        assert torch.equal(tg.cpu(), torch.from_numpy(m_tg)), f"targets differ after batch {i} (n={n})"
        assert int(cnt.item()) == m_cnt and int(ovf.item()) == m_ovf, (i, int(cnt.item()), m_cnt, int(ovf.item()), m_ovf)
    assert straddled and past and m_ovf == 1


@pytest.mark.parametrize("task,K", [("binary", 1), ("multiclass", 5)])
def test_auroc_reserved_store_equals_the_list_mode_and_raises_after_overflow(task, K):
    from stil_tta_amd.metrics import AUROC
    g = gen(K, 17)
    a, b = AUROC(task, num_classes=K), AUROC(task, num_classes=K)
    b.reserve(100, "cuda")
    for n in (13, 1, 40, 46):                                                    # exactly 100 rows: full, not overflowed
        s = torch.rand(n, generator=g) if task == "binary" else torch.softmax(torch.randn(n, K, generator=g), 1)
        y = torch.randint(0, 2 if task == "binary" else K, (n,), generator=g)
        a.update(s.cuda(), y.cuda())
        b.update(s.cuda(), y.cuda())
    va, vb = a.compute(), b.compute()
    assert torch.equal(va, vb) and torch.equal(a.per_class, b.per_class)
    s = torch.rand(1, generator=g) if task == "binary" else torch.softmax(torch.randn(1, K, generator=g), 1)
    b.update(s.cuda(), torch.zeros(1, dtype=torch.int64).cuda())
    with pytest.raises(RuntimeError):
        b.compute()
    b.reset()
    b.update(s.cuda().repeat(4, *([1] * (s.dim() - 1))), torch.tensor([0, 1, 0, 1]).cuda())
    assert torch.isfinite(b.compute())


# =====================================================================================================================
# small step kernels: float64 / integer references
# =====================================================================================================================
@pytest.mark.parametrize("K", [2, 5, 286, 300, 1000])
@pytest.mark.parametrize("rows", [1, 37, 256])
def test_da_apply(L, rows, K):
    g = gen(rows, K)
    p = torch.softmax(2 * torch.randn(rows, K, generator=g), 1)
    qm = torch.exp(torch.linspace(np.log(1e-4), 0.0, K))[torch.randperm(K, generator=g)]       # 1e-4 ... 1
    out = torch.full((rows, K), SENT, device="cuda")
    L.da_apply(P(dev(p)), P(dev(qm)), P(out), rows, K, _st())
    r = p.double() / qm.double()
    close(out, r / r.sum(1, keepdim=True), name="da_apply")
    close(out.double().sum(1), torch.ones(rows, dtype=torch.float64), name="row sums")


@pytest.mark.parametrize("Dp", [128, 100])
@pytest.mark.parametrize("K", [2, 11, 286])
def test_proto_add_and_commit(L, K, Dp):
    """stil_proto_add accumulates [K, Dp + 1] blocks (last column = counts); stil_proto_commit divides where count >= 1, leaves
    the other classes' prototypes bit for bit, counts them in the caller-zeroed `bad`, and does NOT clear the accumulators
    (STiLModel's epoch-end hook does)."""
    g = gen(K, Dp)
    psum = torch.randn(K, Dp, generator=g)
    pcnt = torch.randint(0, 5, (K,), generator=g).float()
    dsum, dcnt = dev(psum), dev(pcnt)
    s64, c64 = psum.double(), pcnt.double()
    for _ in range(3):
        cs = torch.cat([torch.randn(K, Dp, generator=g), torch.randint(0, 9, (K, 1), generator=g).float() / 2.0], 1)
        L.proto_add(P(dev(cs)), P(dsum), P(dcnt), K, Dp, _st())
        s64, c64 = s64 + cs[:, :Dp].double(), c64 + cs[:, Dp].double()
    close(dsum, s64, name="prototypes_sum")
    close(dcnt, c64, name="prototypes_count_sum")
    for nbad in sorted({0, 1, min(3, K)}):
        cnt = dcnt.clone().clamp_(min=1.0)
        bad_classes = torch.randperm(K, generator=g)[:nbad]
        for j, k in enumerate(bad_classes.tolist()):
            cnt[k] = (0.0, 0.5, 0.999)[j % 3]                    # every count below one is "no confident sample"
        protos0 = torch.randn(K, Dp, generator=g)
        protos = dev(protos0)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        s_before, c_before = dsum.clone(), cnt.clone()
        L.proto_commit(P(protos), P(dsum), P(cnt), P(bad), K, Dp, _st())
        torch.cuda.synchronize()
        assert int(bad.item()) == nbad
        good = torch.ones(K, dtype=torch.bool)
        good[bad_classes] = False
        close(protos.cpu()[good], dsum.cpu().double()[good] / cnt.cpu().double()[good, None], name="prototypes")
        assert torch.equal(protos.cpu()[~good], protos0[~good]), "a class without a confident sample must keep its prototype"
        assert torch.equal(dsum, s_before) and torch.equal(cnt, c_before), "commit leaves the accumulators to the caller"


@pytest.mark.parametrize("ld", [2, 4])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 5000])
def test_flag_ratios(L, rows, ld):
    """flag_ratios_kernel counts in integers and divides once: the five outputs are fp32(count) / fp32(rows) exactly."""
    g = gen(rows, ld)
    flags = torch.randint(1, 5, (rows, ld), generator=g).to(torch.uint8)        # columns 2, 3 (ld = 4): case-like noise
    flags[:, 1] = (torch.rand(rows, generator=g) < 0.3).to(torch.uint8)
    out = torch.full((5,), SENT, device="cuda")
    L.flag_ratios(P(dev(flags)), ld, rows, P(out), _st())
    f = flags.numpy().astype(np.int64)
    counts = [int((f[:, 1] != 0).sum())] + [int((f[:, 0] == c).sum()) for c in (1, 2, 3, 4)]
    ref = np.array([np.float32(c) / np.float32(rows) for c in counts], dtype=np.float32)
    assert sum(counts[1:]) == rows
    assert torch.equal(out.cpu(), torch.from_numpy(ref)), (out.cpu().tolist(), ref.tolist())


EMA_SPECIAL = [0, 1, -1, 29, -29, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, -(2 ** 24) - 1, 10 ** 6, -(10 ** 6), 7]


@pytest.mark.parametrize("m", [0.996, 0.999])
@pytest.mark.parametrize("n", [0, 1, 12, 255, 256, 257])
def test_ema_int_trunc(L, n, m):
    """The reference's EMA on an int64 buffer, evaluated by torch on the CPU exactly as it writes it: `v_ema * m + (1 - m) *
    v_main` in float32, truncated toward zero by the copy back."""
    g = gen(n, int(m * 1000))
    sp = torch.tensor(EMA_SPECIAL, dtype=torch.int64)
    e = torch.randint(-2000, 2000, (n + 1,), generator=g)
    v = torch.randint(-2000, 2000, (n + 1,), generator=g)
    k = min(n, sp.numel())
    e[:k], v[:k] = sp[:k], sp.flip(0)[:k]                       # specials against specials
    if n >= 3 * sp.numel():
        v[k:2 * k] = sp                                         # specials on the model side against small ema values
        e[2 * k:3 * k] = sp                                     # and the other way round
    ref = e.clone()
    ref.copy_(ref * m + (1 - m) * v)
    assert ref.dtype == torch.int64 and (e * m).dtype == torch.float32
    de = dev(e)
    L.ema_int_trunc(P(de), P(dev(v)), n, m, _st())
    ref[n:] = e[n:]                                             # the element past n is not touched
    assert torch.equal(de.cpu(), ref), (de.cpu() - ref).abs().max()


@pytest.mark.parametrize("C", [1, 64, 100, 2048])
def test_bn_eval_affine(L, C):
    """ab = [a, beta, running_mean] with a = gamma / sqrt(var + eps); the epilogue applies (y - mean) * a + beta, so the affine
    the three rows define is y * a + b with b = beta - mean * a: both a and that b against float64."""
    g = gen(C)
    gamma, beta, mean = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)
    var = torch.rand(C, generator=g) * 2
    var[0] = 0.0
    gamma[-1] = -abs(gamma[-1]) - 0.5
    eps = 1e-5
    ab = torch.full((3, C), SENT, device="cuda")
    L.bn_eval_affine(P(dev(gamma)), P(dev(beta)), P(dev(mean)), P(dev(var)), P(ab), C, eps, _st())
    a64 = gamma.double() / torch.sqrt(var.double() + float(np.float32(eps)))
    close(ab[0], a64, name="a")
    assert torch.equal(ab[1].cpu(), beta) and torch.equal(ab[2].cpu(), mean)
    close(ab[1].cpu().double() - ab[2].cpu().double() * ab[0].cpu().double(), beta.double() - mean.double() * a64, name="b")


def _drop_add_inputs(n, rowlen, seed):
    g = gen(n, rowlen, seed)
    x, resid = torch.randn(n, generator=g), torch.randn(n, generator=g)
    emask = (torch.rand(n, generator=g) >= 0.1).to(torch.uint8)
    rmask = (torch.rand(n // rowlen, generator=g) >= 0.3).to(torch.uint8)
    return x, resid, emask, rmask


def _offset_copy(t, off):
    """a CUDA copy of the 1-d tensor t that starts `off` elements into its allocation (misaligned for 16-byte / 4-byte loads)"""
    buf = torch.empty(t.numel() + off + 4, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()]
    v.copy_(t)
    return v


@pytest.mark.parametrize("path", ["vector", "scalar_rowlen7", "scalar_x_offset", "scalar_emask_offset"])
def test_drop_add_both_paths_all_operand_combinations(L, path):
    """out = resid + x * k, k in {0, scale}: the 16-byte path (n, rowlen % 4 == 0, aligned operands) and the scalar one, with
    every combination of resid / emask / rmask present or null.  Against float64 at TOL (the multiply-add may be contracted);
    without resid the result is ONE fp32 product and must be exact; dropped elements are exactly resid (or 0)."""
    rowlen = 7 if path == "scalar_rowlen7" else 64
    n = rowlen * 260                                           # vector path: 4160 float4s, more than one block
    scale = 1.0 / (1.0 - 0.1)
    sc32 = float(np.float32(scale))
    x, resid, emask, rmask = _drop_add_inputs(n, rowlen, 1)
    for use_r in (0, 1):
        for use_e in (0, 1):
            for use_m in (0, 1):
                if path == "scalar_emask_offset" and not use_e:
                    continue
                xd = _offset_copy(x, 1) if path == "scalar_x_offset" else dev(x)
                ed = None if not use_e else (_offset_copy(emask, 1) if path == "scalar_emask_offset" else dev(emask))
                rd = dev(resid) if use_r else None
                md = dev(rmask) if use_m else None
                assert (xd.data_ptr() % 16 != 0) == (path == "scalar_x_offset")
                assert ed is None or (ed.data_ptr() % 4 != 0) == (path == "scalar_emask_offset")
                out = torch.full((n,), SENT, device="cuda")
                L.drop_add(P(xd), P(rd), P(ed), P(md), P(out), n, rowlen, scale, _st())
                keep = torch.ones(n, dtype=torch.bool)
                if use_e:
                    keep &= emask.bool()
                if use_m:
                    keep &= rmask.bool().repeat_interleave(rowlen)
                k64 = keep.double() * sc32
                ref = x.double() * k64 + (resid.double() if use_r else 0.0)
                name = f"{path} resid={use_r} emask={use_e} rmask={use_m}"
                close(out, ref, name=name)
                o = out.cpu()
                assert torch.equal(o[~keep], resid[~keep] if use_r else torch.zeros(int((~keep).sum()))), name + ": dropped elements"
                if not use_r:
                    assert torch.equal(o[keep], (x * torch.tensor(sc32))[keep]), name + ": one fp32 product must be exact"


def test_drop_add_vector_and_scalar_paths_agree_bit_for_bit(L):
    rowlen, scale = 64, 1.0 / (1.0 - 0.25)
    n = rowlen * 130
    x, resid, emask, rmask = _drop_add_inputs(n, rowlen, 2)
    outs = []
    for xd in (dev(x), _offset_copy(x, 1)):                    # aligned: drop_add4_kernel; one float off: drop_add_kernel
        out = torch.full((n,), SENT, device="cuda")
        L.drop_add(P(xd), P(dev(resid)), P(dev(emask)), P(dev(rmask)), P(out), n, rowlen, scale, _st())
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]), f"paths differ by {float((outs[0] - outs[1]).abs().max()):.3e}"


@pytest.mark.parametrize("rowlen", [64, 7])
def test_drop_add_backward(ops, rowlen):
    n_rows, scale = 33, 1.0 / (1.0 - 0.2)
    x, resid, emask, rmask = _drop_add_inputs(n_rows * rowlen, rowlen, 3)
    go = torch.randn(n_rows, rowlen, generator=gen(rowlen, 9))
    x64 = x.double().view(n_rows, rowlen).requires_grad_()
    r64 = resid.double().view(n_rows, rowlen).requires_grad_()
    k64 = emask.double().view(n_rows, rowlen) * rmask.double()[:, None] * float(np.float32(scale))
    (x64 * k64 + r64).backward(go.double())
    xd, rd = dev(x.view(n_rows, rowlen)).requires_grad_(), dev(resid.view(n_rows, rowlen)).requires_grad_()
    out = ops.drop_add(xd, rd, dev(emask.view(n_rows, rowlen)), dev(rmask), rowlen, scale)
    out.backward(dev(go))
    close(out, (x64 * k64 + r64).detach(), name="drop_add")
    close(xd.grad, x64.grad, name="dx")
    assert torch.equal(rd.grad.cpu(), go)
    assert torch.equal(xd.grad.cpu(), (go * k64.float())), "dx is one fp32 product per element"


@pytest.mark.parametrize("n", [1, 255, 256, 1027, 100003])
def test_axpby_and_scale_dev(L, ops, n):
    g = gen(n)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a, b = 0.75, -1.3
    a32, b32 = float(np.float32(a)), float(np.float32(b))
    close(ops.axpby(dev(x), dev(y), a, b), a32 * x.double() + b32 * y.double(), name="axpby")
    o = ops.axpby(dev(x), None, a, b)
    assert torch.equal(o.cpu(), x * torch.tensor(a32)), "a * x + 0 is one fp32 product"
    gdev = torch.tensor([-0.37], device="cuda")
    out = torch.full((n,), SENT, device="cuda")
    L.scale_dev(P(dev(x)), P(gdev), 1.7, P(out), n, _st())
    s32 = np.float32(-0.37) * np.float32(1.7)                  # the kernel forms g * c once in fp32, then one product per element
    close(out, x.double() * float(np.float32(-0.37)) * float(np.float32(1.7)), name="scale_dev")
    assert torch.equal(out.cpu(), x * torch.tensor(float(s32)))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100003])
def test_reduce_sum(L, n, accumulate):
    x = torch.randn(max(n, 1), generator=gen(n)) + 0.1
    out = torch.tensor([2.5], device="cuda")
    L.reduce_sum(P(dev(x)), n, 0.3, P(out), accumulate, _st())
    ref = x[:n].double().sum() * float(np.float32(0.3)) + (2.5 if accumulate else 0.0)
    close(out, ref.reshape(1), name="reduce_sum")
    if n == 0:
        assert float(out) == (2.5 if accumulate else 0.0)
    again = torch.tensor([2.5], device="cuda")
    L.reduce_sum(P(dev(x)), n, 0.3, P(again), accumulate, _st())
    assert torch.equal(out, again)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("n", [1, 4, 1021, 1024, 70001, 70004])
@pytest.mark.parametrize("kind", [1, 2])
def test_act_bwd(L, kind, n, aligned):
    """kind 1: dx = dy * (relu_out > 0) (nothing flows at exactly 0); kind 2: dx = dy * gelu'(pre-activation), against float64
    autograd; n odd (scalar kernel), n % 4 == 0 (16-byte kernel) and n % 4 == 0 from a misaligned pointer (scalar again)."""
    g = gen(kind, n)
    pre, dy = 2.5 * torch.randn(n, generator=g), torch.randn(n, generator=g)
    pre[::5] = 0.0
    pre[1::7] = -0.0
    p64 = pre.double().requires_grad_()
    (F.relu(p64) if kind == 1 else F.gelu(p64)).backward(dy.double())
    ref_in = F.relu(pre) if kind == 1 else pre
    rd, dd = (dev(ref_in), dev(dy)) if aligned else (_offset_copy(ref_in, 1), _offset_copy(dy, 1))
    dx = torch.full((n,), SENT, device="cuda")
    L.act_bwd(P(dd), P(rd), P(dx), n, kind, _st())
    close(dx, p64.grad, name=f"act_bwd kind={kind}")
    if kind == 1:
        assert torch.equal(dx.cpu(), torch.where(pre > 0, dy, torch.zeros(n)))
    with pytest.raises(RuntimeError):
        L.act_bwd(P(dd), P(rd), P(dx), n, 3, _st())


@pytest.mark.parametrize("N", [1, 63, 64, 65, 286])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 127, 128, 129, 1025, 5000])
def test_colsum(ops, M, N):
    g = gen(M, N)
    ld = N + 5
    wide = torch.randn(M, ld, generator=g) + 0.5
    wide[:, N:] = NAN                                          # the columns outside the slice are never read
    wd = wide.cuda()
    X = wd[:, :N]
    scale = 0.37
    prev = torch.randn(N, generator=g)
    ref = wide[:, :N].double().sum(0)
    out = torch.full((N,), SENT, device="cuda")
    ops.colsum(X, out, M, N, ld=ld)
    close(out, ref, name="colsum")
    acc = dev(prev)
    ops.colsum(X, acc, M, N, ld=ld, accumulate=1, scale=scale)
    close(acc, prev.double() + float(np.float32(scale)) * ref, name="colsum accumulate")
    again, acc2 = torch.full((N,), SENT, device="cuda"), dev(prev)
    ops.colsum(X, again, M, N, ld=ld)
    ops.colsum(X, acc2, M, N, ld=ld, accumulate=1, scale=scale)
    assert torch.equal(out, again) and torch.equal(acc, acc2), "colsum is not bit-stable"
    dense = wide[:, :N].contiguous().cuda()
    out_d = torch.full((N,), SENT, device="cuda")
    ops.colsum(dense, out_d, M, N)
    assert torch.equal(out, out_d), "the leading dimension changed the sums"


# =====================================================================================================================
# row losses at the shapes the products use: float64 references.  Each case_* returns (inputs, ref) where ref(dtype) evaluates
# the torch expression on the CPU in that dtype; the GPU tests compare with ref(float64), the CPU test checks ref(float32).
# =====================================================================================================================
ROWS = (1, 13, 256)
KS = (1, 2, 3, 64, 255, 256, 257, 286, 513, 1000)
SCALES = (10.0, 30.0)
SPIKE = 88.0


def make_logits(rows, K, scale, *key):
    """logits scaled by 1 / T (T = 0.1: 10; 30 for headroom); with >= 13 rows, row 0 has all logits equal and row 1 one logit
    88 above the rest (softmax saturates to exactly one class); a single row is the saturated one at scale 30."""
    g = gen(rows, K, int(scale), *key)
    z = scale * torch.randn(rows, K, generator=g)
    spike_row = 1 if rows >= 13 else (0 if scale == 30.0 else None)
    if rows >= 13:
        z[0] = 1.5
    if spike_row is not None:
        z[spike_row] = 0.5 * torch.randn(K, generator=g)
        z[spike_row, K // 2] = z[spike_row].max() + SPIKE
    return z, g, spike_row


def case_ce_hard(rows, K, scale):
    z, g, _ = make_logits(rows, K, scale, 1)
    y = torch.randint(0, K, (rows,), generator=g)

    def ref(dtype):
        zz = z.to(dtype).requires_grad_()
        rl = F.cross_entropy(zz, y, reduction="none")
        rl.mean().backward()
        return {"row_loss": rl.detach(), "dlogits_x_rows": zz.grad * rows}
    return (z, y), ref


def case_ce_soft(rows, K, scale, weighted, normalised):
    z, g, _ = make_logits(rows, K, scale, 2, weighted, normalised)
    q = torch.softmax(torch.randn(rows, K, generator=g), 1) if normalised else 1.7 * torch.rand(rows, K, generator=g) / K ** 0.5
    w = None
    if weighted:
        w = torch.rand(rows, generator=g) + 0.25
        w[::3] = 0.0                                           # rows the confidence mask switches off

    def ref(dtype):
        zz = z.to(dtype).requires_grad_()
        rl = F.cross_entropy(zz, q.to(dtype), reduction="none")
        if w is not None:
            rl = rl * w.to(dtype)
        rl.mean().backward()
        return {"row_loss": rl.detach(), "dlogits_x_rows": zz.grad * rows}
    return (z, q, w), ref


def case_row_softmax(rows, K, scale):
    z, g, spike_row = make_logits(rows, K, scale, 3)
    go = torch.randn(rows, K, generator=g)

    def ref(dtype):
        zz = z.to(dtype).requires_grad_()
        p = torch.softmax(zz, 1)
        p.backward(go.to(dtype))
        return {"p": p.detach(), "dz": zz.grad}
    return (z, go, spike_row), ref


def case_proto_loss(rows, K, scale, Dp=128):
    """T = 1 / scale on unit-norm features and prototypes; with >= 13 rows, row 0 is the zero feature (all logits equal) and row 1
    a multiple of one prototype that puts its logit at least 88 above the rest."""
    g = gen(rows, K, int(scale), Dp, 4)
    T = 1.0 / scale
    feat = F.normalize(torch.randn(rows, Dp, generator=g))
    protos = F.normalize(torch.randn(K, Dp, generator=g))
    hard = torch.randint(0, K, (rows,), generator=g).to(torch.int32)
    conf = (torch.rand(rows, generator=g) >= 0.3).to(torch.uint8)
    if rows >= 13:
        feat[0] = 0.0
        cos = (protos @ protos[K // 2]).clone()
        cos[K // 2] = -1.0
        feat[1] = protos[K // 2] * (SPIKE * T / max(1e-3, 1.0 - float(cos.max())))
        conf[:2] = 1
        hard[1] = K // 2

    def ref(dtype):
        ff = feat.to(dtype).requires_grad_()
        p = torch.softmax(ff @ protos.to(dtype).t() / T, 1)
        rl = -torch.log(p[torch.arange(rows), hard.long()] + 1e-7) * conf.to(dtype)
        rl.mean().backward()
        return {"row_loss": rl.detach(), "dfeat_x_rows": ff.grad * rows}
    return (feat, protos, hard, conf, T), ref


L2_SPECIAL = 2          # with >= 13 rows: row 0 all zero (the eps = 1e-12 clamp), row 1 of norm 1e-20


def case_l2norm(rows, D, scale):
    g = gen(rows, D, int(scale), 5)
    x = scale * torch.randn(rows, D, generator=g)
    go = torch.randn(rows, D, generator=g)
    if rows >= 13:
        x[0] = 0.0
        x[1] = (F.normalize(torch.randn(1, D, generator=g).double()) * 1e-20).float()[0]

    def ref(dtype):
        xx = x.to(dtype).requires_grad_()
        y = F.normalize(xx, dim=1)
        y.backward(go.to(dtype))
        return {"y": y.detach(), "dx": xx.grad}
    return (x, go), ref


def tokmean_T(D):
    return 1 if D == 3 else (33 if D == 64 else 7)


def case_tokmean(B, D, scale):
    T = tokmean_T(D)
    g = gen(B, D, int(scale), T, 6)
    x = scale * torch.randn(B, T, D, generator=g)
    go = torch.randn(B, D, generator=g)

    def ref(dtype):
        xx = x.to(dtype).requires_grad_()
        y = xx.mean(1)
        y.backward(go.to(dtype))
        return {"y": y.detach(), "dx": xx.grad}
    return (x, go, T), ref


def case_geglu(rows, H, scale):
    g = gen(rows, H, int(scale), 7)
    h = (scale / 10.0) * torch.randn(rows, 2 * H, generator=g)         # gates spread over +-3 (scale 10) and +-9 (scale 30)
    go = torch.randn(rows, H, generator=g)

    def ref(dtype):
        hh = h.to(dtype).requires_grad_()
        a, gates = hh.chunk(2, -1)
        y = a * F.gelu(gates)
        y.backward(go.to(dtype))
        return {"y": y.detach(), "dh": hh.grad}
    return (h, go), ref


def proto_dps(K):
    return (128, 100) if K == 286 else (128,)


def row_loss_cases():
    """(name, builder, args) of every row-loss input of this module: the CPU test walks the same list."""
    out = []
    for rows in ROWS:
        for K in KS:
            for s in SCALES:
                out.append(("ce_hard", case_ce_hard, (rows, K, s)))
                for weighted in (0, 1):
                    for normalised in (0, 1):
                        out.append(("ce_soft", case_ce_soft, (rows, K, s, weighted, normalised)))
                out.append(("row_softmax", case_row_softmax, (rows, K, s)))
                for Dp in proto_dps(K):
                    out.append(("proto_loss", case_proto_loss, (rows, K, s, Dp)))
                out.append(("l2norm", case_l2norm, (rows, K, s)))
                out.append(("tokmean", case_tokmean, (rows, K, s)))
                out.append(("geglu", case_geglu, (rows, K, s)))
    out.append(("proto_loss", case_proto_loss, (2, PROTO_LOSS_KMAX, 10.0, 4)))
    return out


def close_rows(a, b, special, name):
    """close() on the ordinary rows together and on each of the first `special` rows by itself (their magnitudes differ from
    the others' by many orders: one scale for all would hide them)"""
    a, b = a.detach().cpu(), b.detach().cpu()
    for r in range(special):
        close(a[r], b[r], name=f"{name} row {r}")
    if a.shape[0] > special:
        close(a[special:], b[special:], name=name)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_ce_hard(L, rows, K):
    for scale in SCALES:
        (z, y), ref = case_ce_hard(rows, K, scale)
        r = ref(torch.float64)
        _, zv = strided(z)
        dzb, dzv = out_strided(rows, K)
        rl = torch.full((rows,), SENT, device="cuda")
        L.ce_hard(P(zv), K + 3, P(dev(y)), P(rl), P(dzv), K + 3, rows, K, 1.0 / rows, _st())
        close(rl, r["row_loss"], name=f"ce_hard row_loss scale={scale}")
        close(dzv * rows, r["dlogits_x_rows"], name=f"ce_hard dlogits scale={scale}")
        assert bool((dzb[:, K:] == SENT).all()), "dlogits written past K"
        rl2 = torch.full((rows,), SENT, device="cuda")
        L.ce_hard(P(dev(z)), K, P(dev(y)), P(rl2), None, K, rows, K, 1.0 / rows, _st())        # contiguous, no gradient wanted
        assert torch.equal(rl, rl2)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_ce_soft(L, rows, K):
    for scale in SCALES:
        for weighted in (0, 1):
            for normalised in (0, 1):
                (z, q, w), ref = case_ce_soft(rows, K, scale, weighted, normalised)
                r = ref(torch.float64)
                _, zv = strided(z)
                _, qv = strided(q)
                dzb, dzv = out_strided(rows, K)
                rl = torch.full((rows,), SENT, device="cuda")
                L.ce_soft(P(zv), K + 3, P(qv), K + 3, P(None if w is None else dev(w)), P(rl), P(dzv), K + 3, rows, K, 1.0 / rows, _st())
                name = f"ce_soft scale={scale} weighted={weighted} normalised={normalised}"
                close(rl, r["row_loss"], name=name + " row_loss")
                close(dzv * rows, r["dlogits_x_rows"], name=name + " dlogits")
                assert bool((dzb[:, K:] == SENT).all()), "dlogits written past K"
                if w is not None:
                    off = (w == 0)
                    assert bool((rl.cpu()[off] == 0).all()) and bool((dzv.cpu()[off] == 0).all()), "a zero row weight must switch the row off"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_row_softmax(L, rows, K):
    for scale in SCALES:
        (z, go, spike_row), ref = case_row_softmax(rows, K, scale)
        r = ref(torch.float64)
        p = torch.full((rows, K), SENT, device="cuda")
        L.row_softmax_fwd(P(dev(z)), P(p), rows, K, _st())
        close(p, r["p"], name=f"softmax scale={scale}")
        close(p.double().sum(1), torch.ones(rows, dtype=torch.float64), name="row sums")
        if spike_row is not None:
            pr = p[spike_row].cpu()
            assert float(pr[K // 2]) == 1.0 and float(pr.sum()) == 1.0, "a logit 88 above the rest takes the whole row"
        if rows >= 13:
            assert torch.equal(p[0].cpu(), torch.full((K,), float(p[0, 0]))), "equal logits give equal probabilities"
        dz = torch.full((rows, K), SENT, device="cuda")
        L.row_softmax_bwd(P(dev(go)), P(p), P(dz), rows, K, _st())
        close(dz, r["dz"], name=f"softmax bwd scale={scale}")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_proto_loss(L, rows, K):
    for scale in SCALES:
        for Dp in proto_dps(K):
            (feat, protos, hard, conf, T), ref = case_proto_loss(rows, K, scale, Dp)
            r = ref(torch.float64)
            rl = torch.full((rows,), SENT, device="cuda")
            df = torch.full((rows, Dp), SENT, device="cuda")
            L.proto_loss(P(dev(feat)), P(dev(protos)), P(dev(hard)), P(dev(conf)), P(rl), P(df), rows, K, Dp, T, _st())
            close(rl, r["row_loss"], name=f"proto_loss scale={scale} Dp={Dp}")
            close(df * rows, r["dfeat_x_rows"], name=f"proto_loss dfeat scale={scale} Dp={Dp}")
            off = conf == 0
            assert bool((rl.cpu()[off] == 0).all()) and bool((df.cpu()[off] == 0).all())


PROTO_LOSS_KMAX = 60 * 1024 // 4        # the guard: K floats of logits in at most 60 KiB of LDS


def test_proto_loss_at_its_lds_bound(L):
    rows, Dp = 2, 4
    (feat, protos, hard, conf, T), ref = case_proto_loss(rows, PROTO_LOSS_KMAX, 10.0, Dp)
    r = ref(torch.float64)
    rl = torch.full((rows,), SENT, device="cuda")
    df = torch.full((rows, Dp), SENT, device="cuda")
    L.proto_loss(P(dev(feat)), P(dev(protos)), P(dev(hard)), P(dev(conf)), P(rl), P(df), rows, PROTO_LOSS_KMAX, Dp, T, _st())
    close(rl, r["row_loss"], name="proto_loss at K max")
    close(df * rows, r["dfeat_x_rows"], name="proto_loss dfeat at K max")
    big = torch.zeros(PROTO_LOSS_KMAX + 1, Dp, device="cuda")
    rl.fill_(SENT)
    with pytest.raises(RuntimeError):
        L.proto_loss(P(dev(feat)), P(big), P(dev(hard)), P(dev(conf)), P(rl), P(df), rows, PROTO_LOSS_KMAX + 1, Dp, T, _st())
    assert bool((rl == SENT).all())


@pytest.mark.parametrize("D", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_l2norm(L, rows, D):
    for scale in SCALES:
        (x, go), ref = case_l2norm(rows, D, scale)
        r = ref(torch.float64)
        y = torch.full((rows, D), SENT, device="cuda")
        nrm = torch.full((rows,), SENT, device="cuda")
        L.l2norm_fwd(P(dev(x)), P(y), P(nrm), rows, D, _st())
        special = L2_SPECIAL if rows >= 13 else 0
        close_rows(y, r["y"], special, f"l2norm scale={scale}")
        close(nrm, x.double().norm(dim=1).clamp_min(1e-12), name="norms")
        dx = torch.full((rows, D), SENT, device="cuda")
        L.l2norm_bwd(P(dev(go)), P(y), P(nrm), P(dx), rows, D, _st())
        close_rows(dx, r["dx"], special, f"l2norm bwd scale={scale}")
        if special:
            assert torch.equal(y[0].cpu(), torch.zeros(D)) and bool(torch.isfinite(dx[:2]).all())
            rel_close(y[1], r["y"][1], "the row of norm 1e-20 (x / eps, ~1e-8)")
            rel_close(nrm[:2], torch.full((2,), 1e-12, dtype=torch.float64), "clamped norms")


@pytest.mark.parametrize("D", KS)
@pytest.mark.parametrize("B", ROWS)
def test_tokmean(L, B, D):
    for scale in SCALES:
        (x, go, T), ref = case_tokmean(B, D, scale)
        r = ref(torch.float64)
        y = torch.full((B, D), SENT, device="cuda")
        L.tokmean_fwd(P(dev(x)), P(y), B, T, D, _st())
        close(y, r["y"], name=f"tokmean T={T} scale={scale}")
        dx = torch.full((B, T, D), SENT, device="cuda")
        L.tokmean_bwd(P(dev(go)), P(dx), B, T, D, _st())
        close(dx, r["dx"], name=f"tokmean bwd T={T}")


@pytest.mark.parametrize("H", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_geglu(L, rows, H):
    for scale in SCALES:
        (h, go), ref = case_geglu(rows, H, scale)
        r = ref(torch.float64)
        y = torch.full((rows, H), SENT, device="cuda")
        L.geglu_fwd(P(dev(h)), P(y), rows, H, _st())
        close(y, r["y"], name=f"geglu scale={scale}")
        dh = torch.full((rows, 2 * H), SENT, device="cuda")
        L.geglu_bwd(P(dev(go)), P(dev(h)), P(dh), rows, H, _st())
        close(dh, r["dh"], name=f"geglu bwd scale={scale}")


def test_size_queries_and_library_info(L):
    """The sizes the header documents for the caller-owned workspaces ([chunks][N] partials of a column sum, [splits][N][K] slabs
    of a weight gradient, the tabular embedding's two [ncols + 1, D] planes), and the three informational entry points."""
    for M, N in [(1, 1), (127, 5), (128, 64), (129, 286), (5000, 65)]:
        assert L.colsum_chunks(M) == (M + 127) // 128
        assert L.colsum_workspace_bytes(M, N) == L.colsum_chunks(M) * N * 4
    for M, N, K in [(256, 64, 64), (6272, 256, 2304), (37, 7, 286)]:
        assert L.wgrad_splits(M, N, K, 0) >= 1
        assert L.wgrad_workspace_bytes(M, N, K, 0) == L.wgrad_splits(M, N, K, 0) * N * K * 4
    assert L.tab_embed_bwd_workspace_bytes(64, 512) == 2 * 65 * 512 * 4
    assert L.version() >= 100 and L.device_count() == torch.cuda.device_count()
    out = torch.zeros(5, device="cuda")
    with pytest.raises(RuntimeError, match="stil_flag_ratios"):
        L.flag_ratios(P(out), 1, 4, P(out), _st())               # ld < 2: rejected on the host
    assert "stil_flag_ratios" in L.last_error()


# =====================================================================================================================
# metrics
# =====================================================================================================================
def _topk(L, scores_view, ld, y, N, K, k):
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    L.metric_topk(P(scores_view), ld, P(y), N, K, k, P(cnt), _st())
    return cnt.cpu().tolist()


def test_metric_topk_on_a_column_slice_and_k_edges(L):
    """ld = K + 5 (the padding holds +inf: a read past K beats every target); k = K counts every row with a valid target; k > K
    is not rejected and equals k = K (fewer than k scores can beat the target either way); N = 0 leaves the counters alone."""
    from oracle import metrics_oracle as MO
    N, K = 203, 7
    g = gen(N, K)
    s = (torch.randn(N, K, generator=g) * 10).round() / 10              # one decimal: plenty of ties
    y = torch.randint(0, K, (N,), generator=g)
    _, sv = strided(s, pad=5, fill=float("inf"))
    yd = dev(y)
    for k in (1, 2, 5):
        hits, tot = _topk(L, sv, K + 5, yd, N, K, k)
        assert tot == N and hits == round(MO.topk_accuracy(s.numpy(), y.numpy(), k) * N), k
        assert [hits, tot] == _topk(L, dev(s), K, yd, N, K, k)
    assert _topk(L, sv, K + 5, yd, N, K, K) == [N, N]
    assert _topk(L, sv, K + 5, yd, N, K, K + 1) == [N, N] and _topk(L, sv, K + 5, yd, N, K, 1000) == [N, N]
    assert _topk(L, sv, K + 5, yd, 0, K, 1) == [0, 0]
    with pytest.raises(RuntimeError):
        _topk(L, sv, K - 1, yd, N, K, 1)                                # ld < K


def test_metric_binary_at_the_threshold(L):
    """(prob > threshold) == (target == 1), as oracle/metrics_oracle.py: a score exactly at the threshold is a negative."""
    from oracle import metrics_oracle as MO
    g = gen(99)
    N = 777
    p = torch.rand(N, generator=g)
    p[::4] = 0.5
    p[1::8] = float(np.nextafter(np.float32(0.5), np.float32(1)))
    p[2::8] = float(np.nextafter(np.float32(0.5), np.float32(0)))
    y = torch.randint(0, 2, (N,), generator=g)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    L.metric_binary(P(dev(p)), P(dev(y)), N, 0.5, P(cnt), _st())
    hits, tot = cnt.cpu().tolist()
    assert tot == N and hits == round(MO.binary_accuracy(p.numpy(), y.numpy(), 0.5) * N)
    at = p == 0.5
    expect = [int((y[at] == 0).sum()), int(at.sum())]
    cnt.zero_()
    L.metric_binary(P(dev(p[at])), P(dev(y[at])), int(at.sum()), 0.5, P(cnt), _st())
    assert cnt.cpu().tolist() == expect
    L.metric_binary(P(dev(p)), P(dev(y)), 0, 0.5, P(cnt), _st())                 # N = 0: nothing counted
    assert cnt.cpu().tolist() == expect


def _auroc(L, s, y):
    from stil_tta_amd.ops import _ws
    N, K = s.shape
    nb = L.auroc_workspace_bytes(N, K)
    assert nb > 0
    sd = dev(s)
    ws = _ws.get(nb, sd.device)
    per, macro = torch.full((K,), SENT, device="cuda"), torch.full((1,), SENT, device="cuda")
    L.auroc(P(sd), K, P(dev(y)), N, K, P(per), P(macro), P(ws), nb, _st())
    return per.cpu().double().numpy(), float(macro)


def test_auroc_single_row_and_all_scores_equal(L):
    from oracle import metrics_oracle as MO
    # N = 1: no class has both positives and negatives -> 0 everywhere
    per, macro = _auroc(L, torch.tensor([[0.2, 0.5, 0.3]]), torch.tensor([1]))
    assert per.tolist() == [0.0, 0.0, 0.0] and macro == 0.0
    per, macro = _auroc(L, torch.tensor([[0.7]]), torch.tensor([1]))
    assert per.tolist() == [0.0] and macro == 0.0
    # every score equal: each positive ties with every negative -> 0.5 for every class that is present, 0 for an absent one
    N, K = 64, 4
    y = torch.randint(0, K - 1, (N,), generator=gen(4))                 # class K - 1 is absent
    s = torch.full((N, K), 0.25)
    per, macro = _auroc(L, s, y)
    ref_macro, ref_per = MO.multiclass_auroc(s.numpy(), y.numpy())
    assert ref_per.tolist() == [0.5, 0.5, 0.5, 0.0]
    assert per.tolist() == ref_per.tolist() and macro == float(np.float32(ref_macro))
    yb = torch.randint(0, 2, (N,), generator=gen(6))
    per, macro = _auroc(L, torch.full((N, 1), 0.5), yb)
    assert per.tolist() == [0.5] and macro == 0.5 == MO.binary_auroc(np.full(N, 0.5), yb.numpy() == 1)
    with pytest.raises(RuntimeError):
        L.auroc(P(dev(s)), K, P(dev(y)), 0, K, None, None, None, 0, _st())      # N = 0 is rejected on the host


# =====================================================================================================================
# stil_tab_corrupt_draw: properties at every size, the exact draws of a Python model of the counter hash at the small ones
# =====================================================================================================================
_M64 = (1 << 64) - 1


def _aug_hash(seed, ctr):
    z = (seed + 0x9E3779B97F4A7C15 * (ctr + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return (z >> 16) & 0xFFFFFFFF


def _draw_model(B, n_cols, n_rows, k, seed, offset, step=0):
    """partial Fisher-Yates over the columns and k uniform rows per sample, as augment.hip documents it"""
    idx, pos = np.zeros((B, k), np.int32), np.zeros((B, k), np.int32)
    for b in range(B):
        base = (offset + step * 0x100000000 + b * 2 * k) & _M64
        perm = list(range(n_cols))
        for j in range(k):
            r = j + ((_aug_hash(seed, (base + j) & _M64) * (n_cols - j)) >> 32)
            perm[j], perm[r] = perm[r], perm[j]
        idx[b] = perm[:k]
        pos[b] = [(_aug_hash(seed, (base + k + j) & _M64) * n_rows) >> 32 for j in range(k)]
    return idx, pos


def _draw(L, B, n_cols, n_rows, k, seed, offset, step=None):
    idx = torch.full((B, k), -9, dtype=torch.int32, device="cuda")
    pos = torch.full((B, k), -9, dtype=torch.int32, device="cuda")
    L.tab_corrupt_draw(P(idx), P(pos), B, n_cols, n_rows, k, seed, offset, P(step), _st())
    return idx.cpu().numpy(), pos.cpu().numpy()


@pytest.mark.parametrize("k_full", [0, 1])
@pytest.mark.parametrize("n_cols", [1, 5, 64, 8192])
@pytest.mark.parametrize("B", [1, 64])
def test_tab_corrupt_draw(L, B, n_cols, k_full):
    k = n_cols if k_full else 1
    n_rows, seed = 1000, 2022
    drawn = 12345
    idx, pos = _draw(L, B, n_cols, n_rows, k, seed, drawn)
    assert idx.min() >= 0 and idx.max() < n_cols and pos.min() >= 0 and pos.max() < n_rows
    srt = np.sort(idx, axis=1)
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "a row drew the same column twice"
    if k == n_cols:
        assert bool((srt == np.arange(n_cols)[None]).all())
    idx2, pos2 = _draw(L, B, n_cols, n_rows, k, seed, drawn)
    assert np.array_equal(idx, idx2) and np.array_equal(pos, pos2), "the same (seed, drawn) must repeat the draws"
    nxt = drawn + B * 2 * k                                             # TabularCorruptor.drawn after this batch
    idx3, pos3 = _draw(L, B, n_cols, n_rows, k, seed, nxt)
    if B * k >= 4:
        assert not (np.array_equal(idx, idx3) and np.array_equal(pos, pos3)), "the next counter range repeated the draws"
    step = torch.tensor([3], dtype=torch.int64, device="cuda")
    idx4, pos4 = _draw(L, B, n_cols, n_rows, k, seed, drawn, step)
    if n_cols <= 64:
        for got, (o, s) in (((idx, pos), (drawn, 0)), ((idx3, pos3), (nxt, 0)), ((idx4, pos4), (drawn, 3))):
            mi, mp = _draw_model(B, n_cols, n_rows, k, seed, o, s)
            assert np.array_equal(got[0], mi) and np.array_equal(got[1], mp), (o, s)


def test_tab_corrupt_draw_rejects_more_than_8192_columns(L):
    idx = torch.full((1, 1), -9, dtype=torch.int32, device="cuda")
    pos = torch.full((1, 1), -9, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        L.tab_corrupt_draw(P(idx), P(pos), 1, 8193, 10, 1, 1, 0, None, _st())
    with pytest.raises(RuntimeError):
        L.tab_corrupt_draw(P(idx), P(pos), 1, 5, 10, 6, 1, 0, None, _st())      # k > n_cols
    torch.cuda.synchronize()
    assert int(idx[0, 0]) == -9 and int(pos[0, 0]) == -9
