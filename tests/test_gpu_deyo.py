"""DeYO test-time adaptation (Lee et al., ICLR 2024, "Entropy is not enough for test-time adaptation") in STiLModel.test_step:
a patch-shuffled second view and the PLPD selection on top of TENT (tests/test_gpu_tta.py), beside EATA (tests/test_gpu_eata.py).

1. stil_patch_shuffle bit for bit against its restatement as a torch index gather (vector and scalar path, patches that are no
   power of two), identity, out-of-range entries, sentinels, bad arguments.
2. stil_deyo_rows against float64 (close() at TOL of test_gpu_ops; decisions, counts, first maximum and gate exactly) on
   constructed inputs whose every decision is far from its threshold (tests/test_deyo_cpu.py checks that), ld = K + 3 views,
   sentinels, repetition, bad arguments, the n == 0 cases; tie to stil_eata_rows.
3. The step against the contract restated here in float64 on the oracle, on the device's ReLU / max-pool decisions of BOTH
   forwards.  The clean forward is traced inside the step.  The shuffled forward runs under no_grad, where the device keeps no
   decisions; the test repeats it with gradients on (a second model holding the same state, tta.adapting_pass on the shuffled
   images) and takes the decisions of that pass.  Classifier scaled as in tests/test_gpu_eata.py; tta_ent_margin /
   tta_plpd_margin placed by a float64 pre-pass in the widest gap of the sorted H, and of the PLPD of the reliable rows.
4. Properties: n == 0 batch, no weight-gradient product, no synchronisation beyond a "tent" step's, the permutation round
   trip and its generator, state rules, freeze() + inference_mode, fit.test."""
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_gpu_ops import TOL, close  # noqa: E402
from oracle import stil_oracle as O  # noqa: E402
import test_gpu_eata as E  # noqa: E402
import test_gpu_tta as T  # noqa: E402

SENTINEL = -7.25
ROWS = (1, 7, 512)
KS = (1, 2, 286, 1000)
VARIANTS = ("mixed", "none_reliable", "plpd_fails", "tied")
A_ENT, A_PLPD = 0.75, 1.25      # exact in float32
DEFAULT_PLPD = 0.2


# ------------------------------------------------------------------------------------------ check 1: the shuffle
SHUFFLE_CASES = [(1, 3, 8, 8, 4), (3, 3, 32, 32, 4), (2, 1, 12, 12, 3), (2, 3, 20, 20, 4), (2, 3, 64, 64, 4), (2, 3, 16, 16, 1)]


def shuffle_input(B, C, H, W, grid, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * B + 11 * H + grid)
    x = torch.randn(B, C, H, W, generator=g)
    perm = torch.stack([torch.randperm(grid * grid, generator=g) for _ in range(B)]).to(torch.int32)
    return x, perm


def shuffle_ref(x, grid, perm):
    """include/stil_deyo.h restated as one gather: dst[b, c, y, x] = src[b, c, (q / g) ph + y % ph, (q % g) pw + x % pw],
    q = perm[b, (y / ph) g + x / pw], and q = the slot itself where the entry is outside [0, g^2)."""
    B, C, H, W = x.shape
    ph, pw = H // grid, W // grid
    yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
    slot = (yy // ph) * grid + xx // pw                                  # [H, W]
    q = torch.as_tensor(perm).long()[:, slot]                            # [B, H, W]
    q = torch.where((q < 0) | (q >= grid * grid), slot.expand_as(q), q)
    idx = ((q // grid) * ph + yy % ph) * W + (q % grid) * pw + xx % pw
    return x.reshape(B, C, H * W).gather(2, idx.reshape(B, 1, H * W).expand(B, C, H * W)).reshape(B, C, H, W)


def _run_shuffle(L, x, grid, perm):
    """-> dst with one sentinel image before and one after it"""
    B, C, H, W = x.shape
    buf = torch.full((B + 2, C, H, W), SENTINEL, device="cuda")
    src = x.cuda().contiguous()
    pd = perm.to(torch.int32).cuda().contiguous()
    L.patch_shuffle(src.data_ptr(), buf[1:].data_ptr(), B, C, H, W, grid, pd.data_ptr(), None)
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), x), "the source changed"
    return buf.cpu()


@pytest.mark.parametrize("B,C,H,W,grid", SHUFFLE_CASES)
def test_patch_shuffle_is_the_gather_bit_for_bit(B, C, H, W, grid):
    from stil_tta_amd._lib import lib
    L = lib()
    x, perm = shuffle_input(B, C, H, W, grid)
    out = _run_shuffle(L, x, grid, perm)
    assert bool((out[0] == SENTINEL).all() and (out[B + 1] == SENTINEL).all()), "a sentinel around dst changed"
    assert torch.equal(out[1:B + 1], shuffle_ref(x, grid, perm))
    ident = torch.arange(grid * grid, dtype=torch.int32).repeat(B, 1)
    assert torch.equal(_run_shuffle(L, x, grid, ident)[1:B + 1], x)
    # entries out of range leave their slots in place
    bad = perm.clone()
    bad[:, 0] = -1
    bad[:, -1] = grid * grid
    if grid > 1:
        bad[0, 1] = 2 ** 31 - 1
        bad[0, 2 % (grid * grid)] = -2 ** 31
    o = _run_shuffle(L, x, grid, bad)
    assert bool((o[0] == SENTINEL).all() and (o[B + 1] == SENTINEL).all())
    ref = shuffle_ref(x, grid, bad)
    assert torch.equal(o[1:B + 1], ref)
    ph, pw = H // grid, W // grid
    assert torch.equal(ref[:, :, :ph, :pw], x[:, :, :ph, :pw]) and torch.equal(ref[:, :, H - ph:, W - pw:], x[:, :, H - ph:, W - pw:])


def test_patch_shuffle_takes_the_scalar_path_on_a_misaligned_view():
    """pw % 4 == 0 but the pointers are 4 floats + 1 into their allocations: 4-byte accesses, same result."""
    from stil_tta_amd._lib import lib
    L = lib()
    B, C, H, W, grid = 2, 3, 32, 32, 4
    x, perm = shuffle_input(B, C, H, W, grid)
    n = x.numel()
    src = torch.full((n + 8,), SENTINEL, device="cuda")
    dst = torch.full((n + 8,), SENTINEL, device="cuda")
    src[5:5 + n] = x.cuda().view(-1)
    L.patch_shuffle(src[5:].data_ptr(), dst[1:].data_ptr(), B, C, H, W, grid, perm.cuda().data_ptr(), None)
    torch.cuda.synchronize()
    d = dst.cpu()
    assert float(d[0]) == SENTINEL and bool((d[1 + n:] == SENTINEL).all())
    assert torch.equal(d[1:1 + n].view(B, C, H, W), shuffle_ref(x, grid, perm))


def test_patch_shuffle_rejects_bad_arguments():
    from stil_tta_amd._lib import lib
    fn = lib()._dll.stil_patch_shuffle
    x = torch.zeros(2, 3, 8, 8, device="cuda")
    y = torch.zeros(2, 3, 8, 8, device="cuda")
    perm = torch.arange(16, dtype=torch.int32, device="cuda").repeat(2, 1)
    xp, yp, pp = x.data_ptr(), y.data_ptr(), perm.data_ptr()
    assert fn(xp, yp, 2, 3, 8, 8, 4, pp, None) == 0
    assert fn(xp, yp, 2, 3, 8, 8, 3, pp, None) != 0                      # grid does not divide H, W
    assert fn(xp, yp, 1, 3, 8, 16, 16, pp, None) != 0 and fn(xp, yp, 1, 3, 16, 8, 16, pp, None) != 0   # grid divides one of H, W only
    assert fn(xp, xp, 2, 3, 8, 8, 4, pp, None) != 0                      # src == dst
    assert fn(xp, xp + 64, 2, 3, 8, 8, 4, pp, None) != 0                 # overlapping
    assert fn(None, yp, 2, 3, 8, 8, 4, pp, None) != 0 and fn(xp, None, 2, 3, 8, 8, 4, pp, None) != 0 and fn(xp, yp, 2, 3, 8, 8, 4, None, None) != 0
    assert fn(xp, yp, 0, 3, 8, 8, 4, pp, None) != 0 and fn(xp, yp, 2, 3, 8, 8, 0, pp, None) != 0 and fn(xp, yp, 2, -3, 8, 8, 4, pp, None) != 0
    torch.cuda.synchronize()
    assert bool((y == 0).all())


# ------------------------------------------------------------------------------------------ check 2: the row kernel
def deyo_cases():
    return [(r, k, v) for r in ROWS for k in KS for v in VARIANTS]


def first_max(z):
    K = z.shape[1]
    return torch.where(z == z.max(dim=1, keepdim=True).values, torch.arange(K)[None, :], K).min(dim=1).values


def place(v, default):
    """The threshold among the values v (float64): the middle of E.widest_gap when there are at least four values and that gap
    is at least 0.02 wide (values that differ by rounding alone form no gap), else `default`."""
    if v.numel() >= 4:
        mid, half = E.widest_gap(v)
        if half >= 1e-2:
            return mid
    return default


def deyo_input(rows, K, variant, seed=0):
    """-> (Z, Zs [rows, K] float32, tau_ent, tau_plpd, e0).  Row families:
    0 one logit +60 on a class j other than 0, and Zs with class j 8 BELOW its noise (H ~ 0, PLPD ~ 1: selected);
    1 every logit tied (H = ln K: unreliable);
    2 the peaked row of family 0 with Zs = Z (H ~ 0, PLPD = 0: reliable, fails the PLPD filter);
    3 one logit +8 on class j, Zs as in family 0 (a moderate entropy and PLPD: weights well away from those of family 0);
    4 two EQUAL logits +60 on classes j1 < j2, Zs low on j1 and high on j2: PLPD = +0.5 by the first maximum, -0.5 by the other.
    "mixed": r % 4 of families 0-3; "none_reliable": family 1; "plpd_fails": families 2, 1 alternating; "tied": 4, 1 alternating.
    The thresholds come from `place` on the float64 H and on the float64 PLPD of the reliable rows (defaults 0.5 ln K, 0.2).
    K == 1: H = 0 = tau_ent exactly, nothing is reliable."""
    g = torch.Generator().manual_seed(seed + 1000 * rows + K)
    z = torch.rand(rows, K, generator=g) * 2.0 - 1.0
    zs = torch.rand(rows, K, generator=g) * 2.0 - 1.0
    for r in range(rows):
        fam = {"mixed": r % 4, "none_reliable": 1, "plpd_fails": (2, 1)[r % 2], "tied": (4, 1)[r % 2]}[variant]
        j = 0 if K == 1 else 1 + int(torch.randint(0, K - 1, (1,), generator=g))
        if fam == 0 or fam == 2:
            z[r, j] += 60.0
            zs[r, j] -= 8.0
            if fam == 2:
                zs[r] = z[r]
        elif fam == 1:
            z[r] = 3.5
        elif fam == 3:
            z[r, j] += 8.0
            zs[r, j] -= 8.0
        else:
            j = 0 if K == 1 else int(torch.randint(0, K - 1, (1,), generator=g))
            j2 = 0 if K == 1 else j + 1 + int(torch.randint(0, K - 1 - j, (1,), generator=g))
            z[r, j] = 60.0
            z[r, j2] = 60.0
            zs[r, j] -= 8.0
            if j2 != j:
                zs[r, j2] += 8.0
    z, zs = z.float(), zs.float()
    lnk = math.log(K)
    x, xs = z.double(), zs.double()
    logp = torch.log_softmax(x, dim=1)
    H = -(logp.exp() * logp).sum(dim=1)
    yh = first_max(z)
    d = logp.exp().gather(1, yh[:, None])[:, 0] - torch.softmax(xs, dim=1).gather(1, yh[:, None])[:, 0]
    tau_ent = float(np.float32(place(H, 0.5 * lnk)))
    rel = H < tau_ent
    tau_plpd = float(np.float32(place(d[rel], DEFAULT_PLPD)))
    return z, zs, tau_ent, tau_plpd, float(np.float32(0.4 * lnk))


def deyo_ref(z, zs, tau_ent, tau_plpd, e0, a_ent, a_plpd, dtype, grad_scale=1.0):
    """The contract of include/stil_deyo.h with autograd in `dtype`."""
    x = z.detach().to(dtype).clone().requires_grad_(True)
    logp = torch.log_softmax(x, dim=1)
    p = logp.exp()
    H = -(p * logp).sum(dim=1)
    pd, Hd = p.detach(), H.detach()
    yh = first_max(z)
    d = pd.gather(1, yh[:, None])[:, 0] - torch.softmax(zs.detach().to(dtype), dim=1).gather(1, yh[:, None])[:, 0]
    rel = Hd < tau_ent
    sel = rel & (d > tau_plpd)
    w = a_ent * torch.exp(e0 - Hd) + a_plpd * torch.exp(d)
    n = int(sel.sum())
    if n > 0:
        loss = (sel.to(dtype) * w * H).sum() / n
        (g,) = torch.autograd.grad(loss * grad_scale, [x])
    else:
        loss, g = torch.zeros((), dtype=dtype), torch.zeros_like(x)
    return dict(loss=loss.detach(), grad=g, probs=pd, H=Hd, lse=torch.logsumexp(x.detach(), dim=1), plpd=d, w=w, yhat=yh, rel=rel, sel=sel,
                n=n, n_rel=int(rel.sum()))


def _run_rows(L, zb, zsb, ld, lds, rows, K, tau_ent, tau_plpd, e0, a_ent, a_plpd, gs, nt=5):
    dev = "cuda"
    f = lambda n, **kw: torch.full((n,), SENTINEL, device=dev, **kw)
    o = dict(lse=f(rows + 1, dtype=torch.float64), Hd=f(rows + 1, dtype=torch.float64), Wd=f(rows + 1, dtype=torch.float64),
             p=torch.full((rows + 1, ld), SENTINEL, device=dev), H=f(rows + 1), plpd=f(rows + 1), w=f(rows + 1),
             yhat=torch.full((rows + 1,), -9, dtype=torch.int32, device=dev), rel=torch.full((rows + 1,), 9, dtype=torch.uint8, device=dev),
             sel=torch.full((rows + 1,), 9, dtype=torch.uint8, device=dev), dZ=torch.full((rows + 1, ld), SENTINEL, device=dev),
             counts=torch.full((5,), -3, dtype=torch.int32, device=dev), loss=f(2),
             act=torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8, device=dev), gate=torch.full((nt + 1,), 9, dtype=torch.uint8, device=dev))
    L.deyo_rows(zb.data_ptr(), ld, zsb.data_ptr(), lds, rows, K, tau_ent, tau_plpd, e0, a_ent, a_plpd, gs, o["lse"].data_ptr(), o["Hd"].data_ptr(),
                o["Wd"].data_ptr(), o["p"].data_ptr(), ld, o["H"].data_ptr(), o["plpd"].data_ptr(), o["w"].data_ptr(), o["yhat"].data_ptr(),
                o["rel"].data_ptr(), o["sel"].data_ptr(), o["dZ"].data_ptr(), ld, o["counts"].data_ptr(), o["loss"].data_ptr(),
                o["act"].data_ptr(), o["gate"].data_ptr(), nt, None)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _padded(z, rows, K, ld):
    zb = torch.full((rows + 1, ld), SENTINEL, dtype=torch.float32)
    zb[:rows, :K] = z
    return zb.cuda()


@pytest.mark.parametrize("rows,K,variant", deyo_cases())
def test_deyo_rows_against_float64(rows, K, variant):
    from stil_tta_amd._lib import lib
    L = lib()
    z, zs, tau_ent, tau_plpd, e0 = deyo_input(rows, K, variant)
    gs = float(np.float32(0.75))
    ref = deyo_ref(z, zs, tau_ent, tau_plpd, e0, A_ENT, A_PLPD, torch.float64, gs)
    if variant == "none_reliable" or K == 1:
        assert ref["n"] == 0 and ref["n_rel"] == 0
    if variant == "plpd_fails":
        assert ref["n"] == 0 and (K == 1 or ref["n_rel"] > 0)
    for pad in (0, 3):
        ld = K + pad
        zb = _padded(z, rows, K, ld)
        zsb = _padded(zs, rows, K, ld + pad)            # its own stride
        a, b = (_run_rows(L, zb, zsb, ld, ld + pad, rows, K, tau_ent, tau_plpd, e0, A_ENT, A_PLPD, gs) for _ in range(2))
        for k in a:
            assert torch.equal(a[k], b[k]), f"{k}: not bit-identical on repetition"
        # sentinels: padding columns, the row past the end, the element past every vector
        assert bool((a["p"][rows] == SENTINEL).all() and (a["dZ"][rows] == SENTINEL).all())
        for k in ("H", "plpd", "w", "lse", "Hd", "Wd"):
            assert float(a[k][rows]) == SENTINEL, k
        assert int(a["rel"][rows]) == 9 and int(a["sel"][rows]) == 9 and int(a["gate"][5]) == 9 and int(a["yhat"][rows]) == -9
        assert int(a["counts"][4]) == -3 and float(a["loss"][1]) == SENTINEL
        if pad:
            assert bool((a["p"][:, K:] == SENTINEL).all() and (a["dZ"][:, K:] == SENTINEL).all())
        # decisions, first maximum, counts, gate: exact
        assert torch.equal(a["yhat"][:rows].long(), ref["yhat"])
        assert torch.equal(a["sel"][:rows].bool(), ref["sel"]) and torch.equal(a["rel"][:rows].bool(), ref["rel"])
        assert a["counts"][:4].tolist() == [ref["n"], ref["n_rel"], 0, 0]
        assert a["gate"][:5].tolist() == ([1, 0, 1, 1, 0] if ref["n"] > 0 else [0] * 5)
        close(a["lse"][:rows], ref["lse"], name="lse")
        close(a["p"][:rows, :K], ref["probs"], name="probs")
        close(a["H"][:rows], ref["H"], name="H")
        assert torch.equal(a["Hd"][:rows].float(), a["H"][:rows]) and torch.equal(a["Wd"][:rows].float(), a["w"][:rows])
        close(a["plpd"][:rows], ref["plpd"], name="plpd")
        close(a["w"][:rows], ref["w"], name="w")
        close(a["loss"][:1], ref["loss"].view(1), name="loss")
        close(a["dZ"][:rows, :K], ref["grad"], name="dZ")
        if ref["n"] == 0:
            assert bool((a["dZ"][:rows, :K] == 0).all()) and float(a["loss"][0]) == 0.0
        # tie to TENT's kernel: p, H, lse bit for bit
        lse = torch.empty(rows, dtype=torch.float64, device="cuda")
        p = torch.empty(rows, ld, device="cuda")
        H = torch.empty(rows, device="cuda")
        mean = torch.empty(1, device="cuda")
        L.entropy_rows(zb.data_ptr(), ld, rows, K, 1.0, lse.data_ptr(), p.data_ptr(), ld, H.data_ptr(), None, ld, mean.data_ptr(), None)
        torch.cuda.synchronize()
        assert torch.equal(a["lse"][:rows], lse.cpu()) and torch.equal(a["H"][:rows], H.cpu())
        assert torch.equal(a["p"][:rows, :K], p.cpu()[:, :K])


@pytest.mark.parametrize("rows,K,variant", [(r, k, v) for r in ROWS for k in KS for v in ("mixed", "tied")])
def test_entropy_only_deyo_rows_is_eata_rows_bit_for_bit(rows, K, variant):
    """a_plpd = 0, plpd_margin = -2, ent_margin = e0 = E, a_ent = 1: loss, dZ, sel and counts[0] of stil_eata_rows with an invalid m."""
    from stil_tta_amd._lib import lib
    L = lib()
    z, zs, tau_ent, _, _ = deyo_input(rows, K, variant)
    gs = float(np.float32(0.75))
    zb, zsb = _padded(z, rows, K, K), _padded(zs, rows, K, K)
    a = _run_rows(L, zb, zsb, K, K, rows, K, tau_ent, -2.0, tau_ent, 1.0, 0.0, gs)
    e = E._run_rows(L, zb, K, rows, K, tau_ent, E.D_MARGIN, torch.zeros(K), 0, gs)
    for k in ("loss", "dZ", "sel", "rel", "H", "p", "w", "lse", "gate"):
        assert torch.equal(a[k], e[k]), k
    assert int(a["counts"][0]) == int(e["counts"][0]) and int(a["counts"][1]) == int(e["counts"][1])
    if variant == "mixed" and K > 1:
        assert int(a["counts"][0]) > 0


def test_deyo_rows_rejects_bad_arguments():
    import ctypes
    from stil_tta_amd._lib import lib
    fn = lib()._dll.stil_deyo_rows
    z, zs = torch.zeros(4, 8, device="cuda"), torch.zeros(4, 8, device="cuda")
    lse, hd, wd = (torch.zeros(4, dtype=torch.float64, device="cuda") for _ in range(3))
    p, dz = torch.zeros(4, 8, device="cuda"), torch.zeros(4, 8, device="cuda")
    H, d, w = (torch.zeros(4, device="cuda") for _ in range(3))
    yh = torch.zeros(4, dtype=torch.int32, device="cuda")
    rel, sel = (torch.zeros(4, dtype=torch.uint8, device="cuda") for _ in range(2))
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    act, gate = (torch.zeros(3, dtype=torch.uint8, device="cuda") for _ in range(2))
    f32 = ctypes.c_float

    def call(ld=8, lds=8, rows=4, K=8, ldp=8, ldd=8, a_ent=1.0, a_plpd=1.0, zs_=zs, yh_=yh, act_=act, nt=3):
        return fn(z.data_ptr(), ld, None if zs_ is None else zs_.data_ptr(), lds, rows, K, f32(1.0), f32(0.2), f32(0.8), f32(a_ent), f32(a_plpd), f32(1.0),
                  lse.data_ptr(), hd.data_ptr(), wd.data_ptr(), p.data_ptr(), ldp, H.data_ptr(), d.data_ptr(), w.data_ptr(),
                  None if yh_ is None else yh_.data_ptr(), rel.data_ptr(), sel.data_ptr(), dz.data_ptr(), ldd, cnt.data_ptr(), loss.data_ptr(),
                  None if act_ is None else act_.data_ptr(), gate.data_ptr(), nt, None)
    assert call() == 0
    assert call(ld=7) != 0 and call(lds=7) != 0 and call(K=0) != 0 and call(rows=0) != 0 and call(ldp=4) != 0 and call(ldd=4) != 0
    assert call(a_ent=-1.0) != 0 and call(a_plpd=float("nan")) != 0 and call(a_ent=float("inf")) != 0
    assert call(zs_=None) != 0 and call(yh_=None) != 0 and call(act_=None) != 0 and call(nt=-1) != 0
    assert call(act_=None, nt=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ check 3: the step, restated
GRID = 4
SHUFFLE_SEED = 2024


def deyo_restated(sd, keys, x, perm, hp, dtype, margins=None, decisions=None, decisions_s=None, e0=None, a_ent=1.0, a_plpd=1.0):
    """The contract on one batch in `dtype` on a copy of the state: the forward on the clean batch (gradients for `keys`), the
    forward on the patch-shuffled images and the unchanged table (none), the DeYO loss.  margins None: the pre-pass (tau_ent
    from E.widest_gap of this forward's H, tau_plpd from that of the reliable rows' PLPD).  -> dict"""
    xs = [shuffle_ref(x[0], GRID, torch.as_tensor(perm)), x[1]]
    s, out_m, flips = E._forward(sd, keys, x, hp, dtype, decisions)
    _, out_s, flips_s = E._forward(sd, [], xs, hp, dtype, decisions_s)
    out_s = out_s.detach()
    logp = torch.log_softmax(out_m, dim=1)
    p = logp.exp()
    H = -(p * logp).sum(dim=1)
    pd, Hd = p.detach(), H.detach()
    yh = first_max(out_m.detach())
    d = pd.gather(1, yh[:, None])[:, 0] - torch.softmax(out_s, dim=1).gather(1, yh[:, None])[:, 0]
    gaps = {}
    if margins is None:
        te, gaps["H"] = E.widest_gap(Hd)
        tp, gaps["plpd"] = E.widest_gap(d[Hd < float(np.float32(te))])
        margins = (float(np.float32(te)), float(np.float32(tp)))
    te, tp = margins
    e0 = 0.4 * math.log(hp.num_classes) if e0 is None else e0
    rel = Hd < te
    sel = rel & (d > tp)
    w = a_ent * torch.exp(e0 - Hd) + a_plpd * torch.exp(d)
    n = int(sel.sum())
    assert n > 0
    loss = (sel.to(dtype) * w * H).sum() / n
    g = dict(zip(keys, [t.detach() for t in torch.autograd.grad(loss, [s[k] for k in keys])]))
    flips = dict(flips)
    flips.update({"shuffled " + t: v for t, v in flips_s.items()})
    return dict(p=pd, H=Hd, plpd=d, w=w, yhat=yh, sel=sel, rel=rel, n=n, loss=loss.detach(), g=g, zs=out_s, margins=margins, gaps=gaps, flips=flips)


# (label, hparams, B, tta_params, batch seeds, state seed)
PARITY = [
    ("dvm_b32_bn_online", lambda: T.dvm_hp(32), 32, "bn", (201, 205), 11),
    ("dvm_b32_norm", lambda: T.dvm_hp(32), 32, "norm", (301,), 21),
    ("cardiac_b32_bn", lambda: T.cardiac_hp(32), 32, "bn", (401,), 31),
]


def _shuffled_decisions(S, hp, sd_before, which, x, perm):
    """The device's ReLU / max-pool decisions of the forward on the shuffled images: the step runs it under no_grad, where none
    are kept, so it is repeated here with gradients on, on a second model holding the same state.  -> (decisions, out_m)"""
    from stil_tta_amd import tta
    m2 = T.make_model(hp, sd_before, tta=True, tta_method="tent", tta_params=which)
    m2.freeze()
    xd = T.to_dev((x, torch.zeros(1)))[0]
    xs = [tta.patch_shuffle(xd[0], GRID, perm), xd[1]]
    with S._trace_decisions() as trace:
        out = tta.adapting_pass(m2, xs, tta._begin(m2), tta.entropy)[0]
        torch.cuda.synchronize()
        return S._device_decisions(m2, trace), out, xs[0]


@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_deyo_step_matches_the_contract_restated_in_float64(case):
    """Bars are TENT's (tests/test_gpu_tta.py): predictions (of both forwards) <= 3e-5 scaled, every gradient of A <= 3 e32 +
    1e-4, Adam within 2.2 lr step, everything else bit-identical; the selection equals the float64 one on every row; loss,
    entropy, PLPD and weight within 3 e32 + 2e-5 (1 + max|value|), e32 the fp32 restatement's own distance from float64."""
    import test_gpu_step as S
    label, mk_hp, B, which, seeds, sseed = case
    hp = mk_hp()
    lr = 1e-3
    sd = E.scaled_state(hp, sseed)
    m = T.make_model(hp, sd, tta=True, tta_method="deyo", tta_params=which, tta_lr=lr, tta_patch_grid=GRID, tta_shuffle_seed=SHUFFLE_SEED,
                     tta_reweight_ent=A_ENT, tta_reweight_plpd=A_PLPD)
    m.freeze()
    keys = T.adapted_keys(m)
    from stil_tta_amd import tta
    rng = np.random.default_rng(SHUFFLE_SEED)          # the draws the model's own generator will make
    bad, opt = [], {}
    kw = dict(a_ent=A_ENT, a_plpd=A_PLPD)
    for step, seed in enumerate(seeds, start=1):
        x, y = T.tta_batch(hp, B, seed)
        perm = tta.draw_perm(rng, B, GRID)
        sd_before = {k: v.cpu() for k, v in m.state_dict().items()}
        pre = deyo_restated(sd_before, keys, x, perm, hp, torch.float64, **kw)
        te, tp = pre["margins"]
        print(f"[{label}] batch {step}: tau_ent {te:.4f} (half gap {pre['gaps']['H']:.2e}) tau_plpd {tp:.4f} (half gap {pre['gaps']['plpd']:.2e}) "
              f"reliable {int(pre['rel'].sum())}/{B} selected {pre['n']}/{B}")
        m.hp.tta_ent_margin, m.hp.tta_plpd_margin = te, tp
        dec_s, out_s, xs_dev = _shuffled_decisions(S, hp, sd_before, which, x, perm)
        before = T.full_state(m)
        with S._trace_decisions() as trace:
            m.test_step(T.to_dev((x, y)), step - 1)
            torch.cuda.synchronize()
            decisions = S._device_decisions(m, trace)
        lt = m.last_tta
        assert np.array_equal(lt["perm"], perm), "the step drew another permutation than a generator seeded alike"
        assert torch.equal(xs_dev.cpu(), shuffle_ref(x[0], GRID, torch.as_tensor(perm)))
        assert torch.equal(out_s, lt["y_hat_shuffled"]), "the traced repeat of the shuffled forward is not the step's: its decisions are another pass's"
        r64 = deyo_restated(sd_before, keys, x, perm, hp, torch.float64, margins=(te, tp), decisions=decisions, decisions_s=dec_s, **kw)
        r64free = pre                                  # the pre-pass decides on its own (rounded) margins: the free float64 restatement
        r32 = deyo_restated(sd_before, keys, x, perm, hp, torch.float32, margins=(te, tp), **kw)
        S._check_flips(r64["flips"])
        eH = float((r32["H"].double() - r64free["H"]).abs().max())
        ed = float((r32["plpd"].double() - r64free["plpd"]).abs()[r64free["rel"]].max())
        frac = pre["n"] / B
        print(f"[{label}] batch {step}: fp32 restatement error H {eH:.2e} PLPD (reliable rows) {ed:.2e}; selected fraction {frac:.3f}")
        if pre["gaps"]["H"] < 100 * eH or pre["gaps"]["plpd"] < 100 * ed:
            bad.append((step, "conditioning", pre["gaps"], eH, ed))
        if not (bool((r64free["rel"] & ~r64free["sel"]).any()) and bool(r64free["sel"].any())):
            bad.append((step, "the PLPD filter has one outcome only on the reliable rows"))
        d = S._scaled(lt["probs"].cpu().double().numpy(), r64["p"].numpy())
        ds = S._scaled(torch.softmax(lt["y_hat_shuffled"].cpu().double(), 1).numpy(), torch.softmax(r64["zs"], 1).numpy())
        print(f"[{label}] batch {step}: predictions scaled error {d:.2e}, of the shuffled view {ds:.2e} "
              f"(fp32 restatement: {S._scaled(r32['p'].double().numpy(), r64free['p'].numpy()):.2e})")
        if d > 3e-5:
            bad.append((step, "predictions", d))
        if ds > 3e-5:
            bad.append((step, "predictions of the shuffled view", ds))
        if not torch.equal(lt["selected"].cpu().bool(), r64["sel"]) or not torch.equal(lt["reliable"].cpu().bool(), r64["rel"]):
            bad.append((step, "selection", int((lt["selected"].cpu().bool() != r64["sel"]).sum())))
        if int(lt["n_selected"]) != r64["n"] or int(lt["n_reliable"]) != int(r64["rel"].sum()):
            bad.append((step, "counts", int(lt["n_selected"]), r64["n"]))
        # loss, entropy, PLPD and weight are functions of logits that the scaled head amplifies: the bar has the shape of the
        # gradients', three times the fp32 restatement's own distance from float64 plus close()'s rounding floor of the value
        for name, got, key in (("loss", lt["loss"].view(1), "loss"), ("entropy", lt["entropy"], "H"), ("plpd", lt["plpd"], "plpd"), ("weight", lt["weight"], "w")):
            ref, e32 = r64[key].double().view(-1), float((r32[key].double() - r64free[key].double()).abs().max())
            err, bound = float((got.cpu().double().view(-1) - ref).abs().max()), 3 * e32 + TOL * (1.0 + float(ref.abs().max()))
            print(f"[{label}] batch {step}: {name} error {err:.2e} (fp32 restatement {e32:.2e}, bar {bound:.2e})")
            if err > bound:
                bad.append((step, name, err, e32))
        gd = T.device_grads(m)
        ratios = []
        for k in keys:
            e32, err = T._rel(r32["g"][k].double(), r64free["g"][k]), T._rel(gd[k], r64["g"][k])
            ratios.append((err / (3 * e32 + 1e-4), k, err, e32))
            if err > 3 * e32 + 1e-4:
                bad.append((step, "grad " + k, err, e32))
        print(f"[{label}] batch {step}: gradient error / (3*e32 + 1e-4), worst four: {sorted(ratios, reverse=True)[:4]}")
        sd32 = {k: v.clone() for k, v in sd_before.items()}
        O.adam_step(sd32, r32["g"], opt, step, lr)
        after = T.full_state(m)
        aset = set(keys)
        for k, v in after.items():
            if k in aset:
                dev = float((v.cpu() - sd32[k]).abs().max())
                if dev > 2.2 * lr * step:
                    bad.append((step, "adam " + k, dev))
            elif not torch.equal(v, before[k]):
                bad.append((step, "changed " + k))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:10]}"


# ------------------------------------------------------------------------------------------ check 4: properties
def _small(which="bn", method="deyo", **tta):
    """B = 16, 64 px; margins that select every row unless a test narrows them"""
    hp = T.dvm_hp(16, img_size=64)
    sd = E.scaled_state(hp, 5)
    tta.setdefault("tta_ent_margin", 6.0)
    tta.setdefault("tta_plpd_margin", -2.0)
    return hp, sd, (lambda: T.make_model(hp, sd, tta=True, tta_method=method, tta_params=which, **tta))


def _moments(m):
    st = m._tent
    return dict(exp_avg=st.exp_avg.clone(), exp_avg_sq=st.exp_avg_sq.clone(), steps=st.steps.clone())


def test_a_batch_that_selects_nothing_moves_nothing_and_still_scores():
    hp, sd, mk = _small()
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, 11)), T.to_dev(T.tta_batch(hp, 16, 12))
    m = mk()
    m.test_step(b1, 0)
    assert int(m.last_tta["n_selected"]) == 16 and int(m._tent.steps.max()) == 1
    for margins in ((0.0, -2.0), (6.0, 2.0)):          # nothing reliable; every reliable row fails the PLPD filter
        s1, e1 = T.full_state(m), _moments(m)
        m.hp.tta_ent_margin, m.hp.tta_plpd_margin = margins
        p = m.test_step(b2, 1)
        torch.cuda.synchronize()
        assert int(m.last_tta["n_selected"]) == 0 and float(m.last_tta["loss"]) == 0.0
        assert int(m.last_tta["n_reliable"]) == (0 if margins[0] == 0.0 else 16)
        s2, e2 = T.full_state(m), _moments(m)
        for k in s1:
            assert torch.equal(s1[k], s2[k]), k
        for k in e1:
            assert torch.equal(e1[k], e2[k]), k
        assert p.shape == (16, hp.num_classes) and bool(torch.isfinite(p).all())
        close(p.sum(1), torch.ones(16), name="scores")


@pytest.mark.parametrize("which", ["bn", "norm"])
def test_deyo_step_issues_no_weight_gradient_product(which, monkeypatch):
    from stil_tta_amd._lib import lib
    hp, sd, mk = _small(which)
    m = mk()
    L = lib()
    calls = []
    for name in ("wgrad_tn", "wgrad_tn_partial"):
        orig = getattr(L, name)
        monkeypatch.setitem(L.__dict__, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    A0 = {k: v.clone() for k, v in m.state_dict().items() if k in set(T.adapted_keys(m))}
    m.test_step(T.to_dev(T.tta_batch(hp, 16, 7)), 0)
    torch.cuda.synchronize()
    assert calls == [], f"{len(calls)} weight-gradient launches in a DeYO step"
    assert any(not torch.equal(m.state_dict()[k], v) for k, v in A0.items()), "the DeYO step adapted nothing"


def test_deyo_step_synchronises_no_more_than_a_tent_step():
    hp, sd, mk = _small()
    _, _, mk_tent = _small(method="tent")
    batches = [T.to_dev(T.tta_batch(hp, 16, 30 + i)) for i in range(3)]
    e, t = mk(), mk_tent()
    for mm in (e, t):                                  # first batch outside the count: lazy state, layouts
        mm.test_step(batches[0], 0)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:  # control: the counter sees a device -> host read
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            float(e.last_tta["loss"])
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert any("synchroniz" in str(w.message).lower() for w in rec), "the sync counter sees nothing"
    we, wt = E._sync_warnings(e, batches[1:]), E._sync_warnings(t, batches[1:])
    print(f"synchronising calls over two steps: deyo {len(we)}, tent {len(wt)}")
    assert len(we) <= len(wt), (we, wt)
    e.hp.tta_ent_margin = 0.0                          # and the n == 0 decision stays on the device too
    assert len(E._sync_warnings(e, batches[1:])) <= len(wt)


def test_the_permutation_fed_back_rebuilds_the_shuffled_batch_and_the_generator_rules():
    from stil_tta_amd import tta
    hp, sd, mk = _small()
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, 11)), T.to_dev(T.tta_batch(hp, 16, 12))
    m = mk()
    m.test_step(b1, 0)
    perm1, zs1 = m.last_tta["perm"].copy(), m.last_tta["y_hat_shuffled"].clone()
    assert perm1.shape == (16, 16) and perm1.dtype == np.int32
    assert np.array_equal(np.sort(perm1, axis=1), np.tile(np.arange(16), (16, 1))) and not np.array_equal(perm1, np.sort(perm1, axis=1))
    xs = tta.patch_shuffle(b1[0][0], m.hp.tta_patch_grid, perm1)
    assert torch.equal(xs.cpu(), shuffle_ref(b1[0][0].cpu(), m.hp.tta_patch_grid, torch.as_tensor(perm1)))
    assert torch.equal(tta.patch_shuffle(b1[0][0], m.hp.tta_patch_grid, torch.as_tensor(perm1).cuda()), xs)      # a device perm
    # the shuffled logits are the forward-only baseline's on that batch, from the source state
    _, _, mk_bn = _small(method="bn_adapt")
    bn = mk_bn()
    bn.test_step(([xs, b1[0][1]], b1[1]), 0)
    assert torch.equal(bn.last_tta["y_hat_m"], zs1)
    # the generator runs on through reset_tta() and episodes; a new state restarts it from tta_shuffle_seed
    m.test_step(b2, 1)
    perm2 = m.last_tta["perm"].copy()
    assert not np.array_equal(perm1, perm2)
    m.reset_tta()
    m.test_step(b1, 2)
    assert not np.array_equal(m.last_tta["perm"], perm1) and not np.array_equal(m.last_tta["perm"], perm2)
    m.load_state_dict({k: v.cuda() for k, v in sd.items()})
    assert m._tent is None
    m.test_step(b1, 0)
    assert np.array_equal(m.last_tta["perm"], perm1) and torch.equal(m.last_tta["y_hat_shuffled"], zs1)
    _, _, mk_other = _small(tta_shuffle_seed=7)
    o = mk_other()
    o.test_step(b1, 0)
    assert not np.array_equal(o.last_tta["perm"], perm1)
    with pytest.raises(ValueError):
        tta.patch_shuffle(b1[0][0], 4, perm1[:, :9])
    with pytest.raises(ValueError):
        tta.patch_shuffle(b1[0][0], 5, perm1)


def test_state_rules_reset_episodic_and_load_state_dict():
    """Scores and A: the permutations differ from batch to batch (the generator runs on), so the rules are checked on runs
    that see the same draws: a fresh model per comparison."""
    hp, sd, mk = _small()
    b1, b2 = T.to_dev(T.tta_batch(hp, 16, 11)), T.to_dev(T.tta_batch(hp, 16, 12))
    o = mk()
    A0 = {k: v.clone() for k, v in o.state_dict().items() if k in set(T.adapted_keys(o))}
    q1 = o.test_step(b1, 0).clone()
    q2 = o.test_step(b2, 1).clone()
    assert any(not torch.equal(o.state_dict()[k], v) for k, v in A0.items())
    o.reset_tta()
    for k, v in A0.items():
        assert torch.equal(o.state_dict()[k], v), k
    st = o._tent
    assert int(st.steps.max()) == 0 and float(st.exp_avg.abs().max()) == 0 and float(st.exp_avg_sq.abs().max()) == 0
    # the clean forward of the first batch after a reset starts from the source values: its scores are batch 1's
    assert torch.equal(o.test_step(b1, 2), q1)
    # episodic: every batch starts from A0 and fresh moments; the scores come before the update, so they are a fresh model's
    _, _, mk_ep = _small(tta_episodic=True)
    ep = mk_ep()
    ep.test_step(b1, 0)
    p2 = ep.test_step(b2, 1).clone()
    f = mk()
    assert torch.equal(f.test_step(b2, 0), p2)
    assert not torch.equal(p2, q2), "online batch 2 equals the episodic one: nothing carried over"
    assert int(ep._tent.steps.max()) == 1
    # load_state_dict drops the state
    o.load_state_dict({k: v.cuda() for k, v in sd.items()})
    assert o._tent is None
    assert torch.equal(o.test_step(b1, 0), q1) and torch.equal(o.test_step(b2, 1), q2)


def test_freeze_and_inference_mode():
    hp, sd, mk = _small()
    b = T.to_dev(T.tta_batch(hp, 16, 14))
    a, c = mk(), mk()
    a.freeze()
    c.freeze()
    with torch.inference_mode():
        pa = a.test_step(b, 0)
    pc = c.test_step(b, 0)
    assert torch.equal(pa, pc)
    sa, sc = T.full_state(a), T.full_state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert any(not torch.equal(sa[k], v) for k, v in T.full_state(mk()).items() if k in set(T.adapted_keys(a)))
    assert not any(q.requires_grad for q in a.parameters())


def test_fit_test_takes_the_adapting_path(tmp_path):
    from stil_tta_amd import fit
    hp, sd, mk = _small()
    loader = [T.tta_batch(hp, 16, 20 + i) for i in range(3)]
    ck = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": {k: v.clone() for k, v in sd.items()}}, ck)
    a = mk()
    a.test_step(T.to_dev(loader[0]), 0)                # state from an earlier run: the checkpoint load must discard it, generator included
    ra = fit.test(a, loader, ck)
    h = mk()
    h.freeze()
    h.acc_test.reset()
    h.auc_test.reset()
    for i, bt in enumerate(loader):
        h.test_step(T.to_dev(bt), i)
    rh = {k: float(v) for k, v in h.test_epoch_end().items()}
    assert ra.keys() == rh.keys() and all(ra[k] == rh[k] or (ra[k] != ra[k] and rh[k] != rh[k]) for k in ra), (ra, rh)
    sa, sh = T.full_state(a), T.full_state(h)
    for k in sa:
        assert torch.equal(sa[k], sh[k]), k
    off = T.make_model(hp, sd, tta=True)
    fit.test(off, loader, ck)
    so = T.full_state(off)
    assert any(not torch.equal(so[k], sa[k]) for k in T.adapted_keys(a)), "fit.test with DeYO left A where the run without TTA leaves it"
