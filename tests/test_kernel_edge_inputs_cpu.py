"""CPU side of tests/test_gpu_kernel_edges.py.  Conditioning: on every float case of tests/kernel_edge_cases.py, fp32 ATen on the
CPU passes the very check the GPU test applies to the kernel (the `check_*` functions of that module) against the float64
reference; Adam's bound is re-measured.  Discrete outputs: the float64 reference is unambiguous on every row (a top-1 vs top-2
gap and a distance to the threshold of at least MIN_GAP), every planted tie is exact in fp32, every case of the CGPL partition
occurs.  Models: the dropout hash and the float64 Adam are exercised here, so that a mistake in a model shows without a GPU.
Sizes: the grid-stride cases exceed the launch caps they are meant to exceed."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_edge_cases as C  # noqa: E402
import test_gpu_kernel_edges as GE  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------
# conditioning: fp32 ATen meets the GPU test's own checks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_pseudo", [False, True])
@pytest.mark.parametrize("Bu,K,Dp", C.CGPL_TABLE)
def test_fp32_aten_meets_the_cgpl_checks(Bu, K, Dp, use_pseudo):
    c = C.cgpl_case(Bu, K, Dp)
    r64 = C.cgpl_reference(c, torch.float64, use_pseudo)
    assert all(bool(torch.isfinite(v).all()) for v in r64.values())
    GE.check_cgpl_floats(C.cgpl_reference(c, torch.float32, use_pseudo), r64)


@pytest.mark.parametrize("repeat_ratio", C.REPEAT_RATIOS)
@pytest.mark.parametrize("B,B_l,K,Dp", C.PROTO_ACCUM_TABLE)
def test_fp32_aten_meets_the_proto_accum_check(B, B_l, K, Dp, repeat_ratio):
    feat, hard, conf = C.proto_accum_case(B, B_l, K, Dp)
    r64 = C.proto_accum_reference(feat, hard, conf, B_l, K, repeat_ratio, torch.float64)
    GE.check_proto_accum(C.proto_accum_reference(feat, hard, conf, B_l, K, repeat_ratio, torch.float32), r64)
    cnt = r64[:, Dp]
    assert float(cnt[K - 1]) == 0 and bool((cnt > 0).any()), "a class without a member, and one with"
    assert bool((conf == 0).any()) and bool(((hard < 0) | (hard >= K)).any())
    members = conf.bool() & (hard >= 0) & (hard < K)
    assert float(cnt.sum()) == pytest.approx(float(members[:B_l].sum()) / repeat_ratio + float(members[B_l:].sum()), rel=1e-6)


def test_proto_accum_cases_pass_the_block_width():
    assert any(Dp + 1 > C.PROTO_ACCUM_THREADS for _, _, _, Dp in C.PROTO_ACCUM_TABLE) and any(Dp + 1 < C.PROTO_ACCUM_THREADS for _, _, _, Dp in C.PROTO_ACCUM_TABLE)


@pytest.mark.parametrize("lam0,lam1", C.CLIP_LAMS)
@pytest.mark.parametrize("B", C.CLIP_BS)
def test_fp32_aten_meets_the_clip_checks(B, lam0, lam1):
    Z = C.clip_case(B)
    assert abs(float(Z.abs().max()) - C.CLIP_SCALE) < 1e-5 and (B == 1 or float(Z.min()) < 0 < float(Z.max()))
    GE.check_clip(*C.clip_reference(Z, lam0, lam1, torch.float32), *C.clip_reference(Z, lam0, lam1, torch.float64))


@pytest.mark.parametrize("R,D", C.CLUB_TABLE)
def test_fp32_aten_meets_the_club_checks(R, D):
    mu, y = C.club_case(R, D)
    GE.check_club(C.club_reference(mu, y, torch.float32), C.club_reference(mu, y, torch.float64))


@pytest.mark.parametrize("rows,D", C.LN_VECTOR + C.LN_SCALAR + (C.LN_ALIGN,))
def test_fp32_aten_meets_the_layernorm_checks(rows, D):
    x, gamma, beta, gy, _, _ = C.ln_case(rows, D)
    r64 = C.ln_reference(x, gamma, beta, gy, torch.float64)
    assert all(bool(torch.isfinite(v).all()) for v in r64.values())
    GE.check_ln(C.ln_reference(x, gamma, beta, gy, torch.float32), r64)


def test_layernorm_cases_take_the_paths_they_are_named_for():
    assert all(D % 4 == 0 for _, D in C.LN_VECTOR) and all(D % 4 for _, D in C.LN_SCALAR) and C.LN_ALIGN[1] % 4 == 0
    assert max(r for r, _ in C.LN_VECTOR) > C.LN_BLOCK_CAP * C.LN_ROWS_PER_BLOCK
    assert any(8 * D * 4 > 64 * 1024 for _, D in C.LN_VECTOR) and any(8 * D * 4 > 64 * 1024 for _, D in C.LN_SCALAR), "the > 64 KiB LDS request"
    assert any(D == C.LN_MAX_D for _, D in C.LN_VECTOR)
    assert any(D < 4 for _, D in C.LN_SCALAR) and any(64 < D for _, D in C.LN_SCALAR)


def test_adam_bound_is_four_times_the_measured_aten_error():
    live = C.adam_live_mask()
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i in range(len(C.ADAM_CONFIGS)):
        P64, M64, V64, steps = C.adam_run_reference(i)
        assert steps == [5, 3, 5, 5, 0]
        p, m, v = C.adam_run_aten(i)
        for k, a, b in (("p", p, P64), ("m", m, M64), ("v", v, V64)):
            assert bool((b[~live] == C.SENT).all()) and bool(torch.isfinite(b[live]).all())
            worst[k] = max(worst[k], C.scaled_err(a[live], b[live]))
        GE.check_adam(p[live], m[live], v[live], P64[live], M64[live], V64[live])
    for k, e in worst.items():
        assert 0.8 * C.ADAM_ATEN_ERR[k] <= e <= C.ADAM_ATEN_ERR[k], f"{k}: measured {e:.3e}, recorded {C.ADAM_ATEN_ERR[k]:.3e}"
        assert C.ADAM_BOUND[k] == 4.0 * C.ADAM_ATEN_ERR[k]


# ---------------------------------------------------------------------------------------------------------------------
# discrete outputs are unambiguous
# ---------------------------------------------------------------------------------------------------------------------
def _gap(p):
    t = p.double().topk(min(2, p.shape[1]), 1)[0]
    return t[:, 0] - t[:, 1] if p.shape[1] > 1 else torch.ones(len(p), dtype=torch.float64)


@pytest.mark.parametrize("K", C.ONEHOT_KS)
@pytest.mark.parametrize("rows", C.ONEHOT_ROWS)
def test_onehot_cases_are_unambiguous(rows, K):
    p, th, idx, mask = C.onehot_case(rows, K)
    assert bool((_gap(p) >= C.MIN_GAP).all()) and bool(((p.max(1)[0].double() - C.f32(th)).abs() >= C.MIN_GAP).all())
    assert torch.equal(p.argmax(1).to(torch.int32), idx) and torch.equal((p.max(1)[0] >= C.f32(th)).float(), mask)
    if rows > 1:
        assert 0 < float(mask.sum()) < rows
        assert K <= 64 or (bool((idx >= 64).any()) and bool((idx < 64).any()))


def test_onehot_tie_rows_tie_exactly():
    p, th, idx, mask = C.onehot_tie_case()
    assert p.shape[1] == C.TIE_K
    mx = p.max(1, keepdim=True)[0]
    tied = [torch.nonzero(r).flatten().tolist() for r in (p == mx)]
    assert [t[0] for t in tied] == idx.tolist()
    for cols in C.TIE_PLACEMENTS:
        assert list(cols) in tied
    assert (5 % 64 != 70 % 64) and (5 % 64 == 69 % 64)
    at_th = (mx.flatten() == np.float32(th))
    assert int(at_th.sum()) == 2 and bool((mask[at_th] == 1).all()) and 0 < float(mask.sum()) < len(mask)
    others = p.clone()
    others[p == mx] = 0
    assert bool((mx.flatten().double() - others.max(1)[0].double() >= C.MIN_GAP).all())
    off = mx.flatten() != np.float32(th)
    assert bool(((mx.flatten().double() - float(th)).abs()[off] >= C.MIN_GAP).all())


@pytest.mark.parametrize("Bu,K,Dp", C.CGPL_TABLE)
def test_cgpl_cases_are_unambiguous(Bu, K, Dp):
    c = C.cgpl_case(Bu, K, Dp)
    tie_heads = {(u, h) for u, h, _, _ in c["ties"]}
    for h, name in enumerate(("zm", "zi", "zt")):
        p32, p64 = c[name].softmax(1), c[name].double().softmax(1)
        assert torch.equal(p32.argmax(1), c["top"][h]), f"{name}: argmax(softmax) in fp32 ATen is the planted column (first index on ties)"
        keep = torch.tensor([(u, h) not in tie_heads for u in range(Bu)])
        assert bool((_gap(p64)[keep] >= C.MIN_GAP).all()) and torch.equal(p64.argmax(1)[keep], c["top"][h][keep])
    for u, h, c0, c1 in c["ties"]:
        z = c[("zm", "zi", "zt")[h]][u]
        p = z.softmax(0)
        assert c0 < c1 and float(z[c0]) == float(z[c1]) and float(p[c0]) == float(p[c1]) == float(p.max()), "a tie is exact in fp32"
        rest = p.double().clone()
        rest[[c0, c1]] = 0
        assert float(p.double().max() - rest.max()) >= C.MIN_GAP
    a, b, d = c["top"]
    cs = torch.where((a == b) & (a == d), 1, torch.where(a == b, 2, torch.where(a == d, 3, 4)))
    assert torch.equal(cs, c["case"])
    if Bu >= 16:
        assert set(c["case"].tolist()) == {1, 2, 3, 4}, "all four cases"
    if K > 70:
        assert {(h, c1) for _, h, _, c1 in c["ties"]} == {(h, c1) for h in range(3) for _, c1 in C.TIE_PLACEMENTS}
    pred = C.cgpl_reference(c, torch.float64, True)["pred_full"]
    assert bool((_gap(pred) >= C.MIN_GAP).all()) and bool(((pred.max(1)[0] - c["th"]).abs() >= C.MIN_GAP).all())
    flags, hard, w3 = C.cgpl_discrete(c, True)
    if Bu >= 16:
        assert 0 < int(flags[:, 1].sum()) < Bu, "rows on both sides of the threshold"
        assert all(0 < float(w.sum()) < Bu for w in w3) and 0 < int(c["mr"].sum()) < Bu
    pred32 = C.cgpl_reference(c, torch.float32, True)["pred_full"]
    assert torch.equal(pred32.argmax(1).to(torch.int32), hard) and torch.equal((pred32.max(1)[0] >= c["th"]).to(torch.uint8), flags[:, 1])
    assert (c["ld"] > K) == (K == C.CGPL_LD_PAD_K) and (c["pred_in"] is not None) == (K == C.CGPL_PRED_IN_K)
    if c["pred_in"] is not None:
        assert float((c["pred_in"] - c["zm"].softmax(1)).abs().max()) > 1e-3, "pred_in is not softmax(zm)"


def test_cgpl_table_reaches_the_loops_it_names():
    ks = [K for _, K, _ in C.CGPL_TABLE]
    assert min(ks) == 2 and any(K > 256 for K in ks) and {64, 65} <= set(ks) and C.CGPL_LD_PAD_K in ks and C.CGPL_PRED_IN_K in ks
    assert all(3 * K * 4 <= 60 * 1024 for K in ks)


# ---------------------------------------------------------------------------------------------------------------------
# pooling, im2col: the references behave as the GPU test assumes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,Cc", C.POOL_TABLE)
def test_pool_cases_hold_ties_nan_windows_and_all_minus_inf_windows(N, H, W, Cc):
    x, gy = C.pool_case(N, H, W, Cc, "ties")
    assert torch.equal(gy, gy.round()) and torch.equal(x, x.round())
    if H * W > 1:
        y, _ = C.pool_reference(x, gy)
        cols = F.unfold(x, 3, padding=1, stride=2).view(N, Cc, 9, -1)       # zero padded: count ties among the maxima >= 0 only
        ymax = y.reshape(N, Cc, 1, -1)
        assert bool((((cols == ymax) & (ymax > 0)).sum(2) > 1).any()), "a tie inside a window"
    x, gy = C.pool_case(N, H, W, Cc, "nan")
    y, dx = C.pool_reference(x, gy)
    assert int(torch.isnan(x).sum()) == N and bool(torch.isnan(y).any()) and not bool(torch.isnan(dx).any())
    iy, ix = min(1, H - 1), min(2, W - 1)
    assert float(dx[0, 1, iy, ix]) == float(gy[0, 1][torch.isnan(y[0, 1])].sum()), "ATen: the NaN takes every window that holds it"
    x, gy = C.pool_case(N, H, W, Cc, "neginf")
    y, dx = C.pool_reference(x, gy)
    assert float(y[0, 0, 0, 0]) == float("-inf") and float(dx[0, 0, 0, 0]) == float(gy[0, 0, 0, 0]), "ATen: first in-bounds element"
    if H >= 4 and W >= 4:
        assert float(y[0, 0, 1, 1]) == float("-inf") and float(dx[0, 0, 1, 1]) == float(gy[0, 0, 1, 1]), "the interior all -inf window"


def test_pool_table_has_odd_and_rectangular_maps():
    assert any(H % 2 and W % 2 and H != W for _, H, W, _ in C.POOL_TABLE) and any(H == 1 and W == 1 for _, H, W, _ in C.POOL_TABLE)
    assert all(Cc % 4 == 0 for *_, Cc in C.POOL_TABLE)


def test_im2col_cases_cover_short_and_ragged_row_blocks():
    ms = [N * ((H + 2 * pad - k) // stride + 1) * ((W + 2 * pad - k) // stride + 1) for N, _, H, W, k, stride, pad, _ in C.IM2COL_TABLE]
    assert any(m < C.IM2COL_ROWS_PER_BLOCK for m in ms) and any(m > C.IM2COL_ROWS_PER_BLOCK and m % C.IM2COL_ROWS_PER_BLOCK for m in ms)
    assert any(Kp > Cin * k * k for _, Cin, _, _, k, _, _, Kp in C.IM2COL_TABLE) and all(Kp % 4 == 0 and Kp >= Cin * k * k for _, Cin, _, _, k, _, _, Kp in C.IM2COL_TABLE)
    x = torch.arange(2 * 1 * 5 * 6, dtype=torch.float32).reshape(2, 1, 5, 6)
    col = C.im2col_reference(x, 3, 1, 1)
    assert col.shape == (60, 9) and float(col[0, 4]) == 0.0 and float(col[0, 0]) == 0.0 and float(col[7, 4]) == 7.0 and float(col[7, 5]) == 8.0 and float(col[30, 4]) == 30.0


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
def test_hash_model_is_deterministic_and_keeps_at_the_binomial_rate():
    n = 1 << 18
    # murmur3's 64-bit finaliser maps 0 to 0, and has published vectors
    assert int(C.hash_u32(np.array([0], dtype=np.uint64))[0]) == 0
    x = 1
    x ^= x >> 33; x = (x * 0xff51afd7ed558ccd) & C._M64; x ^= x >> 33; x = (x * 0xc4ceb9fe1a85ec53) & C._M64; x ^= x >> 33
    assert int(C.hash_u32(np.array([1], dtype=np.uint64))[0]) == (x >> 16) & 0xffffffff
    for seed, offset, step in C.RNG_STREAMS:
        u = C.rng_uniform(n, seed, offset, step)
        assert u.dtype == np.float32 and 0.0 <= float(u.min()) and float(u.max()) < 1.0
        for p in C.RNG_PS:
            a, b = C.rng_mask_model(n, seed, offset, p, step), C.rng_mask_model(n, seed, offset, p, step)
            assert np.array_equal(a, b)
            keep = 1.0 - float(np.float32(p))
            sigma = np.sqrt(n * keep * (1.0 - keep))
            assert abs(float(a.sum()) - n * keep) <= 5.0 * sigma + 1e-9, (seed, offset, step, p)
        assert bool(C.rng_mask_model(n, seed, offset, 0.0, step).all())
    a = C.rng_mask_model(n, 7, 0, 0.5)
    assert not np.array_equal(a, C.rng_mask_model(n, 8, 0, 0.5)) and not np.array_equal(a, C.rng_mask_model(n, 7, 0, 0.5, 0 + 1))
    assert np.array_equal(a, C.rng_mask_model(n, 7, 0, 0.5, 0)), "step counter 0 is the stream without a counter"
    o = 777
    assert np.array_equal(C.rng_mask_model(n - o, 7, 2 ** 40 + o, 0.5), C.rng_mask_model(n, 7, 2 ** 40, 0.5)[o:])
    assert not np.array_equal(C.rng_mask_model(n, 7, 2 ** 40, 0.5), a)


def test_float64_adam_first_step_is_the_closed_form():
    g = C.gen(53)
    p0, gr = torch.randn(C.ADAM_CHUNK, generator=g).double(), torch.randn(C.ADAM_CHUNK, generator=g)
    for cfg in C.ADAM_CONFIGS:
        wd, gs, (b1, b2), eps = (C.f32(cfg[0]), C.f32(cfg[1]), tuple(C.f32(b) for b in cfg[2]), C.f32(cfg[3]))
        P, M, V, steps = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), [0]
        C.adam_reference(P, M, V, gr, steps, [1], [0], cfg)
        ge = gr.double() * gs + wd * p0
        want = p0 - C.f32(C.ADAM_LR) * ge / (ge.abs() + eps)                  # m / (1 - b1) = g, v / (1 - b2) = g^2
        assert steps == [1] and float((P - want).abs().max()) < 1e-12
        assert float((M - (1.0 - b1) * ge).abs().max()) < 1e-15 and float((V - (1.0 - b2) * ge * ge).abs().max()) < 1e-15
        before = P.clone()
        C.adam_reference(P, M, V, gr, steps, [0], [0], cfg)
        assert steps == [1] and torch.equal(P, before), "an inactive tensor does not move and does not count"


def test_adam_configs_and_slabs_cover_what_they_claim():
    assert {c[0] for c in C.ADAM_CONFIGS} == {0.0, 0.01} and {c[1] for c in C.ADAM_CONFIGS} == {1.0, 0.5, 0.125}
    assert {c[2] for c in C.ADAM_CONFIGS} == {(0.9, 0.999), (0.5, 0.9)} and {c[3] for c in C.ADAM_CONFIGS} == {1e-8, 1e-3}
    assert -1 in C.ADAM_C2T and C.ADAM_C2T.count(2) == 2 and C.ADAM_NEVER in C.ADAM_C2T
    assert [int(C.adam_active(s)[1]) for s in range(1, 6)] == [1, 0, 1, 0, 1]
    assert C.ADAM_BIG_CHUNKS > C.ADAM_GRID_CAP and sum(ch >= C.ADAM_GRID_CAP for ch in C.ADAM_BIG_LIVE) == 2 and max(C.ADAM_BIG_LIVE) < C.ADAM_BIG_CHUNKS
    assert C.ADAM_BIG_CHUNKS * C.ADAM_CHUNK * 4 < 72 * 2 ** 20


def test_ema_and_rng_sizes_exceed_the_grid_caps():
    assert max(C.EMA_NS) > C.EMA_GRID_CAP * 256 * 4 and all(n % 4 == 0 for n in C.EMA_NS) and max(C.EMA_NS) == 8392708
    assert max(C.RNG_NS) > C.RNG_GRID_CAP * 256 and max(C.RNG_NS) == 4195304
    assert any(s >= 2 ** 32 for s, _, _ in C.RNG_STREAMS) and any(s == 0 for s, _, _ in C.RNG_STREAMS) and any(o == 2 ** 40 for _, o, _ in C.RNG_STREAMS)
    assert {0, 1, 5} <= {st for _, _, st in C.RNG_STREAMS}
    e, v = C.ema_case(1024)
    assert torch.equal(C.ema_reference(e, v, 0.0), v)
