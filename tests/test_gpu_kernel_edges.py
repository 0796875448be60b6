"""The kernels every STiL step runs, at the shapes where they branch (tests/kernel_edge_cases.py): each test calls the entry point
(through `_lib.lib()` or its thin `ops` wrapper) and compares with the float64 or exact integer reference of the cases module,
never with another kernel of the library.  Float outputs: the suite's `close()` at `TOL` (`rel_close` where magnitudes are far
below 1); tests/test_kernel_edge_inputs_cpu.py asserts on the CPU that fp32 ATen meets the same checks (the `check_*` functions
below) on the same inputs, so a kernel that misses one is wrong, not unlucky.  Discrete outputs, masks, copies and the
optimizer's untouched regions are compared exactly, on sentinel-filled buffers with NaN where nothing may be read."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_edge_cases as C  # noqa: E402
from test_gpu_entry_points import NAN, SENT, TOL, P, _release_operands, _st, close, dev, out_strided, rel_close, strided  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from stil_tta_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from stil_tta_amd._lib import lib
    return lib()


def sent(*shape, dtype=torch.float32, fill=SENT):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


# ---------------------------------------------------------------------------------------------------------------------
# the float checks, shared with the CPU test (which feeds them fp32 ATen instead of the kernel)
# ---------------------------------------------------------------------------------------------------------------------
def check_cgpl_floats(out, ref):
    for k in ("pseudo_label", "pseudo_orig", "prediction"):
        if out.get(k) is not None:
            close(out[k], ref[k], name=k)


def check_proto_accum(out, ref):
    close(out, ref, name="class_sum_cnt")


def check_clip(loss, dz, ref_loss, ref_dz):
    close(loss, ref_loss, name="clip loss")
    rel_close(dz, ref_dz, "clip dZ")


def check_club(out, ref):
    for a, b, name in zip(out, ref, ("club", "est", "dmu", "dy")):
        close(a, b, name=name)


def check_ln(out, ref, keys=("y", "mean_rstd", "dx", "dgamma", "dbeta")):
    for k in keys:
        close(out[k], ref[k], name=k)


def check_adam(p, m, v, P64, M64, V64):
    """on the live elements: scaled error (close()'s own measure) within ADAM_BOUND = 4 x ATen-fp32's"""
    for name, a, b in (("p", p, P64), ("m", m, M64), ("v", v, V64)):
        err = C.scaled_err(a, b)
        assert err <= C.ADAM_BOUND[name], f"adam {name}: scaled error {err:.3e} > {C.ADAM_BOUND[name]:.3e}"


# =====================================================================================================================
# A. csrc/loss.hip
# =====================================================================================================================
def _onehot(L, p, th):
    rows, K = p.shape
    oh, mask, idx = sent(rows + 1, K), sent(rows + 1), sent(rows + 1, dtype=torch.int32, fill=-5)
    L.onehot_argmax(P(dev(p)), rows, K, th, P(oh), P(mask), P(idx), _st())
    torch.cuda.synchronize()
    assert bool((oh[rows] == SENT).all()) and float(mask[rows]) == SENT and int(idx[rows]) == -5, "a write past the last row"
    return oh[:rows].cpu(), mask[:rows].cpu(), idx[:rows].cpu()


@pytest.mark.parametrize("K", C.ONEHOT_KS)
@pytest.mark.parametrize("rows", C.ONEHOT_ROWS)
def test_onehot_argmax_beyond_one_wave(L, rows, K):
    p, th, idx_ref, mask_ref = C.onehot_case(rows, K)
    oh, mask, idx = _onehot(L, p, th)
    assert torch.equal(idx, idx_ref), (idx.tolist(), idx_ref.tolist())
    assert torch.equal(mask, mask_ref)
    assert torch.equal(oh, F.one_hot(idx_ref.long(), K).float())


def test_onehot_argmax_ties_across_and_within_lanes_and_at_the_threshold(L):
    p, th, idx_ref, mask_ref = C.onehot_tie_case()
    oh, mask, idx = _onehot(L, p, th)
    assert torch.equal(idx, idx_ref), (idx.tolist(), idx_ref.tolist())
    assert torch.equal(mask, mask_ref), (mask.tolist(), mask_ref.tolist())
    assert torch.equal(oh, F.one_hot(idx_ref.long(), C.TIE_K).float())


@pytest.mark.parametrize("want_orig", [False, True])
@pytest.mark.parametrize("use_pseudo", [False, True])
@pytest.mark.parametrize("Bu,K,Dp", C.CGPL_TABLE)
def test_cgpl_pgls_at_every_width(L, Bu, K, Dp, use_pseudo, want_orig):
    c = C.cgpl_case(Bu, K, Dp)
    ld = c["ld"]
    zs = [strided(c[k], ld - K)[1] if ld > K else dev(c[k]) for k in ("zm", "zi", "zt")]
    assert all(z.stride(0) == ld for z in zs)
    pl, pred = sent(Bu + 1, K), sent(Bu + 1, K)
    po = sent(Bu + 1, K) if want_orig else None
    flags, hard, w3 = sent(Bu + 1, 4, dtype=torch.uint8, fill=99), sent(Bu + 1, dtype=torch.int32, fill=-5), sent(3 * Bu + 1)
    pin = None if c["pred_in"] is None else dev(c["pred_in"])
    L.cgpl_pgls(P(zs[0]), P(zs[1]), P(zs[2]), ld, P(dev(c["feat"])), P(dev(c["protos"])), P(dev(c["mr"])), P(pl), P(po), P(pred), P(flags), P(hard),
                P(w3), P(pin), Bu, K, Dp, C.CGPL_R, C.CGPL_T, c["th"], 1 if use_pseudo else 0, _st())
    torch.cuda.synchronize()
    ref = C.cgpl_reference(c, torch.float64, use_pseudo)
    check_cgpl_floats({"pseudo_label": pl[:Bu], "pseudo_orig": None if po is None else po[:Bu], "prediction": pred[:Bu]}, ref)
    flags_ref, hard_ref, w3_ref = C.cgpl_discrete(c, use_pseudo)
    assert torch.equal(flags[:Bu].cpu(), flags_ref), (flags[:Bu, 0].tolist(), flags_ref[:, 0].tolist())
    assert torch.equal(hard[:Bu].cpu(), hard_ref), (hard[:Bu].tolist(), hard_ref.tolist())
    assert torch.equal(w3[:3 * Bu].cpu().view(3, Bu), w3_ref)
    if not use_pseudo:
        assert bool((pred[:Bu] == 0).all())
    for buf in (pl, pred) + ((po,) if want_orig else ()):
        assert bool((buf[Bu] == SENT).all()), "a write past the last row"
    assert bool((flags[Bu] == 99).all()) and int(hard[Bu]) == -5 and float(w3[3 * Bu]) == SENT


@pytest.mark.parametrize("repeat_ratio", C.REPEAT_RATIOS)
@pytest.mark.parametrize("B,B_l,K,Dp", C.PROTO_ACCUM_TABLE)
def test_proto_accum(L, B, B_l, K, Dp, repeat_ratio):
    feat, hard, conf = C.proto_accum_case(B, B_l, K, Dp)
    out = sent(K + 1, Dp + 1)
    L.proto_accum(P(dev(feat)), P(dev(hard)), P(dev(conf)), P(out), B, B_l, K, Dp, repeat_ratio, _st())
    torch.cuda.synchronize()
    ref = C.proto_accum_reference(feat, hard, conf, B_l, K, repeat_ratio, torch.float64)
    check_proto_accum(out[:K], ref)
    assert bool((out[K] == SENT).all()), "a write past the last class"
    empty = ref[:, Dp] == 0
    assert bool(empty[K - 1]) and bool((out[:K].cpu()[empty] == 0).all()), "a class without a member is a zero row and a zero count"


@pytest.mark.parametrize("lam0,lam1", C.CLIP_LAMS)
@pytest.mark.parametrize("B", C.CLIP_BS)
def test_clip_fwd_bwd_on_a_logit_matrix(L, B, lam0, lam1):
    Z = C.clip_case(B)
    Zd, lse, terms, loss = dev(Z), sent(2 * B + 1, dtype=torch.float64), sent(B + 1), sent(2)
    L.clip_fwd(P(Zd), P(lse), P(terms), P(loss), B, lam0, lam1, _st())
    dZ = sent(B * B + 1)
    L.clip_bwd(P(Zd), P(lse), P(dev(torch.tensor([C.CLIP_G]))), P(dZ), B, lam0, lam1, _st())
    torch.cuda.synchronize()
    ref_loss, ref_dz = C.clip_reference(Z, lam0, lam1, torch.float64)
    check_clip(loss[0], dZ[:B * B].view(B, B), ref_loss, ref_dz)
    close(lse[:B], torch.logsumexp(Z.double(), 1), name="row log-sum-exp")
    close(lse[B:2 * B], torch.logsumexp(Z.double(), 0), name="column log-sum-exp")
    assert float(lse[2 * B]) == SENT and float(terms[B]) == SENT and float(loss[1]) == SENT and float(dZ[B * B]) == SENT


@pytest.mark.parametrize("R,D", C.CLUB_TABLE)
def test_club_against_the_materialised_form(ops, R, D):
    mu, y = C.club_case(R, D)
    md, yd = dev(mu).requires_grad_(), dev(y).requires_grad_()
    c, e = ops.ClubFn.apply(md, yd)
    (C.CLUB_G[0] * c + C.CLUB_G[1] * e).backward()
    check_club((c, e, md.grad, yd.grad), C.club_reference(mu, y, torch.float64))


# =====================================================================================================================
# B. csrc/optim.hip, rng_mask
# =====================================================================================================================
def _adam(L, Pd, Gd, Md, Vd, c2t, steps, active, cfg):
    wd, gs, (b1, b2), eps = cfg
    L.adam_step(P(Pd), P(Gd), P(Md), P(Vd), P(c2t), P(steps), P(active), len(steps), Pd.numel(), C.ADAM_LR, b1, b2, eps, wd, gs, _st())


@pytest.mark.parametrize("cfg_index", range(len(C.ADAM_CONFIGS)))
def test_adam_five_steps_with_padding_and_a_lagging_tensor(L, cfg_index):
    cfg = C.ADAM_CONFIGS[cfg_index]
    P0, Gs = C.adam_case(cfg_index)
    live = C.adam_live_mask()
    M0 = torch.zeros_like(P0)
    M0[~live] = SENT
    Pd, Md, Vd = dev(P0), dev(M0), dev(M0.clone())
    c2t, steps = dev(torch.tensor(C.ADAM_C2T, dtype=torch.int32)), dev(torch.zeros(len(C.ADAM_NUMEL), dtype=torch.int32))
    lag = torch.tensor([t == 1 for t in C.ADAM_C2T]).repeat_interleave(C.ADAM_CHUNK)
    for i, G in enumerate(Gs):
        act = C.adam_active(i + 1)
        before = [t.cpu() for t in (Pd, Md, Vd)]
        _adam(L, Pd, dev(G), Md, Vd, c2t, steps, dev(act), cfg)
        torch.cuda.synchronize()
        frozen = ~live | (lag if not act[1] else torch.zeros_like(lag))
        for name, b, a in zip("pmv", before, (Pd, Md, Vd)):
            assert torch.equal(a.cpu()[frozen].view(torch.int32), b[frozen].view(torch.int32)), f"step {i + 1}: {name} changed where nothing is active"
            assert bool((a.cpu()[~live] == SENT).all())
    P64, M64, V64, steps_ref = C.adam_run_reference(cfg_index)
    assert steps.cpu().tolist() == steps_ref == [5, 3, 5, 5, 0]
    check_adam(Pd.cpu()[live], Md.cpu()[live], Vd.cpu()[live], P64[live], M64[live], V64[live])


def test_adam_slab_beyond_the_grid_cap(L):
    """16384 + 3 chunks, all padding but four: chunks 16384 and 16386 are reached only by the second trip of the chunk loop"""
    nch, cfg = C.ADAM_BIG_CHUNKS, C.ADAM_CONFIGS[2]
    assert nch > C.ADAM_GRID_CAP and max(C.ADAM_BIG_LIVE) >= C.ADAM_GRID_CAP
    n = nch * C.ADAM_CHUNK
    g = C.gen(nch, 43)
    c2t = torch.full((nch,), -1, dtype=torch.int32)
    Pd, Md, Vd, Gd = sent(n), sent(n), sent(n), sent(n, fill=NAN)
    p0, m0, v0, g0 = (torch.randn(4 * C.ADAM_CHUNK, generator=g), 0.1 * torch.randn(4 * C.ADAM_CHUNK, generator=g),
                      0.1 * torch.rand(4 * C.ADAM_CHUNK, generator=g), torch.randn(4 * C.ADAM_CHUNK, generator=g))
    for j, ch in enumerate(C.ADAM_BIG_LIVE):
        c2t[ch] = j
        s, d = slice(j * C.ADAM_CHUNK, (j + 1) * C.ADAM_CHUNK), slice(ch * C.ADAM_CHUNK, (ch + 1) * C.ADAM_CHUNK)
        Pd[d], Md[d], Vd[d], Gd[d] = p0[s].cuda(), m0[s].cuda(), v0[s].cuda(), g0[s].cuda()
    steps0 = [2, 0, 7, 1]
    steps, active = dev(torch.tensor(steps0, dtype=torch.int32)), dev(torch.ones(4, dtype=torch.uint8))
    _adam(L, Pd, Gd, Md, Vd, dev(c2t), steps, active, cfg)
    torch.cuda.synchronize()
    P64, M64, V64, st = p0.double(), m0.double(), v0.double(), list(steps0)
    C.adam_reference(P64, M64, V64, g0, st, [1] * 4, [0, 1, 2, 3], cfg)
    assert steps.cpu().tolist() == st
    livem = torch.zeros(n, dtype=torch.bool, device="cuda")
    got = []
    for t in (Pd, Md, Vd):
        got.append(torch.cat([t[ch * C.ADAM_CHUNK:(ch + 1) * C.ADAM_CHUNK] for ch in C.ADAM_BIG_LIVE]).cpu())
    for ch in C.ADAM_BIG_LIVE:
        livem[ch * C.ADAM_CHUNK:(ch + 1) * C.ADAM_CHUNK] = True
    for name, t in zip("pmv", (Pd, Md, Vd)):
        assert bool((t[~livem] == SENT).all()), f"{name}: a padding chunk was written"
    check_adam(*got, P64, M64, V64)


@pytest.mark.parametrize("m", C.EMA_MOMENTA)
@pytest.mark.parametrize("n", C.EMA_NS)
def test_ema_update_is_bit_exact_past_the_grid_cap(L, n, m):
    assert max(C.EMA_NS) > C.EMA_GRID_CAP * 256 * 4
    e, v = C.ema_case(n)
    ed, vd = dev(torch.cat([e, torch.full((8,), SENT)])), dev(v)
    L.ema_update(P(ed), P(vd), n, m, _st())
    torch.cuda.synchronize()
    assert torch.equal(ed[:n].cpu(), C.ema_reference(e, v, m)), "EMA must be bit-exact"
    assert bool((ed[n:] == SENT).all()) and torch.equal(vd.cpu(), v)


def test_ema_update_on_a_sub_slab(L):
    """flat.py ema_update_range: the call starts 1024 floats into both slabs; the neighbours must not move"""
    off, n, m = 1024, 2048, 0.996
    e, v = C.ema_case(n)
    eb, vb = torch.full((off + n + 1024,), SENT), torch.full((off + n + 1024,), NAN)
    eb[off:off + n], vb[off:off + n] = e, v
    ed, vd = dev(eb), dev(vb)
    L.ema_update(ctypes.c_void_p(ed.data_ptr() + 4 * off), ctypes.c_void_p(vd.data_ptr() + 4 * off), n, m, _st())
    torch.cuda.synchronize()
    eb[off:off + n] = C.ema_reference(e, v, m)
    assert torch.equal(ed.cpu(), eb)


def _mask(L, n, seed, offset, p, step_dev):
    out = sent(n + 64, dtype=torch.uint8, fill=7)
    L.rng_mask(P(out), n, seed, offset, p, P(step_dev), _st())
    torch.cuda.synchronize()
    assert bool((out[n:] == 7).all()), "bytes after n were written"
    return out[:n].cpu().numpy()


@pytest.mark.parametrize("p", C.RNG_PS)
@pytest.mark.parametrize("n", C.RNG_NS)
def test_rng_mask_equals_the_integer_model_byte_for_byte(L, n, p):
    assert max(C.RNG_NS) > C.RNG_GRID_CAP * 256
    for seed, offset, step in C.RNG_STREAMS:
        step_dev = None
        if step is not None:
            step_dev = dev(torch.zeros(1, dtype=torch.int64))
            for _ in range(step):
                L.counter_inc(P(step_dev), _st())
            assert int(step_dev.item()) == step
        got = _mask(L, n, seed, offset, p, step_dev)
        want = C.rng_mask_model(n, seed, offset, p, step)
        assert np.array_equal(got, want), f"seed {seed} offset {offset} step {step}: {int((got != want).sum())} of {n} bytes differ"


def test_rng_mask_offset_continues_the_stream(L):
    n, o, seed, p = 5000, 777, 2022, 0.5
    for base in (0, 2 ** 40):
        a = _mask(L, n, seed, base + o, p, None)
        b = _mask(L, n + o, seed, base, p, None)
        assert np.array_equal(a, b[o:]) and np.array_equal(b, C.rng_mask_model(n + o, seed, base, p))


# =====================================================================================================================
# C. csrc/bn.hip, csrc/transformer.hip
# =====================================================================================================================
def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.cpu().permute(0, 3, 1, 2).contiguous()


def _same(a, b):
    """equal, NaN matching NaN (and infinities by sign)"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, 0.0, 1e30, -1e30), torch.nan_to_num(b, 0.0, 1e30, -1e30))


def run_pool(L, x, gy):
    N, Cc, H, W = x.shape
    OH, OW = gy.shape[2:]
    xd, gd = dev(_nhwc(x)), dev(_nhwc(gy))
    y, idx, dx = sent(N, OH, OW, Cc), sent(N, OH, OW, Cc, dtype=torch.uint8, fill=99), sent(N, H, W, Cc)
    L.maxpool3x3s2_fwd(P(xd), P(y), P(idx), N, H, W, Cc, OH, OW, _st())
    L.maxpool3x3s2_bwd(P(gd), P(idx), P(dx), N, H, W, Cc, OH, OW, _st())
    torch.cuda.synchronize()
    return _nchw(y), _nchw(dx)


@pytest.mark.parametrize("kind", C.POOL_KINDS)
@pytest.mark.parametrize("N,H,W,Cc", C.POOL_TABLE)
def test_maxpool_ties_nan_and_all_minus_inf_windows_route_like_aten(L, N, H, W, Cc, kind):
    x, gy = C.pool_case(N, H, W, Cc, kind)
    y_ref, dx_ref = C.pool_reference(x, gy)
    y, dx = run_pool(L, x, gy)
    assert _same(y, y_ref), "forward"
    assert torch.equal(dx, dx_ref), f"dx differs from ATen at {int((dx != dx_ref).sum())} elements; first image, channel 0:\n{dx[0, 0]}\nATen:\n{dx_ref[0, 0]}"
    if kind == "nan":
        iy, ix = min(1, H - 1), min(2, W - 1)
        wins = [(oy, ox) for oy in range(y.shape[2]) for ox in range(y.shape[3]) if abs(2 * oy - iy) <= 1 and abs(2 * ox - ix) <= 1]
        assert wins and all(bool(torch.isnan(y[:, 1, oy, ox]).all()) for oy, ox in wins)
        assert int(torch.isnan(y).sum()) == N * len(wins)
        assert torch.equal(dx[:, 1, iy, ix], sum(gy[:, 1, oy, ox] for oy, ox in wins))
    if kind == "neginf":
        assert torch.equal(dx[:, 0, 0, 0], gy[:, 0, 0, 0]), "the all -inf corner window's gradient goes to its first in-bounds element"


@pytest.mark.parametrize("N,Cin,H,W,k,stride,pad,Kp", C.IM2COL_TABLE)
def test_im2col_nchw_equals_unfold(L, N, Cin, H, W, k, stride, pad, Kp):
    x = torch.randn(N, Cin, H, W, generator=C.gen(N, Cin, H, W, k))
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    M, K, spare = N * OH * OW, Cin * k * k, 5
    col = sent(M + spare, Kp, fill=NAN)
    L.im2col_nchw(P(dev(x)), P(col), N, Cin, H, W, OH, OW, k, k, stride, pad, Kp, _st())
    torch.cuda.synchronize()
    col = col.cpu()
    assert torch.equal(col[:M, :K], C.im2col_reference(x, k, stride, pad))
    assert bool((col[:M, K:] == 0).all()), "padding columns must be written as zero"
    assert bool(torch.isnan(col[M:]).all()), "rows beyond M were written"


@pytest.mark.parametrize("R,Cc", C.TRANSPOSE_TABLE)
def test_transpose_equals_t(L, R, Cc):
    x = torch.randn(R, Cc, generator=C.gen(R, Cc, 47))
    out = sent(R * Cc + 8)
    L.transpose(P(dev(x)), P(out), R, Cc, _st())
    torch.cuda.synchronize()
    assert torch.equal(out[:R * Cc].cpu().view(Cc, R), x.t().contiguous()) and bool((out[R * Cc:] == SENT).all())


def run_ln(L, x, gamma, beta, gy, dg0, db0, misalign=False):
    """forward, backward with accumulate = 0, backward with accumulate = 1 on prefilled accumulators -> dict (and the accumulated pair).
    misalign: x sits one float into its buffer, which sends forward and backward to the scalar kernels."""
    rows, D = x.shape
    if misalign:
        buf = dev(torch.cat([torch.full((1,), NAN), x.reshape(-1), torch.full((3,), NAN)]))
        xd = buf[1:1 + rows * D].view(rows, D)
        assert xd.data_ptr() % 16 == 4
    else:
        xd = dev(x)
        assert xd.data_ptr() % 16 == 0
    gm, bt, gd = dev(gamma), dev(beta), dev(gy)
    y, mr, dx = sent(rows * D + 4), sent(2 * rows + 2), sent(rows * D + 4)
    L.layernorm_fwd(P(xd), P(gm), P(bt), P(y), P(mr), rows, D, C.LN_EPS, _st())
    nb = L.layernorm_bwd_workspace_bytes(rows, D)
    ws = sent(nb // 4 + 4)
    dg, db = sent(D + 1), sent(D + 1)
    L.layernorm_bwd(P(gd), P(xd), P(gm), P(mr), P(dx), P(dg), P(db), rows, D, 0, P(ws), nb, _st())
    dga, dba = dev(torch.cat([dg0, torch.full((1,), SENT)])), dev(torch.cat([db0, torch.full((1,), SENT)]))
    L.layernorm_bwd(P(gd), P(xd), P(gm), P(mr), P(dx), P(dga), P(dba), rows, D, 1, P(ws), nb, _st())
    torch.cuda.synchronize()
    for t, n in ((y, rows * D), (mr, 2 * rows), (dx, rows * D), (dg, D), (db, D), (dga, D), (dba, D), (ws, nb // 4)):
        assert bool((t[n:] == SENT).all()), "a write past the end of an output"
    return {"y": y[:rows * D].view(rows, D), "mean_rstd": mr[:2 * rows].view(rows, 2), "dx": dx[:rows * D].view(rows, D), "dgamma": dg[:D], "dbeta": db[:D],
            "dgamma_acc": dga[:D], "dbeta_acc": dba[:D]}


def _ln_check(L, rows, D, misalign=False):
    x, gamma, beta, gy, dg0, db0 = C.ln_case(rows, D)
    out = run_ln(L, x, gamma, beta, gy, dg0, db0, misalign)
    ref = C.ln_reference(x, gamma, beta, gy, torch.float64)
    check_ln(out, ref)
    close(out["dgamma_acc"], dg0.double() + ref["dgamma"], name="dgamma, accumulate = 1")
    close(out["dbeta_acc"], db0.double() + ref["dbeta"], name="dbeta, accumulate = 1")


@pytest.mark.parametrize("rows,D", C.LN_VECTOR)
def test_layernorm_vector_kernels(L, rows, D):
    assert D % 4 == 0
    if rows == max(r for r, _ in C.LN_VECTOR):
        assert rows > C.LN_BLOCK_CAP * C.LN_ROWS_PER_BLOCK
    _ln_check(L, rows, D)


@pytest.mark.parametrize("rows,D", C.LN_SCALAR)
def test_layernorm_scalar_kernels_by_shape(L, rows, D):
    assert D % 4 != 0
    _ln_check(L, rows, D)


@pytest.mark.parametrize("misalign", [False, True])
def test_layernorm_both_instantiations_on_the_same_rows(L, misalign):
    _ln_check(L, *C.LN_ALIGN, misalign=misalign)


def test_layernorm_bwd_refuses_before_any_write(L):
    rows = 4
    for D, short in ((C.LN_MAX_D + 1, 0), (64, 4)):
        x, gamma, beta, gy, _, _ = C.ln_case(rows, D)
        nb = L.layernorm_bwd_workspace_bytes(rows, D)
        dx, dg, db, ws, mr = sent(rows * D), sent(D), sent(D), sent(nb // 4), dev(torch.ones(rows, 2))
        with pytest.raises(RuntimeError):
            L.layernorm_bwd(P(dev(gy)), P(dev(x)), P(dev(gamma)), P(mr), P(dx), P(dg), P(db), rows, D, 0, P(ws), nb - short, _st())
        torch.cuda.synchronize()
        for t in (dx, dg, db, ws):
            assert bool((t == SENT).all()), f"D = {D}: a refused call wrote"
