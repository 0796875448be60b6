"""The six attention kernels of csrc/transformer.hip through the C ABI (`stil_attention_fwd` / `stil_attention_bwd`), each
compared with a float64 evaluation of the definition (tests/attention_cases.py) at rectangular and ragged windows.

What one case checks, for an overlapping and a disjoint placement of the two windows (q_off != kv_off, both non-zero) and three
kinds of input (randn; logits of about +-50, a nearly one-hot softmax; a keep-mask at p = 0.1 with one query row fully dropped
and one fully kept):
  * `out`, `probs` and `dqkv` against float64, within 4 x the largest error fp32 ATen makes on the inputs of that kind
    (attention_cases.bounds(), capped at test_gpu_ops.py::test_attention's 2e-5 / 2e-5 / 5e-5; DESIGN.md section 2 records the figures);
  * exactly: `probs` is the same with and without a mask; every element outside the query rows of `out`, outside the Q rows of
    the query window and the K / V rows of the key window of `dqkv`, and in the margins around all three buffers keeps its
    sentinel bit for bit; a second backward into the same `dqkv` doubles it exactly (the += contract);
  * whatever a kernel must not read (other tokens, other slots, other rows of dout) holds NaN.
`stil_attention_config` names the kernel each case runs, and the module asserts that every kernel is reached by a ragged square,
by Sq < Skv and by Sq > Skv.  Each comparison prints its figure (`ATTN_ERR ...`) before it asserts."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as A  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -777.0
MARGIN = 64          # floats of sentinel before and after each output buffer


@pytest.fixture(scope="module")
def L():
    from stil_tta_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def bounds():
    return A.bounds()


def _st():
    from stil_tta_amd.ops import _stream
    return _stream()


def P(t):
    return None if t is None else t.data_ptr()


def guarded(shape):
    """-> (flat buffer, view of `shape` in its middle), all SENT, MARGIN floats of it on either side"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * MARGIN,), SENT, dtype=torch.float32, device="cuda")
    return flat, flat[MARGIN:MARGIN + n].view(shape)


def untouched(t):
    """every element still holds the sentinel's bits"""
    return bool((t.contiguous().view(torch.int32) == torch.tensor(SENT).view(torch.int32).item()).all())


def margins_untouched(flat):
    return untouched(flat[:MARGIN]) and untouched(flat[-MARGIN:])


def report(case, wi, kind, key, a, b, bound):
    e = A.nerr(a, b)
    print(f"ATTN_ERR {A.case_id(case)} fwd={case[5]} bwd={case[6]} win={wi} {kind} {key} {e:.3e} bound {bound:.3e}")
    return e


def test_every_kernel_is_reached_in_every_orientation(L):
    codes = {c[:3]: (L.attention_config(*c[:3], 0), L.attention_config(*c[:3], 1)) for c in A.CASES}
    assert codes == {c[:3]: c[5:] for c in A.CASES}, "the dispatch no longer sends the cases to the kernels listed in attention_cases.py"
    assert A.coverage_gaps(codes) == []


@pytest.mark.parametrize("case", A.CASES, ids=A.case_id)
def test_attention_kernels_against_float64(L, bounds, case):
    Sq, Skv, d, B, H, fwd_code, bwd_code = case
    assert (L.attention_config(Sq, Skv, d, 0), L.attention_config(Sq, Skv, d, 1)) == (fwd_code, bwd_code)
    scale = d ** -0.5
    failures = []
    for wi, (q_off, kv_off, T) in enumerate(A.windows(Sq, Skv)):
        for kind in A.KINDS:
            qkv, dout, mask, p = A.make_inputs(case, kind, wi)
            ref = A.attn_eval(qkv, dout, mask, p, q_off, Sq, kv_off, Skv, torch.float64)
            qkv_d, dout_d = qkv.cuda(), dout.cuda()
            mask_d = None if mask is None else mask.cuda()
            out_f, out = guarded((B, T, H * d))
            pr_f, pr = guarded((B, H, Sq, Skv))
            L.attention_fwd(P(qkv_d), P(out), P(pr), P(mask_d), B, T, H, d, q_off, Sq, kv_off, Skv, scale, p, _st())
            torch.cuda.synchronize()
            for key, got in (("out", out[:, q_off:q_off + Sq]), ("probs", pr)):
                if not report(case, wi, kind, key, got, ref[key], bounds[kind][key]) <= bounds[kind][key]:   # a NaN fails too
                    failures.append((wi, kind, key))
            rows = torch.ones(T, dtype=torch.bool)
            rows[q_off:q_off + Sq] = False
            assert untouched(out[:, rows.cuda()]), f"out written outside the query rows (win {wi}, {kind})"
            assert margins_untouched(out_f) and margins_untouched(pr_f), f"forward wrote past a buffer (win {wi}, {kind})"
            if kind == "mask":         # the maskless forward on the same q, k
                _, pr2 = guarded((B, H, Sq, Skv))
                _, out2 = guarded((B, T, H * d))
                L.attention_fwd(P(qkv_d), P(out2), P(pr2), None, B, T, H, d, q_off, Sq, kv_off, Skv, scale, 0.0, _st())
                torch.cuda.synchronize()
                assert torch.equal(pr2.view(torch.int32), pr.view(torch.int32)), f"probs depend on the mask (win {wi})"
            if bwd_code < 0:
                continue
            dq_f, dqkv = guarded((B, T, 3, H, d))
            dqkv[:, q_off:q_off + Sq, 0] = 0.0
            dqkv[:, kv_off:kv_off + Skv, 1:] = 0.0
            args = (P(dout_d), P(qkv_d), P(pr), P(mask_d), P(dqkv), B, T, H, d, q_off, Sq, kv_off, Skv, scale, p, _st())
            L.attention_bwd(*args)
            torch.cuda.synchronize()
            once = dqkv.clone()
            inside = torch.zeros(T, 3, dtype=torch.bool)
            inside[q_off:q_off + Sq, 0] = True
            inside[kv_off:kv_off + Skv, 1:] = True
            inside = inside.cuda()
            got = torch.where(inside[None, :, :, None, None], once, torch.zeros_like(once))
            if not report(case, wi, kind, "dqkv", got, ref["dqkv"], bounds[kind]["dqkv"]) <= bounds[kind]["dqkv"]:
                failures.append((wi, kind, "dqkv"))
            assert untouched(once.permute(1, 2, 0, 3, 4)[~inside]), f"dqkv written outside the two windows (win {wi}, {kind})"
            assert margins_untouched(dq_f), f"backward wrote past dqkv (win {wi}, {kind})"
            L.attention_bwd(*args)
            torch.cuda.synchronize()
            twice = dqkv.permute(1, 2, 0, 3, 4)[inside]
            assert torch.equal(twice, 2.0 * once.permute(1, 2, 0, 3, 4)[inside]), f"a second backward is not += (win {wi}, {kind})"
            assert untouched(dqkv.permute(1, 2, 0, 3, 4)[~inside]) and margins_untouched(dq_f)
    assert not failures, f"beyond the bound {bounds}: {failures}"


@pytest.mark.parametrize("Sq,Skv,d", A.REFUSED_BWD)
def test_refused_backward_launches_nothing(L, Sq, Skv, d):
    """no backward kernel fits 160 KiB of LDS: the entry point refuses on the host, names the reason and writes nothing"""
    assert L.attention_config(Sq, Skv, d, 1) < 0 <= L.attention_config(Sq, Skv, d, 0)
    B, H, T = 1, 2, Sq + 8
    qkv = torch.randn(B, T, 3, H, d, device="cuda")
    dout = torch.randn(B, T, H * d, device="cuda")
    pr = torch.rand(B, H, Sq, Skv, device="cuda")
    dq_f, dqkv = guarded((B, T, 3, H, d))
    with pytest.raises(RuntimeError, match=r"stil_attention_bwd.*LDS"):
        L.attention_bwd(P(dout), P(qkv), P(pr), None, P(dqkv), B, T, H, d, 2, Sq, 5, Skv, d ** -0.5, 0.0, _st())
    assert "160 KiB" in L.last_error()
    torch.cuda.synchronize()
    assert untouched(dq_f)


def test_forward_that_needs_a_gradient_refuses_what_the_backward_would():
    """ops.attention at (129, 129, d = 64): the forward kernel takes it, the backward would not -- with a gradient to come the
    call fails before any launch; under no_grad it runs and matches float64"""
    from stil_tta_amd import ops
    Sq = Skv = 129
    d, B, H, T = 64, 1, 2, 129
    g = torch.Generator().manual_seed(129)
    qkv = torch.randn(B, T, 3, H, d, generator=g)
    qd = qkv.reshape(B, T, 3 * H * d).cuda().requires_grad_()
    with pytest.raises(RuntimeError, match="stil_attention_bwd would refuse"):
        ops.attention(qd, H, [(0, Sq, 0, Skv)])
    with torch.no_grad():
        o = ops.attention(qd, H, [(0, Sq, 0, Skv)])
    ref = A.attn_eval(qkv, torch.zeros(B, T, H * d), None, 0.0, 0, Sq, 0, Skv, torch.float64)["out"]
    e = A.nerr(o, ref)
    bound = A.bounds()["randn"]["out"]
    print(f"ATTN_ERR 129x129x64 no_grad out {e:.3e} bound {bound:.3e}")
    assert e <= bound
