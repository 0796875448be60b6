"""Cases, inputs and references shared by tests/test_gpu_attention.py and tests/test_attention_config_cpu.py (no test lives
here).  One case = (Sq, Skv, d, B, H, fwd, bwd): a window of Sq queries and Skv keys at head dim d and the kernel code
`stil_attention_config` must report for its forward and backward (0 = VALU, 1 = 256-thread MFMA, 2 = 512-thread MFMA, -1 =
refused).  The codes are what the GPU test's coverage rests on; the CPU test compares them with the built library, so a retune
of the dispatch that drops a kernel from the coverage fails without a GPU.

Reference: softmax attention written from its definition with torch ops in a chosen dtype,
    S = scale Q K^T,  P = softmax(S),  Pd = P * keep / (1 - p),  O = Pd V,
    dV = Pd^T dO,  dP = (dO V^T) * keep / (1 - p),  dS = P * (dP - rowsum(dP * P)),  dQ = scale dS K,  dK = scale dS^T Q,
evaluated in float64 (the reference) and in float32 (ATen on the CPU: the yardstick the kernels' bound is derived from)."""
import torch

B_, H_ = 2, 3     # one workgroup per (batch, head); the odd H catches a wrong b / h split
CASES = [
    # 256-thread MFMA kernels
    (48, 48, 64, B_, H_, 1, 1), (30, 40, 128, B_, H_, 1, 1), (40, 44, 112, B_, H_, 1, 1), (44, 40, 112, B_, H_, 1, 1),
    (47, 77, 16, B_, H_, 1, 1), (31, 63, 64, B_, H_, 1, 1), (15, 47, 80, B_, H_, 1, 1),
    (47, 47, 64, B_, H_, 1, 1), (45, 45, 128, B_, H_, 1, 1), (67, 45, 64, B_, H_, 1, 1),   # added: ragged squares, and Sq > Skv past one tile row more
    (45, 47, 96, B_, H_, 1, 0), (40, 30, 128, B_, H_, 1, 0),
    (3, 47, 128, B_, H_, 0, 1), (47, 3, 128, B_, H_, 0, 1), (43, 1, 64, B_, H_, 0, 1), (16, 16, 16, B_, H_, 0, 1),
    (43, 43, 128, B_, H_, 0, 1), (77, 47, 16, B_, H_, 0, 1),    # added: a ragged square and Sq > Skv on the 256-thread backward alone
    # 512-thread MFMA kernels, rectangular
    (17, 113, 16, B_, H_, 2, 2), (113, 17, 16, B_, H_, 2, 2), (20, 120, 64, B_, H_, 2, 2), (120, 20, 64, B_, H_, 2, 2),
    (33, 90, 32, B_, H_, 2, 2), (90, 33, 48, B_, H_, 2, 2), (50, 61, 128, B_, H_, 2, 2), (61, 50, 80, B_, H_, 2, 2),
    (61, 61, 80, B_, H_, 2, 2),                                 # added: a ragged square on the 512-thread kernels
    # VALU kernels
    (1, 1, 16, B_, H_, 0, 0), (17, 17, 16, B_, H_, 0, 0), (33, 47, 64, B_, H_, 0, 0), (47, 33, 64, B_, H_, 0, 0),
    (31, 17, 112, B_, H_, 0, 0), (10, 23, 12, B_, H_, 0, 0), (23, 10, 20, B_, H_, 0, 0),
    # near the 160 KiB LDS limit
    (125, 128, 64, 1, 2, 2, 2), (128, 121, 64, 1, 2, 2, 2), (176, 170, 16, 1, 2, 2, 2), (90, 96, 128, 1, 2, 2, 2),
    (135, 135, 12, 1, 2, 0, 0),
    (146, 146, 64, 1, 2, 0, -1),                                # forward only: the backward is refused
]
REFUSED_BWD = [(129, 129, 64), (97, 97, 128)]                   # forward on the VALU kernel, backward refused on the host
KINDS = ("randn", "sharp", "mask")
DROP_P = 0.1
CAP = {"out": 2e-5, "probs": 2e-5, "dqkv": 5e-5}              # test_gpu_ops.py::test_attention's tolerances: nothing here is looser
FACTOR = 4.0                                                    # kernel bound = FACTOR x the largest fp32-ATen error


KERNELS = {(0, 0): "attn_fwd_kernel", (0, 1): "attn_fwd_mfma_kernel<256>", (0, 2): "attn_fwd_mfma_kernel<512>",
           (1, 0): "attn_bwd_kernel", (1, 1): "attn_bwd_mfma_kernel<256>", (1, 2): "attn_bwd_mfma_kernel<512>"}


def coverage_gaps(codes):
    """codes: {(Sq, Skv, d): (fwd, bwd)} -> what the coverage condition still misses: every kernel by a ragged square (sizes not
    multiples of 16), by Sq < Skv and by Sq > Skv (both sides above 1), the VALU kernels also by a head dim that is no multiple
    of 16"""
    need = {(k, o) for k in KERNELS for o in ("square", "Sq<Skv", "Sq>Skv")} | {((0, 0), "d%16"), ((1, 0), "d%16")}
    for (Sq, Skv, d), fb in codes.items():
        for bwd, code in enumerate(fb):
            if code < 0:
                continue
            if Sq == Skv and Sq % 16:
                need.discard(((bwd, code), "square"))
            if 1 < Sq < Skv:
                need.discard(((bwd, code), "Sq<Skv"))
            if Sq > Skv > 1:
                need.discard(((bwd, code), "Sq>Skv"))
            if d % 16:
                need.discard(((bwd, code), "d%16"))
    return sorted((KERNELS[k], o) for k, o in need)


def case_id(c):
    return "x".join(str(v) for v in c[:3])


def windows(Sq, Skv):
    """(q_off, kv_off, T) twice: overlapping token ranges, then disjoint ones with the keys first; q_off != kv_off, both > 0"""
    return [(2, 5, max(2 + Sq, 5 + Skv) + 3), (1 + Skv + 2, 1, 1 + Skv + 2 + Sq + 3)]


def make_inputs(case, kind, wi):
    """-> qkv [B, T, 3, H, d], dout [B, T, H d], keep-mask [B, H, Sq, Skv] uint8 or None, drop_p.  Everything a kernel must not
    read holds NaN: tokens outside both windows, the K / V slots of tokens only queried, the Q slot of tokens only attended to,
    and the rows of dout outside the query window."""
    Sq, Skv, d, B, H = case[:5]
    q_off, kv_off, T = windows(Sq, Skv)[wi]
    g = torch.Generator().manual_seed(1000003 * Sq + 1009 * Skv + 17 * d + 3 * KINDS.index(kind) + wi)
    amp = (50.0 / 3.5) ** 0.5 if kind == "sharp" else 1.0      # scale q k^T ~ N(0, amp^4): logits reach about +-50
    qkv = torch.full((B, T, 3, H, d), float("nan"), dtype=torch.float64)
    qkv[:, q_off:q_off + Sq, 0] = torch.randn(B, Sq, H, d, generator=g, dtype=torch.float64) * amp
    qkv[:, kv_off:kv_off + Skv, 1] = torch.randn(B, Skv, H, d, generator=g, dtype=torch.float64) * amp
    qkv[:, kv_off:kv_off + Skv, 2] = torch.randn(B, Skv, H, d, generator=g, dtype=torch.float64)
    dout = torch.full((B, T, H * d), float("nan"), dtype=torch.float64)
    dout[:, q_off:q_off + Sq] = torch.randn(B, Sq, H * d, generator=g, dtype=torch.float64)
    mask = None
    if kind == "mask":
        mask = (torch.rand(B, H, Sq, Skv, generator=g) >= DROP_P).to(torch.uint8)
        mask[0, 0, 0, :] = 0           # a query row with every key dropped
        mask[-1, -1, -1, :] = 1        # and one with none dropped
    # the inputs ARE fp32 numbers: round once, so that the float64 reference and the kernels see the same values
    return qkv.float(), dout.float(), mask, (DROP_P if mask is not None else 0.0)


def attn_eval(qkv, dout, mask, drop_p, q_off, Sq, kv_off, Skv, dtype):
    """the definition above in `dtype` -> out [B, Sq, H d], probs [B, H, Sq, Skv], dqkv [B, T, 3, H, d] (zero outside the windows)"""
    B, T, _, H, d = qkv.shape
    x = qkv.to(dtype)
    q = x[:, q_off:q_off + Sq, 0].permute(0, 2, 1, 3)          # [B, H, Sq, d]
    k = x[:, kv_off:kv_off + Skv, 1].permute(0, 2, 1, 3)
    v = x[:, kv_off:kv_off + Skv, 2].permute(0, 2, 1, 3)
    do = dout[:, q_off:q_off + Sq].to(dtype).reshape(B, Sq, H, d).permute(0, 2, 1, 3)
    scale = torch.tensor(d ** -0.5, dtype=torch.float32).to(dtype)      # the fp32 number the entry point receives
    keep = 1.0 if mask is None else mask.to(dtype) * (torch.tensor(1.0, dtype=torch.float32) / (1.0 - torch.tensor(drop_p, dtype=torch.float32))).to(dtype)
    P = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    Pd = P * keep
    O = Pd @ v
    dV = Pd.transpose(-1, -2) @ do
    dP = (do @ v.transpose(-1, -2)) * keep
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    dQ = (dS @ k) * scale
    dK = (dS.transpose(-1, -2) @ q) * scale
    dqkv = torch.zeros(B, T, 3, H, d, dtype=dtype)
    dqkv[:, q_off:q_off + Sq, 0] = dQ.permute(0, 2, 1, 3)
    dqkv[:, kv_off:kv_off + Skv, 1] = dK.permute(0, 2, 1, 3)
    dqkv[:, kv_off:kv_off + Skv, 2] = dV.permute(0, 2, 1, 3)
    return {"out": O.permute(0, 2, 1, 3).reshape(B, Sq, H * d), "probs": P, "dqkv": dqkv}


def nerr(a, b):
    """max |a - b| / (1 + |b| + max|b|): the normalisation of test_gpu_ops.close()"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b).abs() / (1.0 + b.abs() + b.abs().max())).max())


def combos():
    for case in CASES:
        for wi in range(2):
            for kind in KINDS:
                yield case, wi, kind


_ATEN = {}


def aten_errors():
    """{kind of input: {kind of output: the largest error of the fp32 ATen evaluation against float64 over every case and window}}"""
    if not _ATEN:
        worst = {kind: {"out": 0.0, "probs": 0.0, "dqkv": 0.0} for kind in KINDS}
        for case, wi, kind in combos():
            Sq, Skv = case[:2]
            q_off, kv_off, _ = windows(Sq, Skv)[wi]
            qkv, dout, mask, p = make_inputs(case, kind, wi)
            r64 = attn_eval(qkv, dout, mask, p, q_off, Sq, kv_off, Skv, torch.float64)
            r32 = attn_eval(qkv, dout, mask, p, q_off, Sq, kv_off, Skv, torch.float32)
            for key in worst[kind]:
                worst[kind][key] = max(worst[kind][key], nerr(r32[key], r64[key]))
        _ATEN.update(worst)
    return {kind: dict(v) for kind, v in _ATEN.items()}


def bounds():
    """the kernels' bound per input kind and output kind: FACTOR x the fp32-ATen error on the inputs of that kind, capped at
    test_attention's tolerance.  The sharp inputs carry ATen's largest error (the fp32 rounding of a logit near 50 / scale moves a
    probability by a few 1e-6 whoever computes it); bounding the other kinds by their own yardstick keeps them 15 x tighter than
    one bound over all inputs would."""
    return {kind: {key: min(CAP[key], FACTOR * e) for key, e in v.items()} for kind, v in aten_errors().items()}
