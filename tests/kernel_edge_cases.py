"""Cases, seeded inputs and references shared by tests/test_gpu_kernel_edges.py and tests/test_kernel_edge_inputs_cpu.py (no
test lives here; nothing here needs a GPU).  The kernels are the ones every STiL step runs and the suite used to check at one
shape each; the shapes below are their branch points (a 64-lane stride, a 256-thread loop, a grid cap, the scalar
instantiation, a border window).

References are the operation written from its definition with torch ops in a chosen dtype -- float64 is the reference, float32
(ATen on the CPU) the yardstick: the CPU test asserts that fp32 ATen meets, against float64, the very bound the GPU test applies
to the kernel -- or an exact integer model (the dropout hash, the pooling taps, argmax).  Scalars a kernel receives as `float`
are rounded to fp32 before the float64 reference uses them, so the reference states the kernel's problem and not a nearby one.

Bounds that are not the suite's `TOL`:
  ADAM_BOUND   4 x the largest scaled error of torch.optim.Adam (fp32, CPU) against `adam_reference` (float64) after the five
               steps of every ADAM_CONFIGS entry, measured on `adam_case`'s inputs (exceptions).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

NAN = float("nan")
SENT = -777.0
MIN_GAP = 1e-4              # discrete outputs: top-1 vs top-2 probability, and |max - threshold|, on every non-tie row


def gen(*key):
    g = torch.Generator()
    g.manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) % (2 ** 31))
    return g


def f32(x):
    """the double a kernel sees for a scalar passed as `float`"""
    return float(np.float32(x))


# =====================================================================================================================
# A. stil_onehot_argmax: exact
# =====================================================================================================================
ONEHOT_ROWS = (1, 37)
ONEHOT_KS = (1, 2, 63, 64, 65, 130, 286, 1000)
ONEHOT_TH = 0.6
TIE_K = 130
TIE_PLACEMENTS = ((5, 70), (5, 69))         # different lanes of the 64-lane wave / the same lane on two trips


def onehot_case(rows, K):
    """-> (p [rows, K] fp32, threshold, idx, mask).  Every row has one planted maximum (at a column that walks through all
    lanes and trips, the last column included), above the threshold on even rows and below it on odd ones; the background
    stays below 0.5."""
    g = gen(rows, K, 11)
    p = 0.5 * torch.rand(rows, K, generator=g)
    col = torch.tensor([(K - 1 + 29 * r) % K for r in range(rows)])
    val = torch.where(torch.arange(rows) % 2 == 0, 0.7 + 0.25 * torch.rand(rows, generator=g), torch.full((rows,), 0.55))
    p[torch.arange(rows), col] = val
    return p, ONEHOT_TH, col.to(torch.int32), (val >= f32(ONEHOT_TH)).float()


def onehot_tie_case():
    """K = 130 rows with two exactly equal maxima (TIE_PLACEMENTS, and both at once), above and below the threshold, and rows
    whose maximum IS the fp32 threshold (mask 1): alone, and tied across lanes.  The first index wins everywhere."""
    K, th = TIE_K, np.float32(ONEHOT_TH)
    g = gen(K, 13)
    rows, idx, mask = [], [], []
    for cols, v in [((5, 70), 0.9), ((5, 69), 0.9), ((5, 69, 70), 0.8), ((69, 70), 0.55), ((5, 70), 0.55), ((70, 129), 0.9), ((17,), float(th)),
                    ((5, 70), float(th)), ((64, 128), 0.75), ((63, 64), 0.75), ((0, 129), 0.75)]:
        r = 0.5 * torch.rand(K, generator=g)
        r[list(cols)] = v
        rows.append(r); idx.append(min(cols)); mask.append(1.0 if np.float32(v) >= th else 0.0)
    return torch.stack(rows), float(th), torch.tensor(idx, dtype=torch.int32), torch.tensor(mask)


# =====================================================================================================================
# A. stil_cgpl_pgls
# =====================================================================================================================
CGPL_TABLE = ((1, 2, 16), (37, 2, 16), (37, 64, 128), (37, 65, 128), (40, 286, 128), (40, 300, 128), (16, 1000, 100))
CGPL_R, CGPL_T = 0.9, 0.1
CGPL_LD_PAD_K = 286             # zm / zi / zt are `ldz = K + 3` views with NaN padding at this K
CGPL_PRED_IN_K = 300            # pred_in (the distribution-aligned prediction) is given at this K
CGPL_MARGINS = (6.0, 2.0)       # added to the planted top-1 column: confident rows / unconfident rows


@functools.lru_cache(maxsize=None)
def cgpl_case(Bu, K, Dp):
    """-> dict of fp32 inputs and the planted discrete truth.  Row u (a regular row) gets case u % 4 + 1 by planting each head's
    top-1: a margin on a chosen column over 0.05 * randn noise.  Where K > 70 the last six rows are tie rows: all heads peak at
    column 5, and head h carries an exactly equal logit at column 70 (another lane) or 69 (the same lane, next trip) -- equal
    logits give bit-equal fp32 probabilities, the first index wins, the row is case 1.  The threshold is an input: it sits in
    the middle of the gap the float64 prediction leaves between the confident and the unconfident rows."""
    g = gen(Bu, K, Dp, 17)
    n_tie = 6 if K > 70 else 0
    n_reg = Bu - n_tie
    z = [0.05 * torch.randn(Bu, K, generator=g) for _ in range(3)]
    top = torch.zeros(3, Bu, dtype=torch.int64)
    case = torch.zeros(Bu, dtype=torch.int64)
    margin = torch.zeros(Bu)
    for u in range(n_reg):
        a = (7 * u + 3) % K
        o1 = (a + 1 + (13 * u) % (K - 1)) % K
        o2 = (a + 1 + (13 * u + 5) % (K - 1)) % K
        cs = u % 4 + 1
        b, d = {1: (a, a), 2: (a, o1), 3: (o1, a), 4: (o1, o2 if u % 8 < 4 else o1)}[cs]
        case[u], margin[u] = cs, CGPL_MARGINS[(u // 4) % 2]
        for h, c in enumerate((a, b, d)):
            top[h, u] = c
            z[h][u, c] += margin[u]
    ties = []
    feat = F.normalize(torch.randn(Bu, Dp, generator=g))
    protos = F.normalize(torch.randn(K, Dp, generator=g))
    for j in range(n_tie):
        u, h, (c0, c1) = n_reg + j, j % 3, TIE_PLACEMENTS[j // 3]
        case[u], margin[u] = 1, CGPL_MARGINS[0]
        for hh in range(3):
            top[hh, u] = c0
            z[hh][u, c0] = CGPL_MARGINS[0] + 0.01 * hh
        z[h][u, c1] = z[h][u, c0]
        ties.append((u, h, c0, c1))
        feat[u] = F.normalize(protos[c0] + 0.05 * torch.randn(Dp, generator=g), dim=0)   # the prototype term breaks the tie in `prediction`
    mr = (torch.rand(Bu, generator=g) >= 0.5).to(torch.uint8)
    pred_in = None
    if K == CGPL_PRED_IN_K:
        qm = 0.75 + 0.5 * torch.rand(K, generator=g)
        pi = z[0].softmax(1) / qm
        pred_in = pi / pi.sum(1, keepdim=True)
    c = dict(Bu=Bu, K=K, Dp=Dp, zm=z[0], zi=z[1], zt=z[2], feat=feat, protos=protos, mr=mr, pred_in=pred_in, top=top, case=case, margin=margin,
             ties=ties, ld=K + 3 if K == CGPL_LD_PAD_K else K)
    mx = cgpl_reference(c, torch.float64, True)["pred_full"].max(1)[0]
    hi, lo = mx[margin == CGPL_MARGINS[0]], mx[margin == CGPL_MARGINS[1]]
    c["th"] = f32((float(lo.max()) + float(hi.min())) / 2.0) if len(lo) and float(lo.max()) < float(hi.min()) else 0.45
    return c


def cgpl_reference(c, dtype, use_pseudo):
    """STiLModel.py:262-299 from the planted cases, in `dtype`: q0 = softmax(mean of the agreeing heads' logits), tp = softmax(feat
    . protos^T / T), pseudo_label = r q0 + (1 - r) tp, prediction = r pm + (1 - r) tp with pm = softmax(zm) or pred_in."""
    r, T = f32(CGPL_R), f32(CGPL_T)
    zm, zi, zt = c["zm"].to(dtype), c["zi"].to(dtype), c["zt"].to(dtype)
    cs = c["case"][:, None]
    v = torch.where(cs == 1, (zm + zi + zt) / 3.0, torch.where(cs == 2, (zm + zi) / 2.0, torch.where(cs == 3, (zm + zt) / 2.0, zm)))
    q0 = v.softmax(1)
    tp = (c["feat"].to(dtype) @ c["protos"].to(dtype).t() / T).softmax(1)
    pm = zm.softmax(1) if c["pred_in"] is None else c["pred_in"].to(dtype)
    pred = r * pm + (1.0 - r) * tp
    return {"pseudo_label": r * q0 + (1.0 - r) * tp, "pseudo_orig": q0, "prediction": pred if use_pseudo else torch.zeros_like(pred), "pred_full": pred}


def cgpl_discrete(c, use_pseudo):
    """flags [Bu, 4], hard [Bu], w3 [3, Bu] from the planted cases and the float64 prediction (unambiguous: the CPU test asserts the gaps)"""
    pred = cgpl_reference(c, torch.float64, True)["pred_full"]
    cs, mr = c["case"], c["mr"].bool()
    mask1 = pred.max(1)[0] >= c["th"]
    flags = torch.zeros(c["Bu"], 4, dtype=torch.uint8)
    flags[:, 0], flags[:, 1] = cs.to(torch.uint8), mask1.to(torch.uint8)
    flags[:, 2] = (mask1 if use_pseudo else torch.zeros_like(mask1)).to(torch.uint8)
    hard = (pred.argmax(1) if use_pseudo else torch.zeros(c["Bu"], dtype=torch.int64)).to(torch.int32)
    w3 = torch.stack([mask1 & (cs == 1), mask1 & ((cs == 1) | (cs == 3) | ((cs == 4) & mr)), mask1 & ((cs == 1) | (cs == 2) | ((cs == 4) & ~mr))]).float()
    return flags, hard, w3


# =====================================================================================================================
# A. stil_proto_accum
# =====================================================================================================================
PROTO_ACCUM_TABLE = ((46, 6, 11, 128), (40, 0, 2, 16), (8, 8, 5, 100), (300, 44, 286, 128), (64, 16, 7, 256))
PROTO_ACCUM_THREADS = 192       # the launch's block width: the last table entry has Dp + 1 > 192
REPEAT_RATIOS = (1.0, 2.0, 3.0)


def proto_accum_case(B, B_l, K, Dp):
    """-> feat [B, Dp], hard [B] int32 (class K - 1 never occurs; every 7th row lies outside [0, K)), conf [B] uint8 (a third zero)"""
    g = gen(B, B_l, K, Dp)
    feat = F.normalize(torch.randn(B, Dp, generator=g))
    hard = torch.randint(0, max(K - 1, 1), (B,), generator=g).to(torch.int32)
    for j, r in enumerate(range(3, B, 7)):
        hard[r] = (-1, K, K + 5, -(2 ** 31), 2 ** 31 - 1)[j % 5]
    conf = (torch.rand(B, generator=g) >= 0.33).to(torch.uint8)
    return feat, hard, conf


def proto_accum_reference(feat, hard, conf, B_l, K, repeat_ratio, dtype):
    """utils cal_prototypes on the labelled and the unlabelled part, then labelled / repeat_ratio + unlabelled: [K, Dp + 1]"""
    f = torch.cat([feat.to(dtype), torch.ones(len(feat), 1, dtype=dtype)], 1)
    out = torch.zeros(K, f.shape[1], dtype=dtype)
    inv = float(np.float32(1.0) / np.float32(repeat_ratio))         # the kernel's fp32 1 / repeat_ratio
    for part, w in ((slice(0, B_l), inv), (slice(B_l, None), 1.0)):
        sel = conf[part].bool() & (hard[part] >= 0) & (hard[part] < K)
        s = torch.zeros_like(out)
        s.index_add_(0, hard[part][sel].long(), f[part][sel])
        out = out + s * w
    return out


# =====================================================================================================================
# A. stil_clip_fwd / bwd on a logit matrix, stil_club_fwd / bwd
# =====================================================================================================================
CLIP_BS = (1, 2, 63, 64, 65, 257, 300)
CLIP_LAMS = ((0.3, 0.7), (0.5, 0.5), (1.0, 0.0))
CLIP_SCALE = 14.0               # cosines / T at T = 0.07 reach +-14.3: the largest |logit| of every case is 14
CLIP_G = 1.7                    # the upstream gradient


def clip_case(B):
    g = gen(B, 23)
    n0, n1 = F.normalize(torch.randn(B, 8, generator=g)), F.normalize(torch.randn(B, 8, generator=g))
    c = n0 @ n1.t()
    return (CLIP_SCALE * c / c.abs().max()).contiguous()


def clip_reference(Z, lam0, lam1, dtype):
    """utils/clip_loss.py:35-38 -> (loss, dZ for the upstream gradient CLIP_G)"""
    z = Z.to(dtype).requires_grad_()
    lab = torch.arange(len(z))
    loss = f32(lam0) * F.cross_entropy(z, lab) + f32(lam1) * F.cross_entropy(z.t(), lab)
    (dz,) = torch.autograd.grad(loss, z, torch.tensor(f32(CLIP_G), dtype=dtype))
    return loss.detach(), dz


CLUB_TABLE = ((1, 64), (2, 5), (3, 63), (5, 64), (7, 65), (130, 200), (257, 64))
CLUB_G = (1.5, -0.75)           # upstream gradients of (club, est)


def club_case(R, D):
    g = gen(R, D, 29)
    return torch.randn(R, D, generator=g), 0.5 + torch.randn(R, D, generator=g)


def club_reference(mu, y, dtype):
    """club.py:107-130 in its materialised [R, R, D] form -> (club, est, dmu, dy) for the upstream gradients CLUB_G"""
    mu, y = mu.to(dtype).requires_grad_(), y.to(dtype).requires_grad_()
    pos = (-(mu - y) ** 2 / 2.0).sum(-1)
    neg = (-((y.unsqueeze(0) - mu.unsqueeze(1)) ** 2).mean(dim=1) / 2.0).sum(-1)
    club, est = (pos - neg).mean(), ((mu - y) ** 2).sum(1).mean(0)
    dmu, dy = torch.autograd.grad(CLUB_G[0] * club + CLUB_G[1] * est, (mu, y))
    return club.detach(), est.detach(), dmu, dy


# =====================================================================================================================
# B. stil_adam_step
# =====================================================================================================================
ADAM_GRID_CAP = 16384           # blocks of adam_kernel: a slab of more chunks takes the loop's second trip
ADAM_CHUNK = 1024
ADAM_LR = 1e-3
ADAM_STEPS = 5
# (weight_decay, grad_scale, (beta1, beta2), eps): a reduced cross in which every value of the four axes occurs
ADAM_CONFIGS = ((0.0, 1.0, (0.9, 0.999), 1e-8), (0.01, 0.5, (0.9, 0.999), 1e-8), (0.01, 0.125, (0.5, 0.9), 1e-3), (0.0, 0.5, (0.5, 0.9), 1e-3),
                (0.01, 1.0, (0.9, 0.999), 1e-3), (0.0, 0.125, (0.9, 0.999), 1e-8))
# chunk -> tensor; tensor 1 sits out steps 2 and 4, tensor 4 never takes part (sentinel-filled, like the -1 padding chunks)
ADAM_C2T = (0, -1, 1, 2, 2, -1, 3, 4, -1)
ADAM_NUMEL = (1000, 700, 2048, 5, 1024)
ADAM_NEVER = 4
ADAM_BIG_LIVE = (0, ADAM_GRID_CAP - 1, ADAM_GRID_CAP, ADAM_GRID_CAP + 2)
ADAM_BIG_CHUNKS = ADAM_GRID_CAP + 3
# measured (tests/test_kernel_edge_inputs_cpu.py re-measures and fails if this drifts): largest scaled error
# |a - b| / (1 + |b| + max|b|) of torch.optim.Adam fp32 against adam_reference after ADAM_STEPS steps over ADAM_CONFIGS
ADAM_ATEN_ERR = {"p": 7.04e-8, "m": 6.46e-8, "v": 2.93e-7}
ADAM_BOUND = {k: 4.0 * e for k, e in ADAM_ATEN_ERR.items()}


def adam_active(step):
    """[n_tensors] uint8 for the 1-based step"""
    a = torch.ones(len(ADAM_NUMEL), dtype=torch.uint8)
    a[ADAM_NEVER] = 0
    if step in (2, 4):
        a[1] = 0
    return a


def adam_layout(c2t=ADAM_C2T, numel=ADAM_NUMEL):
    """-> [(tensor, first float, numel)] of the slab (tensors padded to whole chunks)"""
    out, seen = [], set()
    for ch, t in enumerate(c2t):
        if t >= 0 and t not in seen:
            seen.add(t)
            out.append((t, ch * ADAM_CHUNK, numel[t]))
    return out


def adam_case(cfg_index):
    """-> (P0 [n], [G_1 .. G_5] slabs).  Live tensors hold randn parameters (tensor 2's gradients are 1e-3 small, where eps = 1e-3
    matters); the tail of a tensor's last chunk is zero as in flat.py; padding chunks and the never-active tensor hold SENT in
    the parameters and NaN in the gradients."""
    g = gen(cfg_index, 31)
    n = len(ADAM_C2T) * ADAM_CHUNK
    P = torch.full((n,), SENT)
    Gs = [torch.full((n,), NAN) for _ in range(ADAM_STEPS)]
    for t, off, ne in adam_layout():
        if t == ADAM_NEVER:
            continue
        chunks = ADAM_C2T.count(t) * ADAM_CHUNK
        P[off:off + chunks] = 0.0
        P[off:off + ne] = torch.randn(ne, generator=g)
        for G in Gs:
            G[off:off + chunks] = 0.0
            G[off:off + ne] = torch.randn(ne, generator=g) * (1e-3 if t == 2 else 1.0)
    return P, Gs


def adam_reference(P, M, V, G, steps, active, c2t, cfg, lr=ADAM_LR):
    """One torch.optim.Adam step (weight decay folded into the gradient, per-tensor step counts, inactive tensors skipped)
    restated in float64 on whole chunks, in place on the float64 slabs P, M, V; `steps` is a list of ints."""
    wd, gs, (b1, b2), eps = cfg
    wd, gs, b1, b2, eps, lr = f32(wd), f32(gs), f32(b1), f32(b2), f32(eps), f32(lr)
    for t in range(len(steps)):
        if active[t]:
            steps[t] += 1
    for ch, t in enumerate(c2t):
        if t < 0 or not active[t]:
            continue
        s = slice(ch * ADAM_CHUNK, (ch + 1) * ADAM_CHUNK)
        g = G[s].double() * gs
        if wd != 0.0:
            g = g + wd * P[s]
        M[s] = b1 * M[s] + (1.0 - b1) * g
        V[s] = b2 * V[s] + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** steps[t], 1.0 - b2 ** steps[t]
        P[s] = P[s] - (lr / bc1) * (M[s] / (V[s].sqrt() / np.sqrt(bc2) + eps))


def adam_run_reference(cfg_index):
    """-> float64 (P, M, V), step counts after ADAM_STEPS steps, and the slabs after each step (for the bit-for-bit checks)"""
    P0, Gs = adam_case(cfg_index)
    P, M, V = P0.double(), torch.zeros_like(P0).double(), torch.zeros_like(P0).double()
    live = adam_live_mask()
    M[~live], V[~live] = SENT, SENT
    steps = [0] * len(ADAM_NUMEL)
    for i, G in enumerate(Gs):
        adam_reference(P, M, V, G, steps, adam_active(i + 1), ADAM_C2T, ADAM_CONFIGS[cfg_index])
    return P, M, V, steps


def adam_live_mask(c2t=ADAM_C2T, never=(ADAM_NEVER,)):
    m = torch.tensor([t >= 0 and t not in never for t in c2t]).repeat_interleave(ADAM_CHUNK)
    return m


def adam_run_aten(cfg_index):
    """torch.optim.Adam in fp32 on the CPU over the same tensors: grad * grad_scale, grad None on the steps a tensor sits out"""
    wd, gs, betas, eps = ADAM_CONFIGS[cfg_index]
    P0, Gs = adam_case(cfg_index)
    lay = [(t, off, ADAM_C2T.count(t) * ADAM_CHUNK) for t, off, _ in adam_layout() if t != ADAM_NEVER]
    params = {t: P0[off:off + n].clone().requires_grad_() for t, off, n in lay}
    opt = torch.optim.Adam(list(params.values()), lr=ADAM_LR, betas=betas, eps=eps, weight_decay=wd)
    for i, G in enumerate(Gs):
        act = adam_active(i + 1)
        for t, off, n in lay:
            params[t].grad = (G[off:off + n] * gs).clone() if act[t] else None
        opt.step()
    P, M, V = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0)
    for t, off, n in lay:
        P[off:off + n] = params[t].detach()
        M[off:off + n], V[off:off + n] = opt.state[params[t]]["exp_avg"], opt.state[params[t]]["exp_avg_sq"]
    return P, M, V


def scaled_err(a, b):
    """the suite's close() as a number: max |a - b| / (1 + |b| + max|b|)"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b).abs() / (1.0 + b.abs() + b.abs().max())).max())


# =====================================================================================================================
# B. stil_ema_update, stil_rng_mask
# =====================================================================================================================
EMA_GRID_CAP = 8192             # blocks of 256 quads
EMA_NS = (4, 1020, 1024, EMA_GRID_CAP * 256 * 4 + 4100)
EMA_MOMENTA = (0.0, 0.996, 0.999)


def ema_case(n):
    g = gen(n, 37)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


def ema_reference(e, v, m):
    """the reference's own statement, evaluated by ATen on the CPU (STiLModel.py:154-168)"""
    return e.clone().mul_(m).add_((1.0 - m) * v)


RNG_GRID_CAP = 16384            # blocks of 256 threads
RNG_NS = (1, 255, 257, RNG_GRID_CAP * 256 + 1000)
RNG_PS = (0.0, 0.1, 0.5, 0.8, 0.999)
# (seed, offset, step counter or None)
RNG_STREAMS = ((0, 0, None), (2 ** 32 + 7, 2 ** 40, 0), (7, 2 ** 40, 1), (2 ** 33 + 1, 3, 5), (2022, 12345, None))
_M64 = (1 << 64) - 1


def hash_u32(x):
    """csrc/transformer.hip hash_u32 on a numpy uint64 array (arithmetic modulo 2^64)"""
    x = x.copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return (x >> np.uint64(16)) & np.uint64(0xffffffff)


@functools.lru_cache(maxsize=8)
def rng_uniform(n, seed, offset, step):
    """the kernel's u in [0, 1) for elements 0 .. n - 1: a multiple of 2^-24, exact in fp32"""
    st = 0 if step is None else (step * 0xD1B54A32D192ED03) & _M64
    base = (seed * 0x9E3779B97F4A7C15 + st + offset) & _M64
    with np.errstate(over="ignore"):
        r = hash_u32(np.uint64(base) + np.arange(n, dtype=np.uint64))
    return (r >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def rng_mask_model(n, seed, offset, p, step=None):
    return (rng_uniform(n, seed, offset, step) >= np.float32(p)).astype(np.uint8)


# =====================================================================================================================
# C. max-pool, im2col, transpose, LayerNorm
# =====================================================================================================================
POOL_TABLE = ((1, 1, 1, 4), (2, 2, 3, 4), (2, 7, 9, 8), (1, 8, 6, 64), (3, 5, 5, 12))
POOL_KINDS = ("ties", "nan", "neginf")


def pool_case(N, H, W, C, kind):
    """-> (x NCHW, gy NCHW), both integer valued (dx is then exact).  x takes seven values, so maxima tie inside windows and
    between overlapping ones; "nan": one NaN element per image in channel 1; "neginf": channels 0 and 2 hold -inf on their
    top-left 4 x 4 corner -- the border windows there (and, from H, W >= 4 on, the interior window (1, 1)) see nothing else."""
    g = gen(N, H, W, C, POOL_KINDS.index(kind))
    x = torch.randint(-3, 4, (N, C, H, W), generator=g).float()
    if kind == "nan":
        x[:, 1, min(1, H - 1), min(2, W - 1)] = NAN
    if kind == "neginf":
        x[:, 0, :4, :4] = float("-inf")
        x[:, 2, :4, :4] = float("-inf")
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randint(1, 9, (N, C, OH, OW), generator=g).float()
    return x, gy


def pool_reference(x, gy):
    xr = x.clone().requires_grad_()
    y = F.max_pool2d(xr, 3, 2, 1)
    y.backward(gy)
    return y.detach(), xr.grad


IM2COL_TABLE = ((1, 3, 7, 7, 7, 2, 3, 148), (2, 3, 13, 9, 7, 2, 3, 160), (2, 1, 5, 6, 3, 1, 1, 12), (3, 4, 8, 8, 1, 1, 0, 4))
IM2COL_ROWS_PER_BLOCK = 32
TRANSPOSE_TABLE = ((1, 1), (1, 33), (31, 33), (32, 32), (33, 65), (100, 286), (640, 128))


def im2col_reference(x, k, stride, pad):
    """[N * OH * OW, Cin * k * k] with column c * k * k + ky * k + kx: F.unfold, rows in (n, oy, ox) order"""
    u = F.unfold(x, k, padding=pad, stride=stride)
    return u.permute(0, 2, 1).reshape(-1, u.shape[1]).contiguous()


LN_VECTOR = ((1, 4), (3, 8), (5, 252), (4, 256), (6, 260), (9, 2080), (2, 4096), (33000, 8))
LN_SCALAR = ((5, 1), (7, 3), (6, 63), (4, 65), (9, 257), (3, 2081))
LN_ALIGN = (130, 96)            # run twice on the same data: aligned (vector kernel) and one float into its buffer (scalar kernel)
LN_EPS = 1e-5
LN_MAX_D = 4096
LN_BLOCK_CAP, LN_ROWS_PER_BLOCK = 1024, 32      # rows > 32768: a block of the backward owns more than 32 rows


def ln_case(rows, D):
    """-> x, gamma, beta, gy, and the dgamma / dbeta already in the accumulators for the accumulate = 1 call"""
    g = gen(rows, D, 41)
    x, gamma, beta, gy = torch.randn(rows, D, generator=g), 0.5 + torch.rand(D, generator=g), torch.randn(D, generator=g), torch.randn(rows, D, generator=g)
    if D == 1:
        # the variance is 0 whatever x holds and dx = rstd * (g gamma - mean(g gamma)) is 316 x a difference of equal numbers: with
        # dyadic x, g and gamma every product and sum on the way is exact in fp32 in any order, so the answer 0 is reachable
        x, gamma, gy = (x * 8).round() / 8, torch.full((1,), 0.5), (gy * 8).round() / 8
    return x, gamma, beta, gy, torch.randn(D, generator=g), torch.randn(D, generator=g)


def ln_reference(x, gamma, beta, gy, dtype):
    x, gamma, beta = x.to(dtype).requires_grad_(), gamma.to(dtype).requires_grad_(), beta.to(dtype).requires_grad_()
    y = F.layer_norm(x, x.shape[1:], gamma, beta, eps=f32(LN_EPS) if dtype == torch.float64 else LN_EPS)
    dx, dg, db = torch.autograd.grad(y, (x, gamma, beta), gy.to(dtype))
    mean = x.detach().mean(1)
    rstd = 1.0 / torch.sqrt(x.detach().var(1, unbiased=False) + f32(LN_EPS))
    return {"y": y.detach(), "mean_rstd": torch.stack([mean, rstd], 1), "dx": dx, "dgamma": dg, "dbeta": db}
