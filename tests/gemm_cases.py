"""Cases, inputs and float64 definitions shared by tests/test_gpu_gemm.py and tests/test_gemm_cases_cpu.py (no test lives here,
nothing GPU-side is imported).

One NT case names a launch of `stil_gemm_nt` completely -- shape, gather geometry and output map, every leading dimension, a per-
operand element offset (0: 16-byte aligned, 1: not), `tune`, the forced split, the epilogue operands -- and the CONFIG code
`stil_gemm_nt_config` must report for it; one weight-gradient case does the same for `stil_wgrad_tn` / `stil_wgrad_config`.  The
codes are what the GPU module's coverage rests on; the CPU module compares them with the built library, so a retune that moves
a case to another kernel fails without a GPU.

Definitions (plain torch, evaluated in float64 = the reference, and in float32 = ATen on the CPU, the yardstick):
  Agather[m, (ky KW + kx) C + c] = src[n, iy, ix, c], m = (n, oy, ox);  mode 0: iy = oy stride - pad_y + ky;  mode 1: iy = (oy +
      pad_y - ky) / stride where divisible;  zero outside the source;  with a_bn / x_bn the source is relu((y - mean) a + beta) formed
      from rows 0, 2, 3 of the statistics block BEFORE the gather (padding taps stay zero);
  P = Agather W^T;  v = ((alpha P - sub) scale / sqrt(scale_var + var_eps) + shift + bias) + resid;  pre = v;  v = act(v);
      v = 0 where relu_mask <= 0;  C[rowmap(m)] = v;
  colstats[2t], [2t + 1] = mean, sum of squared deviations of alpha P over the rows of tile t;
  bstats[2(t0 + t)], [.. + 1] = sum g', sum g' xhat over the rows of 64-row tile t, g' = v (bs_relu 0) or v [(y - mean) a + beta > 0];
  dW[n, k] = sum_m dY[m, n] Xgather[m, k], stored (N, C, KH, KW) for KH KW > 1, else its first Kdst columns."""
import zlib
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

TOL = 2e-5          # tests/test_gpu_ops.py's tolerance: no bound here is looser
FACTOR = 4.0        # kernel bound = FACTOR x the family's fp32-ATen error (the rule of tests/test_gpu_attention.py)
MARGIN = 64         # floats of NaN (inputs) / sentinel (outputs) before and after every buffer
SENT = -777.0
NAN = float("nan")
FAMILIES = ("plain", "gather", "split", "stats", "backward", "wgrad")


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------------------
# geometries: source H x W, GEMM rows over OH x OW, taps KH x KW; (os, opy, opx, oOH, oOW) = the output row map
def _g(H, W, OH, OW, KH, KW, stride, pad_y, pad_x, mode=0, os=1, opy=0, opx=0, oOH=None, oOW=None):
    return NS(H=H, W=W, OH=OH, OW=OW, KH=KH, KW=KW, stride=stride, pad_y=pad_y, pad_x=pad_x, mode=mode, os=os, opy=opy, opx=opx,
              oOH=OH if oOH is None else oOH, oOW=OW if oOW is None else oOW)


GEOMS = {
    "plain": _g(1, 1, 1, 1, 1, 1, 1, 0, 0),
    "3x3s1": _g(5, 5, 5, 5, 3, 3, 1, 1, 1),
    "3x3s2": _g(7, 5, 4, 3, 3, 3, 2, 1, 1),                       # H != W
    "1x1s2": _g(7, 5, 4, 3, 1, 1, 2, 0, 0),
    "m1s1": _g(5, 4, 5, 4, 3, 3, 1, 1, 1, mode=1),                # mode 1 at stride 1
    "dgrad2": _g(4, 3, 7, 5, 3, 3, 2, 1, 1, mode=1),              # the generic stride-2 input-gradient gather
    "phase00": _g(4, 3, 4, 3, 2, 2, 1, 0, 1, os=2, opy=0, opx=0, oOH=8, oOW=6),    # the strided output map, one launch per phase
    "phase01": _g(4, 3, 4, 3, 2, 2, 1, 0, 0, os=2, opy=0, opx=1, oOH=8, oOW=6),
    "phase10": _g(4, 3, 4, 3, 2, 2, 1, 1, 1, os=2, opy=1, opx=0, oOH=8, oOW=6),
    "phase11": _g(4, 3, 4, 3, 2, 2, 1, 1, 0, os=2, opy=1, opx=1, oOH=8, oOW=6),
    "padyx": _g(6, 6, 6, 4, 3, 3, 1, 1, 0),                       # pad_y != pad_x on the identity map
    "grid3x3": _g(3, 3, 3, 3, 3, 3, 1, 1, 1),                     # OH OW < 16: a 16-row step crosses images
    "grid1x5": _g(1, 5, 1, 5, 3, 3, 1, 1, 1),
    "1x1pad": _g(5, 5, 7, 5, 1, 1, 1, 1, 0),                      # a single tap WITH padding rows
}
GATHER_KINDS = [k for k in GEOMS if k not in ("plain", "1x1pad")]
WG_GEOMS = ["3x3s1", "3x3s2", "1x1s2", "grid3x3", "grid1x5"]      # stil_wgrad_tn: forward gathers with one pad


def is_plain(g):
    """the launcher's own rule (include/stil_hip.h, stil_gemm_nt_config's `plain`)"""
    return (g.KH * g.KW == 1 and g.stride == 1 and g.pad_y == 0 and g.pad_x == 0 and g.mode == 0 and g.os == 1
            and g.H == g.OH and g.W == g.OW)


# ------------------------------------------------------------------------------------------------------------------------------
# the reachable set, read off stil_gemm_nt (from `if (a_bn)` to the end of LAUNCH_NT, and the lean-kernel branch above it) and
# wgrad_tn_impl, as CONFIG codes (include/stil_hip.h)
def nt_code(variant, bkd=0, acc2=0, vec=1, plain=1, a_bn=0, b3=0):
    return variant + 100 * bkd + 1000 * acc2 + 10000 * vec + 100000 * plain + 1000000 * a_bn + 10000000 * b3


def nt_decode(code):
    return NS(variant=code % 100, bkd=code // 100 % 10, acc2=code // 1000 % 10, vec=code // 10000 % 10, plain=code // 100000 % 10,
              a_bn=code // 1000000 % 10, b3=code // 10000000 % 10)


def nt_kernel(code):
    """the template instantiation a CONFIG code launches.  Two codes may name one kernel: the 64x128 tile has no 32-deep variant and
    the 128-row tiles run 32-deep k-tiles in two LDS buffers whatever the code's bkd digit says (1 or 2)."""
    k = nt_decode(code)
    tf = lambda b: "true" if b else "false"
    if k.variant == 44:
        return f"gemm_nt_big_kernel<{tf(k.acc2)}, {tf(k.a_bn)}>"
    TM, TN = (2 if k.variant in (21, 22) else 1), (2 if k.variant in (12, 22) else 1)
    bk32 = k.bkd > 0 and k.variant != 12
    NB = 1 if (k.variant == 11 and k.bkd == 2) else 2
    return f"gemm_nt_kernel<{TM}, {TN}, {32 if bk32 else 16}, {tf(k.vec)}, {tf(k.acc2)}, {tf(k.plain)}, {tf(k.a_bn)}, {NB}, {tf(k.b3)}>"


_AP = [(a, p) for a in (0, 1) for p in (0, 1)]
NT_REACHABLE = (
    [nt_code(v, 0, a, 0, p) for v in (11, 12, 21, 22) for a, p in _AP]            # scalar loads x tiles x ACC2 x PLAIN        16
    + [nt_code(11, b, a, 1, p) for b in (0, 1, 2) for a, p in _AP]                # vector, 64x64: BK 16, BK 32 x 2, BK 32 x 1   12
    + [nt_code(12, 0, a, 1, p) for a, p in _AP]                                   # vector, 64x128: BK 16                        4
    + [nt_code(v, b, a, 1, p) for v in (21, 22) for b in (0, 1) for a, p in _AP]  # vector, 128-row tiles: BK 16, BK 32         16
    + [nt_code(11, 0, a, 1, p, a_bn=1) for a, p in _AP]                           # operand-staging BatchNorm                    4
    + [nt_code(11, 2, 1, 1, p, a_bn=ab, b3=1) for ab in (0, 1) for p in (0, 1)]   # split precision                              4
    + [nt_code(44, 2, a, 1, 1, a_bn=ab) for a in (0, 1) for ab in (0, 1)]         # the lean 128x128 kernel                      4
)
NT_KERNELS = sorted({nt_kernel(c) for c in NT_REACHABLE})


def wg_code(tile, vec=1, xbn=0, reduce4=1):
    return tile + 100 * vec + 1000 * xbn + 10000 * reduce4


def wg_kernel(code):
    TN, TK = {11: (1, 1), 12: (1, 2), 22: (2, 2)}[code % 100]
    vec, xbn = code // 100 % 10, code // 1000 % 10
    return f"gemm_tn_kernel<{TN}, {TK}, {'true' if vec else 'false'}{', true' if xbn else ''}>"


WG_REACHABLE = [wg_code(t, v, x, 1) for t in (11, 12, 22) for v, x in ((0, 0), (1, 0), (1, 1))]
WG_KERNELS = sorted({wg_kernel(c) for c in WG_REACHABLE})
WG_REDUCES = [("wgrad_reduce4_kernel", "taps==1"), ("wgrad_reduce4_kernel", "taps>1"), ("wgrad_reduce_kernel", "taps==1"),
              ("wgrad_reduce_kernel", "taps>1")]


# ------------------------------------------------------------------------------------------------------------------------------
# NT cases
EPI_ALL = ("alpha", "sub", "scale", "scale_var", "shift", "bias", "resid", "pre", "relu_mask")


def nt(name, N, C, code, geom="plain", M=None, nb=None, tune=0, family=None, lda=None, ldb=None, ldc=None, off=(), epi=(), act=0,
       force=None, splits=1, panel=0, bs_relu=0, bs_tile0=0, base=None):
    g = GEOMS[geom]
    nb = M if geom == "plain" else nb
    M = nb * g.OH * g.OW
    K = g.KH * g.KW * C
    epi = tuple(epi)
    ldc = N if ldc is None else ldc
    if family is None:
        family = ("split" if splits > 1 else "backward" if "bstats" in epi else "stats" if "colstats" in epi
                  else "plain" if geom == "plain" else "gather")
    return NS(name=name, M=M, N=N, K=K, C=C, nb=nb, geom=geom, g=g, tune=tune, code=code, family=family,
              lda=C if lda is None else lda, ldb=K if ldb is None else ldb, ldc=ldc,
              ldr=ldc + 4 if "resid" in epi else 0, ldm=ldc + 8 if "relu_mask" in epi else 0,     # ldr != ldc, ldm != ldc
              off=frozenset(off), epi=frozenset(epi), act=act, alpha=0.7 if "alpha" in epi else 1.0, var_eps=1e-5 if "scale_var" in epi else 0.0,
              force=force, splits=splits, panel=panel, bs_relu=bs_relu, bs_tile0=bs_tile0, base=base or name)


def nt_tile(c):
    """(rows, columns) of the block tile the case's kernel owns"""
    v = nt_decode(c.code).variant
    return (128 if v in (21, 22, 44) else 64), (128 if v in (12, 22, 44) else 64)


def nt_stat_rows(c):
    """granularity of colstats: stil_gemm_nt_tile_rows (64 for the 64-row tiles and the lean kernel)"""
    return 128 if nt_decode(c.code).variant in (21, 22) else 64


def _tune_for(k):
    """an explicit tune for a CONFIG code: tile, bkd (code 0 <- never, 1 <- two buffers, 2 <- one buffer), acc2 (forced on / off)"""
    if k.b3:
        return 100011
    return k.variant + 100 * {0: 2, 1: 1, 2: 3}[k.bkd] + 1000 * (2 if k.acc2 else 1)


def _kernel_cases():
    """two cases per reachable template instantiation: M below one tile (M = 1 among them), N ragged, a K tail where the rules admit
    one; and M past a tile and ragged, N past a tile and ragged, padded leading dimensions.  Gathers rotate through GATHER_KINDS."""
    out, gi, mi = [], 0, 0
    for code in NT_REACHABLE:
        k = nt_decode(code)
        if k.variant == 44:
            continue
        BM, BN = (128 if k.variant in (21, 22) else 64), (128 if k.variant in (12, 22) else 64)
        bk16 = k.bkd == 0
        for which in ("small", "ragged"):
            small = which == "small"
            kw = dict(tune=_tune_for(k), code=code)
            if k.a_bn:
                kw["epi"] = ("a_bn",)
            if k.vec:
                N = BN + 4 if small else 2 * BN + 12
                off = ()
            else:
                N = 3 if small else BN + 7                   # below 4, and odd
                off = ("A",) if small else ("W", "C")
            if not small:
                kw["ldc"] = N + (4 if k.vec else 1)
            if k.plain:
                if bk16 and not k.a_bn:
                    C = (84 if k.vec else 85) if small else 112            # K % 16 != 0: the tail
                elif bk16:
                    C = 80 if small else 112                               # a_bn: Cin % 16 == 0, not a whole 32-deep tile
                else:
                    C = 96 if small else 160
                M = (1, 37, 50, 63)[mi % 4] if small else 2 * BM + 5
                mi += small
                if not small:
                    kw.update(lda=C + (4 if k.vec else 3), ldb=C + (8 if k.vec else 5))
                out.append(nt(f"k{code}_{which}", N, C, M=M, off=off, **kw))
            else:
                kinds = [q for q in GATHER_KINDS if not (k.a_bn and GEOMS[q].mode == 1)]
                geom = kinds[gi % len(kinds)]
                gi += 1
                g = GEOMS[geom]
                taps = g.KH * g.KW
                if taps == 1:
                    C = ((80, 112) if bk16 else (96, 160))[not small]
                elif taps == 4:
                    C = ((48, 80) if bk16 else (32, 64))[not small]
                else:
                    C = ((16, 48) if bk16 else (32, 64))[not small]
                ohw = g.OH * g.OW
                nb = 1 if small else BM // ohw + 2
                if (nb * ohw) % BM == 0:
                    nb += 1
                if not small:
                    kw.update(lda=C + (4 if k.vec else 3), ldb=taps * C + (8 if k.vec else 5))
                out.append(nt(f"k{code}_{which}_{geom}", N, C, geom=geom, nb=nb, off=off, **kw))
    return out


def _epilogue_cases():
    """every epilogue operand singly and all together on 64x64 wide, 64x64 scalar (tune + 10000) and the 64x128 / 128x64 / 128x128
    tiles.  (150, 136, 48): ragged in both directions on every tile; resid / relu_mask with ldr, ldm != ldc."""
    out = []
    singles = [("alpha",), ("sub",), ("scale",), ("scale", "scale_var"), ("shift",), ("bias",), ("resid",), ("pre",), ("relu_mask",)]
    for tile, tune, variant in (("11w", 211, 11), ("11s", 10211, 11), ("12", 212, 12), ("21", 221, 21), ("22", 222, 22)):
        code = nt_code(variant, 0, 0, 1, 1)
        for epi in singles:
            out.append(nt(f"epi{tile}_{epi[-1]}", 136, 48, code, M=150, tune=tune, epi=epi, ldc=140, base=f"epi_{epi[-1]}"))
        for act in (1, 2):
            out.append(nt(f"epi{tile}_act{act}", 136, 48, code, M=150, tune=tune, act=act, ldc=140, base=f"epi_act{act}"))
            out.append(nt(f"epi{tile}_all_act{act}", 136, 48, code, M=150, tune=tune, epi=EPI_ALL, act=act, ldc=140, base=f"epi_all{act}"))
    return out


def _stats_cases():
    out = []
    for tile, tune, variant in (("11w", 211, 11), ("11s", 10211, 11), ("12", 212, 12), ("21", 221, 21), ("22", 222, 22)):
        out.append(nt(f"colstats{tile}", 136, 48, nt_code(variant, 0, 0, 1, 1), M=150, tune=tune, epi=("colstats", "alpha"), base="colstats"))
    out.append(nt("colstats_abn", 68, 48, nt_code(11, 0, 0, 1, 1, a_bn=1), M=70, tune=211, epi=("colstats", "a_bn")))
    out.append(nt("colstats_3x3s1", 68, 32, nt_code(11, 2, 0, 1, 0), geom="3x3s1", nb=3, tune=0, epi=("colstats",)))
    # BatchNorm-backward sums: the 16-byte epilogue of the 64x64 tile; mask carried (bs_relu 0) and recomputed (2), bs_tile0 > 0,
    # and under the strided output map (bs_y is indexed like the output)
    out.append(nt("bstats_relu0", 136, 48, nt_code(11, 0, 0, 1, 1), M=150, tune=211, epi=("bstats", "resid", "relu_mask"), bs_relu=0, bs_tile0=0))
    out.append(nt("bstats_relu2_tile3", 136, 48, nt_code(11, 0, 0, 1, 1), M=150, tune=211, epi=("bstats",), bs_relu=2, bs_tile0=3))
    out.append(nt("bstats_phase10", 68, 32, nt_code(11, 2, 0, 1, 0), geom="phase10", nb=7, tune=0, epi=("bstats",), bs_relu=2, bs_tile0=1))
    return out


def _big_cases():
    """gemm_nt_big_kernel: interior tiles only (M, N % 128 == 0) and at least 256 tiles of 64x64"""
    b = lambda a, ab=0: nt_code(44, 2, a, 1, 1, a_bn=ab)
    return [
        nt("big_k32_all", 1024, 32, b(0), M=1024, tune=44, epi=EPI_ALL, act=2),
        nt("big_k544", 512, 544, b(1), M=2048, tune=44, epi=("resid",), act=1, base="big544"),
        nt("big544_on_11", 512, 544, nt_code(11, 2, 1, 1, 1), M=2048, tune=11, epi=("resid",), act=1, base="big544"),
        nt("big_wide544_colstats", 1024, 544, b(1), M=1024, tune=44, epi=("colstats",), panel=4, base="wide544"),
        nt("wide544_on_11", 1024, 544, nt_code(11, 2, 1, 1, 1), M=1024, tune=11, epi=("colstats",), panel=4, base="wide544"),
        nt("narrow_no_panel", 1020, 32, nt_code(11, 2, 0, 1, 1), M=70, tune=11, panel=0),
        nt("big_abn_k32", 1024, 32, b(0, 1), M=1024, tune=44, epi=("a_bn", "bias")),
        nt("big_abn_acc2_k96", 512, 96, b(1, 1), M=2048, tune=2044, epi=("a_bn",)),
        nt("big_bstats", 1024, 32, b(0), M=1024, tune=44, epi=("bstats",), bs_relu=2, bs_tile0=2),
    ]


def _split_cases():
    """split-K (64x64 tiles, K >= 256, a workspace): the policy's choice and forced 2 / 3 / 7 / 8 slices of 17 32-deep k-tiles
    (K = 544: kpt = 10 / 6 / 4 / 4 -- the last slice short, and at 7 or 8 slices two or three empty), 34 16-deep ones, scalar loads at
    K = 286, a_bn, colstats, bstats and a 3x3 convolution whose slice boundary (k-tile 16 of 3 per tap) falls inside a tap"""
    out = [nt("split544_policy", 132, 544, nt_code(11, 2, 1, 1, 1), M=70, tune=0, force=0, splits=4, epi=("bias",), base="split544")]
    for s in (2, 3, 7, 8):
        out.append(nt(f"split544_force{s}", 132, 544, nt_code(11, 2, 1, 1, 1), M=70, tune=0, force=s, splits=s, epi=("bias",), base="split544"))
    out.append(nt("split544_bk16_force7", 132, 544, nt_code(11, 0, 0, 1, 1), M=70, tune=1211, force=7, splits=7, epi=("bias",), base="split544"))
    out.append(nt("split544_2buf_force3", 132, 544, nt_code(11, 1, 1, 1, 1), M=70, tune=111, force=3, splits=3, epi=("bias",), base="split544"))
    for s in (2, 3):
        out.append(nt(f"split286_scalar_force{s}", 7, 286, nt_code(11, 0, 0, 0, 1), M=37, tune=0, force=s, splits=s, epi=("resid",), act=1, base="split286"))
    out.append(nt("split272_abn_force3", 68, 272, nt_code(11, 0, 0, 1, 1, a_bn=1), M=70, tune=0, force=3, splits=3, epi=("a_bn",)))
    out.append(nt("split544_colstats_force3", 132, 544, nt_code(11, 2, 1, 1, 1), M=70, tune=0, force=3, splits=3, epi=("colstats",), base="split544"))
    out.append(nt("split544_bstats_force2", 132, 544, nt_code(11, 2, 1, 1, 1), M=70, tune=0, force=2, splits=2, epi=("bstats",), bs_relu=2, bs_tile0=1, base="split544"))
    out.append(nt("split_conv48_force2", 68, 48, nt_code(11, 0, 0, 1, 0), geom="3x3s1", nb=3, tune=211, force=2, splits=2, epi=("bias",)))
    return out


def _special_cases():
    """arguments no other test passes: a single tap with padding rows on an interior tile (32-deep and 16-deep), and bk16 / bk32 twins"""
    out = [nt("conv1x1_pad_bk32", 64, 32, nt_code(11, 2, 0, 1, 0), geom="1x1pad", nb=2, tune=0),
           nt("conv1x1_pad_bk16", 64, 48, nt_code(11, 0, 0, 1, 0), geom="1x1pad", nb=2, tune=0),
           nt("conv1x1_pad_abn", 64, 48, nt_code(11, 0, 0, 1, 0, a_bn=1), geom="1x1pad", nb=2, tune=0, epi=("a_bn",))]
    for acc in (1, 2):
        for bkd_t, bkd_c in ((2, 0), (1, 1), (3, 2)):
            out.append(nt(f"twin160_acc{acc}_bkd{bkd_c}", 136, 160, nt_code(11, bkd_c, acc - 1, 1, 1), M=150, tune=11 + 100 * bkd_t + 1000 * acc,
                          base="twin160"))
    return out


NT_CASES = _kernel_cases() + _epilogue_cases() + _stats_cases() + _big_cases() + _split_cases() + _special_cases()
NT_BY_NAME = {c.name: c for c in NT_CASES}
assert len(NT_BY_NAME) == len(NT_CASES)

# pairs of cases on the same operands whose products are documented to agree bit for bit (include/stil_hip.h, csrc/gemm.hip)
NT_EXACT = (
    [(f"twin160_acc{a}_bkd0", f"twin160_acc{a}_bkd{b}", "16-deep vs 32-deep k-tiles") for a in (1, 2) for b in (1, 2)]
    + [(f"epi11w_{n}", f"epi11s_{n}", "16-byte vs scalar epilogue") for n in ("all_act1", "all_act2", "resid", "pre", "relu_mask", "scale_var")]
    + [("colstats11w", "colstats11s", "16-byte vs scalar epilogue")]
    + [("big544_on_11", "big_k544", "tune 44 vs 11"), ("wide544_on_11", "big_wide544_colstats", "tune 44 vs 11")]
)
B3_CASES = [c.name for c in NT_CASES if nt_decode(c.code).b3]


def nt_slices(c):
    """the k-tile ranges [begin, end) of the slices of a split case, by the kernel's arithmetic (kpt in gemm_nt_kernel)"""
    k = nt_decode(c.code)
    BK = 32 if k.bkd else 16
    per_tap = cdiv(c.C, BK)
    nk_all = (1 if k.plain else c.g.KH * c.g.KW) * per_tap
    kpt = cdiv(nk_all, c.splits)
    kpt = cdiv(kpt, 64 // BK) * (64 // BK)
    return [(min(nk_all, s * kpt), min(nk_all, s * kpt + kpt)) for s in range(c.splits)], per_tap


def nt_tags(c):
    """which orientations of its kernel the case exercises"""
    k = nt_decode(c.code)
    BM, BN = nt_tile(c)
    tags = {"reached"}
    if c.M > BM and c.M % BM:
        tags.add("M%tile")
    if c.M < BM:
        tags.add("M<tile")
    if c.N % BN:
        tags.add("N%tile")
    if k.bkd == 0 and not k.b3 and ((c.K % 16 != 0) if (k.plain and not k.a_bn) else (c.C % 32 != 0)):
        tags.add("Ktail")
    return tags


def nt_coverage_gaps(cases):
    """what the NT table still misses: every reachable instantiation by M ragged past a tile, M below a tile, N ragged, and a K tail
    where 16-deep k-tiles admit one (the lean kernel only takes interior tiles: reached); every gather kind; M = 1; one image"""
    need = set()
    for code in NT_REACHABLE:
        k, kern = nt_decode(code), nt_kernel(code)
        need.add((kern, "reached"))
        if k.variant != 44:
            need |= {(kern, "M%tile"), (kern, "M<tile"), (kern, "N%tile")}
            if k.bkd == 0 and not k.b3:
                need.add((kern, "Ktail"))
    need |= {("gather", q) for q in GATHER_KINDS} | {("shape", "M=1"), ("shape", "one image")}
    for c in cases:
        kern = nt_kernel(c.code)
        for t in nt_tags(c):
            need.discard((kern, t))
        need.discard(("gather", c.geom))
        if c.M == 1:
            need.discard(("shape", "M=1"))
        if c.geom != "plain" and c.nb == 1:
            need.discard(("shape", "one image"))
    return sorted(need)


# ------------------------------------------------------------------------------------------------------------------------------
# weight-gradient cases
def wg(name, N, C, code, geom="plain", M=None, nb=None, tune=0, ldy=None, ldx=None, off=(), Kdst=None, accumulate=0, x_bn=False,
       force=0, splits=1, partial=False):
    g = GEOMS[geom]
    nb = M if geom == "plain" else nb
    M = nb * g.OH * g.OW
    K = g.KH * g.KW * C
    return NS(name=name, M=M, N=N, K=K, C=C, nb=nb, geom=geom, g=g, tune=tune, code=code, family="wgrad", ldy=N if ldy is None else ldy,
              ldx=C if ldx is None else ldx, off=frozenset(off), Kdst=K if Kdst is None else Kdst, accumulate=accumulate, x_bn=x_bn,
              force=force, splits=splits, partial=partial, base=name)


def wg_slabs(c):
    """row ranges [begin, end) of the slabs, by wgrad_tn_impl's arithmetic: slabs of 16 ceil(ceil(M / s) / 16) rows"""
    mps = cdiv(cdiv(c.M, c.splits), 16) * 16
    return [(z * mps, max(z * mps, min(c.M, z * mps + mps))) for z in range(c.splits)]


def _wg_kernel_cases():
    out, gi = [], 0
    for tile in (11, 12, 22):
        BN, BK = (128 if tile == 22 else 64), (64 if tile == 11 else 128)
        tune = 11 if tile == 11 else 22
        for kind in ("scalar", "vec", "xbn"):
            vec = kind != "scalar"
            code = wg_code(tile, int(vec), int(kind == "xbn"), 1)
            # small: one tile, ragged N and K, M below 16 or no multiple of 16; a plain product
            N = {11: 36, 12: 36, 22: 68}[tile] - (0 if vec else 1)
            C = 40 if vec else 37
            M = 9 if kind != "vec" else 37
            out.append(wg(f"w{code}_small", N, C, code if vec else wg_code(tile, 0, 0, 0), M=M, tune=tune, x_bn=kind == "xbn"))
            # ragged: past a tile in N (the 64-column tile of N <= 64 excepted) and K, a gather, padded leading dimensions
            geom = WG_GEOMS[gi % len(WG_GEOMS)]
            gi += 1
            g = GEOMS[geom]
            taps = g.KH * g.KW
            C = 20 if taps > 1 else 148
            N = {11: 68, 12: 60, 22: 132}[tile] + (0 if vec else 1)
            nb = 40 // (g.OH * g.OW) + 3
            if (nb * g.OH * g.OW) % 16 == 0:
                nb += 1
            out.append(wg(f"w{code}_ragged_{geom}", N, C, code, geom=geom, nb=nb, tune=tune, x_bn=kind == "xbn", ldy=N + (4 if vec else 3),
                          ldx=C + (8 if vec else 4), off=() if vec else ("dY",)))
    return out


def _wg_slab_cases():
    v, s_ = wg_code(11, 1, 0, 1), wg_code(11, 0, 0, 0)
    out = [wg(f"slab100_force{f}", 36, 40, v, M=100, force=f, splits=min(f, 6)) for f in (1, 2, 5, 6)]       # 6 = M / 16: two empty slabs
    out += [
        wg("slab9_force5", 36, 40, v, M=9, force=5, splits=1),                                               # M < 16: one slab
        wg("slab_policy5", 20, 24, v, M=1300, splits=5),                                                     # the policy's own split
        wg("slab_grid3x3_force2", 36, 20, v, geom="grid3x3", nb=5, force=2, splits=2),                       # slab 1 starts inside image 3
        wg("slab_grid1x5_force2", 36, 20, v, geom="grid1x5", nb=9, force=2, splits=2, accumulate=1),
        wg("kdst_reduce4", 36, 40, v, M=37, Kdst=33),
        wg("kdst_reduce4_acc", 36, 40, v, M=37, Kdst=33, accumulate=1, force=2, splits=2),
        wg("kdst_reduce", 35, 37, s_, M=37, Kdst=30),
        wg("kdst_reduce_acc", 35, 37, s_, M=37, Kdst=30, accumulate=1, force=2, splits=2),
        wg("reduce_taps_unaligned_ws", 36, 20, wg_code(11, 1, 0, 0), geom="3x3s1", nb=2, off=("ws",), force=3, splits=3),
        wg("reduce_taps_unaligned_ws_acc", 36, 20, wg_code(11, 1, 0, 0), geom="3x3s2", nb=4, off=("ws",), accumulate=1),
        wg("partial_force5", 36, 40, v, M=100, force=5, splits=5, partial=True),
        wg("partial_taps_xbn", 68, 20, wg_code(22, 1, 1, 1), geom="3x3s1", nb=3, tune=22, x_bn=True, force=2, splits=2, partial=True),
    ]
    return out


WG_CASES = _wg_kernel_cases() + _wg_slab_cases()
WG_BY_NAME = {c.name: c for c in WG_CASES}
assert len(WG_BY_NAME) == len(WG_CASES)


def wg_tags(c):
    BN, BK = (128 if c.code % 100 == 22 else 64), (64 if c.code % 100 == 11 else 128)
    tags = {"reached"}
    if c.N % BN:
        tags.add("N%tile")
    if c.K % BK:
        tags.add("K%tile")
    if c.K > BK:
        tags.add("K>tile")
    if c.M % 16:
        tags.add("M%16")
    return tags


def wg_coverage_gaps(cases):
    need = {(wg_kernel(code), t) for code in WG_REACHABLE for t in ("reached", "N%tile", "K%tile", "K>tile", "M%16")}
    need |= {r for r in WG_REDUCES} | {("slabs", q) for q in ("M<16", "empty slab", "many", "force 1", "force 2", "force 5", "force M/16")}
    need |= {("reduce", q) for q in ("Kdst<K reduce4", "Kdst<K reduce", "accumulate 0", "accumulate 1", "partial")}
    need |= {("gather", q) for q in WG_GEOMS}
    for c in cases:
        for t in wg_tags(c):
            need.discard((wg_kernel(c.code), t))
        taps = c.g.KH * c.g.KW
        if not c.partial:
            red = "wgrad_reduce4_kernel" if c.code // 10000 else "wgrad_reduce_kernel"
            need.discard((red, "taps>1" if taps > 1 else "taps==1"))
            need.discard(("reduce", f"accumulate {c.accumulate}"))
            if c.Kdst < c.K and taps == 1:
                need.discard(("reduce", "Kdst<K reduce4" if c.code // 10000 else "Kdst<K reduce"))
        else:
            need.discard(("reduce", "partial"))
        need.discard(("gather", c.geom))
        if c.M < 16:
            need.discard(("slabs", "M<16"))
        if any(b == e for b, e in wg_slabs(c)):
            need.discard(("slabs", "empty slab"))
        if c.splits >= 5 and not c.force:
            need.discard(("slabs", "many"))
        if c.force:
            need.discard(("slabs", "force M/16" if c.force == c.M // 16 else f"force {c.force}"))
    return sorted(need)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs (fp32 numbers, seeded by the case's `base`: twins share their operands) and the definitions
def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.base.encode()))


def _stats_block(y2d, gen):
    """[4][C] = mean, rstd, a = gamma rstd, beta of the columns of y2d, as stil_bn_train_fwd_tiles writes it"""
    mean = y2d.mean(0)
    rstd = 1.0 / torch.sqrt(y2d.var(0, unbiased=False) + 1e-5)
    gamma, beta = 0.5 + torch.rand(y2d.shape[1], generator=gen), 0.2 * torch.randn(y2d.shape[1], generator=gen)
    return torch.stack([mean, rstd, gamma * rstd, beta]).float().contiguous()


def nt_inputs(c):
    """logical operands: A [nb, H, W, C], W [N, K], per-column vectors [N], resid / relu_mask / bs_y [M, N] in GEMM-row order"""
    gen, g = _gen(c), c.g
    r = lambda *s: torch.randn(*s, generator=gen)
    x = {"A": r(c.nb, g.H, g.W, c.C), "W": r(c.N, c.K) * (2.0 * c.K ** -0.5)}
    for n in ("sub", "shift", "bias"):
        x[n] = r(c.N)
    x["scale"] = 0.5 + torch.rand(c.N, generator=gen)
    x["scale_var"] = 0.5 + torch.rand(c.N, generator=gen)
    x["resid"], x["relu_mask"] = r(c.M, c.N), r(c.M, c.N)
    x["a_bn"] = _stats_block(x["A"].reshape(-1, c.C) * 1.5 + 0.2, gen)
    x["a_bn"][1] = NAN                                  # rstd: the operand staging reads rows 0, 2 and 3 only
    x["bs_y"] = r(c.M, c.N) * 2 + 0.3
    x["bs_stats"] = _stats_block(x["bs_y"], gen)
    return x


def gather(src, g, C):
    """src [nb, H, W, C] -> Agather [nb OH OW, KH KW C]"""
    nb = src.shape[0]
    oy, ox = torch.arange(g.OH)[:, None], torch.arange(g.OW)[None, :]
    cols = []
    for ky in range(g.KH):
        for kx in range(g.KW):
            if g.mode == 0:
                iy, ix = oy * g.stride - g.pad_y + ky, ox * g.stride - g.pad_x + kx
                ok = torch.ones(g.OH, g.OW, dtype=torch.bool)
            else:
                ty, tx = oy + g.pad_y - ky, ox + g.pad_x - kx
                ok = (ty >= 0) & (tx >= 0) & (ty % g.stride == 0) & (tx % g.stride == 0)
                iy, ix = torch.div(ty, g.stride, rounding_mode="floor"), torch.div(tx, g.stride, rounding_mode="floor")
            ok = ok & (iy >= 0) & (iy < g.H) & (ix >= 0) & (ix < g.W)
            iyc, ixc = iy.clamp(0, g.H - 1).expand(g.OH, g.OW), ix.clamp(0, g.W - 1).expand(g.OH, g.OW)
            v = src[:, iyc, ixc, :]
            cols.append(torch.where(ok[None, :, :, None], v, torch.zeros((), dtype=src.dtype)))
    return torch.cat(cols, dim=-1).reshape(nb * g.OH * g.OW, g.KH * g.KW * C)


def _staged(src, stats, dtype):
    """relu((y - mean) a + beta) from rows 0, 2, 3 of the statistics block"""
    st = stats.to(dtype)
    return torch.relu((src - st[0]) * st[2] + st[3])


def row_map(c):
    """output row of every GEMM row m = (n, oy, ox), and the number of output rows"""
    g = c.g
    m = torch.arange(c.M)
    n, rem = m // (g.OH * g.OW), m % (g.OH * g.OW)
    oy, ox = rem // g.OW, rem % g.OW
    return (n * g.oOH + oy * g.os + g.opy) * g.oOW + ox * g.os + g.opx, c.nb * g.oOH * g.oOW


def nt_eval(c, x, dtype):
    """the definition in `dtype` -> {"C", "pre", "colstats", "bstats"} in GEMM-row order (those the case asks for)"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)             # the fp32 number the entry point receives
    src = x["A"].to(dtype)
    if "a_bn" in c.epi:
        src = _staged(src, x["a_bn"], dtype)
    P = gather(src, c.g, c.C) @ x["W"].to(dtype).t()
    v = P * f32(c.alpha)
    out = {}
    if "colstats" in c.epi:
        T = nt_stat_rows(c)
        rows = []
        for t in range(cdiv(c.M, T)):
            blk = v[T * t: T * t + T]
            mean = blk.mean(0)
            rows += [mean, ((blk - mean) ** 2).sum(0)]
        out["colstats"] = torch.stack(rows)
    e = lambda n: x[n].to(dtype)
    if "scale" in c.epi or "sub" in c.epi or "shift" in c.epi or "bias" in c.epi:
        sc = e("scale") if "scale" in c.epi else torch.ones(c.N, dtype=dtype)
        if "scale_var" in c.epi:
            sc = sc / torch.sqrt(e("scale_var") + f32(c.var_eps))
        v = (v - (e("sub") if "sub" in c.epi else 0.0)) * sc + (e("shift") if "shift" in c.epi else 0.0) + (e("bias") if "bias" in c.epi else 0.0)
    if "resid" in c.epi:
        v = v + e("resid")
    if "pre" in c.epi:
        out["pre"] = v
    if c.act == 1:
        v = torch.relu(v)
    elif c.act == 2:
        v = F.gelu(v)
    if "relu_mask" in c.epi:
        v = torch.where(x["relu_mask"] > 0, v, torch.zeros((), dtype=dtype))
    out["C"] = v
    if "bstats" in c.epi:
        y, st = e("bs_y"), x["bs_stats"].to(dtype)
        gq = torch.where((y - st[0]) * st[2] + st[3] > 0, v, torch.zeros((), dtype=dtype)) if c.bs_relu == 2 else v
        xhat = (y - st[0]) * st[1]
        rows = []
        for t in range(cdiv(c.M, 64)):
            sl = slice(64 * t, 64 * t + 64)
            rows += [gq[sl].sum(0), (gq[sl] * xhat[sl]).sum(0)]
        out["bstats"] = torch.stack(rows)
    return out


def wg_inputs(c):
    gen, g = _gen(c), c.g
    r = lambda *s: torch.randn(*s, generator=gen)
    x = {"dY": r(c.M, c.N), "X": r(c.nb, g.H, g.W, c.C)}
    x["x_bn"] = _stats_block(x["X"].reshape(-1, c.C) * 1.5 + 0.2, gen)
    x["x_bn"][1] = NAN
    x["init"] = r(c.N, c.Kdst)                          # what dW holds before an accumulating call
    return x


def wg_eval(c, x, dtype):
    """-> {"dW": [N, Kdst] in the destination layout, "P": [N, K] the sum of the slabs in the kernel's (tap, channel) order}"""
    src = x["X"].to(dtype)
    if c.x_bn:
        src = _staged(src, x["x_bn"], dtype)
    P = x["dY"].to(dtype).t() @ gather(src, c.g, c.C)
    taps = c.g.KH * c.g.KW
    dW = P.view(c.N, taps, c.C).permute(0, 2, 1).reshape(c.N, c.K) if taps > 1 else P
    dW = dW[:, :c.Kdst]
    if c.accumulate:
        dW = dW + x["init"].to(dtype)
    return {"dW": dW, "P": P}


def nerr(a, b):
    """max |a - b| / (1 + |b| + max|b|): the normalisation of test_gpu_ops.close(); NaN if anything is"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b).abs() / (1.0 + b.abs() + b.abs().max())).max())


def check_nt(c, got, ref, bound, tag="GEMM_ERR"):
    """prints every figure, -> the outputs of the case beyond `bound` (a NaN is beyond it)"""
    bad = []
    for key, r in ref.items():
        e = nerr(got[key], r)
        print(f"{tag} {c.family} {c.name} {nt_kernel(c.code)} {key} {e:.3e} bound {bound:.3e}")
        if not e <= bound:
            bad.append((key, e))
    return bad


def check_wg(c, got, ref, bound, keys=("dW",), tag="GEMM_ERR"):
    bad = []
    for key in keys:
        e = nerr(got[key], ref[key])
        print(f"{tag} {c.family} {c.name} {wg_kernel(c.code)} {key} {e:.3e} bound {bound:.3e}")
        if not e <= bound:
            bad.append((key, e))
    return bad


_REF, _ATEN = {}, {}


def reference(c):
    """(inputs, float64 outputs) of a case, computed once per process and left unchanged"""
    if c.name not in _REF:
        x = (wg_inputs if c.family == "wgrad" else nt_inputs)(c)
        _REF[c.name] = (x, (wg_eval if c.family == "wgrad" else nt_eval)(c, x, torch.float64))
    return _REF[c.name]


def aten_errors():
    """{family: the largest error of the fp32 ATen evaluation against float64 over the family's cases and outputs}"""
    if not _ATEN:
        worst = {f: 0.0 for f in FAMILIES}
        for c in NT_CASES + WG_CASES:
            x, r64 = reference(c)
            r32 = (wg_eval if c.family == "wgrad" else nt_eval)(c, x, torch.float32)
            keys = ("dW",) if c.family == "wgrad" else r64.keys()
            worst[c.family] = max([worst[c.family]] + [nerr(r32[k], r64[k]) for k in keys])
        _ATEN.update(worst)
    return dict(_ATEN)


def bounds():
    """the kernels' bound per family: FACTOR x the family's yardstick, capped at TOL"""
    return {f: min(TOL, FACTOR * e) for f, e in aten_errors().items()}


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())
