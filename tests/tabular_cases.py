"""The cases of tests/test_gpu_tabular.py as data, and the float64 definitions they are compared with.

Three families, one per pair of entry points: `tab` (stil_tab_embed_fwd / _bwd, models/Transformer.py:240-256), `saint`
(stil_saint_embed_fwd / _bwd, STiLModel_SAINT_backbone.py:159-180) and `mlp` (stil_colmlp_fwd / _bwd, the per-column
simple_MLP(1 -> hid -> d) of SAINT/model_util.py:79-87).  Every operand comes from a seeded CPU generator; the definitions are the
reference model's formulas written out in torch and differentiated by float64 autograd; `*_seq32` restates each in fp32 with
the batch sums taken one sample after the other, which is the order of the kernels (no atomics, one thread per output
element looping over b) and so the yardstick for the tolerance the GPU module uses.

This module imports neither the library nor CUDA: tests/test_tabular_cases_cpu.py runs everything here on the host."""
import functools
from collections import namedtuple

import torch

SENT = -777.0
NAN = float("nan")
MAXE, BLOCK = 16, 256                       # colmlp_bwd_kernel: dW2 entries per thread, threads per block
TAB_BLOCKS = (64, 256)                      # tab_embed_bwd_fin (64 threads, one element each) / _tok and _emb (256, stride loop)
SAINT_BLOCK = 64                            # saint_embed_bwd_emb / _pos (stride loop)

Tab = namedtuple("Tab", "name B D cards ncon")               # x = [categorical columns | continuous columns]
Saint = namedtuple("Saint", "name B d cards ncon")           # cards: the categorical columns (the CLS column is added)
Mlp = namedtuple("Mlp", "name B d hid ncon ncat bwd edges")  # bwd: the backward takes the shape; edges: the ReLU units below


def gen(*key):
    g = torch.Generator()
    g.manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) % (2 ** 31))
    return g


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------- cases
TAB_LAYOUTS = {"cat": ((1, 4, 3, 5), 0), "con": ((), 3), "mixed": ((3, 1, 4), 2)}
TAB_CASES = [Tab(f"{lay}_D{D}_B{B}", B, D, *TAB_LAYOUTS[lay]) for lay in TAB_LAYOUTS for D in (1, 48, 64, 260, 512) for B in (1, 9, 300)]

SAINT_CARDS = {0: (), 1: (4,), 5: (1, 4, 3, 5, 2)}
SAINT_CASES = [Saint(f"ncat{n}_d{d}_B{B}", B, d, SAINT_CARDS[n], 3 if n else 2) for n in (0, 1, 5) for d in (8, 32, 72) for B in (1, 12, 257)]

MLP_CASES = [
    Mlp("model_B12", 12, 32, 100, 3, 2, True, True),
    Mlp("model_B1", 1, 32, 100, 1, 0, True, True),
    Mlp("model_B257", 257, 32, 100, 3, 0, True, True),
    Mlp("maxe_hid256", 12, 16, 256, 1, 2, True, True),
    Mlp("maxe_d256", 12, 256, 16, 3, 0, True, True),
    Mlp("ragged_40x100", 257, 40, 100, 1, 2, True, True),
    Mlp("odd_33x7", 1, 33, 7, 3, 2, True, True),
    Mlp("one_by_one", 12, 1, 1, 3, 0, True, False),
    Mlp("fwd_only_64x200", 12, 64, 200, 3, 2, False, True),
]
# every count of dW2 entries per thread below the bound: d * hid = 256 k - 16, a ragged last group of 240
MLP_CASES += [Mlp(f"ne{k}", 3, 16, 16 * k - 1, 1 + 2 * (k % 2), 2 * (k % 2), True, True) for k in range(2, 16)]

CASES = {"tab": TAB_CASES, "saint": SAINT_CASES, "mlp": MLP_CASES}
BY_NAME = {(f, c.name): c for f, cs in CASES.items() for c in cs}
RUNS = [(f, c.name, acc) for f, cs in CASES.items() for c in cs for acc in (0, 1)]   # every case with accumulate 0 and 1
# the forward of both SAINT kernels on one token buffer: (saint case, hidden width of the column MLPs)
OWNERSHIP = [("ncat5_d32_B12", 100), ("ncat0_d8_B257", 100), ("ncat1_d72_B1", 100)]


def accumulates(family, name):
    """the accumulate values the GPU module runs this case's backward with"""
    return [a for f, n, a in RUNS if (f, n) == (family, name)]


def mlp_ne(c):
    return cdiv(c.d * c.hid, BLOCK)


def tab_layout(c):
    return "cat" if not c.ncon else ("mixed" if c.cards else "con")


def coverage_gaps(runs=None):
    """what the list of (family, case, accumulate) runs does not reach, computed from the case data"""
    runs = RUNS if runs is None else runs
    gaps = []
    by = {f: [BY_NAME[f, n] for ff, n, _ in runs if ff == f] for f in CASES}
    bwd = [c for c in by["mlp"] if c.bwd]
    gaps += [("mlp", f"ne={k}") for k in range(1, MAXE + 1) if k not in {mlp_ne(c) for c in bwd}]
    full = [c for c in bwd if c.d * c.hid == MAXE * BLOCK]
    gaps += [("mlp", t) for t, ok in (("ne=16 with hid=256", any(c.hid == BLOCK for c in full)), ("ne=16 with d=256", any(c.d == BLOCK for c in full)),
                                      ("ragged last group", any(c.d * c.hid % BLOCK and mlp_ne(c) == MAXE for c in bwd)),
                                      ("hid>d", any(c.hid > c.d for c in bwd)), ("hid<d", any(c.hid < c.d for c in bwd)),
                                      ("forward beyond the backward's bound", any(not c.bwd for c in by["mlp"])),
                                      ("relu edges", any(c.edges for c in bwd)), ("tok0=1", any(c.ncat == 0 for c in bwd)),
                                      ("tok0=3", any(c.ncat == 2 for c in bwd)), ("ncon=1", any(c.ncon == 1 for c in bwd)),
                                      ("ncon=3", any(c.ncon == 3 for c in bwd))) if not ok]
    for blk in TAB_BLOCKS:
        Ds = {c.D for c in by["tab"]}
        gaps += [("tab", f"D{rel}{blk}") for rel, ok in (("<", any(D < blk for D in Ds)), (">", any(D > blk for D in Ds))) if not ok]
    gaps += [("tab", "partial last 64-thread block")] if not any(c.D > 64 and c.D % 64 for c in by["tab"]) else []
    ds = {c.d for c in by["saint"]}
    gaps += [("saint", f"d{rel}{SAINT_BLOCK}") for rel, ok in (("<", any(d < SAINT_BLOCK for d in ds)), (">", any(d > SAINT_BLOCK for d in ds))) if not ok]
    gaps += [("tab", f"layout {lay}") for lay in TAB_LAYOUTS if lay not in {tab_layout(c) for c in by["tab"]}]
    gaps += [("saint", f"ncat={n}") for n in SAINT_CARDS if n not in {len(c.cards) for c in by["saint"]}]
    for f in CASES:
        Bs = {c.B for c in by[f]}
        gaps += [(f, "B=1")] if 1 not in Bs else []
        gaps += [(f, "B beyond one block")] if not any(B > BLOCK for B in Bs) else []
        for acc in (0, 1):
            missing = {c.name for c in CASES[f] if c in by[f]} - {n for ff, n, a in runs if ff == f and a == acc}
            gaps += [(f, f"accumulate={acc}")] if missing or not by[f] else []
    return gaps


# --------------------------------------------------------------------------------------------------------------- inputs
def interleave(ncat, ncon):
    """columns of x by kind, mixed as field_lengths=[3,4,1,5,1,1,2] mixes them -> (cat_cols, con_cols)"""
    cat, con, i = [], [], 0
    while len(cat) < ncat or len(con) < ncon:
        k = "NKKNKNNK"[i % 8]
        i += 1
        if k == "K" and len(cat) < ncat:
            cat.append(len(cat) + len(con))
        elif k == "N" and len(con) < ncon:
            con.append(len(cat) + len(con))
    return cat, con


def codes(cards, B, g):
    """[B, len(cards)] integer codes with the edges: a column of one category; in the first column of 4 or more categories no
    sample draws code 2; in the first column of exactly 3 every sample has code 1"""
    cols, holed, same = [], False, False
    for card in cards:
        v = torch.randint(0, card, (B,), generator=g)
        if card >= 4 and not holed:
            v = torch.where(v == 2, torch.full_like(v, card - 1), v)
            holed = True
        elif card == 3 and not same:
            v = torch.ones_like(v)
            same = True
        cols.append(v)
    return torch.stack(cols, 1) if cols else torch.zeros((B, 0), dtype=torch.long)


def _r(g, *shape):
    return torch.randn(*shape, generator=g)


def _table(cards):
    offs = torch.tensor([0] + list(cards), dtype=torch.int64).cumsum(0)[:-1].to(torch.int32)
    rowcol = torch.cat([torch.full((c,), j, dtype=torch.int32) for j, c in enumerate(cards)]) if cards else torch.zeros(0, dtype=torch.int32)
    return offs, rowcol


@functools.lru_cache(maxsize=None)
def tab_inputs(c):
    g = gen(1, c.B, c.D, len(c.cards), c.ncon)
    ncat, T = len(c.cards), len(c.cards) + c.ncon + 1
    con = _r(g, c.B, c.ncon)
    if c.ncon:
        con[0, 0] = 0.0                                                   # an exact zero among the continuous values
    x = dict(x=torch.cat([codes(c.cards, c.B, g).float(), con], 1), g=_r(g, c.B, T, c.D), cls=_r(g, c.D), colemb=_r(g, T, c.D))
    x["offs"], x["rowcol"] = _table(list(c.cards))
    if ncat:
        x["emb"] = _r(g, sum(c.cards), c.D)
    if c.ncon:
        x["con_w"], x["con_b"] = _r(g, c.D), _r(g, c.D)
    for k in TAB_GRADS:
        if k[2:] in x:
            x["pre_" + k] = _r(g, *x[k[2:]].shape)
    return x


TAB_GRADS = ("d_emb", "d_con_w", "d_con_b", "d_cls", "d_colemb")


@functools.lru_cache(maxsize=None)
def saint_inputs(c):
    """x [B, ncat + ncon] with the columns interleaved; the table has the CLS column (one row) in front; pos has ncat + ncon rows"""
    g = gen(2, c.B, c.d, len(c.cards), c.ncon)
    ncat = len(c.cards)
    cat_cols, con_cols = interleave(ncat, c.ncon)
    xx = torch.empty(c.B, ncat + c.ncon)
    xx[:, cat_cols] = codes(c.cards, c.B, g).float()
    xx[:, con_cols] = _r(g, c.B, c.ncon)
    cards = [1] + list(c.cards)
    x = dict(x=xx, cat_cols=torch.tensor(cat_cols, dtype=torch.int32), con_cols=torch.tensor(con_cols, dtype=torch.int32),
             g=_r(g, c.B, ncat + c.ncon + 1, c.d), emb=_r(g, sum(cards), c.d), pos=_r(g, ncat + c.ncon, c.d))
    x["offs"], x["rowcol"] = _table(cards)
    x["pre_d_emb"], x["pre_d_pos"] = _r(g, *x["emb"].shape), _r(g, *x["pos"].shape)
    return x


MLP_PARAMS = ("w1", "b1", "W2", "b2")


def _mlp_params(g, c):
    p = dict(w1=[_r(g, c.hid) for _ in range(c.ncon)], b1=[_r(g, c.hid) for _ in range(c.ncon)],
             W2=[_r(g, c.d, c.hid) / c.hid ** 0.5 for _ in range(c.ncon)], b2=[_r(g, c.d) for _ in range(c.ncon)])
    for k in MLP_PARAMS:
        p["pre_d_" + k] = [_r(g, *t.shape) for t in p[k]]
    return p


@functools.lru_cache(maxsize=None)
def mlp_inputs(c):
    """x [B, ncat + ncon] interleaved; per column w1 [hid], b1 [hid], W2 [d, hid], b2 [d], each a tensor of its own.
    With c.edges, column 0 has sample 0 at x = 0 and unit 0 with b1 = 0 (pre-activation exactly 0), unit 1 dead for every
    sample (w1 = 0, b1 = -1) and unit 2 live for every sample (w1 = 0, b1 = 1)."""
    g = gen(3, c.B, c.d, c.hid, c.ncon, c.ncat)
    cat_cols, con_cols = interleave(c.ncat, c.ncon)
    xx = torch.empty(c.B, c.ncat + c.ncon)
    xx[:, cat_cols] = torch.randint(0, 3, (c.B, c.ncat), generator=g).float()
    xx[:, con_cols] = _r(g, c.B, c.ncon)
    x = dict(x=xx, cat_cols=torch.tensor(cat_cols, dtype=torch.int32), con_cols=torch.tensor(con_cols, dtype=torch.int32),
             g=_r(g, c.B, c.ncat + c.ncon + 1, c.d), **_mlp_params(g, c))
    if c.edges:
        assert c.hid >= 3
        xx[0, con_cols[0]] = 0.0
        x["b1"][0][0] = 0.0
        x["w1"][0][1], x["b1"][0][1] = 0.0, -1.0
        x["w1"][0][2], x["b1"][0][2] = 0.0, 1.0
    return x


@functools.lru_cache(maxsize=None)
def ownership_inputs(name, hid):
    """a saint case plus column MLPs of its width: the operands of both forwards on one [B, nfeats, d] buffer"""
    c = BY_NAME["saint", name]
    m = Mlp(name, c.B, c.d, hid, c.ncon, len(c.cards), False, False)
    return c, m, dict(saint_inputs(c), **_mlp_params(gen(4, c.B, c.d, hid), m))


def relu_units(c, x):
    """(exactly zero, dead for every sample, live for every sample) pre-activations of column 0, counted in float64"""
    pre = x["x"][:, x["con_cols"][0].item()].double()[:, None] * x["w1"][0].double() + x["b1"][0].double()
    return int((pre == 0).sum()), int((pre < 0).all(0).sum()), int((pre > 0).all(0).sum())


def table_index(x, cls_column):
    """[B, tokens] rows of the embedding table: code + offset, the CLS column (SAINT) has code 0"""
    cols = x["x"][:, x["cat_cols"].long()] if cls_column else x["x"][:, :x["offs"].numel()]
    code = cols.long()
    if cls_column:
        code = torch.cat([torch.zeros(code.shape[0], 1, dtype=torch.long), code], 1)
    return code + x["offs"].long()


def undrawn_rows(x, cls_column):
    n = x["emb"].shape[0]
    return sorted(set(range(n)) - set(table_index(x, cls_column).flatten().tolist()))


# ---------------------------------------------------------------------------------------------------------- definitions
def tab_forward(c, x, p, dt, offs=None):
    """h [B, 1 + ncols, D]: cls | cat_embedding(x_cat + offsets) | x_con * w + b, all plus the column embedding"""
    ncat = len(c.cards)
    parts = [p["cls"].expand(c.B, 1, c.D)]
    if ncat:
        idx = x["x"][:, :ncat].long() + (x["offs"] if offs is None else offs).long()
        parts.append(p["emb"][idx % p["emb"].shape[0]])
    if c.ncon:
        parts.append(x["x"][:, ncat:].to(dt).unsqueeze(-1) * p["con_w"] + p["con_b"])
    return torch.cat(parts, 1) + p["colemb"]


def saint_forward(c, x, p, dt, offs=None):
    """out [B, ncat + 1, d] = embeds(cat(cls code 0, x_categ) + categories_offset) + pos_encodings(arange(ncat + 1))"""
    ncat = len(c.cards)
    code = torch.cat([torch.zeros(c.B, 1, dtype=torch.long), x["x"][:, x["cat_cols"].long()].long()], 1)
    idx = code + (x["offs"] if offs is None else offs).long()
    return p["emb"][idx % p["emb"].shape[0]] + p["pos"][:ncat + 1]


def mlp_forward(c, x, p, dt):
    """out [B, ncon, d]: column j is Linear(hid, d)(relu(Linear(1, hid)(x[:, con_cols[j]])))"""
    outs = []
    for j in range(c.ncon):
        xv = x["x"][:, x["con_cols"][j].item()].to(dt)
        outs.append(torch.relu(xv[:, None] * p["w1"][j] + p["b1"][j]) @ p["W2"][j].T + p["b2"][j])
    return torch.stack(outs, 1)


def _leaves(x, names, dt):
    out = {}
    for k in names:
        if k in x:
            v = x[k]
            out[k] = [t.to(dt).requires_grad_() for t in v] if isinstance(v, list) else v.to(dt).requires_grad_()
    return out


def _autograd(fwd, c, x, names, g):
    p = _leaves(x, names, torch.float64)
    out = fwd(c, x, p, torch.float64)
    flat = [t for k in p for t in (p[k] if isinstance(p[k], list) else [p[k]])]
    grads = iter(torch.autograd.grad(out, flat, g.double(), allow_unused=True))
    ref = {"out": out.detach()}
    for k in p:
        if isinstance(p[k], list):
            ref["d_" + k] = [next(grads) for _ in p[k]]
        else:
            gr = next(grads)
            ref["d_" + k] = torch.zeros_like(p[k]) if gr is None else gr
    return ref


@functools.lru_cache(maxsize=None)
def tab_reference(c):
    return _autograd(tab_forward, c, tab_inputs(c), ("emb", "con_w", "con_b", "cls", "colemb"), tab_inputs(c)["g"])


@functools.lru_cache(maxsize=None)
def saint_reference(c):
    x = saint_inputs(c)
    return _autograd(saint_forward, c, x, ("emb", "pos"), x["g"][:, :len(c.cards) + 1])


@functools.lru_cache(maxsize=None)
def mlp_reference(c):
    x = mlp_inputs(c)
    return _autograd(mlp_forward, c, x, MLP_PARAMS, x["g"][:, c.ncat + 1:])


@functools.lru_cache(maxsize=None)
def ownership_reference(name, hid):
    """the full [B, nfeats, d] buffer in float64: the categorical tokens, then the continuous ones"""
    c, m, x = ownership_inputs(name, hid)
    f64 = lambda names: {k: ([t.double() for t in x[k]] if isinstance(x[k], list) else x[k].double()) for k in names}
    return torch.cat([saint_forward(c, x, f64(("emb", "pos")), torch.float64), mlp_forward(m, x, f64(MLP_PARAMS), torch.float64)], 1)


REFERENCE = {"tab": tab_reference, "saint": saint_reference, "mlp": mlp_reference}
INPUTS = {"tab": tab_inputs, "saint": saint_inputs, "mlp": mlp_inputs}


def mlp_manual_grads(c, x, ge=False):
    """the column MLP's gradients written out in float64 (no autograd), with the ReLU mask `> 0` as ATen takes it, or `>= 0`"""
    out = {"d_" + k: [] for k in MLP_PARAMS}
    for j in range(c.ncon):
        xv = x["x"][:, x["con_cols"][j].item()].double()
        gb = x["g"][:, c.ncat + 1 + j].double()
        pre = xv[:, None] * x["w1"][j].double() + x["b1"][j].double()
        hv = pre.clamp_min(0)
        dh = (gb @ x["W2"][j].double()) * ((pre >= 0) if ge else (pre > 0))
        out["d_w1"].append((dh * xv[:, None]).sum(0))
        out["d_b1"].append(dh.sum(0))
        out["d_W2"].append(gb.T @ hv)
        out["d_b2"].append(gb.sum(0))
    return out


# ------------------------------------------------------------------------------------- fp32, batch sums in batch order
def _seq(rows):
    """sum of rows[0], rows[1], ... taken one after the other in fp32"""
    s = torch.zeros_like(rows[0])
    for r in rows:
        s = s + r
    return s


def _seq_scatter(idx, g, nrows):
    """table gradient: sample b adds g[b, token] to row idx[b, token]; rows of one sample are distinct (one per column)"""
    d = torch.zeros(nrows, g.shape[-1])
    for b in range(g.shape[0]):
        d[idx[b]] = d[idx[b]] + g[b]
    return d


def tab_seq32(c):
    x = tab_inputs(c)
    ncat, g = len(c.cards), x["g"]
    p = {k: x[k] for k in ("emb", "con_w", "con_b", "cls", "colemb") if k in x}
    r = {"out": tab_forward(c, x, p, torch.float32)}
    r["d_colemb"] = _seq(g)
    r["d_cls"] = r["d_colemb"][0].clone()
    if ncat:
        r["d_emb"] = _seq_scatter(table_index(x, False), g[:, 1:1 + ncat], x["emb"].shape[0])
    if c.ncon:
        tmpw = _seq(g[:, 1 + ncat:] * x["x"][:, ncat:, None])
        r["d_con_w"], r["d_con_b"] = _seq(tmpw), _seq(r["d_colemb"][1 + ncat:])
    return r


def saint_seq32(c):
    x = saint_inputs(c)
    ncat, g = len(c.cards), x["g"][:, :len(c.cards) + 1]
    r = {"out": saint_forward(c, x, {"emb": x["emb"], "pos": x["pos"]}, torch.float32)}
    r["d_emb"] = _seq_scatter(table_index(x, True), g, x["emb"].shape[0])
    r["d_pos"] = torch.zeros_like(x["pos"])
    r["d_pos"][:ncat + 1] = _seq(g)
    return r


def mlp_seq32(c):
    x = mlp_inputs(c)
    r = {"out": mlp_forward(c, x, {k: x[k] for k in MLP_PARAMS}, torch.float32)}
    r.update({"d_" + k: [] for k in MLP_PARAMS})
    for j in range(c.ncon):
        xv, gb, w1, b1, W2 = x["x"][:, x["con_cols"][j].item()], x["g"][:, c.ncat + 1 + j], x["w1"][j], x["b1"][j], x["W2"][j]
        hv = torch.relu(xv[:, None] * w1 + b1)
        dh = (gb @ W2) * (hv > 0)
        r["d_w1"].append(_seq(dh * xv[:, None]))
        r["d_b1"].append(_seq(dh))
        r["d_W2"].append(_seq(gb[:, :, None] * hv[:, None, :]))
        r["d_b2"].append(_seq(gb))
    return r


SEQ32 = {"tab": tab_seq32, "saint": saint_seq32, "mlp": mlp_seq32}


# ------------------------------------------------------------------------------------------------------------ comparing
def ratio(a, b, tol):
    """worst error of `a` over the allowance close() gives it against `b`: at most 1 exactly where close(a, b, tol) passes"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if not b.numel():
        return 0.0
    scale = float(b.abs().max())
    r = ((a - b).abs() / (tol * (1.0 + b.abs() + scale))).max()
    return float("inf") if torch.isnan(r) else float(r)


def pairs(got, ref, pre=None):
    """(name, got tensor, expected tensor) over a result dictionary whose values are tensors or per-column lists; with `pre`
    (the prefill of an accumulating call, keyed pre_<name>) the expectation of every gradient is prefill + gradient"""
    for k, v in ref.items():
        if k not in got:
            continue
        gl, rl = (got[k], v) if isinstance(v, list) else ([got[k]], [v])
        pl = [None] * len(rl) if pre is None or k == "out" else (pre["pre_" + k] if isinstance(v, list) else [pre["pre_" + k]])
        for j, (a, b, q) in enumerate(zip(gl, rl, pl)):
            yield (f"{k}[{j}]" if isinstance(v, list) else k), a, (b if q is None else q.double() + b)


# -------------------------------------------------------------- the reference as a subtly wrong kernel would compute it
def broken(family, c, bug):
    """float64 result dictionary with one defect, or None where the defect cannot show on this case"""
    x, ref = INPUTS[family](c), REFERENCE[family](c)
    out = {k: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for k, v in ref.items()}
    if bug == "row_dropped":                       # one batch row missing from one table row's sum
        if family == "mlp" or "emb" not in x:
            return None
        idx = table_index(x, family == "saint")
        tok0 = 1 if family == "tab" else 0
        out["d_emb"][idx[c.B // 2, -1]] -= x["g"][c.B // 2, tok0 + idx.shape[1] - 1].double()
        return out
    if bug == "offsets_swapped":                   # two columns look their codes up in each other's rows
        if family == "mlp" or x["offs"].numel() < 2:
            return None
        offs = x["offs"].clone()
        offs[-1], offs[-2] = x["offs"][-2], x["offs"][-1]
        fwd, names = (tab_forward, ("emb", "con_w", "con_b", "cls", "colemb")) if family == "tab" else (saint_forward, ("emb", "pos"))
        p = {k: x[k].double() for k in names if k in x}
        out["out"] = fwd(c, x, p, torch.float64, offs=offs)
        return out
    if bug == "relu_ge":
        if family != "mlp" or not c.bwd:
            return None
        out.update(mlp_manual_grads(c, x, ge=True))
        return out
    if bug == "tok0_off_by_one":                   # every continuous token one place to the right, the last one lost
        if family != "mlp" or c.ncon < 2:
            return None
        out["out"] = torch.cat([torch.full_like(ref["out"][:, :1], SENT), ref["out"][:, :-1]], 1)
        return out
    raise ValueError(bug)
