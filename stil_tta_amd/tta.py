"""Test-time adaptation in STiLModel.test_step (the TODO of STiLModel.py:523-524): TENT (Wang et al., ICLR 2021), EATA (Niu et
al., ICML 2022), SHOT-IM (Liang et al., ICML 2020), MEMO's marginal entropy over augmented views (Zhang et al., NeurIPS 2022),
DeYO's entropy-and-PLPD selection on a patch-shuffled second view (Lee et al., ICLR 2024), SAR's sharpness-aware two-pass
entropy steps with model recovery (Niu et al., ICLR 2023), READ's confidence-aware adaptation of the fusion attention with the
encoders frozen (Yang et al., ICLR 2024) and the forward-only "bn_adapt" baseline, optionally under a source-statistics BatchNorm
prior (tta_bn_prior).

Every method but SAR and READ is ONE adapting pass (`adapting_pass`) with its own loss and whatever follows the backward:
    tent_step              entropy           -> Adam over A
    eata_step              eata_entropy      -> Fisher anchor (when an estimate is loaded) -> Adam over A gated by n > 0
    shot_im_step           infomax           -> Adam over A
    marginal_entropy_step  marginal_entropy on V views of every sample (make_views) -> Adam over A -> the forward of
                           bn_adapt_step on the clean batch: the one method whose scores come after the update
    deyo_step              the forward of bn_adapt_step on the patch-shuffled images (patch_shuffle), then deyo_entropy on the
                           clean batch -> Adam over A gated by n > 0
    sar_step               sar_entropy -> A + rho g / |g| -> sar_entropy again on the rows the first pass kept -> A restored ->
                           Adam over A gated by n > 0 -> recovery of A when the running mean of the loss falls below tta_sar_reset
    read_step              its own pass (`fusion_pass`): the encoders in eval mode under no_grad, then the fusion layers and heads
                           under grad with read_loss -> Adam over A = the last fusion layer's qkv weight and bias (tta_params "fusion")
    cgpl_step              the pass with all three heads' logits kept: cgpl_loss (STiL's own consensus pseudo-labels over out_m, out_i,
                           out_t, smoothed by the prototypes) -> Adam over A gated by n > 0
    roid_step              roid_loss (ROID, Marsden et al., WACV 2024: the soft likelihood ratio of the rows a diversity selection keeps,
                           weighted by certainty and diversity) -> Adam over A -> A pulled a fixed fraction of the way back to its
                           source values (weight ensembling); the reported scores are corrected by the batch's prior, forward only
    rotta_step             RoTTA (Yuan et al., CVPR 2023; as recalled: unpinned): the EMA teacher scores the batch and decides, by
                           pseudo-label, age and uncertainty, which samples enter a category-balanced bank held on the device
                           (`RottaState`); the pass then runs on the augmented BANK, not the batch, with rotta_loss against the
                           teacher's logits of the bank -> Adam over A gated by n > 0 -> the teacher moves tta_rotta_nu towards A
    estimate_fisher        argmax_ce         -> fisher += g^2 / N
    bn_adapt_step          the pass's forward alone under no_grad, softmax_rows: no state, no gradient
    lame_step              LAME (Boudiaf et al., CVPR 2022; as recalled: unpinned): test_step's own forward in eval mode (with tta_bn_prior
                           or tta_bn_momentum: bn_adapt_step's), then lame_correct on the logits and the multimodal classifier's input:
                           the batch's probabilities are pulled together along a k-nearest-neighbour graph of the features (`lame_correct`);
                           the one method that touches only the outputs: no state, no gradient, nothing of the model moves
    dua_step               encoder_imaging alone on V views of every sample under no_grad, which moves the BatchNorm memory by alpha_t
                           (DUA, Mirza et al., CVPR 2022) -> the clean batch scored in eval mode on the memory: no gradient
With tta_bn_momentum every forward above normalises on the BatchNorm memory (`BnMemory`, model._bn_mem: a running estimate of the
target statistics in RoTTA's manner, Yuan et al., CVPR 2023) in place of the checkpoint's statistics: all forwards of a batch read
the same estimate, exactly one of them writes the update, and the step commits it at its end.
A = the adapted set (`param_names`); the state of an adapting model (`TentState` / `EataState` / `DeyoState` / `SarState` / `CgplState` / `RoidState` / `RottaState`) lives in
`model._tent`, and with it the augmenter of marginal_entropy_step's and rotta_step's views (`TentState.views`) and the generator of deyo_step's
shuffles (`DeyoState.rng`).
Adaptation is rank-local (no collectives) and composes no launch of the training step."""
from __future__ import annotations

import contextlib
import math
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import lib
from .flat import ALIGN, FlatState, _round_up
from .ops import _chk, _p, _scale_by, _stream, join_side

PARAMS = ("bn", "norm", "fusion")
VIEW_POLICIES = ("contrastive", "hard_eval", "soft_eval", "weak", "strong")   # augment._policy's transform families
ROTTA_MAX_SLOTS = 4096   # STIL_ROTTA_MAX_SLOTS of csrc/stil_rotta.h: the one workgroup that walks the samples bounds the bank
LAME_MAX_ROWS = 2048     # STIL_LAME_MAX_ROWS of csrc/stil_lame.h: a row's distances are ranked in the LDS of its workgroup
LAME_AFFINITIES = ("knn", "rbf")   # STIL_LAME_KNN, STIL_LAME_RBF: the index is the kind stil_lame_affinity takes


def _number(hp, key, lo=None, strict=False, also=()):
    """hp.<key> must be one of `also` (None, False) or a finite number (no bool), not below `lo` when one is given (`strict`:
    above it)"""
    v = getattr(hp, key)
    if any(v is a for a in also):
        return
    ok = not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)
    if not ok or (lo is not None and (v <= lo if strict else v < lo)):
        bound = "" if lo is None else f" {'>' if strict else '>='} {lo}"
        raise ValueError(f"{key} must be {', '.join(map(str, also)) + ' or ' if also else ''}a finite number{bound}, not {v!r}")


def _int_from(hp, key, lo):
    v = getattr(hp, key)
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError(f"{key} must be an int >= {lo}, not {v!r}")


def check_hparams(hp):
    if hp.tta_method not in METHODS:
        raise ValueError(f"Unknown tta_method {hp.tta_method!r}: valid are {METHODS}")
    if hp.tta_params not in PARAMS:
        raise ValueError(f"Unknown tta_params {hp.tta_params!r}: valid are {PARAMS}")
    _number(hp, "tta_bn_prior", 0, also=(None,))
    _number(hp, "tta_div_weight", 0)
    _number(hp, "tta_div_eps", 0, strict=True)
    _int_from(hp, "tta_views", 1)
    if not isinstance(hp.tta_view_policy, str) or hp.tta_view_policy not in VIEW_POLICIES:
        raise ValueError(f"Unknown tta_view_policy {hp.tta_view_policy!r}: valid are {VIEW_POLICIES}")
    _int_from(hp, "tta_view_seed", 0)   # the generator takes no negative seed
    g = hp.tta_patch_grid
    if isinstance(g, bool) or not isinstance(g, int) or g < 1 or hp.img_size % g != 0:
        raise ValueError(f"tta_patch_grid must be an int >= 1 that divides img_size = {hp.img_size}, not {g!r}")
    _number(hp, "tta_ent_margin", also=(None,))
    _number(hp, "tta_plpd_margin")
    _number(hp, "tta_reweight_ent", 0)
    _number(hp, "tta_reweight_plpd", 0)
    _int_from(hp, "tta_shuffle_seed", 0)
    _number(hp, "tta_sar_rho", 0)
    _number(hp, "tta_sar_reset", 0, strict=True, also=(None, False))   # True is refused: False alone switches recovery off
    _number(hp, "tta_bn_momentum", 0, strict=True, also=(None,))
    _number(hp, "tta_bn_momentum_decay", 0, strict=True)
    _number(hp, "tta_bn_momentum_min", 0)
    for key, v in (("tta_bn_momentum", hp.tta_bn_momentum), ("tta_bn_momentum_decay", hp.tta_bn_momentum_decay), ("tta_bn_momentum_min", hp.tta_bn_momentum_min)):
        if v is not None and v > 1:
            raise ValueError(f"{key} must not exceed 1, not {v!r}")
    _number(hp, "tta_read_gamma", 0, strict=True, also=(None,))
    if hp.tta_read_gamma is not None and hp.tta_read_gamma > 1:
        raise ValueError(f"tta_read_gamma must not exceed 1, not {hp.tta_read_gamma!r}")
    _number(hp, "tta_pl_threshold", 0, also=(None,))
    _number(hp, "tta_pl_rate", 0, also=(None,))
    if hp.tta_pl_rate is not None and hp.tta_pl_rate > 1:
        raise ValueError(f"tta_pl_rate must not exceed 1, not {hp.tta_pl_rate!r}")
    _int_from(hp, "tta_pl_seed", 0)
    _number(hp, "tta_roid_temperature", 0, strict=True)
    _number(hp, "tta_roid_src_momentum", 0)
    _number(hp, "tta_roid_clip", 0, strict=True)
    _number(hp, "tta_roid_eps", 0, strict=True)
    if hp.tta_roid_src_momentum > 1:
        raise ValueError(f"tta_roid_src_momentum must not exceed 1, not {hp.tta_roid_src_momentum!r}")
    if hp.tta_roid_clip >= 1:
        raise ValueError(f"tta_roid_clip must lie below 1, not {hp.tta_roid_clip!r}")
    if not isinstance(hp.tta_roid_prior_correction, bool):
        raise ValueError(f"tta_roid_prior_correction must be True or False, not {hp.tta_roid_prior_correction!r}")
    if hp.tta_method == "roid":   # the momentum of EATA's running mean, reused for ROID's: checked where ROID reads it
        _number(hp, "tta_probs_momentum", 0)
        if hp.tta_probs_momentum > 1:
            raise ValueError(f"tta_probs_momentum must not exceed 1, not {hp.tta_probs_momentum!r}")
    _int_from(hp, "tta_rotta_capacity", 1)
    _number(hp, "tta_rotta_nu", 0)
    _number(hp, "tta_rotta_lambda_t", 0)
    _number(hp, "tta_rotta_lambda_u", 0)
    if hp.tta_rotta_nu > 1:
        raise ValueError(f"tta_rotta_nu must not exceed 1, not {hp.tta_rotta_nu!r}")
    if hp.tta_rotta_capacity > ROTTA_MAX_SLOTS:
        raise ValueError(f"tta_rotta_capacity must not exceed {ROTTA_MAX_SLOTS}, the bound of stil_rotta_bank_update, not {hp.tta_rotta_capacity!r}")
    if not isinstance(hp.tta_lame_affinity, str) or hp.tta_lame_affinity not in LAME_AFFINITIES:
        raise ValueError(f"Unknown tta_lame_affinity {hp.tta_lame_affinity!r}: valid are {LAME_AFFINITIES}")
    _int_from(hp, "tta_lame_knn", 1)
    _number(hp, "tta_lame_lambda", 0)
    _int_from(hp, "tta_lame_steps", 1)
    _number(hp, "tta_lame_tol", 0)
    if hp.tta_method == "read" and hp.tta_params != "fusion":
        raise ValueError(f"tta_method 'read' adapts the fusion attention alone: set tta_params 'fusion' (this model: {hp.tta_params!r})")
    if hp.tta_params == "fusion" and hp.tta_method != "read":
        raise ValueError(f"tta_params 'fusion' is the adapted set of tta_method 'read' alone: set tta_method 'read' (this model: {hp.tta_method!r})")
    if hp.tta_method == "read":
        for key in ("tta_bn_prior", "tta_bn_momentum"):
            if getattr(hp, key) is not None:
                raise ValueError(f"tta_method 'read' keeps the encoders' normalisation at the source: {key} must be None, not {getattr(hp, key)!r}")
    if hp.tta_method == "dua" and hp.tta_bn_momentum is None:
        raise ValueError("tta_method 'dua' adapts the running estimate of the BatchNorm statistics alone: set tta_bn_momentum (DUA: 0.1)")
    if hp.tta_method == "rotta" and hp.tta_bn_momentum is None:
        raise ValueError("tta_method 'rotta' normalises on the running estimate of the BatchNorm statistics, its robust BatchNorm: set tta_bn_momentum (RoTTA: 0.05)")
    if hp.tta_method is not None and hp.tabular_encoder == "saint":
        raise NotImplementedError("test-time adaptation is not implemented for the SAINT tabular encoder")


def enabled(hp) -> bool:
    return bool(getattr(hp, "tta", False)) and hp.tta_method in METHODS[1:]


def param_names(model) -> List[str]:
    """The adapted set A, as state_dict names: weight and bias of every BatchNorm2d of model.encoder_imaging (downsample
    BNs included); with tta_params == "norm" also of every LayerNorm of model.encoder_tabular and model.transformer.
    With tta_params == "fusion" (READ): weight and bias of the Q/K/V projection of the LAST fusion layer, nothing else."""
    if model.hp.tta_params == "fusion":
        last = len(model.model.transformer) - 1
        return [f"model.transformer.{last}.attn.qkv.weight", f"model.transformer.{last}.attn.qkv.bias"]
    groups = [("model.encoder_imaging", model.model.encoder_imaging, nn.BatchNorm2d)]
    if model.hp.tta_params == "norm":
        groups += [("model.encoder_tabular", model.model.encoder_tabular, nn.LayerNorm), ("model.transformer", model.model.transformer, nn.LayerNorm)]
    out = []
    for prefix, root, kind in groups:
        for n, mod in root.named_modules():
            if isinstance(mod, kind):
                out += [f"{prefix}.{n}.weight", f"{prefix}.{n}.bias"]
    return out


# ---------------------------------------------------------------------------------------------- losses
class _RowLossFn(torch.autograd.Function):
    """The one autograd node of the losses below: launch(z) -> (loss, probabilities or None, dZ) makes the loss's single
    library call, which forms dZ in the same launch sequence; the probabilities carry no gradient and backward scales dZ by the
    incoming gradient.  Given further logit tensors after `launch`, launch takes the tuple of them all and returns one dZ per
    tensor."""

    @staticmethod
    def forward(ctx, z, launch, *more):
        if more:   # several logit tensors (cgpl_loss): launch((z, ...)) -> (loss, p, (dZ, ...)), one gradient per tensor
            loss, p, dzs = launch((z,) + more)
            ctx.save_for_backward(*dzs)
        else:
            loss, p, dz = launch(z)
            ctx.save_for_backward(dz)
        if p is not None:
            ctx.mark_non_differentiable(p)
        return loss, p

    @staticmethod
    def backward(ctx, g, _gp=None):
        dz, *more = ctx.saved_tensors
        return (_scale_by(dz, g), None) + tuple(_scale_by(d, g) for d in more)


def _empty(z, n, dtype, count=None):
    """-> one uninitialised [n] tensor of `dtype` on z's device, or a generator of `count` of them"""
    if count is None:
        return torch.empty((n,), dtype=dtype, device=z.device)
    return (torch.empty((n,), dtype=dtype, device=z.device) for _ in range(count))


def entropy(z):
    """TENT's loss (Wang et al., ICLR 2021): mean over rows of H(softmax(z)), H(p) = -sum_k p_k log p_k, for test-time
    adaptation in STiLModel.test_step (STiLModel.py:523-524).  The probabilities are the scores the step reports, so no
    separate softmax launch runs.  One launch forms lse, p, the row entropies and dZ / rows (stil_entropy_rows).
    -> (mean row entropy of softmax(z) [autograd], softmax(z) [no grad], {})"""
    def launch(z):
        _chk(z)
        R, K = z.shape
        lse, h = _empty(z, R, torch.float64), _empty(z, R, torch.float32)
        p, dz = torch.empty_like(z), torch.empty_like(z)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        lib().entropy_rows(_p(z), K, R, K, 1.0 / R, _p(lse), _p(p), K, _p(h), _p(dz), K, _p(loss), _stream())
        return loss, p, dz

    return _RowLossFn.apply(z.contiguous(), launch) + ({},)


def eata_entropy(z, e_margin, d_margin, momentum, m, m_valid, active=None, gate=None):
    """EATA's loss (Niu et al., ICML 2022) beside entropy: (1/n) sum over the selected rows of w_r H_r, the selection
    (reliable: H_r < e_margin; non-redundant: |cos(m, p_r)| < d_margin), the weights w_r = exp(e_margin - H_r), the update of
    the running mean m and the gate of the Adam step, all in stil_eata_rows: n stays on the device.  dZ is already divided by n
    (zero when n == 0); w carries no gradient.
    -> (EATA's weighted entropy of the selected rows [autograd], softmax(z) [no grad], info); updates m / m_valid / gate;
    info = dict(H, cos, w, rel, sel, counts [n, n_reliable, m valid before, -], lse)."""
    info = {}

    def launch(z):
        _chk(z, m, m_valid, active, gate)
        R, K = z.shape
        lse, hd = _empty(z, R, torch.float64, 2)
        h, c, w = _empty(z, R, torch.float32, 3)
        rel, sel = _empty(z, R, torch.uint8, 2)
        p, dz = torch.empty_like(z), torch.empty_like(z)
        counts = torch.zeros((4,), dtype=torch.int32, device=z.device)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        nt = 0 if active is None else active.numel()
        lib().eata_rows(_p(z), K, R, K, float(e_margin), float(d_margin), float(momentum), 1.0, _p(m), _p(m_valid), _p(lse), _p(hd), _p(p), K,
                        _p(h), _p(c), _p(w), _p(rel), _p(sel), _p(dz), K, _p(counts), _p(loss), _p(active), _p(gate), nt, _stream())
        info.update(H=h, cos=c, w=w, rel=rel, sel=sel, counts=counts, lse=lse)
        return loss, p, dz

    return _RowLossFn.apply(z.contiguous(), launch) + (info,)


def deyo_entropy(z, zs, ent_margin, plpd_margin, e0, a_ent=1.0, a_plpd=1.0, active=None, gate=None):
    """DeYO's loss (Lee et al., ICLR 2024) beside eata_entropy: (1/n) sum over the selected rows of w_r H_r, with z the logits
    of the batch and zs those of its patch-shuffled images (no gradient).  plpd_r = p_r[yhat_r] - softmax(zs_r)[yhat_r], yhat_r
    the first maximum of z_r; the selection (reliable: H_r < ent_margin; and plpd_r > plpd_margin), the weights w_r =
    a_ent exp(e0 - H_r) + a_plpd exp(plpd_r) and the gate of the Adam step, all in stil_deyo_rows: n stays on the device.
    dZ is already divided by n (zero when n == 0); w carries no gradient.
    -> (DeYO's weighted entropy of the selected rows [autograd], softmax(z) [no grad], info); updates gate;
    info = dict(H, plpd, w, yhat, rel, sel, counts [n, n_reliable, 0, 0], lse)."""
    info = {}
    zs = zs.detach().contiguous()

    def launch(z):
        _chk(z, zs, active, gate)
        R, K = z.shape
        if tuple(zs.shape) != (R, K):
            raise ValueError(f"deyo_entropy: logits {tuple(z.shape)} against shuffled logits {tuple(zs.shape)}")
        lse, hd, wd = _empty(z, R, torch.float64, 3)
        h, d, w = _empty(z, R, torch.float32, 3)
        yhat = _empty(z, R, torch.int32)
        rel, sel = _empty(z, R, torch.uint8, 2)
        p, dz = torch.empty_like(z), torch.empty_like(z)
        counts = torch.empty((4,), dtype=torch.int32, device=z.device)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        nt = 0 if active is None else active.numel()
        lib().deyo_rows(_p(z), K, _p(zs), K, R, K, float(ent_margin), float(plpd_margin), float(e0), float(a_ent), float(a_plpd), 1.0,
                        _p(lse), _p(hd), _p(wd), _p(p), K, _p(h), _p(d), _p(w), _p(yhat), _p(rel), _p(sel), _p(dz), K, _p(counts),
                        _p(loss), _p(active), _p(gate), nt, _stream())
        info.update(H=h, plpd=d, w=w, yhat=yhat, rel=rel, sel=sel, counts=counts, lse=lse)
        return loss, p, dz

    return _RowLossFn.apply(z.contiguous(), launch) + (info,)


def sar_entropy(z, margin, prior=None, active=None, gate=None, ema=None, ema_valid=None, momentum=0.9, reset=0.0, recover=None):
    """SAR's loss (Niu et al., ICLR 2023) beside eata_entropy: (1/n) sum over the selected rows of H_r, unweighted; a row is
    selected when H_r < margin and, in the second pass, the first pass selected it too (`prior`, its `sel`).  With `ema` (the
    second pass) the running mean of the loss (ema, ema_valid) and the recovery flag (reset <= 0: never raised) are updated as
    well, all in stil_sar_rows: n, the gate of the Adam step and the recovery decision stay on the device.  dZ is already
    divided by n (zero when n == 0).
    -> (the mean entropy of the selected rows [autograd], softmax(z) [no grad], info); updates gate;
    info = dict(H, sel, counts [n, rows with H < margin, rows the prior admits, 0], lse)."""
    info = {}

    def launch(z):
        _chk(z, prior, active, gate, ema, ema_valid, recover)
        R, K = z.shape
        if prior is not None and (prior.dtype != torch.uint8 or prior.numel() != R):
            raise ValueError(f"sar_entropy: a prior selection of {prior.numel()} {prior.dtype} entries for {R} rows")
        lse, hd = _empty(z, R, torch.float64, 2)
        h, sel = _empty(z, R, torch.float32), _empty(z, R, torch.uint8)
        p, dz = torch.empty_like(z), torch.empty_like(z)
        counts = torch.empty((4,), dtype=torch.int32, device=z.device)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        nt = 0 if active is None else active.numel()
        lib().sar_rows(_p(z), K, R, K, float(margin), 1.0, _p(prior), _p(lse), _p(hd), _p(p), K, _p(h), _p(sel), _p(dz), K, _p(counts),
                       _p(loss), _p(active), _p(gate), nt, _p(ema), _p(ema_valid), float(momentum), float(reset), _p(recover), _stream())
        info.update(H=h, sel=sel, counts=counts, lse=lse)
        return loss, p, dz

    return _RowLossFn.apply(z.contiguous(), launch) + (info,)


def patch_shuffle(x, grid, perm):
    """DeYO's second view of the images x [B, C, H, W] (float32, on the device): every image cut into grid x grid patches and
    patch slot s (row-major) filled with source patch perm[b, s], every channel alike (stil_patch_shuffle: a bit-exact copy).
    perm: [B, grid^2] integers, a host array (numpy / CPU tensor: staged through pinned memory, no blocking copy) or an int32
    device tensor; an entry outside [0, grid^2) leaves its slot in place.  -> the shuffled images (a new tensor)"""
    _chk(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"patch_shuffle: images must be float32 [B, C, H, W], not {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    B, C, H, W = x.shape
    grid = int(grid)
    if grid < 1 or H % grid or W % grid:
        raise ValueError(f"patch_shuffle: grid = {grid} must divide H = {H} and W = {W}")
    if not torch.is_tensor(perm):
        perm = torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int32))
    if tuple(perm.shape) != (B, grid * grid):
        raise ValueError(f"patch_shuffle: perm of shape {tuple(perm.shape)} for {B} images of {grid * grid} patches")
    if perm.device != x.device:
        perm = perm.to(torch.int32).contiguous().pin_memory().to(x.device, non_blocking=True)
    elif perm.dtype != torch.int32 or not perm.is_contiguous():
        perm = perm.to(torch.int32).contiguous()
    out = torch.empty_like(x)
    lib().patch_shuffle(_p(x), _p(out), B, C, H, W, grid, _p(perm), _stream())
    return out


def infomax(z, div_weight=1.0, eps=1e-5):
    """SHOT's information-maximisation loss (Liang et al., ICML 2020) beside entropy: mean row entropy of softmax(z) plus
    div_weight x D, D = sum_k pbar_k log(pbar_k + eps) with pbar the batch mean of the rows' softmax (minus the entropy of the
    marginal: it penalises the batch that predicts one class everywhere).  stil_infomax_rows forms lse, p, the row entropies,
    pbar, D and dZ / rows; the gradient couples the rows through pbar.  With div_weight == 0 loss, probabilities and dZ are
    entropy's bit for bit.
    -> (mean row entropy + div_weight x D of softmax(z) [autograd], softmax(z) [no grad], info);
    info = dict(loss_entropy, loss_diversity, marginal [K], H, lse), all on the device."""
    info = {}

    def launch(z):
        _chk(z)
        R, K = z.shape
        lse, h, pbar = _empty(z, R, torch.float64), _empty(z, R, torch.float32), _empty(z, K, torch.float32)
        p, dz = torch.empty_like(z), torch.empty_like(z)
        out = _empty(z, 3, torch.float32)
        ws = _empty(z, 2 * K + R, torch.float64)
        lib().infomax_rows(_p(z), K, R, K, 1.0 / R, float(div_weight), float(eps), _p(lse), _p(p), K, _p(h), _p(pbar), _p(dz), K,
                           _p(out), _p(ws), _stream())
        info.update(loss_entropy=out[1], loss_diversity=out[2], marginal=pbar, H=h, lse=lse)
        return out[0], p, dz

    return _RowLossFn.apply(z.contiguous(), launch) + (info,)


def read_gamma(hp) -> float:
    """tta_read_gamma resolved: None -> exp(-1), where the row loss is -c ln c"""
    return math.exp(-1.0) if hp.tta_read_gamma is None else float(hp.tta_read_gamma)


def read_loss(z, gamma=math.exp(-1.0), div_weight=1.0, eps=1e-5):
    """READ's loss (Yang et al., ICLR 2024; form and constants as recalled: unpinned) beside infomax: the mean over rows of
    f_r = c_r log(e gamma / c_r), c_r = softmax(z_r)[yhat_r] the confidence and yhat_r the first maximum of z_r, plus
    div_weight x D, infomax's batch-balance term.  df/dc = ln(gamma / c): minimising f raises the confidence of the rows above
    gamma and lowers that of the rows below (the noisy ones); gamma = 1/e gives f = -c ln c.  stil_read_rows forms lse, p, yhat,
    c, f, pbar, D and dZ / rows (yhat held fixed); pbar and D are stil_infomax_rows' bit for bit.
    -> (mean f + div_weight x D [autograd], softmax(z) [no grad], info);
    info = dict(loss_confidence, loss_balance, marginal [K], yhat [int32], conf, f, lse), all on the device."""
    info = {}

    def launch(z):
        _chk(z)
        R, K = z.shape
        lse, pbar = _empty(z, R, torch.float64), _empty(z, K, torch.float32)
        conf, f = _empty(z, R, torch.float32, 2)
        yhat = _empty(z, R, torch.int32)
        p, dz = torch.empty_like(z), torch.empty_like(z)
        out = _empty(z, 3, torch.float32)
        ws = _empty(z, 2 * K, torch.float64)
        lib().read_rows(_p(z), K, R, K, 1.0 / R, float(gamma), float(div_weight), float(eps), _p(lse), _p(p), K, _p(yhat), _p(conf),
                        _p(f), _p(pbar), _p(dz), K, _p(out), _p(ws), _stream())
        info.update(loss_confidence=out[1], loss_balance=out[2], marginal=pbar, yhat=yhat, conf=conf, f=f, lse=lse)
        return out[0], p, dz

    return _RowLossFn.apply(z.contiguous(), launch) + (info,)


def cgpl_rate(hp) -> float:
    """tta_pl_rate resolved: None -> rate_pseudo, the weight of the consensus label against the prototype classifier's"""
    return float(hp.rate_pseudo if hp.tta_pl_rate is None else hp.tta_pl_rate)


def cgpl_threshold(hp) -> float:
    """tta_pl_threshold resolved: None -> th1"""
    return float(hp.th1 if hp.tta_pl_threshold is None else hp.tta_pl_threshold)


def cgpl_loss(zm, zi, zt, feat, protos, coin, rate, T, th, active=None, gate=None):
    """STiL's own loss on unlabelled rows (STiLModel.py:255-303 with use_ema False) beside eata_entropy, on the logits of the
    three heads: the case of every row from which heads agree on the first maximum (1: all three; 2_i: multimodal and imaging;
    2_t: multimodal and tabular; 3: otherwise), the pseudo-label q = rate softmax(mean logits of the agreeing heads) + (1 - rate)
    softmax(feat . protos^T / T), the confidence max_k (rate softmax(zm) + (1 - rate) tp) >= th, and per head the soft
    cross-entropy -sum_k q_k log softmax(z_h)_k over the rows its case assigns to it (multimodal: case 1; imaging: 1, 2_t, 3 with
    coin; tabular: 1, 2_i, 3 without), each summed and divided by ALL rows; q carries no gradient.  All in stil_cgpl_rows: n and the
    gate of the Adam step stay on the device.  feat (the normalised multimodal projection) and protos may be None when rate == 1.
    -> (the sum of the three losses [autograd w.r.t. zm, zi, zt], softmax(zm) [no grad], info); updates gate;
    info = dict(loss_m, loss_i, loss_t, pseudo_label, conf, flags [rows, 4: case 1..4, mask1, mask1, 0], ce3, counts [n, case 1,
    2_i, 2_t, 3], lse3)."""
    info = {}
    rate = float(rate)
    smooth = rate < 1.0
    if smooth:
        if feat is None or protos is None:
            raise ValueError(f"cgpl_loss: rate = {rate} < 1 needs the projection and the prototypes")
        feat, protos = feat.detach().contiguous(), protos.detach().contiguous()

    def launch(zs):
        zm, zi, zt = zs
        _chk(zm, zi, zt, coin, active, gate, *((feat, protos) if smooth else ()))
        R, K = zm.shape
        if tuple(zi.shape) != (R, K) or tuple(zt.shape) != (R, K):
            raise ValueError(f"cgpl_loss: logits of shapes {tuple(zm.shape)}, {tuple(zi.shape)}, {tuple(zt.shape)}")
        if coin.dtype != torch.uint8 or coin.numel() != R:
            raise ValueError(f"cgpl_loss: {coin.numel()} {coin.dtype} coins for {R} rows")
        Dp = 1
        if smooth:
            Dp = feat.shape[1]
            if tuple(feat.shape) != (R, Dp) or tuple(protos.shape) != (K, Dp):
                raise ValueError(f"cgpl_loss: projection {tuple(feat.shape)} against prototypes {tuple(protos.shape)} for {R} rows of {K} classes")
        dev = zm.device
        lse3 = torch.empty((3, R), dtype=torch.float64, device=dev)
        ce3 = torch.empty((3, R), dtype=torch.float32, device=dev)
        p, q = torch.empty_like(zm), torch.empty_like(zm)
        dzs = tuple(torch.empty_like(zm) for _ in range(3))
        conf = _empty(zm, R, torch.float32)
        flags = torch.empty((R, 4), dtype=torch.uint8, device=dev)
        counts = torch.empty((5,), dtype=torch.int32, device=dev)
        out = _empty(zm, 4, torch.float32)
        ws = _empty(zm, R * K, torch.float64) if smooth else None
        nt = 0 if active is None else active.numel()
        lib().cgpl_rows(_p(zm), _p(zi), _p(zt), K, _p(feat) if smooth else None, _p(protos) if smooth else None, _p(coin), R, K, Dp,
                        float(T), rate, float(th), 1.0 / R, _p(lse3), _p(p), _p(q), K, _p(conf), _p(flags), _p(ce3), _p(dzs[0]), _p(dzs[1]),
                        _p(dzs[2]), K, _p(counts), _p(out), _p(active), _p(gate), nt, _p(ws), _stream())
        info.update(loss_m=out[1], loss_i=out[2], loss_t=out[3], pseudo_label=q, conf=conf, flags=flags, ce3=ce3, counts=counts, lse3=lse3)
        return out[0], p, dzs

    return _RowLossFn.apply(zm.contiguous(), launch, zi.contiguous(), zt.contiguous()) + (info,)


def roid_loss(z, ema, tau=1.0 / 3.0, clip=0.99, eps=1e-5, momentum=0.9, correct=True):
    """ROID's loss (Marsden, Doebler, Yang, WACV 2024; definition as recalled: unpinned) beside eata_entropy: (1/rows) sum over the
    kept rows of w_r slr_r, slr_r = -sum_k q_k log(q_k / (1 - q_k) + eps) the soft likelihood ratio of q = min(softmax(z_r), clip).
    With d_r = 1 - cos(softmax(z_r), ema) (diversity against the running mean prediction `ema` [K], read as it stands before the
    call) and c_r = -H_r (certainty), both min-max normalised over the batch to dn, cn (a range <= 1e-9 gives 0 for every row: this
    project's rule), a row is kept unless dn_r lies below the batch mean of dn, and w_r = exp(dn_r cn_r / tau); keep and w carry no
    gradient.  Then ema <- momentum ema + (1 - momentum) pbar, pbar the batch-mean prediction over all rows, and with `correct` the
    scores are softmax(z) reweighted by the prior s (from pbar, smoothed) and renormalised.  All in stil_roid_rows: nothing is read back.
    -> (the weighted soft likelihood ratio [autograd], the corrected scores or with correct False softmax(z) [no grad], info);
    updates ema; info = dict(H, cos, dn, cn, w, keep, slr, counts [kept, rows, d range degenerate, c range degenerate], pbar, prior,
    probs, lse)."""
    info = {}

    def launch(z):
        _chk(z, ema)
        R, K = z.shape
        if ema.dtype != torch.float32 or ema.numel() != K or not ema.is_contiguous():
            raise ValueError(f"roid_loss: a running mean of {ema.numel()} {ema.dtype} entries for {K} classes")
        lse = _empty(z, R, torch.float64)
        h, c, slr, dn, cn, w = _empty(z, R, torch.float32, 6)
        keep = _empty(z, R, torch.uint8)
        pbar, prior = _empty(z, K, torch.float32, 2)
        p, dz = torch.empty_like(z), torch.empty_like(z)
        scores = torch.empty_like(z) if correct else None
        counts = torch.empty((4,), dtype=torch.int32, device=z.device)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        ws = _empty(z, 4 * R + 2 * K, torch.float64)
        lib().roid_rows(_p(z), K, R, K, _p(ema), float(tau), float(clip), float(eps), float(momentum), 1.0, int(bool(correct)), _p(lse),
                        _p(p), K, _p(h), _p(c), _p(slr), _p(dn), _p(cn), _p(w), _p(keep), _p(pbar), _p(prior), _p(scores), K, _p(dz), K,
                        _p(counts), _p(loss), _p(ws), _stream())
        info.update(H=h, cos=c, dn=dn, cn=cn, w=w, keep=keep, slr=slr, counts=counts, pbar=pbar, prior=prior, probs=p, lse=lse)
        return loss, (scores if correct else p), dz

    return _RowLossFn.apply(z.contiguous(), launch) + (info,)


def rotta_loss(z, zt, label, age, active=None, gate=None):
    """RoTTA's loss on the bank (Yuan, Xie, Li, CVPR 2023; definition as recalled: unpinned) beside eata_entropy: z the student's
    logits of the N slots (on their augmented images), zt the teacher's (no gradient), label [N] int32 (-1: an empty slot) and age [N]
    int32 the bank's bookkeeping.  With n the number of filled slots, loss = (1/n) sum over them of w_i CE(softmax(zt_i), softmax(z_i)),
    w_i = e_i / (1 + e_i), e_i = exp(-age_i / N) the timeliness weight; dZ = w_i (softmax(z_i) - softmax(zt_i)) / n, exactly 0 on an
    empty slot; with n == 0 loss and dZ are 0 and the gate closes.  All in stil_rotta_rows: n and the gate of the Adam step stay on
    the device.
    -> (the weighted cross-entropy [autograd], None, info); updates gate; info = dict(ce, w, counts [n, N, 0, 0])."""
    info = {}
    zt = zt.detach().contiguous()

    def launch(z):
        _chk(z, zt, label, age, active, gate)
        R, K = z.shape
        if tuple(zt.shape) != (R, K):
            raise ValueError(f"rotta_loss: student logits {tuple(z.shape)} against teacher logits {tuple(zt.shape)}")
        for name, t in (("label", label), ("age", age)):
            if t.dtype != torch.int32 or t.numel() != R or not t.is_contiguous():
                raise ValueError(f"rotta_loss: {name} of {t.numel()} {t.dtype} entries for {R} slots")
        ce, w = _empty(z, R, torch.float32, 2)
        dz = torch.empty_like(z)
        counts = torch.empty((4,), dtype=torch.int32, device=z.device)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        ws = _empty(z, 4 * R, torch.float64)
        nt = 0 if active is None else active.numel()
        lib().rotta_rows(_p(z), K, _p(zt), K, _p(label), _p(age), R, K, 1.0, _p(ce), _p(w), _p(dz), K, _p(counts), _p(loss), _p(active),
                         _p(gate), nt, _p(ws), _stream())
        info.update(ce=ce, w=w, counts=counts)
        return loss, None, dz

    return _RowLossFn.apply(z.contiguous(), launch) + (info,)


def lame_correct(z, feats, k=5, kind="knn", lam=1.0, max_steps=100, tol=1e-8):
    """LAME's correction (Boudiaf, Mueller, Ben Ayed, Bertinetto, CVPR 2022, "Parameter-free Online Test-time Adaptation"; definition
    and defaults as recalled from the paper and its published code: unpinned) of the logits z [rows, K] of one batch along the
    features feats [rows, D]; no autograd, nothing of the model is read.  With fhat the normalised features and d2 = 2 - 2 <fhat_i,
    fhat_j>, every row gets its k' = min(k, rows - 1) nearest other rows (ties to the lower index, a NaN distance last), weighted 1
    ("knn") or exp(-d2 / (2 s2)) ("rbf", s2 the mean distance to the k'-th neighbour); A = (W + W^T) / 2; then from
    u = log(softmax(z) + 1e-10) and Y^0 = softmax(u) the Jacobi iteration Y^n_i = softmax(u_i + lam sum_j A_ij Y^(n-1)_j) runs until
    its energy moves by no more than tol relatively (after step 2 at the earliest; tol 0: never) or max_steps steps are done.  The
    stopping rule is decided on the device: all 3 + 2 + max_steps + 1 launches of stil_lame_affinity and stil_lame_rows (csrc/stil_lame.h
    states the arithmetic) are enqueued, those after the rule has fired return at once, nothing is read back.
    Unlike the published code, on purpose: all in double; the energy uses A Y^(n-1), what the update read; this project's tie and NaN
    rules; no "linear" affinity.
    -> (Y [rows, K] the corrected scores, p = softmax(z) in stil_entropy_rows' bits, info); info = dict(nbr [rows, k] int32 (-1: padding),
    wts [rows, k], dk [rows] float64, steps [1] int32, energy [max_steps] float64 (NaN from `steps` on), lse [rows] float64)."""
    z, feats = z.detach().contiguous(), feats.detach().contiguous()
    _chk(z, feats)
    if z.dim() != 2 or feats.dim() != 2 or feats.shape[0] != z.shape[0] or z.dtype != torch.float32 or feats.dtype != torch.float32:
        raise ValueError(f"lame_correct: float32 logits [rows, K] and features [rows, D], not {tuple(z.shape)} {z.dtype} and {tuple(feats.shape)} {feats.dtype}")
    R, K = z.shape
    D = feats.shape[1]
    if R > LAME_MAX_ROWS:
        raise ValueError(f"lame_correct: a batch of {R} rows exceeds LAME_MAX_ROWS = {LAME_MAX_ROWS}, the bound of stil_lame_affinity")
    if kind not in LAME_AFFINITIES:
        raise ValueError(f"lame_correct: unknown affinity {kind!r}: valid are {LAME_AFFINITIES}")
    if isinstance(k, bool) or not isinstance(k, int) or k < 1 or isinstance(max_steps, bool) or not isinstance(max_steps, int) or max_steps < 1:
        raise ValueError(f"lame_correct: k and max_steps must be ints >= 1, not {k!r} and {max_steps!r}")
    dev = z.device
    nbr = torch.empty((R, k), dtype=torch.int32, device=dev)
    wts = torch.empty((R, k), dtype=torch.float32, device=dev)
    dk, lse = _empty(z, R, torch.float64, 2)
    ws = _empty(z, max(R * (1 + min(k, R)), 2 * R * R + 3 * R * K + 3 * R + 2), torch.float64)   # the two calls are ordered: one scratch
    lib().lame_affinity(_p(feats), D, R, D, k, LAME_AFFINITIES.index(kind), _p(nbr), _p(wts), _p(dk), _p(ws), _stream())
    p, Y = torch.empty_like(z), torch.empty_like(z)
    energy = torch.full((max_steps,), float("nan"), dtype=torch.float64, device=dev)
    steps = torch.empty((1,), dtype=torch.int32, device=dev)
    lib().lame_rows(_p(z), K, R, K, _p(nbr), _p(wts), k, float(lam), max_steps, float(tol), _p(lse), _p(p), K, _p(Y), K, _p(energy),
                    _p(steps), _p(ws), _stream())
    return Y, p, dict(nbr=nbr, wts=wts, dk=dk, steps=steps, energy=energy, lse=lse)


def marginal_entropy(z, groups, views, want_probs=False):
    """MEMO's loss (Zhang, Levine, Finn, NeurIPS 2022) beside entropy: z holds `views` consecutive rows per sample (row g V + v is
    view v of sample g); the loss is the mean over the samples of the entropy of the sample's mean prediction over its views.
    stil_marginal_entropy_groups forms lse, the marginals (through a log-sum-exp over the views, never the logarithm of an
    underflowed mean), their entropies and dZ / groups.  With views == 1 it is entropy's loss.
    -> (mean over the samples of the entropy of the mean prediction over each sample's views [autograd],
    softmax(z) [no grad] when asked for or None, info); info = dict(marginal [G, K], marginal_entropy [G], lse), all on the device."""
    info = {}
    groups, views = int(groups), int(views)

    def launch(z):
        _chk(z)
        R, K = z.shape
        if R != groups * views:
            raise ValueError(f"marginal_entropy: {R} rows are not {groups} samples x {views} views")
        lse = _empty(z, R, torch.float64)
        p = torch.empty_like(z) if want_probs else None
        pbar = torch.empty((groups, K), dtype=torch.float32, device=z.device)
        hbar, out = _empty(z, groups, torch.float32), _empty(z, 1, torch.float32)
        dz = torch.empty_like(z)
        ws = _empty(z, groups * (K + (K + 255) // 256), torch.float64)
        lib().marginal_entropy_groups(_p(z), K, groups, views, K, 1.0 / groups, _p(lse), _p(p), K, _p(pbar), K, _p(hbar), _p(dz), K,
                                      _p(out), _p(ws), _stream())
        info.update(marginal=pbar, marginal_entropy=hbar, lse=lse)
        return out[0], p, dz

    return _RowLossFn.apply(z.contiguous(), launch) + (info,)


def argmax_ce(z):
    """-> (mean_r CE(z[r], argmax_k z[r]) (first maximum) [autograd], None, {}): the loss of the Fisher estimate"""
    R, K = z.shape
    onehot = torch.empty((R, K), dtype=torch.float32, device=z.device)
    mask = torch.empty((R,), dtype=torch.float32, device=z.device)
    idx = torch.empty((R,), dtype=torch.int32, device=z.device)
    lib().onehot_argmax(_p(z.detach()), R, K, 0.0, _p(onehot), _p(mask), _p(idx), _stream())
    return ops.CEHardFn.apply(z, idx.long()), None, {}


# ---------------------------------------------------------------------------------------------- state
class TentState:
    """Test-time adaptation state over the flat slab (TENT, Wang et al., ICLR 2021; STiLModel.test_step): the adapted set A
    (`names`, a subset of FlatState.names), its own gradient slab and Adam moments / step counts in the student slab's
    layout (stil_adam_step with `active` = A), and the source values of A.  The training slabs (FlatState._grads,
    exp_avg, exp_avg_sq, steps) are never written: during a pass every parameter's gradient slot points into this
    state's slab (`redirect`)."""

    def __init__(self, flat: FlatState, names: List[str]):
        self.flat = flat
        ids = [flat.names.index(n) for n in names]
        self.ids = ids
        self.tensors = [flat.tensors[i] for i in ids]
        dev = flat.params.device
        self.grads = torch.zeros(flat.total, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(flat.total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(flat.total, dtype=torch.float32, device=dev)
        self.steps = torch.zeros(len(flat.tensors), dtype=torch.int32, device=dev)
        act = torch.zeros(len(flat.tensors), dtype=torch.uint8)
        act[ids] = 1
        self.active = act.to(dev)
        base = flat._grads.data_ptr()
        self._slots = [self.grads[(t._gslot.data_ptr() - base) // 4:][:t.numel()].view(t.shape) for t in flat.tensors]
        self.source: Optional[List[torch.Tensor]] = None
        self.views = None   # marginal_entropy_step's ImageAugmenter: reset() leaves its generator running, drop() forgets it

    @torch.no_grad()
    def snapshot(self):
        self.source = [t.detach().clone() for t in self.tensors]

    @torch.no_grad()
    def reset(self):
        """A <- its source values (as it is before the first snapshot), and what a new episode clears: moments, step counts."""
        if self.source is not None:
            torch._foreach_copy_([t.data for t in self.tensors], self.source)
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.steps.zero_()

    @contextlib.contextmanager
    def redirect(self):
        """Gradient slots -> this state's (zeroed) slab for the duration; slots, `_stil_touched` flags restored after."""
        ts = self.flat.tensors
        saved = [(t._gslot, t._stil_touched) for t in ts]
        self.grads.zero_()
        for t, s in zip(ts, self._slots):
            t._gslot, t._stil_touched = s, False
        try:
            yield
        finally:
            join_side()
            for t, (g, touched) in zip(ts, saved):
                t._gslot, t._stil_touched = g, touched

    @torch.no_grad()
    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8, mask=None):
        """Adam over A, no weight decay.  mask: the per-tensor mask to step under instead of `active` (EATA's `gate`: with
        n == 0 neither A, nor its moments, nor its step counts move)."""
        f = self.flat
        lib().adam_step(_p(f.params), _p(self.grads), _p(self.exp_avg), _p(self.exp_avg_sq), _p(f.chunk2tensor), _p(self.steps),
                        _p(self.active if mask is None else mask), len(f.tensors), f.total, float(lr), float(betas[0]), float(betas[1]),
                        float(eps), 0.0, 1.0, _stream())


class CompactState(TentState):
    """TentState with the source values held COMPACT, the layout EataState and SarState share: `achunks` lists the 1024-float
    slab chunks of A, chunk j of `theta0` (and of every buffer built like it) belongs to slab chunk achunks[j]; `source` holds
    views into `theta0`, so reset() restores as TentState's.  For A = the 106 BatchNorm affines of a ResNet-50 that is 114
    chunks: 456 KiB per buffer, against 178 MiB for a slab in the flat layout."""

    def __init__(self, flat: FlatState, names: List[str]):
        super().__init__(flat, names)
        dev = flat.params.device
        base = flat.params.data_ptr()
        chunks, self._spans = [], []
        for t in self.tensors:
            o = (t.data_ptr() - base) // 4
            self._spans.append((len(chunks) * ALIGN, t.numel()))
            chunks += list(range(o // ALIGN, (o + _round_up(t.numel())) // ALIGN))
        self.n_achunks = len(chunks)
        self.achunks = torch.tensor(chunks, dtype=torch.int32).to(dev)
        self.theta0 = torch.zeros(self.n_achunks * ALIGN, dtype=torch.float32, device=dev)

    def _compact_views(self, buf):
        return [buf[o:o + n].view(t.shape) for (o, n), t in zip(self._spans, self.tensors)]

    def _slab_args(self, mask=None):
        """what every slab entry point takes to find A's chunks: achunks, n_achunks, chunk2tensor, active, n_tensors, n
        (`mask`: a per-tensor mask to walk under in place of `active`)"""
        f = self.flat
        return _p(self.achunks), self.n_achunks, _p(f.chunk2tensor), _p(self.active if mask is None else mask), len(f.tensors), f.total

    @torch.no_grad()
    def snapshot(self):
        self.source = self._compact_views(self.theta0)
        torch._foreach_copy_(self.source, [t.detach() for t in self.tensors])


class EataState(CompactState):
    """CompactState plus what EATA adds (Niu et al., ICML 2022): the running mean `m` [K] of the selected predictions and its
    validity flag, the gated copy of the Adam mask (`gate` = active and n > 0, written by stil_eata_rows), and the Fisher
    estimate, compact like the source values."""

    def __init__(self, flat: FlatState, names: List[str], num_classes: int):
        super().__init__(flat, names)
        dev = flat.params.device
        self.fisher: Optional[torch.Tensor] = None
        self.partial = torch.zeros(max(self.n_achunks, 1), dtype=torch.float64, device=dev)
        self.m = torch.zeros(num_classes, dtype=torch.float32, device=dev)
        self.m_valid = torch.zeros(1, dtype=torch.int32, device=dev)
        self.gate = torch.zeros_like(self.active)

    @torch.no_grad()
    def reset(self):
        """TentState.reset, and the running mean of the selected predictions is cleared too; the Fisher estimate is kept."""
        super().reset()
        self.m.zero_()
        self.m_valid.zero_()

    # ---- Fisher estimate: one tensor per member of A <-> the compact slab
    @torch.no_grad()
    def new_fisher(self):
        self.fisher = torch.zeros_like(self.theta0)

    @torch.no_grad()
    def fisher_accum(self, scale: float):
        """fisher += grads^2 * scale over A's chunks of this state's gradient slab"""
        lib().eata_fisher_accum(_p(self.fisher), _p(self.grads), *self._slab_args(), float(scale), _stream())

    @torch.no_grad()
    def anchor(self, alpha: float, out: torch.Tensor):
        """grads += 2 alpha F (theta - theta0) over A's chunks; out[0] = alpha sum F (theta - theta0)^2"""
        lib().eata_anchor(_p(self.flat.params), _p(self.theta0), _p(self.fisher), _p(self.grads), *self._slab_args(), float(alpha),
                          _p(self.partial), _p(out), _stream())

    def fisher_tensors(self) -> List[torch.Tensor]:
        return [v.clone() for v in self._compact_views(self.fisher)]

    @torch.no_grad()
    def load_fisher(self, tensors: List[torch.Tensor]):
        self.new_fisher()
        views = self._compact_views(self.fisher)
        for v, t in zip(views, tensors):
            if tuple(v.shape) != tuple(t.shape):
                raise ValueError(f"Fisher estimate of shape {tuple(t.shape)} for a parameter of shape {tuple(v.shape)}")
        torch._foreach_copy_(views, [t.detach().to(self.fisher.device, torch.float32) for t in tensors])


class SarState(CompactState):
    """CompactState plus what SAR adds (Niu et al., ICLR 2023): `saved` (A before the ascent step) and `e` (the ascent step
    rho g / |g|), compact like the source values and readable until the next step; `norm` (|g|, double) and its per-chunk
    scratch `partial`; the gated copy of the Adam mask (`gate` = active and n2 > 0, written by stil_sar_rows); `sel1`, the first
    pass's selection of the latest batch; the running mean of the second pass's loss (`ema`, `ema_valid`) and the recovery flag
    (`recover`), all on the device."""

    def __init__(self, flat: FlatState, names: List[str]):
        super().__init__(flat, names)
        dev = flat.params.device
        self.saved = torch.zeros_like(self.theta0)
        self.e = torch.zeros_like(self.theta0)
        self.partial = torch.zeros(max(self.n_achunks, 1), dtype=torch.float64, device=dev)
        self.norm = torch.zeros(1, dtype=torch.float64, device=dev)
        self.gate = torch.zeros_like(self.active)
        self.sel1: Optional[torch.Tensor] = None
        self.ema = torch.zeros(1, dtype=torch.float32, device=dev)
        self.ema_valid = torch.zeros(1, dtype=torch.int32, device=dev)
        self.recover = torch.zeros(1, dtype=torch.int32, device=dev)

    @torch.no_grad()
    def reset(self):
        """TentState.reset, and the running mean of the loss is forgotten too."""
        super().reset()
        self.ema.zero_()
        self.ema_valid.zero_()
        self.recover.zero_()

    @torch.no_grad()
    def perturb(self, rho: float):
        """norm <- |grads| over A; saved <- A; e <- rho grads / (norm + 1e-12); A <- A + e"""
        lib().sar_perturb(_p(self.flat.params), _p(self.grads), _p(self.saved), _p(self.e), *self._slab_args(), float(rho),
                          _p(self.partial), _p(self.norm), _stream())

    @torch.no_grad()
    def restore(self):
        """A <- saved, a copy"""
        lib().sar_restore(_p(self.flat.params), _p(self.saved), *self._slab_args(), _stream())

    @torch.no_grad()
    def recover_if_flagged(self):
        """When `recover` is set: A <- its source values, moments and step counts cleared, the running mean forgotten; decided
        on the device, nothing is written otherwise."""
        lib().sar_recover(_p(self.flat.params), _p(self.theta0), _p(self.exp_avg), _p(self.exp_avg_sq), _p(self.steps),
                          *self._slab_args(), _p(self.recover), _p(self.ema_valid), _stream())


def draw_perm(rng: np.random.Generator, B: int, grid: int) -> np.ndarray:
    """-> int32 [B, grid^2]: one uniform permutation of the patch slots per image, drawn from `rng`"""
    return rng.permuted(np.tile(np.arange(grid * grid, dtype=np.int32), (B, 1)), axis=1)


class DeyoState(TentState):
    """TentState plus what DeYO adds (Lee et al., ICLR 2024): the gated copy of the Adam mask (`gate` = active and n > 0,
    written by stil_deyo_rows) and the host generator of the patch permutations, seeded once: reset() leaves it running,
    drop() forgets it."""

    def __init__(self, flat: FlatState, names: List[str], seed: int):
        super().__init__(flat, names)
        self.gate = torch.zeros_like(self.active)
        self.rng = np.random.default_rng(seed)

        self._pin = None    # the pinned staging buffer of the permutations and the event of its last upload
        self._pin_done = None

    def draw(self, B: int, grid: int) -> np.ndarray:
        return draw_perm(self.rng, B, grid)

    def upload(self, perm: np.ndarray) -> torch.Tensor:
        """perm (host, int32 [B, grid^2]) -> a device tensor, staged through this state's pinned buffer by a non-blocking copy.
        The buffer is rewritten only once its previous upload has run (an event query; a wait only if the device is more than
        a whole step behind the host)."""
        src = torch.from_numpy(perm)
        if self._pin is None or self._pin.shape != src.shape:
            self._pin, self._pin_done = torch.empty(src.shape, dtype=torch.int32).pin_memory(), None
        if self._pin_done is not None and not self._pin_done.query():
            self._pin_done.synchronize()
        self._pin.copy_(src)
        out = self._pin.to(self.active.device, non_blocking=True)
        self._pin_done = torch.cuda.Event()
        self._pin_done.record()
        return out


class CgplState(TentState):
    """TentState plus what the consensus pseudo-label step adds: the gated copy of the Adam mask (`gate` = active and n > 0,
    written by stil_cgpl_rows) and the device counter of the coins' generator, one per adapted batch: reset() leaves it running,
    drop() forgets it."""

    def __init__(self, flat: FlatState, names: List[str]):
        super().__init__(flat, names)
        self.gate = torch.zeros_like(self.active)
        self.coin_step = torch.zeros(1, dtype=torch.int64, device=flat.params.device)


class RoidState(CompactState):
    """CompactState plus what ROID adds (Marsden, Doebler, Yang, WACV 2024): `ema` [K], the running mean prediction the diversity of
    a row is measured against (1 / K until a batch has moved it), and the weight ensembling of A with its compact source values."""

    def __init__(self, flat: FlatState, names: List[str], num_classes: int):
        super().__init__(flat, names)
        self.ema = torch.full((num_classes,), 1.0 / num_classes, dtype=torch.float32, device=flat.params.device)

    @torch.no_grad()
    def reset(self):
        """TentState.reset, and the running mean prediction returns to 1 / K."""
        super().reset()
        self.ema.fill_(1.0 / self.ema.numel())

    @torch.no_grad()
    def ensemble(self, momentum: float):
        """A <- momentum A + (1 - momentum) source values, over A's chunks (stil_roid_ensemble); momentum 1 writes nothing"""
        lib().roid_ensemble(_p(self.flat.params), _p(self.theta0), *self._slab_args(), float(momentum), _stream())


class RottaState(CompactState):
    """CompactState plus what RoTTA adds (Yuan, Xie, Li, CVPR 2023): `teacher`, the EMA teacher's values of A, compact like the
    source values (it equals them at creation and after reset()); the gated copy of the Adam mask (`gate` = active and n > 0,
    written by stil_rotta_rows); and the bank of N = `capacity` test samples, allocated at the first batch from that batch's shapes,
    all on the device: bank_img [N, 3, H, W] and bank_tab [N, C] (float32, zero-filled), label [N] (int32, -1: empty), unc [N]
    (float32), age [N] (int32), occ [K] (int32: filled slots per class), n [1] (int32: the filled slots are the prefix [0, n)) and
    owner [N] (int32: which sample of the latest batch a slot took, -1: none).  The first sample bank of this module: nothing in it
    is RoTTA's but the decision rule of stil_rotta_bank_update."""

    def __init__(self, flat: FlatState, names: List[str], num_classes: int, capacity: int):
        super().__init__(flat, names)
        self.K, self.capacity = int(num_classes), int(capacity)
        self.teacher = torch.zeros_like(self.theta0)
        self.gate = torch.zeros_like(self.active)
        self.bank_img: Optional[torch.Tensor] = None
        self.bank_tab: Optional[torch.Tensor] = None

    @torch.no_grad()
    def snapshot(self):
        super().snapshot()
        self.teacher.copy_(self.theta0)

    @torch.no_grad()
    def reset(self):
        """TentState.reset; the teacher returns to the source values and the bank is emptied: labels -1, occ, n and age 0, images
        and table zeroed."""
        super().reset()
        if self.source is not None:
            self.teacher.copy_(self.theta0)
        if self.bank_img is not None:
            self.label.fill_(-1)
            self.owner.fill_(-1)
            for t in (self.unc, self.age, self.occ, self.n, self.bank_img, self.bank_tab):
                t.zero_()

    @torch.no_grad()
    def ensure_bank(self, x_img, x_tab):
        """the bank, allocated from the first batch's shapes; a batch of other shapes is an error"""
        N, dev = self.capacity, x_img.device
        if self.bank_img is None:
            self.bank_img = torch.zeros((N,) + tuple(x_img.shape[1:]), dtype=torch.float32, device=dev)
            self.bank_tab = torch.zeros((N,) + tuple(x_tab.shape[1:]), dtype=torch.float32, device=dev)
            self.label = torch.full((N,), -1, dtype=torch.int32, device=dev)
            self.owner = torch.full((N,), -1, dtype=torch.int32, device=dev)
            self.unc = torch.zeros((N,), dtype=torch.float32, device=dev)
            self.age = torch.zeros((N,), dtype=torch.int32, device=dev)
            self.occ = torch.zeros((self.K,), dtype=torch.int32, device=dev)
            self.n = torch.zeros((1,), dtype=torch.int32, device=dev)
        if tuple(x_img.shape[1:]) != tuple(self.bank_img.shape[1:]) or tuple(x_tab.shape[1:]) != tuple(self.bank_tab.shape[1:]):
            raise ValueError(f"rotta: a batch of samples {tuple(x_img.shape[1:])}, {tuple(x_tab.shape[1:])} for a bank of "
                             f"{tuple(self.bank_img.shape[1:])}, {tuple(self.bank_tab.shape[1:])}")

    @torch.no_grad()
    def exchange(self):
        """A <-> teacher over A's chunks, bit-exact (stil_rotta_exchange)"""
        lib().rotta_exchange(_p(self.flat.params), _p(self.teacher), *self._slab_args(), _stream())

    @torch.no_grad()
    def move_teacher(self, nu: float):
        """teacher <- (1 - nu) teacher + nu A over A's chunks, under the gate: a batch with n == 0 moves nothing (stil_rotta_teacher)"""
        lib().rotta_teacher(_p(self.flat.params), _p(self.teacher), *self._slab_args(mask=self.gate), float(nu), _stream())

    @torch.no_grad()
    def bank_update(self, zt, lambda_t: float, lambda_u: float):
        """The bank's bookkeeping moved over the batch whose teacher logits are zt [B, K] (stil_rotta_bank_update).
        -> dict(probs, H, yhat, accepted, slot_of, counts [accepted, evictions, n after, 0], lse); writes label, unc, age, occ, n, owner"""
        _chk(zt)
        zt = zt.contiguous()
        B, K = zt.shape
        if K != self.K:
            raise ValueError(f"rotta: logits of {K} classes for a bank of {self.K}")
        lse, h = _empty(zt, B, torch.float64), _empty(zt, B, torch.float32)
        yhat, slot_of = _empty(zt, B, torch.int32, 2)
        acc = _empty(zt, B, torch.uint8)
        p = torch.empty_like(zt)
        counts = torch.empty((4,), dtype=torch.int32, device=zt.device)
        lib().rotta_bank_update(_p(zt), K, B, K, self.capacity, float(lambda_t), float(lambda_u), _p(self.label), _p(self.unc), _p(self.age),
                                _p(self.occ), _p(self.n), _p(self.owner), _p(lse), _p(p), K, _p(h), _p(yhat), _p(acc), _p(slot_of),
                                _p(counts), _stream())
        return dict(probs=p, H=h, yhat=yhat, accepted=acc, slot_of=slot_of, counts=counts, lse=lse)

    @torch.no_grad()
    def bank_store(self, x_img, x_tab):
        """bank_img[s], bank_tab[s] <- the sample owner[s] of the batch, for every slot the latest bank_update handed over
        (stil_rotta_bank_store: a bit-exact gather)"""
        _chk(x_img, x_tab)
        B = x_img.shape[0]
        lib().rotta_bank_store(_p(x_img), _p(x_tab), _p(self.owner), self.capacity, B, x_img[0].numel(), x_tab[0].numel(),
                               _p(self.bank_img), _p(self.bank_tab), _stream())


def bn_momentum(hp, t: int) -> float:
    """alpha_t of the t-th update of the BatchNorm memory, t = 1, 2, ...: min(1, tta_bn_momentum x tta_bn_momentum_decay^t +
    tta_bn_momentum_min), DUA's schedule (Mirza et al., CVPR 2022); with the default decay 1 and minimum 0 it is tta_bn_momentum."""
    return min(1.0, float(hp.tta_bn_momentum) * float(hp.tta_bn_momentum_decay) ** int(t) + float(hp.tta_bn_momentum_min))


class BnMemory:
    """The running estimate of the TARGET BatchNorm statistics of model.encoder_imaging (tta_bn_momentum; RoTTA's robust
    BatchNorm, Yuan et al., CVPR 2023; DUA, Mirza et al., CVPR 2022), held in model._bn_mem beside and independent of TentState:
    two [2, sum C] float32 buffers (row 0 the means, row 1 the variances) with one [C] view per layer and row.  Every forward of a
    batch READS the front buffer; the one forward that updates the estimate WRITES the back buffer (ops.bn_memory's `update`), and
    commit() swaps the two at the end of the step and counts the update in `t`, on the host: nothing is read back.  `alpha` is the
    momentum of the current batch (bn_momentum(hp, t + 1), set by begin()).  load_source() copies the layers' running buffers into
    the front buffer and zeroes t; the model's running_mean / running_var / num_batches_tracked are read there and never written.
    `views`: dua_step's ImageAugmenter, seeded once (tta_view_seed): load_source() leaves its generator running."""

    def __init__(self, model):
        hp = model.hp
        self.layers = [mod for mod in model.model.encoder_imaging.modules() if isinstance(mod, nn.BatchNorm2d)]
        total = sum(mod.num_features for mod in self.layers)
        dev = self.layers[0].running_mean.device
        self.bufs = [torch.zeros((2, total), dtype=torch.float32, device=dev) for _ in range(2)]
        self._views = [{}, {}]   # per buffer: running_mean.data_ptr() of the layer -> (mean [C], var [C])
        o = 0
        for mod in self.layers:
            C = mod.num_features
            for buf, views in zip(self.bufs, self._views):
                views[mod.running_mean.data_ptr()] = (buf[0, o:o + C], buf[1, o:o + C])
            o += C
        self.front, self.t, self.alpha = 0, 0, bn_momentum(hp, 1)
        self.views = None
        if hp.tta_method == "dua":
            from .augment import ImageAugmenter
            self.views = ImageAugmenter(img_size=hp.img_size, target=hp.target, kind=hp.tta_view_policy, augmentation_rate=1.0,
                                        seed=hp.tta_view_seed, augmentation_speedup=False)
        self.load_source()

    def _pairs(self, which):
        return [self._views[which][mod.running_mean.data_ptr()] for mod in self.layers]

    @torch.no_grad()
    def load_source(self):
        pairs = self._pairs(self.front)
        torch._foreach_copy_([p[0] for p in pairs] + [p[1] for p in pairs],
                             [mod.running_mean for mod in self.layers] + [mod.running_var for mod in self.layers])
        self.t = 0

    def begin(self, hp):
        """before the first forward of a batch: under tta_episodic the estimate returns to the checkpoint's; alpha <- alpha_(t+1)"""
        if hp.tta_episodic:
            self.load_source()
        self.alpha = bn_momentum(hp, self.t + 1)

    def layer(self, running_mean):
        """-> (mean, var) to read and (mean, var) to write, [C] views, of the layer that owns `running_mean`"""
        key = running_mean.data_ptr()
        try:
            return self._views[self.front][key] + self._views[1 - self.front][key]
        except KeyError:
            raise RuntimeError("BnMemory: this BatchNorm layer is not one the memory was built over (the model's buffers moved since; "
                               "tta.drop(model) forgets the memory, the next batch rebuilds it)") from None

    def commit(self):
        self.front, self.t = 1 - self.front, self.t + 1

    def state(self):
        """-> [(mean, var)] per layer, in encoder_imaging's module order: copies of the current estimate"""
        return [(m.clone(), v.clone()) for m, v in self._pairs(self.front)]


def _memory(model) -> Optional[BnMemory]:
    """model._bn_mem when tta_bn_momentum is set (created on first use, the model being on its device), else None"""
    if model.hp.tta_bn_momentum is None:
        return None
    if model._bn_mem is None:
        model._bn_mem = BnMemory(model)
    return model._bn_mem


def _begin_memory(model) -> Optional[BnMemory]:
    mem = _memory(model)
    if mem is not None:
        mem.begin(model.hp)
    return mem


def _commit_memory(model):
    if model._bn_mem is not None and model.hp.tta_bn_momentum is not None:
        model._bn_mem.commit()


def _state(model) -> TentState:
    """model._tent, created on first use (the model is on its device)"""
    if model._tent is None:
        names = [n[len("model."):] for n in param_names(model)]   # FlatState names the backbone's own parameters
        if model.hp.tta_method == "eata":
            model._tent = EataState(model.flat, names, model.hp.num_classes)
        elif model.hp.tta_method == "deyo":
            model._tent = DeyoState(model.flat, names, model.hp.tta_shuffle_seed)
        elif model.hp.tta_method == "sar":
            model._tent = SarState(model.flat, names)
        elif model.hp.tta_method == "cgpl":
            model._tent = CgplState(model.flat, names)
        elif model.hp.tta_method == "roid":
            model._tent = RoidState(model.flat, names, model.hp.num_classes)
        elif model.hp.tta_method == "rotta":
            model._tent = RottaState(model.flat, names, model.hp.num_classes, model.hp.tta_rotta_capacity)
        else:
            model._tent = TentState(model.flat, names)
        if model.hp.tta_method in ("marginal_entropy", "rotta"):
            from .augment import ImageAugmenter   # the torchvision-branch kernels: test images arrive as float CHW
            hp = model.hp
            model._tent.views = ImageAugmenter(img_size=hp.img_size, target=hp.target, kind=hp.tta_view_policy, augmentation_rate=1.0,
                                               seed=hp.tta_view_seed, augmentation_speedup=False)
    return model._tent


def _eata_state(model) -> EataState:
    if model.hp.tta_method != "eata":
        raise ValueError(f"the Fisher estimate belongs to tta_method 'eata' (this model: {model.hp.tta_method!r})")
    model.setup_device()
    return _state(model)


def _begin(model) -> TentState:
    """The state a batch adapts under: with tta_episodic A is restored and the state reset before every batch; the source
    values are taken whenever none are held (the first adapted batch since construction / load_state_dict / reset)."""
    model.setup_device()
    st = _state(model)
    if model.hp.tta_episodic:
        st.reset()
    if st.source is None:
        st.snapshot()
    _begin_memory(model)
    return st


def drop(model):
    """Forget the adaptation state (moments, step counts, source values; EATA's running mean of predictions and its Fisher
    estimate, which belongs to the weights it was estimated on; the running estimate of the BatchNorm statistics): load_state_dict
    calls this."""
    model._tent = None
    model._bn_mem = None


def reset(model):
    """A <- its source values (A as it stood at the first adapted batch since construction / load_state_dict / reset),
    moments and step counts cleared; the next adapted batch takes the source values afresh.  EATA: the running mean of
    the selected predictions is cleared too, the Fisher estimate is kept.  SAR: the running mean of the loss is forgotten too.
    The running estimate of the BatchNorm statistics (tta_bn_momentum) returns to the checkpoint's and its update count to 0."""
    with torch.inference_mode(False):
        if model._tent is not None:
            model._tent.reset()
            model._tent.source = None
        if model._bn_mem is not None:
            model._bn_mem.load_source()


# ---------------------------------------------------------------------------------------------- the adapting pass
def _inputs(model, x):
    dev = model.prototypes.device
    x_img, x_tab = (t.to(dev, torch.float32).contiguous() for t in x[:2])
    if x_img.is_inference():
        x_img = x_img.clone()
    if x_tab.is_inference():
        x_tab = x_tab.clone()
    return x_img, x_tab


def _bn_scope(model, B, update):
    """The BatchNorm rule of an adapting forward on B images.  Without tta_bn_momentum: the batch statistics, under tta_bn_prior = N
    blended with the checkpoint's at rho = B / (N + B).  With it the memory (model._bn_mem, the estimate as the batch found it) takes
    the checkpoint's place: rho = B / (N + B) under tta_bn_prior = N, otherwise rho = alpha_t, i.e. the layer normalises by exactly
    the updated estimate (RoTTA); `update`: this forward is the one of its batch that writes the update (biased variance)."""
    N = model.hp.tta_bn_prior
    mem = _memory(model)
    if mem is None:
        return contextlib.nullcontext() if N is None else ops.bn_prior(N, B)
    return ops.bn_memory(mem, mem.alpha if N is None else B / (N + B), mem.alpha, unbiased=False, update=update)


def _forward(model, x_img, x_tab, update=False, outputs="m", scope=None):
    """The adapting forward -> out_m (outputs "all": the 10-tuple of forward_all, out_m first): no MI-layer dropout; BatchNorm over
    the B images of this batch by `_bn_scope`'s rule (a short last batch gets its own rho), running buffers untouched.  scope: a
    BatchNorm rule of the caller's in place of `_bn_scope`'s (rotta_step's passes over its bank)."""
    with ops.frozen_bn_stats(), (_bn_scope(model, x_img.shape[0], update) if scope is None else scope):
        outs = model.model.forward_all((x_img, x_tab), train=True, mi_masks=None)
        return outs if outputs == "all" else outs[0]


def _score_forward(model, x_img, x_tab, update=False, outputs="m"):
    """The forward of `_forward` alone, under no_grad on the layouts of the current weights -> out_m (outputs "all": the 10-tuple)"""
    with torch.no_grad():
        model.flat.refresh_layouts(student=True, teacher=False)
        return _forward(model, x_img, x_tab, update, outputs)


@contextlib.contextmanager
def _grads_of(model, st):
    """requires_grad on A only, no gradient collectives (adaptation is per rank), layouts of the current weights, grad mode on
    and every gradient slot in st's slab; flags, exchange and slots restored after"""
    adapted = {id(t) for t in st.tensors}
    flags = [(q, q.requires_grad) for q in model.parameters()]
    exchange, ops._exchange = ops._exchange, None
    try:
        for q, _ in flags:
            q.requires_grad_(id(q) in adapted)
        model.flat.refresh_layouts(student=True, teacher=False)
        with torch.enable_grad(), st.redirect():
            yield
    finally:
        ops._exchange = exchange
        for q, f in flags:
            q.requires_grad_(f)


def adapting_pass(model, x, st, loss_fn, update=True, outputs="m", scope=None):
    """One adapting forward and backward on the inputs x = (images, table, ...) of a batch: the forward of `_forward`,
    loss_fn(out_m) -> (loss, probs, extras) (outputs "all": loss_fn takes the whole 10-tuple of forward_all), gradients of the
    loss for A only (no weight-gradient products) in st.grads.
    Writes st.grads and whatever loss_fn writes and, with tta_bn_momentum and `update`, the back buffer of the BatchNorm memory
    (a constant of the backward); never a parameter, BatchNorm buffer, teacher, prototype or training slab.  scope: `_forward`'s.
    The caller holds torch.inference_mode(False).  -> (out_m, loss, probs, extras), detached."""
    x_img, x_tab = _inputs(model, x)
    with _grads_of(model, st):
        outs = _forward(model, x_img, x_tab, update, outputs, scope)
        loss, probs, extras = loss_fn(outs)
        loss.backward()
    out_m = outs[0] if outputs == "all" else outs
    return out_m.detach(), loss.detach(), probs, extras


def _e_margin(hp):
    """tta_e_margin resolved: None -> 0.4 ln K, EATA's published fraction of the maximal entropy"""
    return 0.4 * math.log(hp.num_classes) if hp.tta_e_margin is None else float(hp.tta_e_margin)


def tent_step(model, batch):
    """TENT (Wang et al., ICLR 2021) on one test batch: forward with batch-statistics BatchNorm (running buffers untouched,
    no MI-layer dropout), loss = mean row entropy of softmax(out_m), gradients for A only (no weight-gradient products),
    one Adam step over A (tta_lr, betas (0.9, 0.999), eps 1e-8, no weight decay).  Writes A, its own moments and step counts,
    acc_test / auc_test and last_tta; never the training slabs, buffers, teacher or prototypes.  The scores are softmax(out_m)
    of this forward, before the update.  Rank-local: no collectives.  Works after freeze() and inside torch.inference_mode()."""
    x, y = batch
    with torch.inference_mode(False):
        st = _begin(model)
        out_m, loss, probs, _ = adapting_pass(model, x, st, entropy)
        st.adam_step(model.hp.tta_lr)
        _commit_memory(model)
        model.last_tta = dict(loss=loss, y_hat_m=out_m, probs=probs)
        return model._score_test(probs, y)


def eata_step(model, batch):
    """EATA (Niu et al., ICML 2022) on one test batch: TENT's forward (batch-statistics BatchNorm, no MI-layer dropout) and
    input-gradient-only backward, with (1) the loss restricted to the reliable (H_r < tta_e_margin) and non-redundant
    (|cos(m, p_r)| < tta_d_margin, m = running mean of the selected predictions) rows, weighted by exp(E0 - H_r) and
    averaged over the n selected rows, and (2) when a Fisher estimate is loaded, the anchor tta_fisher_alpha sum F (A - A0)^2
    added to the loss and its gradient to A's.  One Adam step over A if and only if n > 0: n, the counts and that gate stay
    on the device (stil_eata_rows writes the gated Adam mask), so the step reads nothing back.  Writes what tent_step writes
    and m / m_valid; never the Fisher estimate.  The scores are softmax(out_m) of this forward.  With tta_episodic, m is
    cleared and A restored before each batch: the redundancy filter and the anchor are inert there (m is always invalid,
    A - A0 = 0)."""
    x, y = batch
    hp = model.hp
    with torch.inference_mode(False):
        st = _begin(model)
        e0 = _e_margin(hp)
        out_m, loss_ent, probs, info = adapting_pass(model, x, st, lambda z: eata_entropy(
            z, e0, hp.tta_d_margin, hp.tta_probs_momentum, st.m, st.m_valid, st.active, st.gate))
        loss_anchor = torch.zeros((1,), dtype=torch.float32, device=out_m.device)
        if st.fisher is not None:
            st.anchor(hp.tta_fisher_alpha, loss_anchor)
        st.adam_step(hp.tta_lr, mask=st.gate)
        _commit_memory(model)
        model.last_tta = dict(loss=loss_ent + loss_anchor[0], y_hat_m=out_m, probs=probs, n_selected=info["counts"][0],
                              n_reliable=info["counts"][1], loss_entropy=loss_ent, loss_anchor=loss_anchor[0],
                              selected=info["sel"], reliable=info["rel"], entropy=info["H"], cos=info["cos"], weight=info["w"])
        return model._score_test(probs, y)


def shot_im_step(model, batch):
    """SHOT-IM (Liang et al., ICML 2020; the baseline the TENT paper reports beside itself) on one test batch: tent_step with
    the information-maximisation loss, mean row entropy + tta_div_weight x sum_k pbar_k log(pbar_k + tta_div_eps), pbar the mean
    prediction of THIS batch (no running marginal).  SHOT's frozen classifier head holds by construction (A never contains
    it); its pseudo-label term is not part of this method.  State, Adam, episodic mode, tta_bn_prior and what is written are
    tent_step's; tta_div_weight = 0 is tent_step bit for bit.  last_tta: loss, loss_entropy, loss_diversity, marginal (pbar,
    [K]), y_hat_m, probs, all on the device: the step reads nothing back."""
    x, y = batch
    hp = model.hp
    with torch.inference_mode(False):
        st = _begin(model)
        out_m, loss, probs, info = adapting_pass(model, x, st, lambda z: infomax(z, hp.tta_div_weight, hp.tta_div_eps))
        st.adam_step(hp.tta_lr)
        _commit_memory(model)
        model.last_tta = dict(loss=loss, loss_entropy=info["loss_entropy"], loss_diversity=info["loss_diversity"],
                              marginal=info["marginal"], y_hat_m=out_m, probs=probs)
        return model._score_test(probs, y)


def make_views(model, x, draws=None):
    """The views marginal_entropy_step adapts on (and dua_step takes its statistics from), from the inputs x = (images [B, 3, H, W], table [B, C], ...) of a batch:
    every image repeated tta_views times, sample-major (row g V + v is view v of sample g), and augmented by the model-owned
    ImageAugmenter (family tta_view_policy, every row augmented, seeded by tta_view_seed when the adaptation state is created);
    the table rows repeated UNCHANGED (the model holds no table to draw corrupted cells from).  draws: the host draws of an
    earlier call (last_tta["draws"]), which rebuild its views bit for bit and leave the generator alone; None draws afresh.
    With tta_method "rotta" x is the bank (rotta_step's strong view of it): ONE view per slot, whatever tta_views says.
    -> (views [B V, 3, P, P], table [B V, C], draws)"""
    if model.hp.tta_method not in ("marginal_entropy", "dua", "rotta"):
        raise ValueError(f"augmented views belong to tta_method 'marginal_entropy', 'dua' and 'rotta' (this model: {model.hp.tta_method!r})")
    with torch.inference_mode(False), torch.no_grad():
        model.setup_device()
        aug = _memory(model).views if model.hp.tta_method == "dua" else _state(model).views   # dua holds no TentState
        x_img, x_tab = _inputs(model, x)
        V = 1 if model.hp.tta_method == "rotta" else model.hp.tta_views
        B, _, H, W = x_img.shape
        if draws is None:
            draws = aug.draw(B * V, H, W)
        views = aug(x_img.repeat_interleave(V, dim=0), draws, want_orig=False)[0]
        return views, x_tab.repeat_interleave(V, dim=0), draws


def marginal_entropy_step(model, batch):
    """MEMO (Zhang, Levine, Finn, NeurIPS 2022) on one test batch of B samples, B = 1 being the case it is made for:
    (1) V = tta_views augmented views of every sample (make_views); (2) the adapting pass on the B V rows with the loss
    mean_g H(mean_v softmax(out_m[g V + v])), gradients for A only (no weight-gradient products), under tta_bn_prior = N at
    rho = B V / (N + B V); (3) one Adam step over A; (4) the scores: the forward of bn_adapt_step on the CLEAN batch with the
    updated A, at rho = B / (N + B).  This is the one method that scores after its update: with one sample and tta_episodic,
    scores taken before it would show no adaptation at all.  With B > 1 the samples share one update, of the mean of their
    marginal entropies.  MEMO as published is B = 1, tta_episodic: True, tta_bn_prior: 16, and adapts every parameter; here A is
    the norm affines, as for every method.  State, Adam, episodic mode, reset and what is written are tent_step's; the views'
    generator runs on through reset_tta() and episodes, and is dropped with the state by load_state_dict.
    last_tta: loss, marginal [B, K], marginal_entropy [B] of the adapting pass, y_hat_m and probs [B, K] of the scoring
    forward, all on the device, and draws, the host dict make_views rebuilds the views from."""
    x, y = batch
    hp = model.hp
    with torch.inference_mode(False):
        st = _begin(model)
        x_img, x_tab = _inputs(model, x)
        B, V = x_img.shape[0], hp.tta_views
        views, tab_rep, draws = make_views(model, (x_img, x_tab))
        _, loss, _, info = adapting_pass(model, (views, tab_rep), st, lambda z: marginal_entropy(z, B, V))
        st.adam_step(hp.tta_lr)
        _commit_memory(model)   # before the scoring forward: this method scores after its update, of the memory too
        out_m = _score_forward(model, x_img, x_tab)
        probs = ops.softmax_rows(out_m)
        model.last_tta = dict(loss=loss, marginal=info["marginal"], marginal_entropy=info["marginal_entropy"], y_hat_m=out_m,
                              probs=probs, draws=draws)
        return model._score_test(probs, y)


def deyo_step(model, batch):
    """DeYO (Lee et al., ICLR 2024) on one test batch: (1) one permutation of the tta_patch_grid^2 patch slots per image, drawn
    on the host from the state's generator (seeded by tta_shuffle_seed when the adaptation state is created; it runs on through
    reset_tta() and episodes and is dropped with the state by load_state_dict), checked to be a permutation and uploaded
    from the state's pinned buffer without a blocking copy; (2) the forward of bn_adapt_step on the patch-shuffled images and the UNCHANGED table, under
    no_grad: zs; (3) TENT's forward and input-gradient-only backward on the clean batch with the loss restricted to the rows
    with H_r < tta_ent_margin and plpd_r = p_r[yhat_r] - softmax(zs_r)[yhat_r] > tta_plpd_margin, weighted by
    tta_reweight_ent exp(E0 - H_r) + tta_reweight_plpd exp(plpd_r) (E0 = tta_e_margin) and averaged over the n selected rows;
    (4) one Adam step over A if and only if n > 0: n, the counts and that gate stay on the device, the step reads nothing back.
    Unlike the published code, (2) runs on ALL B rows, not only the entropy-reliable ones: shapes stay fixed and nothing is
    read back; its BatchNorm therefore uses the statistics of the whole shuffled batch (under tta_bn_prior like every
    adapting forward).  Writes what tent_step writes.  The scores are softmax(out_m) of the clean forward, before the update.
    last_tta: loss, n_selected, n_reliable, entropy, plpd, weight, reliable, selected, y_hat_m, probs, y_hat_shuffled (zs), all
    on the device, and perm, the host array patch_shuffle rebuilds the shuffled batch from."""
    x, y = batch
    hp = model.hp
    with torch.inference_mode(False):
        st = _begin(model)
        x_img, x_tab = _inputs(model, x)
        g = hp.tta_patch_grid
        perm = st.draw(x_img.shape[0], g)
        if not np.array_equal(np.sort(perm, axis=1), np.broadcast_to(np.arange(g * g, dtype=np.int32), perm.shape)):
            raise RuntimeError("deyo_step: a drawn row is not a permutation of the patch slots")
        tau = 0.5 * math.log(hp.num_classes) if hp.tta_ent_margin is None else float(hp.tta_ent_margin)
        e0 = _e_margin(hp)
        zs = _score_forward(model, patch_shuffle(x_img, g, st.upload(perm)), x_tab)
        out_m, loss, probs, info = adapting_pass(model, (x_img, x_tab), st, lambda z: deyo_entropy(
            z, zs, tau, hp.tta_plpd_margin, e0, hp.tta_reweight_ent, hp.tta_reweight_plpd, st.active, st.gate))
        st.adam_step(hp.tta_lr, mask=st.gate)
        _commit_memory(model)
        model.last_tta = dict(loss=loss, n_selected=info["counts"][0], n_reliable=info["counts"][1], entropy=info["H"],
                              plpd=info["plpd"], weight=info["w"], reliable=info["rel"], selected=info["sel"], y_hat_m=out_m,
                              probs=probs, y_hat_shuffled=zs, perm=perm)
        return model._score_test(probs, y)


def sar_reset_value(hp):
    """tta_sar_reset resolved: None -> 0.2 ln K / ln 1000 (the published ImageNet constant at the same fraction of the maximal
    entropy: this project's rule, not the paper's), False -> 0.0 (recovery disabled), a number -> itself."""
    c = hp.tta_sar_reset
    if c is False:
        return 0.0
    return 0.2 * math.log(hp.num_classes) / math.log(1000.0) if c is None else float(c)


SAR_EMA_MOMENTUM = 0.9   # of the running mean of the second pass's loss: the published value


def sar_step(model, batch):
    """SAR (Niu et al., ICLR 2023) on one test batch, two adapting passes on the same inputs: (1) TENT's forward and
    input-gradient-only backward with the loss (1/n1) sum of H_r over the rows with H_r < tta_e_margin, unweighted; (2) the ascent
    step over A: saved <- A, A <- A + tta_sar_rho g / (|g| + 1e-12), |g| over the whole of A (stil_sar_perturb reads A and g from
    the slabs; between the passes only A changes, the norm affines are read from the slab by their kernels and the conv / Linear
    layouts that refresh_layouts rebuilds hold none of them, so no cached form of A survives); (3) the second pass at the perturbed
    A, BatchNorm again by the batch's statistics (under tta_bn_prior), with the loss (1/n2) sum of H2_r over the rows the first pass
    kept AND with H2_r < tta_e_margin; (4) A <- saved, a copy; (5) one Adam step over A on the second pass's gradients if and only if
    n2 > 0; (6) with n2 > 0 the running mean of the second loss: ema <- L2, or 0.9 ema + 0.1 L2 when one is held; (7) unless
    tta_sar_reset is False: when a running mean is held and lies below tta_sar_reset, A <- its source values, moments and step counts
    cleared, the running mean forgotten -- after the Adam step, which it thereby discards, as in the published code.  n1, n2, the gate,
    the running mean and the recovery decision stay on the device: the step reads nothing back.  Writes what tent_step writes and the
    running mean.  The scores are softmax(out_m) of the FIRST pass, before any change.
    last_tta: loss (L2), loss_first, n_selected (n2), n_first (n1), n_reliable (rows with H2 < margin), grad_norm (|g| of the first
    pass, double), ema, ema_valid, recovered (after the step), entropy, entropy_second, selected_first, selected, y_hat_m, probs, all
    on the device."""
    x, y = batch
    hp = model.hp
    with torch.inference_mode(False):
        st = _begin(model)
        e0 = _e_margin(hp)
        c = sar_reset_value(hp)
        xs = _inputs(model, x)
        out_m, loss1, probs, i1 = adapting_pass(model, xs, st, lambda z: sar_entropy(z, e0))
        st.sel1 = i1["sel"]
        st.perturb(hp.tta_sar_rho)
        _, loss2, _, i2 = adapting_pass(model, xs, st, lambda z: sar_entropy(
            z, e0, st.sel1, st.active, st.gate, st.ema, st.ema_valid, SAR_EMA_MOMENTUM, c, st.recover), update=False)
        st.restore()
        st.adam_step(hp.tta_lr, mask=st.gate)
        if c > 0.0:
            st.recover_if_flagged()
        _commit_memory(model)
        model.last_tta = dict(loss=loss2, loss_first=loss1, n_selected=i2["counts"][0], n_first=i1["counts"][0],
                              n_reliable=i2["counts"][1], grad_norm=st.norm[0].clone(), ema=st.ema[0].clone(),
                              ema_valid=st.ema_valid[0].clone(), recovered=st.recover[0].clone(), entropy=i1["H"],
                              entropy_second=i2["H"], selected_first=i1["sel"], selected=i2["sel"], y_hat_m=out_m, probs=probs)
        return model._score_test(probs, y)


def fusion_pass(model, x, st, loss_fn):
    """READ's pass on the inputs x = (images, table, ...) of a batch, not `adapting_pass`: (1) under no_grad, encoder_imaging in
    eval mode on the checkpoint's running statistics and the tabular encoder, the launches plain test_step makes; (2) under grad,
    forward_all(train=False) on those tokens: only A (the last fusion layer's qkv weight and bias) requires grad, so autograd
    records nothing before that layer's qkv product and the backward never enters an encoder or an earlier fusion layer;
    (3) loss_fn(out_m) -> (loss, probs, extras) and its backward, the two gradients into st.grads (one weight-gradient product
    and one column sum).  Writes st.grads and whatever loss_fn writes; never a parameter, BatchNorm buffer, teacher, prototype or
    training slab.  The caller holds torch.inference_mode(False).  -> (out_m, loss, probs, extras), detached."""
    x_img, x_tab = _inputs(model, x)
    net = model.model
    with _grads_of(model, st):
        with torch.no_grad():
            x_i = net.encoder_imaging.run(x_img, False, None)
            x_t = net.tabular_tokens(x_tab, False)
        out_m = net.forward_all((x_img, x_tab), train=False, x_i=x_i, x_t=x_t)[0]
        loss, probs, extras = loss_fn(out_m)
        loss.backward()
    return out_m.detach(), loss.detach(), probs, extras


def read_step(model, batch):
    """READ (Yang et al., ICLR 2024, "Test-time Adaptation against Multi-modal Reliability Bias"; form and constants as recalled:
    unpinned) on one test batch: the modality encoders and their normalisation stay at the source (eval-mode BatchNorm on the
    checkpoint's statistics, no gradient), A = the Q/K/V projection of the last fusion layer (tta_params "fusion"), the loss
    read_loss = mean_r c_r log(e gamma / c_r) + tta_div_weight x sum_k pbar_k log(pbar_k + tta_div_eps) with gamma = tta_read_gamma
    (None: 1/e), one Adam step over A (tta_lr; READ's published rate is 1e-4, as recalled).  The first method whose backward never
    enters the ResNet (`fusion_pass`).  Writes A, its own moments and step counts, acc_test / auc_test and last_tta; never the
    training slabs, buffers, teacher or prototypes.  The scores are softmax(out_m) of this forward, before the update: on the
    first batch those of test_step without adaptation.  tta_bn_prior and tta_bn_momentum are refused with this method.  State,
    Adam, episodic mode and reset are tent_step's.  Rank-local: no collectives.
    last_tta: loss, loss_confidence, loss_balance, y_hat_m, probs, yhat, conf, marginal, all on the device: the step reads nothing
    back."""
    x, y = batch
    hp = model.hp
    with torch.inference_mode(False):
        st = _begin(model)
        out_m, loss, probs, info = fusion_pass(model, x, st, lambda z: read_loss(z, read_gamma(hp), hp.tta_div_weight, hp.tta_div_eps))
        st.adam_step(hp.tta_lr)
        model.last_tta = dict(loss=loss, loss_confidence=info["loss_confidence"], loss_balance=info["loss_balance"], y_hat_m=out_m,
                              probs=probs, yhat=info["yhat"], conf=info["conf"], marginal=info["marginal"])
        return model._score_test(probs, y)


def cgpl_step(model, batch):
    """STiL's own semi-supervised branch (CGPL, PGLS and the three soft cross-entropies, STiLModel.py:255-303 with use_ema False:
    the pseudo-labels come from the student's own detached outputs) run on one test batch, every row taken as unlabelled: (1) TENT's
    forward, all ten outputs of forward_all kept; (2) under no_grad and unless the rate is 1, the normalised multimodal projection of
    cat(e_si, e_c, e_st); (3) one coin per row, drawn on the device from (tta_pl_seed, the state's batch counter); (4) cgpl_loss with
    rate = tta_pl_rate (None: rate_pseudo), th = tta_pl_threshold (None: th1), T = temperature and the checkpoint's prototypes;
    (5) one backward through all three heads, gradients for A only (no weight-gradient products); (6) one Adam step over A if and only
    if n > 0 rows reach the threshold: n, the counts and that gate stay on the device, the step reads nothing back.  The modality
    heads act here: a row whose tabular head disagrees with the other two (case 2_i) pulls that head alone towards their consensus,
    and with tta_params "norm" that gradient reaches the tabular encoder's LayerNorms through out_t; under an image shift the roles
    swap.  Not part of this method: the checkpoint's EMA teacher as the label source, any update of the prototypes, the ITC, CLUB and
    prototype losses, and distribution alignment (hp.DA is not applied at test time: its queue belongs to training).  Writes what
    tent_step writes; tta_bn_prior and tta_bn_momentum compose as for tent_step.  The scores are softmax(out_m) of this forward,
    before the update.  The coin counter runs on through reset_tta() and episodes and is dropped with the state by load_state_dict.
    last_tta: loss, loss_m, loss_i, loss_t, y_hat_m, y_hat_i, y_hat_t, probs, pseudo_label, conf, flags, coin, counts, all on the
    device."""
    x, y = batch
    hp = model.hp
    with torch.inference_mode(False):
        st = _begin(model)
        rate, th = cgpl_rate(hp), cgpl_threshold(hp)
        heads = {}

        def loss_fn(outs):
            zm, zi, zt, e_si, _, _, e_st, _, _, e_c = outs
            feat = None
            if rate < 1.0:
                with torch.no_grad():
                    feat = model.project_3features(torch.cat((e_si.detach(), e_c.detach(), e_st.detach()), dim=1))[0]
            coin = ops.rng_mask((zm.shape[0],), 0.5, hp.tta_pl_seed, 0, zm.device, st.coin_step)
            heads.update(y_hat_i=zi.detach(), y_hat_t=zt.detach(), coin=coin)
            return cgpl_loss(zm, zi, zt, feat, model.prototypes, coin, rate, float(hp.temperature), th, st.active, st.gate)

        out_m, loss, probs, info = adapting_pass(model, x, st, loss_fn, outputs="all")
        lib().counter_inc(_p(st.coin_step), _stream())
        st.adam_step(hp.tta_lr, mask=st.gate)
        _commit_memory(model)
        model.last_tta = dict(loss=loss, loss_m=info["loss_m"], loss_i=info["loss_i"], loss_t=info["loss_t"], y_hat_m=out_m,
                              y_hat_i=heads["y_hat_i"], y_hat_t=heads["y_hat_t"], probs=probs, pseudo_label=info["pseudo_label"],
                              conf=info["conf"], flags=info["flags"], coin=heads["coin"], counts=info["counts"])
        return model._score_test(probs, y)


def roid_step(model, batch):
    """ROID (Marsden, Doebler, Yang, WACV 2024, "Universal Test-time Adaptation through Weight Ensembling, Diversity Weighting, and
    Prior Correction"; definition as recalled: unpinned) on one test batch: (1) TENT's forward and input-gradient-only backward with
    roid_loss, the soft likelihood ratio of the rows whose diversity against the running mean prediction is not below the batch's
    mean, weighted by exp(dn cn / tta_roid_temperature) and divided by ALL rows (clip tta_roid_clip, eps tta_roid_eps); the running
    mean moves at tta_probs_momentum; (2) one Adam step over A; (3) weight ensembling: A <- tta_roid_src_momentum A +
    (1 - tta_roid_src_momentum) source values after EVERY step, the continuous pull back to the source that needs neither source
    data nor a trigger (1: off; 0: A returns to the source after every batch); (4) with tta_roid_prior_correction the reported scores
    are softmax(out_m) reweighted by the smoothed batch-mean prediction and renormalised (forward only: it moves the scores under
    label shift, never A).  Not part of this method: ROID's consistency branch (a second pass on an augmented view under a
    symmetric cross-entropy).  Writes what tent_step writes and the running mean; tta_bn_prior, tta_bn_momentum and tta_episodic
    compose as for tent_step.  The scores come from this forward, before the update.  The step reads nothing back.
    last_tta: loss, y_hat_m, probs (the reported scores), probs_raw (softmax(out_m)), n_kept, kept, weight, marginal (pbar), prior
    (s), all on the device."""
    x, y = batch
    hp = model.hp
    with torch.inference_mode(False):
        st = _begin(model)
        out_m, loss, scores, info = adapting_pass(model, x, st, lambda z: roid_loss(
            z, st.ema, hp.tta_roid_temperature, hp.tta_roid_clip, hp.tta_roid_eps, hp.tta_probs_momentum, hp.tta_roid_prior_correction))
        st.adam_step(hp.tta_lr)
        st.ensemble(hp.tta_roid_src_momentum)
        _commit_memory(model)
        model.last_tta = dict(loss=loss, y_hat_m=out_m, probs=scores, probs_raw=info["probs"], n_kept=info["counts"][0], kept=info["keep"],
                              weight=info["w"], marginal=info["pbar"], prior=info["prior"])
        return model._score_test(scores, y)


def rotta_step(model, batch):
    """RoTTA (Yuan, Xie, Li, CVPR 2023, "Robust Test-Time Adaptation in Dynamic Scenarios"; definition as recalled: unpinned) on one
    test batch, the method made for a temporally correlated (class-ordered) stream: the adapting pass learns from a category-balanced
    BANK of tta_rotta_capacity test samples kept across batches on the device, not from the batch.  (1) A <-> teacher, which puts the
    EMA teacher into A; (2) the teacher's forward on the clean batch under no_grad, the ONE forward of the batch that writes the
    BatchNorm memory (tta_bn_momentum, RoTTA's robust BatchNorm: required): its logits give the reported scores; (3) the bank's
    bookkeeping moves over the batch, sample by sample (stil_rotta_bank_update: a sample whose pseudo-label's class holds less than
    its share N / K of the slots is added, or replaces the slot of highest score lambda_t / (1 + exp(-age / N)) + lambda_u unc / ln K
    among the classes of maximal occupancy, otherwise it replaces the highest-scoring slot of its own class; in both cases only when
    that score exceeds its own, lambda_t / 2 + lambda_u H / ln K), the accepted samples are gathered into the bank
    (stil_rotta_bank_store) and the memory is committed; (4) the teacher's forward on all N slots of the bank under no_grad, then
    A <-> teacher back; (5) the adapting pass on the AUGMENTED bank images (make_views: tta_view_policy, tta_view_seed, one view per
    slot) and the unchanged table rows with rotta_loss, the timeliness-weighted cross-entropy against the teacher's logits of the
    bank; (6) one Adam step over A if and only if the bank holds a sample; (7) teacher <- (1 - tta_rotta_nu) teacher + tta_rotta_nu A
    under the same gate: a batch whose bank is empty moves neither A, moments, step counts nor teacher.  The step reads nothing back.
    Unlike the published code, on purpose: (a) both passes over the bank normalise on the committed memory ALONE (rho = 0, nothing
    written): the rows stay independent, so empty, zero-filled slots cannot leak into the filled ones, and exactly one forward of
    the batch writes the memory -- the published robust BatchNorm updates on every forward; (b) the model adapts once per test
    batch, the published update_frequency being tied to the batch size.
    Writes what tent_step writes, the teacher and the bank; never the checkpoint's own EMA teacher.  The scores are the TEACHER's of
    the clean batch, before the update; they are formed by the launch bn_adapt_step makes (softmax_rows), so tta_rotta_nu 0 with
    tta_lr 0 reports bn_adapt's scores bit for bit.  tta_bn_prior composes in (2) as for tent_step; tta_episodic and reset_tta() empty
    the bank and return the teacher to the source; the views' generator runs on, as marginal_entropy_step's.
    last_tta: loss, y_hat_m (the teacher's logits of the batch), probs, probs_bank (stil_rotta_bank_update's own softmax of y_hat_m),
    accepted, slot_of, n_bank, bank_label, bank_age (after the batch), weight [N], all on the device, and draws, the host dict
    make_views rebuilds the views from."""
    x, y = batch
    hp = model.hp
    with torch.inference_mode(False):
        st = _begin(model)
        mem = _memory(model)
        x_img, x_tab = _inputs(model, x)
        st.ensure_bank(x_img, x_tab)
        st.exchange()
        zt_in = _score_forward(model, x_img, x_tab, update=True)
        probs = ops.softmax_rows(zt_in)
        upd = st.bank_update(zt_in, hp.tta_rotta_lambda_t, hp.tta_rotta_lambda_u)
        st.bank_store(x_img, x_tab)
        _commit_memory(model)
        on_memory = lambda: ops.bn_memory(mem, 0.0, mem.alpha, update=False)   # noqa: E731  the committed estimate alone, nothing written
        with torch.no_grad():
            zt_bank = _forward(model, st.bank_img, st.bank_tab, scope=on_memory())
        st.exchange()
        views, tab, draws = make_views(model, (st.bank_img, st.bank_tab))
        _, loss, _, info = adapting_pass(model, (views, tab), st, lambda z: rotta_loss(z, zt_bank, st.label, st.age, st.active, st.gate),
                                         update=False, scope=on_memory())
        st.adam_step(hp.tta_lr, mask=st.gate)
        st.move_teacher(hp.tta_rotta_nu)
        model.last_tta = dict(loss=loss, y_hat_m=zt_in, probs=probs, probs_bank=upd["probs"], accepted=upd["accepted"],
                              slot_of=upd["slot_of"], n_bank=upd["counts"][2], bank_label=st.label.clone(), bank_age=st.age.clone(),
                              weight=info["w"], draws=draws)
        return model._score_test(probs, y)


def bn_adapt_step(model, batch):
    """"BN adapt" / "Norm", the forward-only baseline of the TTA papers: the forward of the adapting pass (BatchNorm
    statistics of this batch, blended with the source statistics under tta_bn_prior; no MI-layer dropout) and its scores.
    No adapted set, no gradient, no optimiser, no TentState: without tta_bn_momentum reset_tta() and tta_episodic have nothing to
    act on; with it this forward is the one that updates the BatchNorm memory, which they return to the checkpoint's statistics.
    Writes acc_test / auc_test, last_tta and that memory, nothing else; Adam never runs."""
    x, y = batch
    with torch.inference_mode(False), torch.no_grad():
        model.setup_device()
        _begin_memory(model)
        out_m = _score_forward(model, *_inputs(model, x), update=True)
        _commit_memory(model)
        probs = ops.softmax_rows(out_m)
        model.last_tta = dict(y_hat_m=out_m, probs=probs)
        return model._score_test(probs, y)


def lame_step(model, batch):
    """LAME (Boudiaf, Mueller, Ben Ayed, Bertinetto, CVPR 2022, "Parameter-free Online Test-time Adaptation"; definition and defaults
    as recalled from the paper and its published code: unpinned) on one test batch, the forward-only method made for the streams on
    which adapting the model degrades (class-ordered, label-shifted; batches of two or three classes): the model and its
    normalisation stay at the source, the batch's output probabilities are corrected (`lame_correct`: tta_lame_knn neighbours per row
    under tta_lame_affinity, tta_lame_lambda, at most tta_lame_steps steps, tta_lame_tol).
    The forward: with tta_bn_prior and tta_bn_momentum both None it is the plain test_step's (eval mode, the checkpoint's statistics,
    forward_all(..., train=False)); with either set it is bn_adapt_step's (`_score_forward` with the update, then the memory's
    commit): the paper's "LAME on adapted statistics".  The features are the multimodal classifier's own input, cat(e_si, e_c, e_st).
    No TentState, no adapted set, no optimiser, no gradient: reset_tta() and tta_episodic act on the BatchNorm memory only, as for
    bn_adapt_step.  The step reads nothing back; a batch above LAME_MAX_ROWS rows is refused before its forward.
    Not part of this method: the "linear" affinity, LAME stacked on a method that adapts parameters, neighbours across batches.
    last_tta: y_hat_m, probs (Y, the reported scores), probs_raw (softmax(y_hat_m) by the launch test_step and bn_adapt_step make, so
    bit for bit theirs; lame_correct's own p, stil_entropy_rows' bits, differs from it in the last place), features, neighbours
    [B, tta_lame_knn] (-1: padding), steps [1], energy [tta_lame_steps] (NaN from `steps` on), all on the device."""
    x, y = batch
    hp = model.hp
    with torch.inference_mode(False), torch.no_grad():
        model.setup_device()
        x_img, x_tab = _inputs(model, x)
        if x_img.shape[0] > LAME_MAX_ROWS:
            raise ValueError(f"tta_method 'lame': a batch of {x_img.shape[0]} rows exceeds LAME_MAX_ROWS = {LAME_MAX_ROWS}")
        if hp.tta_bn_prior is None and hp.tta_bn_momentum is None:
            outs = model.model.forward_all((x_img, x_tab), train=False)
        else:
            _begin_memory(model)
            outs = _score_forward(model, x_img, x_tab, update=True, outputs="all")
            _commit_memory(model)
        out_m = outs[0].detach().contiguous()
        feats = torch.cat([outs[3], outs[9], outs[6]], dim=1)
        probs_raw = ops.softmax_rows(out_m)
        Y, _, info = lame_correct(out_m, feats, hp.tta_lame_knn, hp.tta_lame_affinity, hp.tta_lame_lambda, hp.tta_lame_steps, hp.tta_lame_tol)
        model.last_tta = dict(y_hat_m=out_m, probs=Y, probs_raw=probs_raw, features=feats, neighbours=info["nbr"], steps=info["steps"],
                              energy=info["energy"])
        return model._score_test(Y, y)


def dua_step(model, batch):
    """DUA (Mirza et al., CVPR 2022, "The norm must go on") on one test batch of B samples, B = 1 being the case it is made for.
    Forward only: no adapted set, no gradient, no optimiser, no TentState; the BatchNorm memory (BnMemory) is all that adapts.
    (1) V = tta_views augmented views of every sample (make_views; the augmenter and its generator, seeded by tta_view_seed, live in
    the memory); (2) one forward of encoder_imaging, the only part of the model with BatchNorm layers, on the B V views under
    no_grad in training mode: every layer normalises by the statistics of the views (rho = 1) and moves the memory by
    alpha_t = min(1, tta_bn_momentum x tta_bn_momentum_decay^t + tta_bn_momentum_min) towards them, UNBIASED variance, which is
    the training-mode rule of nn.BatchNorm2d the published code relies on; (3) commit; (4) the clean batch scored in eval mode on
    the memory alone (rho = 0, nothing written); (5) softmax_rows.  tta_bn_prior has no say here.  With B > 1 the samples share one
    update.  The published setting is a configuration, not the default: batches of 1, tta_views 64, tta_bn_momentum 0.1,
    tta_bn_momentum_decay 0.94, tta_bn_momentum_min 0.005 (as recalled: unpinned), not episodic.
    Unlike the paper, on purpose: the views come from this project's own transform families (tta_view_policy), not the paper's
    augmentation list; and make_views repeats the table row of a sample unchanged for its views (the statistics pass itself reads
    the images only).
    last_tta: y_hat_m, probs [B, K] of the scoring forward, on the device; alpha (alpha_t of this batch, a float) and draws, the
    host dict make_views rebuilds the views from."""
    x, y = batch
    with torch.inference_mode(False), torch.no_grad():
        model.setup_device()
        mem = _begin_memory(model)
        x_img, x_tab = _inputs(model, x)
        views, _, draws = make_views(model, (x_img, x_tab))
        model.flat.refresh_layouts(student=True, teacher=False)
        with ops.frozen_bn_stats(), ops.bn_memory(mem, 1.0, mem.alpha, unbiased=True, update=True):
            model.model.encoder_imaging.run(views, True, None)
        mem.commit()
        with ops.frozen_bn_stats(), ops.bn_memory(mem, 0.0, mem.alpha, update=False):
            out_m = model.model.forward_all((x_img, x_tab), train=True, mi_masks=None)[0]
        probs = ops.softmax_rows(out_m)
        model.last_tta = dict(y_hat_m=out_m, probs=probs, alpha=mem.alpha, draws=draws)
        return model._score_test(probs, y)


STEPS = {"tent": tent_step, "eata": eata_step, "bn_adapt": bn_adapt_step, "shot_im": shot_im_step,
         "marginal_entropy": marginal_entropy_step, "deyo": deyo_step, "sar": sar_step, "dua": dua_step,
         "read": read_step, "cgpl": cgpl_step, "roid": roid_step, "rotta": rotta_step, "lame": lame_step}   # tta_method -> STiLModel.test_step's body
METHODS = (None,) + tuple(STEPS)


# ---------------------------------------------------------------------------------------------- EATA's Fisher estimate
def estimate_fisher(model, batches, max_batches: Optional[int] = None) -> int:
    """EATA's Fisher estimate of A at the CURRENT parameters (call it on the source model: before the first adapted batch
    or after reset_tta()), from `batches` of source-like data laid out as test_step's (labels unused): per batch, the
    adapting pass with y_r = argmax_k out_m[r] (first maximum), l = mean_r CE(out_m[r], y_r), g = dl/dA;
    F = (1/N) sum over the batches of g^2.  No parameter, BatchNorm buffer, teacher, prototype or training slab is written,
    and Adam never runs.  `batches` without a len() and no max_batches are materialised first (N scales every term).
    -> the number of batches used."""
    with torch.inference_mode(False):
        st = _eata_state(model)
        try:
            N = len(batches)
        except TypeError:
            N = None
        if max_batches is not None:
            N = int(max_batches) if N is None else min(N, int(max_batches))
        if N is None:
            batches = list(batches)
            N = len(batches)
        if N < 1:
            raise ValueError("estimate_tta_fisher needs at least one batch")
        st.new_fisher()
        seen = 0
        for batch in batches:
            if seen >= N:
                break
            adapting_pass(model, batch[0], st, argmax_ce, update=False)
            st.fisher_accum(1.0 / N)
            seen += 1
        if seen < N:  # an iterable shorter than max_batches: the mean is over the batches seen
            if seen == 0:
                st.fisher = None
                raise ValueError("estimate_tta_fisher needs at least one batch")
            st.fisher.mul_(N / seen)
    return seen


def fisher_state(model) -> Dict[str, torch.Tensor]:
    """{state_dict name of a member of A: its Fisher estimate} (copies; {} when none is loaded).  Not part of state_dict(),
    whose keys are the reference's."""
    st = model._tent
    if getattr(st, "fisher", None) is None:
        return {}
    return dict(zip(param_names(model), st.fisher_tensors()))


def load_fisher(model, fisher: Dict[str, torch.Tensor]):
    """Load a Fisher estimate saved by fisher_state(); the keys must be exactly param_names()."""
    names = param_names(model)
    if set(fisher.keys()) != set(names):
        raise ValueError(f"Fisher estimate for {len(fisher)} tensors, the adapted set has {len(names)}: "
                         f"missing {sorted(set(names) - set(fisher))[:3]}, unexpected {sorted(set(fisher) - set(names))[:3]}")
    with torch.inference_mode(False):
        _eata_state(model).load_fisher([fisher[n] for n in names])
