"""cenet_amd.ops.dseb_loss — DSEB combine (dseb.py:40-50,63-76,156-163) and the fused segmentation loss (utils/core.py:44-131,161-188).
Part of the cenet_amd.ops package (split by operator family in round 6; `from cenet_amd import ops` re-exports the names in `__all__`)."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import Tensor
from torch.autograd import Function

from .. import kern
from .infra import _c, _empty, _zeros, grad_buf


# =====================================================================================================
# DSEB combine (dseb.py:40-50,63-76,156-163)
# =====================================================================================================
class DsebCombineFn(Function):
    """z = ycoef*y + w[c]*edge(y, recon_s) + diff*y; `recons[s]` is None for scale 1.0 (e_s == 0); diff may be None."""

    @staticmethod
    def forward(ctx, y, w, diff, ycoef, n, *recons):
        y, diff = _c(y), _c(diff)
        recons = [_c(r) for r in recons]
        B, Cn = y.shape[:2]
        HW = y.numel() // (B * Cn)
        z = torch.empty_like(y)
        kern.dseb_combine_fwd(y, recons, n, w, diff, ycoef, z, B, Cn, HW)
        ctx.save_for_backward(y, w, diff, *[r for r in recons if r is not None])
        ctx.ycoef = ycoef
        ctx.mask = [r is not None for r in recons]
        ctx.refs = (w,)
        ctx.n = n
        return z

    @staticmethod
    def backward(ctx, g):
        y, w, diff = ctx.saved_tensors[:3]
        present = list(ctx.saved_tensors[3:])
        recons, it = [], iter(present)
        for m in ctx.mask:
            recons.append(next(it) if m else None)
        g = _c(g)
        B, Cn = y.shape[:2]
        HW = y.numel() // (B * Cn)
        dy = torch.empty_like(y)
        ddiff = torch.empty_like(y) if diff is not None else None
        drs = [torch.empty_like(y) if r is not None else None for r in recons]
        dw = grad_buf(ctx.refs[0])
        if dw is None:
            dw = _zeros(w.shape, y)
        kern.dseb_combine_bwd(y, recons, ctx.n, w, diff, ctx.ycoef, g, dy, drs, ddiff, dw, B, Cn, HW)
        return (dy, None, ddiff, None, None) + tuple(drs)


def dseb_combine(y, w, diff, recons: Sequence[Optional[Tensor]], ycoef: float = 2.0):
    return DsebCombineFn.apply(y, w, diff, ycoef, len(recons), *recons)


# =====================================================================================================
# loss (utils/core.py:44-80,161-188)
# =====================================================================================================
class DiceCELossFn(Function):
    """w_dice * Dice + w_ce * CE + w_bd * BoundaryDoU in one pass over the logits each way (core.py:44-131,161-188)."""

    @staticmethod
    def forward(ctx, logits, labels, w_dice, w_ce, w_bd=0.0):
        logits, labels = _c(logits), _c(labels)
        B, K = logits.shape[:2]
        H, W = (logits.shape[2], logits.shape[3]) if logits.dim() == 4 else (1, logits.numel() // (B * K))
        acc = _empty((16384,), logits)  # CENET_LOSS_ACC_FLOATS (include/cenet_hip.h): replicated partial sums, one value per line
        loss = _empty((1,), logits)
        kern.seg_loss_fwd(logits, labels, acc, loss, B, K, H, W, w_dice, w_ce, w_bd)
        ctx.save_for_backward(logits, labels, acc)
        ctx.cfg = (w_dice, w_ce, w_bd, H, W)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        logits, labels, acc = ctx.saved_tensors
        w_dice, w_ce, w_bd, H, W = ctx.cfg
        B, K = logits.shape[:2]
        g = _c(g).reshape(1)
        d = torch.empty_like(logits)
        kern.seg_loss_bwd(logits, labels, acc, g, d, B, K, H, W, w_dice, w_ce, w_bd)
        return d, None, None, None, None


def dice_ce_loss(logits, labels, w_dice=0.5, w_ce=0.5, w_boundary=0.0):
    return DiceCELossFn.apply(logits, labels, w_dice, w_ce, w_boundary)


class SegLossExFn(Function):
    """The loss with options (csrc/seg_loss_ex.hip): class weights, ignore_index, a Jaccard term, DiceLoss(softmax=False).
    Forward = one pass that stores a row of partial sums per workgroup + a one-workgroup launch that adds the rows in a fixed
    order (no float atomics: bitwise reproducible); backward = one launch.  cw: [2K] device weights (Dice, then CE) or None."""

    @staticmethod
    def forward(ctx, logits, labels, cw, cfg):
        logits, labels = _c(logits), _c(labels)
        B, K, H, W = logits.shape
        ws = _empty((kern.seg_loss_ex_ws_floats(B, K, H, W),), logits)
        loss = _empty((1,), logits)
        kern.seg_loss_ex_fwd(logits, labels, cw, ws, loss, B, K, H, W, *cfg)
        ctx.save_for_backward(logits, labels, ws)
        ctx.cw, ctx.cfg = cw, cfg
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        logits, labels, ws = ctx.saved_tensors
        B, K, H, W = logits.shape
        d = torch.empty_like(logits)
        kern.seg_loss_ex_bwd(logits, labels, ctx.cw, ws, _c(g).reshape(1), d, B, K, H, W, *ctx.cfg)
        return d, None, None, None


_CLASS_WEIGHTS: dict = {}  # (device, K, Dice weights, CE weights) -> the [2K] device buffer uploaded for them


def class_weight_buffer(K: int, dice_class_weights, ce_class_weights, device):
    """The [2K] fp32 buffer (Dice weights, then CE weights) the loss kernels read, or None when both are None (all ones).
    Sequences of K numbers are uploaded once per (device, values) and cached.  Device tensors are used as they are when they
    are the two halves of one contiguous buffer (a later write into it is seen by the next launch, a graph replay included);
    any other pair of tensors, or a tensor with a sequence / None, is packed by one device copy per call."""
    wd, wc = dice_class_weights, ce_class_weights
    if wd is None and wc is None:
        return None
    device = torch.device(device)
    for name, w in (("dice_class_weights", wd), ("ce_class_weights", wc)):
        if w is None:
            continue
        n = w.numel() if isinstance(w, Tensor) else len(w)
        if n != K:
            raise ValueError(f"{name}: {n} weights for {K} classes")
        if isinstance(w, Tensor) and (w.dtype != torch.float32 or w.device != device):
            raise ValueError(f"{name}: expected an fp32 tensor on {device}, got {w.dtype} on {w.device}")
    if isinstance(wd, Tensor) or isinstance(wc, Tensor):
        if (isinstance(wd, Tensor) and isinstance(wc, Tensor) and wd.is_contiguous() and wc.is_contiguous()
                and wd.untyped_storage().data_ptr() == wc.untyped_storage().data_ptr()
                and wc.storage_offset() == wd.storage_offset() + K):
            return wd.detach().reshape(-1).as_strided((2 * K,), (1,), wd.storage_offset())
        def half(w):
            if isinstance(w, Tensor):
                return w.detach().reshape(-1)
            return class_weight_buffer(K, [1.0] * K if w is None else w, None, device)[:K]

        return torch.cat([half(wd), half(wc)])
    key = (str(device), K, None if wd is None else tuple(float(x) for x in wd), None if wc is None else tuple(float(x) for x in wc))
    buf = _CLASS_WEIGHTS.get(key)
    if buf is None:
        ones = [1.0] * K
        vals = list(key[2] if wd is not None else ones) + list(key[3] if wc is not None else ones)
        buf = _CLASS_WEIGHTS[key] = torch.tensor(vals, dtype=torch.float32).to(device)
    return buf


def seg_loss(logits, labels, *, w_dice=0., w_ce=0., w_boundary=0., w_jaccard=0., dice_class_weights=None,
             ce_class_weights=None, ignore_index=None, jaccard_smooth=1.0, from_probs=False):
    """loss = w_dice Dice + w_ce CE + w_boundary BoundaryDoU + w_jaccard Jaccard on logits [B,K,H,W] (fp32 or bf16) and labels
    [B,H,W] (class ids as floats, each in [0,K) or equal to ignore_index), sums over the whole batch (include/cenet_hip.h spells
    the terms out).  dice_class_weights: DiceLoss.forward's `weight` (core.py:67-80); ce_class_weights / ignore_index:
    torch.nn.CrossEntropyLoss(weight, ignore_index), mean reduction — a batch whose every pixel is ignored gives NaN, as torch
    does; ignore_index also masks the Dice and Jaccard sums as `flatten` (utils/utils.py:39-50) does.  from_probs:
    DiceLoss(softmax=False), the input holds probabilities and the gradient is with respect to them.  The gradient goes to
    `logits` only and is exactly 0 at ignored pixels."""
    if logits.dim() != 4 or labels.shape != (logits.shape[0],) + tuple(logits.shape[2:]):
        raise ValueError(f"seg_loss: logits [B,K,H,W] and labels [B,H,W], got {tuple(logits.shape)} and {tuple(labels.shape)}")
    if from_probs and (w_ce != 0 or w_boundary != 0 or w_jaccard != 0):
        raise ValueError("seg_loss: from_probs is DiceLoss(softmax=False): only the Dice term is defined on probabilities")
    if ignore_index is not None and w_boundary != 0:
        raise NotImplementedError("seg_loss: BoundaryDoU with ignore_index (a boundary count over a mask with holes is not "
                                  "defined by the reference)")
    cw = class_weight_buffer(logits.shape[1], dice_class_weights, ce_class_weights, logits.device)
    cfg = (float(w_dice), float(w_ce), float(w_boundary), float(w_jaccard), float(jaccard_smooth),
           None if ignore_index is None else int(ignore_index), bool(from_probs))
    return SegLossExFn.apply(logits, labels, cw, cfg)


# =====================================================================================================
# distance-map losses (csrc/edt.hip cenet_dist_maps_*, csrc/dist_loss.hip; not in the reference)
# =====================================================================================================
def _dist_shapes(logits, labels, what):
    if logits is not None and logits.dim() != 4:
        raise ValueError(f"{what}: logits [B,K,H,W] expected, got {tuple(logits.shape)}")
    if labels is not None and labels.dim() != 3:
        raise ValueError(f"{what}: labels [B,H,W] expected, got {tuple(labels.shape)}")
    if logits is not None and labels is not None and labels.shape != (logits.shape[0],) + tuple(logits.shape[2:]):
        raise ValueError(f"{what}: logits [B,K,H,W] and labels [B,H,W], got {tuple(logits.shape)} and {tuple(labels.shape)}")
    for t in (logits, labels):
        if t is not None and not t.is_cuda and not kern._lib.is_hostsim():
            raise ValueError(f"{what}: the distance-map losses run on the MI355X only: tensor is not on a CUDA/HIP device")


def distance_maps(labels: Tensor, K: int) -> Tensor:
    """labels [B,H,W] (class ids as floats) -> int32 [B,K-1,H,W]: for every foreground class c the exact squared Euclidean
    distance of each pixel to the nearest pixel of the other kind of the mask {label == c} (inside: to the nearest pixel
    outside, outside: to the nearest pixel of the class); 0 on a plane whose class is absent or fills it.  A handful of launches,
    no sync, the same bits on every run."""
    _dist_shapes(None, labels, "distance_maps")
    B, H, W = labels.shape
    labels = _c(labels.float())
    ws = _empty((kern.dist_maps_ws_ints(B, K, H, W),), labels, torch.int32)
    d2 = _empty((B, K - 1, H, W), labels, torch.int32)
    kern.dist_maps_labels(labels, ws, d2, B, K, H, W)
    return d2


def pred_distance_maps(logits: Tensor) -> Tensor:
    """logits [B,K,H,W] (fp32 or bf16) -> the same maps for the thresholded prediction {softmax_c > 1/2}, c = 1 .. K-1"""
    _dist_shapes(logits, None, "pred_distance_maps")
    B, K, H, W = logits.shape
    logits = _c(logits.detach())
    ws = _empty((kern.dist_maps_ws_ints(B, K, H, W),), logits, torch.int32)
    d2 = _empty((B, K - 1, H, W), logits, torch.int32)
    kern.dist_maps_logits(logits, ws, d2, B, K, H, W)
    return d2


class DistLossFn(Function):
    """w[0] * surface loss + w[1] * Hausdorff-DT loss (csrc/dist_loss.hip; include/cenet_hip.h spells the terms out).  The maps
    are built inside the forward (the prediction's only with the Hausdorff term) and kept for the backward as constants.
    w: fp32 [2] on the device, read by the kernels; the gradient goes to `logits` only."""

    @staticmethod
    def forward(ctx, logits, labels, w, surface, hausdorff):
        logits, labels = _c(logits), _c(labels)
        B, K, H, W = logits.shape
        d2g = distance_maps(labels, K)
        d2p = pred_distance_maps(logits) if hausdorff else None
        ws = _empty((kern.dist_loss_ws_floats(B, K, H, W),), logits)
        loss = _empty((1,), logits)
        kern.dist_loss_fwd(logits, labels, d2g, d2p, w, ws, loss, B, K, H, W, surface, hausdorff)
        ctx.save_for_backward(logits, labels, d2g, w, *(() if d2p is None else (d2p,)))
        ctx.cfg = (surface, hausdorff)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        logits, labels, d2g, w, *rest = ctx.saved_tensors
        surface, hausdorff = ctx.cfg
        B, K, H, W = logits.shape
        d = torch.empty_like(logits)
        kern.dist_loss_bwd(logits, labels, d2g, rest[0] if rest else None, w, _c(g).reshape(1).float(), d, B, K, H, W, surface,
                           hausdorff)
        return d, None, None, None, None


_DIST_WEIGHTS: dict = {}  # (device, w_surface, w_hausdorff) -> the [2] device buffer uploaded for them


def dist_loss(logits, labels, weights, *, surface=True, hausdorff=True):
    """loss = weights[0] * surface loss + weights[1] * Hausdorff-DT loss (alpha = 2) on logits [B,K,H,W] (fp32 or bf16) and labels
    [B,H,W] (class ids as floats in [0,K)), both over the foreground classes 1 .. K-1.  weights: a pair of floats, uploaded once
    per pair of values and cached, or an fp32 [2] tensor on the logits' device, used as it is (a later write into it is seen by
    the next call, a graph replay included).  surface / hausdorff: which terms are present; an absent term costs nothing — without
    the Hausdorff term the prediction's distance maps are not built."""
    if not (surface or hausdorff):
        raise ValueError("dist_loss: neither the surface nor the Hausdorff term is present")
    _dist_shapes(logits, labels, "dist_loss")
    if isinstance(weights, Tensor):
        if weights.dtype != torch.float32 or weights.device != logits.device or weights.numel() != 2 or not weights.is_contiguous():
            raise ValueError(f"dist_loss: weights: a contiguous fp32 [2] tensor on {logits.device} expected, got "
                             f"{weights.dtype} {tuple(weights.shape)} on {weights.device}")
        w = weights.detach().reshape(2)
    else:
        if len(weights) != 2:
            raise ValueError(f"dist_loss: weights: (surface, hausdorff) expected, got {len(weights)} values")
        key = (str(logits.device), float(weights[0]), float(weights[1]))
        w = _DIST_WEIGHTS.get(key)
        if w is None:
            w = _DIST_WEIGHTS[key] = torch.tensor(key[1:], dtype=torch.float32).to(logits.device)
    return DistLossFn.apply(logits, labels.float(), w, bool(surface), bool(hausdorff))


# =====================================================================================================
# Lovasz-Softmax (Berman, Triki, Blaschko 2018; csrc/lovasz.hip; not in the reference)
# =====================================================================================================
class LovaszFn(Function):
    """The Lovasz-Softmax loss (include/cenet_hip.h spells it out).  Forward: keys, the batched radix sort, integer ranks and the
    coefficients a = dloss / dp [B,K,H,W] fp32, which the backward — one launch — applies.  The workspace comes from the caching
    allocator and is free again after the forward; nothing synchronises.  The gradient goes to `inputs` only."""

    @staticmethod
    def forward(ctx, inputs, target, per_image, classes_all, ignore_index, from_probs):
        inputs, target = _c(inputs), _c(target)
        B, K, H, W = inputs.shape
        ws = _empty((kern.lovasz_ws_bytes(B, K, H, W, per_image) // 4,), inputs, torch.int32)
        coef = _empty((B, K, H, W), inputs)
        loss = _empty((1,), inputs)
        kern.lovasz_fwd(inputs, target, ws, coef, loss, B, K, H, W, per_image, classes_all, ignore_index, from_probs)
        ctx.save_for_backward(inputs, coef)
        ctx.from_probs = from_probs
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        inputs, coef = ctx.saved_tensors
        B, K, H, W = inputs.shape
        d = torch.empty_like(inputs)
        kern.lovasz_bwd(inputs, coef, _c(g).reshape(1).float(), d, B, K, H, W, ctx.from_probs)
        return d, None, None, None, None, None


def lovasz_softmax(inputs, target, *, per_image=False, classes="present", ignore_index=None, from_probs=False):
    """The Lovasz-Softmax loss on inputs [B,K,H,W] (fp32 or bf16 logits; probabilities with from_probs) and target [B,H,W] (class
    ids as floats): per class the pixels ordered by descending error |[target == c] - p_c| — equal errors by ascending pixel
    index, so the result is a function of the inputs alone — and the errors weighted by the increments of the Jaccard loss along
    that order.  classes: "present" (the mean over the classes that occur in the labels) or "all"; per_image: the loss of every
    image on its own, then the mean over the images; ignore_index: pixels with that label are in no class and get no gradient."""
    if classes not in ("present", "all"):
        raise ValueError(f"lovasz_softmax: classes is 'present' or 'all', got {classes!r}")
    if inputs.dim() != 4 or target.shape != (inputs.shape[0],) + tuple(inputs.shape[2:]):
        raise ValueError(f"lovasz_softmax: inputs [B,K,H,W] and target [B,H,W] expected, got {tuple(inputs.shape)} and "
                         f"{tuple(target.shape)}")
    return LovaszFn.apply(inputs, target.float(), bool(per_image), classes == "all",
                          None if ignore_index is None else int(ignore_index), bool(from_probs))


def lovasz_order(errors: Tensor) -> Tensor:
    """errors [S,n] fp32, non-negative -> int32 [S,n]: the stable descending order of every row, numpy's
    argsort(-errors, kind="stable") — the sort of lovasz_softmax on its own"""
    if errors.dim() != 2 or errors.dtype != torch.float32:
        raise ValueError(f"lovasz_order: errors [S,n] fp32 expected, got {errors.dtype} {tuple(errors.shape)}")
    S, n = errors.shape
    errors = _c(errors)
    ws = _empty((kern.lovasz_order_ws_bytes(S, n) // 4,), errors, torch.int32)
    perm = _empty((S, n), errors, torch.int32)
    kern.lovasz_order(errors, ws, perm, S, n)
    return perm


# =====================================================================================================
# Top-k cross-entropy (hard-pixel mining, the CE half of nnU-Net's DC_and_topk_loss; csrc/topk_ce.hip; not in the reference)
# =====================================================================================================
class TopKCEFn(Function):
    """The top-k cross-entropy (include/cenet_hip.h spells it out).  Forward: keys, the radix select of the threshold, the tie
    rank and the weights wgt [B,H,W] fp32, which the backward — one launch — applies.  kpercent is one fp32 on the device, read
    there.  The workspace comes from the caching allocator and is free again after the forward; nothing synchronises.  The
    gradient goes to `logits` only."""

    @staticmethod
    def forward(ctx, logits, target, kpercent, per_image, ignore_index):
        logits, target = _c(logits), _c(target)
        B, K, H, W = logits.shape
        ws = _empty((kern.topk_ce_ws_bytes(B, H, W, per_image) // 4,), logits, torch.int32)
        wgt = _empty((B, H, W), logits)
        loss = _empty((1,), logits)
        kern.topk_ce_fwd(logits, target, kpercent, ws, wgt, loss, B, K, H, W, per_image, ignore_index)
        ctx.save_for_backward(logits, target, wgt)
        ctx.ignore_index = ignore_index
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        logits, target, wgt = ctx.saved_tensors
        B, K, H, W = logits.shape
        d = torch.empty_like(logits)
        kern.topk_ce_bwd(logits, target, wgt, _c(g).reshape(1).float(), d, B, K, H, W, ctx.ignore_index)
        return d, None, None, None, None


_TOPK_PERCENT = {}  # (device, value) -> the value as one fp32 on the device: a Python number is uploaded once per value


def _topk_percent(k, ref: Tensor) -> Tensor:
    if isinstance(k, Tensor):
        if k.numel() != 1 or k.dtype != torch.float32 or k.device != ref.device:
            raise ValueError(f"topk_ce: k as a tensor is one fp32 on the logits' device, got {k.dtype} {tuple(k.shape)} on {k.device}")
        return _c(k).reshape(1)
    k = float(k)
    if not 0.0 < k <= 100.0:
        raise ValueError(f"topk_ce: k is a percentage, 0 < k <= 100, got {k}")
    buf = _TOPK_PERCENT.get((ref.device, k))
    if buf is None:
        buf = _TOPK_PERCENT[(ref.device, k)] = torch.tensor([k], dtype=torch.float32, device=ref.device)
    return buf


def topk_ce(inputs, target, k=10.0, *, per_image=False, ignore_index=None):
    """The top-k cross-entropy on inputs [B,K,H,W] (fp32 or bf16 logits) and target [B,H,W] (class ids as floats): the mean of the
    cross-entropy over the k % of the valid pixels with the largest loss, m = max(1, floor(n_valid k / 100)) of them — equal
    losses by ascending pixel index, so the result is a function of the inputs alone.  k: a Python number (0 < k <= 100, uploaded
    once per value) or a one-element fp32 tensor on the device, which is read there in place (a schedule can write into it, a
    captured graph included; the device clamps it into (0, 100]).  per_image: every image on its own, then the mean over the
    images that have a valid pixel; ignore_index: pixels with that label (and pixels whose label is no class) are in no count and
    get no gradient.  No valid pixel at all: 0."""
    if inputs.dim() != 4 or target.shape != (inputs.shape[0],) + tuple(inputs.shape[2:]):
        raise ValueError(f"topk_ce: inputs [B,K,H,W] and target [B,H,W] expected, got {tuple(inputs.shape)} and "
                         f"{tuple(target.shape)}")
    return TopKCEFn.apply(inputs, target.float(), _topk_percent(k, inputs), bool(per_image),
                          None if ignore_index is None else int(ignore_index))


def topk_mask(values: Tensor, m) -> Tensor:
    """values [S,n] fp32, non-negative; m: an int or S ints (a sequence or an int32 tensor) -> uint8 [S,n], 1 on the m[s] largest
    values of row s, equal values by ascending index — the selection of topk_ce on its own"""
    if values.dim() != 2 or values.dtype != torch.float32:
        raise ValueError(f"topk_mask: values [S,n] fp32 expected, got {values.dtype} {tuple(values.shape)}")
    S, n = values.shape
    values = _c(values)
    if not isinstance(m, Tensor):
        m = torch.tensor([int(m)] * S if isinstance(m, int) else [int(v) for v in m], dtype=torch.int32)
    if m.numel() != S:
        raise ValueError(f"topk_mask: {m.numel()} counts for {S} rows")
    m = _c(m.to(device=values.device, dtype=torch.int32))
    ws = _empty((kern.topk_mask_ws_bytes(S, n) // 4,), values, torch.int32)
    mask = _empty((S, n), values, torch.uint8)
    kern.topk_mask(values, m, ws, mask, S, n)
    return mask


__all__ = ["DsebCombineFn", "dseb_combine", "DiceCELossFn", "dice_ce_loss", "SegLossExFn", "class_weight_buffer", "seg_loss",
           "distance_maps", "pred_distance_maps", "DistLossFn", "dist_loss", "LovaszFn", "lovasz_softmax", "lovasz_order",
           "TopKCEFn", "topk_ce", "topk_mask"]
