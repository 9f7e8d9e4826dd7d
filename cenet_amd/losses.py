"""Loss interface mirroring reference src/utils/core.py:161-188 (`Criterion(num_classes, args)(outputs, labels)`).

Dice, cross-entropy and BoundaryDoULoss (core.py:44-131) are terms of ONE fused HIP kernel each way
(cenet_amd.ops.dice_ce_loss): the per-class sums they share are accumulated once, the boundary-pixel counts of
BoundaryDoULoss come from the same pass over the labels, and the backward is a single kernel for any weighting.

Class weights (DiceLoss.forward's `weight`, CrossEntropyLoss's `weight`), `ignore_index`, JaccardLoss (core.py:134-158) and
DiceLoss(softmax=False) go through cenet_amd.ops.seg_loss (csrc/seg_loss_ex.hip): the same one pass, partial sums stored per
workgroup and added in a fixed order instead of float atomics.  A call that uses none of them keeps the first path.

The distance-map losses `surface` (Kervadec et al. 2019) and `hausdorff` (Karimi & Salcudean 2019, alpha = 2) go through
cenet_amd.ops.dist_loss: the exact distance maps of every label map (and, for `hausdorff`, of the thresholded prediction) are
built on the device inside the step (csrc/edt.hip) and one fused kernel each way reads them (csrc/dist_loss.hip).  They are
not in the reference; a Criterion that names neither launches nothing of this.

`lovasz` (LovaszSoftmaxLoss; Berman, Triki, Blaschko 2018) goes through cenet_amd.ops.lovasz_softmax: the loss that optimises
the Jaccard index itself needs every pixel's rank among the errors of its class, which csrc/lovasz.hip gets from a batched stable
radix sort on the device.  Not in the reference either, and a Criterion that does not name it launches nothing of it.

`topk` (TopKCrossEntropyLoss; hard-pixel mining, the CE half of nnU-Net's DC_and_topk_loss) goes through cenet_amd.ops.topk_ce:
the cross-entropy averaged over the k % of pixels with the largest loss, which csrc/topk_ce.hip finds with a radix select on the
device.  Not in the reference, and a Criterion that does not name it launches nothing of it.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops


class DiceLoss(nn.Module):
    """core.py:44-80.  `weight`: K numbers (uploaded once per set of values) or a device tensor; softmax=False: `inputs`
    already holds probabilities and receives the gradient directly."""

    def __init__(self, n_classes):
        super().__init__()
        self.n_classes = n_classes

    def forward(self, inputs, target, weight=None, softmax=False):
        if softmax and weight is None:
            return ops.dice_ce_loss(inputs, target, 1.0, 0.0)
        return ops.seg_loss(inputs, target, w_dice=1.0, dice_class_weights=weight, from_probs=not softmax)


class BoundaryDoULoss(nn.Module):
    """core.py:83-131 (no hard-coded .cuda(): the boundary counts are computed on the device that holds the labels)."""

    def __init__(self, n_classes):
        super().__init__()
        self.n_classes = n_classes

    def forward(self, inputs, target):
        return ops.dice_ce_loss(inputs, target, 0.0, 0.0, 1.0)


class JaccardLoss(nn.Module):
    """core.py:134-158: mean over the classes of 1 - (I + smooth) / (union + smooth) on the pixels whose label is not
    ignore_index (`flatten`, utils/utils.py:39-50).  input [B,K,H,W] logits, target [B,H,W] class ids as floats."""

    def __init__(self, ignore_index=255, smooth=1.0):
        super().__init__()
        self.ignore_index = ignore_index
        self.smooth = smooth

    def forward(self, input, target):
        return ops.seg_loss(input, target, w_jaccard=1.0, ignore_index=self.ignore_index, jaccard_smooth=self.smooth)


class SurfaceLoss(nn.Module):
    """The surface (boundary) loss of Kervadec et al. 2019 over the foreground classes: the mean of softmax probability times
    the signed distance to the ground-truth contour (+ distance outside the class, -(distance - 1) inside).  inputs [B,K,H,W]
    logits, target [B,H,W] class ids as floats."""

    def __init__(self, n_classes):
        super().__init__()
        self.n_classes = n_classes

    def forward(self, inputs, target):
        return ops.dist_loss(inputs, target, (1.0, 0.0), surface=True, hausdorff=False)


class HausdorffDTLoss(nn.Module):
    """The distance-transform Hausdorff loss of Karimi & Salcudean 2019 with alpha = 2 over the foreground classes: the mean of
    (p - g)^2 times the sum of the squared distance maps of the ground truth and of the prediction thresholded at 1/2."""

    def __init__(self, n_classes):
        super().__init__()
        self.n_classes = n_classes

    def forward(self, inputs, target):
        return ops.dist_loss(inputs, target, (0.0, 1.0), surface=False, hausdorff=True)


class LovaszSoftmaxLoss(nn.Module):
    """The Lovasz-Softmax loss of Berman, Triki, Blaschko 2018 (Alg. 1), the tight convex surrogate of the Jaccard index: per
    class the errors |[target == c] - softmax_c| in descending order, weighted by the increments of the Jaccard loss along that
    order.  classes: "present" (mean over the classes that occur) or "all"; per_image: per image, then the mean over the images;
    ignore_index: that label is in no class.  inputs [B,K,H,W] logits, target [B,H,W] class ids as floats."""

    def __init__(self, per_image=False, classes="present", ignore_index=None):
        super().__init__()
        if classes not in ("present", "all"):
            raise ValueError(f"LovaszSoftmaxLoss: classes is 'present' or 'all', got {classes!r}")
        self.per_image, self.classes, self.ignore_index = bool(per_image), classes, ignore_index

    def forward(self, inputs, target):
        return ops.lovasz_softmax(inputs, target, per_image=self.per_image, classes=self.classes, ignore_index=self.ignore_index)


class TopKCrossEntropyLoss(nn.Module):
    """The top-k cross-entropy: the mean of the cross-entropy over the k % of the valid pixels with the largest loss (at least
    one), equal losses by ascending pixel index.  k: a percentage, 0 < k <= 100, kept in the buffer `percent` ([1] fp32, follows
    .to()) and read on the device; per_image: every image on its own, then the mean over the images; ignore_index: that label
    is in no count.  No class weights, no probability threshold (OHEM's thresh / min_kept), logits only.
    inputs [B,K,H,W] logits, target [B,H,W] class ids as floats."""

    def __init__(self, k=10.0, per_image=False, ignore_index=None):
        super().__init__()
        if not 0.0 < float(k) <= 100.0:
            raise ValueError(f"TopKCrossEntropyLoss: k is a percentage, 0 < k <= 100, got {k}")
        self.per_image, self.ignore_index = bool(per_image), ignore_index
        self.register_buffer("percent", torch.tensor([float(k)], dtype=torch.float32))

    def forward(self, inputs, target):
        return ops.topk_ce(inputs, target, self.percent, per_image=self.per_image, ignore_index=self.ignore_index)


def _class_weights(value, K, name):
    """None, a comma string or a sequence of K floats -> None or a list of K floats"""
    if value is None:
        return None
    vals = [float(v) for v in (value.split(',') if isinstance(value, str) else value)]
    if len(vals) != K:
        raise ValueError(f"{name}: {len(vals)} weights for {K} classes")
    return vals


class Criterion(nn.Module):
    """core.py:161-188 with `jaccard` as a fourth loss name and four optional attributes of `args` (each read with a default):
    dice_class_weights / ce_class_weights (comma string or sequence of num_classes floats), ignore_index (int) and
    jaccard_smooth (default 1.0).  Without any of them and without `jaccard` the call is ops.dice_ce_loss as before.
    The class weights are uploaded at construction into the buffer `class_weights` ([2K]: Dice, then CE), which follows
    .to(); writing new values into it takes effect at the next call, inside a captured graph too.
    CE over a batch whose every pixel is ignored is NaN (as torch.nn.CrossEntropyLoss); boundary + ignore_index is refused.
    `surface` and `hausdorff` (SurfaceLoss, HausdorffDTLoss) are two more loss names: their term is added to the total of the
    other names (which is not computed when none of them is named).  Their weights live in the buffer `dist_weights` ([2]:
    surface, hausdorff), read on the device by every call; set_dist_weights() writes into it without a sync, so a weight
    schedule costs a captured step no recapture.  Either name with ignore_index is refused, as boundary is.
    `lovasz` (LovaszSoftmaxLoss) is one more name whose term, times its weight of loss_weights, is added in the same way; it
    honours ignore_index and reads two more optional attributes, lovasz_per_image (default False) and lovasz_classes (default
    "present").  A Criterion that does not name it calls nothing of it.
    `topk` (TopKCrossEntropyLoss) is added the same way; it honours ignore_index and reads topk_percent (default 10.0) and
    topk_per_image (default False).  The percentage lives in the buffer `topk_percent` ([1] fp32), read on the device by every
    call; set_topk_percent() writes into it without a sync, so a schedule costs a captured step no recapture."""

    def __init__(self, num_classes, args):
        super().__init__()
        self.num_classes = num_classes
        names = args.loss_type.split(',')
        weights = [float(w) for w in args.loss_weights.split(',')]
        self.w_dice = self.w_ce = self.w_bd = self.w_jac = 0.0
        has_jaccard = False
        self.has_base = self.has_surface = self.has_hausdorff = False
        w_dist = [0.0, 0.0]
        self.has_lovasz, self.w_lovasz = False, 0.0
        self.has_topk, self.w_topk = False, 0.0
        for n, w in zip(names, weights):
            if n == "topk":
                self.has_topk, self.w_topk = True, self.w_topk + w
                continue
            if n == "lovasz":
                self.has_lovasz, self.w_lovasz = True, self.w_lovasz + w
                continue
            if n in ("surface", "hausdorff"):
                w_dist[1 if n == "hausdorff" else 0] += w
                self.has_surface = self.has_surface or n == "surface"
                self.has_hausdorff = self.has_hausdorff or n == "hausdorff"
                continue
            self.has_base = True
            if n == "dice":
                self.w_dice += w
            elif n == "ce":
                self.w_ce += w
            elif n == "boundary":
                self.w_bd += w
            elif n == "jaccard":
                self.w_jac += w
                has_jaccard = True
            else:
                raise NotImplementedError(f"Loss {n} not implemented")
        wd = _class_weights(getattr(args, "dice_class_weights", None), num_classes, "dice_class_weights")
        wc = _class_weights(getattr(args, "ce_class_weights", None), num_classes, "ce_class_weights")
        ignore_index = getattr(args, "ignore_index", None)
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        smooth = getattr(args, "jaccard_smooth", None)
        self.jaccard_smooth = 1.0 if smooth is None else float(smooth)
        self.extended = has_jaccard or wd is not None or wc is not None or ignore_index is not None or smooth is not None
        if self.ignore_index is not None and self.w_bd != 0.0:
            raise NotImplementedError("Loss boundary with ignore_index not implemented: the reference defines no boundary count "
                                      "over a label mask with holes")
        if self.ignore_index is not None and (self.has_surface or self.has_hausdorff):
            raise NotImplementedError("Loss surface / hausdorff with ignore_index not implemented: a distance map over a label "
                                      "mask with holes is not defined")
        self.lovasz_per_image = bool(getattr(args, "lovasz_per_image", False))
        self.lovasz_classes = getattr(args, "lovasz_classes", None) or "present"
        if self.has_lovasz and self.lovasz_classes not in ("present", "all"):
            raise ValueError(f"lovasz_classes is 'present' or 'all', got {self.lovasz_classes!r}")
        self.topk_per_image = bool(getattr(args, "topk_per_image", False))
        percent = getattr(args, "topk_percent", None)
        percent = 10.0 if percent is None else float(percent)
        if self.has_topk:
            if not 0.0 < percent <= 100.0:
                raise ValueError(f"topk_percent is a percentage, 0 < k <= 100, got {percent}")
            self.register_buffer("topk_percent", torch.tensor([percent], dtype=torch.float32))
        else:
            self.topk_percent = None
        if self.has_surface or self.has_hausdorff:
            self.register_buffer("dist_weights", torch.tensor(w_dist, dtype=torch.float32))
        else:
            self.dist_weights = None
        if wd is not None or wc is not None:
            ones = [1.0] * num_classes
            self.register_buffer("class_weights", torch.tensor((wd or ones) + (wc or ones), dtype=torch.float32))
        else:
            self.class_weights = None

    def set_dist_weights(self, surface=None, hausdorff=None):
        """new weights of the `surface` / `hausdorff` terms (None: unchanged), written into `dist_weights` on its device by a fill
        launch each: no sync, and the next call — a graph replay included — reads them"""
        if self.dist_weights is None:
            raise ValueError("set_dist_weights: loss_type names neither surface nor hausdorff")
        with torch.no_grad():
            for i, v in enumerate((surface, hausdorff)):
                if isinstance(v, torch.Tensor):
                    self.dist_weights[i].copy_(v.reshape(()), non_blocking=True)
                elif v is not None:
                    self.dist_weights[i].fill_(float(v))

    def set_topk_percent(self, v):
        """a new percentage of the `topk` term (a number in (0, 100], or a one-element tensor), written into `topk_percent` on its
        device by one launch: no sync, and the next call — a graph replay included — reads it"""
        if self.topk_percent is None:
            raise ValueError("set_topk_percent: loss_type does not name topk")
        with torch.no_grad():
            if isinstance(v, torch.Tensor):
                self.topk_percent.copy_(v.reshape(1), non_blocking=True)
            else:
                if not 0.0 < float(v) <= 100.0:
                    raise ValueError(f"set_topk_percent: a percentage, 0 < k <= 100, got {v}")
                self.topk_percent.fill_(float(v))

    def forward(self, outputs, labels):
        if not self.has_topk:
            return self._but_topk(outputs, labels)
        topk = self.w_topk * ops.topk_ce(outputs, labels, self.topk_percent, per_image=self.topk_per_image,
                                         ignore_index=self.ignore_index)
        others = self.has_lovasz or self.has_base or self.dist_weights is not None
        return self._but_topk(outputs, labels) + topk if others else topk

    def _but_topk(self, outputs, labels):
        """the total of every name but `topk`"""
        if not self.has_lovasz:
            return self._named(outputs, labels)
        lovasz = self.w_lovasz * ops.lovasz_softmax(outputs, labels, per_image=self.lovasz_per_image, classes=self.lovasz_classes,
                                                    ignore_index=self.ignore_index)
        return self._named(outputs, labels) + lovasz if self.has_base or self.dist_weights is not None else lovasz

    def _named(self, outputs, labels):
        """the total of every name but `lovasz` and `topk`"""
        if self.dist_weights is None:
            return self._base(outputs, labels)
        dist = ops.dist_loss(outputs, labels, self.dist_weights, surface=self.has_surface, hausdorff=self.has_hausdorff)
        return self._base(outputs, labels) + dist if self.has_base else dist

    def _base(self, outputs, labels):
        if not self.extended:
            return ops.dice_ce_loss(outputs, labels, self.w_dice, self.w_ce, self.w_bd)
        K, cw = self.num_classes, self.class_weights
        return ops.seg_loss(outputs, labels, w_dice=self.w_dice, w_ce=self.w_ce, w_boundary=self.w_bd, w_jaccard=self.w_jac,
                            dice_class_weights=None if cw is None else cw[:K], ce_class_weights=None if cw is None else cw[K:],
                            ignore_index=self.ignore_index, jaccard_smooth=self.jaccard_smooth)
