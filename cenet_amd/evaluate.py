"""Evaluation path on the device: batched inference, argmax masks and Dice without leaving HBM.

Mirrors the reference's call sites:
  * `val()` of src/main_acdc.py:218-231 — per batch `dc(argmax(softmax(net(x))), label)` with medpy's binary Dice (non-zero
    = foreground) averaged over the loader  -> `val_dice`, `validate`
  * `calculate_dice_percase` / `test_single_volume` of src/utils/metrics_eval.py:24-34,37-84 — per foreground class over a
    whole volume, with the wrapper rules (pred>0 & gt==0 -> 1, otherwise 0)  -> `volume_class_dice`
The reference predicts slice by slice with batch size 1 and computes the metric on the host; here a volume's slices go
through the network in batches (under `ops.batch1_semantics()`, so that every slice is computed exactly as a batch-1
forward would: CCU's BatchNorm1d is the one batch-size-dependent op of the eval-mode network, cfam.py:260) and one kernel
produces the masks and the overlap counts (loss_optim.hip).
  * `calculate_metric_percase` of src/utils/metrics_eval.py:9-21 — (dice, hd95, jaccard, assd) per class  ->
    `metric_percase`, `test_single_volume`.  medpy's surface distances (border extraction + distance of every border voxel
    to the other border) run on the device in exact integer arithmetic (metrics.hip); only the final percentile / mean of
    the few thousand distances is taken on the host, in float64 like numpy does.  `label_metrics` scores all classes of a
    volume from the two label maps at once; `method=` picks between the all-pairs minimum and the exact distance transform
    (edt.hip), which is linear in the voxels and so also handles the noise an untrained network predicts.
    `spacing=` (medpy's `voxelspacing`, which the reference does not pass) reports hd95 / assd in the volume's physical unit
    through fp64 forms of the same kernels; `nsd_tolerance=` / `surface_dice` add the normalised surface Dice.
The scipy cubic `zoom` of slices that do not have the network's input size is the reference's own host-side dependency
(metrics_eval.py:45,55); `resize="host"` (the default) calls it the same way, `resize="device"` runs both resizes on the device
(csrc/volresize.hip through `predict_volume`: the volume is uploaded once and only the metric numbers come back).
  * `val_single_volume` (metrics_eval.py:87-122) and `inference` (utils_acdc.py:7-33) — the per-epoch test run of
    main_acdc.py:270-289 and `--eval`.
"""
from __future__ import annotations

import math
from typing import Iterable, List, Sequence, Tuple

import numpy as np
import torch

from . import kern, ops


def predict_counts(logits: torch.Tensor, labels: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits [B,K,H,W] -> (pred [B,H,W] class ids as float, counts [K+1,3] int32 or None).
    counts[c] = (|pred==c & gt==c|, |pred==c|, |gt==c|); counts[K] = the same for the binary masks pred>0 / gt>0."""
    logits = logits.contiguous()
    B, K = logits.shape[:2]
    HW = logits.numel() // (B * K)
    pred = torch.empty((B,) + tuple(logits.shape[2:]), device=logits.device, dtype=torch.float32)
    counts = None
    if labels is not None:
        labels = labels.reshape(B, -1).contiguous().float()
        counts = torch.empty((K + 1, 3), device=logits.device, dtype=torch.int32)
    kern.argmax_counts(logits, labels, pred, counts, B, K, HW)
    return pred, counts


def binary_dice(counts: torch.Tensor) -> float:
    """medpy.metric.binary.dc on the non-zero masks (main_acdc.py:228): 2|A∩B| / (|A|+|B|), 0.0 when both are empty."""
    inter, npred, ngt = (int(v) for v in counts[-1].tolist())
    return 2.0 * inter / (npred + ngt) if (npred + ngt) else 0.0


def class_dice(counts: torch.Tensor) -> List[float]:
    """calculate_dice_percase (metrics_eval.py:24-34) for classes 1..K-1."""
    out = []
    for inter, npred, ngt in counts[1:-1].tolist():
        if npred > 0 and ngt > 0:
            out.append(2.0 * inter / (npred + ngt))
        elif npred > 0 and ngt == 0:
            out.append(1.0)
        else:
            out.append(0.0)
    return out


@torch.no_grad()
def val_dice(net, images: torch.Tensor, labels: torch.Tensor) -> float:
    """one iteration of val() (main_acdc.py:222-228): images [B,Cin,H,W], labels [B,H,W] (or [B,1,H,W])."""
    _, counts = predict_counts(net(images), labels)
    return binary_dice(counts)


@torch.no_grad()
def validate(net, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]]) -> float:
    """val() of main_acdc.py:218-231: mean over the loader of the per-batch binary Dice; sets eval mode like the reference."""
    net.eval()
    vals = [val_dice(net, x, y) for x, y in batches]
    return sum(vals) / max(len(vals), 1)


@torch.no_grad()
def volume_class_dice(net, volume: torch.Tensor, label: torch.Tensor, classes: int, batch_slices: int = 32) -> List[float]:
    """test_single_volume (metrics_eval.py:37-84) for slices that already have the network input size: volume [D,H,W],
    label [D,H,W]; returns the Dice of classes 1..classes-1 over the whole volume."""
    net.eval()
    total = torch.zeros((classes + 1, 3), device=volume.device, dtype=torch.int64)
    for s in range(0, volume.shape[0], batch_slices):
        x = volume[s:s + batch_slices].unsqueeze(1).float()
        with ops.batch1_semantics():  # the reference feeds one slice per forward (metrics_eval.py:46-49): CCU skips its BN
            logits = net(x)
        _, counts = predict_counts(logits, label[s:s + batch_slices])
        total += counts.long()
    return class_dice(total)


# ---------------------------------------------------------------------------------------------------------------------
# surface-distance metrics (metrics_eval.py:9-21 -> medpy.metric.binary.{hd95, assd, jc})
# ---------------------------------------------------------------------------------------------------------------------
def surface_points(mask: torch.Tensor) -> torch.Tensor:
    """Border voxels of a boolean volume [D,H,W] (or image [H,W]) as int32 (z,y,x) rows: mask XOR its erosion by the
    face-connected structuring element with background outside the array (medpy `__surface_distances`)."""
    if mask.dim() == 2:
        mask = mask.unsqueeze(0)
        # a 2-D input has no z neighbours in medpy (2-D structuring element): pad so the z faces count as set
        m = (mask != 0).to(torch.uint8).repeat(3, 1, 1).contiguous()
        border = torch.empty_like(m)
        kern.surface_border(m, border, 3, m.shape[1], m.shape[2])
        pts = torch.nonzero(border[1:2]).to(torch.int32).contiguous()
        return pts
    m = (mask != 0).to(torch.uint8).contiguous()
    border = torch.empty_like(m)
    kern.surface_border(m, border, m.shape[0], m.shape[1], m.shape[2])
    return torch.nonzero(border).to(torch.int32).contiguous()


def _directed_sq(a_pts: torch.Tensor, b_pts: torch.Tensor, spacing=None) -> torch.Tensor:
    if spacing is not None:
        out = torch.empty((a_pts.shape[0],), dtype=torch.float64, device=a_pts.device)
        kern.min_sqdist_spaced(a_pts, b_pts, out, spacing)
        return out
    out = torch.full((a_pts.shape[0],), 2 ** 31 - 1, dtype=torch.int32, device=a_pts.device)
    kern.min_sqdist(a_pts, b_pts, out)
    return out


METHODS = ("auto", "edt", "pairs")
_INT_MAX = 2 ** 31 - 1
# method="auto": the transform when a class has more border-voxel pairs than this many per voxel of the union bounding box of its
# two borders, the all-pairs kernel below that (DESIGN.md §9 has the scan behind the number: the two methods cross between 549 and
# 741 pairs per box voxel on the MI355X, at about 640 by linear interpolation of the time differences)
AUTO_PAIRS_PER_BOX_VOXEL = 640
# the same threshold for the fp64 kernels a `spacing` selects: their all-pairs kernel is slower against its transform than the
# integer one, so they cross earlier (profiles/volume_metrics_spacing.json: between 403 and 549 pairs per box voxel on
# the MI355X, at 503 by linear interpolation of the time differences)
AUTO_PAIRS_PER_BOX_VOXEL_SPACED = 500


def _spacing(spacing, ndim: int):
    """medpy's `voxelspacing` for an array of `ndim` (2 or 3) axes -> None, or (sz, sy, sx) as floats (an image: sz = 1.0, which no
    distance within the one plane reads).  A number broadcasts; a sequence has one entry per axis, (z, y, x) or (y, x).  Anything
    else, and an entry that is not positive and finite, raises ValueError."""
    if spacing is None:
        return None
    what = f"spacing: a positive finite number or {ndim} of them ({'z, y, x' if ndim == 3 else 'y, x'}) expected, got {spacing!r}"
    if isinstance(spacing, (str, bytes, dict, set)) or torch.is_tensor(spacing) and spacing.dim() > 1:
        raise ValueError(what)
    try:
        sp = (float(spacing),) * ndim if np.ndim(spacing) == 0 else tuple(float(v) for v in spacing)
    except (TypeError, ValueError):
        raise ValueError(what) from None
    if len(sp) != ndim or not all(0.0 < v < float("inf") for v in sp):
        raise ValueError(what)
    return (1.0,) * (3 - ndim) + sp


def _tolerance(nsd_tolerance):
    """None, or the NSD tolerance as a float; ValueError unless it is positive and finite"""
    if nsd_tolerance is None:
        return None
    try:
        tau = math.nan if isinstance(nsd_tolerance, (str, bytes)) else float(nsd_tolerance)
    except (TypeError, ValueError):
        raise ValueError(f"nsd tolerance: a positive finite number expected, got {nsd_tolerance!r}") from None
    if not 0.0 < tau < float("inf"):
        raise ValueError(f"nsd tolerance: a positive finite number expected, got {nsd_tolerance!r}")
    return tau


def _nsd(d1: np.ndarray, d2: np.ndarray, tau: float) -> float:
    return float(np.count_nonzero(d1 <= tau) + np.count_nonzero(d2 <= tau)) / float(d1.size + d2.size)


def _download(t: torch.Tensor) -> np.ndarray:
    """the one device-to-host copy the label-map metrics go through (two calls per volume: the class table, the distances)"""
    return t.cpu().numpy()


def _label_table(pred: torch.Tensor, gt: torch.Tensor, classes: int):
    """two label volumes [D,H,W] (or images [H,W]: medpy's 2-D rule, no z neighbours) -> (border labels of pred, of gt: uint8
    [D,H,W], the voxel's class on that class's border, else 0; the per-class table of kern.label_borders as int64 numpy)"""
    if pred.shape != gt.shape or pred.dim() not in (2, 3):
        raise ValueError(f"two label volumes [D,H,W] or images [H,W] of one shape expected, got {tuple(pred.shape)}, {tuple(gt.shape)}")
    if not 2 <= classes <= 64:
        raise ValueError(f"2 <= classes <= 64 expected, got {classes}")
    zfaces = pred.dim() == 3
    if not zfaces:
        pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
    pred, gt = pred.float().contiguous(), gt.float().contiguous()
    D, H, W = pred.shape
    blp = torch.empty((D, H, W), dtype=torch.uint8, device=pred.device)
    blg = torch.empty_like(blp)
    table = torch.zeros((classes, kern.LB_COLS), dtype=torch.int32, device=pred.device)
    table[:, 5:] = _INT_MAX
    kern.label_borders(pred, gt, blp, blg, table, classes, D, H, W, zfaces)
    return blp, blg, _download(table).astype(np.int64)


def _border_offsets(bl: torch.Tensor, c: int, n: int) -> torch.Tensor:
    counts = torch.empty((n + kern.CP_CHUNK - 1) // kern.CP_CHUNK, dtype=torch.int32, device=bl.device)
    kern.border_count(bl, c, n, counts)
    return (torch.cumsum(counts, 0) - counts).to(torch.int32)


def _surface_sq(blp: torch.Tensor, blg: torch.Tensor, tab: np.ndarray, todo: Sequence[int], method: str, spacing=None):
    """squared surface distances of the classes `todo` (both masks non-empty): {c: (pred border -> gt border, gt border -> pred
    border)} as int32 numpy arrays in C order of the border voxels.  Everything is queued without a synchronisation, sized from
    the table; one download at the end brings all the arrays.  `spacing` (sz, sy, sx): the fp64 kernels, float64 arrays in the
    spacing's unit squared."""
    if not todo:
        return {}
    dev = blp.device
    per_voxel = AUTO_PAIRS_PER_BOX_VOXEL if spacing is None else AUTO_PAIRS_PER_BOX_VOXEL_SPACED
    sq_t = torch.int32 if spacing is None else torch.float64
    plan, total, scratch = [], 0, 0
    for c in todo:
        row = [int(v) for v in tab[c]]
        na, nb = row[3], row[4]
        lo = [min(row[5 + k], row[11 + k]) for k in range(3)]
        hi = [max(-row[8 + k], -row[14 + k]) for k in range(3)]
        box = [h - l + 1 for l, h in zip(lo, hi)]
        vol = box[0] * box[1] * box[2]
        edt = method == "edt" or (method == "auto" and na * nb > per_voxel * vol and kern.edt_supported(*box))
        plan.append((c, na, nb, lo, box, vol, edt, total))
        total += na + nb
        scratch = max(scratch, vol if edt else 0)
    # (the integer all-pairs kernel merges into its output, which starts at INT_MAX; the fp64 kernels write theirs)
    out = torch.full((total,), _INT_MAX, dtype=sq_t, device=dev) if spacing is None else torch.empty((total,), dtype=sq_t, device=dev)
    tmp = torch.empty(scratch, dtype=sq_t, device=dev) if scratch else None
    d2 = torch.empty(scratch, dtype=sq_t, device=dev) if scratch else None
    xd = torch.empty(scratch, dtype=torch.int32, device=dev) if scratch and spacing is not None else None
    for c, na, nb, lo, box, vol, edt, off in plan:
        # the union bounding box of the two borders holds every query and every feature voxel, so the transform of the crop equals
        # the transform of the volume at every query voxel
        a = blp[lo[0]:lo[0] + box[0], lo[1]:lo[1] + box[1], lo[2]:lo[2] + box[2]].contiguous()
        b = blg[lo[0]:lo[0] + box[0], lo[1]:lo[1] + box[1], lo[2]:lo[2] + box[2]].contiguous()
        offs_a, offs_b = _border_offsets(a, c, vol), _border_offsets(b, c, vol)
        oa, ob = out[off:off + na], out[off + na:off + na + nb]
        if edt and spacing is not None:
            kern.edt_sq_spaced_raw(b, c, xd, tmp, d2, *box, spacing)
            kern.border_gather(a, c, *box, offs_a, d2, oa)
            kern.edt_sq_spaced_raw(a, c, xd, tmp, d2, *box, spacing)
            kern.border_gather(b, c, *box, offs_b, d2, ob)
        elif edt:
            kern.edt_sq_raw(b, c, tmp, d2, *box)
            kern.border_gather(a, c, *box, offs_a, d2, oa)
            kern.edt_sq_raw(a, c, tmp, d2, *box)
            kern.border_gather(b, c, *box, offs_b, d2, ob)
        else:
            pa = torch.empty((na, 3), dtype=torch.int32, device=dev)
            pb = torch.empty((nb, 3), dtype=torch.int32, device=dev)
            kern.border_gather(a, c, *box, offs_a, None, pa)
            kern.border_gather(b, c, *box, offs_b, None, pb)
            if spacing is not None:
                kern.min_sqdist_spaced(pa, pb, oa, spacing)
                kern.min_sqdist_spaced(pb, pa, ob, spacing)
            else:
                kern.min_sqdist(pa, pb, oa)
                kern.min_sqdist(pb, pa, ob)
    arr = _download(out)
    return {c: (arr[off:off + na], arr[off + na:off + na + nb]) for c, na, nb, _, _, _, _, off in plan}


def _sqrt64(sq: np.ndarray) -> np.ndarray:
    return np.sqrt(sq.astype(np.float64))


def label_metrics(pred: torch.Tensor, gt: torch.Tensor, classes: int, kind: str = "acdc", method: str = "auto", spacing=None,
                  nsd_tolerance=None):
    """The per-class metric loop of test_single_volume (metrics_eval.py:60-62, utils_synapse.py:80-82) from the two label
    volumes [D,H,W] (or images [H,W]) directly: [(dice, hd95, jaccard, assd)] (kind="acdc", calculate_metric_percase of
    metrics_eval.py:9-21) or [(dice, hd95)] (kind="synapse", utils_synapse.py:12-21) for classes 1..classes-1, with the
    reference's rules for empty masks.  One kernel pass yields every class's borders, counts and bounding boxes; two downloads per
    volume (that table, then all the distance arrays) whatever `classes` is.  `method`: see `surface_distances`, chosen per class.
    `spacing`: the voxel spacing as `surface_distances` takes it; hd95 and assd are then in its unit (millimetres), from the fp64
    kernels, still with two downloads.  `nsd_tolerance` (a distance in that unit): every tuple gains the normalised surface Dice
    of `surface_dice` as its LAST element, counted on the host from the same arrays.  Its rule for empty masks follows the
    tuple's Dice rule, 1 for a prediction without ground truth and 0 otherwise: one more of the reference's odd family (a class
    absent from both scores 0, a false positive scores 1), not a definition of its own."""
    assert kind in ("acdc", "synapse"), kind
    assert method in METHODS, method
    if pred.dim() in (2, 3):  # (any other rank is refused by _label_table below)
        spacing = _spacing(spacing, pred.dim())
    tau = _tolerance(nsd_tolerance)
    blp, blg, tab = _label_table(pred, gt, classes)
    todo = [c for c in range(1, classes) if tab[c, 1] > 0 and tab[c, 2] > 0]
    sq = _surface_sq(blp, blg, tab, todo, method, spacing)
    res = []
    for c in range(1, classes):
        inter, np_, ng = (int(v) for v in tab[c, :3])
        if c in sq:
            d1, d2 = _sqrt64(sq[c][0]), _sqrt64(sq[c][1])
            dice = 2.0 * inter / float(np_ + ng)
            h95 = float(np.percentile(np.hstack((d1, d2)), 95))
            if kind == "acdc":
                m = (dice, h95, inter / float(np_ + ng - inter), float(np.mean((d1.mean(), d2.mean()))))
            else:
                m = (dice, h95)
            res.append(m if tau is None else m + (_nsd(d1, d2, tau),))
        elif np_ > 0 and ng == 0:
            m = (1, 0, 1, 0) if kind == "acdc" else (1, 0)
            res.append(m if tau is None else m + (1,))
        else:
            m = (0, 0, 0, 0) if kind == "acdc" else (0, 0)
            res.append(m if tau is None else m + (0,))
    return res


def surface_distances(result: torch.Tensor, reference: torch.Tensor, method: str = "auto",
                      spacing=None) -> Tuple[np.ndarray, np.ndarray]:
    """Both directed surface-distance sets (result->reference, reference->result) as float64 arrays, in voxels (unit voxel
    spacing) unless `spacing` is given.  Raises RuntimeError on an empty mask, as medpy does.  method="pairs": every border voxel against every border voxel of the
    other mask (metrics.hip); "edt": the exact distance transform of one border read at the other (edt.hip), over the union
    bounding box of the two; "auto": whichever the sizes favour.  The arrays are identical either way.
    `spacing`: medpy's `voxelspacing` — a positive number for every axis, or one per array axis, (z, y, x) for a volume and (y, x)
    for an image (ValueError for anything else): the distances are in its unit, from the fp64 forms of the same kernels.  Which
    voxels are border voxels does not depend on it.  With a spacing the methods agree to rounding (a few units in the last place;
    bit for bit when the spacings are dyadic), not necessarily in every bit: they sum the three terms in different orders."""
    assert method in METHODS, method
    if result.dim() in (2, 3):
        spacing = _spacing(spacing, result.dim())
    elif spacing is not None:
        raise ValueError(f"spacing: a volume [D,H,W] or an image [H,W] expected, got {tuple(result.shape)}")
    if method == "pairs" or (method == "auto" and (result.shape != reference.shape or result.dim() not in (2, 3))):
        ra, rb = surface_points(result), surface_points(reference)
        if ra.shape[0] == 0:
            raise RuntimeError("The first supplied array does not contain any binary object.")
        if rb.shape[0] == 0:
            raise RuntimeError("The second supplied array does not contain any binary object.")
        d1 = _directed_sq(ra, rb, spacing).cpu().numpy().astype(np.float64)
        d2 = _directed_sq(rb, ra, spacing).cpu().numpy().astype(np.float64)
        return np.sqrt(d1), np.sqrt(d2)
    blp, blg, tab = _label_table(result != 0, reference != 0, 2)
    if tab[1, 1] == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if tab[1, 2] == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    sq = _surface_sq(blp, blg, tab, [1], method, spacing)[1]
    return _sqrt64(sq[0]), _sqrt64(sq[1])


def hd95(result: torch.Tensor, reference: torch.Tensor, method: str = "auto", spacing=None) -> float:
    d1, d2 = surface_distances(result, reference, method, spacing)
    return float(np.percentile(np.hstack((d1, d2)), 95))


def assd(result: torch.Tensor, reference: torch.Tensor, method: str = "auto", spacing=None) -> float:
    d1, d2 = surface_distances(result, reference, method, spacing)
    return float(np.mean((d1.mean(), d2.mean())))


def surface_dice(result: torch.Tensor, reference: torch.Tensor, tolerance: float, spacing=None, method: str = "auto") -> float:
    """Normalised surface Dice (NSD) at `tolerance`: with d1, d2 the two arrays of `surface_distances(result, reference, method,
    spacing)`, (|{d1 <= tolerance}| + |{d2 <= tolerance}|) / (|d1| + |d2|) — the share of border voxels of either mask that lie
    within `tolerance` of the other mask's border.  The tolerance is in the unit of `spacing` (voxels without one) and must be
    positive and finite (ValueError).  Raises RuntimeError on an empty mask, as `surface_distances` does.
    This is the VOXEL-COUNT form: every border voxel weighs the same.  The surfel-area form of Nikolov et al. (2018), which weighs
    each surface element by its physical area, is a different number on anisotropic volumes and is not computed here."""
    tau = _tolerance(tolerance)
    if tau is None:
        raise ValueError("nsd tolerance: a positive finite number expected, got None")
    d1, d2 = surface_distances(result, reference, method, spacing)
    return _nsd(d1, d2, tau)


def metric_percase(pred: torch.Tensor, gt: torch.Tensor, method: str = "auto", spacing=None) -> Tuple[float, float, float, float]:
    """calculate_metric_percase (metrics_eval.py:9-21): (dice, hd95, jaccard, assd) of two binary volumes, with its rules
    for empty masks.  `spacing`: as `surface_distances` takes it."""
    assert method in METHODS, method
    if method != "pairs" and pred.shape == gt.shape and pred.dim() in (2, 3):
        return label_metrics(pred != 0, gt != 0, 2, "acdc", method, spacing)[0]
    if pred.dim() in (2, 3):
        _spacing(spacing, pred.dim())  # (refused here, whatever the masks hold; surface_distances reads it again)
    p, g = pred != 0, gt != 0
    np_, ng = int(p.sum()), int(g.sum())
    if np_ > 0 and ng > 0:
        inter = int((p & g).sum())
        dice = 2.0 * inter / float(np_ + ng)
        jac = inter / float(np_ + ng - inter)
        d1, d2 = surface_distances(p, g, method, spacing)
        return dice, float(np.percentile(np.hstack((d1, d2)), 95)), jac, float(np.mean((d1.mean(), d2.mean())))
    if np_ > 0 and ng == 0:
        return 1, 0, 1, 0
    return 0, 0, 0, 0


# ---------------------------------------------------------------------------------------------------------------------
# connected-component post-processing (csrc/ccl.hip; not in the reference, off unless asked for)
# ---------------------------------------------------------------------------------------------------------------------
POSTPROCESS = (None, "lcc")


def _check_postprocess(postprocess):
    if postprocess not in POSTPROCESS:
        raise ValueError(f"postprocess: None or 'lcc' (keep the largest connected component of each class) expected, "
                         f"got {postprocess!r}")


def _ccl_volume(label_map: torch.Tensor, classes: int, connectivity: int, per_slice: bool):
    """the label map as a contiguous fp32 volume [D,H,W] (an image [H,W]: D = 1), refused before anything is allocated"""
    from . import _lib
    if label_map.dim() not in (2, 3):
        raise ValueError(f"a label volume [D,H,W] or image [H,W] expected, got {tuple(label_map.shape)}")
    if not label_map.is_cuda and not _lib.is_hostsim():
        raise ValueError("connected components run on the MI355X only: the label map is not on a CUDA/HIP device")
    shape = (1,) + tuple(label_map.shape) if label_map.dim() == 2 else tuple(label_map.shape)
    kern._ccl_check(classes, *shape, connectivity, not per_slice)
    return label_map.reshape(shape).float().contiguous()


def _ccl_roots(vol: torch.Tensor, classes: int, connectivity: int, per_slice: bool) -> torch.Tensor:
    roots = torch.empty(vol.shape, dtype=torch.int32, device=vol.device)
    kern.ccl_label(vol, roots, classes, *vol.shape, connectivity, not per_slice)
    return roots


def connected_components(label_map: torch.Tensor, classes: int, connectivity: int = 1, per_slice: bool = False) -> torch.Tensor:
    """Components of every class of a label map [D,H,W] (or [H,W]) at once: int32, same shape, each voxel of class 1..classes-1
    gets the smallest linear index of its component, background -1.  connectivity 1 / 2 / 3 as
    scipy.ndimage.generate_binary_structure; per_slice: every slice on its own (connectivity 1 or 2)."""
    vol = _ccl_volume(label_map, classes, connectivity, per_slice)
    return _ccl_roots(vol, classes, connectivity, per_slice).reshape(label_map.shape)


def component_sizes(roots: torch.Tensor) -> torch.Tensor:
    """int32, same shape as `roots`: a component's voxel count at its root's position, 0 elsewhere"""
    roots = roots.contiguous()
    sizes = torch.empty_like(roots)
    kern.ccl_sizes(roots, sizes, roots.numel())
    return sizes


def keep_largest_component(label_map: torch.Tensor, classes: int, connectivity: int = 1, per_slice: bool = False,
                           min_size: int = 0) -> Tuple[torch.Tensor, np.ndarray]:
    """Keep the largest component of every class (per_slice: of every class in every slice) and set the other voxels to 0; among
    components of equal size the first in raster order stays.  min_size > 0 also keeps every component of at least that many voxels.
    -> (filtered fp32 map of the same shape, numpy [classes, 3]: components found, voxels kept, voxels removed per class).
    One download (the table); a map without foreground comes back as zeros with a zero table."""
    if min_size < 0:
        raise ValueError(f"min_size >= 0 expected, got {min_size}")
    vol = _ccl_volume(label_map, classes, connectivity, per_slice)
    D, H, W = vol.shape
    roots = _ccl_roots(vol, classes, connectivity, per_slice)
    sizes = component_sizes(roots)
    ws = torch.empty(kern.ccl_ws_ints(classes, D, not per_slice), dtype=torch.int32, device=vol.device)
    out = torch.empty_like(vol)
    table = torch.empty((classes, 3), dtype=torch.int32, device=vol.device)
    kern.ccl_keep(vol, roots, sizes, ws, out, table, classes, D, H, W, not per_slice, min_size)
    return out.reshape(label_map.shape), _download(table)


def _postprocessed(pred_d: torch.Tensor, classes: int, postprocess, connectivity: int, per_slice: bool) -> torch.Tensor:
    if postprocess is None:
        return pred_d
    return keep_largest_component(pred_d, classes, connectivity, per_slice)[0]


# ---------------------------------------------------------------------------------------------------------------------
# flip / rotate test-time augmentation (csrc/tta.hip; the reference's tta_model of utils/utils.py:146-168 is the "flips" set, on
# masks; here the class probabilities of the views are averaged).  Off unless asked for.
# ---------------------------------------------------------------------------------------------------------------------
TTA_SETS = kern.TTA_SETS


def _tta_mask(tta, PH: int, PW: int) -> Tuple[int, int]:
    """(view mask, T) of `tta` (a name of TTA_SETS or a tuple of view codes) for a [PH, PW] network input"""
    mask, T = kern.tta_view_mask(tta)
    if mask & 0xF0 and PH != PW:
        raise ValueError(f"tta={tta!r} holds transposed views (codes 4..7), which need a square patch, got {(PH, PW)}")
    return mask, T


def _tta_device_only(tta, resize, on_dev):
    """the volume wrappers run `tta` through predict_volume only: anything that would take the host route is an error"""
    if tta is None:
        return
    kern.tta_view_mask(tta)
    if resize != "device":
        raise ValueError(f"tta={tta!r} needs resize='device', got resize={resize!r}")
    if on_dev is None:
        raise ValueError(f"tta={tta!r}: this case takes the host route (a 2-D input, or an axis of length 1 to resize), which has no "
                         f"test-time augmentation")


@torch.no_grad()
def tta_predict(net, images: torch.Tensor, tta, labels: torch.Tensor = None):
    """Test-time augmentation of a 2-D batch: images [B, C, H, W] -> (pred [B, H, W] class ids as float, conf [B, H, W]: the
    winner's mean probability over the views, counts [K + 1, 3] int32 as `predict_counts` returns them, or None without `labels`).
    The T views of `tta` are made in one launch, go through `net` as ONE batch [T * B, C, H, W], and one kernel un-views the T
    logit stacks, averages their softmax and takes the argmax.  The network's mode and batch semantics are the caller's."""
    if images.dim() != 4:
        raise ValueError(f"images [B, C, H, W] expected, got {tuple(images.shape)}")
    B, C, H, W = images.shape
    mask, T = _tta_mask(tta, H, W)
    if min(H, W) < 2:
        raise ValueError(f"tta needs image sides >= 2, got {(H, W)}")
    images = images.float().contiguous()
    views = torch.empty((T * B, C, H, W), device=images.device, dtype=torch.float32)
    kern.tta_views(images, views, B, C, H, W, mask)
    logits = net(views).contiguous()
    K = logits.shape[1]
    pred = torch.empty((B, H, W), device=images.device, dtype=torch.float32)
    conf = torch.empty_like(pred)
    counts = None
    if labels is not None:
        labels = labels.reshape(B, H, W).float().contiguous()
        counts = torch.empty((K + 1, 3), device=images.device, dtype=torch.int32)
    kern.tta_argmax_resize_counts(logits, labels, pred, conf, counts, B, K, H, W, H, W, mask)
    return pred, conf, counts


def _device_case(image, label, device, patch_size):
    """image and label [D, H, W] on the device (one upload each), or None when the device resize does not take the case: a 2-D
    input, or an axis of length 1 that has to be resized (scipy special-cases those; the host path handles them)"""
    image = image.squeeze(0) if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
    label = label.squeeze(0) if torch.is_tensor(label) else torch.from_numpy(np.ascontiguousarray(label))
    if image.dim() != 3:
        return None
    H, W = image.shape[1:]
    PH, PW = int(patch_size[0]), int(patch_size[1])
    if (H, W) != (PH, PW) and not kern.vol_resize_supported(H, W, PH, PW):
        return None
    return image.to(device), label.to(device)


def _predict_volume_host(net, image: np.ndarray, label: np.ndarray, patch_size, batch_slices, device) -> np.ndarray:
    """the prediction loop of val_single_volume with the reference's host resizes (the loop `test_single_volume` runs)"""
    from scipy.ndimage import zoom
    D, x, y = image.shape
    resize = (x != patch_size[0] or y != patch_size[1])
    prediction = np.zeros_like(label)
    for s in range(0, D, batch_slices):
        sl = image[s:s + batch_slices]
        if resize:
            sl = np.stack([zoom(a, (patch_size[0] / x, patch_size[1] / y), order=3) for a in sl])
        inp = torch.from_numpy(np.ascontiguousarray(sl)).unsqueeze(1).float().to(device)
        with ops.batch1_semantics():
            logits = net(inp)
        pred, _ = predict_counts(logits)
        out = pred.reshape(-1, patch_size[0], patch_size[1]).cpu().numpy()
        for i in range(out.shape[0]):
            prediction[s + i] = zoom(out[i], (x / patch_size[0], y / patch_size[1]), order=0) if resize else out[i]
    return prediction


def _save_case(test_save_path, case, z_spacing, prediction, image, label):
    """the reference writes NIfTI files through SimpleITK (absent here): .npy volumes and the spacing in a side-car text file"""
    import os
    os.makedirs(test_save_path, exist_ok=True)
    for tag, vol in (("pred", prediction), ("img", image), ("gt", label)):
        vol = vol.cpu().numpy() if torch.is_tensor(vol) else vol
        np.save(os.path.join(test_save_path, f"{case}_{tag}.npy"), np.asarray(vol, dtype=np.float32))
    with open(os.path.join(test_save_path, f"{case}_spacing.txt"), "w") as f:
        f.write(f"1 1 {z_spacing}\n")


@torch.no_grad()
def predict_volume(net, volume: torch.Tensor, patch_size: Sequence[int], batch_slices: int = 32, normalize=None,
                   labels: torch.Tensor = None, tta=None, conf_out: torch.Tensor = None, window_overlap=None,
                   window_importance: str = "gaussian") -> Tuple[torch.Tensor, torch.Tensor]:
    """The prediction loop of test_single_volume (metrics_eval.py:41-58, utils_synapse.py:53-76) without leaving the device:
    volume [D, H, W] on the device -> (prediction [D, H, W] class ids as float, counts [K + 1, 3] int64 over the whole volume
    when `labels` [D, H, W] is given, else None).  Per chunk of `batch_slices` slices: zoom(order=3) to `patch_size` (skipped when
    the slices already have it, as the reference does), optional `normalize = (mean, std)`, forward with the reference's batch-1
    semantics, argmax + zoom(order=0) back in one kernel.  H, W and the patch sides must be >= 2 when they differ.
    `tta` (a name of TTA_SETS or a tuple of view codes; None: off): a chunk holds max(1, batch_slices // T) slices, whose T views go
    through the network as one batch of at most `batch_slices`; one kernel un-views the logit stacks, averages their softmax, takes
    the argmax and resizes back.  `conf_out` (with `tta` only): a [D, H, W] fp32 tensor on the volume's device that receives the
    winning class's mean probability.  All sides must be >= 2 then.
    `window_overlap` (None: off, all of the above unchanged; a number in [0, 1)): sliding-window inference, `patch_size` is the
    window and nothing is resized in either direction (`_predict_volume_sw`); `window_importance`: "gaussian" or "constant".
    `tta` and `conf_out` (the winner's blended probability) are both allowed then."""
    assert volume.dim() == 3, "volume [D,H,W] expected"
    D, H, W = volume.shape
    PH, PW = int(patch_size[0]), int(patch_size[1])
    if window_overlap is not None:
        return _predict_volume_sw(net, volume, (PH, PW), batch_slices, normalize, labels, tta, conf_out, window_overlap,
                                  window_importance)
    resize = (H != PH or W != PW)
    if resize and not kern.vol_resize_supported(H, W, PH, PW):
        raise ValueError(f"the device resize needs sides >= 2, got {(H, W)} -> {(PH, PW)}")
    if tta is None and conf_out is not None:
        raise ValueError("conf_out is the mean probability over the views of `tta`: it cannot be given with tta=None")
    if tta is not None:
        return _predict_volume_tta(net, volume, (PH, PW), batch_slices, normalize, labels, tta, conf_out)
    volume = volume.float().contiguous()
    pred = torch.empty((D, H, W), device=volume.device, dtype=torch.float32)
    total = None
    if labels is not None:
        labels = labels.reshape(D, H, W).float().contiguous()
    stage = torch.empty(min(D, batch_slices) * H * W, device=volume.device, dtype=torch.float64) if resize else None
    for s in range(0, D, batch_slices):
        sl = volume[s:s + batch_slices]
        n = sl.shape[0]
        if resize:
            inp = torch.empty((n, 1, PH, PW), device=volume.device, dtype=torch.float32)
            kern.vol_resize_cubic(sl, stage, inp, n, H, W, PH, PW, normalize)
        else:
            inp = sl.unsqueeze(1)
            if normalize is not None:
                inp = (inp - normalize[0]) / normalize[1]
        with ops.batch1_semantics():  # slice-by-slice semantics of the reference (CCU's `if B > 1` BatchNorm, cfam.py:260)
            logits = net(inp).contiguous()
        K = logits.shape[1]
        counts = None
        if labels is not None:
            counts = torch.empty((K + 1, 3), device=volume.device, dtype=torch.int32)
        kern.argmax_resize_counts(logits, None if labels is None else labels[s:s + n], pred[s:s + n], counts, n, K, PH, PW, H, W)
        if counts is not None:
            total = counts.long() if total is None else total + counts.long()
    return pred, total


def _predict_volume_tta(net, volume, patch, batch_slices, normalize, labels, tta, conf_out):
    """predict_volume with test-time augmentation: per chunk resize in (unchanged), views, one forward, fused merge"""
    D, H, W = volume.shape
    PH, PW = patch
    mask, T = _tta_mask(tta, PH, PW)
    if min(H, W, PH, PW) < 2:
        raise ValueError(f"tta needs sides >= 2, got {(H, W)} -> {(PH, PW)}")
    if conf_out is not None and (tuple(conf_out.shape) != (D, H, W) or conf_out.dtype != torch.float32
                                 or conf_out.device != volume.device or not conf_out.is_contiguous()):
        raise ValueError(f"conf_out: a contiguous fp32 tensor {(D, H, W)} on {volume.device} expected, got "
                         f"{tuple(conf_out.shape)} {conf_out.dtype} on {conf_out.device}")
    resize = (H != PH or W != PW)
    chunk = max(1, batch_slices // T)
    volume = volume.float().contiguous()
    pred = torch.empty((D, H, W), device=volume.device, dtype=torch.float32)
    total = None
    if labels is not None:
        labels = labels.reshape(D, H, W).float().contiguous()
    stage = torch.empty(min(D, chunk) * H * W, device=volume.device, dtype=torch.float64) if resize else None
    for s in range(0, D, chunk):
        sl = volume[s:s + chunk]
        n = sl.shape[0]
        if resize:
            inp = torch.empty((n, 1, PH, PW), device=volume.device, dtype=torch.float32)
            kern.vol_resize_cubic(sl, stage, inp, n, H, W, PH, PW, normalize)
        else:
            inp = sl.unsqueeze(1)
            if normalize is not None:
                inp = (inp - normalize[0]) / normalize[1]
            inp = inp.contiguous()
        views = torch.empty((T * n, 1, PH, PW), device=volume.device, dtype=torch.float32)
        kern.tta_views(inp, views, n, 1, PH, PW, mask)
        with ops.batch1_semantics():  # every view of every slice is computed as a batch-1 forward would compute it
            logits = net(views).contiguous()
        K = logits.shape[1]
        counts = None
        if labels is not None:
            counts = torch.empty((K + 1, 3), device=volume.device, dtype=torch.int32)
        kern.tta_argmax_resize_counts(logits, None if labels is None else labels[s:s + n], pred[s:s + n],
                                      None if conf_out is None else conf_out[s:s + n], counts, n, K, PH, PW, H, W, mask)
        if counts is not None:
            total = counts.long() if total is None else total + counts.long()
    return pred, total


# ---------------------------------------------------------------------------------------------------------------------
# sliding-window inference at the image's own resolution (csrc/sliding_window.hip): nnU-Net's window grid, MONAI's Gaussian
# importance map; not in the reference, whose resize recipe stays the default.  Off unless asked for.
# ---------------------------------------------------------------------------------------------------------------------
_SW_WEIGHTS = {}  # (P, importance, device) -> the factor on the device: a handful of small vectors, uploaded once each


def _window_args(window_overlap, window_importance):
    """both checked before anything runs"""
    if isinstance(window_overlap, bool) or not isinstance(window_overlap, (int, float)) or not 0.0 <= window_overlap < 1.0:
        raise ValueError(f"window_overlap: None or a number in [0, 1) expected, got {window_overlap!r}")
    if window_importance not in kern.SW_IMPORTANCE:
        raise ValueError(f"window_importance: one of {kern.SW_IMPORTANCE} expected, got {window_importance!r}")


def _sw_device_only(window_overlap, window_importance, resize, on_dev):
    """the volume wrappers run the sliding window through predict_volume only, as `_tta_device_only`"""
    if window_overlap is None:
        return {}
    _window_args(window_overlap, window_importance)
    if resize != "device":
        raise ValueError(f"window_overlap={window_overlap!r} needs resize='device', got resize={resize!r}")
    if on_dev is None:
        raise ValueError(f"window_overlap={window_overlap!r}: this case takes the host route (a 2-D input, or an axis of length 1), "
                         f"which has no sliding-window inference")
    return dict(window_overlap=window_overlap, window_importance=window_importance)


def _sw_weight(P: int, importance: str, device) -> torch.Tensor:
    key = (P, importance, str(device))
    if key not in _SW_WEIGHTS:
        _SW_WEIGHTS[key] = torch.from_numpy(kern.sw_weights(P, importance)).to(device)
    return _SW_WEIGHTS[key]


def _sw_plan(H, W, PH, PW, overlap, importance, tta, device):
    """(oy, ox, wy, wx, view mask, T): the origin tables (host lists) and the importance map's two factors on `device`"""
    _window_args(overlap, importance)
    mask, T = (1, 1) if tta is None else _tta_mask(tta, PH, PW)
    return (kern.sw_origins(H, PH, overlap), kern.sw_origins(W, PW, overlap), _sw_weight(PH, importance, device),
            _sw_weight(PW, importance, device), mask, T)


def _sw_chunk(net, src, plan, patch, max_batch, normalize, pad_value, labels, pred, conf, semantics=None):
    """one chunk src [n, C, H, W] of a sliding-window prediction: all windows in one launch, their views in one more, the network
    in forwards of at most `max_batch` written into ONE logits buffer, one merge launch into pred / conf [n, H, W].  Returns the
    chunk's counts [K + 1, 3] int32 (None without labels)."""
    import contextlib
    oy, ox, wy, wx, mask, T = plan
    PH, PW = patch
    n, C, H, W = src.shape
    nb = n * len(oy) * len(ox)
    windows = torch.empty((nb, C, PH, PW), device=src.device, dtype=torch.float32)
    kern.sw_windows(src, windows, oy, ox, n, C, H, W, PH, PW, normalize, pad_value)
    if T > 1:
        views = torch.empty((T * nb, C, PH, PW), device=src.device, dtype=torch.float32)
        kern.tta_views(windows, views, nb, C, PH, PW, mask)
    else:
        views = windows
    with (semantics() if semantics is not None else contextlib.nullcontext()):
        if T * nb <= max_batch:
            logits = net(views).contiguous()
        else:
            logits = None
            for s in range(0, T * nb, max_batch):
                part = net(views[s:s + max_batch])
                if logits is None:
                    logits = torch.empty((T * nb,) + tuple(part.shape[1:]), device=part.device, dtype=part.dtype)
                logits[s:s + max_batch].copy_(part)
    K = logits.shape[1]
    counts = None
    if labels is not None:
        counts = torch.empty((K + 1, 3), device=src.device, dtype=torch.int32)
    kern.sw_merge_counts(logits, labels, wy, wx, oy, ox, pred, conf, counts, n, K, PH, PW, H, W, mask)
    return counts


@torch.no_grad()
def sliding_window_predict(net, images: torch.Tensor, window: Sequence[int], overlap: float = 0.5, importance: str = "gaussian",
                           tta=None, labels: torch.Tensor = None, batch_windows: int = 32, normalize=None,
                           pad_value: float = 0.0):
    """Sliding-window inference of a 2-D batch, the counterpart of `tta_predict`: images [B, C, H, W] -> (pred [B, H, W] class ids
    as float, conf [B, H, W]: the winner's blended probability, counts [K + 1, 3] int32 as `predict_counts` returns them, or None
    without `labels`).  The network sees [window] crops at the images' own resolution (origins: `kern.sw_origins`, `overlap` in
    [0, 1); an image smaller than the window is centred in it and padded with `pad_value`), optionally normalised with
    `normalize = (mean, std)`; the windows' softmax is blended with the `importance` map ("gaussian" or "constant") and, with
    `tta`, over its views.  A chunk holds max(1, batch_windows // (windows per image * T)) images; its windows go through `net` in
    forwards of at most `batch_windows`.  The network's mode and batch semantics are the caller's."""
    if images.dim() != 4:
        raise ValueError(f"images [B, C, H, W] expected, got {tuple(images.shape)}")
    B, C, H, W = images.shape
    PH, PW = int(window[0]), int(window[1])
    plan = _sw_plan(H, W, PH, PW, overlap, importance, tta, images.device)
    batch_windows = max(1, int(batch_windows))
    chunk = max(1, batch_windows // (len(plan[0]) * len(plan[1]) * plan[5]))
    images = images.float().contiguous()
    pred = torch.empty((B, H, W), device=images.device, dtype=torch.float32)
    conf = torch.empty_like(pred)
    if labels is not None:
        labels = labels.reshape(B, H, W).float().contiguous()
    total = None
    for s in range(0, B, chunk):
        counts = _sw_chunk(net, images[s:s + chunk], plan, (PH, PW), batch_windows, normalize, pad_value,
                           None if labels is None else labels[s:s + chunk], pred[s:s + chunk], conf[s:s + chunk])
        if counts is not None:
            total = counts if total is None else total.add_(counts)
    return pred, conf, total


def _predict_volume_sw(net, volume, patch, batch_slices, normalize, labels, tta, conf_out, overlap, importance):
    """predict_volume with `window_overlap`: per chunk of max(1, batch_slices // (windows per slice * T)) slices the windows, their
    views, the forwards (at most `batch_slices` windows each, batch-1 semantics: the split cannot change a value) and the fused
    merge.  The origin tables ride in the kernel arguments and the importance factors are on the device before the loop, which
    makes no host round trip."""
    D, H, W = volume.shape
    PH, PW = patch
    plan = _sw_plan(H, W, PH, PW, overlap, importance, tta, volume.device)
    if conf_out is not None and (tuple(conf_out.shape) != (D, H, W) or conf_out.dtype != torch.float32
                                 or conf_out.device != volume.device or not conf_out.is_contiguous()):
        raise ValueError(f"conf_out: a contiguous fp32 tensor {(D, H, W)} on {volume.device} expected, got "
                         f"{tuple(conf_out.shape)} {conf_out.dtype} on {conf_out.device}")
    batch_slices = max(1, int(batch_slices))
    chunk = max(1, batch_slices // (len(plan[0]) * len(plan[1]) * plan[5]))
    volume = volume.float().contiguous()
    pred = torch.empty((D, H, W), device=volume.device, dtype=torch.float32)
    total = None
    if labels is not None:
        labels = labels.reshape(D, H, W).float().contiguous()
    for s in range(0, D, chunk):
        counts = _sw_chunk(net, volume[s:s + chunk].unsqueeze(1), plan, (PH, PW), batch_slices, normalize, 0.0,
                           None if labels is None else labels[s:s + chunk], pred[s:s + chunk],
                           None if conf_out is None else conf_out[s:s + chunk], semantics=ops.batch1_semantics)
        if counts is not None:
            total = counts.long() if total is None else total + counts.long()
    return pred, total


def _surface_kwargs(spacing, nsd_tolerance, ndim: int) -> dict:
    """what the volume wrappers add to their `label_metrics` call: nothing for (None, None), so that call is then the one it has
    always been; both are checked here, before the network runs"""
    _spacing(spacing, ndim)
    _tolerance(nsd_tolerance)
    kw = {}
    if spacing is not None:
        kw["spacing"] = spacing
    if nsd_tolerance is not None:
        kw["nsd_tolerance"] = nsd_tolerance
    return kw


@torch.no_grad()
def test_single_volume(image, label, net, classes: int, patch_size: Sequence[int] = (224, 224), batch_slices: int = 32,
                       device=None, resize: str = "host", test_save_path=None, case=None,
                       z_spacing: float = 1.0, postprocess=None, lcc_connectivity: int = 1,
                       lcc_per_slice: bool = False, tta=None, spacing=None,
                       nsd_tolerance=None, window_overlap=None,
                       window_importance: str = "gaussian") -> List[Tuple[float, float, float, float]]:
    """test_single_volume (metrics_eval.py:37-84) for a 3-D volume: image / label [1,D,H,W] or [D,H,W] (tensor or ndarray).
    Slices are resized to `patch_size` with scipy's cubic zoom and the predictions back with order 0 exactly as the
    reference does (host side), but the network runs on batches of slices and the metrics on the device.
    `resize="device"`: image and label are uploaded once and both resizes run on the device (`predict_volume`); a case the
    device resize does not take (an axis of length 1) goes the host way.  `test_save_path`: see `_save_case`.
    `postprocess="lcc"`: the prediction goes through `keep_largest_component(pred, classes, lcc_connectivity, lcc_per_slice)` on
    the device before it is scored and saved (not in the reference; None: no such step).
    `tta` (a name of TTA_SETS or a tuple of view codes): test-time augmentation inside `predict_volume`, before `postprocess`;
    it needs resize="device" and a case the device resize takes, and raises ValueError otherwise.
    `spacing`: the volume's voxel spacing, a number or (z, y, x), in which hd95 and assd are then reported (`label_metrics`; None:
    voxels, as the reference).  `z_spacing` is not read for it: it only goes into the side-car file of `test_save_path`.
    `nsd_tolerance`: every tuple gains the normalised surface Dice at that tolerance as its last element.
    `window_overlap` (None: off; a number in [0, 1)) / `window_importance`: sliding-window inference inside `predict_volume`
    with `patch_size` windows instead of the two resizes; needs resize="device" like `tta`, and composes with it and with
    everything after the prediction.
    Returns [(dice, hd95, jaccard, assd)] for classes 1..classes-1."""
    from scipy.ndimage import zoom
    assert resize in ("host", "device"), resize
    _check_postprocess(postprocess)
    surf = _surface_kwargs(spacing, nsd_tolerance, 3)
    device = device or next(net.parameters()).device
    net.eval()
    on_dev = _device_case(image, label, device, patch_size) if resize == "device" else None
    _tta_device_only(tta, resize, on_dev)
    sw = _sw_device_only(window_overlap, window_importance, resize, on_dev)
    if on_dev is not None:
        pred_d, _ = predict_volume(net, on_dev[0], patch_size, batch_slices, tta=tta, **sw)
        pred_d = _postprocessed(pred_d, classes, postprocess, lcc_connectivity, lcc_per_slice)
        if test_save_path is not None:
            _save_case(test_save_path, case, z_spacing, pred_d, on_dev[0], on_dev[1])
        return label_metrics(pred_d, on_dev[1], classes, "acdc", **surf)
    image = image.squeeze(0).cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    label = label.squeeze(0).cpu().numpy() if torch.is_tensor(label) else np.asarray(label)
    assert image.ndim == 3, "volume [D,H,W] expected"
    D, x, y = image.shape
    resize = (x != patch_size[0] or y != patch_size[1])
    prediction = np.zeros_like(label)
    for s in range(0, D, batch_slices):
        sl = image[s:s + batch_slices]
        if resize:
            sl = np.stack([zoom(a, (patch_size[0] / x, patch_size[1] / y), order=3) for a in sl])
        inp = torch.from_numpy(np.ascontiguousarray(sl)).unsqueeze(1).float().to(device)
        with ops.batch1_semantics():  # slice-by-slice semantics of the reference (CCU's `if B > 1` BatchNorm, cfam.py:260)
            logits = net(inp)
        pred, _ = predict_counts(logits)
        out = pred.reshape(-1, patch_size[0], patch_size[1]).cpu().numpy()
        for i in range(out.shape[0]):
            prediction[s + i] = zoom(out[i], (x / patch_size[0], y / patch_size[1]), order=0) if resize else out[i]
    pred_d = torch.from_numpy(np.ascontiguousarray(prediction)).to(device)
    lab_d = torch.from_numpy(np.ascontiguousarray(label)).to(device)
    if postprocess is not None:
        pred_d = prediction = _postprocessed(pred_d, classes, postprocess, lcc_connectivity, lcc_per_slice)
    if test_save_path is not None:
        _save_case(test_save_path, case, z_spacing, prediction, image, label)
    return label_metrics(pred_d, lab_d, classes, "acdc", **surf)


# ---------------------------------------------------------------------------------------------------------------------------
# Synapse (utils/utils_synapse.py:12-100) and skin (utils/utils_skin.py:97-170) evaluation wrappers
# ---------------------------------------------------------------------------------------------------------------------------
def synapse_metric_percase(pred: torch.Tensor, gt: torch.Tensor, method: str = "auto", spacing=None) -> Tuple[float, float]:
    """calculate_metric_percase of utils_synapse.py:12-21: (dice, hd95) of two binary volumes; (1, 0) for a prediction without
    ground truth, (0, 0) otherwise.  `spacing`: as `surface_distances` takes it."""
    assert method in METHODS, method
    if method != "pairs" and pred.shape == gt.shape and pred.dim() in (2, 3):
        return label_metrics(pred != 0, gt != 0, 2, "synapse", method, spacing)[0]
    if pred.dim() in (2, 3):
        _spacing(spacing, pred.dim())  # (refused here, whatever the masks hold; surface_distances reads it again)
    p, g = pred != 0, gt != 0
    np_, ng = int(p.sum()), int(g.sum())
    if np_ > 0 and ng > 0:
        inter = int((p & g).sum())
        d1, d2 = surface_distances(p, g, method, spacing)
        return 2.0 * inter / float(np_ + ng), float(np.percentile(np.hstack((d1, d2)), 95))
    if np_ > 0 and ng == 0:
        return 1, 0
    return 0, 0


@torch.no_grad()
def synapse_test_single_volume(image, label, net, classes: int, patch_size: Sequence[int] = (256, 256), test_save_path=None,
                               case=None, z_spacing: float = 1.0, batch_slices: int = 32, device=None, resize: str = "host",
                               postprocess=None, lcc_connectivity: int = 1, lcc_per_slice: bool = False, tta=None,
                               spacing=None, nsd_tolerance=None, window_overlap=None, window_importance: str = "gaussian"):
    """test_single_volume of utils_synapse.py:49-97: every slice of the volume [1, D, H, W] is resized to `patch_size` (cubic
    zoom), normalised with Normalize([0.5], [0.5]) (`ToTensor` leaves float arrays unscaled), classified, and the prediction
    resized back with order 0; returns [(dice, hd95)] for classes 1..classes-1.  A 2-D input takes the reference's second branch
    (one forward, no normalisation).  The slices go through the network in batches (with the reference's batch-1 semantics),
    the metrics run on the device.  `test_save_path` (NIfTI files through SimpleITK, which is absent here) writes .npy volumes
    with the spacing (1, 1, z_spacing) in a side-car text file instead.  `resize="device"`: as for `test_single_volume`, with the
    normalisation inside the resize kernel; the 2-D branch has no resize and is the same in both modes.  `postprocess`,
    `lcc_connectivity`, `lcc_per_slice`, `tta`: as for `test_single_volume` (the 2-D branch takes no `tta`: ValueError).
    `spacing` (a number, or one entry per axis of the input: (z, y, x), or (y, x) for the 2-D branch) and `nsd_tolerance`: as for
    `test_single_volume`; the tuples are then (dice, hd95 in that unit[, nsd]).  `z_spacing` stays the side-car's alone.
    `window_overlap` / `window_importance`: as for `test_single_volume` (the normalisation is then fused into the window gather;
    the 2-D branch takes none: ValueError)."""
    from scipy.ndimage import zoom
    assert resize in ("host", "device"), resize
    _check_postprocess(postprocess)
    nd = (image.squeeze(0) if torch.is_tensor(image) else np.asarray(image)).ndim
    surf = _surface_kwargs(spacing, nsd_tolerance, nd if nd in (2, 3) else 3)
    device = device or next(net.parameters()).device
    net.eval()
    on_dev = _device_case(image, label, device, patch_size) if resize == "device" else None
    _tta_device_only(tta, resize, on_dev)
    sw = _sw_device_only(window_overlap, window_importance, resize, on_dev)
    if on_dev is not None:
        pred_d, _ = predict_volume(net, on_dev[0], patch_size, batch_slices, normalize=(0.5, 0.5), tta=tta, **sw)
        pred_d = _postprocessed(pred_d, classes, postprocess, lcc_connectivity, lcc_per_slice)
        if test_save_path is not None:
            _save_case(test_save_path, case, z_spacing, pred_d, on_dev[0], on_dev[1])
        return label_metrics(pred_d, on_dev[1], classes, "synapse", **surf)
    image = image.squeeze(0).cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    label = label.squeeze(0).cpu().numpy() if torch.is_tensor(label) else np.asarray(label)
    if image.ndim == 3:
        D, x, y = image.shape
        resize = (x != patch_size[0] or y != patch_size[1])
        prediction = np.zeros_like(label)
        for s in range(0, D, batch_slices):
            sl = image[s:s + batch_slices]
            if resize:
                sl = np.stack([zoom(a, (patch_size[0] / x, patch_size[1] / y), order=3) for a in sl])
            inp = torch.from_numpy(np.ascontiguousarray(sl)).unsqueeze(1).float()
            inp = ((inp - 0.5) / 0.5).to(device)
            with ops.batch1_semantics():
                logits = net(inp)
            pred, _ = predict_counts(logits)
            out = pred.reshape(-1, patch_size[0], patch_size[1]).cpu().numpy()
            for i in range(out.shape[0]):
                prediction[s + i] = zoom(out[i], (x / patch_size[0], y / patch_size[1]), order=0) if resize else out[i]
    else:
        inp = torch.from_numpy(np.ascontiguousarray(image)).unsqueeze(0).unsqueeze(0).float().to(device)
        pred, _ = predict_counts(net(inp))
        prediction = pred.squeeze(0).cpu().numpy().astype(label.dtype)
    pred_d = torch.from_numpy(np.ascontiguousarray(prediction)).to(device)
    lab_d = torch.from_numpy(np.ascontiguousarray(label)).to(device)
    if postprocess is not None:
        pred_d = prediction = _postprocessed(pred_d, classes, postprocess, lcc_connectivity, lcc_per_slice)
    metric_list = label_metrics(pred_d, lab_d, classes, "synapse", **surf)
    if test_save_path is not None:
        _save_case(test_save_path, case, z_spacing, prediction, image, label)
    return metric_list


@torch.no_grad()
def val_single_volume(image, label, net, classes: int, patch_size: Sequence[int] = (224, 224), batch_slices: int = 32,
                      device=None, resize: str = "device", tta=None, window_overlap=None,
                      window_importance: str = "gaussian") -> List[float]:
    """val_single_volume (metrics_eval.py:87-122): the prediction of `test_single_volume`, scored with calculate_dice_percase
    only — Dice of classes 1..classes-1 over the whole volume.  `resize="device"`: the overlap counts come out of the argmax +
    resize-back kernel, nothing but those 3 (K + 1) integers leaves the device.  `resize="host"` (and cases the device resize
    does not take): the reference's host resizes, counts from the device.  `tta`: as for `test_single_volume`; the counts then
    come out of the merge kernel.  `window_overlap` / `window_importance`: as for `test_single_volume`."""
    assert resize in ("host", "device"), resize
    device = device or next(net.parameters()).device
    net.eval()
    on_dev = _device_case(image, label, device, patch_size) if resize == "device" else None
    _tta_device_only(tta, resize, on_dev)
    sw = _sw_device_only(window_overlap, window_importance, resize, on_dev)
    if on_dev is not None:
        _, counts = predict_volume(net, on_dev[0], patch_size, batch_slices, labels=on_dev[1], tta=tta, **sw)
        return class_dice(counts)[:classes - 1]
    image = image.squeeze(0).cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    label = label.squeeze(0).cpu().numpy() if torch.is_tensor(label) else np.asarray(label)
    assert image.ndim == 3, "volume [D,H,W] expected"
    prediction = _predict_volume_host(net, image, label, patch_size, batch_slices, device)
    pred_d = torch.from_numpy(np.ascontiguousarray(prediction)).to(device)
    lab_d = torch.from_numpy(np.ascontiguousarray(label)).to(device)
    out = []
    for c in range(1, classes):  # calculate_dice_percase (metrics_eval.py:24-34)
        p, g = pred_d == c, lab_d == c
        np_, ng = int(p.sum()), int(g.sum())
        out.append(2.0 * int((p & g).sum()) / (np_ + ng) if np_ > 0 and ng > 0 else (1.0 if np_ > 0 else 0.0))
    return out


@torch.no_grad()
def inference(net, volumes, classes: int, patch_size: Sequence[int] = (224, 224), z_spacing: float = 1.0, test_save_path=None,
              log=print, resize: str = "device", batch_slices: int = 32, device=None, postprocess=None,
              lcc_connectivity: int = 1, lcc_per_slice: bool = False, tta=None, spacing=None,
              nsd_tolerance=None, window_overlap=None, window_importance: str = "gaussian") -> Tuple[float, float]:
    """inference (utils_acdc.py:7-33): `test_single_volume` for every case of `volumes` (the test loader's dicts: `image`
    [1, D, H, W], `label`, `case_name` — a string or the DataLoader's one-element list), the reference's per-case and per-class
    log lines through `log`, and (mean dice, mean hd95): the metric table averaged over the cases, then over the classes.
    `postprocess`, `lcc_connectivity`, `lcc_per_slice`, `tta` and `window_overlap` / `window_importance` go to `test_single_volume`.
    `spacing`: the voxel spacing hd95 and assd are reported in — a number or (z, y, x) for all cases, or one per case: a dict
    {case_name: spacing}, which must hold every case, or a list with one spacing per case in the order of `volumes` (a list of
    three NUMBERS is one spacing for all cases).  `nsd_tolerance`: the tables gain the normalised surface Dice as a fifth column,
    one more log line reports its means, and the result is (mean dice, mean hd95, mean nsd)."""
    _check_postprocess(postprocess)
    _tolerance(nsd_tolerance)
    per_case = isinstance(spacing, dict) or (isinstance(spacing, (list, tuple)) and any(np.ndim(v) > 0 or v is None for v in spacing))
    if not per_case:
        _spacing(spacing, 3)
    post = {} if postprocess is None else dict(postprocess=postprocess, lcc_connectivity=lcc_connectivity,
                                               lcc_per_slice=lcc_per_slice)
    if tta is not None:
        post["tta"] = tta
    if window_overlap is not None:
        _window_args(window_overlap, window_importance)
        post.update(window_overlap=window_overlap, window_importance=window_importance)
    if nsd_tolerance is not None:
        post["nsd_tolerance"] = nsd_tolerance
    net.eval()
    total, n = 0.0, 0
    for i, batch in enumerate(volumes):
        case = batch["case_name"]
        case = case[0] if isinstance(case, (list, tuple)) else case
        if per_case:
            try:
                post["spacing"] = spacing[case] if isinstance(spacing, dict) else spacing[i]
            except (KeyError, IndexError):
                raise ValueError(f"inference: no spacing for case {case!r} (index {i})") from None
        elif spacing is not None:
            post["spacing"] = spacing
        m = test_single_volume(batch["image"], batch["label"], net, classes, patch_size=patch_size, batch_slices=batch_slices,
                               device=device, resize=resize, test_save_path=test_save_path, case=case, z_spacing=z_spacing,
                               **post)
        total = total + np.array(m, dtype=np.float64)
        n += 1
        mm = np.mean(m, axis=0)
        log("idx %d case %s mean_dice %f mean_hd95 %f, mean_jacard %f mean_asd %f" % (i, case, mm[0], mm[1], mm[2], mm[3]))
    if n == 0:
        raise ValueError("inference: no test volumes")
    table = total / n
    for c in range(1, classes):
        log("Mean class (%d) mean_dice %f mean_hd95 %f, mean_jacard %f mean_asd %f" % ((c,) + tuple(table[c - 1][:4])))
    performance, mean_hd95 = float(np.mean(table, axis=0)[0]), float(np.mean(table, axis=0)[1])
    log("Testing performance in best val model) mean_dice:%f mean_hd95:%f" % (performance, mean_hd95))
    if nsd_tolerance is not None:
        mean_nsd = float(np.mean(table, axis=0)[4])
        log("mean_nsd at tolerance %g per class: %s mean_nsd:%f" % (float(nsd_tolerance), " ".join("%f" % v for v in table[:, 4]),
                                                                    mean_nsd))
        return performance, mean_hd95, mean_nsd
    return performance, mean_hd95


def _binary_dc(result: torch.Tensor, reference: torch.Tensor) -> float:
    """medpy.metric.binary.dc as the skin scripts call it — on arrays of DIFFERENT rank (argmax output [B, H, W] or [H, W]
    against the label batch [B, 1, H, W]): the intersection is counted on the numpy-broadcast of the two boolean arrays, the
    sizes on each array alone; 0.0 when both are empty"""
    a, b = result != 0, reference != 0
    sa, sb = int(a.sum()), int(b.sum())
    return 2.0 * int((a & b).sum()) / float(sa + sb) if (sa + sb) else 0.0


def _skin_predict(net, img, tta, window, window_overlap):
    """the class map of one skin batch: the plain argmax, `tta_predict`, or with `window` (the network's input size; `window_overlap`
    defaults to 0.5) `sliding_window_predict`, which takes `tta` along"""
    if window is None:
        if window_overlap is not None:
            raise ValueError(f"window_overlap={window_overlap!r} needs `window`, the network's input size")
        return predict_counts(net(img))[0] if tta is None else tta_predict(net, img, tta)[0]
    return sliding_window_predict(net, img, window, 0.5 if window_overlap is None else window_overlap, tta=tta)[0]


@torch.no_grad()
def skin_val(net, vl_loader, device=None, tta=None, window=None, window_overlap=None) -> float:
    """val of utils_skin.py:97-113: mean over the loader's batches of dc(argmax(softmax(logits), 1).squeeze(0), label batch).
    `tta`: the prediction of `tta_predict` instead of the plain argmax.  `window` (and `window_overlap`, 0.5 when None): the
    prediction of `sliding_window_predict` at the images' own size."""
    device = device or next(net.parameters()).device
    net.eval()
    dc_sum, n = 0.0, 0
    for batch in vl_loader:
        img, lab = batch["image"].to(device), batch["label"].to(device)
        pred = _skin_predict(net, img.float(), tta, window, window_overlap)
        dc_sum += _binary_dc(pred.squeeze(0), lab)
        n += 1
    return dc_sum / max(n, 1)


@torch.no_grad()
def skin_test(net, te_loader, device=None, tta=None, window=None, window_overlap=None) -> Tuple[float, float, float]:
    """test of utils_skin.py:131-170 (batch size 1, as the reference's test loader): (mean dice, pixel accuracy, mean IoU) with
    the ground truth read as `label[0, 0]` and calc_iou(pd > 0.5, gt > 0.5) = |A & B| / |A or B| (0.0 for an empty union,
    utils_skin.py:13-27).  `tta`: the prediction of `tta_predict` instead of the plain argmax; `window` / `window_overlap`: as for
    `skin_val`."""
    device = device or next(net.parameters()).device
    net.eval()
    dc_sum, correct, total, ious, n = 0.0, 0, 0, [], 0
    for batch in te_loader:
        img, lab = batch["image"].float().to(device), batch["label"].float().to(device)
        pred = _skin_predict(net, img, tta, window, window_overlap)
        pd = pred.squeeze(0)
        gt = lab[0, 0]
        correct += int((pd == gt).sum())
        total += gt.numel()
        a, b = pd > 0.5, gt > 0.5
        union = int((a | b).sum())
        ious.append(int((a & b).sum()) / union if union else 0.0)
        dc_sum += _binary_dc(pd, lab)
        n += 1
    return dc_sum / max(n, 1), correct / max(total, 1), float(np.mean(ious)) if ious else 0.0
