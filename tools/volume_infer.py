"""Wall time of evaluate.test_single_volume with the resizes on the host (scipy, the reference's way) and on the device
(csrc/volresize.hip), split into resize-in / forward / resize-back / metrics.

ACDC preset with the oracle's deterministic weights (seed 42), one ACDC-like volume (10 x 256 x 216) and one Synapse-like volume
(148 x 512 x 512) from a seed.  Per volume and mode: one warm-up call, five timed calls (torch.cuda.synchronize() on both sides;
median and spread reported), then three instrumented calls in which every part is wrapped with a synchronize on both sides (the
split; its parts do not overlap, so their sum is above the plain call's time; `other` is what the wrappers do not cover: uploads,
the host path's argmax and device-to-host copy, Python).  The surface-distance metrics compare every border voxel of one mask with
every border voxel of the other (--metrics pairs); with random weights a prediction can be noise with millions of border voxels, so
above --metrics-cap pairs the metrics are stubbed out (in BOTH modes) and the line says so.  The cap applies to `pairs` only:
--metrics edt (the exact distance transform, csrc/edt.hip) and auto are linear in the voxels and always timed.
--report adds the metrics alone (`evaluate.label_metrics` on label volumes that are already on the device; one warm-up, median of
five, spread, all methods in this one process): per volume size the network's prediction and a uniform-noise prediction against the
blob labels, under the parent's per-class `metric_percase(method="pairs")` loop, `pairs`, `edt` and `auto`; and the crossover scan
behind `evaluate.AUTO_PAIRS_PER_BOX_VOXEL`: two overlapping balls of growing radius under both methods.  Prints one JSON line.
--tta NAME adds a third mode, `device_tta`: resize="device" with that view set of evaluate.TTA_SETS (its split has `tta_views`, and
`resize_back` is the fused merge).
--window-overlap X adds the mode `device_window`: resize="device" with sliding-window inference (PATCH windows at the volume's own
resolution, no resize; its split has `sw_windows` and `sw_merge`), with the view set of --tta when that is given.
--spacing Z Y X scores in that voxel spacing (hd95 / assd in its unit, the fp64 kernels of csrc/edt.hip), --nsd TAU adds the
normalised surface Dice at that tolerance.  With --spacing, --report is the SPACED report instead (`spaced_report`, written to
--report-out as well, profiles/volume_metrics_spacing.json): per volume the spaced transform and the spaced `label_metrics` beside
the unit-spacing path on the same volume and box (median of --reps runs), the host route they replace (download, then scipy's
`distance_transform_edt(sampling=)` per class and direction; median of --host-reps), and the crossover scan behind
`evaluate.AUTO_PAIRS_PER_BOX_VOXEL_SPACED` with its interpolated crossing.
    python tools/volume_infer.py [--bf16] [--only acdc|synapse] [--metrics pairs|edt|auto] [--metrics-cap 5e10] [--report] [--tta NAME]
                                 [--spacing Z Y X] [--nsd TAU] [--reps 20] [--host-reps 3] [--report-out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import scipy.ndimage
import torch

from cenet_amd import build, evaluate, kern
from cenet_amd.networks import CENet
from oracle import cenet_oracle as O
from oracle.golden_cases import MODEL_CONFIGS, config_from_kwargs

VOLUMES = {"acdc": (10, 256, 216), "synapse": (148, 512, 512)}
PATCH = (224, 224)
K = 4


def make_volume(shape, seed):
    """smooth intensities in [0, 1] (low-resolution noise, linearly upsampled) and blob labels cut from a second field"""
    rng = np.random.default_rng(seed)
    low = [rng.random((max(2, shape[0] // 4), 8, 8)) for _ in range(2)]
    up = [scipy.ndimage.zoom(v, [s / l for s, l in zip(shape, v.shape)], order=1) for v in low]
    image = up[0].astype(np.float32)
    label = np.clip((up[1] * K).astype(np.int64), 0, K - 1).astype(np.float32)
    return torch.from_numpy(image)[None], torch.from_numpy(label)[None]


class Parts:
    """accumulates the wall time of the wrapped parts of one call"""

    def __init__(self):
        self.t = {}

    def wrap(self, name, fn):
        def timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            key = name(*a, **k) if callable(name) else name
            self.t[key] = self.t.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
            return out
        return timed


SURFACE = {}  # spacing= / nsd_tolerance= of --spacing / --nsd, handed to test_single_volume


def call(net, image, label, mode, dev, tta=None, window_overlap=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=32, device=dev, resize=mode, tta=tta,
                                    **({} if window_overlap is None else {"window_overlap": window_overlap}), **SURFACE)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, m


def split_call(net, image, label, mode, dev, tta=None, window_overlap=None):
    """one call with every part wrapped; the wrappers are taken off again"""
    p = Parts()
    saved = (scipy.ndimage.zoom, kern.vol_resize_cubic, kern.argmax_resize_counts, evaluate.label_metrics, net.forward,
             kern.tta_views, kern.tta_argmax_resize_counts, kern.sw_windows, kern.sw_merge_counts)
    kern.tta_views = p.wrap("tta_views", saved[5])
    kern.tta_argmax_resize_counts = p.wrap("resize_back", saved[6])
    kern.sw_windows = p.wrap("sw_windows", saved[7])
    kern.sw_merge_counts = p.wrap("sw_merge", saved[8])
    scipy.ndimage.zoom = p.wrap(lambda *a, **k: "resize_in" if k.get("order", 3) == 3 else "resize_back", saved[0])
    kern.vol_resize_cubic = p.wrap("resize_in", saved[1])
    kern.argmax_resize_counts = p.wrap("resize_back", saved[2])
    evaluate.label_metrics = p.wrap("metrics", saved[3])
    net.forward = p.wrap("forward", saved[4])
    try:
        total, _ = call(net, image, label, mode, dev, tta, window_overlap)
    finally:
        scipy.ndimage.zoom, kern.vol_resize_cubic, kern.argmax_resize_counts, evaluate.label_metrics = saved[:4]
        kern.tta_views, kern.tta_argmax_resize_counts, kern.sw_windows, kern.sw_merge_counts = saved[5:]
        del net.forward
    p.t["other"] = total - sum(p.t.values())
    p.t["total"] = total
    return p.t


def timed(fn, reps=5):
    """one warm-up, then `reps` calls with a synchronize on both sides: {median, spread, runs} in ms"""
    fn()
    runs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(runs), 3), "spread": round(max(runs) - min(runs), 3), "runs": [round(v, 3) for v in runs]}


def border_pairs(pred, lab, classes):
    """largest border-pair count of a class and the totals, from the table label_metrics itself works from"""
    _, _, tab = evaluate._label_table(pred, lab, classes)
    return max(int(tab[c, 3]) * int(tab[c, 4]) for c in range(1, classes)), int(tab[1:, 3].sum()), int(tab[1:, 4].sum())


def metrics_report(net, dev, cap, only):
    """the metrics alone, every method in this process"""
    rep = {"volumes": {}, "crossover": []}
    for name, shape in VOLUMES.items():
        if only and name != only:
            continue
        image, label = make_volume(shape, seed=sum(shape))
        lab = label[0].to(dev)
        net_pred, _ = evaluate.predict_volume(net, image[0].to(dev), PATCH)
        noise = torch.from_numpy(np.random.default_rng(1).integers(0, K, shape).astype(np.float32)).to(dev)
        for tag, pred in (("net_pred", net_pred), ("noise_pred", noise)):
            pairs, nbp, nbg = border_pairs(pred, lab, K)
            e = {"shape": list(shape), "classes": K, "max_border_pairs": pairs, "border_voxels_pred": nbp, "border_voxels_gt": nbg}
            if pairs <= cap:
                e["parent_per_class_loop"] = timed(lambda: [evaluate.metric_percase(pred == c, lab == c, method="pairs")
                                                            for c in range(1, K)])
                e["pairs"] = timed(lambda: evaluate.label_metrics(pred, lab, K, method="pairs"))
            else:
                e["parent_per_class_loop"] = e["pairs"] = "capped"
            e["edt"] = timed(lambda: evaluate.label_metrics(pred, lab, K, method="edt"))
            e["auto"] = timed(lambda: evaluate.label_metrics(pred, lab, K, method="auto"))
            if pairs <= cap:
                e["equal"] = evaluate.label_metrics(pred, lab, K, method="pairs") == evaluate.label_metrics(pred, lab, K, method="edt")
            rep["volumes"][f"{name}/{tag}"] = e
        if name == "synapse":  # noise against noise with the Synapse class count: every class of both volumes is all border
            rng = np.random.default_rng(2)
            p9, g9 = (torch.from_numpy(rng.integers(0, 9, shape).astype(np.float32)).to(dev) for _ in range(2))
            pairs, nbp, nbg = border_pairs(p9, g9, 9)
            rep["volumes"]["synapse/noise_vs_noise_k9"] = {
                "shape": list(shape), "classes": 9, "max_border_pairs": pairs, "border_voxels_pred": nbp, "border_voxels_gt": nbg,
                "parent_per_class_loop": "capped", "pairs": "capped",
                "edt": timed(lambda: evaluate.label_metrics(p9, g9, 9, kind="synapse", method="edt"))}
            del p9, g9
    if not only:
        # crossover: two overlapping balls in 160 x 256 x 256, one class; cost estimate of `auto` = na * nb against the box volume
        D, H, W = 160, 256, 256
        zz, yy, xx = np.ogrid[:D, :H, :W]
        for r in (3, 6, 12, 24, 36, 48, 64, 72):
            a = ((zz - 80) ** 2 + (yy - 128) ** 2 + (xx - 120) ** 2 <= r * r).astype(np.float32)
            b = ((zz - 80) ** 2 + (yy - 128) ** 2 + (xx - 120 - max(1, r // 4)) ** 2 <= r * r).astype(np.float32)
            ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            _, _, tab = evaluate._label_table(ta, tb, 2)
            row = [int(v) for v in tab[1]]
            box = [max(-row[8 + k], -row[14 + k]) - min(row[5 + k], row[11 + k]) + 1 for k in range(3)]
            vol = box[0] * box[1] * box[2]
            p = timed(lambda: evaluate.label_metrics(ta, tb, 2, method="pairs"))
            e = timed(lambda: evaluate.label_metrics(ta, tb, 2, method="edt"))
            rep["crossover"].append({"radius": r, "na": row[3], "nb": row[4], "box": box, "pairs_per_box_voxel": round(row[3] * row[4] / vol, 2),
                                     "pairs_ms": p["median"], "pairs_spread": p["spread"], "edt_ms": e["median"], "edt_spread": e["spread"]})
    rep["auto_pairs_per_box_voxel"] = evaluate.AUTO_PAIRS_PER_BOX_VOXEL
    return rep


def _ball_pair(dev, r, D=160, H=256, W=256):
    """the crossover scan's two overlapping balls of radius r, and (na, nb, union box) from label_metrics' own table"""
    zz, yy, xx = np.ogrid[:D, :H, :W]
    a = ((zz - 80) ** 2 + (yy - 128) ** 2 + (xx - 120) ** 2 <= r * r).astype(np.float32)
    b = ((zz - 80) ** 2 + (yy - 128) ** 2 + (xx - 120 - max(1, r // 4)) ** 2 <= r * r).astype(np.float32)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    _, _, tab = evaluate._label_table(ta, tb, 2)
    row = [int(v) for v in tab[1]]
    box = [max(-row[8 + k], -row[14 + k]) - min(row[5 + k], row[11 + k]) + 1 for k in range(3)]
    return ta, tb, row[3], row[4], box


def host_route(pred, lab, classes, spacing):
    """what a user did without `spacing=`: download both label maps, then medpy's algorithm on scipy per class and direction"""
    p, g = pred.cpu().numpy(), lab.cpu().numpy()
    out = []
    for c in range(1, classes):
        if (p == c).any() and (g == c).any():
            d1 = O.surface_distances(p == c, g == c, voxelspacing=spacing)
            d2 = O.surface_distances(g == c, p == c, voxelspacing=spacing)
            out.append((float(np.percentile(np.hstack((d1, d2)), 95)), float(np.mean((d1.mean(), d2.mean())))))
        else:
            out.append((0.0, 0.0))
    return out


def timed_host(fn, reps):
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        runs.append((time.perf_counter() - t0) * 1e3)
        print(f"  host route run: {runs[-1]:.0f} ms", file=sys.stderr, flush=True)
    return {"median": round(statistics.median(runs), 3), "spread": round(max(runs) - min(runs), 3), "runs": [round(v, 3) for v in runs]}


def spaced_report(net, dev, only, spacing, nsd, reps, host_reps):
    """the metrics alone with a voxel spacing, beside the unit-spacing path and the host route"""
    rep = {"spacing": list(spacing), "nsd_tolerance": nsd, "reps": reps, "host_reps": host_reps, "volumes": {}, "crossover": []}
    for name, shape in VOLUMES.items():
        if only and name != only:
            continue
        print(f"spaced report: {name}", file=sys.stderr, flush=True)
        image, label = make_volume(shape, seed=sum(shape))
        lab = label[0].to(dev)
        net_pred, _ = evaluate.predict_volume(net, image[0].to(dev), PATCH)
        noise = torch.from_numpy(np.random.default_rng(1).integers(0, K, shape).astype(np.float32)).to(dev)
        # the transform alone, whole volume: the labels' class-1 border as the feature set
        _, blg, _ = evaluate._label_table(lab, lab, K)
        n = blg.numel()
        ti, di = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        tf, df = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
        general = (spacing[0], spacing[1], spacing[2] * 1.0009765625)  # sy != sx: the fp64 y pass as well
        rep["volumes"][f"{name}/transform"] = {
            "shape": list(shape),
            "unit_int32": timed(lambda: kern.edt_sq_raw(blg, 1, ti, di, *shape), reps),
            "spaced_fp64": timed(lambda: kern.edt_sq_spaced_raw(blg, 1, ti, tf, df, *shape, spacing), reps),
            "spaced_fp64_sy_ne_sx": timed(lambda: kern.edt_sq_spaced_raw(blg, 1, ti, tf, df, *shape, general), reps)}
        del ti, di, tf, df
        for tag, pred in (("net_pred", net_pred), ("noise_pred", noise)):
            pairs, nbp, nbg = border_pairs(pred, lab, K)
            e = {"shape": list(shape), "classes": K, "max_border_pairs": pairs, "border_voxels_pred": nbp, "border_voxels_gt": nbg}
            e["edt_unit"] = timed(lambda: evaluate.label_metrics(pred, lab, K, method="edt"), reps)
            e["edt_spaced"] = timed(lambda: evaluate.label_metrics(pred, lab, K, method="edt", spacing=spacing, nsd_tolerance=nsd), reps)
            e["auto_spaced"] = timed(lambda: evaluate.label_metrics(pred, lab, K, method="auto", spacing=spacing, nsd_tolerance=nsd), reps)
            if tag == "net_pred" and host_reps > 0:
                e["host_scipy"] = timed_host(lambda: host_route(pred, lab, K, spacing), host_reps)
                want = host_route(pred, lab, K, spacing)
                got = evaluate.label_metrics(pred, lab, K, method="edt", spacing=spacing)
                e["max_rel_diff_to_host"] = max(abs(g[k] - w[j]) / max(w[j], 1e-300) for g, w in zip(got, want)
                                                for k, j in ((1, 0), (3, 1)) if w[j] > 0)
            rep["volumes"][f"{name}/{tag}"] = e
    if not only:
        for r in (3, 6, 12, 24, 36, 48, 64, 72, 84):
            ta, tb, na, nb, box = _ball_pair(dev, r)
            vol = box[0] * box[1] * box[2]
            p = timed(lambda: evaluate.label_metrics(ta, tb, 2, method="pairs", spacing=spacing), reps)
            e = timed(lambda: evaluate.label_metrics(ta, tb, 2, method="edt", spacing=spacing), reps)
            rep["crossover"].append({"radius": r, "na": na, "nb": nb, "box": box, "pairs_per_box_voxel": round(na * nb / vol, 2),
                                     "pairs_ms": p["median"], "pairs_spread": p["spread"], "edt_ms": e["median"], "edt_spread": e["spread"]})
        # the crossing: linear interpolation of (pairs - edt) between the last row where pairs wins and the next
        rows = rep["crossover"]
        rep["crossing_pairs_per_box_voxel"] = None
        for lo, hi in zip(rows, rows[1:]):
            dl, dh = lo["pairs_ms"] - lo["edt_ms"], hi["pairs_ms"] - hi["edt_ms"]
            if dl <= 0 < dh:
                x0, x1 = lo["pairs_per_box_voxel"], hi["pairs_per_box_voxel"]
                rep["crossing_pairs_per_box_voxel"] = round(x0 + (x1 - x0) * (-dl) / (dh - dl), 1)
    rep["auto_pairs_per_box_voxel_spaced"] = evaluate.AUTO_PAIRS_PER_BOX_VOXEL_SPACED
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--only", choices=sorted(VOLUMES))
    ap.add_argument("--metrics-cap", type=float, default=5e10)
    ap.add_argument("--metrics", choices=evaluate.METHODS, default="auto")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--tta", choices=sorted(evaluate.TTA_SETS), default=None,
                    help="also time resize='device' with this test-time augmentation set (entry `device_tta`)")
    ap.add_argument("--window-overlap", type=float, default=None,
                    help="also time resize='device' with sliding-window inference at this overlap in [0, 1) (entry `device_window`; "
                         "it takes --tta along)")
    ap.add_argument("--spacing", type=float, nargs=3, metavar=("Z", "Y", "X"), default=None,
                    help="voxel spacing: hd95 / assd in its unit; with --report: the spaced report")
    ap.add_argument("--nsd", type=float, default=None, help="tolerance of the normalised surface Dice (the unit of --spacing)")
    ap.add_argument("--reps", type=int, default=20, help="timed runs per entry of the spaced report")
    ap.add_argument("--host-reps", type=int, default=3, help="timed runs of the host route in the spaced report (0: leave it out)")
    ap.add_argument("--report-out", default=None, help="also write the spaced report (with the run's header) to this file")
    ap.add_argument("--report-only", action="store_true", help="skip the test_single_volume timings")
    args = ap.parse_args()
    if args.spacing is not None:
        SURFACE["spacing"] = tuple(args.spacing)
    if args.nsd is not None:
        SURFACE["nsd_tolerance"] = args.nsd
    dev = torch.device("cuda:0")
    kw = MODEL_CONFIGS["acdc"]["kw"]
    net = CENet(**kw)
    net.load_state_dict(O.make_state_dict(config_from_kwargs(kw), seed=42), strict=True)
    net = net.to(dev).eval()
    kern.set_compute_bf16(args.bf16)
    res = {"tool": "volume_infer", "device": torch.cuda.get_device_name(0), "kernel_src_sha16": build.source_sha16(),
           "precision": "bf16" if args.bf16 else "fp32", "patch": list(PATCH), "batch_slices": 32, "unit": "ms", "metrics_method": args.metrics, "tta": args.tta, "window_overlap": args.window_overlap,
           "spacing": args.spacing, "nsd_tolerance": args.nsd, "volumes": {}}
    real_metric = evaluate.label_metrics
    for name, shape in VOLUMES.items():
        if (args.only and name != args.only) or args.report_only:
            continue
        image, label = make_volume(shape, seed=sum(shape))
        # how much work the surface metrics would be on this prediction
        pred, _ = evaluate.predict_volume(net, image[0].to(dev), PATCH)
        lab_d = label[0].to(dev)
        pairs = border_pairs(pred, lab_d, K)[0]
        timed_metrics = args.metrics != "pairs" or pairs <= args.metrics_cap
        if timed_metrics:
            evaluate.label_metrics = lambda p, g, k, kind="acdc", method=args.metrics, **kw: real_metric(p, g, k, kind, method, **kw)
        else:
            evaluate.label_metrics = lambda p, g, k, kind="acdc", method=None, **kw: [(0.0,) * (5 if args.nsd else 4)] * (k - 1)
        entry = {"shape": list(shape), "max_border_pairs": pairs, "metrics_timed": timed_metrics}
        preds = {}
        modes = [("host", None, None), ("device", None, None)] + ([("device_tta", args.tta, None)] if args.tta else []) + \
            ([("device_window", args.tta, args.window_overlap)] if args.window_overlap is not None else [])
        for mode, tta, wov in modes:
            how = mode.split("_")[0]
            call(net, image, label, how, dev, tta, wov)  # warm-up
            runs = [call(net, image, label, how, dev, tta, wov)[0] for _ in range(5)]
            splits = [split_call(net, image, label, how, dev, tta, wov) for _ in range(3)]
            keys = sorted(set().union(*splits))
            entry[mode] = {"total_runs": [round(v, 3) for v in runs], "total_median": round(statistics.median(runs), 3),
                           "total_spread": round(max(runs) - min(runs), 3),
                           "split_median": {k: round(statistics.median(s.get(k, 0.0) for s in splits), 3) for k in keys}}
            preds[mode] = evaluate.val_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize=how, tta=tta,
                                                     window_overlap=wov)
        evaluate.label_metrics = real_metric
        entry["speedup"] = round(entry["host"]["total_median"] / entry["device"]["total_median"], 3)
        entry["class_dice"] = {m: [round(v, 6) for v in preds[m]] for m in preds}
        entry["class_dice_equal"] = preds["host"] == preds["device"]
        res["volumes"][name] = entry
    if args.report and args.spacing is not None:
        res["metrics_spacing"] = spaced_report(net, dev, args.only, tuple(args.spacing), args.nsd, args.reps, args.host_reps)
        if args.report_out:
            with open(args.report_out, "w") as f:
                f.write(json.dumps({k: v for k, v in res.items() if k != "volumes"}) + "\n")
    elif args.report:
        res["metrics"] = metrics_report(net, dev, args.metrics_cap, args.only)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
