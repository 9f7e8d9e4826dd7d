"""Wall time of evaluate.test_single_volume with the resizes on the host (scipy, the reference's way) and on the device
(csrc/volresize.hip), split into resize-in / forward / resize-back / metrics.

ACDC preset with the oracle's deterministic weights (seed 42), one ACDC-like volume (10 x 256 x 216) and one Synapse-like volume
(148 x 512 x 512) from a seed.  Per volume and mode: one warm-up call, five timed calls (torch.cuda.synchronize() on both sides;
median and spread reported), then three instrumented calls in which every part is wrapped with a synchronize on both sides (the
split; its parts do not overlap, so their sum is above the plain call's time; `other` is what the wrappers do not cover: uploads,
the host path's argmax and device-to-host copy, Python).  The surface-distance metrics compare every border voxel of one mask with
every border voxel of the other; with random weights a prediction can be noise with millions of border voxels, so above
--metrics-cap pairs the metrics are stubbed out (in BOTH modes) and the line says so.  Prints one JSON line.
    python tools/volume_infer.py [--bf16] [--only acdc|synapse] [--metrics-cap 5e10]"""
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


def call(net, image, label, mode, dev):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=32, device=dev, resize=mode)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, m


def split_call(net, image, label, mode, dev):
    """one call with every part wrapped; the wrappers are taken off again"""
    p = Parts()
    saved = (scipy.ndimage.zoom, kern.vol_resize_cubic, kern.argmax_resize_counts, evaluate.metric_percase, net.forward)
    scipy.ndimage.zoom = p.wrap(lambda *a, **k: "resize_in" if k.get("order", 3) == 3 else "resize_back", saved[0])
    kern.vol_resize_cubic = p.wrap("resize_in", saved[1])
    kern.argmax_resize_counts = p.wrap("resize_back", saved[2])
    evaluate.metric_percase = p.wrap("metrics", saved[3])
    net.forward = p.wrap("forward", saved[4])
    try:
        total, _ = call(net, image, label, mode, dev)
    finally:
        scipy.ndimage.zoom, kern.vol_resize_cubic, kern.argmax_resize_counts, evaluate.metric_percase = saved[:4]
        del net.forward
    p.t["other"] = total - sum(p.t.values())
    p.t["total"] = total
    return p.t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--only", choices=sorted(VOLUMES))
    ap.add_argument("--metrics-cap", type=float, default=5e10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = MODEL_CONFIGS["acdc"]["kw"]
    net = CENet(**kw)
    net.load_state_dict(O.make_state_dict(config_from_kwargs(kw), seed=42), strict=True)
    net = net.to(dev).eval()
    kern.set_compute_bf16(args.bf16)
    res = {"tool": "volume_infer", "device": torch.cuda.get_device_name(0), "kernel_src_sha16": build.source_sha16(),
           "precision": "bf16" if args.bf16 else "fp32", "patch": list(PATCH), "batch_slices": 32, "unit": "ms", "volumes": {}}
    real_metric = evaluate.metric_percase
    for name, shape in VOLUMES.items():
        if args.only and name != args.only:
            continue
        image, label = make_volume(shape, seed=sum(shape))
        # how much work the surface metrics would be on this prediction
        pred, _ = evaluate.predict_volume(net, image[0].to(dev), PATCH)
        lab_d = label[0].to(dev)
        pairs = 0
        for c in range(1, K):
            na, nb = (int(evaluate.surface_points(v == c).shape[0]) for v in (pred, lab_d))
            pairs = max(pairs, na * nb)
        timed_metrics = pairs <= args.metrics_cap
        if not timed_metrics:
            evaluate.metric_percase = lambda p, g: (0.0, 0.0, 0.0, 0.0)
        entry = {"shape": list(shape), "max_border_pairs": pairs, "metrics_timed": timed_metrics}
        preds = {}
        for mode in ("host", "device"):
            call(net, image, label, mode, dev)  # warm-up
            runs = [call(net, image, label, mode, dev)[0] for _ in range(5)]
            splits = [split_call(net, image, label, mode, dev) for _ in range(3)]
            keys = sorted(set().union(*splits))
            entry[mode] = {"total_runs": [round(v, 3) for v in runs], "total_median": round(statistics.median(runs), 3),
                           "total_spread": round(max(runs) - min(runs), 3),
                           "split_median": {k: round(statistics.median(s.get(k, 0.0) for s in splits), 3) for k in keys}}
            preds[mode] = evaluate.val_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize=mode)
        evaluate.metric_percase = real_metric
        entry["speedup"] = round(entry["host"]["total_median"] / entry["device"]["total_median"], 3)
        entry["class_dice"] = {m: [round(v, 6) for v in preds[m]] for m in preds}
        entry["class_dice_equal"] = preds["host"] == preds["device"]
        res["volumes"][name] = entry
    print(json.dumps(res))


if __name__ == "__main__":
    main()
