"""Device-side Synapse augmentation (data.SegAugmenter, csrc/augment_ops.hip): samples/s of one host process feeding the preset's
batch, and the time of every stage.

    python tools/augment_ops_bench.py --out profiles/augment_ops.json

Batch 24 (the Synapse preset's), 512 x 512 slices -> 224 x 224, Normalize(0.5, 0.5).  Three plans: the costliest (four stages of
warps and blurs on every sample: COSTLIEST below), plans as `draw` makes them (0 .. 4 of the ten operators per sample), and no
operator at all (gather + resize only).  Then every operator alone as a one-stage cenet_augment_ops call, and the resize and
normalize steps that follow.  Every timing is a host clock around work that ends in a device synchronise, after warm-up; the median
of the repeats is reported with their minimum and maximum.  Needs the MI355X: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cenet_amd import data as D, kern  # noqa: E402

STEP_IMAGES_PER_S = 1385  # the Synapse preset's captured training step (README status table)
BATCH, SIDE, OUT = 24, 512, (224, 224)


def rotation(shape, deg):
    a = np.deg2rad(deg)
    return ("affine", *D.centred_affine([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], shape))


def grid_warp(shape, rng, s=0.03):
    return ("grid_warp", rng.normal(0.0, s, (4, 4)) * shape[0], rng.normal(0.0, s, (4, 4)) * shape[1])


def costliest_chain(shape, rng):
    """four stages of warps and blurs: the two kinds of warp and the blur twice (a drawn plan has distinct operators, so at most
    one blur and otherwise cheaper ones in its place: see the per-operator times this tool reports)"""
    return [grid_warp(shape, rng), ("blur", 1.0), rotation(shape, rng.uniform(-40, 40)), ("blur", 1.0)]


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "repeats": repeats}


def rate(t, n):
    return {**t, "samples_per_s_median": n / (t["median_ms"] * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_ops_bench: no GPU (the device path has no fallback and a CPU timing says nothing)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    samples = [(rng.random((SIDE, SIDE)).astype(np.float32), rng.integers(0, 9, (SIDE, SIDE)).astype(np.uint8)) for _ in range(64)]
    sl = D.DeviceSlices(samples, dev)
    aug = D.SegAugmenter(sl, OUT, normalize=(0.5, 0.5), seed=1)
    idx = [int(i) for i in rng.permutation(64)[:BATCH]]
    shape = (SIDE, SIDE)

    plans = {"costliest": aug.plan(idx, [costliest_chain(shape, rng) for _ in idx]), "no_op": aug.plan(idx, [[] for _ in idx])}
    res = {"tool": "tools/augment_ops_bench.py", "device": torch.cuda.get_device_name(0), "batch": BATCH, "slice": [SIDE, SIDE],
           "output": list(OUT), "training_step_images_per_s": STEP_IMAGES_PER_S,
           "timing": "host clock around calls ending in a device synchronise; apply = table upload + cenet_augment_ops + "
                     "cenet_augment_acdc (resize) + normalize", "apply": {}, "stages": {}}
    for name, plan in plans.items():
        res["apply"][name] = rate(timed(lambda: aug.apply(plan), 5, a.repeats), BATCH)
    res["apply"]["draw_and_apply"] = rate(timed(lambda: aug(idx), 5, a.repeats), BATCH)
    res["apply"]["draw_only_host"] = timed(lambda: aug.draw(idx), 5, a.repeats)
    res["costliest_over_training_step"] = res["apply"]["costliest"]["samples_per_s_median"] / STEP_IMAGES_PER_S

    # every operator alone: one stage for the whole batch, tables already on the device
    aug.apply(plans["no_op"])  # (allocates the work buffers)
    one = {"copy": ("copy",), "flip_ud": ("flip_ud",), "flip_lr": ("flip_lr",), "affine_rotate": rotation(shape, 33.0),
           "affine_scale": ("affine", *D.centred_affine([[1 / 0.6, 0], [0, 1 / 1.7]], shape)), "grid_warp": grid_warp(shape, rng),
           "blur_sigma1_radius4": ("blur", 1.0), "blur_sigma4_radius16": ("blur", 4.0), "noise": ("noise", 1.275, 1, 2),
           "contrast": ("contrast", 1.3, 0.0)}
    for name, op in one.items():
        tab, dp = aug.plan(idx, [[op] for _ in idx])
        tab_d, dp_d = torch.from_numpy(tab).to(dev), torch.from_numpy(dp).to(dev)
        res["stages"][name] = timed(lambda: kern.augment_ops(sl.pool_img, sl.pool_lab, tab, dp, tab_d, dp_d, aug._buf["img"],
                                                             aug._buf["lab"], aug.stride, sl.max_h, sl.max_w, BATCH, 1), 3, a.repeats)
    plain = D.SegAugmenter(sl, OUT, seed=1)
    t_resize = timed(lambda: plain.apply(plans["no_op"]), 3, a.repeats)
    res["stages"]["gather_resize_cubic_to_224 (copy stage + cenet_augment_acdc, with table upload)"] = t_resize
    img = torch.rand(BATCH, 1, *OUT, device=dev)
    res["stages"]["normalize"] = timed(lambda: kern.augment_normalize(img, 0.5, 0.5), 3, a.repeats)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
