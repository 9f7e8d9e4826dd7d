"""Device-side skin augmentation (data.ComposeAugmenter, csrc/augment_image_ops.hip): samples/s of one host process feeding the
preset's batch, the time of every stage, of the two elastic-field passes and of the min-max pair.

    python tools/augment_image_ops_bench.py --out profiles/augment_image_ops.json

Batch 8 (the skin preset's), 3 x 512 x 512, min-max.  Three plans: the costliest (rotation with mirror border, k = 7 blur and the
sigma = 50 elastic warp on every sample), plans as `draw` makes them, and no operator at all (gather only).  Then every operator
alone as a one-stage cenet_augment_image_ops call and the min-max pair: a host clock around work that ends in a device synchronise,
after warm-up; the median of the repeats is reported with their minimum and maximum.  The elastic one-stage call holds three
kernels (field axis 0, field axis 1, the warp): their separate durations come from the profiler's kernel records of the same calls
(torch.profiler, device time per kernel name) and are reported as "unmeasured" when the profiler returns none.
Needs the MI355X: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cenet_amd import data as D, kern  # noqa: E402

STEP_IMAGES_PER_S = 197  # the skin preset's captured training step (README status table)
BATCH, CH, SIDE = 8, 3, 512
KERNELS = ("aimg_field_axis0_kernel", "aimg_field_axis1_kernel", "aimg_stage_kernel", "amm_partial_kernel", "amm_apply_kernel")


def rotation(shape, deg, mode="mirror"):
    a = np.deg2rad(deg)
    return ("affine", *D.centred_affine([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], shape), mode)


def elastic(rng, mode="mirror"):
    k0, k1 = (int(v) for v in rng.integers(0, 2 ** 32, 2, dtype=np.uint64))
    return ("elastic", 1.0, k0, k1, mode)


def costliest_chain(shape, rng):
    return [rotation(shape, rng.uniform(-30, 30)), ("blur", 7), elastic(rng)]


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


def kernel_times(fn, repeats):
    """device time per launch of the kernels of KERNELS over `repeats` calls of fn, from the profiler's kernel records"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(repeats):
                fn()
            torch.cuda.synchronize()
        per = {k: [] for k in KERNELS}
        for ev in prof.events():
            for k in KERNELS:
                if k in ev.name:
                    per[k].append(float(getattr(ev, "device_time", getattr(ev, "cuda_time", 0.0))) * 1e-3)
        out = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "launches": len(v)}
               for k, v in per.items() if v}
        return out or "unmeasured (the profiler returned no kernel records)"
    except Exception as e:  # noqa: BLE001 (a profiler that is not there leaves the host-clock numbers standing)
        return f"unmeasured ({type(e).__name__}: {e})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_image_ops_bench: no GPU (the device path has no fallback and a CPU timing says nothing)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    shape = (SIDE, SIDE)
    im = D.DeviceImages([((rng.random((CH, *shape)) * 255).astype(np.float32), rng.integers(0, 2, shape).astype(np.uint8))
                         for _ in range(24)], dev)
    aug = D.ComposeAugmenter(im, seed=1)
    idx = [int(i) for i in rng.permutation(24)[:BATCH]]

    plans = {"costliest": aug.plan(idx, [costliest_chain(shape, rng) for _ in idx]), "no_op": aug.plan(idx, [[] for _ in idx])}
    res = {"tool": "tools/augment_image_ops_bench.py", "device": torch.cuda.get_device_name(0), "batch": BATCH,
           "image": [CH, SIDE, SIDE], "training_step_images_per_s": STEP_IMAGES_PER_S,
           "timing": "host clock around calls ending in a device synchronise; apply = table upload + cenet_augment_image_ops (field "
                     "passes + stages) + cenet_augment_minmax; kernels = device time per launch from the profiler's kernel records",
           "apply": {}, "stages": {}}
    for name, plan in plans.items():
        res["apply"][name] = rate(timed(lambda: aug.apply(plan), 5, a.repeats), BATCH)
    res["apply"]["draw_and_apply"] = rate(timed(lambda: aug(idx), 5, a.repeats), BATCH)
    res["apply"]["draw_only_host"] = timed(lambda: aug.draw(idx), 5, a.repeats)
    res["costliest_over_training_step"] = res["apply"]["costliest"]["samples_per_s_median"] / STEP_IMAGES_PER_S

    # every operator alone: one stage for the whole batch, tables already on the device
    buf = aug._buf
    one = {"copy": ("copy",), "flip_ud": ("flip_ud",), "flip_lr": ("flip_lr",), "affine_rotate_constant": rotation(shape, 23.0, "constant"),
           "affine_rotate_mirror": rotation(shape, 23.0), "blur_k3_radius1": ("blur", 3), "blur_k7_radius3": ("blur", 7),
           "blur_radius16": ("blur", D.gaussian_weights(4.0)[1]), "brightness_contrast": ("brightness_contrast", 1.1, 12.0, 0.0, 255.0),
           "elastic_sigma50_radius200 (field axis 0 + field axis 1 + warp)": elastic(rng)}
    calls = {}
    for name, op in one.items():
        tab, dp, fw = aug.plan(idx, [[op] for _ in idx])
        tab_d, dp_d = torch.from_numpy(tab).to(dev), torch.from_numpy(dp).to(dev)
        fw_d = None if fw is None else torch.from_numpy(fw).to(dev)
        calls[name] = (lambda tab=tab, dp=dp, fw=fw, tab_d=tab_d, dp_d=dp_d, fw_d=fw_d: kern.augment_image_ops(
            im.pool_img, im.pool_lab, tab, dp, tab_d, dp_d, fw, fw_d, buf["field"] if fw is not None else None, buf["img"],
            buf["lab"], None, len(im), CH, SIDE, SIDE, BATCH, 1))
        res["stages"][name] = timed(calls[name], 3, a.repeats)
    x = torch.rand(BATCH * CH * SIDE * SIDE, device=dev) * 255
    y = torch.empty_like(x)
    minmax = lambda: kern.augment_minmax(x, y, buf["part"], BATCH, CH * SIDE * SIDE)  # noqa: E731
    res["stages"]["minmax (partial + apply)"] = timed(minmax, 3, a.repeats)
    res["kernels"] = {"elastic_one_stage": kernel_times(calls["elastic_sigma50_radius200 (field axis 0 + field axis 1 + warp)"], 10),
                      "minmax": kernel_times(minmax, 10)}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
