"""Sliding-window inference: the two launches of csrc/sliding_window.hip (kern.sw_windows, kern.sw_merge_counts) against the torch
composition of the same result on the device — crops of a padded copy for the window batch; for the merge a softmax over the window
batch (un-viewed per view), times the weight map, accumulated window by window into a padded canvas, divided by the weight sum,
argmax.  The composition is the yardstick; the kernels are never one for themselves.

    python tools/sw_bench.py --out profiles/sliding_window.json

Shapes: n = 8, K = 9, 512 x 512 with 224 windows at overlap 0.5 (a Synapse chunk: 4 x 4 = 16 windows per slice by nnU-Net's rule) and
n = 32, K = 4, 256 x 216 with 224 windows (an ACDC chunk: two windows along y, one padded window along x); no augmentation and
"flips"; logits in fp32 and bf16.  The two routes run alternately in one process; a sample is a device-event time around `--inner`
back-to-back calls, divided by their number; the median of the samples is reported with their minimum and maximum.  The two routes'
class maps are compared before anything is timed.  Beside every time: the bytes the launch must move when every element is touched
once, and the rate that makes, next to the copy rate the project quotes.
--volume adds one 148 x 512 x 512 volume through evaluate.synapse_test_single_volume(resize="device") with and without
window_overlap=0.5 (the Synapse preset with the oracle's deterministic weights; wall time only: random weights and a synthetic
volume say nothing about accuracy).  Needs the MI355X: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cenet_amd import build, evaluate, kern  # noqa: E402

HBM_MEASURED_TBS = 6.29  # float4 copy on the MI355X


def codes(mask):
    return [g for g in range(8) if mask >> g & 1]


def torch_unview(v, g):
    if g & 1:
        v = torch.flip(v, (-1,))
    if g & 2:
        v = torch.flip(v, (-2,))
    if g & 4:
        v = v.transpose(-1, -2)
    return v


def _pads(o, P, L):
    """padding before and after an axis so that every window lies inside the padded axis"""
    return max(0, -o[0]), max(0, o[-1] + P - L)


def windows_composition(x, oy, ox, P):
    n, C, H, W = x.shape
    (ty, by), (lx, rx) = _pads(oy, P, H), _pads(ox, P, W)
    xp = torch.nn.functional.pad(x, (lx, rx, ty, by))
    return torch.stack([xp[:, :, y0 + ty:y0 + ty + P, x0 + lx:x0 + lx + P] for y0 in oy for x0 in ox], dim=1).reshape(-1, C, P, P)


def merge_composition(logits, mask, n, oy, ox, wmap, P, H, W):
    T, NB, K = logits.shape[:3]
    (ty, by), (lx, rx) = _pads(oy, P, H), _pads(ox, P, W)
    acc = torch.zeros(n, K, H + ty + by, W + lx + rx, device=logits.device)
    wsum = torch.zeros(H + ty + by, W + lx + rx, device=logits.device)
    prob = None
    for t, g in enumerate(codes(mask)):
        p = torch.softmax(torch_unview(logits[t].float(), g), dim=1)
        prob = p if prob is None else prob + p
    prob = (prob * wmap).reshape(n, len(oy), len(ox), K, P, P)
    for iy, y0 in enumerate(oy):
        for ix, x0 in enumerate(ox):
            acc[:, :, y0 + ty:y0 + ty + P, x0 + lx:x0 + lx + P] += prob[:, iy, ix]
            wsum[y0 + ty:y0 + ty + P, x0 + lx:x0 + lx + P] += wmap
    acc = acc[:, :, ty:ty + H, lx:lx + W] / (wsum[ty:ty + H, lx:lx + W] * T)
    top, am = acc.max(dim=1)
    return am.float(), top


def timed_pair(fa, fb, warmup, repeats, inner):
    """alternating samples of two routes: device events around `inner` calls each"""
    out = ([], [])
    for _ in range(warmup):
        fa(), fb()
    for _ in range(repeats):
        for ts, fn in zip(out, (fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / inner)
    return tuple({"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "repeats": repeats,
                  "calls_per_sample": inner} for ts in out)


def volume_times(dev, reps):
    from cenet_amd.networks import CENet
    from oracle import cenet_oracle as O
    from oracle.golden_cases import MODEL_CONFIGS, config_from_kwargs
    import scipy.ndimage
    kw = MODEL_CONFIGS["synapse"]["kw"]
    K = kw["num_classes"]
    net = CENet(**kw)
    net.load_state_dict(O.make_state_dict(config_from_kwargs(kw), seed=42), strict=True)
    net = net.to(dev).eval()
    shape = (148, 512, 512)
    rng = np.random.default_rng(sum(shape))
    low = [rng.random((37, 8, 8)) for _ in range(2)]
    up = [scipy.ndimage.zoom(v, [s / l for s, l in zip(shape, v.shape)], order=1) for v in low]
    image = torch.from_numpy(up[0].astype(np.float32))[None]
    label = torch.from_numpy(np.clip((up[1] * K).astype(np.int64), 0, K - 1).astype(np.float32))[None]
    real = evaluate.label_metrics
    evaluate.label_metrics = lambda p, g, k, kind="acdc", **kw_: [(0.0, 0.0)] * (k - 1)  # the prediction alone, in both modes
    out = {"shape": list(shape), "classes": K, "patch": [224, 224], "batch_slices": 32, "metrics": "stubbed out in both modes",
           "unit": "ms"}
    try:
        for tag, extra in (("resize", {}), ("window_overlap_0.5", {"window_overlap": 0.5})):
            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                evaluate.synapse_test_single_volume(image, label, net, K, patch_size=(224, 224), batch_slices=32, device=dev,
                                                    resize="device", **extra)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            run()
            runs = [run() for _ in range(reps)]
            out[tag] = {"median": round(statistics.median(runs), 3), "min": round(min(runs), 3), "max": round(max(runs), 3),
                        "runs": len(runs)}
            print(json.dumps({tag: out[tag]}), flush=True)
    finally:
        evaluate.label_metrics = real
    out["windows_per_slice"] = len(kern.sw_origins(512, 224, 0.5)) ** 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--volume", action="store_true")
    ap.add_argument("--volume-reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sw_bench: no GPU (the kernels have no fallback and a CPU timing says nothing)")
    dev = torch.device("cuda:0")
    rows, ok, P = [], True, 224
    for n, K, H, W in ((8, 9, 512, 512), (32, 4, 256, 216)):
        oy, ox = kern.sw_origins(H, P, 0.5), kern.sw_origins(W, P, 0.5)
        nb = n * len(oy) * len(ox)
        w1 = torch.from_numpy(kern.sw_weights(P)).to(dev)
        wmap = w1[:, None] * w1[None, :]
        g = torch.Generator(device="cpu").manual_seed(n * 100 + K)
        x = torch.randn(n, 1, H, W, generator=g).to(dev)
        out = torch.empty(nb, 1, P, P, device=dev)
        kern.sw_windows(x, out, oy, ox, n, 1, H, W, P, P)
        same = bool(torch.equal(out, windows_composition(x, oy, ox, P)))
        ok = ok and same
        k, c = timed_pair(lambda: kern.sw_windows(x, out, oy, ox, n, 1, H, W, P, P), lambda: windows_composition(x, oy, ox, P), 3,
                          a.repeats, a.inner)
        nbytes = out.numel() * 4 * 2  # every window pixel written once, and read once where it is not padding
        row = {"launch": "sw_windows", "n": n, "C": 1, "size": [H, W], "window": [P, P], "overlap": 0.5, "windows_per_slice":
               len(oy) * len(ox), "equal_to_composition": same, "kernel": k, "torch_composition": c,
               "composition_over_kernel": c["median_ms"] / k["median_ms"], "bytes_to_move": nbytes,
               "kernel_GBs_on_those_bytes": nbytes / (k["median_ms"] * 1e-3) / 1e9}
        rows.append(row)
        print(json.dumps(row), flush=True)
        for name, mask in (("none", 0x01), ("flips", 0x07)):
            T = len(codes(mask))
            for dtype in (torch.float32, torch.bfloat16):
                logits = torch.empty(T, nb, K, P, P, device=dev, dtype=dtype)
                for t in range(T):  # (made view by view: the fp32 stack of the larger shape is 0.7 GB)
                    logits[t] = (torch.randn(nb, K, P, P, generator=g) * 3).to(dev).to(dtype)
                pred, conf = torch.empty(n, H, W, device=dev), torch.empty(n, H, W, device=dev)
                kern.sw_merge_counts(logits, None, w1, w1, oy, ox, pred, conf, None, n, K, P, P, H, W, mask)
                want_pred, want_conf = merge_composition(logits, mask, n, oy, ox, wmap, P, H, W)
                differ = int((pred != want_pred).sum())
                conf_err = float((conf - want_conf).abs().max())
                # (the two routes round their sums differently: near-ties may fall either way, as tests/sw_ref.py allows)
                ok = ok and differ <= 5e-3 * pred.numel() and conf_err <= 4e-6
                del want_pred, want_conf
                k, c = timed_pair(lambda: kern.sw_merge_counts(logits, None, w1, w1, oy, ox, pred, conf, None, n, K, P, P, H, W, mask),
                                  lambda: merge_composition(logits, mask, n, oy, ox, wmap, P, H, W), 2, a.repeats, a.inner)
                # every logit once (a window's padding, which is never read, included: an upper bound), pred and conf out
                nbytes = logits.numel() * logits.element_size() + 2 * pred.numel() * 4
                row = {"launch": "sw_merge_counts", "n": n, "K": K, "size": [H, W], "window": [P, P], "overlap": 0.5,
                       "windows_per_slice": len(oy) * len(ox), "tta": name, "T": T,
                       "logits": "bf16" if dtype is torch.bfloat16 else "fp32", "voxels_differing_from_composition": differ,
                       "voxels": pred.numel(), "max_conf_difference": conf_err, "kernel": k, "torch_composition": c,
                       "composition_over_kernel": c["median_ms"] / k["median_ms"], "bytes_to_move": nbytes,
                       "kernel_GBs_on_those_bytes": nbytes / (k["median_ms"] * 1e-3) / 1e9}
                rows.append(row)
                print(json.dumps(row), flush=True)
                del logits
    res = {"tool": "tools/sw_bench.py", "device": torch.cuda.get_device_name(0), "kernel_src_sha16": build.source_sha16(),
           "hbm_measured_TBs": HBM_MEASURED_TBS,
           "timing": "device events around back-to-back calls, the two routes alternating in one process; ms per call; median of "
                     "`repeats` samples after warm-up, one box, one session",
           "rows": rows}
    if a.volume:
        res["volume"] = volume_times(dev, a.volume_reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
