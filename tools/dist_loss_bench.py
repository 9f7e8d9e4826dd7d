"""The distance-map losses on the device (csrc/edt.hip cenet_dist_maps_*, csrc/dist_loss.hip) against the host route they replace,
and what they cost the captured training step.

    python tools/dist_loss_bench.py --out profiles/dist_loss.json [--no-step]

(a) ops.distance_maps, ops.pred_distance_maps and the loss forward + backward on ready maps, each on its own, at (B, K, H, W) =
    (32, 4, 224, 224), (32, 9, 224, 224), (32, 2, 512, 512), fp32 and bf16 logits: device events around each call, the stream idle
    before and after, median of 20 after warm-up.  With the bytes the launches have to move when every access misses once, and the
    rate that makes, beside the measured HBM copy rate.
(b) the host route: download, scipy.ndimage.distance_transform_edt per (image, class) plane — twice, for the mask and for its
    complement — upload; host clock, median of 3.
(c) the captured bf16 ACDC step (bench.py's model, B = 32) through cenet_amd.train.train_acdc with loss_type dice,ce /
    dice,ce,surface / dice,ce,surface,hausdorff, run alternately in rounds: a device event at every 20th iteration (train_acdc
    reads the loss back there, so the stream is idle), the intervals in ms per step, the first of each run left out; the median
    over all rounds and the spread of the per-round medians.
Needs the MI355X: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.ndimage import distance_transform_edt, zoom

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from cenet_amd import build, kern, ops, train  # noqa: E402

HBM_MEASURED_TBS = 6.29  # float4 copy on the MI355X
SHAPES = [(32, 4, 224, 224), (32, 9, 224, 224), (32, 2, 512, 512)]


def blobs(shape, seed, thresh=0.55):
    rng = np.random.default_rng(seed)
    low = rng.random(tuple(max(2, s // 4) for s in shape))
    return zoom(low, [s / l for s, l in zip(shape, low.shape)], order=1) > thresh


def pattern(B, K, H, W, seed):
    vol = np.zeros((B, H, W), np.float32)
    for c in range(1, K):
        vol[blobs((B, H, W), seed + c)] = c
    return vol


def counted_bytes(B, K, H, W, esz):
    """bytes each part moves when every access misses the caches once (the envelope stack of the y pass comes on top)"""
    n = B * (K - 1) * H * W  # pixels of the output maps; the transform runs on 2 n (every mask and its complement)
    stack = 2 * n * (1 + (1 + 4) + (4 + 4) + (4 + 4)) + (2 * n * 4 + n * 4)  # features out, x sweeps, y pass, the two halves added
    logits, labels = B * K * H * W * esz, B * H * W * 4
    return {"label_maps": labels + stack, "pred_maps": logits + stack,
            "loss_fwd_bwd": 2 * (logits + labels + 8 * n) + logits}


def device_timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "repeats": repeats}


def host_timed(fn, repeats):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "repeats": repeats}


def host_maps(masks_d):
    """bool [B,K-1,H,W] on the device -> int32 maps on the device, by the host"""
    m = masks_d.cpu().numpy()
    out = np.zeros(m.shape, np.int32)
    for b in range(m.shape[0]):
        for c in range(m.shape[1]):
            p = m[b, c]
            if p.any() and not p.all():
                out[b, c] = np.rint(distance_transform_edt(p) ** 2 + distance_transform_edt(~p) ** 2)
    return torch.from_numpy(out).to(masks_d.device)


def parts(dev, repeats, host_repeats):
    rows = []
    for B, K, H, W in SHAPES:
        lab = torch.from_numpy(pattern(B, K, H, W, seed=K)).to(dev)
        pat = torch.from_numpy(pattern(B, K, H, W, seed=7 + K)).long()
        x32 = 6.0 * torch.nn.functional.one_hot(pat, K).permute(0, 3, 1, 2).float() + 0.5 * torch.randn(
            B, K, H, W, generator=torch.Generator().manual_seed(K))
        gmask = torch.stack([lab == c for c in range(1, K)], dim=1)
        w = torch.tensor([0.7, 0.01], device=dev)
        for dtype in (torch.float32, torch.bfloat16):
            x = x32.to(dtype).to(dev)
            pmask = torch.softmax(x.double(), dim=1)[:, 1:] > 0.5
            d2g, d2p = ops.distance_maps(lab, K), ops.pred_distance_maps(x)
            same = bool(torch.equal(d2g, host_maps(gmask))) and bool(torch.equal(d2p, host_maps(pmask)))
            ws, loss, dx = torch.empty(kern.dist_loss_ws_floats(B, K, H, W), device=dev), torch.empty(1, device=dev), torch.empty_like(x)
            gout = torch.ones(1, device=dev)

            def fwd_bwd():
                kern.dist_loss_fwd(x, lab, d2g, d2p, w, ws, loss, B, K, H, W, True, True)
                kern.dist_loss_bwd(x, lab, d2g, d2p, w, gout, dx, B, K, H, W, True, True)

            t = {"label_maps": device_timed(lambda: ops.distance_maps(lab, K), 3, repeats),
                 "pred_maps": device_timed(lambda: ops.pred_distance_maps(x), 3, repeats),
                 "loss_fwd_bwd": device_timed(fwd_bwd, 3, repeats)}
            nbytes = counted_bytes(B, K, H, W, x.element_size())
            row = {"shape": [B, K, H, W], "logits": str(dtype).replace("torch.", ""), "planes": B * (K - 1),
                   "maps_equal_to_host_route": same, "device": t, "counted_bytes": nbytes,
                   "effective_TBs_on_counted_bytes": {k: nbytes[k] / (t[k]["median_ms"] * 1e-3) / 1e12 for k in t}}
            if dtype == torch.float32:  # (the host route does not depend on how the logits are stored)
                row["host_route"] = {"label_maps": host_timed(lambda: host_maps(gmask), host_repeats),
                                     "pred_maps": host_timed(lambda: host_maps(pmask), host_repeats)}
                row["speedup_median"] = {k: row["host_route"][k]["median_ms"] / t[k]["median_ms"] for k in row["host_route"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def step_times(dev, rounds, intervals):
    """ms per captured step, per loss_type: {name: {"median_ms", "round_medians_ms", ...}}"""
    cfg = bench.CONFIGS["acdc"]
    B, S, K = cfg["batch"], cfg["size"], cfg["classes"]
    g = torch.Generator().manual_seed(3)
    batch = {"image": torch.randn(B, cfg["in_ch"], S, S, generator=g).to(dev),
             "label": torch.from_numpy(pattern(B, K, S, S, seed=11)).to(dev)}
    loader = [batch] * (20 * (intervals + 1))
    configs = {"dice,ce": "0.5,0.5", "dice,ce,surface": "0.5,0.5,0.05", "dice,ce,surface,hausdorff": "0.5,0.5,0.05,0.001"}
    per = {name: [] for name in configs}
    old = kern.set_compute_bf16(True)
    try:
        for _ in range(rounds):
            for name, weights in configs.items():
                events = []

                def log(line, events=events):
                    if line.startswith("iteration"):  # (train_acdc has just read the loss back: the stream is idle)
                        e = torch.cuda.Event(enable_timing=True)
                        e.record()
                        events.append(e)
                train.train_acdc(bench.make_model(dev, cfg), loader, num_classes=K, max_epochs=1, base_lr=0.01, device=dev,
                                 graph=True, log_every=20, log=log, loss_type=name, loss_weights=weights)
                torch.cuda.synchronize()
                per[name].append([a.elapsed_time(b) / 20 for a, b in zip(events[:-1], events[1:])])
    finally:
        kern.set_compute_bf16(old)
    out = {}
    for name, runs in per.items():
        allv, meds = [v for r in runs for v in r], [float(np.median(r)) for r in runs]
        out[name] = {"median_ms": float(np.median(allv)), "min_ms": float(min(allv)), "max_ms": float(max(allv)),
                     "intervals_of_20_steps": len(allv), "round_medians_ms": meds, "round_spread_ms": max(meds) - min(meds)}
    base = out["dice,ce"]["median_ms"]
    for name in out:
        out[name]["added_ms"] = out[name]["median_ms"] - base
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--intervals", type=int, default=7, help="timed intervals of 20 steps per run of (c)")
    ap.add_argument("--no-step", action="store_true", help="leave (c), the captured training step, out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dist_loss_bench: no GPU (the device path has no fallback and a CPU timing says nothing)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/dist_loss_bench.py", "device": torch.cuda.get_device_name(0), "kernel_src_sha16": build.source_sha16(),
           "hbm_measured_TBs": HBM_MEASURED_TBS,
           "timing": "(a) device events around one call, stream idle before and after; (b) host clock; (c) device events every "
                     "20 replayed steps of train_acdc, ms per step",
           "parts": parts(dev, a.repeats, a.host_repeats)}
    if not a.no_step:
        res["captured_acdc_step_bf16"] = step_times(dev, a.rounds, a.intervals)
        print(json.dumps(res["captured_acdc_step_bf16"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if all(r["maps_equal_to_host_route"] for r in res["parts"]) else 1


if __name__ == "__main__":
    sys.exit(main())
