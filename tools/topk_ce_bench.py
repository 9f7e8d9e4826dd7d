"""The top-k cross-entropy on the device (csrc/topk_ce.hip) against the same loss composed from torch ops, launch by launch, and
what it costs the captured training step.

    python tools/topk_ce_bench.py --out profiles/topk_ce.json [--no-step]

Every GPU step below is a child process of its own under its own time limit; the first that fails ends the run.
(a) `parts`: forward + backward of ops.topk_ce's two kern calls at (B, K, H, W) = (32, 4, 224, 224) and (32, 9, 224, 224), fp32 and
    bf16 logits, k = 10: device events around the pair, the stream idle before and after, median of 20 after warm-up.  Beside it
    the torch composition of the same result, timed in the same run: F.cross_entropy(reduction="none"), torch.topk(., m,
    sorted=False), mean, autograd backward.
(b) `launches`: the device time of every launch of the pair, from torch.profiler's kernel records over 10 calls (a run of its own:
    tracing slows the host), with the bytes each launch has to move when every access misses once and the rate that makes, beside
    the measured HBM copy rate.
(c) `step`: the captured bf16 ACDC step (bench.py's model, B = 32) through cenet_amd.train.train_acdc with loss_type dice,ce (the
    step as it was before this loss existed: that path calls nothing of it) and dice,ce,topk, run alternately in rounds: a device
    event at every 20th iteration (train_acdc reads the loss back there, so the stream is idle), ms per step, the first interval
    of each run left out.
Needs the MI355X: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from cenet_amd import build, kern, train  # noqa: E402
from dist_loss_bench import device_timed, pattern  # noqa: E402
from lovasz_bench import HBM_MEASURED_TBS, case  # noqa: E402

SHAPES = [(32, 4, 224, 224), (32, 9, 224, 224)]
PERCENT = 10.0
LIMITS = {"parts": 300, "launches": 240, "step": 540}  # seconds per child process


def kept_count(n, k=PERCENT):
    return max(1, int(float(n) * float(np.float32(k)) / 100.0))


def torch_topk_ce(x, lab, m, acc=torch.float32):
    """acc: the type it computes in — fp32 is what a training script would run, float64 the check of the device path's result"""
    ce = torch.nn.functional.cross_entropy(x.to(acc), lab.long(), reduction="none").reshape(-1)
    return torch.topk(ce, m, sorted=False).values.mean()


def counted_bytes(B, K, H, W, esz, k=PERCENT):
    """bytes per launch kind when every access misses the caches once; the backward reads logits and labels of the kept pixels only"""
    px = B * H * W
    return {"tk_keys_kernel": px * K * esz + 8 * px, "tk_hist_kernel": 4 * px, "tile_count_kernel": 4 * px,
            "tk_weights_kernel": 8 * px, "tk_bwd_kernel": 4 * px + px * K * esz + int(k / 100 * (px * K * esz + 4 * px))}


SMALL = ("tk_pick_kernel", "tile_rowscan_kernel", "tk_finalize_kernel", "zero")


def fwd_bwd_fn(x, lab):
    B, K, H, W = x.shape
    ws = torch.empty(kern.topk_ce_ws_bytes(B, H, W, False) // 4, dtype=torch.int32, device=x.device)
    wgt, loss = torch.empty(B, H, W, device=x.device), torch.empty(1, device=x.device)
    dx, gout = torch.empty_like(x), torch.ones(1, device=x.device)
    kp = torch.tensor([PERCENT], device=x.device)

    def fn():
        kern.topk_ce_fwd(x, lab, kp, ws, wgt, loss, B, K, H, W, False, None)
        kern.topk_ce_bwd(x, lab, wgt, gout, dx, B, K, H, W, None)
    return fn, loss, dx, wgt


def parts(dev, repeats):
    rows = []
    for B, K, H, W in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            x, lab = case(B, K, H, W, dtype, dev)
            fn, loss, dx, wgt = fwd_bwd_fn(x, lab)
            m = kept_count(B * H * W)

            def composed(acc=torch.float32):
                xr = x.detach().requires_grad_(True)
                torch_topk_ce(xr, lab, m, acc).backward()
                return xr.grad

            t = {"fwd_bwd": device_timed(fn, 3, repeats), "torch_composition_fwd_bwd": device_timed(composed, 3, repeats)}
            ref64 = torch_topk_ce(x, lab, m, torch.float64)
            gref64 = composed(torch.float64).float()
            row = {"shape": [B, K, H, W], "logits": str(dtype).replace("torch.", ""), "percent": PERCENT, "kept": m, "device": t,
                   "speedup_median": t["torch_composition_fwd_bwd"]["median_ms"] / t["fwd_bwd"]["median_ms"],
                   "loss": loss.item(), "torch_composition_loss": torch_topk_ce(x, lab, m).item(),
                   "torch_composition_float64_loss": ref64.item(), "kept_on_device": int((wgt != 0).sum().item()),
                   "grad_rel_l2_to_torch_composition_float64": (torch.linalg.norm(dx.float() - gref64) / torch.linalg.norm(gref64)).item(),
                   "workspace_MB": kern.topk_ce_ws_bytes(B, H, W, False) / 1e6}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def launches(dev, calls=10):
    from torch.profiler import ProfilerActivity, profile
    rows = []
    for B, K, H, W in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            x, lab = case(B, K, H, W, dtype, dev)
            fn = fwd_bwd_fn(x, lab)[0]
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
            nbytes = counted_bytes(B, K, H, W, x.element_size())
            per = {}
            for ev in prof.key_averages():
                us = getattr(ev, "self_device_time_total", 0) or getattr(ev, "self_cuda_time_total", 0)
                kind = next((k for k in list(nbytes) + list(SMALL) if k in ev.key), None)
                if kind is None or not us:
                    continue
                d = per.setdefault(kind, {"us_per_call": 0.0, "launches_per_call": 0.0})
                d["us_per_call"] += us / calls
                d["launches_per_call"] += ev.count / calls
            for kind, d in per.items():
                if kind in nbytes:
                    d["counted_bytes_per_launch"] = nbytes[kind]
                    d["TBs_on_counted_bytes"] = nbytes[kind] * d["launches_per_call"] / (d["us_per_call"] * 1e-6) / 1e12
            total_us = sum(d["us_per_call"] for d in per.values())
            total_bytes = sum(nbytes[k] * per[k]["launches_per_call"] for k in nbytes if k in per)
            row = {"shape": [B, K, H, W], "logits": str(dtype).replace("torch.", ""), "per_launch_kind": per,
                   "sum_us_per_call": total_us, "counted_bytes_per_call": total_bytes,
                   "TBs_on_counted_bytes": total_bytes / (total_us * 1e-6) / 1e12,
                   "largest_launch_kind": max(per, key=lambda k: per[k]["us_per_call"]),
                   "note": "zero: the fill launch in front of the forward (every launch whose name holds `zero`)"}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if not all(any(k.startswith("tk_") for k in r["per_launch_kind"]) for r in rows):
        raise SystemExit("topk_ce_bench: the profiler recorded no kernel of csrc/topk_ce.hip")
    return rows


def step_times(dev, rounds, intervals):
    """ms per captured step, per loss_type (tools/dist_loss_bench.py's method)"""
    cfg = bench.CONFIGS["acdc"]
    B, S, K = cfg["batch"], cfg["size"], cfg["classes"]
    g = torch.Generator().manual_seed(3)
    batch = {"image": torch.randn(B, cfg["in_ch"], S, S, generator=g).to(dev),
             "label": torch.from_numpy(pattern(B, K, S, S, seed=11)).to(dev)}
    loader = [batch] * (20 * (intervals + 1))
    configs = {"dice,ce": "0.5,0.5", "dice,ce,topk": "0.5,0.5,0.5"}
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
    for name in out:
        out[name]["added_ms"] = out[name]["median_ms"] - out["dice,ce"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--intervals", type=int, default=5, help="timed intervals of 20 steps per run of (c)")
    ap.add_argument("--no-step", action="store_true", help="leave (c), the captured training step, out")
    ap.add_argument("--part", choices=list(LIMITS), default=None, help="(internal) run one part in this process, print its JSON")
    a = ap.parse_args()
    if a.part:
        if not torch.cuda.is_available():
            raise SystemExit("topk_ce_bench: no GPU (the device path has no fallback and a CPU timing says nothing)")
        dev = torch.device("cuda:0")
        res = {"parts": lambda: parts(dev, a.repeats), "launches": lambda: launches(dev),
               "step": lambda: step_times(dev, a.rounds, a.intervals)}[a.part]()
        print("DEVICE " + torch.cuda.get_device_name(0))
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    # (this process starts the parts and never opens the GPU itself)
    res = {"tool": "tools/topk_ce_bench.py", "device": None, "kernel_src_sha16": build.source_sha16(),
           "hbm_measured_TBs": HBM_MEASURED_TBS, "tile": kern.topk_tile(), "percent": PERCENT,
           "timing": "(a) device events around forward + backward, stream idle before and after, median of 20; (b) torch.profiler "
                     "kernel records over 10 calls, a run of its own; (c) device events every 20 replayed steps of train_acdc"}
    names = {"parts": "parts", "launches": "launches", "step": "captured_acdc_step_bf16"}
    for part in LIMITS:
        if part == "step" and a.no_step:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--repeats", str(a.repeats), "--rounds", str(a.rounds),
               "--intervals", str(a.intervals)]
        p = subprocess.run(cmd, timeout=LIMITS[part], stdout=subprocess.PIPE, text=True)  # a fresh child; its stderr passes through
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            raise SystemExit(f"topk_ce_bench: part {part} ended with status {p.returncode}; nothing further is run")
        res["device"] = next(l for l in p.stdout.splitlines() if l.startswith("DEVICE "))[7:]
        res[names[part]] = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
