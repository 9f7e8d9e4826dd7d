"""The Lovasz-Softmax loss on the device (csrc/lovasz.hip) against the same loss composed from torch ops, launch by launch, and
what it costs the captured training step.

    python tools/lovasz_bench.py --out profiles/lovasz.json [--no-step]

Every GPU step below is a child process of its own under its own time limit; the first that fails ends the run.
(a) `parts`: forward + backward of ops.lovasz_softmax at (B, K, H, W) = (32, 4, 224, 224), (32, 9, 224, 224), (8, 2, 512, 512), fp32
    and bf16 logits: device events around the pair, the stream idle before and after, median of 20 after warm-up.  Beside it the same
    loss composed from torch ops on the device, written from the paper (softmax, abs, torch.sort(stable=True), gather, cumsum,
    autograd), and ops.lovasz_order against torch.sort on the same errors: the sort alone.
(b) `launches`: the device time of every launch of the pair, from torch.profiler's kernel records over 10 calls (a run of its own:
    tracing slows the host), with the bytes each launch has to move when every access misses once and the rate that makes, beside
    the measured HBM copy rate.
(c) `step`: the captured bf16 ACDC step (bench.py's model, B = 32) through cenet_amd.train.train_acdc with loss_type dice,ce and
    dice,ce,lovasz, run alternately in rounds: a device event at every 20th iteration (train_acdc reads the loss back there, so the
    stream is idle), ms per step, the first interval of each run left out.
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
from cenet_amd import build, kern, ops, train  # noqa: E402
from dist_loss_bench import device_timed, pattern  # noqa: E402

HBM_MEASURED_TBS = 6.29  # float4 copy on the MI355X
SHAPES = [(32, 4, 224, 224), (32, 9, 224, 224), (8, 2, 512, 512)]
LIMITS = {"parts": 420, "launches": 300, "step": 540}  # seconds per child process


def case(B, K, H, W, dtype, dev):
    lab = torch.from_numpy(pattern(B, K, H, W, seed=K)).to(dev)
    pat = torch.from_numpy(pattern(B, K, H, W, seed=7 + K)).long()
    x = 6.0 * torch.nn.functional.one_hot(pat, K).permute(0, 3, 1, 2).float() + 0.5 * torch.randn(
        B, K, H, W, generator=torch.Generator().manual_seed(K))
    return x.contiguous().to(dtype).to(dev), lab  # (the sum takes the one-hot's permuted strides: kern takes raw pointers)


def torch_lovasz(x, lab, acc=torch.float32):
    """Berman et al., Alg. 1, classes present in the labels (the bench's labels hold every class: no read-back for the check).
    acc: the type it computes in — fp32 is what a training script would run, and there the increment, a difference of two numbers
    near 1, keeps few digits at this many pixels; float64 is the check of the fused path's result"""
    K = x.shape[1]
    p = torch.softmax(x.to(acc), dim=1)
    total = 0.0
    for c in range(K):
        fg = (lab == c).to(acc).reshape(-1)
        e = (fg - p[:, c].reshape(-1)).abs()
        es, perm = torch.sort(e, descending=True, stable=True)
        fs = fg[perm]
        G = fs.sum()
        jac = 1.0 - (G - fs.cumsum(0)) / (G + (1.0 - fs).cumsum(0))
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        total = total + torch.dot(es, jac)
    return total / K


def counted_bytes(B, K, H, W, esz):
    """bytes per launch kind when every access misses the caches once; S n = B K H W (key, payload) pairs, T tiles a segment"""
    sn, T = B * K * H * W, -(-(B * H * W) // kern.lovasz_tile())
    return {"lv_keys_kernel": sn * esz + B * H * W * 4 + 8 * sn, "lv_hist_kernel": 4 * sn + 4 * K * 256 * T,
            "tile_rowscan_kernel": 8 * K * 256 * T, "lv_scatter_kernel": 16 * sn + 4 * K * 256 * T, "tile_count_kernel": 4 * sn,
            "lv_coef_kernel": 12 * sn, "lv_bwd_kernel": sn * esz * 2 + 4 * sn}


def fwd_bwd_fn(x, lab):
    B, K, H, W = x.shape
    ws = torch.empty(kern.lovasz_ws_bytes(B, K, H, W, False) // 4, dtype=torch.int32, device=x.device)
    coef, loss = torch.empty(x.shape, device=x.device), torch.empty(1, device=x.device)
    dx, gout = torch.empty_like(x), torch.ones(1, device=x.device)

    def fn():
        kern.lovasz_fwd(x, lab, ws, coef, loss, B, K, H, W, False, False, None, False)
        kern.lovasz_bwd(x, coef, gout, dx, B, K, H, W, False)
    return fn, loss, dx


def parts(dev, repeats):
    rows = []
    for B, K, H, W in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            x, lab = case(B, K, H, W, dtype, dev)
            fn, loss, dx = fwd_bwd_fn(x, lab)

            def composed(acc=torch.float32):
                xr = x.detach().requires_grad_(True)
                torch_lovasz(xr, lab, acc).backward()
                return xr.grad

            t = {"fwd_bwd": device_timed(fn, 3, repeats), "torch_composition_fwd_bwd": device_timed(composed, 3, repeats)}
            ref, ref64 = torch_lovasz(x, lab), torch_lovasz(x, lab, torch.float64)
            gref, gref64 = composed().float(), composed(torch.float64).float()
            row = {"shape": [B, K, H, W], "logits": str(dtype).replace("torch.", ""), "device": t,
                   "speedup_median": t["torch_composition_fwd_bwd"]["median_ms"] / t["fwd_bwd"]["median_ms"],
                   "loss": loss.item(), "torch_composition_loss": ref.item(),
                   "torch_composition_float64_loss": ref64.item(),
                   "grad_rel_l2_to_torch_composition_float64": (torch.linalg.norm(dx.float() - gref64) / torch.linalg.norm(gref64)).item(),
                   "torch_composition_fp32_grad_rel_l2_to_float64": (torch.linalg.norm(gref - gref64) / torch.linalg.norm(gref64)).item(),
                   "workspace_MB": kern.lovasz_ws_bytes(B, K, H, W, False) / 1e6}
            if dtype == torch.float32:  # the sort alone, on the errors of this case
                p = torch.softmax(x, dim=1)
                e = torch.stack([((lab == c).float() - p[:, c]).abs().reshape(-1) for c in range(K)])
                ts = {"lovasz_order": device_timed(lambda: ops.lovasz_order(e), 3, repeats),
                      "torch_sort_stable": device_timed(lambda: torch.sort(e, dim=1, descending=True, stable=True), 3, repeats)}
                row["sort_alone"] = ts
                row["sort_equal_to_torch"] = bool(torch.equal(ops.lovasz_order(e).long(),
                                                              torch.sort(e, dim=1, descending=True, stable=True).indices))
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
                kind = next((k for k in nbytes if k in ev.key), None) or ("lv_finalize_kernel" if "lv_finalize" in ev.key else None)
                if kind is None or not us:
                    continue
                d = per.setdefault(kind, {"us_per_call": 0.0, "launches_per_call": 0.0})
                d["us_per_call"] += us / calls
                d["launches_per_call"] += ev.count / calls
            for kind, d in per.items():
                if kind in nbytes:
                    d["counted_bytes_per_launch"] = nbytes[kind]
                    # (the row scan: the bytes of the four digit-count scans over the time of all five — the fifth, of the g counts,
                    # moves a 256th of them —, so its rate reads slightly low)
                    n_big = d["launches_per_call"] - 1 if kind == "tile_rowscan_kernel" else d["launches_per_call"]
                    d["TBs_on_counted_bytes"] = nbytes[kind] * n_big / (d["us_per_call"] * 1e-6) / 1e12
            row = {"shape": [B, K, H, W], "logits": str(dtype).replace("torch.", ""), "per_launch_kind": per,
                   "sum_us_per_call": sum(d["us_per_call"] for d in per.values()),
                   "note": "tile_rowscan_kernel: bytes of the digit-count scans over the time of all scans, the g-count scan included"}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if not all(r["per_launch_kind"] for r in rows):
        raise SystemExit("lovasz_bench: the profiler recorded no kernel of csrc/lovasz.hip")
    return rows


def step_times(dev, rounds, intervals):
    """ms per captured step, per loss_type (tools/dist_loss_bench.py's method)"""
    cfg = bench.CONFIGS["acdc"]
    B, S, K = cfg["batch"], cfg["size"], cfg["classes"]
    g = torch.Generator().manual_seed(3)
    batch = {"image": torch.randn(B, cfg["in_ch"], S, S, generator=g).to(dev),
             "label": torch.from_numpy(pattern(B, K, S, S, seed=11)).to(dev)}
    loader = [batch] * (20 * (intervals + 1))
    configs = {"dice,ce": "0.5,0.5", "dice,ce,lovasz": "0.5,0.5,0.5"}
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
            raise SystemExit("lovasz_bench: no GPU (the device path has no fallback and a CPU timing says nothing)")
        dev = torch.device("cuda:0")
        res = {"parts": lambda: parts(dev, a.repeats), "launches": lambda: launches(dev),
               "step": lambda: step_times(dev, a.rounds, a.intervals)}[a.part]()
        print("DEVICE " + torch.cuda.get_device_name(0))
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    # (this process starts the parts and never opens the GPU itself)
    res = {"tool": "tools/lovasz_bench.py", "device": None, "kernel_src_sha16": build.source_sha16(),
           "hbm_measured_TBs": HBM_MEASURED_TBS, "tile": kern.lovasz_tile(),
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
            raise SystemExit(f"lovasz_bench: part {part} ended with status {p.returncode}; nothing further is run")
        res["device"] = next(l for l in p.stdout.splitlines() if l.startswith("DEVICE "))[7:]
        res[names[part]] = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
