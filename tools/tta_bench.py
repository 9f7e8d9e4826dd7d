"""Test-time augmentation: the two launches of csrc/tta.hip (kern.tta_views, kern.tta_argmax_resize_counts) against the torch
composition of the same result on the device — torch.flip / transpose per view, softmax, the sum over the views, argmax, then an
index gather for the order-0 resize.  The composition is the yardstick; the kernels are never one for themselves.

    python tools/tta_bench.py --out profiles/tta_infer.json

Shapes: n = 32, K = 4, 224 -> 224 (an ACDC chunk) and n = 8, K = 9, 224 -> 512 (a Synapse chunk); T = 3 ("flips") and 8 ("d4");
logits in fp32 and bf16.  The two routes run alternately in one process; a sample is a device-event time around `--inner`
back-to-back calls, divided by their number; the median of the samples is reported with their minimum and maximum.  The two
routes' class maps are compared before anything is timed.  Beside every time: the bytes the launch must move when every element is
touched once, and the rate that makes, next to the copy rate the project quotes.  Needs the MI355X: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cenet_amd import kern  # noqa: E402

HBM_MEASURED_TBS = 6.29  # float4 copy on the MI355X


def codes(mask):
    return [g for g in range(8) if mask >> g & 1]


def torch_view(x, g):
    if g & 4:
        x = x.transpose(-1, -2)
    if g & 2:
        x = torch.flip(x, (-2,))
    if g & 1:
        x = torch.flip(x, (-1,))
    return x


def torch_unview(v, g):
    if g & 1:
        v = torch.flip(v, (-1,))
    if g & 2:
        v = torch.flip(v, (-2,))
    if g & 4:
        v = v.transpose(-1, -2)
    return v


def views_composition(x, mask):
    return torch.stack([torch_view(x, g) for g in codes(mask)]).contiguous()


def zoom0_index(P, S, dev):
    """source index and inside flag of scipy's order-0 zoom from P to S samples (the rule of csrc/volresize.hip, in float64)"""
    c = torch.arange(S, dtype=torch.float64, device=dev) * ((P - 1) / (S - 1))
    inside = ~(c > P - 1)
    return torch.floor(c + 0.5).long().clamp_(0, P - 1), inside


def merge_composition(logits, mask, sy, sx, inside):
    prob = None
    for t, g in enumerate(codes(mask)):
        p = torch.softmax(torch_unview(logits[t].float(), g), dim=1)
        prob = p if prob is None else prob + p
    top, am = prob.max(dim=1)
    am, top = am[:, sy][:, :, sx].float(), top[:, sy][:, :, sx] * (1.0 / len(codes(mask)))
    return am * inside, top * inside


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tta_bench: no GPU (the kernels have no fallback and a CPU timing says nothing)")
    dev = torch.device("cuda:0")
    rows, ok = [], True
    for n, K, P, S in ((32, 4, 224, 224), (8, 9, 224, 512)):
        sy, inside_y = zoom0_index(P, S, dev)
        sx, inside_x = zoom0_index(P, S, dev)
        inside = (inside_y[:, None] & inside_x[None, :]).float()
        for name, mask in (("flips", 0x07), ("d4", 0xFF)):
            T = len(codes(mask))
            g = torch.Generator(device="cpu").manual_seed(n * 100 + T)
            x = torch.randn(n, 1, P, P, generator=g).to(dev)
            out = torch.empty(T, n, 1, P, P, device=dev)
            kern.tta_views(x, out, n, 1, P, P, mask)
            same = bool(torch.equal(out, views_composition(x, mask)))
            ok = ok and same
            k, c = timed_pair(lambda: kern.tta_views(x, out, n, 1, P, P, mask), lambda: views_composition(x, mask), 3, a.repeats,
                              a.inner)
            nbytes = (1 + T) * x.numel() * 4
            row = {"launch": "tta_views", "n": n, "C": 1, "patch": [P, P], "tta": name, "T": T, "equal_to_composition": same,
                   "kernel": k, "torch_composition": c, "composition_over_kernel": c["median_ms"] / k["median_ms"],
                   "bytes_to_move": nbytes, "kernel_GBs_on_those_bytes": nbytes / (k["median_ms"] * 1e-3) / 1e9}
            rows.append(row)
            print(json.dumps(row), flush=True)
            for dtype in (torch.float32, torch.bfloat16):
                logits = (torch.randn(T, n, K, P, P, generator=g) * 3).to(dev).to(dtype)
                pred, conf = torch.empty(n, S, S, device=dev), torch.empty(n, S, S, device=dev)
                kern.tta_argmax_resize_counts(logits, None, pred, conf, None, n, K, P, P, S, S, mask)
                want_pred, want_conf = merge_composition(logits, mask, sy, sx, inside)
                differ = int((pred != want_pred).sum())
                conf_err = float((conf - want_conf).abs().max())
                # (the two routes round their softmax differently: near-ties may fall either way, as tests/test_tta.py allows)
                ok = ok and differ <= 1e-3 * pred.numel() and conf_err <= 2e-6
                k, c = timed_pair(lambda: kern.tta_argmax_resize_counts(logits, None, pred, conf, None, n, K, P, P, S, S, mask),
                                  lambda: merge_composition(logits, mask, sy, sx, inside), 3, a.repeats, a.inner)
                # every logit the zoom reaches once (all of them when the volume is at least as fine as the patch), pred and conf out
                nbytes = logits.numel() * logits.element_size() + 2 * pred.numel() * 4
                comp_written = T * n * K * P * P * 4
                row = {"launch": "tta_argmax_resize_counts", "n": n, "K": K, "patch": [P, P], "size": [S, S], "tta": name, "T": T,
                       "logits": "bf16" if dtype is torch.bfloat16 else "fp32", "voxels_differing_from_composition": differ,
                       "voxels": pred.numel(), "max_conf_difference": conf_err, "kernel": k, "torch_composition": c,
                       "composition_over_kernel": c["median_ms"] / k["median_ms"], "bytes_to_move": nbytes,
                       "kernel_GBs_on_those_bytes": nbytes / (k["median_ms"] * 1e-3) / 1e9,
                       "probability_bytes_the_composition_writes": comp_written}
                rows.append(row)
                print(json.dumps(row), flush=True)
    res = {"tool": "tools/tta_bench.py", "device": torch.cuda.get_device_name(0), "hbm_measured_TBs": HBM_MEASURED_TBS,
           "timing": "device events around back-to-back calls, the two routes alternating in one process; ms per call",
           "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
