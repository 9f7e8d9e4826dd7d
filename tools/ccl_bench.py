"""Keep-largest-component post-processing: the device path (evaluate.keep_largest_component, csrc/ccl.hip) against the host route
it replaces — download the prediction, scipy.ndimage.label per class, bincount, upload the filtered volume.

    python tools/ccl_bench.py --out profiles/ccl.json [--small]

Volumes: 10 x 256 x 216 (an ACDC case) and 148 x 512 x 512 (a Synapse case); smooth blobs per class plus 1 % salt voxels of a random
class; K = 4 and 9, connectivity 1 and 3.  Every timing is a host clock around work that ends in a device synchronise, after
warm-up; the median of the repeats is reported with their minimum and maximum.  The two routes' results are compared voxel for
voxel before anything is timed.  Needs the MI355X: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import ndimage
from scipy.ndimage import zoom

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cenet_amd import evaluate  # noqa: E402

HBM_MEASURED_TBS = 6.29  # float4 copy on the MI355X
# bytes per voxel the launches have to move when every access misses the caches once: init (label in, parent out) 8, link (label,
# parent) 8, flatten (in, out) 8, sizes (zero, roots in) 8, two selection passes (roots) 8, filter (label, roots in, out) 12;
# the sizes of roots and the neighbours' labels come on top where they miss
COUNTED_BYTES_PER_VOXEL = 52


def blobs(shape, seed, thresh=0.55):
    rng = np.random.default_rng(seed)
    low = rng.random(tuple(max(2, s // 4) for s in shape))
    return zoom(low, [s / l for s, l in zip(shape, low.shape)], order=1) > thresh


def volume(shape, K, seed):
    vol = np.zeros(shape, np.float32)
    for c in range(1, K):
        vol[blobs(shape, seed + c)] = c
    rng = np.random.default_rng(seed)
    salt = rng.random(shape) < 0.01
    vol[salt] = rng.integers(1, K, int(salt.sum()))
    return vol


def host_route(pred_d, K, conn):
    vol = pred_d.cpu().numpy()
    st = ndimage.generate_binary_structure(3, conn)
    out = np.zeros_like(vol)
    for c in range(1, K):
        lab, nl = ndimage.label(vol == c, st)
        if nl:
            out[lab == np.argmax(np.bincount(lab.ravel())[1:]) + 1] = c
    return torch.from_numpy(out).to(pred_d.device)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="the 10 x 256 x 216 volume only")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ccl_bench: no GPU (the device path has no fallback and a CPU timing says nothing)")
    dev = torch.device("cuda:0")
    rows = []
    for shape in [(10, 256, 216)] + ([] if a.small else [(148, 512, 512)]):
        for K in (4, 9):
            pred = torch.from_numpy(volume(shape, K, seed=K)).to(dev)
            n = pred.numel()
            for conn in (1, 3):
                filt, table = evaluate.keep_largest_component(pred, K, conn)
                same = bool(torch.equal(filt, host_route(pred, K, conn)))
                d = timed(lambda: evaluate.keep_largest_component(pred, K, conn), 3, a.repeats)
                h = timed(lambda: host_route(pred, K, conn), 1, a.host_repeats)
                at_peak = d["median_ms"] * 1e-3 * HBM_MEASURED_TBS * 1e12 / n
                row = {"shape": list(shape), "K": K, "connectivity": conn, "voxels": n, "components": int(table[:, 0].sum()),
                       "voxels_removed": int(table[:, 2].sum()), "equal_to_host_route": same, "device": d, "host_route": h,
                       "speedup_median": h["median_ms"] / d["median_ms"],
                       "counted_bytes_per_voxel": COUNTED_BYTES_PER_VOXEL,
                       "effective_GBs_on_counted_bytes": COUNTED_BYTES_PER_VOXEL * n / (d["median_ms"] * 1e-3) / 1e9,
                       "bytes_per_voxel_hbm_could_move_in_that_time": at_peak}
                rows.append(row)
                print(json.dumps(row), flush=True)
    res = {"tool": "tools/ccl_bench.py", "device": torch.cuda.get_device_name(0), "hbm_measured_TBs": HBM_MEASURED_TBS,
           "timing": "host clock around calls ending in a device synchronise; device time includes the table download", "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if all(r["equal_to_host_route"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
