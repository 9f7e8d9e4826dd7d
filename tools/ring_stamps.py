"""Where a K-step of the LDS-DMA ring GEMM spends its cycles: runs four shapes of the training step on the DIAGNOSTIC build of
the library (in-kernel clock reads, csrc/gemm_ring.h RingClock) and prints the median cycles per loop trip and segment over the
stamped workgroups; on the product library (no stamps) it prints the launch times only.

    python -m cenet_amd.build --stamps                      # -> cenet_amd/libcenet_hip_stamps.so
    python -m cenet_amd.build --stamps-tr-builtin           # -> ..._stamps_trb.so: row-fast fragments read through the builtin
    python tools/ring_stamps.py --lib cenet_amd/libcenet_hip_stamps.so
    python tools/ring_stamps.py                             # product library: times only

Segments of one trip, in the order they run (ring kernel): wait = counted s_waitcnt vmcnt; barrier = s_barrier; issue = the
refill's LDS-DMA pieces; reads = fragment reads until lgkmcnt(0); mfma = MFMA issue.  The streaming kernel's trip is one output tile:
barrier, issue of the next tile, reads + mfma per 32 k, wait for the next tile, rest = the epilogue.  Every lap contains one
clock read (`stamp`, subtracted below).  The stamped build's fences forbid overlaps the product kernel has: read the SHARES
of a trip here and the launch time on the product library.  `first` is the first trip of a workgroup (the prologue's latency)."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="library to load instead of cenet_amd/libcenet_hip.so")
ap.add_argument("--wgs", type=int, default=64, help="workgroups stamped per launch")
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

import torch  # noqa: E402

from cenet_amd import _lib, kern  # noqa: E402

if args.lib:
    _lib._LIB = ctypes.CDLL(os.path.abspath(args.lib))
L = _lib.lib()
stamped = hasattr(L, "cenet_ring_stamps")
dev = torch.device("cuda:0")
BF = torch.bfloat16
SEG = ["wait", "barrier", "issue", "reads", "mfma", "rest"]
LAPS = [1, 1, 1, 2, 2, 0]  # clock reads per trip and segment of the ring kernel


def shapes():
    g = torch.Generator().manual_seed(0)

    def rnd(*s):
        return (torch.randn(*s, generator=g) * 0.25).to(BF).to(dev)

    out = []
    for M, N, K in ((6272, 320, 1280), (1568, 512, 2048)):  # tokens x weights: A [M, K] k-fast, B [K, N] row-fast, C row-major
        a, b, c = rnd(M, K), rnd(K, N), torch.empty(M, N, dtype=BF, device=dev)
        out.append((f"M{M} N{N} K{K}", kern.mat_plain(a, K, 1, kfast=1), kern.mat_plain(b, N, 1, kfast=0), c, M, N, K,
                    dict(scr=N, scc=1), (a, b)))
    M, N, K, nb = 320, 196, 320, 32  # per-image 1x1 convolution: shared weights [M, K], planes [K, N] with an unaligned pitch
    a, b, c = rnd(M, K), rnd(nb, K, N), torch.empty(nb, M, N, dtype=BF, device=dev)
    out.append((f"M{M} N{N} K{K} batch{nb}", kern.mat_plain(a, K, 1, kfast=1), kern.mat_plain(b, N, 1, sb=K * N, kfast=0), c, M, N, K,
                dict(scr=N, scc=1, scb=M * N, nbatch=nb), (a, b)))
    M, N, K = 100352, 64, 64  # a stream shape
    a, b, c = rnd(M, K), rnd(K, N), torch.empty(M, N, dtype=BF, device=dev)
    out.append((f"M{M} N{N} K{K}", kern.mat_plain(a, K, 1, kfast=1), kern.mat_plain(b, N, 1, kfast=0), c, M, N, K,
                dict(scr=N, scc=1), (a, b)))
    return out


def launch_us(A, B, C, M, N, K, kw):
    for _ in range(3):
        kern.gemm(A, B, C, M, N, K, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        kern.gemm(A, B, C, M, N, K, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps * 1e3


print(f"library: {args.lib or _lib.LIB_PATH} ({'stamped' if stamped else 'product'} build)")
for name, A, B, C, M, N, K, kw, keep in shapes():
    us = launch_us(A, B, C, M, N, K, kw)
    kernel = kern.last_gemm_kernel()
    print(f"\n{name}: {kernel}  {us:.1f} us per launch" + (" (stamped build: not the product's time)" if stamped else ""))
    if not stamped:
        continue
    buf = torch.zeros(args.wgs * 16, dtype=torch.int64, device=dev)
    L.cenet_ring_stamps.argtypes, L.cenet_ring_stamps.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
    assert L.cenet_ring_stamps(buf.data_ptr(), args.wgs) == 0
    kern.gemm(A, B, C, M, N, K, **kw)
    torch.cuda.synchronize()
    assert L.cenet_ring_stamps(None, 0) == 0
    rec = [r for r in buf.cpu().view(-1, 16).tolist() if r[12] > 0]
    if not rec:
        print("  no stamped workgroup ran a trip")
        continue
    stream = kernel.startswith("gemm_ring_stream")
    laps = [1, 1, 1, 2 * (K // 64), 2 * (K // 64), 1] if stream else LAPS
    cal = statistics.median(r[14] for r in rec)
    trips = statistics.median(r[12] for r in rec)
    print(f"  {len(rec)} workgroups stamped, {trips:.0f} trips each (median); one clock read = {cal:.0f} cycles")
    print(f"  {'':14s}" + "".join(f"{s:>9s}" for s in SEG) + f"{'trip':>9s}")
    for label, steady in (("steady trip", True), ("first trip", False)):
        row, tot = [], 0.0
        for i in range(6):
            if steady:
                v = statistics.median((r[i] - r[6 + i]) / max(r[12] - 1, 1) for r in rec) if trips > 1 else float("nan")
            else:
                v = statistics.median(r[6 + i] for r in rec)
            v -= laps[i] * cal
            row.append(v)
            tot += v
        print(f"  {label:14s}" + "".join(f"{v:9.0f}" for v in row) + f"{tot:9.0f}")
    loop = statistics.median(r[13] / r[12] for r in rec)
    print(f"  loop cycles per trip with the stamps in: {loop:.0f} (= {loop / 2.4e3:.2f} us at 2.4 GHz)")
