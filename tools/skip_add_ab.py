"""skip_mode 'cat' vs 'add' on the benched ACDC step (bf16 mode, B = 32, one hipGraph replay per step as bench.py runs it), both
models built in this process and timed in alternating blocks; plus the hd = 40 pair-kernel instance choice (HDP = 48 against the
HDP = 64 tiles with padding, CENET_DATTN_HD40_HDP64) on the ACDC add-mode 14 x 14 problem, also alternating.  One JSON line each.

    python tools/skip_add_ab.py --batch 32 --steps 20 --rounds 5
"""
import argparse
import collections
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from cenet_amd import kern, losses, ops, optim  # noqa: E402
from cenet_amd.graph import GraphedStep  # noqa: E402
from cenet_amd.networks import CENet  # noqa: E402


def build(mode, B, dev):
    cfg = bench.CONFIGS["acdc"]
    torch.manual_seed(1234)
    net = CENet(input_channels=cfg["in_ch"], num_classes=cfg["classes"], scale_factors=cfg["scales"], diffatt_num_heads=cfg["heads"],
                skip_mode=mode, out_up_block="upcn").to(dev).train()
    arena = optim.ParamArena(net, optim.cenet_segments())
    opt = optim.FusedSGD(arena, lr=0.01, momentum=0.9, weight_decay=1e-4)
    crit = losses.Criterion(cfg["classes"], argparse.Namespace(loss_type="dice,ce", loss_weights="0.5,0.5"))
    x, lab = bench.synthetic(B, dev, 1234)

    def body():
        opt.zero_grad()
        loss = crit(net(x), lab)
        loss.backward()
        opt.step(sync_hyper=False)
        return loss

    # C-ABI launches of one eager step (an attention backward entry launches two kernels: counted as two)
    counts = collections.Counter()
    real = kern._call, kern.gemm, kern.diffattn_heads, kern.attn64, kern.flash_fwd, kern.flash_bwd
    kern._call = lambda name, *a: (counts.update([name]), real[0](name, *a))[1]
    kern.gemm = lambda *a, **k: (counts.update(["gemm"]), real[1](*a, **k))[1]
    kern.diffattn_heads = lambda a, backward=False: (counts.update(["dattn"] * (2 if backward else 1)), real[2](a, backward))[1]
    kern.attn64 = lambda a, backward=False: (counts.update(["attn64"] * (2 if backward else 1)), real[3](a, backward))[1]
    kern.flash_fwd = lambda *a, **k: (counts.update(["flash"]), real[4](*a, **k))[1]
    kern.flash_bwd = lambda *a, **k: (counts.update(["flash"] * 2), real[5](*a, **k))[1]
    try:
        opt.prepare()
        body()
        torch.cuda.synchronize()
    finally:
        kern._call, kern.gemm, kern.diffattn_heads, kern.attn64, kern.flash_fwd, kern.flash_bwd = real
    return (body, opt), sum(counts.values())


def time_block(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def step_ab(B, steps, rounds, dev):
    # both models and optimizers stay alive; the captured step is rebuilt for every timed block, so that ONE hipGraph exists at a
    # time (two captured steps alive in one process ended in an illegal-address fault on the first replay of the older one)
    runs = {m: build(m, B, dev) for m in ("cat", "add")}
    ms = {m: [] for m in runs}
    for _ in range(rounds):
        for m, ((body, opt), _) in runs.items():
            g = GraphedStep(body, optimizer=opt, warmup=2)
            time_block(g, 3)
            ms[m].append(time_block(g, steps))
            del g
            torch.cuda.synchronize()
    for m, (_, launches) in runs.items():
        med = statistics.median(ms[m])
        print(json.dumps({"part": "step", "skip_mode": m, "batch": B, "ms_per_step": round(med, 3),
                          "images_per_s": round(B * 1000.0 / med, 1), "launches_per_step": launches,
                          "blocks_ms": [round(v, 3) for v in ms[m]]}), flush=True)


def hd40_ab(B, reps, rounds, dev):
    """ACDC add mode, 14 x 14 level: C = 320, 4 heads -> hd 40, N = 196"""
    H, hd, N = 4, 40, 196
    E = 2 * H * hd
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, N, E, generator=g).bfloat16().to(dev) for _ in range(3))
    dU = torch.randn(B, 2 * H, N, 2 * hd, generator=g).bfloat16().to(dev)
    U = torch.empty_like(dU)
    lse = torch.empty((B, 2 * H, N), device=dev)
    dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
    ws = torch.empty(kern.diffattn_heads_ws_bytes(B, H, N), dtype=torch.uint8, device=dev)
    a = kern.DiffAttnT()
    a.q, a.k, a.v, a.U, a.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), U.data_ptr(), lse.data_ptr()
    a.dU, a.dq, a.dk, a.dv, a.ws = dU.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr()
    a.B, a.H, a.N, a.hd, a.scale = B, H, N, hd, hd ** -0.5
    res = {}
    for variant in ("48", "64"):
        for part in ("fwd", "bwd"):
            res[(variant, part)] = []
    outs = {}
    for r in range(rounds + 1):
        for variant in ("48", "64"):
            os.environ["CENET_DATTN_HD40_HDP64"] = "1" if variant == "64" else "0"
            for part in ("fwd", "bwd"):
                t = time_block(lambda: kern.diffattn_heads(a, backward=part == "bwd"), reps)
                if r:  # round 0 warms up
                    res[(variant, part)].append(t * 1000.0)
            outs[variant] = (U.float().clone(), dq.float().clone())
    os.environ.pop("CENET_DATTN_HD40_HDP64", None)
    same = all(torch.equal(x, y) for x, y in zip(outs["48"], outs["64"]))
    for variant in ("48", "64"):
        print(json.dumps({"part": "hd40", "HDP": int(variant), "B": B, "N": N, "heads": H,
                          "fwd_us": round(statistics.median(res[(variant, "fwd")]), 1),
                          "bwd_us": round(statistics.median(res[(variant, "bwd")]), 1), "same_outputs": same}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--part", choices=["all", "step", "hd40"], default="all")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    old = kern.set_compute_bf16(True)
    ops.set_wgrad_overlap(False)  # (bench.py captures its step with the weight gradients on the main stream)
    try:
        if a.part in ("all", "hd40"):
            hd40_ab(a.batch, 50, a.rounds, dev)
        if a.part in ("all", "step"):
            step_ab(a.batch, a.steps, a.rounds, dev)
    finally:
        kern.set_compute_bf16(old)


if __name__ == "__main__":
    main()
