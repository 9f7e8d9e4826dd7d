"""Training throughput of the benched ACDC step (bf16 mode, one hipGraph replay per step, as bench.py runs it on one GPU) with
the fused SGD or the fused AdamW optimizer, on the same synthetic batch.  Prints one JSON line per optimizer.

    python tools/adam_step.py --batch 32 --steps 20
    rocprofv3 --kernel-trace --stats -d <dir> -o adam -- python tools/adam_step.py --optim adamw --steps 5
(the second form gives `adam_kernel`'s time per launch next to `sgd_kernel`'s from a run with --optim sgd)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from cenet_amd import kern, losses, ops, optim  # noqa: E402
from cenet_amd.graph import GraphedStep  # noqa: E402


def run(name, B, steps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = bench.make_model(dev)
    arena = optim.ParamArena(net, optim.cenet_segments())
    args = argparse.Namespace(optimizer=name, base_lr=0.01 if name == "sgd" else 1e-3, weight_decay=1e-4, scheduler="cosine")
    opt = optim.get_optimizer(net, args)
    sched = optim.get_scheduler(opt, args, 100000)
    crit = losses.Criterion(4, argparse.Namespace(loss_type="dice,ce", loss_weights="0.5,0.5"))
    x, lab = bench.synthetic(B, dev, seed=1234)

    def body():
        opt.zero_grad()
        loss = crit(net(x), lab)
        loss.backward()
        opt.step(sync_hyper=False)
        return loss

    g = GraphedStep(body, optimizer=opt, warmup=2)
    for _ in range(warmup):
        g()
        sched.step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        loss = g()
        sched.step()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    out = {"optimizer": name, "batch": B, "steps": steps, "ms_per_step": round(ms, 3), "images_per_s": round(B * 1000.0 / ms, 1),
           "loss": float(loss.detach()), "params": arena.numel, "finite": bool(torch.isfinite(arena.params).all())}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optim", choices=["sgd", "adamw", "both"], default="both")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    kern.set_compute_bf16(True)
    ops.set_wgrad_overlap(False)  # (bench.py captures its graph with the weight gradients on the main stream)
    for name in (["sgd", "adamw"] if a.optim == "both" else [a.optim]):
        r = run(name, a.batch, a.steps, a.warmup)
        if not r["finite"]:
            sys.exit(f"{name}: non-finite parameters")


if __name__ == "__main__":
    main()
