"""Cost of the loss with options (csrc/seg_loss_ex.hip) beside the existing fused loss (csrc/loss_optim.hip) at the ACDC shape
(B = 32, K = 4, 224 x 224), fp32 and bf16 logits:   python tools/loss_bench.py [reps] [replays]

Forward + backward of
  dice_ce   ops.dice_ce_loss(w_dice=0.5, w_ce=0.5)                                 the existing kernel pair, the baseline
  neutral   ops.seg_loss with unit class weights, no ignore_index, no Jaccard term
  options   ops.seg_loss(dice + ce + jaccard, both weight vectors, ignore_index=255; the first 9 rows of image 0 and the whole
            last image ignored)
Each configuration is captured once as `reps` (>= 100) forward + backward pairs in one graph, so that the device runs them back to
back without the host in between; the graphs are replayed in turn (`replays` rounds, alternating the configurations) with
device events around each replay.  Reported: the median over the rounds of (replay time / reps), in microseconds, and for the new
path the same split into its forward call (two launches: the pass that stores the rows of partial sums and the one-workgroup
sum) and its backward call.  Writes profiles/seg_loss_ex.json."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cenet_amd import build, kern, ops  # noqa: E402

REPS = max(100, int(sys.argv[1])) if len(sys.argv) > 1 else 200
REPLAYS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
B, K, H, W = 32, 4, 224, 224
dev = torch.device("cuda:0")


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    return g


def main():
    g = torch.Generator().manual_seed(0)
    logits32 = torch.randn(B, K, H, W, generator=g) * 2
    low = torch.rand(B, 1, 14, 14, generator=g)
    labels = torch.floor(torch.nn.functional.interpolate(low, size=(H, W), mode="nearest") * K).clamp_(0, K - 1)[:, 0].contiguous()
    void = labels.clone()
    void[0, :9] = 255
    void[-1] = 255
    labels, void = labels.to(dev), void.to(dev)
    wd, wc = (0.2 + 2.8 * torch.rand(2, K, generator=g)).tolist()
    ones = [1.0] * K
    graphs, keep = {}, []  # keep: every tensor a captured graph reads or writes must stay allocated as long as the graph is replayed
    for mode in ("f32", "bf16"):
        lg = (logits32.to(torch.bfloat16) if mode == "bf16" else logits32).to(dev).requires_grad_(True)

        def pair(loss_fn, lg=lg):
            torch.autograd.grad(loss_fn(lg), lg)

        graphs[mode, "dice_ce"] = graphed(lambda: pair(lambda x: ops.dice_ce_loss(x, labels, 0.5, 0.5)))
        graphs[mode, "neutral"] = graphed(lambda: pair(lambda x: ops.seg_loss(x, labels, w_dice=0.5, w_ce=0.5, dice_class_weights=ones,
                                                                              ce_class_weights=ones)))
        graphs[mode, "options"] = graphed(lambda: pair(lambda x: ops.seg_loss(x, void, w_dice=0.4, w_ce=0.3, w_jaccard=0.3,
                                                                              dice_class_weights=wd, ce_class_weights=wc, ignore_index=255)))
        # the new path's two calls on their own (option set as in `options`)
        cw = ops.class_weight_buffer(K, wd, wc, dev)
        ws = torch.empty(kern.seg_loss_ex_ws_floats(B, K, H, W), device=dev)
        loss, gout, d = torch.empty(1, device=dev), torch.ones(1, device=dev), torch.empty_like(lg)
        cfg = (0.4, 0.3, 0.0, 0.3, 1.0, 255, False)
        x = lg.detach()
        graphs[mode, "options_fwd"] = graphed(lambda: kern.seg_loss_ex_fwd(x, void, cw, ws, loss, B, K, H, W, *cfg))
        graphs[mode, "options_bwd"] = graphed(lambda: kern.seg_loss_ex_bwd(x, void, cw, ws, gout, d, B, K, H, W, *cfg))
        keep += [lg, x, cw, ws, loss, gout, d]
    times = {k: [] for k in graphs}
    for _ in range(REPLAYS + 2):
        for k, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1000.0 / REPS)
    out = {"shape": {"B": B, "K": K, "H": H, "W": W}, "reps_per_replay": REPS, "replays": REPLAYS, "unit": "microseconds",
           "device": torch.cuda.get_device_name(0), "kernel_src_sha16": build.source_sha16(), "median_us": {}, "min_us": {}, "max_us": {}}
    for (mode, name), ts in times.items():
        ts = ts[2:]  # (the first two rounds warm the graphs up)
        out["median_us"][f"{mode}.{name}"] = round(statistics.median(ts), 3)
        out["min_us"][f"{mode}.{name}"] = round(min(ts), 3)
        out["max_us"][f"{mode}.{name}"] = round(max(ts), 3)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "seg_loss_ex.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["median_us"]))


if __name__ == "__main__":
    main()
