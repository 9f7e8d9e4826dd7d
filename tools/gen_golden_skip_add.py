"""Golden vectors for skip_mode='add' (TEST INFRASTRUCTURE; runs ONLY in the build container, on the CPU).

Imports the unmodified reference through oracle/ref_shim exactly as oracle/gen_golden.py does (that module is imported for its path
set-up and helpers, nothing under oracle/ is changed), and writes under tests/golden/:
  mod_dseb_add.npz, mod_dseb_add_hd10.npz, mod_dseb_add_hd4.npz   one DSEBlock(mode='add') each: weights, inputs, eval / train
                                                                   outputs, input and parameter gradients
  model_{acdc,synapse}_add.npz     CENet(skip_mode='add'), B = 2 at 224^2: the quantities of model_acdc.npz
  model_acdc_add_64.npz            eval logits at 64 x 64 (host-checker test)
  schema_acdc_add.json             keys, order and shapes of CENet(skip_mode='add') (ACDC preset)

oracle.cenet_oracle only knows the cat layout, so the weights come from the reference CONSTRUCTOR under a recorded torch seed
(`ctor_seed`); a float64 sum and absolute sum per tensor of those constructor weights is stored (`ck_keys` / `ck_sum`) so that
the tests can check that the product's constructor draws the same weights.  The model fixtures then overwrite every tensor with
oracle.cenet_oracle.fill_state_dict_ (`fill_seed`; at constructor init CFAM's layer scales are 1e-6 and BatchNorm's running
statistics trivial); fill_state_dict_ walks the keys in sorted order and depends on shapes only, so the tests rebuild the same
values from the product's own state dict.  The layer scales are filled at LAYER_SCALE = 0.02, not the 0.5 of the cat fixtures:
with 0.5 the add-mode network amplifies fp32 rounding (the reference's own fp32 logits are 0.79 away from its float64 logits
at 224^2, ACDC) and no 1e-3 comparison is meaningful; at 0.02 that distance is 1.1e-4 (ACDC) / 5.7e-5 (Synapse).
Re-run:  python tools/gen_golden_skip_add.py
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import gen_golden as G  # noqa: E402  (puts ref_shim and the reference sources on sys.path)
from oracle import cenet_oracle as O  # noqa: E402
from oracle.gen_golden_keys import PROBE_BUFFERS, PROBE_KEYS  # noqa: E402

import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
THREADS = 8  # the reference's CPU results move by ~1e-6 between 4 and 8 threads
LAYER_SCALE = 0.02

# name -> (DSEBlock kwargs, B, H, W, ctor seed); head dim = dim / num_heads / 2
DSEB_CASES = {
    "dseb_add": (dict(dim=80, scale_factors=[1.0, 0.5], num_heads=1, input_size=12, mode="add", depth=4), 2, 12, 12, 301),
    "dseb_add_hd10": (dict(dim=80, scale_factors=[0.8, 0.4], num_heads=4, input_size=10, mode="add", depth=4), 2, 10, 10, 302),
    "dseb_add_hd4": (dict(dim=64, scale_factors=[0.8, 0.4], num_heads=8, input_size=10, mode="add", depth=2), 2, 10, 10, 303),
}
MODEL_CASES = {
    "acdc_add": dict(kw=dict(input_channels=1, num_classes=4, scale_factors=[1.0, 0.5], diffatt_num_heads=[4, 4, 4],
                             out_up_block="upcn", skip_mode="add"), batch=2, ctor_seed=5, fill_seed=42),
    "synapse_add": dict(kw=dict(input_channels=1, num_classes=9, scale_factors=[0.8, 0.4], diffatt_num_heads=[16, 8, 8],
                                out_up_block="upcn", skip_mode="add"), batch=2, ctor_seed=5, fill_seed=42),
}


def checksums(sd):
    """per tensor: float64 sum and absolute sum (the form tests/test_wellcond.py pins the cat-mode initialisation with)"""
    keys = list(sd.keys())
    sums = [[sd[k].double().sum().item(), sd[k].double().abs().sum().item()] for k in keys]
    return {"ck_keys": np.array(keys), "ck_sum": np.array(sums, dtype=np.float64)}


def gen_dseb():
    cls = getattr(importlib.import_module("networks.cenet.modules.dseb"), "DSEBlock")
    for name, (kw, B, H, W, seed) in DSEB_CASES.items():
        torch.manual_seed(seed)
        m = cls(**kw)
        rec = {"ctor_seed": np.int64(seed), **checksums(m.state_dict())}
        for k, v in m.state_dict().items():
            rec["sd." + k] = v.detach().clone().numpy()
        g = torch.Generator().manual_seed(seed + 1000)
        ins = [torch.randn(B, kw["dim"], H, W, generator=g).requires_grad_(True) for _ in range(2)]  # (skip, dec)
        for i, t in enumerate(ins):
            rec[f"in{i}"] = t.detach().numpy()
        m.eval()
        with torch.no_grad():
            rec["out_eval"] = m(ins[0].detach(), ins[1].detach()).numpy()
        m.train()
        out = m(ins[0], ins[1])
        cot = torch.randn(out.shape, generator=g)
        (out * cot).sum().backward()
        rec["out"] = out.detach().numpy()
        rec["cot"] = cot.numpy()
        for i, t in enumerate(ins):
            rec[f"gin{i}"] = t.grad.numpy()
        for k, p in m.named_parameters():
            rec["gsd." + k] = p.grad.numpy()
        path = os.path.join(OUT, f"mod_{name}.npz")
        np.savez_compressed(path, **rec)
        print(f"[golden] {name}: hd {kw['dim'] // kw['num_heads'] // 2}  {os.path.getsize(path) / 1024:.0f} KiB")


def build_ref(kw, ctor_seed, fill_seed):
    from networks import CENet
    torch.manual_seed(ctor_seed)
    net = CENet(**kw)
    ck = checksums(net.state_dict())
    if fill_seed is not None:
        O.fill_state_dict_(net.state_dict(), seed=fill_seed, layer_scale=LAYER_SCALE)
    return net, ck


def gen_models(core):
    for name, mc in MODEL_CASES.items():
        kw, B = mc["kw"], mc["batch"]
        K = kw["num_classes"]
        net, ck = build_ref(kw, mc["ctor_seed"], mc["fill_seed"])
        x, lab = G.synthetic_batch(B, kw["input_channels"], K)
        rec = {"x_seed": np.int64(1234), "ctor_seed": np.int64(mc["ctor_seed"]), "fill_seed": np.int64(mc["fill_seed"]),
               "layer_scale": np.float64(LAYER_SCALE), **ck}
        net.eval()
        with torch.no_grad():
            le = net(x)
        rec["logits_eval_sub"] = le[:, :, ::9, ::9].numpy()
        rec["logits_eval_sum"] = np.float64(le.double().sum().item())
        rec["logits_eval_abs"] = np.float64(le.double().abs().sum().item())
        rec["pred_eval_sub"] = torch.argmax(torch.softmax(le, 1), 1)[:, ::5, ::5].numpy().astype(np.int8)
        rec["dice_eval"] = np.float64(O.mean_class_dice(le, lab, K))
        net.train()
        net.backbone.reset_drop_path(0.0)
        crit = core.Criterion(K, argparse.Namespace(loss_type="dice,ce", loss_weights="0.5,0.5"))
        opt = torch.optim.SGD(net.parameters(), lr=0.01, weight_decay=1e-4, momentum=0.9)
        opt.zero_grad()
        lt = net(x)
        loss = crit(lt, lab)
        loss.backward()
        rec["logits_train_sub"] = lt.detach()[:, :, ::9, ::9].numpy()
        rec["loss"] = np.float64(loss.item())
        params = dict(net.named_parameters())
        for k in PROBE_KEYS:
            gk = params[k].grad.reshape(-1)
            rec["g." + k + ".norm"] = np.float64(gk.double().norm().item())
            rec["g." + k + ".head"] = gk[:16].numpy().copy()
        bufs = dict(net.named_buffers())
        for k in PROBE_BUFFERS:
            rec["b." + k] = bufs[k].detach().reshape(-1)[:16].numpy().copy()
        opt.step()
        for k in PROBE_KEYS:
            rec["p1." + k + ".head"] = params[k].detach().reshape(-1)[:16].numpy().copy()
        opt.zero_grad()
        loss2 = crit(net(x), lab)
        loss2.backward()
        opt.step()
        rec["loss2"] = np.float64(loss2.item())
        for k in PROBE_KEYS:
            rec["p2." + k + ".head"] = params[k].detach().reshape(-1)[:16].numpy().copy()
        # the first training pass in float64: the gradient budgets of test_model_parity.py
        net64, _ = build_ref(kw, mc["ctor_seed"], mc["fill_seed"])
        net64 = net64.double()
        net64.train()
        net64.backbone.reset_drop_path(0.0)
        loss64 = crit(net64(x.double()), lab.double())
        loss64.backward()
        rec["loss64"] = np.float64(loss64.item())
        p64 = dict(net64.named_parameters())
        for k in PROBE_KEYS:
            gk = p64[k].grad.reshape(-1)
            rec["g64." + k + ".norm"] = np.float64(gk.norm().item())
            rec["g64." + k + ".head"] = gk[:16].numpy().copy()
        path = os.path.join(OUT, f"model_{name}.npz")
        np.savez_compressed(path, **rec)
        print(f"[golden] model_{name}: loss {loss.item():.6f} -> {loss2.item():.6f}  dice_eval {rec['dice_eval']:.4f}  "
              f"{os.path.getsize(path) / 1024:.0f} KiB")


def gen_small_and_schema():
    mc = MODEL_CASES["acdc_add"]
    net, ck = build_ref(mc["kw"], 7, 7)
    sd = net.state_dict()
    with open(os.path.join(OUT, "schema_acdc_add.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in sd.items()}, f)
    # (dseb.py:117 reshapes the attention output with the block's input_size, fixed for 224^2 inputs: set it for 64^2)
    for lvl, side in ((3, 4), (2, 8), (1, 16)):
        getattr(net.decoder, f"skip_enhancer{lvl}").input_size = side
    net.eval()
    x = torch.randn(1, 1, 64, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        le = net(x)
    path = os.path.join(OUT, "model_acdc_add_64.npz")
    np.savez_compressed(path, ctor_seed=np.int64(7), fill_seed=np.int64(7), layer_scale=np.float64(LAYER_SCALE), x_seed=np.int64(3), logits=le.numpy(), **ck)
    print(f"[golden] model_acdc_add_64: {len(sd)} tensors, logits {tuple(le.shape)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="all", choices=["all", "modules", "models", "small"])
    a = ap.parse_args()
    torch.set_num_threads(THREADS)
    os.makedirs(OUT, exist_ok=True)
    if a.only in ("all", "modules"):
        gen_dseb()
    if a.only in ("all", "small"):
        gen_small_and_schema()
    if a.only in ("all", "models"):
        gen_models(G.load_reference_losses())


if __name__ == "__main__":
    main()
