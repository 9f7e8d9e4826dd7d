"""FusedAdamW + the cosine schedule in the captured step (GPU).

* train.train_acdc(optimizer="adamw", scheduler="cosine"): the replayed loop equals the eager loop on CHANGING batches in both
  storage modes, with the bounds of tests/test_train_loop.py, and the optimizer counts every replayed step;
* five GraphedStep replays of the real ACDC network with FusedAdamW (fp32 mode) equal five eager steps: the lr and the bias
  corrections advance under replay (prepare() uploads them; nothing is baked into the capture)."""
import argparse
import copy

import numpy as np
import pytest
import torch

import bench
from backend import use_hip
from oracle import cenet_oracle as O

pytestmark = pytest.mark.gpu


class _Toy(torch.utils.data.Dataset):
    def __init__(self, n, seed):
        self.x, self.lab = O.synthetic_batch(n, 1, 4, seed=seed)

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return {"image": self.x[i], "label": self.lab[i].long(), "case_name": f"case{i}"}


def _net(dev):
    from cenet_amd.networks import CENet
    torch.manual_seed(77)
    net = CENet(input_channels=1, num_classes=4, scale_factors=[1.0, 0.5], diffatt_num_heads=[4, 4, 4], out_up_block="upcn")
    net.backbone.reset_drop_path(0.0)
    return net.to(dev)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_adamw_cosine_replayed_loop_equals_the_eager_loop(bf16):
    from cenet_amd import kern, optim, train
    dev = use_hip()
    loader = torch.utils.data.DataLoader(_Toy(14, seed=21), batch_size=4, shuffle=False)  # 3 full batches + a ragged one
    xv, lv = O.synthetic_batch(3, 1, 4, seed=5)
    val = lambda: [(xv[i:i + 1].to(dev), lv[i:i + 1].to(dev)) for i in range(3)]  # noqa: E731
    ref_net = _net(dev)
    old = kern.set_compute_bf16(bf16)
    try:
        runs = []
        for graph in (False, True):
            net = copy.deepcopy(ref_net)
            h = train.train_acdc(net, loader, max_epochs=2, base_lr=1e-4, device=dev, graph=graph, val_batches=val, log_every=1,
                                 log=lambda s: None, optimizer="adamw", scheduler="cosine")
            runs.append(h)
    finally:
        kern.set_compute_bf16(old)
    he, hg = runs
    assert type(hg["optimizer"]) is optim.FusedAdamW
    assert len(he["loss"]) == len(hg["loss"]) == 8 and he["lr"] == hg["lr"]
    assert he["lr"][0] == 1e-4 and he["lr"][-1] < he["lr"][1] < 1e-4  # the cosine schedule drove the lr
    le, lg = np.array([v for _, v in he["loss"]]), np.array([v for _, v in hg["loss"]])
    tol = 2e-2 if bf16 else 2e-4
    assert np.abs(le - lg).max() < tol, (le, lg)
    assert len(set(np.round(le, 4))) > 4
    assert abs(he["val_dice"][-1] - hg["val_dice"][-1]) < (5e-2 if bf16 else 5e-3)
    pe, pg = he["arena"].params, hg["arena"].params
    cos = torch.nn.functional.cosine_similarity(pe - pe.mean(), pg - pg.mean(), dim=0).item()
    assert cos > 0.99999
    # one capture, eight iterations counted by the optimizer (the bias corrections follow this counter)
    assert hg["optimizer"]._steps == 8 and he["optimizer"]._steps == 8


def _steps(net, dev, graph, n=5):
    from cenet_amd import losses, optim
    from cenet_amd.graph import GraphedStep
    arena = optim.ParamArena(net, optim.cenet_segments())
    p0 = arena.params.clone()
    opt = optim.FusedAdamW(arena, lr=1e-3, weight_decay=1e-2)
    sched = optim.CosineLR(opt, T_max=8)
    crit = losses.Criterion(4, argparse.Namespace(loss_type="dice,ce", loss_weights="0.5,0.5"))
    x, lab = bench.synthetic(4, dev, 7)

    def body():
        opt.zero_grad()
        loss = crit(net(x), lab)
        loss.backward()
        opt.step(sync_hyper=False)
        return loss

    out = []
    if graph:
        # the capture's warm-up step is a real step: put the model and the optimizer back where they were
        snap = (arena.params.clone(), [b.clone() for b in opt.state_buffers()], opt._steps,
                {k: v.clone() for k, v in net.state_dict().items() if "running_" in k or "num_batches" in k})
        g = GraphedStep(body, optimizer=opt, warmup=1)
        arena.params.copy_(snap[0])
        for b, s in zip(opt.state_buffers(), snap[1]):
            b.copy_(s)
        opt._steps = snap[2]
        net.load_state_dict(snap[3], strict=False)
        arena.refresh_shadow()
        for _ in range(n):
            out.append(float(g().detach()))
            sched.step()
    else:
        for _ in range(n):
            opt.prepare()
            out.append(float(body().detach()))
            sched.step()
    torch.cuda.synchronize()
    return out, arena.params - p0, opt


def test_graphed_adamw_replays_equal_eager_steps():
    from cenet_amd import kern, ops
    dev = use_hip()
    old_bf, old_ov = kern.set_compute_bf16(False), ops.set_wgrad_overlap(False)
    try:
        torch.manual_seed(3)
        base = bench.make_model(dev)
        for m in base.modules():  # DropPath draws host randomness per step: keep the two runs on the same masks
            if hasattr(m, "drop_prob"):
                m.drop_prob = 0.0
        rep = copy.deepcopy(base)
        le, de, oe = _steps(base, dev, graph=False)
        lg, dg, og = _steps(rep, dev, graph=True)
    finally:
        kern.set_compute_bf16(old_bf)
        ops.set_wgrad_overlap(old_ov)
    assert oe._steps == og._steps == 5 and oe.lr == og.lr
    for a, b in zip(le, lg):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (le, lg)
    # the parameter updates agree in direction AND size: a replay stuck on step 1's bias correction (step_size 10x lr) or lr
    # would change the size of every later update
    cos = torch.nn.functional.cosine_similarity(de, dg, dim=0).item()
    ratio = (dg.norm() / de.norm()).item()
    assert cos > 0.999 and abs(ratio - 1) < 1e-2, (cos, ratio)
