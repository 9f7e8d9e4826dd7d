"""The reference's training loop (src/main_acdc.py:200-290) on the MI355X-native step: loader -> DevicePrefetcher -> STATIC input
buffers -> one hipGraph replay per iteration (cenet_amd.graph.GraphedStep) -> learning-rate schedule -> per-epoch validation on the
device (cenet_amd.evaluate.validate).

What differs from the reference loop and why:
  * the batch is copied into two static device tensors and the captured step reads those: a hipGraph replays fixed addresses
    (main_acdc.py:238-240 moves a fresh tensor to the GPU per iteration); the copy is one device-to-device kernel per tensor on
    the training stream, the host-to-device upload already happened on the prefetcher's copy stream;
  * a ragged last batch of an epoch (DataLoader(drop_last=False), main_acdc.py:139) runs eagerly — BatchNorm statistics and the
    Dice sums depend on the batch, so it cannot be padded;
  * the loss is read back once per `log_every` iterations instead of every iteration (main_acdc.py:264-265: a device sync per
    step); the running epoch loss is accumulated on the device;
  * the learning rate (and Adam's bias corrections) for the NEXT step is uploaded by the optimizer's prepare() before each
    replay (no host value is baked into the capture);
  * the epoch log line prints the reference's quantity — the sum of the batch losses over the number of training images
    (main_acdc.py:264-267) — but accumulated on the device and read back once per epoch;
  * the epoch tail of main_acdc.py:270-289 (test inference when the validation Dice does not fall, `best.pth`, the last-epoch
    file) runs when `test_volumes` is given: cenet_amd.evaluate.inference with both resizes on the device, weights through
    cenet_amd.checkpoint.save_weights.  The loop still returns the arena and the optimizer (save_training_state takes them).
`train_acdc(..., graph=False)` is the same loop with eager launches: tests/test_train_loop.py holds the two against each other
on changing batches."""
from __future__ import annotations

import argparse
from typing import Callable, Iterable, List, Optional

import torch

from . import graph as G
from . import losses, optim
from .data import DevicePrefetcher


def _as_batches(loader) -> Iterable[dict]:
    return loader


def criterion_args(loss_type: str = "dice,ce", loss_weights: str = "0.5,0.5", dice_class_weights=None, ce_class_weights=None,
                   ignore_index=None, lovasz_per_image=False, topk_percent=10.0, topk_per_image=False) -> argparse.Namespace:
    """the `args` train_acdc hands losses.Criterion"""
    return argparse.Namespace(loss_type=loss_type, loss_weights=loss_weights, dice_class_weights=dice_class_weights,
                              ce_class_weights=ce_class_weights, ignore_index=ignore_index, lovasz_per_image=lovasz_per_image,
                              topk_percent=topk_percent, topk_per_image=topk_per_image)


def train_acdc(net, tr_loader, *, num_classes: int = 4, max_epochs: int = 1, base_lr: float = 0.05, momentum: float = 0.9,
               weight_decay: float = 1e-4, loss_type: str = "dice,ce", loss_weights: str = "0.5,0.5", device="cuda:0",
               graph: bool = True, val_batches: Optional[Callable[[], Iterable]] = None, log_every: int = 20,
               log: Callable[[str], None] = print, optimizer: str = "sgd", scheduler: str = "poly",
               test_volumes: Optional[Callable[[], Iterable]] = None, save_dir: Optional[str] = None, img_size: int = 224,
               test_resize: str = "device", dice_class_weights=None, ce_class_weights=None, ignore_index=None,
               test_postprocess=None, dist_weight_schedule: Optional[Callable[[int], tuple]] = None, test_tta=None,
               test_spacing=None, test_nsd_tolerance=None, lovasz_per_image=False, topk_percent=10.0,
               topk_per_image=False, topk_schedule: Optional[Callable[[int], float]] = None,
               test_window_overlap=None) -> dict:
    """main_acdc.py:200-290.  tr_loader yields {'image' [B,C,H,W] float (C = the network's input channels), 'label' [B,H,W]} batches (host or device tensors);
    val_batches() yields (image [1,1,H,W], label [1,H,W]) pairs for the per-epoch validation (main_acdc.py:218-231).
    optimizer / scheduler: the reference's --optimizer / --scheduler strings (main_acdc.py:34-35, core.py:12-41); `momentum`
    applies to SGD, Adam / AdamW take betas (0.9, 0.999) and eps 1e-8 as the reference does.
    test_volumes() yields the test loader's dicts (`image` [1,D,H,W], `label`, `case_name`) and needs val_batches: after an
    epoch whose validation Dice is >= the best so far, evaluate.inference runs over them (slices resized to img_size, `test_resize`
    as evaluate.test_single_volume takes it, `test_postprocess` as its `postprocess`: None or "lcc", `test_tta` as its `tta`: None, a name of evaluate.TTA_SETS or a tuple of view codes,
    with test_resize="device" only, `test_window_overlap` as its `window_overlap`: None or a number in [0, 1) for sliding-window
    inference with img_size windows, with test_resize="device" only, `test_spacing` / `test_nsd_tolerance` as its `spacing` / `nsd_tolerance`: the voxel spacing in
    which te_HD95 is then reported, for all cases or per case, and the tolerance of the normalised surface Dice, which adds
    'test_nsd' to the result); only when its Dice is >= the best test Dice do BOTH bests move and `best.pth` is
    written (main_acdc.py:272-278: a validation gain without a test gain moves neither); the last epoch writes
    `epoch=<e>_lr=<lr>_avg_dcs=<last test dice>.pth` (:286-289).  Files go to save_dir (None: none are written).
    -> {'loss': per-iteration losses read back at log points, 'epoch_loss': [...], 'val_dice': [...], 'lr': [...]} and, with
    test_volumes, 'test_dice' / 'test_hd95' (one entry per inference run) and 'best_epochs' (epochs that wrote best.pth)
    loss_type may name `jaccard`; dice_class_weights / ce_class_weights (comma string or num_classes floats) and ignore_index
    are losses.Criterion's optional attributes of the same names (None: the loss path without them).
    loss_type may also name `surface` and `hausdorff` (the distance-map losses, their weights in loss_weights);
    dist_weight_schedule: epoch -> (w_surface, w_hausdorff), called at the start of every epoch and handed to
    Criterion.set_dist_weights — the weights are read on the device, so the captured step is replayed, not recaptured
    (Kervadec's rebalancing moves the surface weight every epoch)
    loss_type may name `lovasz` too (the Lovasz-Softmax loss, its weight in loss_weights; lovasz_per_image: every image on its
    own): sort, ranks and coefficients are launches of the captured step like any other
    loss_type may name `topk` (the top-k cross-entropy, its weight in loss_weights; topk_percent: the k % of pixels with the
    largest loss that count; topk_per_image: every image on its own); topk_schedule: epoch -> percent, called at the start of
    every epoch and handed to Criterion.set_topk_percent — the percentage is read on the device, so the captured step is
    replayed, not recaptured"""
    import os

    from . import checkpoint, evaluate
    if test_volumes is not None and val_batches is None:
        raise ValueError("test_volumes: the test inference is gated by the validation Dice, pass val_batches too")
    evaluate._check_postprocess(test_postprocess)
    if test_tta is not None:
        evaluate._tta_mask(test_tta, img_size, img_size)
        if test_resize != "device":
            raise ValueError(f"test_tta={test_tta!r} needs test_resize='device', got {test_resize!r}")
    if test_window_overlap is not None:
        evaluate._window_args(test_window_overlap, "gaussian")
        if test_resize != "device":
            raise ValueError(f"test_window_overlap={test_window_overlap!r} needs test_resize='device', got {test_resize!r}")
    if save_dir is not None and test_volumes is None:
        raise ValueError("save_dir: the checkpoints of main_acdc.py:272-289 are written by the test inference, pass test_volumes")
    dev = torch.device(device)
    net = net.to(dev).train()
    crit = losses.Criterion(num_classes, criterion_args(loss_type, loss_weights, dice_class_weights, ce_class_weights,
                                                        ignore_index, lovasz_per_image, topk_percent=topk_percent,
                                                        topk_per_image=topk_per_image)).to(dev)
    if dist_weight_schedule is not None and crit.dist_weights is None:
        raise ValueError("dist_weight_schedule: loss_type names neither surface nor hausdorff")
    if topk_schedule is not None and crit.topk_percent is None:
        raise ValueError("topk_schedule: loss_type does not name topk")
    arena = optim.ParamArena(net, optim.cenet_segments())
    if optimizer.lower() == "sgd":
        opt = optim.FusedSGD(arena, lr=base_lr, momentum=momentum, weight_decay=weight_decay)
    else:
        opt = optim.get_optimizer(net, argparse.Namespace(optimizer=optimizer, base_lr=base_lr, weight_decay=weight_decay))
    sched = optim.get_scheduler(opt, argparse.Namespace(scheduler=scheduler, base_lr=base_lr, max_epochs=max_epochs),
                                max_iterations=max_epochs * len(tr_loader))
    hist = {"loss": [], "epoch_loss": [], "val_dice": [], "lr": []}
    if test_volumes is not None:
        hist.update(test_dice=[], test_hd95=[], best_epochs=[])
    best_val = best_test = 0
    te_dice = None
    static = {}
    stepper: List[Optional[G.GraphedStep]] = [None]

    def body(x, lab):
        opt.zero_grad()
        loss = crit(net(x), lab)
        loss.backward()
        opt.step(sync_hyper=False)
        return loss

    def one_step(x, lab):
        if graph and (not static or x.shape == static["x"].shape):
            if not static:
                static["x"], static["lab"] = torch.empty_like(x), torch.empty_like(lab)
            static["x"].copy_(x, non_blocking=True)
            static["lab"].copy_(lab, non_blocking=True)
            if stepper[0] is None:
                # (the capture's warm-up runs are REAL optimizer steps: keep the model where it is with a snapshot)
                snap = (arena.params.clone(), [b.clone() for b in opt.state_buffers()], opt._steps,
                        {k: v.clone() for k, v in net.state_dict().items() if "running_" in k or "num_batches" in k})
                stepper[0] = G.GraphedStep(lambda: body(static["x"], static["lab"]), optimizer=opt, warmup=2)
                arena.params.copy_(snap[0])
                for b, saved in zip(opt.state_buffers(), snap[1]):
                    b.copy_(saved)
                opt._steps = snap[2]
                net.load_state_dict(snap[3], strict=False)
                arena.refresh_shadow()
            return stepper[0]()
        opt.prepare()
        return body(x, lab)

    it = 0
    for epoch in range(max_epochs):
        net.train()
        if dist_weight_schedule is not None:
            crit.set_dist_weights(*dist_weight_schedule(epoch))
        if topk_schedule is not None:
            crit.set_topk_percent(topk_schedule(epoch))
        run = torch.zeros((), device=dev)
        n_img = 0
        for batch in DevicePrefetcher(_as_batches(tr_loader), dev):
            x, lab = batch["image"].float(), batch["label"].float()
            loss = one_step(x, lab)
            hist["lr"].append(sched.get_last_lr()[0])
            sched.step()
            it += 1
            run += loss.detach().float()  # main_acdc.py:264: the plain batch loss ...
            n_img += x.shape[0]
            if it % log_every == 0:
                hist["loss"].append((it, loss.item()))
                log(f"iteration {it} : loss : {hist['loss'][-1][1]:f} lr_: {hist['lr'][-1]:f}")
        hist["epoch_loss"].append(run.item() / max(n_img, 1))  # ... over len(db_train) (main_acdc.py:266), as the reference logs it
        if val_batches is not None:
            hist["val_dice"].append(evaluate.validate(net, val_batches()))
            net.train()
        lr_last = hist["lr"][-1] if hist["lr"] else base_lr  # (an empty loader takes no step)
        log(f"epoch:{epoch:03d}/{max_epochs}, loss:{hist['epoch_loss'][-1]:0.5f}, lr:{lr_last:0.6f}"
            + (f", vl_DCS:{hist['val_dice'][-1] * 100:0.3f}" if hist["val_dice"] else ""))
        if test_volumes is None:
            continue
        vl = hist["val_dice"][-1]
        if vl >= best_val:
            te = evaluate.inference(net, test_volumes(), num_classes, patch_size=(img_size, img_size), log=log,
                                    resize=test_resize,
                                    **({} if test_postprocess is None else {"postprocess": test_postprocess}),
                                    **({} if test_tta is None else {"tta": test_tta}),
                                    **({} if test_window_overlap is None else {"window_overlap": test_window_overlap}),
                                    **({} if test_spacing is None else {"spacing": test_spacing}),
                                    **({} if test_nsd_tolerance is None else {"nsd_tolerance": test_nsd_tolerance}))
            te_dice, te_hd = te[:2]
            if test_nsd_tolerance is not None:
                hist.setdefault("test_nsd", []).append(te[2])
            net.train()
            if te_dice >= best_test:
                best_val, best_test = vl, te_dice
                hist["best_epochs"].append(epoch)
                if save_dir is not None:
                    os.makedirs(save_dir, exist_ok=True)
                    checkpoint.save_weights(net, os.path.join(save_dir, "best.pth"))
                    log(f"save model to {os.path.join(save_dir, 'best.pth')}")
            hist["test_dice"].append(te_dice)
            hist["test_hd95"].append(te_hd)
            log(f"epoch:{epoch:03d}/{max_epochs}, te_DCS:{te_dice * 100:0.3f}, te_HD95:{te_hd:0.2f}")
        if epoch >= max_epochs - 1 and save_dir is not None:
            os.makedirs(save_dir, exist_ok=True)
            path = os.path.join(save_dir, f"epoch={epoch}_lr={lr_last}_avg_dcs={te_dice}.pth")
            checkpoint.save_weights(net, path)
            log(f"save model to {path}")
    hist["arena"], hist["optimizer"] = arena, opt
    return hist
