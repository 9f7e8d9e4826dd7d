"""The device-side Synapse augmentation (data.SegAugmenter, csrc/augment_ops.hip) where it is used: feeding the training loop of
the Synapse configuration through DeviceTrainLoader(augmenter=...), and keeping up with that step."""
import copy
import time

import numpy as np
import pytest
import torch

from backend import use_hip
from cenet_amd import data as D

STEP_IMAGES_PER_S = 1385  # the Synapse preset's captured training step (README status table; batch 24)


def _slices(shapes, seed, dev):
    rng = np.random.default_rng(seed)
    return D.DeviceSlices([(rng.random(s).astype(np.float32), rng.integers(0, 9, s).astype(np.uint8)) for s in shapes], dev)


@pytest.mark.gpu
def test_replayed_synapse_loop_fed_by_the_augmenter_equals_the_eager_loop():
    """train_acdc on the Synapse configuration (9 classes, 224 x 224, heads 16 / 8 / 8, scales 0.8 / 0.4), 2 epochs of 2 batches of 4
    from DeviceTrainLoader over a SegAugmenter: two loaders with the same seeds give the same batches, so the captured-graph loop
    equals the eager loop loss for loss (tests/test_train_loop.py's bound for the fp32 step)"""
    from cenet_amd import train
    from cenet_amd.networks import CENet
    dev = use_hip()
    sl = _slices([(256, 256), (230, 250), (224, 224), (256, 200)] * 2, 3, dev)
    torch.manual_seed(77)
    ref_net = CENet(input_channels=1, num_classes=9, scale_factors=[0.8, 0.4], diffatt_num_heads=[16, 8, 8], out_up_block="upcn")
    ref_net.backbone.reset_drop_path(0.0)  # (stochastic depth draws random masks: both loops must see the same network)
    ref_net = ref_net.to(dev)
    runs, firsts = [], []
    for graph in (False, True):
        aug = D.SegAugmenter(sl, (224, 224), normalize=(0.5, 0.5), seed=12)
        loader = D.DeviceTrainLoader(sl, (224, 224), batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(31),
                                     augmenter=aug)
        h = train.train_acdc(copy.deepcopy(ref_net), loader, num_classes=9, max_epochs=2, base_lr=0.01, device=dev, graph=graph,
                             log_every=1, log=lambda s: None)
        runs.append(np.array([v for _, v in h["loss"]]))
        firsts.append(aug.picked)
        assert h["optimizer"]._steps == 4
    le, lg = runs
    assert firsts[0] == firsts[1] and any(p for p in firsts[0])  # the same (non-trivial) augmentation decisions
    assert len(le) == len(lg) == 4
    assert np.abs(le - lg).max() < 2e-4, (le, lg)
    assert len(set(np.round(le, 4))) > 2  # the batches (and therefore the losses) do change from iteration to iteration


@pytest.mark.gpu
def test_costliest_plan_keeps_up_with_the_synapse_step():
    """batch 24, 512 x 512 -> 224 x 224 with Normalize, four stages of warps and blurs on EVERY sample (grid warp, blur, rotation,
    blur: two blurs, which a draw of distinct operators never gives): table upload + stages + resize + normalize must deliver more
    images per second than the preset's training step consumes"""
    dev = use_hip()
    rng = np.random.default_rng(0)
    sl = _slices([(512, 512)] * 32, 1, dev)
    aug = D.SegAugmenter(sl, (224, 224), normalize=(0.5, 0.5), seed=1)
    idx = [int(i) for i in rng.permutation(32)[:24]]

    def chain():
        a = np.deg2rad(rng.uniform(-40, 40))
        return [("grid_warp", rng.normal(0, 0.03, (4, 4)) * 512, rng.normal(0, 0.03, (4, 4)) * 512), ("blur", 1.0),
                ("affine", *D.centred_affine([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], (512, 512))), ("blur", 1.0)]

    plan = aug.plan(idx, [chain() for _ in idx])
    assert plan[0].shape == (24, 7) and (plan[0][:, 3:] != 0).all()
    for _ in range(3):
        out = aug.apply(plan)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 10
    for _ in range(reps):
        out = aug.apply(plan)
    torch.cuda.synchronize()
    rate = reps * 24 / (time.perf_counter() - t0)
    print(f"costliest plan: {rate:.0f} samples/s (the step: {STEP_IMAGES_PER_S} images/s)")
    assert out["image"].shape == (24, 1, 224, 224) and bool(torch.isfinite(out["image"]).all())
    assert rate > STEP_IMAGES_PER_S, rate
