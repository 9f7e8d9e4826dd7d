"""The device-side skin augmentation (data.ComposeAugmenter, csrc/augment_image_ops.hip) where it is used: feeding the training loop
of the skin configuration through DeviceTrainLoader(augmenter=...), and keeping up with that step."""
import copy
import time

import numpy as np
import pytest
import torch

from backend import use_hip
from cenet_amd import data as D

STEP_IMAGES_PER_S = 197  # the skin preset's captured training step (README status table; batch 8, 512 x 512)


def _images(shape, count, seed, dev):
    rng = np.random.default_rng(seed)
    return D.DeviceImages([((rng.random((3, *shape)) * 255).astype(np.float32), rng.integers(0, 2, shape).astype(np.uint8))
                           for _ in range(count)], dev)


@pytest.mark.gpu
def test_replayed_skin_loop_fed_by_the_augmenter_equals_the_eager_loop():
    """train_acdc on the skin configuration (3 input channels, 2 classes, heads 2 / 2 / 2, scales 1.0 / 0.75 / 0.5 as bench.py's
    ham512, at 224 x 224, loss_type boundary), 2 epochs of 2 batches of 4 from DeviceTrainLoader over a ComposeAugmenter: two
    loaders with the same seeds give the same batches, so the captured-graph loop equals the eager loop loss for loss
    (tests/test_train_loop.py's bound for the fp32 step)"""
    from cenet_amd import train
    from cenet_amd.networks import CENet
    dev = use_hip()
    im = _images((224, 224), 8, 3, dev)
    torch.manual_seed(77)
    ref_net = CENet(input_channels=3, num_classes=2, scale_factors=[1.0, 0.75, 0.5], diffatt_num_heads=[2, 2, 2], out_up_block="upcn")
    ref_net.backbone.reset_drop_path(0.0)  # (stochastic depth draws random masks: both loops must see the same network)
    ref_net = ref_net.to(dev)
    runs, firsts = [], []
    for graph in (False, True):
        aug = D.ComposeAugmenter(im, seed=12)
        loader = D.DeviceTrainLoader(im, None, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(31), augmenter=aug)
        h = train.train_acdc(copy.deepcopy(ref_net), loader, num_classes=2, max_epochs=2, base_lr=0.01, loss_type="boundary",
                             loss_weights="1.0", device=dev, graph=graph, log_every=1, log=lambda s: None)
        runs.append(np.array([v for _, v in h["loss"]]))
        firsts.append(aug.picked)
        assert h["optimizer"]._steps == 4
    le, lg = runs
    assert firsts[0] == firsts[1] and any(p for p in firsts[0])  # the same (non-trivial) augmentation decisions
    assert len(le) == len(lg) == 4
    print(f"eager {le}, replayed {lg}")
    assert np.abs(le - lg).max() < 2e-4, (le, lg)
    assert len(set(np.round(le, 4))) > 2  # the batches (and therefore the losses) do change from iteration to iteration


@pytest.mark.gpu
def test_costliest_plan_keeps_up_with_the_skin_step():
    """batch 8, 3 x 512 x 512, EVERY sample rotated (mirror border), blurred with k = 7 and warped elastically with the preset's
    sigma = 50 field (radius 200), then min-max: table upload + the two field passes + stages + min-max must deliver more samples
    per second than the preset's training step consumes"""
    dev = use_hip()
    rng = np.random.default_rng(0)
    im = _images((512, 512), 12, 1, dev)
    aug = D.ComposeAugmenter(im, seed=1)
    idx = [int(i) for i in rng.permutation(12)[:8]]

    def chain():
        a = np.deg2rad(rng.uniform(-30, 30))
        k0, k1 = (int(v) for v in rng.integers(0, 2 ** 32, 2, dtype=np.uint64))
        return [("affine", *D.centred_affine([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], (512, 512)), "mirror"), ("blur", 7),
                ("elastic", 1.0, k0, k1, "mirror")]

    plan = aug.plan(idx, [chain() for _ in idx])
    assert plan[0].shape == (8, 4) and (plan[0][:, 1:] != 0).all() and len(plan[2]) == 201
    for _ in range(3):
        out = aug.apply(plan)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 10
    for _ in range(reps):
        out = aug.apply(plan)
    torch.cuda.synchronize()
    rate = reps * 8 / (time.perf_counter() - t0)
    print(f"costliest plan: {rate:.0f} samples/s (the step: {STEP_IMAGES_PER_S} images/s)")
    assert out["image"].shape == (8, 3, 512, 512) and bool(torch.isfinite(out["image"]).all())
    assert float(out["image"].min()) == 0.0 and float(out["image"].max()) <= 1.0
    assert rate > STEP_IMAGES_PER_S, rate
