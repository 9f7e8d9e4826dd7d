"""Volume inference with both resizes on the device (cenet_amd/evaluate.py: predict_volume, test_single_volume /
synapse_test_single_volume / val_single_volume with resize="device", inference; cenet_amd/train.py: the epoch tail of
main_acdc.py:270-289) against the same calls with resize="host" — scipy.ndimage.zoom on the host, the code the reference runs.

The stand-in networks are pointwise, so every output voxel depends on ONE resized input pixel and the comparison can be exact
about its one loophole: the two predictions may differ in at most 0.1 % of the voxels, and only where the two resized inputs
differ in their float32 value.  On the host checker (`sim`) and on the MI355X no voxel differed when this was written."""
import os

import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

from backend import dev, use_hip  # noqa: F401
from cenet_amd import evaluate, kern


class _ConstNet(torch.nn.Module):
    """logits that depend on the input intensity only (so the resize path decides the result)"""

    def __init__(self, K, lo=0.2, hi=0.8):
        super().__init__()
        self.K, self.lo, self.hi = K, lo, hi
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        levels = torch.linspace(self.lo, self.hi, self.K, device=x.device).view(1, self.K, 1, 1)
        return -(x - levels).abs()


class _Proj(torch.nn.Module):
    """fixed 1x1 projection of the (normalised) slice to K logit maps"""

    def __init__(self, K):
        super().__init__()
        g = torch.Generator().manual_seed(2)
        self.w = torch.nn.Parameter(torch.randn(K, 1, generator=g) * 3)
        self.b = torch.nn.Parameter(torch.randn(K, generator=g))

    def forward(self, x):
        return torch.einsum("kc,bchw->bkhw", self.w.to(x.dtype), x) + self.b.view(1, -1, 1, 1)


def _volume(shape, K, seed):
    """smooth random intensities in [0, 1] and a label volume cut from them (class K - 1 left out of the ground truth)"""
    rng = np.random.default_rng(seed)
    low = rng.random((shape[0], 6, 6))
    image = np.stack([zoom(s, (shape[1] / 6, shape[2] / 6), order=1) for s in low]).astype(np.float32)
    label = np.clip((rng.random(shape) * 0.2 + image * K).astype(np.int64), 0, K - 2).astype(np.float32)
    return torch.from_numpy(image)[None], torch.from_numpy(label)[None]


# ragged: every volume its own slice size; one already has the patch size (no resize, as the reference skips it)
VOLUMES = [((5, 30, 26), 7), ((4, 20, 24), 8), ((3, 58, 63), 9), ((4, 16, 16), 10)]
PATCH = (16, 16)


def _assert_same_prediction(pd, ph, image, patch, dev, normalize=None):
    """the file's condition: <= 0.1 % differing voxels, each of them fed by a resized-input pixel whose float32 values differ"""
    assert pd.shape == ph.shape
    diff = np.argwhere(pd != ph)
    print(f"{tuple(pd.shape)}: {len(diff)} of {pd.size} voxels differ")
    assert len(diff) <= 0.001 * pd.size, (len(diff), pd.size)
    if len(diff) == 0:
        return True
    D, H, W = pd.shape
    vol = image[0].numpy()
    host_in = np.stack([zoom(a, (patch[0] / H, patch[1] / W), order=3) for a in vol])
    dev_in = torch.empty(D, 1, patch[0], patch[1], device=dev)
    kern.vol_resize_cubic(torch.from_numpy(vol).to(dev), torch.empty(D * H * W, dtype=torch.float64, device=dev), dev_in, D, H, W,
                          patch[0], patch[1])
    dev_in = dev_in.cpu().numpy()[:, 0]
    for d, y, x in diff:
        sy = int(np.floor(y * ((patch[0] - 1) / (H - 1)) + 0.5))
        sx = int(np.floor(x * ((patch[1] - 1) / (W - 1)) + 0.5))
        assert host_in[d, sy, sx] != dev_in[d, sy, sx], (d, y, x)
    return False


def _saved_pred(path, case):
    return np.load(os.path.join(path, f"{case}_pred.npy"))


@pytest.mark.parametrize("shape,seed", VOLUMES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_single_volume_device_equals_host(dev, tmp_path, shape, seed):
    K = 4
    image, label = _volume(shape, K, seed)
    net = _ConstNet(K).to(dev)
    out = {}
    for mode in ("host", "device"):
        m = evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=2, device=dev, resize=mode,
                                        test_save_path=str(tmp_path / mode), case="c0", z_spacing=2.5)
        out[mode] = (m, _saved_pred(tmp_path / mode, "c0"))
        assert open(tmp_path / mode / "c0_spacing.txt").read() == "1 1 2.5\n"
        assert np.array_equal(np.load(tmp_path / mode / "c0_gt.npy"), label[0].numpy())
        assert np.array_equal(np.load(tmp_path / mode / "c0_img.npy"), image[0].numpy())
    assert len(out["device"][0]) == K - 1 and all(len(t) == 4 for t in out["device"][0])
    if _assert_same_prediction(out["device"][1], out["host"][1], image, PATCH, dev):
        for a, b in zip(out["device"][0], out["host"][0]):
            assert all(abs(u - v) < 1e-12 for u, v in zip(a, b)), (a, b)
    # predict_volume is the same prediction, and it stays on the device
    pred, counts = evaluate.predict_volume(net, image[0].to(dev), PATCH, batch_slices=3)
    assert counts is None and pred.device.type == dev.type and pred.dtype == torch.float32
    assert np.array_equal(pred.cpu().numpy(), out["device"][1])
    # ndarray inputs [D, H, W] as the host path takes them
    m = evaluate.test_single_volume(image[0].numpy(), label[0].numpy(), net, K, patch_size=PATCH, device=dev, resize="device")
    assert m == out["device"][0]


@pytest.mark.parametrize("shape,seed", VOLUMES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_synapse_volume_device_equals_host(dev, tmp_path, shape, seed):
    K = 5
    image, label = _volume(shape, K, seed + 20)
    net = _Proj(K).to(dev)
    out = {}
    for mode in ("host", "device"):
        m = evaluate.synapse_test_single_volume(image, label, net, K, patch_size=PATCH, test_save_path=str(tmp_path / mode),
                                                case="s0", batch_slices=2, device=dev, resize=mode)
        out[mode] = (m, _saved_pred(tmp_path / mode, "s0"))
    assert len(out["device"][0]) == K - 1 and all(len(t) == 2 for t in out["device"][0])
    assert len(np.unique(out["host"][1])) > 2  # the projection really separates classes on this input
    if _assert_same_prediction(out["device"][1], out["host"][1], image, PATCH, dev):
        for a, b in zip(out["device"][0], out["host"][0]):
            assert all(abs(u - v) < 1e-12 for u, v in zip(a, b)), (a, b)


def test_synapse_2d_branch_is_the_same_in_both_modes(dev, tmp_path):
    K = 4
    g = torch.Generator().manual_seed(3)
    image, label = torch.rand(1, 20, 24, generator=g), torch.randint(0, K, (1, 20, 24), generator=g).float()
    net = _Proj(K).to(dev)
    a = evaluate.synapse_test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="host")
    b = evaluate.synapse_test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="device",
                                            test_save_path=str(tmp_path), case="flat")
    assert a == b and _saved_pred(tmp_path, "flat").shape == (20, 24)


def test_length_one_axis_goes_the_host_way(dev):
    """scipy special-cases length-1 axes and the kernels refuse them: resize="device" must give the host result, not fail"""
    K = 3
    image, label = _volume((3, 1, 24), K, 5)
    net = _ConstNet(K).to(dev)
    a = evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="host")
    b = evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="device")
    assert a == b


@pytest.mark.parametrize("shape,seed", VOLUMES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_val_single_volume(dev, tmp_path, shape, seed):
    """Dice per class from the counts fused into the argmax + resize-back kernel: equal to the host mode, and to
    calculate_dice_percase (metrics_eval.py:24-34) applied to the host prediction"""
    K = 4
    image, label = _volume(shape, K, seed + 40)
    net = _ConstNet(K).to(dev)
    got = evaluate.val_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=2, device=dev)  # device is the default
    host = evaluate.val_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=2, device=dev, resize="host")
    evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="host", test_save_path=str(tmp_path),
                                case="v")
    ph = _saved_pred(tmp_path, "v")
    lab = label[0].numpy()
    want = []
    for c in range(1, K):
        p, t = ph == c, lab == c
        want.append(2.0 * (p & t).sum() / (p.sum() + t.sum()) if p.sum() > 0 and t.sum() > 0 else (1.0 if p.sum() > 0 else 0.0))
    assert want[K - 2] in (0.0, 1.0)  # class K - 1 is absent from the ground truth: the wrapper rules are exercised
    assert len(host) == K - 1 and all(abs(a - b) < 1e-12 for a, b in zip(host, want))
    pd, _ = evaluate.predict_volume(net, image[0].to(dev), PATCH, batch_slices=2)
    if _assert_same_prediction(pd.cpu().numpy(), ph, image, PATCH, dev):
        assert len(got) == K - 1 and all(abs(a - b) < 1e-12 for a, b in zip(got, want)), (got, want)


def test_predict_volume_counts_are_predict_counts_of_the_prediction(dev):
    K = 4
    image, label = _volume((5, 30, 26), K, 3)
    net = _ConstNet(K).to(dev)
    whole, cw = evaluate.predict_volume(net, image[0].to(dev), PATCH, batch_slices=5, labels=label[0].to(dev))
    parts, cp = evaluate.predict_volume(net, image[0].to(dev), PATCH, batch_slices=2, labels=label[0].to(dev))
    assert torch.equal(whole, parts) and torch.equal(cw, cp) and cw.dtype == torch.int64 and tuple(cw.shape) == (K + 1, 3)
    p, t = whole.cpu(), label[0]
    for k in range(K):
        assert cw[k].tolist() == [int(((p == k) & (t == k)).sum()), int((p == k).sum()), int((t == k).sum())]
    assert cw[K].tolist() == [int(((p > 0) & (t > 0)).sum()), int((p > 0).sum()), int((t > 0).sum())]


def test_inference_is_the_mean_over_cases_then_classes(dev, tmp_path):
    K = 4
    net = _ConstNet(K).to(dev)
    cases = []
    for i, (shape, seed) in enumerate(VOLUMES[:3]):
        image, label = _volume(shape, K, seed + 60)
        cases.append({"image": image, "label": label, "case_name": [f"case{i}"] if i else "case0"})  # DataLoader list or str
    lines = []
    dice, hd = evaluate.inference(net, cases, K, patch_size=PATCH, z_spacing=3, test_save_path=str(tmp_path), log=lines.append)
    per_case = [np.array(evaluate.test_single_volume(c["image"], c["label"], net, K, patch_size=PATCH, device=dev, resize="device"))
                for c in cases]
    table = sum(per_case) / len(per_case)  # [K - 1, 4]: mean over the cases first ...
    assert abs(dice - np.mean(table, axis=0)[0]) < 1e-12 and abs(hd - np.mean(table, axis=0)[1]) < 1e-12  # ... then the classes
    assert isinstance(dice, float) and isinstance(hd, float)
    assert len(lines) == 3 + (K - 1) + 1
    assert lines[1].startswith("idx 1 case case1 mean_dice %f mean_hd95 %f" % tuple(np.mean(per_case[1], axis=0)[:2]))
    assert lines[3].startswith("Mean class (1) mean_dice %f" % table[0][0])
    assert lines[-1] == "Testing performance in best val model) mean_dice:%f mean_hd95:%f" % (dice, hd)
    assert all(os.path.exists(tmp_path / f"case{i}_pred.npy") for i in range(3))
    # resize="host" goes through the same table
    dh, hh = evaluate.inference(net, cases, K, patch_size=PATCH, log=lambda s: None, resize="host")
    host_case = [np.array(evaluate.test_single_volume(c["image"], c["label"], net, K, patch_size=PATCH, device=dev)) for c in cases]
    assert abs(dh - np.mean(sum(host_case) / 3, axis=0)[0]) < 1e-12 and abs(hh - np.mean(sum(host_case) / 3, axis=0)[1]) < 1e-12


# ---- GPU only ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_predict_volume_makes_no_host_round_trip(monkeypatch):
    """under torch's sync-debug mode every synchronising call raises (a .cpu(), .item(), .numpy() of a device tensor, a blocking
    copy): predict_volume — resize in, forward, argmax + resize back, counts — makes none.  Tensor.cpu / .numpy / .tolist / .item
    are patched to raise as well, so that a host round trip cannot come back unnoticed either way."""
    d = use_hip()
    K = 4
    image, label = _volume((40, 256, 216), K, 11)
    vol, lab = image[0].to(d), label[0].to(d)
    net = _Proj(K).to(d)
    evaluate.predict_volume(net, vol[:2], (224, 224), labels=lab[:2])  # (first use loads the library and warms the allocator)
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("host round trip inside predict_volume")

    for name in ("cpu", "numpy", "tolist", "item"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pred, counts = evaluate.predict_volume(net, vol, (224, 224), batch_slices=32, normalize=(0.5, 0.5), labels=lab)
    finally:
        torch.cuda.set_sync_debug_mode(old)
        monkeypatch.undo()
    torch.cuda.synchronize()
    assert pred.is_cuda and counts.is_cuda and tuple(pred.shape) == (40, 256, 216)
    assert int(counts[:K, 1].sum()) == pred.numel()


def _acdc_net(d):
    from cenet_amd.networks import CENet
    from oracle import cenet_oracle as O
    from oracle.golden_cases import MODEL_CONFIGS, config_from_kwargs
    kw = MODEL_CONFIGS["acdc"]["kw"]
    net = CENet(**kw)
    net.load_state_dict(O.make_state_dict(config_from_kwargs(kw), seed=42), strict=True)
    return net.to(d).eval()


@pytest.mark.gpu
def test_real_cenet_volume_device_resize():
    """ACDC preset, fp32: both procedures are fed the SAME resized input (the device resize's), so the comparison isolates the
    argmax + resize back on real logits: identical predictions.  Then the whole resize="device" call in fp32 and in bf16 mode."""
    from cenet_amd import ops
    d = use_hip()
    net = _acdc_net(d)
    K, D, H, W, P = 4, 6, 256, 216, 224
    image, label = _volume((D, H, W), K, 13)
    vol = image[0].to(d)
    inp = torch.empty(D, 1, P, P, device=d)
    kern.vol_resize_cubic(vol, torch.empty(D * H * W, dtype=torch.float64, device=d), inp, D, H, W, P, P)
    with torch.no_grad(), ops.batch1_semantics():
        logits = net(inp).contiguous()
    # host procedure on these logits (metrics_eval.py:52-58)
    out = torch.argmax(torch.softmax(logits, dim=1), dim=1).cpu().numpy()
    want = np.stack([zoom(o, (H / P, W / P), order=0) for o in out])
    pred = torch.empty(D, H, W, device=d)
    kern.argmax_resize_counts(logits, None, pred, None, D, K, P, P, H, W)
    assert np.array_equal(pred.cpu().numpy(), want.astype(np.float32))
    assert len(np.unique(want)) > 1
    for bf16 in (False, True):
        old = kern.set_compute_bf16(bf16)
        try:
            m = evaluate.test_single_volume(image, label, net, K, patch_size=(P, P), batch_slices=4, device=d, resize="device")
            v = evaluate.val_single_volume(image, label, net, K, patch_size=(P, P), batch_slices=4, device=d)
        finally:
            kern.set_compute_bf16(old)
        assert len(m) == K - 1 and all(len(t) == 4 and all(np.isfinite(t)) for t in m), m
        assert len(v) == K - 1 and all(0.0 <= x <= 1.0 for x in v), v


@pytest.mark.gpu
def test_train_loop_epoch_tail_follows_main_acdc(tmp_path, monkeypatch):
    """main_acdc.py:270-289 with stubbed validation / test results:
        epoch 0: val 0.50 >= 0    -> test 0.40 >= 0    -> bests (0.50, 0.40), best.pth
        epoch 1: val 0.60 >= 0.50 -> test 0.30 <  0.40 -> NEITHER best moves (the reference's quirk), no save
        epoch 2: val 0.55 >= 0.50 -> test 0.45 >= 0.40 -> best.pth again (0.55 < 0.60 would have skipped the test run had epoch 1
                                                          moved the validation best)
    and the last epoch writes epoch=2_lr=..._avg_dcs=0.45.pth."""
    from cenet_amd import checkpoint, train
    from cenet_amd.networks import CENet
    from oracle import cenet_oracle as O
    d = use_hip()
    torch.manual_seed(77)
    net = CENet(input_channels=1, num_classes=4, scale_factors=[1.0, 0.5], diffatt_num_heads=[4, 4, 4], out_up_block="upcn")
    net.backbone.reset_drop_path(0.0)
    x, lab = O.synthetic_batch(2, 1, 4, seed=21)
    loader = [{"image": x, "label": lab.long()}]
    vals, tests = iter([0.50, 0.60, 0.55]), iter([(0.40, 9.0), (0.30, 8.0), (0.45, 7.0)])
    calls = []
    monkeypatch.setattr(evaluate, "validate", lambda net, batches: next(vals))

    def fake_inference(net, volumes, classes, **kw):
        calls.append((list(volumes), classes, kw["patch_size"], kw["resize"]))
        return next(tests)

    monkeypatch.setattr(evaluate, "inference", fake_inference)
    saved = []
    real_save = checkpoint.save_weights
    monkeypatch.setattr(checkpoint, "save_weights", lambda n, p: (saved.append(os.path.basename(p)), real_save(n, p)))
    h = train.train_acdc(net, loader, max_epochs=3, base_lr=0.01, device=d, graph=False, val_batches=lambda: [], log_every=1,
                         log=lambda s: None, test_volumes=lambda: ["vol"], save_dir=str(tmp_path))
    assert h["val_dice"] == [0.50, 0.60, 0.55] and h["test_dice"] == [0.40, 0.30, 0.45] and h["test_hd95"] == [9.0, 8.0, 7.0]
    assert h["best_epochs"] == [0, 2]
    assert calls == [(["vol"], 4, (224, 224), "device")] * 3
    last = f"epoch=2_lr={h['lr'][-1]}_avg_dcs=0.45.pth"
    assert saved == ["best.pth", "best.pth", last]
    assert sorted(os.listdir(tmp_path)) == sorted(["best.pth", last])
    sd = torch.load(tmp_path / "best.pth", map_location="cpu", weights_only=True)
    assert set(sd) == set(net.state_dict()) and all(torch.equal(v, net.state_dict()[k].cpu()) for k, v in sd.items())
    # without the new arguments: today's keys, nothing written
    h0 = train.train_acdc(net, loader, max_epochs=1, base_lr=0.01, device=d, graph=False, log=lambda s: None)
    assert set(h0) == {"loss", "epoch_loss", "val_dice", "lr", "arena", "optimizer"}
    with pytest.raises(ValueError):
        train.train_acdc(net, loader, max_epochs=1, device=d, graph=False, test_volumes=lambda: [])
