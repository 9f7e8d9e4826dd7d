"""Flip / rotate test-time augmentation (csrc/tta.hip through kern.tta_views / kern.tta_argmax_resize_counts, evaluate.tta_predict,
evaluate.predict_volume(tta=...) and the wrappers' `tta=`).  The views are held to their numpy definition bit for bit, the fused
merge (un-view, softmax, mean over the views, argmax, order-0 resize, counts) to a float64 numpy / scipy reference.  `sim` runs the
kernel sources on the host SIMT checker, `hip` (marker gpu) the gfx950 kernels.

The two bounds (conf within 1e-6; predictions equal except at near-ties of the reference, at most 0.1 % of a case) are in
tests/tta_ref.py with their derivation."""
import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

from backend import dev  # noqa: F401
from cenet_amd import evaluate, kern
from tta_ref import CONF_TOL, view_codes, hold_to_reference, reference, smooth_volume, unview, view

# ---- 1. views -----------------------------------------------------------------------------------------------------------------------
def _views(x, mask, dev):
    n, C, PH, PW = x.shape
    T = len(view_codes(mask))
    out = torch.full((T, n, C, PH, PW), float("nan"), device=dev)
    kern.tta_views(torch.from_numpy(x).to(dev), out, n, C, PH, PW, mask)
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("shape,masks", [((2, 3, 7, 7), [1 << g for g in range(8)] + [0xFF, 0xA5]),
                                         ((1, 1, 5, 9), [1, 2, 8, 0x0F, 0x10, 0xFF]),  # the transposed views are refused at this shape
                                         ((1, 2, 40, 40), [0xFF]),   # 2 x 2 tiles, the last ones 8 wide
                                         ((2, 1, 33, 70), [0x0F])],  # 2 x 3 tiles of a rectangular plane
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_views_are_the_numpy_views_bit_for_bit(dev, shape, masks):
    x = np.random.default_rng(shape[-1]).standard_normal(shape).astype(np.float32)
    x[0, 0, 0, 0], x[0, 0, 0, 1], x[0, 0, 1, 0] = np.float32("nan"), -0.0, np.float32("inf")  # bit copies, not arithmetic
    for mask in masks:
        if mask & 0xF0 and shape[2] != shape[3]:
            with pytest.raises(RuntimeError, match="cenet_tta_views_f32"):
                _views(x, mask, dev)
            continue
        got = _views(x, mask, dev)
        for t, g in enumerate(view_codes(mask)):
            assert np.array_equal(_bits(got[t]), _bits(view(x, g))), (mask, g)
    assert np.array_equal(_bits(unview(view(x, 5), 5)), _bits(x)) and np.array_equal(_bits(unview(view(x, 6), 6)), _bits(x))


# ---- 2. merge against float64 ----------------------------------------------------------------------------------------------------
CASES = [(0x07, 2, 4, (16, 16), (30, 26)), (0xFF, 1, 9, (16, 16), (58, 63)), (0xFF, 3, 16, (17, 17), (17, 17)),
         (0x0F, 2, 2, (12, 20), (9, 33)), (0x01, 1, 1, (8, 8), (8, 8)), (0xA5, 2, 5, (16, 16), (8, 40)),
         (0x0F, 1, 3, (16, 16), (59, 30))]
# sizes whose last zoom coordinate rounds above 15, so that scipy writes cval there: (last row, last column) are zeroed
ZEROED = {(30, 26): (True, False), (59, 30): (True, True), (58, 63): (False, False)}


def _merge(stacks, labels, mask, n, K, patch, size, dev, conf=True, counts=None):
    pred = torch.full((n,) + tuple(size), -1.0, device=dev)
    cf = torch.full((n,) + tuple(size), -1.0, device=dev) if conf else None
    if labels is not None and counts is None:
        counts = torch.full((K + 1, 3), -7, dtype=torch.int32, device=dev)
    kern.tta_argmax_resize_counts(stacks.to(dev), None if labels is None else labels.to(dev), pred, cf, counts, n, K, patch[0],
                                  patch[1], size[0], size[1], mask)
    return pred.cpu().numpy(), None if cf is None else cf.cpu().numpy(), counts


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mask,n,K,patch,size", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_merge_against_float64_reference(dev, mask, n, K, patch, size, bf16):
    """Observed (printed by every case): the largest conf error over the fourteen cases is 1.33e-7 on the host checker and 1.33e-7
    on the MI355X (mask 0x07, bf16 logits; fp32 logits: 1.04e-7 on both); no case has a voxel under the gap bound on either
    backend, and no voxel differs from the reference."""
    T = len(view_codes(mask))
    g = torch.Generator().manual_seed(1000 * mask + 10 * K + n)
    stacks = torch.randn(T, n, K, patch[0], patch[1], generator=g) * 3
    if bf16:
        stacks = stacks.bfloat16()  # the reference is computed from the rounded values
    labels = torch.randint(-1, K + 1, (n,) + tuple(size), generator=g).float()  # (a class outside [0, K) at both ends)
    want_pred, want_conf, gap = reference(stacks.float().numpy(), mask, size)
    if size in ZEROED:  # the cval rule really is exercised
        assert (bool((want_conf[:, -1] == 0).all()), bool((want_conf[:, :, -1] == 0).all())) == ZEROED[size]
    pred, conf, counts = _merge(stacks, labels, mask, n, K, patch, size, dev)
    hold_to_reference(f"mask {mask:#04x} n={n} K={K} {patch}->{size} {'bf16' if bf16 else 'fp32'}", pred, conf, want_pred,
                       want_conf, gap)
    if K > 1:  # beyond the last source pixel: class 0, conf exactly 0
        assert (conf[np.isinf(gap)] == 0).all() and (pred[np.isinf(gap)] == 0).all()
    # the counts are those of the kernel's own prediction
    p, t, c = torch.from_numpy(pred), labels, counts.cpu()
    for k in range(K):
        assert c[k].tolist() == [int(((p == k) & (t == k)).sum()), int((p == k).sum()), int((t == k).sum())]
    assert c[K].tolist() == [int(((p > 0) & (t > 0)).sum()), int((p > 0).sum()), int((t > 0).sum())]
    # without labels (and without conf): the same prediction, the count table is left alone
    keep = torch.full((K + 1, 3), -7, dtype=torch.int32, device=dev)
    pred2, none, _ = _merge(stacks, None, mask, n, K, patch, size, dev, conf=False, counts=keep)
    assert none is None and np.array_equal(pred2, pred) and (keep == -7).all()


def test_merge_of_one_view_is_argmax_resize_counts(dev):
    """T = 1, the identity: the class map of the existing kernel (a softmax keeps the order of the logits it is given)"""
    n, K, patch, size = 2, 4, (16, 16), (30, 26)
    logits = torch.randn(1, n, K, *patch, generator=torch.Generator().manual_seed(3)) * 3
    pred, _, _ = _merge(logits, None, 0x01, n, K, patch, size, dev)
    want = torch.empty((n,) + size, device=dev)
    kern.argmax_resize_counts(logits[0].contiguous().to(dev), None, want, None, n, K, patch[0], patch[1], size[0], size[1])
    assert np.array_equal(pred, want.cpu().numpy())


# ---- 3. orientation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,patch", [(0xFF, (16, 16)), (0xA5, (16, 16)), (0x0F, (12, 20)), (0x60, (9, 9))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else hex(v))
def test_every_view_maps_back_onto_the_same_pixel(dev, mask, patch):
    """class 0 is the background (logit 40 everywhere, in every view); view slot t carries logit 80 for class t + 1 at the ONE pixel
    where the marker pixel (2, 5) — which no non-trivial element of D4 fixes — lies in that view.  Merged, every marker falls
    on (2, 5): there class 0 gets nothing, the T marker classes 1 / T each (class 1 wins, conf 1 / T); everywhere else class 0
    has probability 1.  A marker that lands elsewhere (a swapped flip order, a wrong inverse of the views 5 and 6) leaves conf
    (T - 1) / T there, and a tie with class 0 at (2, 5)."""
    codes = view_codes(mask)
    T, K = len(codes), len(codes) + 1
    marker = np.zeros(patch, dtype=np.float32)
    marker[2, 5] = 1.0
    stacks = np.zeros((T, 1, K) + patch, dtype=np.float32)
    stacks[:, 0, 0] = 40.0
    for t, g in enumerate(codes):
        stacks[t, 0, t + 1] = 80.0 * view(marker, g)
    pred, conf, _ = _merge(torch.from_numpy(stacks), None, mask, 1, K, patch, patch, dev)
    want = np.zeros((1,) + patch, dtype=np.float32)
    want[0, 2, 5] = 1.0
    assert np.array_equal(pred, want)
    assert abs(conf[0, 2, 5] - 1.0 / T) <= CONF_TOL
    assert (np.abs(np.delete(conf.ravel(), 2 * patch[1] + 5) - 1.0) <= CONF_TOL).all()


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,K", [(0x07, 4), (0x0F, 2), (0xFF, 4), (0x07, 5), (0xFF, 16)])
def test_equal_logits_give_class_zero(dev, mask, K):
    T = len(view_codes(mask))
    stacks = torch.full((T, 2, K, 16, 16), 0.75)
    pred, conf, _ = _merge(stacks, None, mask, 2, K, (16, 16), (20, 24), dev)
    assert (pred == 0).all()
    if K & (K - 1) == 0:  # 1 / K, its multiples up to T / K and the product with float(1 / T) are exact (or round back) in binary
        assert (conf == np.float32(1.0) / np.float32(K)).all()
    else:
        assert (np.abs(conf - 1.0 / K) <= CONF_TOL).all()


def test_classes_tied_across_views_give_the_lower_index(dev):
    """view 0 prefers class 1 over class 3 by exactly what view 1 prefers class 3 over class 1: the two sums are the same two floats
    added in either order, equal to the bit, and the first maximum is class 1"""
    stacks = torch.full((2, 1, 4, 16, 16), -30.0)
    stacks[0, 0, 1], stacks[0, 0, 3] = 2.0, 1.0
    stacks[1, 0, 1], stacks[1, 0, 3] = 1.0, 2.0
    pred, conf, _ = _merge(stacks, None, 0x03, 1, 4, (16, 16), (16, 16), dev)
    assert (pred == 1).all() and (np.abs(conf - 0.5) <= CONF_TOL).all()
    stacks[1, 0, 3] = 2.0 + 2.0 ** -10  # (and the slightest lead of class 3 is seen)
    pred, _, _ = _merge(stacks, None, 0x03, 1, 4, (16, 16), (16, 16), dev)
    assert (pred == 3).all()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    ENTRY = "cenet_tta_argmax_resize_counts"

    def call(mask=0x07, K=4, patch=(16, 16), size=(16, 16), labels=False, counts=False):
        T = len(view_codes(mask)) if 1 <= mask <= 255 else 1
        kern.tta_argmax_resize_counts(torch.zeros(T, 1, K, *patch, device=dev),
                                      torch.zeros(1, *size, device=dev) if labels else None, torch.empty(1, *size, device=dev), None,
                                      torch.zeros(K + 1, 3, dtype=torch.int32, device=dev) if counts else None, 1, K, patch[0],
                                      patch[1], size[0], size[1], mask)

    call(labels=True, counts=True)  # (the arguments below are refused for the reason named, not for a slip of this helper)
    call(mask=0x10)
    for kw in (dict(mask=0), dict(mask=256), dict(mask=0x10, patch=(12, 20), size=(12, 20)), dict(mask=0xFF, patch=(12, 20)),
               dict(K=17), dict(size=(1, 20)), dict(patch=(16, 1)), dict(labels=True)):
        with pytest.raises(RuntimeError, match=ENTRY):
            call(**kw)
    for mask, shape in ((0, (12, 12)), (256, (12, 12)), (0x20, (12, 20))):
        with pytest.raises(RuntimeError, match="cenet_tta_views_f32"):
            kern.tta_views(torch.zeros(1, 1, *shape, device=dev), torch.empty(1, 1, 1, *shape, device=dev), 1, 1, shape[0], shape[1],
                           mask)
    # the Python layer: names, tuples, the patch size in the message
    assert kern.tta_view_mask("flips") == (0x07, 3) and kern.tta_view_mask("flips4") == (0x0F, 4)
    assert kern.tta_view_mask("d4") == (0xFF, 8) and kern.tta_view_mask((7, 0, 5, 0)) == (0xA1, 3)
    assert evaluate.TTA_SETS == {"flips": 0x07, "flips4": 0x0F, "d4": 0xFF}
    for bad in ("rot", (), (8,), (0, -1), 3, (1.0,)):
        with pytest.raises(ValueError, match="tta"):
            kern.tta_view_mask(bad)
    with pytest.raises(ValueError, match=r"\(12, 20\)"):
        evaluate.tta_predict(torch.nn.Identity(), torch.zeros(1, 2, 12, 20, device=dev), "d4")
    with pytest.raises(ValueError, match=r"\(12, 20\)"):
        evaluate.predict_volume(torch.nn.Identity(), torch.zeros(2, 30, 26, device=dev), (12, 20), tta=(0, 4))


# ---- 6. predict_volume(tta=...) ------------------------------------------------------------------------------------------------------
class _RampNet(torch.nn.Module):
    """not D4-equivariant: pointwise in the intensity (as _Proj of test_volume_inference.py) plus a fixed ramp per class that
    differs along y, along x and under a transpose.  Element-wise only, so a pixel's logits do not depend on the batch it is in."""

    def __init__(self, K, patch, cin=1):
        super().__init__()
        g = torch.Generator().manual_seed(2)
        self.w = torch.nn.Parameter(torch.randn(K, cin, generator=g) * 3)
        self.b = torch.nn.Parameter(torch.randn(K, generator=g))
        yy = torch.linspace(0, 1, patch[0]).view(1, -1, 1)
        xx = torch.linspace(0, 1, patch[1]).view(1, 1, -1)
        a = torch.randn(3, K, 1, 1, generator=g)
        self.register_buffer("ramp", a[0] * yy + a[1] * xx * xx + a[2] * yy * yy * xx)

    def forward(self, x):
        out = self.b.view(1, -1, 1, 1) + self.ramp
        for c in range(x.shape[1]):
            out = out + x[:, c:c + 1] * self.w[:, c].view(1, -1, 1, 1)
        return out


def _volume_reference(net, vol, patch, mask, dev):
    """the recipe of test 2 on the stand-in's logits for numpy-made views of the DEVICE-resized input"""
    D, H, W = vol.shape
    if (H, W) != tuple(patch):
        inp = torch.empty(D, 1, patch[0], patch[1], device=dev)
        kern.vol_resize_cubic(torch.from_numpy(vol).to(dev), torch.empty(D * H * W, dtype=torch.float64, device=dev), inp, D, H, W,
                              patch[0], patch[1])
        inp = inp.cpu().numpy()
    else:
        inp = vol[:, None]
    with torch.no_grad():
        stacks = np.stack([net(torch.from_numpy(np.ascontiguousarray(view(inp, g))).to(dev)).cpu().numpy() for g in view_codes(mask)])
    return reference(stacks, mask, (H, W))


PATCH = (16, 16)


@pytest.mark.parametrize("tta", ["flips", "d4"])
@pytest.mark.parametrize("shape", [(5, 30, 26), (3, 58, 63), (4, 16, 16)], ids=lambda v: "x".join(map(str, v)))
def test_predict_volume_with_tta(dev, shape, tta):
    """Observed: conf within 1.38e-7 of the reference on the host checker and on the MI355X (5 x 30 x 26, flips), no voxel under
    the gap bound, none differing."""
    K = 4
    vol = smooth_volume(shape, shape[1])
    net = _RampNet(K, PATCH).to(dev)
    mask = evaluate.TTA_SETS[tta]
    want_pred, want_conf, gap = _volume_reference(net, vol, PATCH, mask, dev)
    assert len(np.unique(want_pred)) > 1
    labels = torch.from_numpy(np.clip((vol * K).astype(np.int64), 0, K - 2).astype(np.float32))
    out = []
    for bs in (4, 32):
        conf = torch.full(shape, -1.0, device=dev)
        pred, counts = evaluate.predict_volume(net, torch.from_numpy(vol).to(dev), PATCH, batch_slices=bs, labels=labels.to(dev),
                                               tta=tta, conf_out=conf)
        assert pred.device.type == dev.type and counts.dtype == torch.int64 and tuple(counts.shape) == (K + 1, 3)
        out.append((pred.cpu(), conf.cpu(), counts.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*out))  # the chunking does not show: bit-identical
    pred, conf, counts = out[0]
    hold_to_reference(f"{shape} {tta}", pred.numpy(), conf.numpy(), want_pred, want_conf, gap)
    for k in range(K):
        assert counts[k].tolist() == [int(((pred == k) & (labels == k)).sum()), int((pred == k).sum()), int((labels == k).sum())]
    # the views matter to this network: the plain prediction is another one
    plain, _ = evaluate.predict_volume(net, torch.from_numpy(vol).to(dev), PATCH)
    assert not torch.equal(plain.cpu(), pred)


# ---- 7. wrappers -----------------------------------------------------------------------------------------------------------------------
def _case(shape, K, seed):
    vol = smooth_volume(shape, seed)
    label = np.clip((vol * K).astype(np.int64), 0, K - 2).astype(np.float32)
    return torch.from_numpy(vol)[None], torch.from_numpy(label)[None]


def test_volume_wrappers_score_the_tta_prediction(dev):
    K = 4
    image, label = _case((5, 30, 26), K, 21)
    net = _RampNet(K, PATCH).to(dev)
    pred, counts = evaluate.predict_volume(net, image[0].to(dev), PATCH, batch_slices=4, labels=label[0].to(dev), tta="flips")
    m = evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=4, device=dev, resize="device", tta="flips")
    assert m == evaluate.label_metrics(pred, label[0].to(dev), K, "acdc")
    v = evaluate.val_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=4, device=dev, tta="flips")
    assert v == evaluate.class_dice(counts)[:K - 1]
    s = evaluate.synapse_test_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=4, device=dev, resize="device",
                                            tta=(0, 1, 2))
    ps, _ = evaluate.predict_volume(net, image[0].to(dev), PATCH, normalize=(0.5, 0.5), tta="flips")
    assert s == evaluate.label_metrics(ps, label[0].to(dev), K, "synapse")
    # tta before postprocess: the filter sees the merged prediction
    mp = evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="device", tta="flips",
                                     postprocess="lcc")
    assert mp == evaluate.label_metrics(evaluate.keep_largest_component(pred, K)[0], label[0].to(dev), K, "acdc")
    # tta=None is the call without the argument, to the bit
    a, ca = evaluate.predict_volume(net, image[0].to(dev), PATCH, batch_slices=2, labels=label[0].to(dev))
    b, cb = evaluate.predict_volume(net, image[0].to(dev), PATCH, batch_slices=2, labels=label[0].to(dev), tta=None, conf_out=None)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    assert evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="device", tta=None) == \
        evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="device")


def test_inference_forwards_tta(dev, monkeypatch):
    seen = []

    def fake(image, label, net, classes, **kw):
        seen.append(kw)
        return [(0.5, 1.0, 0.25, 2.0)] * (classes - 1)

    monkeypatch.setattr(evaluate, "test_single_volume", fake)
    cases = [{"image": None, "label": None, "case_name": "c0"}]
    net = _RampNet(4, PATCH).to(dev)
    evaluate.inference(net, cases, 4, patch_size=PATCH, log=lambda s: None, tta="d4")
    evaluate.inference(net, cases, 4, patch_size=PATCH, log=lambda s: None, tta=(0, 3), postprocess="lcc")
    evaluate.inference(net, cases, 4, patch_size=PATCH, log=lambda s: None)
    assert seen[0]["tta"] == "d4" and seen[0]["resize"] == "device" and "postprocess" not in seen[0]
    assert seen[1]["tta"] == (0, 3) and seen[1]["postprocess"] == "lcc"
    assert "tta" not in seen[2]


def test_train_acdc_checks_test_tta():
    """(refused before the device is touched; the forwarding itself is in tests/test_tta_gpu.py)"""
    from cenet_amd import train
    net = _RampNet(4, PATCH)
    with pytest.raises(ValueError, match="test_tta"):
        train.train_acdc(net, [], val_batches=lambda: [], test_volumes=lambda: [], test_tta="flips", test_resize="host")
    with pytest.raises(ValueError, match="tta"):
        train.train_acdc(net, [], val_batches=lambda: [], test_volumes=lambda: [], test_tta="rot")


def test_skin_wrappers_go_through_tta_predict(dev):
    K = 2
    g = torch.Generator().manual_seed(12)
    net = _RampNet(K, (12, 12), cin=3).to(dev)
    loader = [{"image": torch.rand(1, 3, 12, 12, generator=g), "label": (torch.rand(1, 1, 12, 12, generator=g) > 0.5).float()}
              for _ in range(2)]
    dc, acc, iou = evaluate.skin_test(net, loader, device=dev, tta="d4")
    dcs, correct, ious = [], 0, []
    for batch in loader:
        pred, conf, counts = evaluate.tta_predict(net, batch["image"].to(dev), "d4")
        assert counts is None and tuple(pred.shape) == (1, 12, 12) and tuple(conf.shape) == (1, 12, 12)
        p, t = pred[0].cpu() > 0.5, batch["label"][0, 0] > 0.5
        dcs.append(2.0 * int((p & t).sum()) / (int(p.sum()) + int(t.sum())))
        correct += int((pred[0].cpu() == batch["label"][0, 0]).sum())
        ious.append(int((p & t).sum()) / int((p | t).sum()))
    assert 0 < sum(ious) and (dc, acc, iou) == (sum(dcs) / 2, correct / 288, float(np.mean(ious)))
    assert evaluate.skin_val(net, loader, device=dev, tta="d4") == dc
    assert (dc, acc, iou) != evaluate.skin_test(net, loader, device=dev)  # (this network is not D4-equivariant)
    assert evaluate.skin_test(net, loader, device=dev, tta=None) == evaluate.skin_test(net, loader, device=dev)
    # tta_predict with labels: the counts of its own prediction, as predict_counts lays them out
    lab = loader[0]["label"].to(dev)
    pred, _, counts = evaluate.tta_predict(net, loader[0]["image"].to(dev), "flips", labels=lab)
    p, t = pred.cpu(), loader[0]["label"][:, 0]
    assert counts.dtype == torch.int32 and counts.cpu()[1].tolist() == [int(((p == 1) & (t == 1)).sum()), int((p == 1).sum()),
                                                                        int((t == 1).sum())]


def test_tta_is_never_silently_ignored(dev):
    K = 4
    image, label = _case((3, 30, 26), K, 5)
    net = _RampNet(K, PATCH).to(dev)
    with pytest.raises(ValueError, match="tta.*resize"):
        evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, tta="flips")  # resize="host" is the default
    with pytest.raises(ValueError, match="tta.*resize"):
        evaluate.val_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="host", tta="flips")
    with pytest.raises(ValueError, match="tta.*resize"):
        evaluate.synapse_test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, tta="flips")
    thin_i, thin_l = _case((3, 1, 24), K, 6)  # an axis of length 1: the host route
    with pytest.raises(ValueError, match="tta"):
        evaluate.test_single_volume(thin_i, thin_l, net, K, patch_size=PATCH, device=dev, resize="device", tta="flips")
    with pytest.raises(ValueError, match="tta"):
        evaluate.val_single_volume(thin_i, thin_l, net, K, patch_size=PATCH, device=dev, tta="flips")
    flat_i, flat_l = torch.rand(1, 20, 24), torch.zeros(1, 20, 24)  # the Synapse 2-D branch
    with pytest.raises(ValueError, match="tta"):
        evaluate.synapse_test_single_volume(flat_i, flat_l, net, K, patch_size=PATCH, device=dev, resize="device", tta="flips")
    with pytest.raises(ValueError, match="conf_out"):
        evaluate.predict_volume(net, image[0].to(dev), PATCH, conf_out=torch.empty(3, 30, 26, device=dev))
    with pytest.raises(ValueError, match="conf_out"):
        evaluate.predict_volume(net, image[0].to(dev), PATCH, tta="flips", conf_out=torch.empty(3, 30, 25, device=dev))
    with pytest.raises(ValueError, match="tta"):
        evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="device", tta="flip")
