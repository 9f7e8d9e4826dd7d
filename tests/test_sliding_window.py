"""Sliding-window inference at the image's own resolution (csrc/sliding_window.hip through kern.sw_origins / sw_weights / sw_windows
/ sw_merge_counts, evaluate.sliding_window_predict, evaluate.predict_volume(window_overlap=...) and the wrappers' `window_overlap=`).
The window batch is held to numpy slicing and padding bit for bit, the fused merge (softmax per window and view, importance-weighted
blend, argmax, counts) to the float64 restatement of tests/sw_ref.py.  `sim` runs the kernel sources on the host SIMT checker, `hip`
(marker gpu) the gfx950 kernels.

The two bounds (conf within 2e-6; predictions equal except at near-ties of the reference, at most 0.5 % of a case) are in
tests/sw_ref.py with their derivation."""
import numpy as np
import pytest
import torch

import sw_ref
from backend import dev  # noqa: F401
from cenet_amd import evaluate, kern
from sw_ref import CONF_TOL, GAP_TOL, hold_to_reference
from tta_ref import smooth_volume, view, view_codes


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- 0. the host side: origins and weights -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,P,overlap,want", [(40, 16, 0.5, [0, 8, 16, 24]), (36, 16, 0.5, [0, 7, 13, 20]), (33, 16, 0, [0, 8, 17]),
                                              (50, 16, 0, [0, 11, 23, 34]), (12, 16, 0.5, [-2]), (12, 16, 0, [-2]), (16, 16, 0.9, [0]),
                                              (13, 16, 0.5, [-1]), (512, 224, 0.5, [0, 96, 192, 288]),
                                              (512, 224, 0.3, [0, 144, 288])])
def test_origins_known_answers(L, P, overlap, want):
    """nnU-Net's rule N = ceil((L - P) / (P (1 - overlap))) + 1.  (512, 224, 0.5): ceil(288 / 112) + 1 = 4 windows per axis, 16 per
    slice; three windows per axis, [0, 144, 288], is what the rule gives up to overlap 0.357.)"""
    assert kern.sw_origins(L, P, overlap) == want == sw_ref.origins(L, P, overlap)
    assert all(isinstance(o, int) for o in kern.sw_origins(L, P, overlap))


def test_origins_and_weights_are_the_reference_ones():
    for L in (1, 9, 16, 17, 31, 70, 100):
        for P in (8, 16, 20, 24):
            for ov in (0, 0.25, 0.5, 0.75, 0.875):
                try:
                    want = sw_ref.origins(L, P, ov)
                except ValueError:  # more than 32 windows
                    with pytest.raises(ValueError, match="at most 32"):
                        kern.sw_origins(L, P, ov)
                    continue
                o = kern.sw_origins(L, P, ov)
                assert o == want
                assert o[0] <= 0 and o[-1] + P >= L and all(a < b <= a + P for a, b in zip(o, o[1:]))
    for P in (1, 8, 20, 224):
        for imp in ("gaussian", "constant"):
            w = kern.sw_weights(P, imp)
            assert w.dtype == np.float32 and np.array_equal(_bits(w), _bits(sw_ref.weights(P, imp))) and (w > 0).all()
    w = kern.sw_weights(16)
    assert w[7] == w[8] == np.float32(np.exp(-0.5 * (0.5 / 2.0) ** 2)) and np.array_equal(w, w[::-1])


# ---- 1. windows ----------------------------------------------------------------------------------------------------------------------
def _windows(x, oy, ox, patch, dev, **kw):
    n, C, H, W = x.shape
    out = torch.full((n * len(oy) * len(ox), C) + tuple(patch), float("nan"), device=dev)
    kern.sw_windows(torch.from_numpy(x).to(dev), out, oy, ox, n, C, H, W, patch[0], patch[1], **kw)
    return out.cpu().numpy()


@pytest.mark.parametrize("overlap", [0, 0.5, 0.75])
@pytest.mark.parametrize("n,C,H,W,patch", [(2, 3, 40, 36, (16, 16)), (1, 1, 12, 40, (16, 16)), (1, 2, 70, 33, (24, 20)),
                                           (2, 1, 16, 16, (16, 16))], ids=_ids)
def test_windows_are_numpy_slices_bit_for_bit(dev, n, C, H, W, patch, overlap):
    x = np.random.default_rng(H * W).standard_normal((n, C, H, W)).astype(np.float32)
    x[0, 0, 0, 0], x[0, 0, 0, 1], x[0, 0, 1, 0] = np.float32("nan"), -0.0, np.float32("inf")  # bit copies, not arithmetic
    x[-1, -1, -1, -1] = -np.float32("inf")
    oy, ox = kern.sw_origins(H, patch[0], overlap), kern.sw_origins(W, patch[1], overlap)
    for pad in (0.0, -1.0):
        got = _windows(x, oy, ox, patch, dev, pad_value=pad)
        assert np.array_equal(_bits(got), _bits(sw_ref.windows(x, oy, ox, patch, pad)))
        # normalised: torch's float32 (x - mean) / std inside the slice, the pad value as given outside
        mean, std = 0.3, 0.7
        norm = ((torch.from_numpy(x) - mean) / std).numpy()
        got = _windows(x, oy, ox, patch, dev, pad_value=pad, normalize=(mean, std))
        want = sw_ref.windows(norm, oy, ox, patch, pad)
        fin = ~np.isnan(want)
        assert np.array_equal(np.isnan(got), ~fin) and np.array_equal(_bits(got)[fin], _bits(want)[fin])
    if H < patch[0]:
        assert (got[:, :, 0] == -1.0).all() and len(oy) == 1  # (the padded rows really exist)


# ---- 2. merge against float64 ----------------------------------------------------------------------------------------------------
CASES = [(0x01, 2, 4, (16, 16), (40, 36), 0.5, "gaussian"),
         (0x01, 4, 9, (16, 16), (12, 40), 0.5, "gaussian"),   # padding along y
         (0x01, 2, 4, (16, 16), (16, 16), 0.5, "gaussian"),   # one window
         (0x01, 2, 3, (16, 16), (32, 48), 0, "constant"),     # abutting tiles
         (0x01, 2, 3, (16, 16), (33, 50), 0, "gaussian"),     # a last window that overlaps after tiles that do not
         (0x01, 2, 1, (8, 8), (20, 9), 0.5, "gaussian"),
         (0x01, 1, 16, (24, 20), (70, 33), 0.5, "gaussian"),  # rectangular windows, K = 16, output tiles cut at 32
         (0x07, 2, 4, (16, 16), (40, 36), 0.5, "gaussian"),
         (0xFF, 1, 5, (16, 16), (37, 41), 0.75, "gaussian"),
         (0x0F, 3, 2, (12, 20), (9, 65), 0.25, "constant"),
         (0x01, 1, 4, (16, 16), (41, 41), 0.875, "gaussian")]  # up to 81 windows on a pixel


def _plan(patch, size, overlap, importance, dev):
    oy, ox = kern.sw_origins(size[0], patch[0], overlap), kern.sw_origins(size[1], patch[1], overlap)
    wy, wx = kern.sw_weights(patch[0], importance), kern.sw_weights(patch[1], importance)
    return oy, ox, wy, wx, torch.from_numpy(wy).to(dev), torch.from_numpy(wx).to(dev)


def _merge(stacks, labels, plan, mask, n, K, patch, size, dev, conf=True, counts=None):
    oy, ox, _, _, wy, wx = plan
    pred = torch.full((n,) + tuple(size), -1.0, device=dev)
    cf = torch.full((n,) + tuple(size), -1.0, device=dev) if conf else None
    if labels is not None and counts is None:
        counts = torch.full((K + 1, 3), -7, dtype=torch.int32, device=dev)
    kern.sw_merge_counts(stacks.to(dev), None if labels is None else labels.to(dev), wy, wx, oy, ox, pred, cf, counts, n, K, patch[0],
                         patch[1], size[0], size[1], mask)
    return pred.cpu().numpy(), None if cf is None else cf.cpu().numpy(), counts


def _case_stacks(mask, n, K, patch, nb, bf16):
    g = torch.Generator().manual_seed(1000 * mask + 10 * K + n + (500000 if bf16 else 0))
    stacks = torch.randn(len(view_codes(mask)), nb, K, patch[0], patch[1], generator=g) * 3
    return (stacks.bfloat16() if bf16 else stacks), g  # the reference is computed from the rounded values


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mask,n,K,patch,size,overlap,importance", CASES, ids=_ids)
def test_merge_against_float64_reference(dev, mask, n, K, patch, size, overlap, importance, bf16):
    """Observed (printed by every case): the largest conf error over the twenty-two cases is 4.30e-7 on the host checker and 4.30e-7
    on the MI355X (K = 16, fp32 logits); the reference excludes at most 2 of 512 voxels (one window, bf16), and no voxel differs
    from the reference on either backend."""
    plan = _plan(patch, size, overlap, importance, dev)
    oy, ox, wy, wx = plan[:4]
    stacks, g = _case_stacks(mask, n, K, patch, n * len(oy) * len(ox), bf16)
    labels = torch.randint(-1, K + 1, (n,) + tuple(size), generator=g).float()  # (a class outside [0, K) at both ends)
    want_pred, want_conf, gap = sw_ref.reference(stacks.float().numpy(), mask, n, oy, ox, wy, wx, size)
    pred, conf, counts = _merge(stacks, labels, plan, mask, n, K, patch, size, dev)
    hold_to_reference(f"mask {mask:#04x} n={n} K={K} {patch} on {size} overlap {overlap} {importance} {'bf16' if bf16 else 'fp32'}",
                      pred, conf, want_pred, want_conf, gap)
    # the counts are those of the kernel's own prediction
    p, t, c = torch.from_numpy(pred), labels, counts.cpu()
    for k in range(K):
        assert c[k].tolist() == [int(((p == k) & (t == k)).sum()), int((p == k).sum()), int((t == k).sum())]
    assert c[K].tolist() == [int(((p > 0) & (t > 0)).sum()), int((p > 0).sum()), int((t > 0).sum())]
    # without labels (and without conf): the same prediction, the count table is left alone; a second call agrees to the bit
    keep = torch.full((K + 1, 3), -7, dtype=torch.int32, device=dev)
    pred2, none, _ = _merge(stacks, None, plan, mask, n, K, patch, size, dev, conf=False, counts=keep)
    assert none is None and np.array_equal(pred2, pred) and (keep == -7).all()
    _, conf3, _ = _merge(stacks, None, plan, mask, n, K, patch, size, dev)
    assert np.array_equal(_bits(conf3), _bits(conf))


@pytest.mark.parametrize("mask,n,K,patch,size,overlap,importance", CASES, ids=_ids)
def test_float32_restatement_stays_within_a_quarter_of_the_bound(mask, n, K, patch, size, overlap, importance):
    """where CONF_TOL comes from: numpy's float32 evaluation of the same sums against float64, printed per case (the worst, 4.3e-7,
    is K = 16 with nine windows on a pixel)"""
    for bf16 in (False, True):
        oy, ox = sw_ref.origins(size[0], patch[0], overlap), sw_ref.origins(size[1], patch[1], overlap)
        wy, wx = sw_ref.weights(patch[0], importance), sw_ref.weights(patch[1], importance)
        stacks, _ = _case_stacks(mask, n, K, patch, n * len(oy) * len(ox), bf16)
        stacks = stacks.float().numpy()
        want_pred, want_conf, gap = sw_ref.reference(stacks, mask, n, oy, ox, wy, wx, size)
        p32, c32 = sw_ref.reference_f32(stacks, mask, n, oy, ox, wy, wx, size)
        ok = gap >= GAP_TOL
        err = float(np.abs(c32.astype(np.float64) - want_conf)[ok].max())
        print(f"float32 numpy, mask {mask:#04x} K={K} {size} {'bf16' if bf16 else 'fp32'}: {err:.3e}, excluded "
              f"{int((~ok).sum())} of {ok.size}")
        assert err <= CONF_TOL / 4 and np.array_equal(p32[ok], want_pred[ok])


# ---- 3. known answers ----------------------------------------------------------------------------------------------------------------
def test_one_window_is_argmax_resize_counts(dev):
    """one window of the slice's size, no augmentation: the class map of the existing kernel at equal sizes"""
    n, K, patch = 2, 4, (16, 16)
    logits = torch.randn(1, n, K, *patch, generator=torch.Generator().manual_seed(3)) * 3
    pred, _, _ = _merge(logits, None, _plan(patch, patch, 0.5, "gaussian", dev), 0x01, n, K, patch, patch, dev)
    want = torch.empty((n,) + patch, device=dev)
    kern.argmax_resize_counts(logits[0].contiguous().to(dev), None, want, None, n, K, patch[0], patch[1], patch[0], patch[1])
    assert np.array_equal(pred, want.cpu().numpy())


@pytest.mark.parametrize("mask,patch", [(0x07, (16, 16)), (0xFF, (16, 16)), (0x0F, (12, 20))], ids=_ids)
def test_one_window_with_views_is_the_tta_merge(dev, mask, patch):
    n, K, T = 2, 5, len(view_codes(mask))
    stacks = torch.randn(T, n, K, *patch, generator=torch.Generator().manual_seed(mask)) * 3
    pred, conf, _ = _merge(stacks, None, _plan(patch, patch, 0, "constant", dev), mask, n, K, patch, patch, dev)
    want, wconf = torch.empty((n,) + patch, device=dev), torch.empty((n,) + patch, device=dev)
    kern.tta_argmax_resize_counts(stacks.to(dev), None, want, wconf, None, n, K, patch[0], patch[1], patch[0], patch[1], mask)
    assert np.array_equal(pred, want.cpu().numpy())
    assert np.abs(conf.astype(np.float64) - wconf.cpu().numpy()).max() <= CONF_TOL


@pytest.mark.parametrize("importance", ["gaussian", "constant"])
@pytest.mark.parametrize("mask,patch,size,overlap", [(0x01, (16, 16), (40, 36), 0.5), (0x01, (16, 16), (12, 40), 0.5),
                                                     (0x01, (24, 20), (70, 33), 0.25), (0x01, (16, 16), (33, 50), 0),
                                                     (0x01, (8, 8), (20, 9), 0.75), (0xFF, (16, 16), (37, 12), 0.5),
                                                     (0x0F, (12, 20), (30, 65), 0.5)], ids=_ids)
def test_logits_of_the_global_position_give_the_global_argmax(dev, mask, patch, size, overlap, importance):
    """every window (and view) carries the SAME logits for a given image pixel, so the blend of equal probabilities is that
    probability: pred is the global argmax, conf the global softmax maximum.  A wrong origin, a swapped (iy, ix) order, a wrong
    offset in the padded case or a wrong inverse of a view puts another pixel's logits there."""
    n, K = 2, 4
    G = (torch.randn(n, K, *size, generator=torch.Generator().manual_seed(size[0] * size[1])) * 3).numpy()
    plan = _plan(patch, size, overlap, importance, dev)
    win = sw_ref.windows(G, plan[0], plan[1], patch, pad_value=np.float32("nan"))  # (the padding must never be read)
    stacks = torch.from_numpy(np.stack([np.ascontiguousarray(view(win, g)) for g in view_codes(mask)]))
    pred, conf, _ = _merge(stacks, None, plan, mask, n, K, patch, size, dev)
    z = np.exp(G.astype(np.float64) - G.max(axis=1, keepdims=True))
    prob = z / z.sum(axis=1, keepdims=True)
    assert np.array_equal(pred, G.argmax(axis=1).astype(np.float32))
    assert np.abs(conf.astype(np.float64) - prob.max(axis=1)).max() <= CONF_TOL


@pytest.mark.parametrize("mask,K", [(0x01, 4), (0x07, 5), (0xFF, 16)])
def test_equal_logits_give_class_zero(dev, mask, K):
    patch, size = (16, 16), (40, 23)
    plan = _plan(patch, size, 0.5, "gaussian", dev)
    stacks = torch.full((len(view_codes(mask)), 2 * len(plan[0]) * len(plan[1]), K, 16, 16), 0.75)
    pred, conf, _ = _merge(stacks, None, plan, mask, 2, K, patch, size, dev)
    assert (pred == 0).all() and (np.abs(conf - 1.0 / K) <= CONF_TOL).all()


def test_nan_logits_never_win(dev):
    """tta.hip's rule: a NaN sum never wins under `>`, the voxel falls to the first class whose sum is a number"""
    patch, size = (16, 16), (24, 16)
    plan = _plan(patch, size, 0.5, "gaussian", dev)
    stacks = torch.zeros(1, len(plan[0]), 3, 16, 16)
    stacks[0, :, 2] = 5.0
    stacks[0, 0, 2, 3, 4] = float("nan")  # window 0, pixel (3, 4): every class of that pixel's softmax is NaN
    pred, _, _ = _merge(stacks, None, plan, 0x01, 1, 3, patch, size, dev)
    assert pred[0, 3, 4] == 0 and (np.delete(pred.ravel(), 3 * 16 + 4) == 2).all()


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------
class _Proj(torch.nn.Module):
    """pointwise in the intensity (the `Proj` of tests/test_tta_gpu.py with input channels): a pixel's logits depend on nothing but
    that pixel, so the network on a window gives what the network on the whole slice gives there"""

    def __init__(self, K, cin=1):
        super().__init__()
        g = torch.Generator().manual_seed(4)
        self.w = torch.nn.Parameter(torch.randn(K, cin, generator=g) * 3)
        self.b = torch.nn.Parameter(torch.randn(K, generator=g))

    def forward(self, x):
        out = self.b.view(1, -1, 1, 1).expand(x.shape[0], -1, x.shape[2], x.shape[3])
        for c in range(x.shape[1]):
            out = out + x[:, c:c + 1] * self.w[:, c].view(1, -1, 1, 1)
        return out


def _whole(net, x, dev):
    """float64 argmax, softmax maximum and top-2 gap of the network on the whole images x [n, C, H, W]"""
    with torch.no_grad():
        z = net(x.to(dev)).double().cpu().numpy()
    z = np.exp(z - z.max(axis=1, keepdims=True))
    p = z / z.sum(axis=1, keepdims=True)
    srt = np.sort(p, axis=1)
    return p.argmax(axis=1).astype(np.float64), p.max(axis=1), srt[:, -1] - srt[:, -2]


@pytest.mark.parametrize("tta", [None, "flips"])
@pytest.mark.parametrize("shape,patch,overlap", [((7, 40, 36), (16, 16), 0.5), ((3, 12, 40), (16, 16), 0.25)], ids=_ids)
def test_predict_volume_with_windows(dev, shape, patch, overlap, tta):
    K = 4
    vol = torch.from_numpy(smooth_volume(shape, shape[1]))
    net = _Proj(K).to(dev)
    norm = (0.5, 0.5)
    want_pred, want_conf, gap = _whole(net, ((vol - norm[0]) / norm[1])[:, None], dev)
    assert len(np.unique(want_pred)) > 1
    labels = torch.clamp((vol * K).floor(), 0, K - 2)
    out = []
    for bs in (1, 5, 32, 32):  # chunk splits, chunks of several forwards, and a second call
        conf = torch.full(shape, -1.0, device=dev)
        pred, counts = evaluate.predict_volume(net, vol.to(dev), patch, batch_slices=bs, normalize=norm, labels=labels.to(dev), tta=tta,
                                               conf_out=conf, window_overlap=overlap)
        assert pred.device.type == dev.type and counts.dtype == torch.int64 and tuple(counts.shape) == (K + 1, 3)
        out.append((pred.cpu(), conf.cpu(), counts.cpu()))
    assert all(torch.equal(a, b) for o in out[1:] for a, b in zip(out[0], o))  # bit-identical
    pred, conf, counts = out[0]
    hold_to_reference(f"predict_volume {shape} windows {patch} tta {tta}", pred.numpy(), conf.numpy(), want_pred, want_conf, gap)
    for k in range(K):
        assert counts[k].tolist() == [int(((pred == k) & (labels == k)).sum()), int((pred == k).sum()), int((labels == k).sum())]
    assert counts[K].tolist() == [int(((pred > 0) & (labels > 0)).sum()), int((pred > 0).sum()), int((labels > 0).sum())]
    plain, none = evaluate.predict_volume(net, vol.to(dev), patch, normalize=norm, window_overlap=overlap, window_importance="constant")
    assert none is None
    hold_to_reference("constant map", plain.cpu().numpy(), want_conf.astype(np.float32), want_pred, want_conf, gap)


def test_sliding_window_predict(dev):
    K, B, C, H, W = 3, 5, 3, 30, 41
    g = torch.Generator().manual_seed(8)
    images = torch.rand(B, C, H, W, generator=g)
    labels = torch.randint(0, K, (B, 1, H, W), generator=g)
    net = _Proj(K, cin=C).to(dev)
    want_pred, want_conf, gap = _whole(net, (images - 0.4) / 0.3, dev)
    out = []
    for bw in (32, 1, 7, 32):
        pred, conf, counts = evaluate.sliding_window_predict(net, images.to(dev), (16, 20), overlap=0.5, labels=labels.to(dev),
                                                             batch_windows=bw, normalize=(0.4, 0.3), pad_value=-1.0)
        assert tuple(pred.shape) == (B, H, W) == tuple(conf.shape) and counts.dtype == torch.int32
        out.append((pred.cpu(), conf.cpu(), counts.cpu()))
    assert all(torch.equal(a, b) for o in out[1:] for a, b in zip(out[0], o))
    pred, conf, counts = out[0]
    hold_to_reference("sliding_window_predict", pred.numpy(), conf.numpy(), want_pred, want_conf, gap)
    t = labels[:, 0].float()
    assert counts[1].tolist() == [int(((pred == 1) & (t == 1)).sum()), int((pred == 1).sum()), int((t == 1).sum())]
    # an image smaller than the window is centred and padded; views ride along; no labels: no counts
    small = torch.rand(2, C, 9, 12, generator=g)
    sp, sc, none = evaluate.sliding_window_predict(net, small.to(dev), (16, 16), tta="d4", importance="constant")
    wp, wc, wgap = _whole(net, small, dev)
    assert none is None
    hold_to_reference("smaller than the window", sp.cpu().numpy(), sc.cpu().numpy(), wp, wc, wgap)


def _case(shape, K, seed):
    vol = smooth_volume(shape, seed)
    label = np.clip((vol * K).astype(np.int64), 0, K - 2).astype(np.float32)
    return torch.from_numpy(vol)[None], torch.from_numpy(label)[None]


PATCH = (16, 16)


def test_volume_wrappers_score_the_window_prediction(dev):
    K = 4
    image, label = _case((5, 30, 26), K, 21)
    net = _Proj(K).to(dev)
    kw = dict(window_overlap=0.5)
    pred, counts = evaluate.predict_volume(net, image[0].to(dev), PATCH, batch_slices=4, labels=label[0].to(dev), **kw)
    m = evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=4, device=dev, resize="device", **kw)
    assert m == evaluate.label_metrics(pred, label[0].to(dev), K, "acdc")
    assert evaluate.val_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=4, device=dev, **kw) == \
        evaluate.class_dice(counts)[:K - 1]
    s = evaluate.synapse_test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="device", tta="flips",
                                            window_overlap=0.25, window_importance="constant")
    ps, _ = evaluate.predict_volume(net, image[0].to(dev), PATCH, normalize=(0.5, 0.5), tta="flips", window_overlap=0.25,
                                    window_importance="constant")
    assert s == evaluate.label_metrics(ps, label[0].to(dev), K, "synapse")
    # postprocess, spacing and the NSD see only the prediction
    mp = evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="device", postprocess="lcc",
                                     spacing=(2.0, 1.0, 1.0), nsd_tolerance=1.0, **kw)
    assert mp == evaluate.label_metrics(evaluate.keep_largest_component(pred, K)[0], label[0].to(dev), K, "acdc",
                                        spacing=(2.0, 1.0, 1.0), nsd_tolerance=1.0)


def test_skin_wrappers_go_through_sliding_window_predict(dev):
    K = 2
    g = torch.Generator().manual_seed(12)
    net = _Proj(K, cin=3).to(dev)
    loader = [{"image": torch.rand(1, 3, 20, 27, generator=g), "label": (torch.rand(1, 1, 20, 27, generator=g) > 0.5).float()}
              for _ in range(2)]
    dc, acc, iou = evaluate.skin_test(net, loader, device=dev, window=(12, 12), window_overlap=0.25)
    dcs, correct, ious = [], 0, []
    for batch in loader:
        pred = evaluate.sliding_window_predict(net, batch["image"].to(dev), (12, 12), 0.25)[0]
        p, t = pred[0].cpu() > 0.5, batch["label"][0, 0] > 0.5
        dcs.append(2.0 * int((p & t).sum()) / (int(p.sum()) + int(t.sum())))
        correct += int((pred[0].cpu() == batch["label"][0, 0]).sum())
        ious.append(int((p & t).sum()) / int((p | t).sum()))
    assert 0 < sum(ious) and (dc, acc, iou) == (sum(dcs) / 2, correct / 1080, float(np.mean(ious)))
    assert evaluate.skin_val(net, loader, device=dev, window=(12, 12), window_overlap=0.25) == dc
    assert evaluate.skin_test(net, loader, device=dev, window=None) == evaluate.skin_test(net, loader, device=dev)
    with pytest.raises(ValueError, match="window"):
        evaluate.skin_val(net, loader, device=dev, window_overlap=0.5)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    ENTRY = "cenet_sw_merge_counts"

    def call(mask=0x01, K=4, patch=(16, 16), size=(40, 36), oy=(0, 8, 16, 24), ox=(0, 7, 13, 20), labels=False, counts=False):
        T = len(view_codes(mask)) if 1 <= mask <= 255 else 1
        kern.sw_merge_counts(torch.zeros(T, len(oy) * len(ox), K, *patch, device=dev),
                             torch.zeros(1, *size, device=dev) if labels else None, torch.ones(patch[0], device=dev),
                             torch.ones(patch[1], device=dev), oy, ox, torch.empty(1, *size, device=dev), None,
                             torch.zeros(K + 1, 3, dtype=torch.int32, device=dev) if counts else None, 1, K, patch[0], patch[1],
                             size[0], size[1], mask)

    call(labels=True, counts=True)  # (the arguments below are refused for the reason named, not for a slip of this helper)
    call(mask=0xFF)
    call(size=(12, 36), oy=(-2,))
    for kw in (dict(mask=0), dict(mask=256), dict(K=17), dict(K=0), dict(labels=True),
               dict(oy=(0, 8, 25)),            # a gap: 8 + 16 < 25
               dict(oy=(0, 8, 8, 24)),         # not strictly ascending
               dict(ox=(0, 13, 7, 20)),
               dict(oy=(0, 8, 16)),            # 16 + 16 < 40: the end is not reached
               dict(ox=(1, 7, 13, 20)),        # the first pixel is not covered
               dict(size=(12, 36), oy=(-16,)),  # a window beside the slice
               dict(oy=tuple(range(33)), size=(48, 36)),
               dict(mask=0x10, patch=(12, 20), size=(12, 20), oy=(0,), ox=(0,)),
               dict(mask=0xFF, patch=(12, 20), size=(12, 20), oy=(0,), ox=(0,))):
        with pytest.raises(RuntimeError, match=ENTRY):
            call(**kw)
    x = torch.zeros(1, 1, 40, 36, device=dev)
    for oy, ox in (((0, 8, 25), (0, 7, 13, 20)), ((0, 8, 16, 24), (0, 7, 13)), ((8, 0, 16, 24), (0, 7, 13, 20))):
        with pytest.raises(RuntimeError, match="cenet_sw_windows_f32"):
            kern.sw_windows(x, torch.empty(len(oy) * len(ox), 1, 16, 16, device=dev), oy, ox, 1, 1, 40, 36, 16, 16)
    # the Python layer
    for bad in (1.0, -0.1, 1.5, "0.5", True):
        with pytest.raises(ValueError, match="overlap"):
            kern.sw_origins(40, 16, bad)
        with pytest.raises(ValueError, match="overlap"):
            evaluate.predict_volume(torch.nn.Identity(), torch.zeros(2, 30, 26, device=dev), PATCH, window_overlap=bad)
        with pytest.raises(ValueError, match="overlap"):
            evaluate.sliding_window_predict(torch.nn.Identity(), torch.zeros(1, 2, 30, 26, device=dev), PATCH, overlap=bad)
    with pytest.raises(ValueError, match="at most 32"):
        kern.sw_origins(1000, 16, 0.5)
    assert len(kern.sw_origins(16 + 31 * 8, 16, 0.5)) == 32
    with pytest.raises(ValueError, match="at most 32"):
        evaluate.predict_volume(torch.nn.Identity(), torch.zeros(2, 30, 600, device=dev), PATCH, window_overlap=0.5)
    with pytest.raises(ValueError, match="importance"):
        kern.sw_weights(16, "hann")
    with pytest.raises(ValueError, match="importance"):
        evaluate.predict_volume(torch.nn.Identity(), torch.zeros(2, 30, 26, device=dev), PATCH, window_overlap=0.5,
                                window_importance="hann")
    with pytest.raises(ValueError, match=r"\(12, 20\)"):
        evaluate.predict_volume(torch.nn.Identity(), torch.zeros(2, 30, 26, device=dev), (12, 20), tta="d4", window_overlap=0.5)
    with pytest.raises(ValueError, match=r"\(12, 20\)"):
        evaluate.sliding_window_predict(torch.nn.Identity(), torch.zeros(1, 2, 30, 26, device=dev), (12, 20), tta=(0, 4))
    with pytest.raises(ValueError, match="conf_out"):
        evaluate.predict_volume(torch.nn.Identity(), torch.zeros(2, 30, 26, device=dev), PATCH, window_overlap=0.5,
                                conf_out=torch.empty(2, 30, 25, device=dev))
    with pytest.raises(ValueError, match="conf_out"):
        evaluate.predict_volume(torch.nn.Identity(), torch.zeros(2, 30, 26, device=dev), PATCH, window_overlap=0.5,
                                conf_out=torch.empty(2, 16, 16, device=dev))


def test_window_overlap_is_never_silently_ignored(dev):
    K = 4
    image, label = _case((3, 30, 26), K, 5)
    net = _Proj(K).to(dev)
    with pytest.raises(ValueError, match="window_overlap.*resize"):
        evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, window_overlap=0.5)  # resize="host"
    with pytest.raises(ValueError, match="window_overlap.*resize"):
        evaluate.val_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="host", window_overlap=0.5)
    with pytest.raises(ValueError, match="window_overlap.*resize"):
        evaluate.synapse_test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, window_overlap=0.5)
    flat_i, flat_l = torch.rand(1, 20, 24), torch.zeros(1, 20, 24)  # the Synapse 2-D branch
    with pytest.raises(ValueError, match="window_overlap"):
        evaluate.synapse_test_single_volume(flat_i, flat_l, net, K, patch_size=PATCH, device=dev, resize="device", window_overlap=0.5)
    thin_i, thin_l = _case((3, 1, 24), K, 6)  # an axis of length 1: the host route
    with pytest.raises(ValueError, match="window_overlap"):
        evaluate.test_single_volume(thin_i, thin_l, net, K, patch_size=PATCH, device=dev, resize="device", window_overlap=0.5)
    with pytest.raises(ValueError, match="window_overlap"):
        evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, device=dev, resize="device", window_overlap=1.0)
    with pytest.raises(ValueError, match="window_overlap"):
        evaluate.inference(net, [], K, patch_size=PATCH, log=lambda s: None, window_overlap=2)
    from cenet_amd import train
    with pytest.raises(ValueError, match="test_window_overlap"):
        train.train_acdc(net, [], val_batches=lambda: [], test_volumes=lambda: [], test_window_overlap=0.5, test_resize="host")
    with pytest.raises(ValueError, match="window_overlap"):
        train.train_acdc(net, [], val_batches=lambda: [], test_volumes=lambda: [], test_window_overlap=1.0)


# ---- 6. defaults -----------------------------------------------------------------------------------------------------------------------
def test_without_window_overlap_every_wrapper_makes_todays_call(dev, monkeypatch):
    K = 4
    image, label = _case((3, 30, 26), K, 5)
    net = _Proj(K).to(dev)
    seen = []

    def fake(net_, volume, patch_size, *a, **kw):
        seen.append((a, kw))
        return torch.zeros(tuple(volume.shape), device=volume.device), torch.zeros(K + 1, 3, dtype=torch.int64, device=volume.device)

    monkeypatch.setattr(evaluate, "predict_volume", fake)
    for off in ({}, dict(window_overlap=None), dict(window_overlap=None, window_importance="constant")):
        evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=4, device=dev, resize="device", **off)
        evaluate.synapse_test_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=4, device=dev, resize="device", **off)
        evaluate.val_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=4, device=dev, **off)
    assert seen[0] == ((4,), {"tta": None}) and seen[1] == ((4,), {"normalize": (0.5, 0.5), "tta": None})
    assert seen[2][0] == (4,) and sorted(seen[2][1]) == ["labels", "tta"] and seen[2][1]["tta"] is None
    for i in range(3, 9):
        assert seen[i][0] == seen[i % 3][0] and sorted(seen[i][1]) == sorted(seen[i % 3][1])
    evaluate.test_single_volume(image, label, net, K, patch_size=PATCH, batch_slices=4, device=dev, resize="device", window_overlap=0.25)
    assert seen[9] == ((4,), {"tta": None, "window_overlap": 0.25, "window_importance": "gaussian"})


def test_inference_forwards_window_overlap(dev, monkeypatch):
    seen = []

    def fake(image, label, net, classes, **kw):
        seen.append(kw)
        return [(0.5, 1.0, 0.25, 2.0)] * (classes - 1)

    monkeypatch.setattr(evaluate, "test_single_volume", fake)
    cases = [{"image": None, "label": None, "case_name": "c0"}]
    net = _Proj(4).to(dev)
    evaluate.inference(net, cases, 4, patch_size=PATCH, log=lambda s: None, window_overlap=0.5)
    evaluate.inference(net, cases, 4, patch_size=PATCH, log=lambda s: None, window_overlap=0, window_importance="constant", tta="d4")
    evaluate.inference(net, cases, 4, patch_size=PATCH, log=lambda s: None)
    evaluate.inference(net, cases, 4, patch_size=PATCH, log=lambda s: None, window_overlap=None, window_importance="constant")
    assert seen[0]["window_overlap"] == 0.5 and seen[0]["window_importance"] == "gaussian" and seen[0]["resize"] == "device"
    assert seen[1]["window_overlap"] == 0 and seen[1]["window_importance"] == "constant" and seen[1]["tta"] == "d4"
    assert "window_overlap" not in seen[2] and "window_importance" not in seen[2] and seen[2] == seen[3]
