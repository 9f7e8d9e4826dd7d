"""The two resizes of the test-time volume inference on the device (csrc/volresize.hip through kern.vol_resize_cubic /
kern.argmax_resize_counts) against scipy.ndimage.zoom called the way the reference calls it (src/utils/metrics_eval.py:45,55).
Resize in: within 1e-6 of scipy and >= 99.9 % of the float32 values bit-identical (the bounds tests/test_augment.py holds the
same arithmetic to).  Argmax + resize back: class ids and overlap counts exactly.  `sim` runs the kernel sources on the host SIMT
checker, `hip` (marker gpu) the gfx950 kernels."""
import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

from backend import dev  # noqa: F401
from cenet_amd import evaluate, kern

# (H, W) -> (PH, PW); the large ones run on the GPU only (the host checker runs the fp64 prefilter lane by lane)
SMALL = [((30, 26), (16, 16)), ((20, 24), (16, 16)), ((58, 63), (224, 224))]
LARGE = [((256, 216), (224, 224)), ((232, 256), (224, 224)), ((248, 256), (224, 224)), ((512, 512), (224, 224)),
         ((160, 200), (224, 224))]
PAIRS = SMALL + LARGE
# sizes whose last zoom coordinate rounds above len - 1, so that scipy writes cval there: (last row, last column) zeroed
ZEROED = {(232, 256): (True, False), (248, 256): (True, False), (58, 63): (True, True), (512, 512): (True, True),
          (256, 216): (False, False), (160, 200): (False, False)}


def _skip_large_on_sim(dev, size):
    if dev.type == "cpu" and size[0] * size[1] > 100 * 100:
        pytest.skip("the host checker runs the fp64 prefilter lane by lane: the small sizes cover the arithmetic")


def _resize_in(stack, patch, dev, normalize=None):
    n, H, W = stack.shape
    src = torch.from_numpy(stack).to(dev)
    stage = torch.empty(n * H * W, dtype=torch.float64, device=dev)
    out = torch.empty(n, 1, patch[0], patch[1], dtype=torch.float32, device=dev)
    kern.vol_resize_cubic(src, stage, out, n, H, W, patch[0], patch[1], normalize)
    return out.cpu().numpy()[:, 0]


@pytest.mark.parametrize("size,patch", PAIRS, ids=lambda v: "x".join(map(str, v)))
def test_resize_in_matches_scipy_zoom(dev, size, patch):
    _skip_large_on_sim(dev, size)
    n = 3 if size[0] * size[1] <= 256 * 256 else 2
    stack = np.random.default_rng(size[0] * 1000 + size[1]).random((n,) + size).astype(np.float32)
    want = np.stack([zoom(a, (patch[0] / size[0], patch[1] / size[1]), order=3) for a in stack])
    got = _resize_in(stack, patch, dev)
    assert got.shape == want.shape and want.dtype == np.float32
    exact = int((got == want).sum())
    print(f"{size} -> {patch}: max |d| = {np.abs(got - want).max():.3e}, identical {exact} / {want.size}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    assert exact >= 0.999 * want.size, (exact, want.size)
    if size in ZEROED:  # the cval rule (a coordinate one ulp above len - 1) really is exercised, and followed
        row, col = ZEROED[size]
        assert bool((want[:, -1] == 0).all()) == row and bool((want[:, :, -1] == 0).all()) == col
        assert bool((got[:, -1] == 0).all()) == row and bool((got[:, :, -1] == 0).all()) == col


@pytest.mark.parametrize("size,patch", [((30, 26), (16, 16)), ((256, 216), (224, 224))], ids=lambda v: "x".join(map(str, v)))
def test_resize_in_with_normalisation(dev, size, patch):
    """mean = std = 0.5: (float32(zoom) - 0.5) / 0.5 in fp32, as the Synapse wrapper computes it on the host"""
    _skip_large_on_sim(dev, size)
    stack = np.random.default_rng(17).random((2,) + size).astype(np.float32)
    z = np.stack([zoom(a, (patch[0] / size[0], patch[1] / size[1]), order=3) for a in stack])
    want = ((torch.from_numpy(z).float() - 0.5) / 0.5).numpy()
    got = _resize_in(stack, patch, dev, normalize=(0.5, 0.5))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    assert int((got == want).sum()) >= 0.999 * want.size


def test_resize_in_one_224_case_on_every_backend(dev):
    """a 224 x 224 output also on the host checker: (58, 63) is in PAIRS; this one is an upscaling without cval"""
    stack = np.random.default_rng(4).random((1, 40, 50)).astype(np.float32)
    want = zoom(stack[0], (224 / 40, 224 / 50), order=3)
    got = _resize_in(stack, (224, 224), dev)[0]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    assert int((got == want).sum()) >= 0.999 * want.size


def _logits(n, K, patch, seed, bf16):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, K, patch[0], patch[1], generator=g)
    # constructed ties: a tenth of the pixels hold one value in every class (-> class 0), another tenth tie the last two classes
    # above the rest (-> K - 2)
    r = torch.rand(n, patch[0], patch[1], generator=g)
    logits = torch.where((r < 0.1).unsqueeze(1), torch.full_like(logits, 0.25), logits)
    tie = ((r >= 0.1) & (r < 0.2)).unsqueeze(1).expand_as(logits).clone()
    tie[:, :K - 2] = False
    logits = torch.where(tie, torch.full_like(logits, 7.0), logits)
    return logits.bfloat16() if bf16 else logits


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", [2, 4, 9])
@pytest.mark.parametrize("size,patch", PAIRS + [((16, 16), (16, 16))], ids=lambda v: "x".join(map(str, v)))
def test_argmax_resize_back_equals_zoom_order0(dev, size, patch, K, bf16):
    _skip_large_on_sim(dev, size)
    n = 2
    logits = _logits(n, K, patch, K * 100 + size[0], bf16)
    labels = torch.randint(0, K, (n,) + size, generator=torch.Generator().manual_seed(K + size[1])).float()
    if K == 9:
        labels[labels == 5] = 0
    # the host procedure (metrics_eval.py:52-58) on the same values (bf16 upcast)
    am = torch.argmax(torch.softmax(logits.float(), dim=1), dim=1).numpy()
    assert (am == torch.argmax(logits.float(), dim=1).numpy()).all()
    if size != patch:
        want = np.stack([zoom(a, (size[0] / patch[0], size[1] / patch[1]), order=0) for a in am])
    else:
        want = am
    assert want.shape == (n,) + size
    pred = torch.empty((n,) + size, dtype=torch.float32, device=dev)
    counts = torch.empty(K + 1, 3, dtype=torch.int32, device=dev)
    kern.argmax_resize_counts(logits.to(dev), labels.to(dev), pred, counts, n, K, patch[0], patch[1], size[0], size[1])
    got = pred.cpu().numpy()
    print(f"{patch} -> {size} K={K}: {int((got != want).sum())} mismatches of {want.size}")
    assert np.array_equal(got, want.astype(np.float32))
    # the counts of predict_counts applied to the host result
    wt = torch.from_numpy(want.astype(np.int64))
    c = counts.cpu()
    for k in range(K):
        assert c[k].tolist() == [int(((wt == k) & (labels == k)).sum()), int((wt == k).sum()), int((labels == k).sum())]
    assert c[K].tolist() == [int(((wt > 0) & (labels > 0)).sum()), int((wt > 0).sum()), int((labels > 0).sum())]
    # without labels: the same prediction, no counts touched
    pred2 = torch.empty_like(pred)
    kern.argmax_resize_counts(logits.to(dev), None, pred2, None, n, K, patch[0], patch[1], size[0], size[1])
    assert torch.equal(pred2, pred)


def test_equal_sizes_are_the_plain_argmax(dev):
    logits = _logits(3, 4, (17, 23), 5, False)
    labels = torch.randint(0, 4, (3, 17, 23), generator=torch.Generator().manual_seed(1)).float()
    want_pred, want_counts = evaluate.predict_counts(logits.to(dev), labels.to(dev))
    pred = torch.empty(3, 17, 23, dtype=torch.float32, device=dev)
    counts = torch.empty(5, 3, dtype=torch.int32, device=dev)
    kern.argmax_resize_counts(logits.to(dev), labels.to(dev), pred, counts, 3, 4, 17, 23, 17, 23)
    assert torch.equal(pred, want_pred) and torch.equal(counts, want_counts)


def test_length_one_axes_are_refused(dev):
    """scipy special-cases length-1 axes; the kernels return CENET_EINVAL and the Python side keeps such cases on the host"""
    assert not kern.vol_resize_supported(1, 20, 16, 16) and not kern.vol_resize_supported(20, 20, 16, 1)
    src = torch.zeros(1, 1, 20, device=dev)
    with pytest.raises(RuntimeError, match="cenet_vol_resize_cubic"):
        kern.vol_resize_cubic(src, torch.empty(20, dtype=torch.float64, device=dev), torch.empty(1, 1, 16, 16, device=dev), 1, 1, 20,
                              16, 16)
    with pytest.raises(RuntimeError, match="cenet_argmax_resize_counts"):
        kern.argmax_resize_counts(torch.zeros(1, 2, 16, 16, device=dev), None, torch.empty(1, 1, 20, device=dev), None, 1, 2, 16, 16,
                                  1, 20)
    with pytest.raises(ValueError):
        evaluate.predict_volume(torch.nn.Identity(), torch.zeros(2, 1, 20, device=dev), (16, 16))
