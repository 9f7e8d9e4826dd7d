"""Boundary-distance maps of label maps and of thresholded predictions (csrc/edt.hip cenet_dist_maps_*, ops.distance_maps /
ops.pred_distance_maps) against scipy.ndimage.distance_transform_edt.  Everything is integer and compared exactly.  Every case
runs on the host SIMT checker and, marked gpu, on the MI355X.

The oracle takes the squared distances from the INDICES scipy returns, not from its float distances (dist_cases.half_map checks
that the two agree on every plane used here).  A plane whose mask is empty or full is zeros."""
import numpy as np
import pytest
import torch

import dist_cases as C
from backend import dev  # noqa: F401
from cenet_amd import _lib, kern, ops
from test_ccl import _guarded, _untouched

DTYPES = [pytest.param(torch.float32, id="f32"), pytest.param(torch.bfloat16, id="bf16")]


def _sync(d):
    if d.type == "cuda":
        torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _run(d, src, shape, from_logits, ws_short=0):
    """the kern call with its output inside a sentinel-filled buffer and its input checked bit for bit afterwards"""
    B, K, H, W = shape
    n = B * (K - 1) * H * W
    t = src.to(d)
    before = t.clone()
    buf, d2, lead = _guarded(n, torch.int32, -7, d)
    ws = torch.empty(kern.dist_maps_ws_ints(B, K, H, W) - ws_short, dtype=torch.int32, device=d)
    (kern.dist_maps_logits if from_logits else kern.dist_maps_labels)(t, ws, d2, B, K, H, W)
    _sync(d)
    assert _untouched(buf, n, lead, -7)
    assert torch.equal(_bits(t), _bits(before))
    return d2.cpu().numpy().reshape(B, K - 1, H, W)


# ---- what the cases are worth, on the oracle's side ------------------------------------------------------------------------------
def test_the_cases_cannot_flip_a_threshold_and_cover_degenerate_planes():
    gt_deg, pred_deg = [], []
    for shape in C.SHAPES:
        K = shape[1]
        masks = [C.label_masks(C.labels(shape), K)]
        for dtype in (torch.float32, torch.bfloat16):
            x = C.logits_as(shape, dtype)[1]
            p = torch.softmax(x.double(), dim=1)
            assert float((p - 0.5).abs().min()) >= 0.39, (shape, dtype)
            masks.append(C.pred_masks(x))
        assert np.array_equal(masks[1], masks[2])  # fp32 and bf16 logits threshold to the same masks
        assert np.array_equal(masks[1], C.label_masks(C.pred_pattern(shape), K))
        deg = [[C.degenerate(p) for img in m for p in img] for m in masks[:2]]
        for dg in deg:
            assert 2 * sum(dg) <= len(dg), shape
        gt_deg.append(any(deg[0]))
        pred_deg.append(any(deg[1]))
    assert any(gt_deg) and any(pred_deg)
    for shape in ((2, 3, 7, 1), (3, 4, 9, 11)):
        i = C.SHAPES.index(shape)
        assert gt_deg[i] and pred_deg[i]


def test_the_oracle_on_a_plane_done_by_hand():
    m = np.zeros((3, 5), bool)
    m[1, 1:4] = True
    m[0, 2] = True
    want = np.array([[2, 1, 1, 1, 2], [1, 1, 1, 1, 1], [2, 1, 1, 1, 2]])
    assert np.array_equal(C.boundary_map(m), want)
    m = np.ones((4, 6), bool)
    m[3, 5] = False  # inside: the squared distance to that one pixel
    y, x = np.indices((4, 6))
    want = (y - 3) ** 2 + (x - 5) ** 2
    want[3, 5] = 1
    assert np.array_equal(C.boundary_map(m), want)
    assert not C.boundary_map(np.ones((3, 5), bool)).any() and not C.boundary_map(np.zeros((3, 5), bool)).any()


# ---- the cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_label_maps(dev, shape):
    lab = torch.from_numpy(C.labels(shape).copy())
    want = C.label_maps(shape)
    got = _run(dev, lab, shape, False)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    pub = ops.distance_maps(lab.to(dev), shape[1])
    assert pub.dtype == torch.int32 and tuple(pub.shape) == want.shape and np.array_equal(pub.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_prediction_maps(dev, shape, dtype):
    x = C.logits_as(shape, dtype)[0]
    want = C.pred_maps(shape, dtype)
    got = _run(dev, x, shape, True)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    pub = ops.pred_distance_maps(x.to(dev))
    assert pub.dtype == torch.int32 and tuple(pub.shape) == want.shape and np.array_equal(pub.cpu().numpy(), want)


def _check_labels(d, lab, K):
    lab = np.ascontiguousarray(lab, dtype=np.float32)
    want = C.maps_of(C.label_masks(lab, K))
    got = _run(d, torch.from_numpy(lab), (lab.shape[0], K) + lab.shape[1:], False)
    assert np.array_equal(got, want)
    return want


@pytest.mark.parametrize("hw", [(1, 5), (9, 11), (50, 150)], ids=lambda s: "x".join(map(str, s)))
def test_all_background_and_all_one_class_give_zeros(dev, hw):
    assert not _check_labels(dev, np.zeros((2,) + hw), 4).any()
    assert not _check_labels(dev, np.full((2,) + hw, 2.0), 4).any()


@pytest.mark.parametrize("corner", [(0, 0), (0, -1), (-1, 0), (-1, -1)])
def test_single_pixel_in_a_corner(dev, corner):
    lab = np.zeros((1, 30, 70))
    lab[0][corner] = 1
    want = _check_labels(dev, lab, 3)
    y, x = np.indices((30, 70))
    cy, cx = corner[0] % 30, corner[1] % 70
    expect = (y - cy) ** 2 + (x - cx) ** 2
    expect[cy, cx] = 1  # the pixel itself: its nearest pixel outside the class is a neighbour
    assert np.array_equal(want[0, 0], expect) and not want[0, 1].any()


@pytest.mark.parametrize("hw", [(7, 1), (9, 11), (33, 130)], ids=lambda s: "x".join(map(str, s)))
def test_checkerboard(dev, hw):
    b, y, x = np.indices((2,) + hw)
    want = _check_labels(dev, ((b + y + x) % 2).astype(np.float32), 2)
    assert (want == 1).all()  # every pixel has a neighbour of the other kind


def test_two_runs_are_bit_identical(dev):
    shape = (2, 4, 30, 70)
    lab, x = torch.from_numpy(C.labels(shape).copy()).to(dev), C.logits_as(shape, torch.float32)[0].to(dev)
    a, b = ops.distance_maps(lab, 4), ops.distance_maps(lab, 4)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    a, b = ops.pred_distance_maps(x), ops.pred_distance_maps(x)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


def test_refusals(dev):
    shape = (3, 4, 9, 11)
    B, K, H, W = shape
    lab, x = torch.from_numpy(C.labels(shape).copy()).to(dev), C.logits_as(shape, torch.float32)[0].to(dev)
    for k in (1, 17):
        with pytest.raises(ValueError, match="classes"):
            ops.distance_maps(lab, k)
        xk = torch.zeros(1, k, 3, 3, device=dev)
        with pytest.raises(ValueError, match="classes"):
            ops.pred_distance_maps(xk)
    with pytest.raises(ValueError):
        ops.distance_maps(lab[0], K)  # [H,W] is no batch
    with pytest.raises(ValueError):
        ops.pred_distance_maps(x[0])
    # the plane count, 2 B (K-1) <= 65535, and the int32 distances: a predicate (nothing that large is allocated)
    assert kern.dist_maps_supported(32, 4, 224, 224) and kern.dist_maps_supported(32767, 2, 1, 1)
    assert not kern.dist_maps_supported(32768, 2, 1, 1) and kern.dist_maps_supported(2184, 16, 1, 1)
    assert not kern.dist_maps_supported(2185, 16, 1, 1)
    assert kern.dist_maps_supported(1, 2, 32768, 32767) and not kern.dist_maps_supported(1, 2, 32768, 32768)
    assert not kern.dist_maps_supported(0, 2, 4, 4) and not kern.dist_maps_supported(1, 2, 0, 4)
    small = torch.zeros(8, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        kern.dist_maps_labels(lab, small, small, 32768, 2, 1, 1)
    # tensors that do not fit the shape, or alias: before the library is touched
    n = B * (K - 1) * H * W
    ws = torch.empty(kern.dist_maps_ws_ints(B, K, H, W), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="elements"):
        kern.dist_maps_labels(lab, ws, torch.empty(n - 1, dtype=torch.int32, device=dev), B, K, H, W)
    with pytest.raises(ValueError, match="alias"):
        kern.dist_maps_labels(lab, ws, ws[:n], B, K, H, W)
    # a workspace one int short: the ABI's error, nothing is launched
    out = torch.full((n,), -7, dtype=torch.int32).to(dev)
    for call, src, name in ((kern.dist_maps_labels, lab, "cenet_dist_maps_labels_f32"), (kern.dist_maps_logits, x, "cenet_dist_maps_logits_f32")):
        with pytest.raises(RuntimeError, match=f"{name} failed with error code 1"):
            call(src, ws[:-1], out, B, K, H, W)
    with pytest.raises(RuntimeError, match="cenet_dist_maps_logits_bf16 failed with error code 1"):
        kern.dist_maps_logits(x.bfloat16(), ws[:-1], out, B, K, H, W)
    _sync(dev)
    assert bool((out == -7).all())
    kern.dist_maps_labels(lab, ws, out, B, K, H, W)
    assert np.array_equal(out.cpu().numpy().reshape(B, K - 1, H, W), C.label_maps(shape))


def test_host_tensors_are_refused_off_the_checker():
    assert not _lib.is_hostsim()
    for call in (lambda: ops.distance_maps(torch.zeros(2, 3, 4), 4), lambda: ops.pred_distance_maps(torch.zeros(2, 4, 3, 4))):
        with pytest.raises(ValueError, match="MI355X"):
            call()
