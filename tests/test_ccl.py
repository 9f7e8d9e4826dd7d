"""Connected components and the keep-largest filter (csrc/ccl.hip, evaluate.connected_components / component_sizes /
keep_largest_component) against scipy.ndimage.label.  Everything is integer and compared exactly.  Every case runs on the host SIMT
checker and, marked gpu, on the MI355X.

ccl.hip works on tiles of 256 consecutive voxels: no shape below is a multiple of it, every axis is the short one once, and
(5, 30, 70) and (3, 50, 150) have rows that straddle tile edges and planes of more than one tile."""
import numpy as np
import pytest
import torch
from scipy import ndimage
from scipy.ndimage import zoom

from backend import dev  # noqa: F401
from cenet_amd import _lib, evaluate, kern

K = 4
SHAPES = [(1, 9, 11), (7, 1, 10), (6, 8, 1), (1, 1, 5), (9, 17, 33), (5, 30, 70), (3, 50, 150), (67, 5, 3), (2, 131, 4)]
MODES = [(1, False), (2, False), (3, False), (1, True), (2, True)]  # (connectivity, per_slice)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def _classes(vol, k):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(vol) & (vol >= 1) & (vol < k) & (np.floor(vol) == vol)
    return np.where(ok, np.nan_to_num(vol, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)


def _oracle(vol, k, conn, per_slice, min_size=0):
    """vol [D,H,W] -> (roots, sizes, filtered, table) as the library defines them, from scipy.ndimage.label per class"""
    cls = _classes(vol, k)
    D = vol.shape[0]
    idx = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)
    roots = np.full(vol.shape, -1, np.int32)
    sizes = np.zeros(vol.shape, np.int32)
    out = np.zeros(vol.shape, np.float32)
    table = np.zeros((k, 3), np.int32)
    for c in range(1, k):
        m = cls == c
        parts = [(slice(z, z + 1), m[z], ndimage.generate_binary_structure(2, conn)) for z in range(D)] if per_slice else \
            [(slice(None), m, ndimage.generate_binary_structure(3, conn))]
        for sl, mask, st in parts:
            lab, nl = ndimage.label(mask, st)
            if nl == 0:
                continue
            lab = lab.reshape(idx[sl].shape)
            count = np.bincount(lab.ravel())
            first = np.asarray(ndimage.minimum(idx[sl], lab, np.arange(1, nl + 1))).astype(np.int64)  # canonical root per label
            fg = lab > 0
            roots[sl][fg] = first[lab[fg] - 1]
            sizes.ravel()[first] = count[1:]
            largest = int(np.argmax(count[1:])) + 1  # the first maximum: scipy numbers components in raster order
            keep = fg & ((lab == largest) | ((count[lab] >= min_size) if min_size > 0 else False))
            out[sl][keep] = c
            table[c] += (nl, int(keep.sum()), int(fg.sum() - keep.sum()))
    return roots, sizes, out, table


# ---- the library, every output inside a sentinel-filled buffer -------------------------------------------------------------------
def _guarded(n, dtype, fill, d, lead=7, tail=9):
    buf = torch.full((lead + n + tail,), fill, dtype=dtype).to(d)
    return buf, buf[lead:lead + n], lead


def _untouched(buf, n, lead, fill):
    b = buf.cpu()
    return bool((b[:lead] == fill).all()) and bool((b[lead + n:] == fill).all())


def _library(d, vol, k, conn, per_slice, min_size=0):
    D, H, W = vol.shape
    n = vol.size
    t = torch.from_numpy(vol).to(d)
    before = t.clone()
    rb, roots, l0 = _guarded(n, torch.int32, -7, d)
    sb, sizes, _ = _guarded(n, torch.int32, -7, d)
    ob, out, _ = _guarded(n, torch.float32, -3.5, d)
    tb, table, _ = _guarded(3 * k, torch.int32, -7, d)
    ws = torch.empty(kern.ccl_ws_ints(k, D, not per_slice), dtype=torch.int32, device=d)
    kern.ccl_label(t, roots, k, D, H, W, conn, not per_slice)
    kern.ccl_sizes(roots, sizes, n)
    kern.ccl_keep(t, roots, sizes, ws, out, table, k, D, H, W, not per_slice, min_size)
    if d.type == "cuda":
        torch.cuda.synchronize()
    assert _untouched(rb, n, l0, -7) and _untouched(sb, n, l0, -7) and _untouched(ob, n, l0, -3.5) and _untouched(tb, 3 * k, l0, -7)
    assert torch.equal(t.view(torch.int32), before.view(torch.int32))  # (bit for bit: the map may hold NaN)
    return (t, roots.cpu().numpy().reshape(vol.shape), sizes.cpu().numpy().reshape(vol.shape), out.cpu().numpy().reshape(vol.shape),
            table.cpu().numpy().reshape(k, 3))


def _check(d, vol, k=K, modes=MODES, min_size=0):
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    for conn, per_slice in modes:
        want = _oracle(vol, k, conn, per_slice, min_size)
        t, *got = _library(d, vol, k, conn, per_slice, min_size)
        for name, g, w in zip(("roots", "sizes", "filtered", "table"), got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, conn, per_slice)
        # the public functions are the same calls
        roots = evaluate.connected_components(t, k, conn, per_slice)
        assert roots.dtype == torch.int32 and np.array_equal(roots.cpu().numpy(), want[0])
        assert np.array_equal(evaluate.component_sizes(roots).cpu().numpy(), want[1])
        filt, table = evaluate.keep_largest_component(t, k, conn, per_slice, min_size)
        assert filt.dtype == torch.float32 and filt.shape == t.shape and filt.data_ptr() != t.data_ptr()
        assert np.array_equal(filt.cpu().numpy(), want[2])
        assert isinstance(table, np.ndarray) and table.shape == (k, 3) and np.array_equal(table, want[3])
    return want


# ---- patterns --------------------------------------------------------------------------------------------------------------------
def _noise(shape, k=K, seed=0):
    return np.random.default_rng(seed).integers(0, k, shape).astype(np.float32)


def _blobs(shape, seed, thresh=0.55):
    """smooth random blobs, as tests/test_edt.py builds them"""
    rng = np.random.default_rng(seed)
    low = rng.random(tuple(max(2, s // 4) for s in shape))
    v = zoom(low, [s / l for s, l in zip(shape, low.shape)], order=1)
    return v > thresh


def _blob_labels(shape, k=K, seed=0):
    vol = np.zeros(shape, np.float32)
    for c in range(1, k):
        vol[_blobs(shape, seed + c)] = c
    return vol


def _spiral(n):
    """a one-voxel-wide spiral with one-voxel gaps that fills an n x n plane: one component, a chain as long as they get"""
    a = np.zeros((n, n), np.float32)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = 1

    def can(y, x, dy, dx):
        ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        return 0 <= ny < n and 0 <= nx < n and a[ny, nx] == 0 and not (0 <= my < n and 0 <= mx < n and a[my, mx] == 1)

    while True:
        if not can(y, x, dy, dx):
            dy, dx = dx, -dy
            if not can(y, x, dy, dx):
                return a
        y, x = y + dy, x + dx
        a[y, x] = 1


def _comb(shape):
    """teeth of class 1 on the even columns, joined only by the last row; class 2 on the odd columns, never joined in a plane"""
    vol = np.zeros(shape, np.float32)
    vol[:, :, 0::2] = 1
    vol[:, :, 1::2] = 2
    vol[:, -1, :] = 1
    return vol


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_noise(dev, shape):
    _check(dev, _noise(shape, seed=sum(shape)))


@pytest.mark.parametrize("shape", [(9, 17, 33), (5, 30, 70), (3, 50, 150), (2, 131, 4)], ids=lambda s: "x".join(map(str, s)))
def test_blobs(dev, shape):
    vol = _blob_labels(shape, seed=sum(shape))
    assert all((vol == c).any() for c in range(1, K))
    _check(dev, vol)


@pytest.mark.parametrize("depth", [1, 9])
def test_spiral(dev, depth):
    vol = np.zeros((depth, 33, 33), np.float32)
    vol[depth // 2] = 3 * _spiral(33)
    assert vol.sum() > 3 * 33 * 33 * 0.45
    want = _check(dev, vol)
    assert want[3][3].tolist() == [1, int((vol == 3).sum()), 0]  # one component, at every connectivity


@pytest.mark.parametrize("shape", [(1, 9, 11), (5, 30, 70)], ids=lambda s: "x".join(map(str, s)))
def test_comb(dev, shape):
    want = _check(dev, _comb(shape))
    assert want[3][1][0] == shape[0]  # (the last mode is per slice: one comb each)


@pytest.mark.parametrize("shape", [(7, 1, 10), (9, 17, 33)], ids=lambda s: "x".join(map(str, s)))
def test_checker(dev, shape):
    z, y, x = np.indices(shape)
    vol = ((z + y + x) % 2 == 0).astype(np.float32)
    _check(dev, vol, modes=MODES[:3])
    # connectivity 1: every voxel its own component; 2 and 3: one component, unless the volume is too flat to have diagonals
    got = [evaluate.keep_largest_component(torch.from_numpy(vol).to(dev), K, c)[1][1, 0] for c in (1, 2, 3)]
    assert got[0] == int(vol.sum()) and (got[1] == got[2] == 1 or shape[1] == 1)
    _check(dev, vol, modes=MODES[3:])


@pytest.mark.parametrize("shape", [(1, 1, 5), (3, 50, 150)], ids=lambda s: "x".join(map(str, s)))
def test_all_one_class_and_empty(dev, shape):
    want = _check(dev, np.full(shape, 2, np.float32))
    assert want[3][2].tolist() == [shape[0], int(np.prod(shape)), 0]
    want = _check(dev, np.zeros(shape, np.float32))
    assert not want[3].any() and not want[2].any() and (want[0] == -1).all()


def test_ties_go_to_the_smaller_root(dev):
    # two components of class 1 and three of class 2, all of three voxels; the winner of each class is its first in raster order
    a = np.zeros((2, 6, 7), np.float32)
    a[0, 0, 0:3] = 1
    a[1, 4, 2:5] = 1
    a[0, 2, 1:4] = a[0, 4, 4] = a[0, 5, 4] = a[1, 5, 4] = a[1, 0, 4:7] = 2
    want = _check(dev, a, modes=[(1, False), (3, False)])
    assert want[3][1].tolist() == [2, 3, 3] and want[3][2].tolist() == [3, 3, 6]
    assert (want[2][0, 0, 0:3] == 1).all() and (want[2][0, 2, 1:4] == 2).all() and want[2].sum() == 3 + 6
    # the same with a component of the larger class lying before the winner of class 1, which no longer starts the volume
    b = np.zeros((2, 6, 7), np.float32)
    b[0, 0, 0:3] = 2
    b[0, 3, 3:6] = 1
    b[1, 1, 0:3] = 1
    b[1, 5, 4:7] = 2
    want = _check(dev, b, modes=[(1, False), (2, True)])
    assert (want[2][0, 3, 3:6] == 1).all() and (want[2][0, 0, 0:3] == 2).all()
    _check(dev, b[:, ::-1].copy())
    _check(dev, b[::-1].copy())


def test_everything_that_is_no_class_is_background(dev):
    bad = np.array([2.5, -1.0, K, np.nan, np.inf, -np.inf, 0.5, 1e9, -0.0], np.float32)
    vol = np.resize(bad, (3, 5, 6))
    want = _check(dev, vol)
    assert (want[0] == -1).all() and not want[2].any() and not want[3].any()
    vol[1, 2, 2:5] = 3  # and a component in their middle survives
    want = _check(dev, vol)
    assert want[3][3].tolist() == [1, 3, 0]


def test_min_size_keeps_the_larger_components_too(dev):
    vol = _noise((5, 30, 70), seed=3)
    _check(dev, vol, modes=[(1, False), (2, True)], min_size=3)
    # what the oracle's filter amounts to, spelled out on the library's own result
    t = torch.from_numpy(vol).to(dev)
    roots = evaluate.connected_components(t, K).cpu().numpy()
    sizes = evaluate.component_sizes(evaluate.connected_components(t, K)).cpu().numpy()
    out = evaluate.keep_largest_component(t, K, min_size=3)[0].cpu().numpy()
    size_of = np.where(roots >= 0, sizes.ravel()[np.maximum(roots, 0)], 0)
    expect = np.zeros(vol.shape, bool)
    for c in range(1, K):
        m = vol == c
        winner = roots[m & (size_of == size_of[m].max())].min()
        expect |= m & ((size_of >= 3) | (roots == winner))
    assert np.array_equal(out > 0, expect) and np.array_equal(out, np.where(expect, vol, 0))
    assert (size_of[expect] < 3).sum() == 0 and 0 < expect.sum() < (vol > 0).sum()


def test_two_runs_are_bit_identical(dev):
    t = torch.from_numpy(_noise((5, 30, 70), seed=5)).to(dev)
    for conn in (1, 3):
        a = evaluate.connected_components(t, K, conn)
        b = evaluate.connected_components(t, K, conn)
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return -(x - torch.linspace(0.2, 0.8, K, device=x.device).view(1, K, 1, 1)).abs()


def test_refusals(dev):
    vol = _noise((3, 8, 9), seed=1)
    t = torch.from_numpy(vol).to(dev)
    for conn in (0, 4):
        with pytest.raises(ValueError):
            evaluate.connected_components(t, K, conn)
        with pytest.raises(ValueError):
            evaluate.keep_largest_component(t, K, conn)
    with pytest.raises(ValueError):
        evaluate.connected_components(t, K, 3, per_slice=True)
    with pytest.raises(ValueError):
        evaluate.keep_largest_component(t, K, 3, per_slice=True)
    for k in (1, 65):
        with pytest.raises(ValueError):
            evaluate.connected_components(t, k)
    # D H W >= 2^31: a predicate, and the launch wrapper refuses before it touches its (tiny) tensors
    assert kern.ccl_supported(148, 512, 512) and kern.ccl_supported(1, 32768, 65535) and not kern.ccl_supported(1, 32768, 65536)
    small = torch.zeros(8, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        kern.ccl_label(t, small, K, 2, 32768, 32768)
    D, H, W = vol.shape
    n = vol.size
    roots = evaluate.connected_components(t, K)
    sizes = evaluate.component_sizes(roots)
    need = kern.ccl_ws_ints(K, D)
    assert need == 2 * K and kern.ccl_ws_ints(K, D, False) == 2 * K * D
    table = torch.full((K, 3), -7, dtype=torch.int32).to(dev)
    with pytest.raises(ValueError, match="alias"):
        kern.ccl_keep(t, roots, sizes, torch.empty(need, dtype=torch.int32, device=dev), t, table, K, D, H, W)
    # a workspace one int short: the ABI's error, nothing is launched
    out = torch.full((n,), -3.5).to(dev)
    for zlinks in (True, False):
        short = torch.empty(kern.ccl_ws_ints(K, D, zlinks) - 1, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match="cenet_ccl_keep_f32 failed with error code 1"):
            kern.ccl_keep(t, roots, sizes, short, out, table, K, D, H, W, zlinks)
    assert bool((out == -3.5).all()) and bool((table == -7).all())
    kern.ccl_keep(t, roots, sizes, torch.empty(need, dtype=torch.int32, device=dev), out, table, K, D, H, W)
    assert np.array_equal(out.cpu().numpy().reshape(vol.shape), _oracle(vol, K, 1, False)[2])
    # an unknown post-processing name, before anything is predicted
    image, label = torch.rand(1, 3, 8, 9), torch.from_numpy(vol)[None]
    net = _Net().to(dev)
    for fn in (evaluate.test_single_volume, evaluate.synapse_test_single_volume):
        with pytest.raises(ValueError, match="postprocess"):
            fn(image, label, net, K, patch_size=(8, 9), device=dev, postprocess="largest")
    with pytest.raises(ValueError, match="postprocess"):
        evaluate.inference(net, [{"image": image, "label": label, "case_name": "c"}], K, patch_size=(8, 9), device=dev,
                           postprocess="cc", log=lambda s: None)


def test_volume_wrappers_filter_before_they_score(dev, tmp_path):
    """postprocess="lcc" on the host-resize path (the device-resize path and the training loop: tests/test_ccl_volume_gpu.py)"""
    rng = np.random.default_rng(4)
    image = rng.random((4, 12, 14)).astype(np.float32)  # pointwise net on noise: a prediction full of islands
    label = np.clip((np.stack([zoom(s, (2, 2), order=1) for s in rng.random((4, 6, 7))]) * K).astype(np.int64), 0, K - 1)
    label = label.astype(np.float32)
    net = _Net().to(dev)
    ti, tl = torch.from_numpy(image)[None], torch.from_numpy(label)[None]
    plain = evaluate.test_single_volume(ti, tl, net, K, patch_size=(12, 14), device=dev, test_save_path=str(tmp_path / "a"), case="c")
    assert plain == evaluate.test_single_volume(ti, tl, net, K, patch_size=(12, 14), device=dev, postprocess=None)
    pred = torch.from_numpy(np.load(tmp_path / "a" / "c_pred.npy")).to(dev)
    for conn, per_slice in ((1, False), (2, True)):
        filt, _ = evaluate.keep_largest_component(pred, K, conn, per_slice)
        want = evaluate.label_metrics(filt, tl[0].to(dev), K, "acdc")
        got = evaluate.test_single_volume(ti, tl, net, K, patch_size=(12, 14), device=dev, test_save_path=str(tmp_path / "b"),
                                          case="c", postprocess="lcc", lcc_connectivity=conn, lcc_per_slice=per_slice)
        assert got == want and got != plain
        assert np.array_equal(np.load(tmp_path / "b" / "c_pred.npy"), filt.cpu().numpy())
        syn = evaluate.synapse_test_single_volume(ti, tl, net, K, patch_size=(12, 14), device=dev, postprocess="lcc",
                                                  lcc_connectivity=conn, lcc_per_slice=per_slice)
        sp = evaluate.synapse_test_single_volume(ti, tl, net, K, patch_size=(12, 14), device=dev, test_save_path=str(tmp_path / "s"),
                                                 case="c")
        spred = torch.from_numpy(np.load(tmp_path / "s" / "c_pred.npy")).to(dev)
        assert syn == evaluate.label_metrics(evaluate.keep_largest_component(spred, K, conn, per_slice)[0], tl[0].to(dev), K,
                                             "synapse") and syn != sp


def test_host_tensors_are_refused_off_the_checker():
    assert not _lib.is_hostsim()
    t = torch.zeros(2, 3, 4)
    for call in (lambda: evaluate.connected_components(t, K), lambda: evaluate.keep_largest_component(t, K)):
        with pytest.raises(ValueError, match="MI355X"):
            call()
