"""Surface metrics by the exact distance transform (csrc/edt.hip): the transform against scipy, the two methods of
`surface_distances` against each other and the restated medpy, and `label_metrics` against the per-class loop.  Every case runs on
the host SIMT checker and, marked gpu, on the MI355X."""
import numpy as np
import pytest
import torch
from scipy.ndimage import distance_transform_edt, zoom

from backend import dev  # noqa: F401
from cenet_amd import evaluate, kern
from oracle import cenet_oracle as O


def _feat(shape, kind, seed=0):
    rng = np.random.default_rng(seed)
    f = np.zeros(shape, bool)
    if kind == "sparse":
        f = rng.random(shape) < 0.02
        f.flat[rng.integers(f.size)] = True
    elif kind == "dense":
        f = rng.random(shape) < 0.5
    elif kind == "corner":
        f[-1, 0, -1] = True
    elif kind == "all":
        f[:] = True
    elif kind == "face":
        f[:, 0, :] = rng.random((shape[0], shape[2])) < 0.3
        f[0, 0, 0] = True
    return f


# edt.hip walks rows in tiles of 128 rows x 64 columns and lines in groups of 64: (5, 30, 70) and (3, 50, 150) have more rows than
# one tile, sides that are no multiples of it, and rows of two and three column chunks; the compaction chunk is 4096 voxels
EDT_CASES = [((1, 9, 11), "sparse"), ((7, 1, 10), "sparse"), ((6, 8, 1), "sparse"), ((1, 1, 5), "corner"), ((4, 6, 5), "corner"),
             ((9, 17, 33), "corner"), ((4, 6, 5), "all"), ((5, 12, 9), "face"), ((5, 30, 70), "sparse"), ((5, 30, 70), "dense"),
             ((3, 50, 150), "sparse"), ((3, 50, 150), "face"), ((67, 5, 3), "sparse"), ((2, 131, 4), "corner")]


@pytest.mark.parametrize("shape,kind", EDT_CASES)
def test_edt_matches_scipy(dev, shape, kind):
    feat = _feat(shape, kind, seed=sum(shape))
    d2 = kern.edt_sq(torch.from_numpy(feat.astype(np.uint8)).to(dev))
    assert d2.dtype == torch.int32 and tuple(d2.shape) == shape
    got = np.sqrt(d2.cpu().numpy().astype(np.float64))
    assert np.array_equal(got, distance_transform_edt(~feat))


def test_edt_refuses_empty_and_oversized(dev):
    with pytest.raises(ValueError):
        kern.edt_sq(torch.zeros((2, 3, 4), dtype=torch.uint8, device=dev))
    assert kern.edt_supported(148, 512, 512) and not kern.edt_supported(1, 1, 46341)
    t = torch.zeros(8, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        kern.edt_sq_raw(torch.ones(8, dtype=torch.uint8, device=dev), -1, t, t, 1, 1, 46341)


def _blobs(shape, seed, thresh=0.55):
    """smooth random blobs: low-resolution noise upsampled, thresholded (as tests/test_evaluate.py builds them)"""
    rng = np.random.default_rng(seed)
    low = rng.random(tuple(max(2, s // 4) for s in shape))
    v = zoom(low, [s / l for s, l in zip(shape, low.shape)], order=1)
    return v > thresh


def _mask_pair(shape, seed):
    if seed == "noise":  # independent uniform labels: nearly every voxel is a border voxel
        rng = np.random.default_rng(99)
        return rng.integers(0, 2, shape).astype(bool), rng.integers(0, 2, shape).astype(bool)
    a, b = _blobs(shape, seed), _blobs(shape, seed + 100)
    if not a.any():
        a.flat[0] = True
    if not b.any():
        b.flat[-1] = True
    return a, b


@pytest.mark.parametrize("shape,seed", [((6, 20, 24), 0), ((3, 9, 7), 1), ((10, 40, 36), 2), ((1, 12, 12), 3), ((24, 24), 4),
                                        ((12, 64, 64), 5), ((8, 24, 20), "noise"), ((20, 22), "noise")])
def test_surface_distances_methods_agree(dev, shape, seed):
    a, b = _mask_pair(shape, seed)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    r1, r2 = O.surface_distances(a, b), O.surface_distances(b, a)
    for method in ("edt", "pairs", "auto"):
        d1, d2 = evaluate.surface_distances(ta, tb, method=method)
        assert d1.dtype == np.float64 and d1.shape == r1.shape and d2.shape == r2.shape, method
        assert np.array_equal(d1, r1) and np.array_equal(d2, r2), method  # element for element, in C order of the border voxels
        assert evaluate.hd95(ta, tb, method=method) == O.hd95_metric(a, b)
        assert evaluate.assd(ta, tb, method=method) == O.assd_metric(a, b)
        got, want = evaluate.metric_percase(ta, tb, method=method), O.metric_percase(a, b)
        assert got[1] == want[1] and got[3] == want[3] and all(abs(g - w) < 1e-12 for g, w in zip(got, want))


def test_surface_distances_empty_masks_raise(dev):
    z = torch.zeros((3, 5, 5), dtype=torch.bool, device=dev)
    one = z.clone()
    one[1, 2, 2] = True
    for method in ("edt", "pairs", "auto"):
        with pytest.raises(RuntimeError, match="first"):
            evaluate.surface_distances(z, one, method=method)
        with pytest.raises(RuntimeError, match="second"):
            evaluate.surface_distances(one, z, method=method)
        assert evaluate.metric_percase(one, z, method=method) == (1, 0, 1, 0)
        assert evaluate.metric_percase(z, one, method=method) == (0, 0, 0, 0)
        assert evaluate.synapse_metric_percase(one, z, method=method) == (1, 0)
        assert evaluate.synapse_metric_percase(z, z, method=method) == (0, 0)


def _label_pair(shape, K, seed):
    """two smooth label maps with classes 0..K-1"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        low = rng.random(tuple(max(2, s // 3) for s in shape))
        v = zoom(low, [s / l for s, l in zip(shape, low.shape)], order=1)
        v = (v - v.min()) / (v.max() - v.min() + 1e-12)
        out.append(np.clip((v * K).astype(np.int64), 0, K - 1).astype(np.float32))
    return out


def _apply(pred, gt, c, scenario):
    if scenario in ("only_pred", "neither"):
        gt[gt == c] = 0
    if scenario in ("only_gt", "neither"):
        pred[pred == c] = 0
    if scenario == "identical":
        gt[gt == c] = 0
        gt[pred == c] = c
    return pred, gt


SCENARIOS = {2: [{}, {1: "only_pred"}, {1: "only_gt"}, {1: "neither"}, {1: "identical"}],
             4: [{1: "only_pred", 2: "only_gt", 3: "identical"}, {2: "neither"}],
             9: [{1: "only_pred", 2: "only_gt", 3: "neither", 4: "identical"}]}


def _want(pred, gt, K, kind):
    res = []
    for c in range(1, K):
        m = O.metric_percase(pred == c, gt == c)
        res.append(m if kind == "acdc" else m[:2])  # utils_synapse.py:12-21 keeps the dice and hd95 of the same three rules
    return res


@pytest.mark.parametrize("K", [2, 4, 9])
@pytest.mark.parametrize("shape", [(6, 28, 30), (26, 34)])
def test_label_metrics_equals_per_class_loop(dev, K, shape):
    for n, scen in enumerate(SCENARIOS[K]):
        pred, gt = _label_pair(shape, K, seed=10 * K + n)
        for c, s in scen.items():
            pred, gt = _apply(pred, gt, c, s)
            assert (pred == c).any() == (s in ("only_pred", "identical")) and (gt == c).any() == (s in ("only_gt", "identical"))
            assert s != "identical" or np.array_equal(pred == c, gt == c)
        tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        for kind in ("acdc", "synapse"):
            want = _want(pred, gt, K, kind)
            for method in ("edt", "pairs", "auto"):
                got = evaluate.label_metrics(tp, tg, K, kind=kind, method=method)
                assert len(got) == K - 1
                for g, w in zip(got, want):
                    assert len(g) == len(w) and g[1] == w[1] and (kind == "synapse" or g[3] == w[3]), (method, g, w)
                    assert all(abs(a - b) < 1e-12 for a, b in zip(g, w)), (method, g, w)


def test_label_metrics_takes_integer_and_bool_labels(dev):
    pred, gt = _label_pair((5, 20, 18), 4, seed=3)
    want = _want(pred, gt, 4, "acdc")
    got = evaluate.label_metrics(torch.from_numpy(pred.astype(np.int64)).to(dev), torch.from_numpy(gt.astype(np.uint8)).to(dev), 4)
    assert all(abs(a - b) < 1e-12 for g, w in zip(got, want) for a, b in zip(g, w))
    got = evaluate.label_metrics(torch.from_numpy(pred == 2).to(dev), torch.from_numpy(gt == 2).to(dev), 2)
    assert all(abs(a - b) < 1e-12 for a, b in zip(got[0], want[1]))


@pytest.mark.parametrize("method", ["edt", "pairs", "auto"])
def test_label_metrics_downloads_do_not_grow_with_classes(dev, method, monkeypatch):
    calls = []
    real = evaluate._download
    monkeypatch.setattr(evaluate, "_download", lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    counts = {}
    for K in (4, 9):
        pred, gt = _label_pair((6, 28, 30), K, seed=K)
        assert all((pred == c).any() and (gt == c).any() for c in range(1, K))
        del calls[:]
        evaluate.label_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), K, method=method)
        counts[K] = len(calls)
    assert counts[4] == counts[9] == 2


def test_volume_wrappers_go_through_label_metrics(dev, monkeypatch):
    """test_single_volume and synapse_test_single_volume score all classes with one label_metrics call"""
    seen = []
    real = evaluate.label_metrics
    monkeypatch.setattr(evaluate, "label_metrics", lambda *a, **k: (seen.append(a[3] if len(a) > 3 else k.get("kind")), real(*a, **k))[1])

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return -(x - torch.linspace(0.2, 0.8, 4, device=x.device).view(1, 4, 1, 1)).abs()

    rng = np.random.default_rng(0)
    image = np.stack([zoom(s, (16 / 6, 16 / 6), order=1) for s in rng.random((4, 6, 6))]).astype(np.float32)
    label = np.clip((image * 4).astype(np.int64), 0, 3).astype(np.float32)
    net = Net().to(dev)
    a = evaluate.test_single_volume(torch.from_numpy(image)[None], torch.from_numpy(label)[None], net, 4, patch_size=(16, 16),
                                    device=dev)
    s = evaluate.synapse_test_single_volume(torch.from_numpy(image)[None], torch.from_numpy(label)[None], net, 4,
                                            patch_size=(16, 16), device=dev)
    assert seen == ["acdc", "synapse"] and len(a) == len(s) == 3 and len(a[0]) == 4 and len(s[0]) == 2
