"""The case the all-pairs surface distance cannot do: a Synapse-size pair of noise label maps, where nearly every voxel is a border
voxel (about 1.9e13 pairs per class and direction).  The distance transform is linear in the voxels, so `label_metrics` finishes;
one class is checked against scipy at full size (one scipy transform of 148 x 512 x 512 takes tens of seconds, hence one class,
both directions), every class on a 40 x 160 x 160 pair.  No time is asserted."""
import numpy as np
import pytest
import torch

from backend import use_hip
from cenet_amd import _lib, evaluate
from oracle import cenet_oracle as O

K = 9


@pytest.fixture
def hip():
    d = use_hip()
    yield d
    _lib._LIB = None
    _lib._HOSTSIM = False


def _noise_pair(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, K, shape).astype(np.float32), rng.integers(0, K, shape).astype(np.float32)


@pytest.mark.gpu
def test_noise_labels_all_classes_match_per_class_loop(hip):
    pred, gt = _noise_pair((40, 160, 160), 1)
    got = evaluate.label_metrics(torch.from_numpy(pred).to(hip), torch.from_numpy(gt).to(hip), K, method="edt")
    assert len(got) == K - 1
    for c, g in zip(range(1, K), got):
        w = O.metric_percase(pred == c, gt == c)
        assert g[1] == w[1] and g[3] == w[3], (c, g, w)
        assert all(abs(a - b) < 1e-12 for a, b in zip(g, w)), (c, g, w)
    syn = evaluate.label_metrics(torch.from_numpy(pred).to(hip), torch.from_numpy(gt).to(hip), K, kind="synapse", method="edt")
    assert syn == [g[:2] for g in got]


@pytest.mark.gpu
def test_synapse_size_noise_volume_completes_and_matches_scipy(hip):
    pred, gt = _noise_pair((148, 512, 512), 2)
    tp, tg = torch.from_numpy(pred).to(hip), torch.from_numpy(gt).to(hip)
    got = evaluate.label_metrics(tp, tg, K, method="edt")
    torch.cuda.synchronize()
    assert len(got) == K - 1 and all(len(g) == 4 and 0.0 < g[0] < 1.0 and g[1] >= 1.0 and g[3] > 0.0 for g in got)
    c = 3
    a, b = pred == c, gt == c
    d1, d2 = evaluate.surface_distances(tp == c, tg == c, method="edt")
    r1, r2 = O.surface_distances(a, b), O.surface_distances(b, a)
    assert d1.shape == r1.shape and d2.shape == r2.shape and d1.size > 3_000_000
    assert np.array_equal(d1, r1) and np.array_equal(d2, r2)
    assert got[c - 1][1] == float(np.percentile(np.hstack((r1, r2)), 95))
    assert got[c - 1][3] == float(np.mean((r1.mean(), r2.mean())))
