"""Test helper: the numpy / scipy float64 reference of the test-time augmentation (tests/test_tta.py, tests/test_tta_gpu.py) and the
two bounds both files hold the kernels to.

  * conf within 1e-6 of the float64 reference: numpy's own float32 evaluation of the same formula stays within 2e-7 of float64,
    which leaves 5x for the device's expf.
  * pred equal to the reference except where the reference's own top-2 gap of the mean probability is below 1e-5 (5x the largest
    gap error, 2e-6, that the conf bound allows); such voxels may be at most 0.1 % of a case."""
import numpy as np
from scipy.ndimage import zoom

CONF_TOL, GAP_TOL, EXCLUDED_MAX = 1e-6, 1e-5, 0.001


def view_codes(mask):
    return [g for g in range(8) if mask >> g & 1]


def view(x, g):
    v = x
    if g & 4:
        v = v.swapaxes(-1, -2)
    if g & 2:
        v = np.flip(v, -2)
    if g & 1:
        v = np.flip(v, -1)
    return v


def unview(v, g):
    if g & 1:
        v = np.flip(v, -1)
    if g & 2:
        v = np.flip(v, -2)
    if g & 4:
        v = v.swapaxes(-1, -2)
    return v


def zoom0(a, size):
    """scipy's order-0 zoom of one [PH, PW] map to `size`, called as the reference calls it (metrics_eval.py:55)"""
    if a.shape == tuple(size):
        return a
    out = zoom(a, (size[0] / a.shape[0], size[1] / a.shape[1]), order=0)
    assert out.shape == tuple(size)
    return out


def reference(stacks, mask, size):
    """stacks [T, n, K, PH, PW] (any float dtype) -> (class map [n, H, W], the winner's mean probability, the top-2 gap of the mean
    probability: inf where zoom writes its cval and for K = 1), all float64 arithmetic"""
    codes = view_codes(mask)
    assert len(codes) == stacks.shape[0]
    mean = 0.0
    for t, g in enumerate(codes):
        z = unview(stacks[t].astype(np.float64), g)
        z = np.exp(z - z.max(axis=1, keepdims=True))
        mean = mean + z / z.sum(axis=1, keepdims=True)
    mean = mean / len(codes)
    am, top = mean.argmax(axis=1), mean.max(axis=1)
    srt = np.sort(mean, axis=1)
    gap = srt[:, -1] - srt[:, -2] if mean.shape[1] > 1 else np.full(top.shape, np.inf)
    n = am.shape[0]
    pred = np.stack([zoom0(am[b].astype(np.float64), size) for b in range(n)])
    conf = np.stack([zoom0(top[b], size) for b in range(n)])
    inside = np.stack([zoom0(np.ones(am.shape[1:]), size) for b in range(n)]) > 0
    gap = np.where(inside, np.stack([zoom0(gap[b], size) for b in range(n)]), np.inf)
    return pred, conf, gap


def hold_to_reference(tag, got_pred, got_conf, want_pred, want_conf, gap):
    """the file's two bounds; returns (largest conf error, number of excluded voxels) after printing them"""
    excluded = gap < GAP_TOL
    err = np.abs(got_conf.astype(np.float64) - want_conf)
    worst = float(err[~excluded].max()) if (~excluded).any() else 0.0
    print(f"{tag}: max |conf - ref| = {worst:.3e}, excluded {int(excluded.sum())} of {excluded.size}, "
          f"{int((got_pred != want_pred).sum())} of them differ")
    assert excluded.sum() <= EXCLUDED_MAX * excluded.size, (int(excluded.sum()), excluded.size)
    assert np.array_equal(got_pred[~excluded], want_pred[~excluded].astype(np.float32))
    # (where the two leaders are closer than the gap bound, either may win, and its mean probability is the gap below at most)
    assert (err <= CONF_TOL + np.where(excluded, gap, 0.0)).all(), float(err.max())
    assert ((got_pred == want_pred) | excluded).all()
    return worst, int(excluded.sum())


def smooth_volume(shape, seed):
    rng = np.random.default_rng(seed)
    low = rng.random((shape[0], 6, 6))
    return np.stack([zoom(s, (shape[1] / 6, shape[2] / 6), order=1) for s in low]).astype(np.float32)
