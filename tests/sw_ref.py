"""Test helper: the numpy float64 restatement of the sliding-window inference (tests/test_sliding_window.py,
tests/test_sliding_window_gpu.py) — it is the specification of csrc/sliding_window.hip — and the bounds both files hold the kernels to.

  * conf within CONF_TOL = 2e-6 of the float64 reference: numpy's own float32 evaluation of the same formula (`reference_f32`
    below: the same additions in the same order) stays within 4.3e-7 of float64 on the cases of tests/test_sliding_window.py, the
    worst being K = 16 with 9 windows on a pixel; that leaves 5x for the device's expf and division.
  * pred equal to the reference except where the reference's own top-2 gap of the blended probability is below GAP_TOL = 2e-5
    (5x the largest gap error, 2 * CONF_TOL, that the conf bound allows); such voxels may be at most 0.5 % of a case.  On those
    cases and seeds the reference alone excludes at most 2 of 512 voxels (the one-window bf16 case, where rounded logits tie
    exactly); every other case stays at or below 0.13 %.  A case that exceeds the cap gets another seed or size, never another cap.
"""
import math

import numpy as np

from tta_ref import unview, view_codes

CONF_TOL, GAP_TOL, EXCLUDED_MAX = 2e-6, 2e-5, 0.005
MAX_WINDOWS = 32


def origins(L, P, overlap):
    """nnU-Net's window origins along an axis of length L for windows of side P"""
    if not 0.0 <= overlap < 1.0:
        raise ValueError(overlap)
    if L <= P:
        return [-((P - L) // 2)]
    N = int(math.ceil((L - P) / (P * (1 - overlap)))) + 1
    if N > MAX_WINDOWS:
        raise ValueError(N)
    return [int(np.round(i * (L - P) / (N - 1))) for i in range(N)]


def weights(P, importance="gaussian"):
    """one factor of the separable importance map: float64 arithmetic, stored as float32 (MONAI's form, sigma_scale = 0.125)"""
    if importance == "constant":
        return np.ones(P, dtype=np.float32)
    assert importance == "gaussian", importance
    i = np.arange(P, dtype=np.float64)
    return np.exp(-0.5 * ((i - (P - 1) / 2) / (0.125 * P)) ** 2).astype(np.float32)


def windows(x, oy, ox, patch, pad_value=0.0, normalize=None):
    """x [n, C, H, W] float32 -> [n * nwy * nwx, C, PH, PW]: numpy slicing and padding; with normalize the float32 expression"""
    n, C, H, W = x.shape
    PH, PW = patch
    out = np.full((n, len(oy), len(ox), C, PH, PW), pad_value, dtype=np.float32)
    for iy, y0 in enumerate(oy):
        for ix, x0 in enumerate(ox):
            ya, yb, xa, xb = max(y0, 0), min(y0 + PH, H), max(x0, 0), min(x0 + PW, W)
            v = x[:, :, ya:yb, xa:xb]
            if normalize is not None:
                v = (v - np.float32(normalize[0])) / np.float32(normalize[1])
            out[:, iy, ix, :, ya - y0:yb - y0, xa - x0:xb - x0] = v
    return out.reshape(n * len(oy) * len(ox), C, PH, PW)


def _blend(stacks, mask, n, oy, ox, wy, wx, size, dtype):
    """acc [n, K, H, W] and wsum [H, W] in `dtype`: windows in ascending (iy, ix), inside a window the views in ascending code"""
    codes = view_codes(mask)
    T, NB, K, PH, PW = stacks.shape
    assert T == len(codes) and NB == n * len(oy) * len(ox)
    H, W = size
    acc, wsum = np.zeros((n, K, H, W), dtype=dtype), np.zeros((H, W), dtype=dtype)
    wmap = (wy.astype(np.float32)[:, None] * wx.astype(np.float32)[None, :]).astype(dtype)  # the product of the two fp32 factors
    st = stacks.reshape(T, n, len(oy), len(ox), K, PH, PW)
    for iy, y0 in enumerate(oy):
        for ix, x0 in enumerate(ox):
            ya, yb, xa, xb = max(y0, 0), min(y0 + PH, H), max(x0, 0), min(x0 + PW, W)
            w = wmap[ya - y0:yb - y0, xa - x0:xb - x0]
            for t, g in enumerate(codes):
                z = unview(st[t, :, iy, ix].astype(dtype), g)
                z = np.exp(z - z.max(axis=1, keepdims=True))
                p = z * (dtype(1) / z.sum(axis=1, keepdims=True))
                acc[:, :, ya:yb, xa:xb] += w * p[:, :, ya - y0:yb - y0, xa - x0:xb - x0]
            wsum[ya:yb, xa:xb] += w  # (once per window: conf = acc / (wsum T) is then a probability)
    return acc, wsum, len(codes)


def reference(stacks, mask, n, oy, ox, wy, wx, size):
    """stacks [T, n * nwy * nwx, K, PH, PW] (any float dtype) -> (class map [n, H, W], the winner's blended probability, the top-2
    gap of the blended probability: inf for K = 1), all float64 arithmetic"""
    acc, wsum, T = _blend(np.asarray(stacks), mask, n, oy, ox, wy, wx, size, np.float64)
    assert (wsum > 0).all()
    prob = acc / (wsum * T)
    am, top = prob.argmax(axis=1), prob.max(axis=1)
    srt = np.sort(prob, axis=1)
    gap = srt[:, -1] - srt[:, -2] if prob.shape[1] > 1 else np.full(top.shape, np.inf)
    return am.astype(np.float64), top, gap


def reference_f32(stacks, mask, n, oy, ox, wy, wx, size):
    """the same formula in numpy float32 (what CONF_TOL is derived from): (class map, conf)"""
    acc, wsum, T = _blend(np.asarray(stacks), mask, n, oy, ox, wy, wx, size, np.float32)
    am = acc.argmax(axis=1)
    best = np.take_along_axis(acc, am[:, None], axis=1)[:, 0]
    return am.astype(np.float64), best / (wsum * np.float32(T))


def hold_to_reference(tag, got_pred, got_conf, want_pred, want_conf, gap):
    """the file's two bounds; returns (largest conf error, number of excluded voxels) after printing them"""
    excluded = gap < GAP_TOL
    err = np.abs(got_conf.astype(np.float64) - want_conf)
    worst = float(err[~excluded].max()) if (~excluded).any() else 0.0
    print(f"{tag}: max |conf - ref| = {worst:.3e}, excluded {int(excluded.sum())} of {excluded.size}, "
          f"{int((got_pred != want_pred).sum())} differ")
    assert excluded.sum() <= EXCLUDED_MAX * excluded.size, (int(excluded.sum()), excluded.size)
    assert np.array_equal(got_pred[~excluded], want_pred[~excluded].astype(np.float32))
    # (where the two leaders are closer than the gap bound either may win, and its probability is the gap below at most)
    assert (err <= CONF_TOL + np.where(excluded, gap, 0.0)).all(), float(err.max())
    return worst, int(excluded.sum())
