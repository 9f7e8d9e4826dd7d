"""Test helper: the cases tests/test_dist_maps.py and tests/test_dist_loss.py share — shapes, label maps, logits and the
scipy oracle of the boundary-distance maps.  Everything is computed once per shape and handed out read-only."""
import functools

import numpy as np
import torch
from scipy.ndimage import distance_transform_edt

from test_ccl import _blobs

# (B, K, H, W): H = 1 and W = 1; widths below, above and no multiple of the x pass's 64-column chunk; P H (P = 2 B (K-1) planes:
# every mask and its complement) from 2 to 528 rows, below and above the x pass's 128-row tile; K = 2 and K = 9
SHAPES = [(1, 2, 1, 5), (2, 3, 7, 1), (3, 4, 9, 11), (2, 4, 30, 70), (1, 3, 50, 150), (5, 2, 33, 33), (2, 9, 17, 33)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _frozen(a):
    a.setflags(write=False)
    return a


def _pattern(shape, seed):
    """class ids [B,H,W]: one smooth blob pattern per foreground class, each from its own seed, later classes on top"""
    B, K, H, W = shape
    vol = np.zeros((B, H, W), np.float32)
    for c in range(1, K):
        vol[_blobs((B, H, W), seed + c)] = c
    return vol


@functools.lru_cache(maxsize=None)
def labels(shape):
    return _frozen(_pattern(shape, sum(shape)))


@functools.lru_cache(maxsize=None)
def pred_pattern(shape):
    return _frozen(_pattern(shape, 7 + sum(shape)))


@functools.lru_cache(maxsize=None)
def logits(shape):
    """fp32 [B,K,H,W]: 6 onehot(prediction pattern) + 0.5 randn — every probability far from the threshold 1/2 (the noise
    takes the seed after the ones the pattern's K - 1 classes took)"""
    B, K, H, W = shape
    pat = torch.from_numpy(pred_pattern(shape).copy()).long()
    onehot = torch.nn.functional.one_hot(pat, K).permute(0, 3, 1, 2).float()
    noise = torch.randn(B, K, H, W, generator=torch.Generator().manual_seed(7 + sum(shape) + K))
    return _frozen((6.0 * onehot + 0.5 * noise).numpy())


def logits_as(shape, dtype):
    """the logits a case feeds the library, and what they are worth in fp32 (bf16: the rounded values)"""
    x = torch.from_numpy(logits(shape).copy()).to(dtype)
    return x, x.float()


def half_map(m):
    """int64 squared distance of every pixel of the boolean plane m to the nearest pixel outside m (0 outside m), from the
    INDICES of scipy's transform — exact integers; m must have a pixel outside"""
    d, idx = distance_transform_edt(m, return_indices=True)
    y, x = np.indices(m.shape)
    d2 = (idx[0] - y).astype(np.int64) ** 2 + (idx[1] - x).astype(np.int64) ** 2
    assert np.array_equal(d2, np.rint(d * d).astype(np.int64))
    return d2


def degenerate(m):
    return not m.any() or bool(m.all())


def boundary_map(m):
    """the boundary-distance map of one plane: inside m the squared distance to the nearest pixel outside, outside m to the
    nearest pixel of m; zeros for an empty or full plane"""
    if degenerate(m):
        return np.zeros(m.shape, np.int64)
    return half_map(m) + half_map(~m)


def maps_of(masks):
    """masks [B,K-1,H,W] bool -> int32 maps"""
    return np.stack([np.stack([boundary_map(p) for p in img]) for img in masks]).astype(np.int32)


def label_masks(lab, K):
    return np.stack([lab == c for c in range(1, K)], axis=1)


def pred_masks(x_f32):
    """x_f32: torch fp32 [B,K,H,W] -> {softmax_c > 1/2} for c >= 1, in float64"""
    p = torch.softmax(x_f32.double(), dim=1)
    return (p[:, 1:] > 0.5).numpy()


@functools.lru_cache(maxsize=None)
def label_maps(shape):
    return _frozen(maps_of(label_masks(labels(shape), shape[1])))


@functools.lru_cache(maxsize=None)
def pred_maps(shape, dtype=torch.float32):
    return _frozen(maps_of(pred_masks(logits_as(shape, dtype)[1])))
