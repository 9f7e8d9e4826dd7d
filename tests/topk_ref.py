"""Test helper: the top-k cross-entropy restated in float64 numpy from the definition in include/cenet_hip.h.  Per segment (the
batch, or one image with per_image): l = logsumexp(x) - x_y over the valid pixels, m = max(1, floor(n_valid k / 100)) evaluated
as the C expression (long long)((double)n_valid * (double)k / 100.0) with k a float32, the kept set =
argsort(-l, kind="stable")[:m], the loss the mean of l over it, then the mean over the segments that have a valid pixel.

Beside loss, gradient and kept mask it returns the NEAR-TIE set N of every segment: the valid pixels other than the m-th one
itself whose l lies within DELTA of the m-th largest.  DELTA = 2^-16 is 8 ulp of fp32 at magnitude 16: it covers the handful of
roundings of an fp32 evaluation (max-subtract, expf, the sum, logf, the subtraction) for |logit| < 16, so a pixel outside N has
the same side of the threshold in fp32 as in float64."""
import types

import numpy as np

DELTA = 2.0 ** -16


def pixel_losses(x_f32, target, ignore_index=None):
    """x_f32 [B,K,H,W] (numpy or torch, what the library's input is worth in fp32), target [B,H,W] float ->
    (l float64 [B,H,W], p float64 [B,K,H,W], onehot bool [B,K,H,W], valid bool [B,H,W])"""
    x = np.asarray(x_f32, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    K = x.shape[1]
    d = x - x.max(axis=1, keepdims=True)
    e = np.exp(d)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    onehot = np.stack([t == c for c in range(K)], axis=1)
    valid = onehot.any(axis=1)
    if ignore_index is not None:
        valid &= t != ignore_index
    l = np.maximum(np.log(s[:, 0]) - np.where(onehot, d, 0.0).sum(axis=1), 0.0)
    return l, p, onehot, valid


def kept_count(n_valid, k):
    """m, bit for bit what the device evaluates"""
    return max(1, int(float(n_valid) * float(np.float32(k)) / 100.0)) if n_valid > 0 else 0


def topk_ref(x_f32, target, k=10.0, *, per_image=False, ignore_index=None, gout=1.0):
    """-> namespace: loss (float), grad (float64 [B,K,H,W], times gout), kept / near (bool [B,H,W]: the kept set and N), wgt
    (float64 [B,H,W]), scale (float64 [B,H,W]: 1 / (m_s S_valid) on EVERY pixel of segment s, what a kept pixel's weight would
    be), kept_form (float64 [B,K,H,W]: gout scale (p - onehot), the gradient a pixel has if it is kept), m / n_valid (per segment),
    segments (the index arrays into the flattened [B,H,W] of every segment)"""
    l, p, onehot, valid = pixel_losses(x_f32, target, ignore_index)
    B = l.shape[0]
    flat_l, flat_valid = l.reshape(-1), valid.reshape(-1)
    per = l[0].size
    segments = [np.arange(b * per, (b + 1) * per) for b in range(B)] if per_image else [np.arange(B * per)]
    kept = np.zeros(flat_l.shape, bool)
    near = np.zeros(flat_l.shape, bool)
    scale = np.zeros(flat_l.shape)
    ms, nvs, seg_losses = [], [], []
    for seg in segments:
        idx = seg[flat_valid[seg]]
        m = kept_count(idx.size, k)
        ms.append(m)
        nvs.append(int(idx.size))
        if m == 0:
            continue
        order = idx[np.argsort(-flat_l[idx], kind="stable")]
        kept[order[:m]] = True
        last = order[m - 1]
        close = idx[np.abs(flat_l[idx] - flat_l[last]) < DELTA]
        near[close[close != last]] = True
        seg_losses.append(flat_l[order[:m]].mean())
    s_valid = len(seg_losses)
    for seg, m in zip(segments, ms):
        if m:
            scale[seg] = 1.0 / (m * s_valid)
    loss = float(np.mean(seg_losses)) if seg_losses else 0.0
    scale = scale.reshape(l.shape)
    kept, near = kept.reshape(l.shape), near.reshape(l.shape)
    wgt = np.where(kept, scale, 0.0)
    kept_form = gout * scale[:, None] * (p - onehot)
    return types.SimpleNamespace(loss=loss, grad=np.where(kept[:, None], kept_form, 0.0), kept=kept, near=near, wgt=wgt, scale=scale,
                                 kept_form=kept_form, m=ms, n_valid=nvs, segments=segments, valid=valid)
