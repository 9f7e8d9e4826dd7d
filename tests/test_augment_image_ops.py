"""Composable augmentation of multi-channel images on the device (csrc/augment_image_ops.hip through cenet_augment_image_ops /
cenet_augment_minmax; cenet_amd/data.py DeviceImages, SKIN_OPS, ComposeAugmenter, DeviceTrainLoader(augmenter=...)): every operator
against the scipy / numpy call that specifies it (include/cenet_hip.h), the elastic field against a numpy restatement with the
test's own Philox, chains against the same calls in sequence, the whole augmenter against a host pipeline built from its plan, and
the draw against the distribution of the reference's albumentations Compose (dataset_ham.py:273-281).
Labels: exact, every pixel.  Images: within ONE float32 ulp (np.spacing) of float32(scipy's float64 result) — the fp64 operation
order is scipy's, only the final rounding can differ; the share of bit-identical values is printed, not asserted.  The field: 1e-15
absolute.  Outputs sit between sentinels, the pools are compared before and after.
`sim` runs the kernel sources on the host SIMT checker, `hip` (marker gpu) the gfx950 kernels."""
import functools
import random

import numpy as np
import pytest
import torch
from scipy import ndimage

from backend import dev  # noqa: F401
from cenet_amd import data as D, kern

GUARD, SENT_F, SENT_B, SENT_D = 512, -777.0, 0xAB, -555.0
SHAPES = [(17, 33), (40, 36)]  # no multiples of the 8 x 32 tile; the first is narrower than two tiles
EXACT = {"equal": 0, "total": 0}


def _images(shape, C, seed, dev, count=4, classes=2):
    rng = np.random.default_rng(seed)
    samples = [((rng.random((C, *shape)) * 255).astype(np.float32), rng.integers(0, classes, shape).astype(np.uint8))
               for _ in range(count)]
    return samples, D.DeviceImages(samples, dev)


# ---- the specification: scipy, and numpy restatements where scipy has no call ---------------------------------------------------------
def philox_np(ctr, key):
    """Philox4x32-10 on uint64 arrays holding 32-bit words: ctr [n, 4], key [n, 2] -> [n, 4]"""
    c = [ctr[:, k].astype(np.uint64) for k in range(4)]
    k0, k1 = key[:, 0].astype(np.uint64), key[:, 1].astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=1)


def full_kernel(half):
    half = np.asarray(half, dtype=np.float64)
    return np.concatenate([half[:0:-1], half])


@functools.lru_cache(maxsize=None)
def _field(H, W, k0, k1, half):
    w = full_kernel(half)
    g = []
    for f in range(2):
        ctr = np.zeros((H * W, 4), dtype=np.uint64)
        ctr[:, 0], ctr[:, 1] = np.arange(H * W), f
        x = philox_np(ctr, np.tile(np.array([[k0, k1]], dtype=np.uint64), (H * W, 1)))[:, 0]
        u = ((x.astype(np.float64) + 0.5) / 2.0 ** 31 - 1.0).reshape(H, W)
        g.append(ndimage.correlate1d(ndimage.correlate1d(u, w, 0, mode="constant", cval=0), w, 1, mode="constant", cval=0))
    return np.stack(g)


def field_np(H, W, k0, k1, half):
    """g [2, H, W] of include/cenet_hip.h for a key and the kernel's weights at distance 0 .. radius"""
    return _field(H, W, int(k0), int(k1), tuple(float(v) for v in half))


def host_op(img32, lab, op, fw):
    """one operator of the table in include/cenet_hip.h on (float32 image [C, H, W], uint8 label) -> (float64 image, uint8 label)"""
    kind, a = op[0], op[1:]
    a64 = img32.astype(np.float64)
    C, H, W = a64.shape
    if kind == "copy":
        return a64, lab
    if kind == "flip_ud":
        return a64[:, ::-1], lab[::-1]
    if kind == "flip_lr":
        return a64[:, :, ::-1], lab[:, ::-1]
    if kind == "affine":
        return (np.stack([ndimage.affine_transform(a64[c], a[0], a[1], order=1, mode=a[2], cval=0) for c in range(C)]),
                ndimage.affine_transform(lab, a[0], a[1], order=0, mode=a[2], cval=0))
    if kind == "blur":
        w = full_kernel(D.blur_weights(a[0])[1] if np.ndim(a[0]) == 0 else a[0])
        return np.stack([ndimage.correlate1d(ndimage.correlate1d(a64[c], w, 0, mode="mirror"), w, 1, mode="mirror")
                         for c in range(C)]), lab
    if kind == "brightness_contrast":
        return np.clip(a[0] * a64 + a[1], a[2], a[3]), lab
    if kind == "elastic":
        g = field_np(H, W, a[1], a[2], fw)
        i, j = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
        co = [i + a[0] * g[0], j + a[0] * g[1]]
        return (np.stack([ndimage.map_coordinates(a64[c], co, order=1, mode=a[3], cval=0) for c in range(C)]),
                ndimage.map_coordinates(lab, co, order=0, mode=a[3], cval=0))
    raise AssertionError(kind)


def host_chain(img32, lab, chain, fw=None):
    """the operators in sequence, rounded to float32 between stages as the work buffers are"""
    for op in chain:
        img, lab = host_op(img32, lab, op, fw)
        img32 = img.astype(np.float32)
    return img32, np.ascontiguousarray(lab)


def decode(tab_row, dp_rows):
    """a sample's chain back from its plan rows (copies dropped)"""
    names = {v: k for k, v in kern.AUG_IMAGE_OPS.items()}
    chain = []
    for word, q in zip(tab_row[1:], dp_rows):
        kind, mode = names[int(word) & 255], "mirror" if int(word) & kern.AUG_IMAGE_MIRROR else "constant"
        if kind == "affine":
            chain.append((kind, q[0:4].reshape(2, 2), q[4:6], mode))
        elif kind == "blur":
            chain.append((kind, q[1:2 + int(q[0])]))
        elif kind == "brightness_contrast":
            chain.append((kind, *q[0:4]))
        elif kind == "elastic":
            chain.append((kind, q[0], int(q[1]), int(q[2]), mode))
        elif kind != "copy":
            chain.append((kind,))
    return chain


# ---- the device side, between sentinels ------------------------------------------------------------------------------------------------
def _guarded(n, value, dtype, dev):
    full = torch.full((n + 2 * GUARD,), value, dtype=dtype, device=dev)
    return full, full[GUARD:GUARD + n]


def _untouched(full, n, value):
    return bool((full[:GUARD] == value).all()) and bool((full[GUARD + n:] == value).all())


def run_ops(im, plan, expect_error=False):
    """cenet_augment_image_ops on guarded buffers -> (image [B, C, H, W] float32, label [B, H, W] uint8, field [B, 2, H, W] float64 or
    None) as numpy; checks the guards, the pools, that the other work buffer's guards hold too and that out_lab is the label"""
    tab, dp, fw = plan
    dev = im.device
    B, S = tab.shape[0], tab.shape[1] - 1
    C0, H0, W0 = im.channels, im.height, im.width
    ni, nl, nf = B * C0 * H0 * W0, B * H0 * W0, B * 2 * H0 * W0
    gi = [_guarded(ni, SENT_F, torch.float32, dev) for _ in range(2)]
    gl = [_guarded(nl, SENT_B, torch.uint8, dev) for _ in range(2)]
    gf, go = _guarded(nf, SENT_D, torch.float64, dev), _guarded(nl, SENT_F, torch.float32, dev)
    pools = im.pool_img.clone(), im.pool_lab.clone()
    up = [None if a is None else torch.from_numpy(a).to(dev) for a in (tab, dp, fw)]
    args = (im.pool_img, im.pool_lab, tab, dp, up[0], up[1], fw, up[2], gf[1] if fw is not None else None, [g[1] for g in gi],
            [g[1] for g in gl], go[1], len(im), C0, H0, W0, B, S)
    if expect_error:
        with pytest.raises(RuntimeError, match="cenet_augment_image_ops failed with error code"):
            kern.augment_image_ops(*args)
        assert all(bool((g[0] == SENT_F).all()) for g in gi + [go]) and all(bool((g[0] == SENT_B).all()) for g in gl)
        assert bool((gf[0] == SENT_D).all())
        assert torch.equal(pools[0], im.pool_img) and torch.equal(pools[1], im.pool_lab)
        return None
    r = kern.augment_image_ops(*args)
    assert r == S & 1
    assert torch.equal(pools[0], im.pool_img) and torch.equal(pools[1], im.pool_lab)
    assert all(_untouched(g[0], ni, SENT_F) for g in gi) and all(_untouched(g[0], nl, SENT_B) for g in gl)
    assert _untouched(gf[0], nf, SENT_D) and _untouched(go[0], nl, SENT_F)
    img = gi[r][1].cpu().numpy().reshape(B, C0, H0, W0)
    lab = gl[r][1].cpu().numpy().reshape(B, H0, W0)
    assert np.array_equal(go[1].cpu().numpy().reshape(B, H0, W0), lab.astype(np.float32))
    return img, lab, (gf[1].cpu().numpy().reshape(B, 2, H0, W0) if fw is not None else None)


def check(gi, gl, want, what):
    wi, wl = want
    assert gi.dtype == np.float32 and gl.dtype == np.uint8 and gi.shape == wi.shape and gl.shape == wl.shape, what
    assert np.array_equal(gl, wl), (what, int((gl != wl).sum()))
    wi32 = np.asarray(wi, dtype=np.float32)
    err = np.abs(gi.astype(np.float64) - wi32.astype(np.float64))
    assert (err <= np.spacing(np.abs(wi32)).astype(np.float64)).all(), (what, float(err.max()))
    EXACT["equal"] += int((gi == wi32).sum())
    EXACT["total"] += gi.size


def report(what):
    print(f"{what}: {EXACT['equal']} of {EXACT['total']} float32 values bit-identical "
          f"({100.0 * EXACT['equal'] / max(EXACT['total'], 1):.4f} %)")
    EXACT.update(equal=0, total=0)


def rot(shape, deg, mode, shift=(0.0, 0.0)):
    a = np.deg2rad(deg)
    return ("affine", *D.centred_affine([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], shape, shift=shift), mode)


def single_ops(shape, mode):
    """the operators that take no field, alone; the affines reach past -(n - 1) and 2 (n - 1), where the mirror fold wraps more than
    once, and sit on half-pixel ties under the identity"""
    H, W = shape
    return [
        ("copy",), ("flip_ud",), ("flip_lr",),
        ("affine", np.eye(2), np.array([1.0, 0.5]), mode),
        ("affine", np.eye(2), np.array([0.0, -0.5]), mode),
        rot(shape, 27.0, mode),
        rot(shape, -30.0, mode, shift=(2.7 * H, -3.4 * W)),                       # whole periods away on both sides
        ("affine", *D.centred_affine([[7.0, 0.0], [0.0, 6.0]], shape), mode),    # coordinates from -3 n to 4 n
        ("affine", *D.centred_affine([[1 / 0.6, 0.3], [0, 1 / 1.7]], shape, shift=(-5.25 * H, 4.5 * W)), mode),
        ("affine", np.eye(2), np.array([-2.0 * (H - 1), 4.0 * (W - 1)]), mode),   # exactly on the fold's period
        ("blur", 3), ("blur", 5), ("blur", 7), ("blur", D.gaussian_weights(4.0)[1]),  # radius 1, 2, 3 and 16
        ("brightness_contrast", 1.17, -31.5, 0.0, 255.0), ("brightness_contrast", 0.8, 40.0, 20.0, 200.0),
        ("brightness_contrast", 3.0, 0.0, 0.0, 255.0),
    ]


# ---- 1. every operator alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_each_operator_alone_equals_scipy(dev, shape, C):
    samples, im = _images(shape, C, 11, dev, classes=9 if C == 1 else 2)  # (one-channel cases carry 9 classes)
    aug = D.ComposeAugmenter(im, seed=0)
    ops = single_ops(shape, "constant") + [op for op in single_ops(shape, "mirror") if op[0] == "affine"]
    order = [2, 0, 3]
    for k in range(0, len(ops), 3):  # B = 3, a different operator per sample
        chains = [[ops[(k + b) % len(ops)]] for b in range(3)]
        img, lab, _ = run_ops(im, aug.plan(order, chains))
        for b, i in enumerate(order):
            check(img[b], lab[b], host_chain(*samples[i], chains[b]), (chains[b][0][0], k + b, shape, C))
    report(f"single operators {shape} C={C}")


# ---- 2. the elastic field and the warp -----------------------------------------------------------------------------------------------
def test_numpy_philox_equals_the_device_generator(dev):
    rows = [(0, 0, 0, 0, 0, 0), (5, 1, 0, 0, 12345, 4000000000), (40 * 36 - 1, 1, 0, 0, 0xFFFFFFFF, 1), (1023 * 1024 + 1023, 0, 0, 0, 7, 9)]
    ck = torch.tensor(rows, dtype=torch.int64).to(dev)
    out = torch.full((len(rows), 4), -1, dtype=torch.int64).to(dev)
    kern.philox4x32_10(ck, out)
    a = np.array(rows, dtype=np.uint64)
    assert np.array_equal(out.cpu().numpy().astype(np.uint64), philox_np(a[:, :4], a[:, 4:]))


FIELDS = [((17, 33), 1.5, 6), ((40, 36), 1.5, 6), ((24, 20), 12.0, 48), ((40, 36), 50.0, 200)]


@pytest.mark.parametrize("shape,sigma,radius", FIELDS, ids=lambda v: str(v).replace(" ", ""))
def test_elastic_field_and_warp_equal_the_scipy_restatement(dev, shape, sigma, radius):
    samples, im = _images(shape, 3, 23, dev)
    aug = D.ComposeAugmenter(im, seed=0)
    fw = D.gaussian_weights(sigma, 4.0)[1]
    assert len(fw) == radius + 1
    keys = [(12345, 4000000000), (12346, 4000000000), (0xFFFFFFFF, 0)]
    order = [1, 3, 0]
    moved = {}
    for alpha, mode in [(1.0, "mirror"), (30.0, "constant"), (200.0, "mirror"), (200.0, "constant")]:
        # (sample 1 has no elastic stage: its part of the scratch stays as it was)
        chains = [[("elastic", alpha, *keys[0], mode)], [("flip_ud",)], [("flip_lr",), ("elastic", alpha, *keys[2], mode)]]
        plan = aug.plan(order, chains, field=(sigma, 4.0))
        assert np.array_equal(plan[2], fw)
        img, lab, g = run_ops(im, plan)
        for b in (0, 2):
            want = field_np(*shape, *chains[b][-1][2:4], fw)
            err = np.abs(g[b] - want).max()
            print(f"field {shape} sigma={sigma}: max |g| {np.abs(want).max():.3e}, max error {err:.3e}, "
                  f"{int((g[b] == want).sum())} of {want.size} exact")
            assert err <= 1e-15, err
        assert (g[1] == SENT_D).all()
        for b, i in enumerate(order):
            check(img[b], lab[b], host_chain(*samples[i], chains[b], fw), ("elastic", alpha, mode, b))
        moved[alpha] = float((lab[0] != samples[order[0]][1]).mean())
        again = run_ops(im, plan)
        assert all(np.array_equal(x, y) for x, y in zip((img, lab, g), again))  # no atomics: bit-identical
    report(f"elastic {shape} sigma={sigma}")
    print(f"label pixels moved: {moved}")
    if sigma < 50.0:  # (the preset's field on a 40 x 36 image moves a pixel by less than its width even at alpha = 200)
        assert moved[200.0] > 0.1, moved
    a = run_ops(im, aug.plan(order, [[("elastic", 1.0, *keys[0], "mirror")]] * 3, field=(sigma, 4.0)))[2]
    b = run_ops(im, aug.plan(order, [[("elastic", 1.0, *keys[1], "mirror")]] * 3, field=(sigma, 4.0)))[2]
    assert np.array_equal(a[0], a[1]) and not np.array_equal(a[0], b[0]) and np.abs(a[0] - b[0]).max() > 1e-6


# ---- 3. chains -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_chains_equal_the_scipy_calls_in_sequence(dev, shape, C):
    samples, im = _images(shape, C, 13, dev, classes=9 if C == 1 else 2)
    aug = D.ComposeAugmenter(im, seed=0)
    field = (1.5, 4.0)
    fw = D.gaussian_weights(*field)[1]
    el = ("elastic", 30.0, 77, 99, "mirror")
    eight = [rot(shape, 25.0, "mirror"), ("flip_lr",), ("flip_ud",), ("brightness_contrast", 1.1, 12.0, 0.0, 255.0), ("blur", 5), el,
             ("affine", *D.centred_affine([[1 / 1.3, 0], [0, 1 / 0.7]], shape), "constant"), ("blur", 3)]
    batches = {
        8: [eight,                                                              # elastic in the middle, S even
            [("blur", 7), ("blur", 3), rot(shape, -30.0, "constant"), ("copy",), rot(shape, 14.0, "mirror")],  # padded with copies
            []],                                                                # no op at all: gathered from the pools unchanged
        7: [eight[:3] + [el] + eight[3:5] + [("flip_ud",)],                     # elastic in the middle, S odd
            [("flip_lr",)],
            [("elastic", 200.0, 5, 6, "constant"), ("brightness_contrast", 0.9, -20.0, 0.0, 255.0)]],
    }
    order = [3, 1, 1]
    for S, chains in batches.items():
        plan = aug.plan(order, chains, field=field)
        assert plan[0].shape == (3, 1 + S) and plan[1].shape == (3, S, 32)
        img, lab, _ = run_ops(im, plan)  # (run_ops holds the result to buffer S & 1)
        for b, i in enumerate(order):
            check(img[b], lab[b], host_chain(*samples[i], chains[b], fw), ("chain", S, b))
            check(img[b], lab[b], host_chain(*samples[i], decode(plan[0][b], plan[1][b]), fw), ("decoded chain", S, b))
    report(f"chains {shape} C={C}")


# ---- 4. min-max ----------------------------------------------------------------------------------------------------------------------
def minmax_np(x):
    mn, mx = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
    out = (x - mn) / ((mx - mn) + np.float32(1e-8))
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("B,n", [(3, 3 * 17 * 33), (1, 3 * 224 * 224)])
def test_minmax_equals_the_numpy_float32_restatement(dev, B, n):
    rng = np.random.default_rng(4)
    x = (rng.random((B, n)) * 255).astype(np.float32)
    if B == 3:
        x[1] = x[1] * np.float32(0.01) - np.float32(3.0)  # samples that differ in range
        x[2] = np.float32(41.5)                            # a constant sample: 0 / 1e-8 = 0
    else:
        x[0, -1], x[0, n // 2] = np.float32(-12.0), np.float32(300.0)  # the extremes in the last and in a middle workgroup's share
    full_x, xs = _guarded(B * n, SENT_F, torch.float32, dev)
    xs.copy_(torch.from_numpy(x).reshape(-1))
    full_y, ys = _guarded(B * n, SENT_F, torch.float32, dev)
    part = torch.full((B * 2 * kern.AUG_MINMAX_PARTS,), SENT_F, dtype=torch.float32, device=dev)
    kern.augment_minmax(xs, ys, part, B, n)
    want = minmax_np(x)
    got = ys.cpu().numpy().reshape(B, n)
    assert _untouched(full_y, B * n, SENT_F) and np.array_equal(xs.cpu().numpy().reshape(B, n), x)
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    if B == 3:
        assert (got[2] == 0).all() and got[0].min() == 0 and got[0].max() <= 1
    kern.augment_minmax(xs, xs, part, B, n)  # in place
    assert np.array_equal(xs.cpu().numpy().reshape(B, n), want) and _untouched(full_x, B * n, SENT_F)


# ---- 5. the augmenter end to end ----------------------------------------------------------------------------------------------------
def host_pipeline(samples, plan, minmax):
    tab, dp, fw = plan
    imgs, labs = [], []
    for b in range(tab.shape[0]):
        img, lab = host_chain(*samples[int(tab[b, 0])], decode(tab[b], dp[b]), fw)
        imgs.append(img)
        labs.append(lab.astype(np.float32))
    imgs = np.stack(imgs)
    return (minmax_np(imgs.reshape(len(imgs), -1)).reshape(imgs.shape) if minmax else imgs), np.stack(labs)


@pytest.mark.parametrize("minmax", [False, True], ids=["plain", "minmax"])
def test_compose_augmenter_equals_the_host_pipeline_of_its_plan(dev, minmax):
    samples, im = _images((40, 36), 3, 17, dev, count=6)
    seen = set()
    for seed in range(4):
        aug = D.ComposeAugmenter(im, minmax=minmax, seed=seed)
        indices = [int(i) for i in np.random.default_rng(seed).permutation(6)]
        plan = aug.draw(indices)
        seen |= {n for p in aug.picked for n in p}
        out = aug.apply(plan)
        assert out["image"].shape == (6, 3, 40, 36) and out["image"].dtype == torch.float32
        assert out["label"].shape == (6, 40, 36) and out["label"].dtype == torch.float32
        wi, wl = host_pipeline(samples, plan, minmax)
        assert np.array_equal(out["label"].cpu().numpy(), wl)
        gi = out["image"].cpu().numpy()
        if minmax:
            assert gi.min() >= 0.0 and gi.max() <= 1.0
        for b in range(6):  # (the same one-ulp bound after the min-max: it is float32 arithmetic, identical on identical inputs)
            check(gi[b], wl[b].astype(np.uint8), (wi[b], wl[b].astype(np.uint8)), ("augmenter", seed, b))
    report(f"augmenter minmax={minmax}")
    assert seen == {n for n, _ in D.SKIN_OPS}  # every transform of the pipeline took part


# ---- 6. the draw ---------------------------------------------------------------------------------------------------------------------
def test_draw_follows_the_pipelines_distribution():
    samples, im = _images((40, 36), 3, 1, torch.device("cpu"), count=2)
    state = random.getstate(), np.random.get_state()
    indices = [0, 1] * 2000
    aug = D.ComposeAugmenter(im, seed=99)
    tab, dp, fw = aug.draw(indices)
    picked = aug.picked
    twin = D.ComposeAugmenter(im, seed=99).draw(indices)
    assert np.array_equal(tab, twin[0]) and np.array_equal(dp, twin[1]) and np.array_equal(fw, twin[2])
    assert not np.array_equal(dp, D.ComposeAugmenter(im, seed=100).draw(indices)[1])
    assert random.getstate() == state[0]
    now = np.random.get_state()
    assert now[0] == state[1][0] and np.array_equal(now[1], state[1][1]) and now[2:] == state[1][2:]

    names = [n for n, _ in D.SKIN_OPS]
    prob = {n: p["p"] for n, p in D.SKIN_OPS}
    assert names == ["rotate", "flip_lr", "flip_ud", "brightness_contrast", "blur", "elastic"]
    assert prob == {"rotate": 0.5, "flip_lr": 0.5, "flip_ud": 0.5, "brightness_contrast": 0.2, "blur": 0.3, "elastic": 0.3}
    N = len(indices)
    assert tab.shape[0] == N and len(picked) == N and tab.shape[1] <= 1 + len(names)
    assert np.array_equal(tab[:, 0], indices)
    for n in names:
        f = sum(n in p for p in picked) / N
        assert abs(f - prob[n]) <= 5 * np.sqrt(prob[n] * (1 - prob[n]) / N), (n, f)
    rank = {n: k for k, n in enumerate(names)}
    assert all(list(p) == sorted(set(p), key=rank.get) for p in picked)  # always SKIN_OPS's order, no op twice

    code, mirror = kern.AUG_IMAGE_OPS, kern.AUG_IMAGE_MIRROR
    assert np.array_equal(fw, D.gaussian_weights(50.0, 4.0)[1]) and len(fw) == 201
    ks, keys = [], set()
    for b, p in enumerate(picked):
        assert (tab[b, 1 + len(p):] == 0).all() and not dp[b, len(p):].any()
        for s, n in enumerate(p):
            word, q = int(tab[b, 1 + s]), dp[b, s]
            if n in ("flip_ud", "flip_lr"):
                assert word == code[n] and not q.any()
            elif n == "rotate":
                assert word == code["affine"] + mirror
                m, off = q[0:4].reshape(2, 2), q[4:6]
                ctr = (np.array([40, 36]) - 1) / 2
                assert np.abs(ctr - m @ ctr - off).max() <= 1e-9
                assert abs(np.rad2deg(np.arctan2(m[0, 1], m[0, 0]))) <= 30 and np.allclose(m @ m.T, np.eye(2), atol=1e-12)
                assert m[1, 0] == -m[0, 1] and m[0, 0] == m[1, 1]
            elif n == "brightness_contrast":
                assert word == code[n] and 0.8 <= q[0] <= 1.2 and abs(q[1]) <= 0.2 * 255 and q[2] == 0.0 and q[3] == 255.0
            elif n == "blur":
                k = 2 * int(q[0]) + 1
                ks.append(k)
                assert word == code["blur"] and k in (3, 5, 7)
                sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
                x = np.arange(-(k // 2), k // 2 + 1)
                w = np.exp(-0.5 * x ** 2 / sigma ** 2)
                assert np.allclose(q[1:2 + k // 2], (w / w.sum())[k // 2:], rtol=1e-14, atol=0) and not q[2 + k // 2:].any()
                assert abs(q[1] + 2 * q[2:2 + k // 2].sum() - 1.0) <= 1e-15
            else:
                assert n == "elastic" and word == code["elastic"] + mirror and q[0] == 1.0
                assert all(0 <= v < 2 ** 32 and v == int(v) for v in q[1:3])
                keys.add((q[1], q[2]))
    assert set(ks) == {3, 5, 7} and all(abs(ks.count(k) / len(ks) - 1 / 3) <= 5 * np.sqrt(2 / 9 / len(ks)) for k in (3, 5, 7))
    assert len(keys) == sum("elastic" in p for p in picked)  # a fresh key per sample


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(dev):
    samples, im = _images((17, 33), 3, 3, dev)
    aug = D.ComposeAugmenter(im, seed=0)
    field = (1.5, 4.0)
    el = ("elastic", 30.0, 1, 2, "mirror")
    ok = aug.plan([0, 3], [[("flip_ud",), el], [("blur", 5), ("brightness_contrast", 1.1, 3.0, 0.0, 255.0)]], field=field)
    assert run_ops(im, ok) is not None
    code = kern.AUG_IMAGE_OPS

    def with_word(word):
        tab, dp, fw = ok[0].copy(), ok[1].copy(), ok[2]
        tab[1, 2] = word
        return tab, dp, fw

    def with_dp(b, s, k, v):
        tab, dp, fw = ok[0].copy(), ok[1].copy(), ok[2]
        dp[b, s, k] = v
        return tab, dp, fw

    def with_index(n):
        tab, dp, fw = ok[0].copy(), ok[1].copy(), ok[2]
        tab[0, 0] = n
        return tab, dp, fw

    bad = {
        "unknown op": with_word(7),
        "negative op word": with_word(-1),
        "stray bit 9": with_word(code["affine"] + 512),
        "stray high bits": with_word(code["copy"] + 65536),
        "mode bit on an op without a mode": with_word(code["blur"] + kern.AUG_IMAGE_MIRROR),
        "S > 8": aug.plan([0, 3], [[("copy",)] * 9, []]),
        "blur radius 17": aug.plan([0, 3], [[], [("blur", D.gaussian_weights(4.2)[1])]]),
        "blur radius 2.5": with_dp(1, 0, 0, 2.5),
        "blur radius -1": with_dp(1, 0, 0, -1.0),
        "field radius 257": aug.plan([0, 3], [[el], []], field=(64.25, 4.0)),
        "a second elastic stage": aug.plan([0, 3], [[el, ("flip_lr",), el], []], field=field),
        "key word 2^32": with_dp(0, 1, 1, 2.0 ** 32),
        "key word -1": with_dp(0, 1, 2, -1.0),
        "lo > hi": with_dp(1, 1, 2, 255.5),
        "sample index N": with_index(4),
        "sample index -1": with_index(-1),
    }
    assert len(bad["field radius 257"][2]) == 258 and bad["S > 8"][0].shape == (2, 10)
    assert len(aug.plan([0, 3], [[el], []], field=(64.0, 4.0))[2]) == 257
    for what, plan in bad.items():
        run_ops(im, plan, expect_error=True)
    assert run_ops(im, ok) is not None  # (and the library still runs the good plan)


def test_refused_shapes(dev):
    """C outside 1..4 and H or W outside 1..1024 straight at the entry point (the wrapper's size assertions would come first)"""
    from cenet_amd import _lib
    tab, dp = np.zeros((1, 2), dtype=np.int64), np.zeros((1, 1, 32), dtype=np.float64)
    t = [torch.zeros(64, dtype=dt, device=dev) for dt in (torch.float32, torch.uint8, torch.int64, torch.float64)]
    wi = [torch.full((64,), SENT_F, dtype=torch.float32, device=dev) for _ in range(2)]
    wl = [torch.full((64,), SENT_B, dtype=torch.uint8, device=dev) for _ in range(2)]

    def call(N, C, H, W):
        return _lib.lib().cenet_augment_image_ops(
            t[0].data_ptr(), t[1].data_ptr(), tab.ctypes.data, dp.ctypes.data, t[2].data_ptr(), t[3].data_ptr(), None, None, 0, None,
            wi[0].data_ptr(), wl[0].data_ptr(), wi[1].data_ptr(), wl[1].data_ptr(), None, N, C, H, W, 1, 1, kern.stream())

    for N, C, H, W in [(1, 0, 4, 4), (1, 5, 2, 2), (1, 1, 0, 4), (1, 1, 4, 0), (1, 1, 1025, 1), (1, 1, 1, 1025), (0, 1, 4, 4)]:
        assert call(N, C, H, W) != 0, (N, C, H, W)
    assert all(bool((a == SENT_F).all()) for a in wi) and all(bool((a == SENT_B).all()) for a in wl)
    assert call(1, 4, 4, 4) == 0 and bool((wi[1] == 0).all()) and bool((wi[0] == SENT_F).all())


# ---- 8. the loader -------------------------------------------------------------------------------------------------------------------
def test_loader_with_the_augmenter_yields_what_the_augmenter_yields(dev):
    samples, im = _images((17, 33), 3, 19, dev, count=7)
    im.names = [f"s{i}" for i in range(7)]
    state = random.getstate()
    loader = D.DeviceTrainLoader(im, None, batch_size=3, shuffle=True, generator=torch.Generator().manual_seed(5),
                                 augmenter=D.ComposeAugmenter(im, seed=8))
    twin = D.ComposeAugmenter(im, seed=8)
    assert loader.aug is not None and not isinstance(loader.aug, D.DeviceAugmenter) and len(loader) == 3 and len(im) == 7
    seen = []
    for _ in range(2):
        for batch in loader:
            idx = [int(n[1:]) for n in batch["case_name"]]
            want = twin(idx)
            assert loader.aug.picked == twin.picked
            assert torch.equal(batch["image"], want["image"]) and torch.equal(batch["label"], want["label"])
            assert batch["image"].shape == (len(idx), 3, 17, 33) and batch["label"].shape == (len(idx), 17, 33)
            seen.append(sorted(idx))
    assert sorted(i for s in seen[:3] for i in s) == list(range(7)) and seen[:3] != seen[3:]
    assert random.getstate() == state


def test_device_images_from_arrays():
    rng = np.random.default_rng(0)
    X, Y = rng.random((3, 3, 5, 6)), (rng.random((3, 1, 5, 6)) > 0.5).astype(np.float64)
    im = D.DeviceImages.from_arrays(X, Y, "cpu", names=["a", "b", "c"])
    assert (len(im), im.channels, im.height, im.width, im.names) == (3, 3, 5, 6, ["a", "b", "c"])
    assert np.array_equal(im.pool_img.numpy().reshape(3, 3, 5, 6), np.uint8(X * 255).astype(np.float32))
    assert np.array_equal(im.pool_lab.numpy().reshape(3, 5, 6), Y[:, 0].astype(np.uint8))
    with pytest.raises(AssertionError):
        D.DeviceImages([(np.zeros((5, 6, 3)), np.zeros((5, 6)))], "cpu")  # channels last
