"""Composable slice augmentation on the device (csrc/augment_ops.hip through cenet_augment_ops / cenet_philox4x32_10;
cenet_amd/data.py SegAugmenter, SYNAPSE_OPS, DeviceTrainLoader(augmenter=...)): every operator against the scipy call that
specifies it (include/cenet_hip.h), the generator against the published Random123 vectors, chains against the same calls in
sequence, the whole augmenter against a host pipeline built from its plan, and the draw against the distribution of the
reference's SomeOf((0, 4), ..., random_order=True) (dataset_synapse.py:86-97).
Labels: exact, every pixel.  Images: within 1e-6 * max(1, |v|) (tests/test_augment.py's bound; noise of scale 1.275 leaves [0, 1]);
the count of exactly equal float32 values is printed.  Outputs sit between sentinels, the pools are compared before and after.
`sim` runs the kernel sources on the host SIMT checker, `hip` (marker gpu) the gfx950 kernels."""
import random

import numpy as np
import pytest
import torch
from scipy import ndimage

from backend import dev, use_hip  # noqa: F401
from cenet_amd import _lib, data as D, kern

RAGGED = [(2, 3), (17, 33), (40, 36), (5, 70), (67, 130)]
GUARD, SENT_F, SENT_B = 512, -777.0, 0xAB
EXACT = {"equal": 0, "total": 0}


def _slices(shapes, seed, dev):
    rng = np.random.default_rng(seed)
    samples = [(rng.random(s).astype(np.float32), rng.integers(0, 9, s).astype(np.uint8)) for s in shapes]
    return samples, D.DeviceSlices(samples, dev)


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


def normal_np(n, k0, k1):
    ctr = np.zeros((n, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(n)
    x = philox_np(ctr, np.tile(np.array([[k0, k1]], dtype=np.uint64), (n, 1)))
    u1, u2 = (x[:, 0].astype(np.float64) + 0.5) / 2.0 ** 32, (x[:, 1].astype(np.float64) + 0.5) / 2.0 ** 32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos((2.0 * np.pi) * u2)


def grid_coordinates(dy, dx, H, W):
    R, C = dy.shape
    i, j = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    gy = i * ((R - 1) / (H - 1)) if H > 1 else i * 0.0
    gx = j * ((C - 1) / (W - 1)) if W > 1 else j * 0.0
    r0, c0 = np.minimum(np.floor(gy), R - 2).astype(int), np.minimum(np.floor(gx), C - 2).astype(int)
    fy, fx = gy - r0, gx - c0

    def at(d):
        return (1.0 - fy) * ((1.0 - fx) * d[r0, c0] + fx * d[r0, c0 + 1]) + fy * ((1.0 - fx) * d[r0 + 1, c0] + fx * d[r0 + 1, c0 + 1])

    return np.stack([i + at(dy), j + at(dx)])


def host_op(img32, lab, op):
    """one operator of the table in include/cenet_hip.h on (float32 image, uint8 label) -> (float64 image, uint8 label)"""
    kind, a = op[0], op[1:]
    a64 = img32.astype(np.float64)
    if kind == "copy":
        return a64, lab
    if kind == "flip_ud":
        return a64[::-1], lab[::-1]
    if kind == "flip_lr":
        return a64[:, ::-1], lab[:, ::-1]
    if kind == "affine":
        return (ndimage.affine_transform(a64, a[0], a[1], order=1, mode="constant", cval=0),
                ndimage.affine_transform(lab, a[0], a[1], order=0, mode="constant", cval=0))
    if kind == "grid_warp":
        co = grid_coordinates(np.asarray(a[0], dtype=np.float64), np.asarray(a[1], dtype=np.float64), *img32.shape)
        return (ndimage.map_coordinates(a64, co, order=1, mode="constant", cval=0),
                ndimage.map_coordinates(lab, co, order=0, mode="constant", cval=0))
    if kind == "blur":
        return ndimage.gaussian_filter(a64, a[0], mode="mirror", truncate=4.0), lab
    if kind == "blur_w":  # the plan's own weights: what gaussian_filter runs, axis 0 then axis 1
        w = np.concatenate([a[0][:0:-1], a[0]])
        return ndimage.correlate1d(ndimage.correlate1d(a64, w, 0, mode="mirror"), w, 1, mode="mirror"), lab
    if kind == "noise":
        return a64 + a[0] * normal_np(a64.size, a[1], a[2]).reshape(a64.shape), lab
    if kind == "contrast":
        return a[1] + a[0] * (a64 - a[1]), lab
    raise AssertionError(kind)


def host_chain(img32, lab, chain):
    """the operators in sequence, rounded to float32 between stages as the work buffers are"""
    for op in chain:
        img, lab = host_op(img32, lab, op)
        img32 = img.astype(np.float32)
    return img32, np.ascontiguousarray(lab)


def decode(tab_row, dp_rows):
    """a sample's chain back from its plan rows (copies dropped)"""
    names = {v: k for k, v in kern.AUG_OPS.items()}
    chain = []
    for word, q in zip(tab_row[3:], dp_rows):
        kind = names[int(word) & 255]
        if kind == "affine":
            chain.append((kind, q[0:4].reshape(2, 2), q[4:6]))
        elif kind == "grid_warp":
            R, C = (int(word) >> 8) & 255, (int(word) >> 16) & 255
            chain.append((kind, q[:R * C].reshape(R, C), q[16:16 + R * C].reshape(R, C)))
        elif kind == "blur":
            chain.append(("blur_w", q[1:2 + int(q[0])]))
        elif kind == "noise":
            chain.append((kind, q[0], int(q[1]), int(q[2])))
        elif kind == "contrast":
            chain.append((kind, q[0], q[1]))
        elif kind != "copy":
            chain.append((kind,))
    return chain


# ---- the device side, between sentinels ------------------------------------------------------------------------------------------------
def run_ops(aug, sl, indices, tab, dp, expect_error=False):
    """cenet_augment_ops on guarded work buffers -> per sample (image [H, W] float32, label [H, W] uint8); checks that nothing outside
    the samples' own H * W elements of the result buffer, and nothing of the pools, was written"""
    dev = sl.device
    B, S, n = tab.shape[0], tab.shape[1] - 3, tab.shape[0] * aug.stride
    full_i = [torch.full((n + 2 * GUARD,), SENT_F, dtype=torch.float32, device=dev) for _ in range(2)]
    full_l = [torch.full((n + 2 * GUARD,), SENT_B, dtype=torch.uint8, device=dev) for _ in range(2)]
    pools = sl.pool_img.clone(), sl.pool_lab.clone()
    args = (sl.pool_img, sl.pool_lab, tab, dp, torch.from_numpy(tab).to(dev), torch.from_numpy(dp).to(dev),
            [t[GUARD:GUARD + n] for t in full_i], [t[GUARD:GUARD + n] for t in full_l], aug.stride, sl.max_h, sl.max_w, B, S)
    if expect_error:
        with pytest.raises(RuntimeError, match="cenet_augment_ops failed with error code"):
            kern.augment_ops(*args)
        assert all(bool((t == SENT_F).all()) for t in full_i) and all(bool((t == SENT_B).all()) for t in full_l)
        assert torch.equal(pools[0], sl.pool_img) and torch.equal(pools[1], sl.pool_lab)
        return None
    r = kern.augment_ops(*args)
    assert r == S & 1
    assert torch.equal(pools[0], sl.pool_img) and torch.equal(pools[1], sl.pool_lab)
    img, lab = full_i[r].cpu().numpy(), full_l[r].cpu().numpy()
    mask = np.ones(n + 2 * GUARD, dtype=bool)
    out = []
    for b, idx in enumerate(indices):
        H, W = (int(v) for v in sl.shapes[idx])
        lo = GUARD + b * aug.stride
        mask[lo:lo + H * W] = False
        out.append((img[lo:lo + H * W].reshape(H, W).copy(), lab[lo:lo + H * W].reshape(H, W).copy()))
    assert (img[mask] == np.float32(SENT_F)).all() and (lab[mask] == SENT_B).all()
    return out


def check(got, want, what):
    (gi, gl), (wi, wl) = got, want
    assert gi.dtype == np.float32 and gl.dtype == np.uint8 and gi.shape == wi.shape == gl.shape == wl.shape, what
    assert np.array_equal(gl, wl), (what, int((gl != wl).sum()))
    wi32 = np.asarray(wi, dtype=np.float32)
    err = np.abs(gi.astype(np.float64) - np.asarray(wi, dtype=np.float64))
    assert (err <= 1e-6 * np.maximum(1.0, np.abs(wi))).all(), (what, float(err.max()))
    EXACT["equal"] += int((gi == wi32).sum())
    EXACT["total"] += gi.size


def _halves(rng, shape, scale):
    return np.round(rng.normal(0.0, scale, shape) * 2.0) / 2.0


def single_ops(shape, rng):
    """the operators run alone on a slice of `shape`, with the edge cases: a half-pixel tie under the identity, control-grid
    displacements that are multiples of one half"""
    H, W = shape
    a = np.deg2rad(rng.uniform(-40, 40))
    sh = np.tan(np.deg2rad(rng.uniform(-16, 16)))
    return [
        ("flip_ud",), ("flip_lr",), ("copy",),
        ("affine", np.eye(2), np.array([1.0, 0.5])),
        ("affine", np.eye(2), np.array([0.0, -0.5])),
        ("affine", *D.centred_affine([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], shape)),
        ("affine", *D.centred_affine([[1 / 0.6, 0], [0, 1 / 1.7]], shape)),
        ("affine", *D.centred_affine([[1, 0], [sh, 1]], shape)),
        ("affine", *D.centred_affine(np.eye(2), shape, shift=(0.15 * H, -0.2 * W))),
        ("grid_warp", rng.normal(0, 0.03, (4, 4)) * H, rng.normal(0, 0.03, (4, 4)) * W),
        ("grid_warp", _halves(rng, (4, 4), 1.5), _halves(rng, (4, 4), 1.5)),
        ("grid_warp", _halves(rng, (2, 8), 1.0), rng.normal(0, 2.0, (2, 8))),
        ("grid_warp", rng.normal(0, 1.0, (5, 3)), rng.normal(0, 1.0, (5, 3))),
        ("blur", 1.0), ("blur", 0.4), ("blur", 4.1),  # radius 4, 2 and 16
        ("noise", 0.005 * 255, 0x243F6A88, 0xA4093822),
        ("contrast", 0.7, 0.0), ("contrast", 1.5, 0.25),
    ]


# ---- 1. the generator ----------------------------------------------------------------------------------------------------------------
RANDOM123 = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_reproduces_the_random123_vectors(dev):
    ck = torch.tensor([c + k for c, k, _ in RANDOM123], dtype=torch.int64).to(dev)
    out = torch.full((3, 4), -1, dtype=torch.int64).to(dev)
    kern.philox4x32_10(ck, out)
    assert out.cpu().tolist() == [list(o) for _, _, o in RANDOM123]
    ref = philox_np(ck.cpu().numpy()[:, :4].astype(np.uint64), ck.cpu().numpy()[:, 4:].astype(np.uint64))
    assert ref.tolist() == [list(o) for _, _, o in RANDOM123]  # (the restatement the noise tests use is held to them too)


# ---- 2. every operator alone --------------------------------------------------------------------------------------------------------
def test_each_operator_alone_equals_scipy(dev):
    samples, sl = _slices(RAGGED, 11, dev)
    aug = D.SegAugmenter(sl, (32, 32), seed=0)
    rng = np.random.default_rng(5)
    per_sample = [single_ops(s, rng) for s in RAGGED]
    EXACT.update(equal=0, total=0)
    for k in range(len(per_sample[0])):
        order = list(np.random.default_rng(k).permutation(len(RAGGED)))  # the samples in a different order every time
        chains = [[per_sample[i][k]] for i in order]
        got = run_ops(aug, sl, order, *aug.plan(order, chains))
        for b, i in enumerate(order):
            check(got[b], host_chain(*samples[i], chains[b]), (per_sample[i][k][0], k, RAGGED[i]))
    print(f"single operators: {EXACT['equal']} of {EXACT['total']} float32 values exactly equal")
    assert EXACT["equal"] >= 0.999 * EXACT["total"], EXACT


# ---- 3. noise ------------------------------------------------------------------------------------------------------------------------
def test_noise_is_keyed_reproducible_and_standard_normal(dev):
    rng = np.random.default_rng(2)
    samples = [(np.zeros((128, 128), dtype=np.float32), rng.integers(0, 9, (128, 128)).astype(np.uint8)),
               (rng.random((17, 33)).astype(np.float32), rng.integers(0, 9, (17, 33)).astype(np.uint8))]
    sl = D.DeviceSlices(samples, dev)
    aug = D.SegAugmenter(sl, (32, 32), seed=0)

    def noise(k0, k1, scale=1.0):
        chains = [[("noise", scale, k0, k1)], [("noise", 0.005 * 255, k1, k0)]]
        return chains, run_ops(aug, sl, [0, 1], *aug.plan([0, 1], chains))

    chains, a = noise(12345, 4000000000)
    for b in range(2):
        check(a[b], host_chain(*samples[b], chains[b]), ("noise", b))
    _, again = noise(12345, 4000000000)
    _, other = noise(12346, 4000000000)
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(a, again))
    assert not np.array_equal(a[0][0], other[0][0]) and not np.array_equal(a[1][0], other[1][0])
    z = a[0][0].astype(np.float64).reshape(-1)  # 0 + 1 * z(p)
    n = z.size
    assert abs(z.mean()) <= 6.0 / np.sqrt(n) and abs(z.std() - 1.0) <= 6.0 / np.sqrt(2 * n), (z.mean(), z.std())


# ---- 4. chains ----------------------------------------------------------------------------------------------------------------------
def test_chains_equal_the_scipy_calls_in_sequence(dev):
    samples, sl = _slices(RAGGED + [(33, 32)], 13, dev)
    aug = D.SegAugmenter(sl, (32, 32), seed=0)
    rng = np.random.default_rng(7)
    order = [5, 0, 1, 2, 3, 4, 1]

    def rot(i, deg):
        a = np.deg2rad(deg)
        return ("affine", *D.centred_affine([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], sl.shapes[i]))

    def grid(i):
        H, W = sl.shapes[i]
        return ("grid_warp", rng.normal(0, 0.03, (4, 4)) * H, rng.normal(0, 0.03, (4, 4)) * W)

    chains = [
        [],                                                                    # no op at all: gathered from the pools unchanged
        [("flip_lr",)],                                                        # padded with three copies
        [rot(1, 25.0), ("blur", 1.0), grid(1), ("flip_ud",)],                  # an intensity op between two warps
        [grid(2), rot(2, -33.0), ("noise", 0.005 * 255, 7, 9), ("contrast", 1.4, 0.0)],  # two warps in a row
        [("blur", 1.0), ("blur", 1.0)],
        [("contrast", 0.5, 0.0), ("affine", *D.centred_affine([[1 / 1.3, 0], [0, 1 / 0.7]], sl.shapes[4])), ("copy",),
         ("affine", *D.centred_affine(np.eye(2), sl.shapes[4], shift=(3.5, -10.0)))],
        [("noise", 0.005 * 255, 1, 2), rot(1, 40.0), ("flip_ud",)],
    ]
    tab, dp = aug.plan(order, chains)
    assert tab.shape == (7, 3 + 4) and dp.shape == (7, 4, 32)
    got = run_ops(aug, sl, order, tab, dp)
    for b, i in enumerate(order):
        check(got[b], host_chain(*samples[i], chains[b]), ("chain", b))
        check(got[b], host_chain(*samples[i], decode(tab[b], dp[b])), ("decoded chain", b))


# ---- 5. the augmenter end to end ----------------------------------------------------------------------------------------------------
def host_pipeline(samples, indices, plan, size, normalize):
    tab, dp = plan
    imgs, labs = [], []
    for b, i in enumerate(indices):
        img, lab = host_chain(*samples[i], decode(tab[b], dp[b]))
        img, lab = D._resize_pair(img, lab, size)  # zoom(order=3) / zoom(order=0), dataset_synapse.py:106-109
        img = img.astype(np.float32)
        if normalize is not None:
            img = (img - np.float32(normalize[0])) / np.float32(normalize[1])
        imgs.append(img)
        labs.append(lab.astype(np.float32))
    return np.stack(imgs)[:, None], np.stack(labs)


def end_to_end(dev, shapes, size, normalize, seeds):
    samples, sl = _slices(shapes, 17, dev)
    seen = set()
    for seed in seeds:
        aug = D.SegAugmenter(sl, size, normalize=normalize, seed=seed)
        indices = list(np.random.default_rng(seed).permutation(len(shapes)))
        plan = aug.draw(indices)
        seen |= {n for p in aug.picked for n in p}
        out = aug.apply(plan)
        assert out["image"].shape == (len(shapes), 1, *size) and out["image"].dtype == torch.float32
        assert out["label"].shape == (len(shapes), *size) and out["label"].dtype == torch.float32
        wi, wl = host_pipeline(samples, indices, plan, size, normalize)
        assert np.array_equal(out["label"].cpu().numpy(), wl)
        gi = out["image"].cpu().numpy()
        err = np.abs(gi.astype(np.float64) - wi)
        assert (err <= 1e-6 * np.maximum(1.0, np.abs(wi))).all(), float(err.max())
    return seen


@pytest.mark.parametrize("normalize", [None, (0.5, 0.5)], ids=["plain", "normalize"])
def test_seg_augmenter_equals_the_host_pipeline_of_its_plan(dev, normalize):
    shapes = [(40, 70), (64, 48), (32, 32), (57, 41), (70, 40), (45, 66)]
    seen = end_to_end(dev, shapes, (32, 32), normalize, seeds=range(4))
    assert seen == {n for n, _ in D.SYNAPSE_OPS}  # every operator of the pipeline took part


@pytest.mark.gpu
def test_seg_augmenter_at_the_preset_size():
    dev = use_hip()
    try:
        end_to_end(dev, [(512, 512), (512, 512)], (224, 224), (0.5, 0.5), seeds=(1, 2, 3))
    finally:
        _lib._LIB, _lib._HOSTSIM = None, False


# ---- 6. the draw ---------------------------------------------------------------------------------------------------------------------
def test_draw_follows_the_pipelines_distribution():
    samples, sl = _slices([(40, 70), (64, 48)], 1, torch.device("cpu"))
    state = random.getstate(), np.random.get_state()
    indices = [0, 1] * 2000
    aug = D.SegAugmenter(sl, (32, 32), seed=99)
    tab, dp = aug.draw(indices)
    picked = aug.picked
    tab2, dp2 = D.SegAugmenter(sl, (32, 32), seed=99).draw(indices)
    assert np.array_equal(tab, tab2) and np.array_equal(dp, dp2)
    tab3, _ = D.SegAugmenter(sl, (32, 32), seed=100).draw(indices)
    assert not np.array_equal(tab, tab3)
    assert random.getstate() == state[0]
    now = np.random.get_state()
    assert now[0] == state[1][0] and np.array_equal(now[1], state[1][1]) and now[2:] == state[1][2:]

    names = [n for n, _ in D.SYNAPSE_OPS]
    N = len(indices)
    assert tab.shape == (N, 3 + 4) and len(picked) == N
    assert all(len(p) <= 4 and len(set(p)) == len(p) and set(p) <= set(names) for p in picked)
    assert {len(p) for p in picked} == {0, 1, 2, 3, 4}
    se = np.sqrt(0.2 * 0.8 / N)
    for n in names:
        f = sum(n in p for p in picked) / N
        assert abs(f - 0.2) <= 6 * se, (n, f)
    first = [p[0] for p in picked if p]  # random order: every op leads a chain equally often
    for n in names:
        f = first.count(n) / len(first)
        assert abs(f - 0.1) <= 6 * np.sqrt(0.1 * 0.9 / len(first)), (n, f)

    code = kern.AUG_OPS
    fired = {"flip_ud": [], "flip_lr": []}
    for b, p in enumerate(picked):
        H, W = (int(v) for v in tab[b, 1:3])
        assert (tab[b, 3 + len(p):] == 0).all() and not dp[b, len(p):].any()
        for s, n in enumerate(p):
            word, q = int(tab[b, 3 + s]), dp[b, s]
            if n in fired:
                assert word in (0, code[n])
                fired[n].append(word != 0)
            elif n == "noise":
                assert word == code["noise"] and q[0] == 0.005 * 255 and all(0 <= v < 2 ** 32 and v == int(v) for v in q[1:3])
            elif n == "blur":
                r, w = D.gaussian_weights(1.0)
                assert word == code["blur"] and q[0] == r == 4 and np.array_equal(q[1:6], w)
            elif n == "contrast":
                assert word == code["contrast"] and 0.5 <= q[0] <= 1.5 and q[1] == 0.0
            elif n == "grid_warp":
                assert word == code["grid_warp"] + 256 * 4 + 65536 * 4
                assert np.abs(q[:16]).max() <= 6 * 0.03 * H and np.abs(q[16:]).max() <= 6 * 0.03 * W and q[:16].any() and q[16:].any()
            else:
                assert word == code["affine"]
                m, off = q[0:4].reshape(2, 2), q[4:6]
                ctr = (np.array([H, W]) - 1) / 2
                shift = ctr - m @ ctr - off  # (zero for the warps about the centre)
                if n == "translate":
                    assert np.array_equal(m, np.eye(2)) and (np.abs(shift) <= 0.2 * np.array([H, W]) + 1e-9).all()
                    continue
                assert np.abs(shift).max() <= 1e-9
                if n == "scale":
                    assert m[0, 1] == m[1, 0] == 0 and all(0.5 <= 1 / v <= 2.0 for v in (m[0, 0], m[1, 1]))
                elif n == "rotate":
                    assert abs(np.rad2deg(np.arctan2(m[0, 1], m[0, 0]))) <= 40 and np.allclose(m @ m.T, np.eye(2), atol=1e-12)
                    assert m[1, 0] == -m[0, 1] and m[0, 0] == m[1, 1]
                elif n == "shear":
                    assert m[0, 0] == m[1, 1] == 1 and m[0, 1] == 0 and abs(np.rad2deg(np.arctan(m[1, 0]))) <= 16
    for n, v in fired.items():
        assert abs(np.mean(v) - 0.5) <= 6 * np.sqrt(0.25 / len(v)), (n, np.mean(v))


def test_draw_options():
    samples, sl = _slices([(40, 70)], 1, torch.device("cpu"))
    aug = D.SegAugmenter(sl, (32, 32), some_of=(2, 3), random_order=False, seed=3)
    aug.draw([0] * 200)
    order = {n: k for k, (n, _) in enumerate(D.SYNAPSE_OPS)}
    assert {len(p) for p in aug.picked} == {2, 3}
    assert all(list(p) == sorted(p, key=order.get) for p in aug.picked)
    with pytest.raises(ValueError, match="some_of"):
        D.SegAugmenter(sl, (32, 32), some_of=(0, 9))


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(dev):
    samples, sl = _slices([(17, 33), (40, 36)], 3, dev)
    aug = D.SegAugmenter(sl, (32, 32), seed=0)
    ok = aug.plan([0, 1], [[("flip_ud",)], [("blur", 1.0), ("copy",)]])
    assert run_ops(aug, sl, [0, 1], *ok) is not None

    def with_word(word):
        tab, dp = (a.copy() for a in ok)
        tab[1, 4] = word
        return tab, dp

    bad = {
        "unknown op code": with_word(8),
        "negative op word": with_word(-1),
        "grid bits on another op": with_word(3 + 256 * 2 + 65536 * 2),
        "S > 8": aug.plan([0, 1], [[("copy",)] * 9, []]),
        "blur radius 17": aug.plan([0, 1], [[], [("blur", 4.2)]]),
        "R * C > 16": aug.plan([0, 1], [[("grid_warp", np.zeros((5, 4)), np.zeros((5, 4)))], []]),
        "R < 2": with_word(4 + 256 * 1 + 65536 * 4),
    }
    assert D.gaussian_weights(4.2)[0] == 17 and bad["S > 8"][0].shape == (2, 12)
    for what, (tab, dp) in bad.items():
        run_ops(aug, sl, [0, 1], tab, dp, expect_error=True)
    small = D.SegAugmenter(sl, (32, 32), seed=0)
    small.stride = 40 * 36 - 1  # H * W > stride
    run_ops(small, sl, [0, 1], *ok, expect_error=True)
    assert run_ops(aug, sl, [0, 1], *ok) is not None  # (and the library still runs the good plan)


# ---- 8. the loader -------------------------------------------------------------------------------------------------------------------
def test_loader_with_an_augmenter_yields_what_the_augmenter_yields(dev):
    shapes = [(40, 36)] * 3 + [(32, 32)] * 2 + [(36, 50)] * 2
    samples, sl = _slices(shapes, 19, dev)
    sl.names = [f"s{i}" for i in range(len(shapes))]
    state = random.getstate()
    loader = D.DeviceTrainLoader(sl, (32, 32), batch_size=3, shuffle=True, generator=torch.Generator().manual_seed(5),
                                 augmenter=D.SegAugmenter(sl, (32, 32), normalize=(0.5, 0.5), seed=8))
    twin = D.SegAugmenter(sl, (32, 32), normalize=(0.5, 0.5), seed=8)
    assert loader.aug is not None and not isinstance(loader.aug, D.DeviceAugmenter) and len(loader) == 3
    seen = []
    for _ in range(2):
        for batch in loader:
            idx = [int(n[1:]) for n in batch["case_name"]]
            want = twin(idx)
            assert torch.equal(batch["image"], want["image"]) and torch.equal(batch["label"], want["label"])
            assert batch["image"].shape == (len(idx), 1, 32, 32)
            seen.append(sorted(idx))
    assert sorted(i for s in seen[:3] for i in s) == list(range(7)) and seen[:3] != seen[3:]
    assert random.getstate() == state  # the global stream the built-in augmenter draws from is not consumed
    plain = D.DeviceTrainLoader(sl, (32, 32), batch_size=3)
    assert isinstance(plain.aug, D.DeviceAugmenter)
