"""Surface metrics with a voxel spacing (csrc/edt.hip `edt_line_w_kernel`, csrc/metrics.hip `min_sqdist_spaced_kernel`): the spaced
transform against scipy's `sampling=`, the methods of `surface_distances(spacing=)` against each other and the restated medpy with
`voxelspacing=`, `label_metrics(spacing=)` against the per-class loop, and the normalised surface Dice against its count formula.
Every case runs on the host SIMT checker and, marked gpu, on the MI355X.

Bounds.  Dyadic spacings (2.5, 1.25, 10, 1.5625, 0.5, 1): every product and sum on both sides is exact in fp64 at these sizes, so
the results must be bit-identical.  General spacings: scipy forms sqrt((s dz)^2 + (s dy)^2 + (s dx)^2), the kernels form sums of
s^2 d^2; each side makes at most about six roundings of 2^-53 on the squared distance, halved by the square root, plus the root's
own, and a tie between two sites picks values that agree to rounding: |got - want| <= 8 eps want, eps = 2^-52, zeros exact.  A
wrong site would be off by a whole voxel step, 1e-2 relative or more."""
import functools
import math

import numpy as np
import pytest
import torch
from scipy.ndimage import distance_transform_edt, zoom

from backend import dev  # noqa: F401
from cenet_amd import _lib, evaluate, kern
from oracle import cenet_oracle as O
from test_edt import SCENARIOS, _apply, _feat, _label_pair, _mask_pair

EPS = 2.0 ** -52
# (2.5, 0.75, 1.25): the transform takes another route when the in-plane spacing is isotropic, which the issue's three all are
DYADIC = [(2.5, 1.25, 1.25), (10, 1.5625, 1.5625), (0.5, 0.5, 0.5), (2.5, 0.75, 1.25)]
GENERAL = [(3.0, 1.4, 1.1), (1.0, 0.7, 1.3), (0.37, 2.9, 0.013), (3.0, 0.7, 0.7)]

# the shapes of tests/test_edt.py (tile edges of the x pass, 64 lines per workgroup, a z line longer than 64)
EDT_CASES = [((1, 9, 11), "sparse"), ((7, 1, 10), "sparse"), ((6, 8, 1), "sparse"), ((1, 1, 5), "corner"), ((4, 6, 5), "all"),
             ((5, 30, 70), "sparse"), ((5, 30, 70), "dense"), ((3, 50, 150), "sparse"), ((67, 5, 3), "sparse"),
             ((2, 131, 4), "corner")]
# the mask pairs of test_surface_distances_methods_agree: (3, 9, 7) has fewer than 256 border voxels, the (8, 24, 20) noise pair more
# than 1024 (more than one LDS tile of the all-pairs kernel)
MASK_CASES = [((6, 20, 24), 0), ((3, 9, 7), 1), ((10, 40, 36), 2), ((1, 12, 12), 3), ((24, 24), 4), ((12, 64, 64), 5),
              ((8, 24, 20), "noise"), ((20, 22), "noise")]


def _close(got, want, exact):
    """bit-identical, or within 8 eps relative with the zeros in the same places"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if exact:
        return got.shape == want.shape and np.array_equal(got, want)
    return got.shape == want.shape and np.array_equal(got == 0, want == 0) and bool(np.all(np.abs(got - want) <= 8 * EPS * want))


def _sp(sp, ndim):
    return sp[3 - ndim:]


@functools.lru_cache(maxsize=None)
def _feat_of(shape, kind):
    f = _feat(shape, kind, seed=sum(shape))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _scipy_edt(shape, kind, sp):
    r = distance_transform_edt(~_feat_of(shape, kind), sampling=sp)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _masks(shape, seed):
    return _mask_pair(shape, seed)  # (shared: no test writes to them)


@functools.lru_cache(maxsize=None)
def _oracle_sd(shape, seed, sp):
    a, b = _masks(shape, seed)
    r = O.surface_distances(a, b, voxelspacing=sp), O.surface_distances(b, a, voxelspacing=sp)
    r[0].setflags(write=False), r[1].setflags(write=False)
    return r


def _spaced_sqrt(dev, shape, kind, sp):
    d2 = kern.edt_sq_spaced(torch.from_numpy(_feat_of(shape, kind).astype(np.uint8)).to(dev), sp)
    assert d2.dtype == torch.float64 and tuple(d2.shape) == shape
    return np.sqrt(d2.cpu().numpy())


# ---- 1, 2, 3: the transform -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", EDT_CASES)
def test_spaced_edt_dyadic_is_bit_identical_to_scipy(dev, shape, kind):
    for sp in DYADIC:
        got, want = _spaced_sqrt(dev, shape, kind, sp), _scipy_edt(shape, kind, sp)
        assert np.array_equal(got, want), (sp, float(np.abs(got - want).max()))


@pytest.mark.parametrize("shape,kind", EDT_CASES)
def test_spaced_edt_general_is_within_rounding_of_scipy(dev, shape, kind):
    for sp in GENERAL:
        got, want = _spaced_sqrt(dev, shape, kind, sp), _scipy_edt(shape, kind, sp)
        assert np.array_equal(got == 0, want == 0), sp
        nz = want > 0
        worst = float((np.abs(got - want)[nz] / want[nz]).max() / EPS) if nz.any() else 0.0
        print(f"{shape} {kind} {sp}: worst |got - want| / want = {worst:.3f} eps")
        assert worst <= 8, (sp, worst)


@pytest.mark.parametrize("shape,kind", EDT_CASES)
def test_spaced_edt_unit_spacing_equals_integer_transform(dev, shape, kind):
    feat = torch.from_numpy(_feat_of(shape, kind).astype(np.uint8)).to(dev)
    got, want = kern.edt_sq_spaced(feat, (1, 1, 1)).cpu().numpy(), kern.edt_sq(feat).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, want)


def test_feature_free_lines_and_volumes_come_out_infinite(dev):
    """the raw entry point on a volume without a feature, and a volume whose only feature leaves whole x rows without one"""
    D, H, W = 3, 5, 70
    xd = torch.empty((D, H, W), dtype=torch.int32, device=dev)
    tmp, d2 = (torch.empty((D, H, W), dtype=torch.float64, device=dev) for _ in range(2))
    kern.edt_sq_spaced_raw(torch.zeros((D, H, W), dtype=torch.uint8, device=dev), -1, xd, tmp, d2, D, H, W, (2.5, 1.25, 1.25))
    assert bool(torch.isinf(d2).all()) and bool((d2 > 0).all())
    labels = torch.zeros((D, H, W), dtype=torch.uint8, device=dev)
    labels[1, 2, 3] = 7  # `match` picks the feature label
    kern.edt_sq_spaced_raw(labels, 7, xd, tmp, d2, D, H, W, (2.5, 1.25, 1.25))
    f = np.zeros((D, H, W), bool)
    f[1, 2, 3] = True
    assert np.array_equal(np.sqrt(d2.cpu().numpy()), distance_transform_edt(~f, sampling=(2.5, 1.25, 1.25)))
    kern.edt_sq_spaced_raw(labels, 6, xd, tmp, d2, D, H, W, (2.5, 1.25, 1.25))
    assert bool(torch.isinf(d2).all())


# ---- 3, 4: surface distances ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", MASK_CASES)
def test_surface_distances_unit_spacing_equals_unspaced(dev, shape, seed):
    a, b = _masks(shape, seed)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    for method in ("edt", "pairs", "auto"):
        want = evaluate.surface_distances(ta, tb, method=method)
        for unit in (1.0, (1,) * len(shape)):
            got = evaluate.surface_distances(ta, tb, method=method, spacing=unit)
            assert got[0].dtype == np.float64 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), method


def test_mask_cases_cover_both_sides_of_the_all_pairs_tile():
    few = O.surface_distances(*_masks((3, 9, 7), 1))
    many = O.surface_distances(*_masks((8, 24, 20), "noise"))
    assert few.size < 256 and many.size > 1024


@pytest.mark.parametrize("sp3", DYADIC + GENERAL, ids=lambda sp: "-".join(str(v) for v in sp))
@pytest.mark.parametrize("shape,seed", MASK_CASES)
def test_spaced_surface_distances_methods_agree_with_oracle(dev, shape, seed, sp3):
    a, b = _masks(shape, seed)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    sp, exact = _sp(sp3, len(shape)), sp3 in DYADIC
    r1, r2 = _oracle_sd(shape, seed, sp)
    got = {}
    for method in ("edt", "pairs", "auto"):
        d1, d2 = got[method] = evaluate.surface_distances(ta, tb, method=method, spacing=sp)
        assert d1.dtype == np.float64 and d1.shape == r1.shape and d2.shape == r2.shape, method
        assert _close(d1, r1, exact) and _close(d2, r2, exact), method  # element for element, in C order of the border voxels
    again = evaluate.surface_distances(ta, tb, method="pairs", spacing=sp)  # no atomics: the same bits on every run
    assert again[0].tobytes() == got["pairs"][0].tobytes() and again[1].tobytes() == got["pairs"][1].tobytes()
    # hd95 and assd are continuous in the distances: the same relative bound
    assert _close(evaluate.hd95(ta, tb, spacing=sp), float(np.percentile(np.hstack((r1, r2)), 95)), False)
    assert _close(evaluate.assd(ta, tb, spacing=sp), float(np.mean((r1.mean(), r2.mean()))), False)


@pytest.mark.parametrize("shape,seed", [((6, 20, 24), 0), ((24, 24), 4)])
def test_percase_wrappers_take_spacing(dev, shape, seed):
    a, b = _masks(shape, seed)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    sp = _sp(DYADIC[0], len(shape))
    r1, r2 = _oracle_sd(shape, seed, sp)
    want = (float(np.percentile(np.hstack((r1, r2)), 95)), float(np.mean((r1.mean(), r2.mean()))))
    for method in ("edt", "pairs", "auto"):
        got = evaluate.metric_percase(ta, tb, method=method, spacing=sp)
        assert (got[1], got[3]) == want and got[0] == evaluate.metric_percase(ta, tb, method=method)[0], method
        assert evaluate.synapse_metric_percase(ta, tb, method=method, spacing=sp) == got[:2], method
        assert (evaluate.hd95(ta, tb, method=method, spacing=sp), evaluate.assd(ta, tb, method=method, spacing=sp)) == want


# ---- 5: label_metrics -------------------------------------------------------------------------------------------------------------
def _want_case(p, g, sp, tau=None):
    """calculate_metric_percase with medpy's voxelspacing, on the oracle's arrays; with `tau` the NSD count formula as well"""
    if p.any() and g.any():
        r1, r2 = O.surface_distances(p, g, voxelspacing=sp), O.surface_distances(g, p, voxelspacing=sp)
        inter, np_, ng = np.count_nonzero(p & g), np.count_nonzero(p), np.count_nonzero(g)
        m = (2.0 * inter / float(np_ + ng), float(np.percentile(np.hstack((r1, r2)), 95)), inter / float(np_ + ng - inter),
             float(np.mean((r1.mean(), r2.mean()))))
        if tau is None:
            return m
        assert min(np.abs(r1 - tau).min(), np.abs(r2 - tau).min()) > 1e-6  # the count is discontinuous at d == tau
        return m + ((np.count_nonzero(r1 <= tau) + np.count_nonzero(r2 <= tau)) / float(r1.size + r2.size),)
    m = (1, 0, 1, 0) if p.any() else (0, 0, 0, 0)
    return m if tau is None else m + (m[0],)


@pytest.mark.parametrize("K", [2, 4, 9])
@pytest.mark.parametrize("shape", [(6, 28, 30), (26, 34)])
def test_label_metrics_with_spacing_equals_per_class_loop(dev, K, shape):
    for n, scen in enumerate(SCENARIOS[K]):
        pred, gt = _label_pair(shape, K, seed=10 * K + n)
        for c, s in scen.items():
            pred, gt = _apply(pred, gt, c, s)
        tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        for sp3, methods in ((DYADIC[0], ("edt", "pairs", "auto")), (GENERAL[0], ("auto",))):
            sp, exact = _sp(sp3, len(shape)), sp3 in DYADIC
            want = [_want_case(pred == c, gt == c, sp) for c in range(1, K)]
            for method in methods:
                for kind, cols in (("acdc", (0, 1, 2, 3)), ("synapse", (0, 1))):
                    got = evaluate.label_metrics(tp, tg, K, kind=kind, method=method, spacing=sp)
                    assert len(got) == K - 1
                    for g, w in zip(got, want):
                        assert len(g) == len(cols), (kind, g)
                        for v, k in zip(g, cols):
                            assert _close(v, w[k], exact and k in (1, 3)) and abs(v - w[k]) < 1e-12, (method, kind, k, g, w)


@pytest.mark.parametrize("method", ["edt", "pairs", "auto"])
def test_label_metrics_with_spacing_keeps_two_downloads(dev, method, monkeypatch):
    calls = []
    real = evaluate._download
    monkeypatch.setattr(evaluate, "_download", lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    counts = {}
    for K in (4, 9):
        pred, gt = _label_pair((6, 28, 30), K, seed=K)
        assert all((pred == c).any() and (gt == c).any() for c in range(1, K))
        del calls[:]
        evaluate.label_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), K, method=method,
                               spacing=(2.5, 1.25, 1.25), nsd_tolerance=2.0)
        counts[K] = len(calls)
    assert counts[4] == counts[9] == 2


# ---- 6: normalised surface Dice ---------------------------------------------------------------------------------------------------
NSD_SPACINGS = [(2.5, 1.25, 1.25), (10, 1.5625, 1.5625), (3.0, 1.4, 1.1)]


@pytest.mark.parametrize("sp3", NSD_SPACINGS, ids=lambda sp: "-".join(str(v) for v in sp))
@pytest.mark.parametrize("shape,seed", MASK_CASES)
def test_surface_dice_matches_the_count_formula(dev, shape, seed, sp3):
    a, b = _masks(shape, seed)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    sp = _sp(sp3, len(shape))
    r1, r2 = _oracle_sd(shape, seed, sp)
    for tau, method in ((1.0, "auto"), (2.0, "auto"), (2.0, "edt"), (1.0, "pairs")):
        # the count is discontinuous at d == tau: no oracle distance may lie within 1e-6 of it, and then no voxel is left out
        assert min(np.abs(r1 - tau).min(), np.abs(r2 - tau).min()) > 1e-6, tau
        want = (np.count_nonzero(r1 <= tau) + np.count_nonzero(r2 <= tau)) / float(r1.size + r2.size)
        assert evaluate.surface_dice(ta, tb, tau, spacing=sp, method=method) == want, (tau, method)


def test_surface_dice_without_a_spacing_counts_in_voxels(dev):
    a, b = _masks((6, 20, 24), 0)
    r1, r2 = O.surface_distances(a, b), O.surface_distances(b, a)
    want = (np.count_nonzero(r1 <= 1.5) + np.count_nonzero(r2 <= 1.5)) / float(r1.size + r2.size)  # (no sqrt of an integer is 1.5)
    assert evaluate.surface_dice(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), 1.5) == want


@pytest.mark.parametrize("K,shape", [(4, (6, 28, 30)), (9, (6, 28, 30)), (4, (26, 34))])
def test_label_metrics_nsd_is_the_last_element(dev, K, shape):
    for n, scen in enumerate(SCENARIOS[K]):
        pred, gt = _label_pair(shape, K, seed=10 * K + n)
        for c, s in scen.items():
            pred, gt = _apply(pred, gt, c, s)
        tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        for sp3, tau in ((NSD_SPACINGS[0], 2.0), (NSD_SPACINGS[2], 1.0)):
            sp = _sp(sp3, len(shape))
            want = [_want_case(pred == c, gt == c, sp, tau) for c in range(1, K)]
            for kind, n_el in (("acdc", 5), ("synapse", 3)):
                got = evaluate.label_metrics(tp, tg, K, kind=kind, spacing=sp, nsd_tolerance=tau)
                assert [len(g) for g in got] == [n_el] * (K - 1)
                assert [g[-1] for g in got] == [w[-1] for w in want], (kind, sp, tau)
                assert [g[:-1] for g in got] == evaluate.label_metrics(tp, tg, K, kind=kind, spacing=sp)
        for c, s in scen.items():  # the empty-mask rule follows the tuple's Dice rule
            assert got[c - 1][-1] == (1 if s == "only_pred" else 0 if s in ("only_gt", "neither") else 1.0), (c, s)


def test_surface_dice_refusals(dev):
    z = torch.zeros((3, 5, 5), dtype=torch.bool, device=dev)
    one = z.clone()
    one[1, 2, 2] = True
    with pytest.raises(RuntimeError, match="first"):
        evaluate.surface_dice(z, one, 1.0, spacing=(2.5, 1.25, 1.25))
    with pytest.raises(RuntimeError, match="second"):
        evaluate.surface_dice(one, z, 1.0)
    assert evaluate.surface_dice(one, one, 1.0, spacing=(2.5, 1.25, 1.25)) == 1.0
    for bad in (0, 0.0, -1.0, math.nan, math.inf, None, "2"):
        with pytest.raises(ValueError):
            evaluate.surface_dice(one, one, bad, spacing=1.0)
    for bad in (0, -2.0, math.nan):
        with pytest.raises(ValueError):
            evaluate.label_metrics(one.float(), one.float(), 2, nsd_tolerance=bad)
    with pytest.raises(ValueError):  # a missing spacing entry
        evaluate.surface_dice(one, one, 1.0, spacing=(1.25, 1.25))


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------
BAD_ENTRIES = (0, 0.0, -1.5, math.nan, math.inf, -math.inf)


def test_bad_spacings_raise_before_any_launch(dev, monkeypatch):
    vol = torch.zeros((3, 6, 5), dtype=torch.bool, device=dev)
    vol[1, 2:4, 1:4] = True
    img = vol[1].clone()
    feat = vol.to(torch.uint8)

    def no_launch(name, *a):
        raise AssertionError(f"{name} was launched")

    monkeypatch.setattr(kern, "_call", no_launch)
    monkeypatch.setattr(kern, "_launch", no_launch)
    bad3 = [(1.25, 1.25), (1, 1, 1, 1), (), "1 1 1", {"z": 1}, [[1, 1, 1]]] + [(2.5, 1.25, v) for v in BAD_ENTRIES] + list(BAD_ENTRIES)
    bad2 = [(2.5, 1.25, 1.25), (1.25,)] + [(v, 1.25) for v in BAD_ENTRIES] + list(BAD_ENTRIES)
    for x, bads in ((vol, bad3), (img, bad2)):
        for bad in bads:
            for method in ("edt", "pairs", "auto"):
                with pytest.raises(ValueError):
                    evaluate.surface_distances(x, x, method=method, spacing=bad)
                with pytest.raises(ValueError):
                    evaluate.metric_percase(x, x, method=method, spacing=bad)
                with pytest.raises(ValueError):
                    evaluate.synapse_metric_percase(x, x, method=method, spacing=bad)
            for fn in (evaluate.hd95, evaluate.assd):
                with pytest.raises(ValueError):
                    fn(x, x, spacing=bad)
            with pytest.raises(ValueError):
                evaluate.label_metrics(x.float(), x.float(), 2, spacing=bad)
            with pytest.raises(ValueError):
                evaluate.surface_dice(x, x, 1.0, spacing=bad)
    for bad in [(1.25, 1.25), 1.0, None] + [(2.5, v, 1.25) for v in BAD_ENTRIES]:
        with pytest.raises(ValueError):
            kern.edt_sq_spaced(feat, bad)
    t = torch.zeros(8, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):  # the bound of the integer transform
        kern.edt_sq_spaced_raw(torch.ones(8, dtype=torch.uint8, device=dev), -1, torch.zeros(8, dtype=torch.int32, device=dev), t, t,
                               1, 1, 46341, (1, 1, 1))
    assert evaluate.AUTO_PAIRS_PER_BOX_VOXEL == 640 and evaluate.AUTO_PAIRS_PER_BOX_VOXEL_SPACED > 0


def test_edt_sq_spaced_refuses_a_feature_free_volume(dev):
    with pytest.raises(ValueError, match="no feature"):
        kern.edt_sq_spaced(torch.zeros((2, 3, 4), dtype=torch.uint8, device=dev), (2.5, 1.25, 1.25))


def test_raw_entry_points_return_einval(dev):
    D, H, W = 2, 3, 4
    feat = torch.ones((D, H, W), dtype=torch.uint8, device=dev)
    xd = torch.zeros((D, H, W), dtype=torch.int32, device=dev)
    tmp, d2 = (torch.full((D, H, W), -1.0, dtype=torch.float64, device=dev) for _ in range(2))
    pts = torch.zeros((2, 3), dtype=torch.int32, device=dev)
    out = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
    lib, P, s = _lib.lib(), kern.P, kern.stream()
    assert lib.cenet_edt_sq_spaced_u8(P(feat), -1, P(xd), P(tmp), P(d2), D, H, W, 2.5, 1.25, 1.25, s) == 0
    assert lib.cenet_min_sqdist_spaced_f64(P(pts), 2, P(pts), 2, 2.5, 1.25, 1.25, None, 0, P(out), s) == 0
    assert bool((d2 == 0).all()) and bool((out == 0).all())
    d2.fill_(-1.0), out.fill_(-1.0)
    for k in range(3):
        for v in BAD_ENTRIES + (1e200, 1e-200):  # (the last two: the square is not finite, or not positive)
            sp = [2.5, 1.25, 1.25]
            sp[k] = v
            assert lib.cenet_edt_sq_spaced_u8(P(feat), -1, P(xd), P(tmp), P(d2), D, H, W, *sp, s) == 1, sp  # CENET_EINVAL
            assert lib.cenet_min_sqdist_spaced_f64(P(pts), 2, P(pts), 2, *sp, None, 0, P(out), s) == 1, sp
    for shape in ((0, 3, 4), (1, 1, 46341), (46341, 1, 1)):
        assert lib.cenet_edt_sq_spaced_u8(P(feat), -1, P(xd), P(tmp), P(d2), *shape, 1.0, 1.0, 1.0, s) == 1, shape
    assert lib.cenet_min_sqdist_spaced_f64(P(pts), 0, P(pts), 2, 1.0, 1.0, 1.0, None, 0, P(out), s) == 1
    assert lib.cenet_border_gather_f64(P(feat), 1, D, H, W, P(xd), None, P(d2), s) == 1  # no coordinate rows in fp64
    assert lib.cenet_min_sqdist_spaced_ws_doubles(300, 5000) > 0  # b is split: a call without the scratch is refused
    big = torch.zeros((5000, 3), dtype=torch.int32, device=dev)
    assert lib.cenet_min_sqdist_spaced_f64(P(big), 300, P(big), 5000, 1.0, 1.0, 1.0, None, 0, P(out), s) == 1
    assert bool((d2 == -1).all()) and bool((out == -1).all())  # nothing was launched
    with pytest.raises(TypeError, match="double"):  # the header types the scratch: an fp32 tensor is refused by name
        kern.edt_sq_spaced_raw(feat, -1, xd, tmp.float(), d2, D, H, W, (1, 1, 1))


# ---- 8: wrappers ------------------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    """the four-class network of test_volume_wrappers_go_through_label_metrics"""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return -(x - torch.linspace(0.2, 0.8, 4, device=x.device).view(1, 4, 1, 1)).abs()


def _tiny_case(seed=0):
    rng = np.random.default_rng(seed)
    image = np.stack([zoom(s, (16 / 6, 16 / 6), order=1) for s in rng.random((4, 6, 6))]).astype(np.float32)
    label = np.clip((image * 4).astype(np.int64), 0, 3).astype(np.float32)
    return torch.from_numpy(image)[None], torch.from_numpy(label)[None]


def test_volume_wrappers_take_spacing_and_nsd(dev, monkeypatch):
    image, label = _tiny_case()
    net = _Net().to(dev)
    sp, tau = (5, 1.25, 1.25), 2.0
    kw = dict(patch_size=(16, 16), device=dev)
    seen = []
    real = evaluate.label_metrics
    monkeypatch.setattr(evaluate, "label_metrics", lambda p, *a, **k: (seen.append((p.clone(), k)), real(p, *a, **k))[1])
    for wrapper, kind, n_el in ((evaluate.test_single_volume, "acdc", 4), (evaluate.synapse_test_single_volume, "synapse", 2)):
        del seen[:]
        plain = wrapper(image, label, net, 4, **kw)
        assert seen[0][1] == {}  # without the new arguments: the call label_metrics has always got
        assert [len(m) for m in plain] == [n_el] * 3
        assert wrapper(image, label, net, 4, z_spacing=7.5, **kw) == plain  # z_spacing alone changes no metric
        got = wrapper(image, label, net, 4, spacing=sp, nsd_tolerance=tau, z_spacing=7.5, **kw)
        assert [len(m) for m in got] == [n_el + 1] * 3
        want = real(seen[-1][0], label[0].to(dev), 4, kind, spacing=sp, nsd_tolerance=tau)
        assert got == want and [m[1] for m in got] == [m[1] for m in real(seen[-1][0], label[0].to(dev), 4, kind, spacing=sp)]
        assert [m[0] for m in got] == [m[0] for m in plain] and [m[1] for m in got] != [m[1] for m in plain]
        only_sp = wrapper(image, label, net, 4, spacing=sp, **kw)
        assert only_sp == [m[:-1] for m in got]
        for bad in ((1.25, 1.25), 0, (5, 1.25, math.nan)):
            with pytest.raises(ValueError):
                wrapper(image, label, net, 4, spacing=bad, **kw)
        with pytest.raises(ValueError):
            wrapper(image, label, net, 4, nsd_tolerance=-1.0, **kw)


def test_inference_takes_one_spacing_or_one_per_case(dev):
    net = _Net().to(dev)
    cases = [dict(zip(("image", "label"), _tiny_case(s)), case_name=[f"c{s}"]) for s in (0, 1)]
    sps = {"c0": (5, 1.25, 1.25), "c1": (10, 1.5625, 1.5625)}
    kw = dict(patch_size=(16, 16), resize="host", device=dev, log=lambda s: None)
    plain = evaluate.inference(net, cases, 4, **kw)
    assert len(plain) == 2
    per = [evaluate.test_single_volume(c["image"], c["label"], net, 4, patch_size=(16, 16), device=dev, spacing=sps[c["case_name"][0]],
                                       nsd_tolerance=2.0) for c in cases]
    table = np.mean(np.array(per, dtype=np.float64), axis=0)
    want = tuple(float(v) for v in np.mean(table, axis=0)[[0, 1, 4]])
    lines = []
    got = evaluate.inference(net, cases, 4, spacing=sps, nsd_tolerance=2.0, **dict(kw, log=lines.append))
    assert got == want and got[0] == plain[0] and got[1] != plain[1]
    assert evaluate.inference(net, cases, 4, spacing=[sps["c0"], sps["c1"]], nsd_tolerance=2.0, **kw) == want
    assert len(lines) == 2 + 3 + 1 + 1 and "mean_nsd" in lines[-1] and "mean_nsd" not in lines[-2]
    one = evaluate.inference(net, cases, 4, spacing=sps["c0"], **kw)
    same = evaluate.inference(net, cases, 4, spacing=[sps["c0"], sps["c0"]], **kw)
    assert len(one) == 2 and one == same
    for bad in ({"c0": sps["c0"]}, [sps["c0"]], (1.25, 1.25), 0.0, [sps["c0"], (1, 1)]):
        with pytest.raises(ValueError):
            evaluate.inference(net, cases, 4, spacing=bad, **kw)


@pytest.mark.gpu
def test_train_acdc_hands_spacing_and_tolerance_to_the_test_inference(monkeypatch):
    from backend import use_hip
    from cenet_amd import train
    from cenet_amd.networks import CENet
    d = use_hip()
    try:
        torch.manual_seed(77)
        net = CENet(input_channels=1, num_classes=4, scale_factors=[1.0, 0.5], diffatt_num_heads=[4, 4, 4], out_up_block="upcn")
        net.backbone.reset_drop_path(0.0)
        x, lab = O.synthetic_batch(2, 1, 4, seed=21)
        loader = [{"image": x, "label": lab.long()}]
        seen = []
        monkeypatch.setattr(evaluate, "validate", lambda net, batches: 0.5)
        monkeypatch.setattr(evaluate, "inference", lambda net, volumes, classes, **kw: (seen.append(kw), (0.4, 9.0, 0.7))[1])
        sp = {"c0": (10, 1.5625, 1.5625)}
        h = train.train_acdc(net, loader, max_epochs=1, base_lr=0.01, device=d, graph=False, val_batches=lambda: [], log=lambda s: None,
                             test_volumes=lambda: ["vol"], test_spacing=sp, test_nsd_tolerance=2.0)
        assert seen[0]["spacing"] is sp and seen[0]["nsd_tolerance"] == 2.0
        assert h["test_dice"] == [0.4] and h["test_hd95"] == [9.0] and h["test_nsd"] == [0.7]
        del seen[:]
        monkeypatch.setattr(evaluate, "inference", lambda net, volumes, classes, **kw: (seen.append(kw), (0.4, 9.0))[1])
        h = train.train_acdc(net, loader, max_epochs=1, base_lr=0.01, device=d, graph=False, val_batches=lambda: [], log=lambda s: None,
                             test_volumes=lambda: ["vol"])
        assert "spacing" not in seen[0] and "nsd_tolerance" not in seen[0] and "test_nsd" not in h
    finally:
        _lib._LIB = None
