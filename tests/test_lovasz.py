"""The Lovasz-Softmax loss (csrc/lovasz.hip, ops.lovasz_softmax / ops.lovasz_order, losses.LovaszSoftmaxLoss / Criterion) against
tests/lovasz_ref.py, the float64 restatement of its definition.  Every case runs on the host SIMT checker and, marked gpu, on the
MI355X.

1. The order: ops.lovasz_order equals numpy's stable descending argsort element for element.
2. The probability path (from_probs): the error is one fp32 operation on both sides, so the order is the reference's and the bounds
   are those of the arithmetic alone: |loss - ref| < 1e-5 max(1, |ref|); fp32 gradient within 1e-5 |ref| per element (about ten
   fp32 roundings of 6e-8, tenfold margin; a reference of exactly 0 wants exactly 0); bf16 gradient within 2^-8 |ref| (one
   output rounding of 2^-9, doubled).
3. The logits path: the device orders by its fp32 softmax, the reference by the float64 one, and elements with nearly equal errors
   may swap; the test bounds the effect: loss as in 2, fp32 gradient relative L2 < 1e-3 and max |got - ref| < 2e-3 max |ref|, bf16
   gradient relative L2 < 1e-2 (the figure of tests/test_bf16_storage.py::test_seg_loss).  per_image and ignore_index take the same
   bounds.
4. gout, reproducibility, refusals, Criterion."""
import argparse
import functools

import numpy as np
import pytest
import torch

import dist_cases as C
from backend import dev  # noqa: F401
from cenet_amd import kern, losses, ops
from lovasz_ref import lovasz_ref

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
EXTRA = [(2, 2, 96, 96), (1, 9, 64, 64)]
COMBOS = [(False, "present"), (False, "all"), (True, "present"), (True, "all")]


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ---- 1. the order -------------------------------------------------------------------------------------------------------------------
LENGTHS = {"1": lambda t: 1, "5": lambda t: 5, "63": lambda t: 63, "64": lambda t: 64, "65": lambda t: 65,
           "tile-1": lambda t: t - 1, "tile": lambda t: t, "3tiles+1": lambda t: 3 * t + 1}


def _order_inputs(S, n, seed):
    rng = np.random.default_rng(seed)
    rnd = rng.random((S, n), dtype=np.float32)
    ends = rnd.copy()
    ends[rng.random((S, n)) < 0.2] = 0.0
    ends[rng.random((S, n)) < 0.2] = 1.0
    ends[:, 0], ends[:, -1] = 1.0, 0.0
    ramp = np.tile(np.linspace(0.0, 1.0, n, dtype=np.float32), (S, 1))
    return {"random": rnd, "eight levels": (rng.integers(0, 8, (S, n)) / 7).astype(np.float32),
            "all equal": np.full((S, n), 0.375, np.float32), "ascending": ramp, "descending": ramp[:, ::-1].copy(),
            "zeros and ones": ends}


def _check_order(d, e, what):
    got = ops.lovasz_order(torch.from_numpy(e).to(d))
    assert got.dtype == torch.int32 and tuple(got.shape) == e.shape
    ref = np.argsort(-e, axis=1, kind="stable")
    assert np.array_equal(got.cpu().numpy(), ref), what


@pytest.mark.parametrize("S", [1, 3, 40])
@pytest.mark.parametrize("length", list(LENGTHS))
def test_order_is_the_stable_descending_sort(dev, length, S):
    n = LENGTHS[length](kern.lovasz_tile())
    for what, e in _order_inputs(S, n, 100 * S + n).items():
        _check_order(dev, e, (what, S, n))


def test_order_over_more_tiles_than_a_scan_group_takes_at_once(dev):
    """300 tiles: the scan of a (segment, digit) row over its tiles takes two steps of 64 lanes with four values each"""
    n = 300 * kern.lovasz_tile() + 3
    rng = np.random.default_rng(5)
    _check_order(dev, (rng.integers(0, 1000, (1, n)) / 999).astype(np.float32), "thousand levels")


# ---- the cases of 2 and 3 ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _labels(shape, variant="plain"):
    lab = torch.from_numpy(C.labels(shape).copy())
    if variant == "absent":  # the last class does not occur
        lab[lab == shape[1] - 1] = 0
    elif variant == "ignore":  # a fifth of the pixels
        lab[torch.rand(lab.shape, generator=torch.Generator().manual_seed(sum(shape))) < 0.2] = 255
    return lab


@functools.lru_cache(maxsize=None)
def _probs(shape, dtype):
    """probabilities by a float64 softmax rounded to fp32 or bf16, and what they are worth in fp32"""
    p = torch.softmax(torch.from_numpy(C.logits(shape).copy()).double(), dim=1).to(dtype)
    return p, p.float()


@functools.lru_cache(maxsize=None)
def _logits(shape, dtype, kind="pattern"):
    if kind == "pattern":
        return C.logits_as(shape, dtype)
    x = (2.0 * torch.randn(shape, generator=torch.Generator().manual_seed(3))).to(dtype)
    return x, x.float()


@functools.lru_cache(maxsize=None)
def _ref(shape, dtype, variant, per_image, classes, path):
    xf = _probs(shape, dtype)[1] if path == "probs" else _logits(shape, dtype, path)[1]
    return lovasz_ref(xf, _labels(shape, variant), per_image=per_image, classes=classes,
                      ignore_index=255 if variant == "ignore" else None, from_probs=path == "probs",
                      order="f32" if path == "probs" else "f64")


def _run(d, x, lab, gout=None, **kw):
    xd = x.to(d).clone().requires_grad_(True)  # (a copy on the checker too: x is shared between the tests)
    loss = ops.lovasz_softmax(xd, lab.to(d), **kw)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward(gradient=gout)
    assert xd.grad.dtype == x.dtype and xd.grad.shape == x.shape
    return loss.detach(), xd.grad


def _close_loss(got, ref):
    print(f"loss {got!r} ref {ref!r} |diff| {abs(got - ref):.3e}")
    assert abs(got - ref) < 1e-5 * max(1.0, abs(ref)), (got, ref)


def _close_elementwise(got, ref, rel):
    got = got.double().cpu().numpy()
    err, bound = np.abs(got - ref), rel * np.abs(ref)
    nz = ref != 0
    print(f"grad max |err| / |ref| {float((err[nz] / np.abs(ref[nz])).max()) if nz.any() else 0.0:.3e} (bound {rel:.3e}), "
          f"{int((~nz).sum())} exact zeros")
    assert (err <= bound).all(), float((err - bound).max())


def _close_l2(got, ref, bf16):
    got = got.double().cpu().numpy()
    rel2 = float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
    relmax = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
    print(f"grad rel L2 {rel2:.3e} max |err| / max |ref| {relmax:.3e}")
    if bf16:
        assert rel2 < 1e-2, rel2
    else:
        assert rel2 < 1e-3 and relmax < 2e-3, (rel2, relmax)


# ---- 2. the probability path -----------------------------------------------------------------------------------------------------------
PROB_CASES = [(s, "plain") for s in C.SHAPES + EXTRA] + [(s, v) for v in ("absent", "ignore") for s in [(3, 4, 9, 11), (2, 4, 30, 70)]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,variant", PROB_CASES, ids=[f"{i}-{v}" for i, v in zip(_ids([s for s, _ in PROB_CASES]),
                                                                                     [v for _, v in PROB_CASES])])
def test_probability_path(dev, shape, variant, dtype):
    p = _probs(shape, dtype)[0]
    lab = _labels(shape, variant)
    if variant == "absent":
        assert not bool((lab == shape[1] - 1).any())
    for per_image, classes in COMBOS:
        print(f"per_image={per_image} classes={classes}")
        ref_loss, ref_grad = _ref(shape, dtype, variant, per_image, classes, "probs")
        loss, grad = _run(dev, p, lab, per_image=per_image, classes=classes, from_probs=True,
                          ignore_index=255 if variant == "ignore" else None)
        _close_loss(loss.item(), ref_loss)
        _close_elementwise(grad, ref_grad, 2.0 ** -8 if dtype == BF16 else 1e-5)
        if variant == "ignore":
            assert bool((grad.cpu()[(lab == 255)[:, None].expand_as(grad)] == 0).all())


# ---- 3. the logits path ------------------------------------------------------------------------------------------------------------------
LOGIT_CASES = [(s, "pattern") for s in C.SHAPES] + [((2, 2, 96, 96), "randn")]


@pytest.mark.parametrize("mode", ["plain", "per_image", "ignore"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,kind", LOGIT_CASES, ids=_ids(C.SHAPES) + ["2x2x96x96-randn"])
def test_logits_path(dev, shape, kind, dtype, mode):
    """Observed on the MI355X, the largest over the eight cases of a mode (relative L2; max |got - ref| / max |ref|):
    fp32 gradient: plain 3.3e-5; 1.1e-4, per_image 5.9e-5; 3.7e-4, ignore_index 3.8e-5; 1.4e-4 (bounds 1e-3; 2e-3);
    bf16 gradient relative L2: plain 1.7e-3, per_image 2.0e-3, ignore_index 1.9e-3 (bound 1e-2);
    |loss - ref| at most 7.5e-8 over every loss this file compares."""
    print(f"case {shape} {kind} {dtype} {mode}")
    x = _logits(shape, dtype, kind)[0]
    variant, per_image = "ignore" if mode == "ignore" else "plain", mode == "per_image"
    ref_loss, ref_grad = _ref(shape, dtype, variant, per_image, "present", kind)
    loss, grad = _run(dev, x, _labels(shape, variant), per_image=per_image, ignore_index=255 if mode == "ignore" else None)
    _close_loss(loss.item(), ref_loss)
    _close_l2(grad, ref_grad, dtype == BF16)


# ---- 4. further checks -----------------------------------------------------------------------------------------------------------------
def test_gout_is_honoured(dev):
    """a non-unit gradient of the loss that is a view into the middle of a larger tensor, and the loss used twice in one graph"""
    shape = (3, 4, 9, 11)
    p, pf = _probs(shape, F32)
    lab = _labels(shape)
    gvec = torch.tensor([9.0, -2.5, 9.0]).to(dev)
    loss, grad = _run(dev, p, lab, gout=gvec[1], from_probs=True)
    ref_loss, ref_grad = lovasz_ref(pf, lab, from_probs=True, order="f32", gout=-2.5)
    _close_loss(loss.item(), ref_loss)
    _close_elementwise(grad, ref_grad, 1e-5)
    xd = p.to(dev).clone().requires_grad_(True)
    (ops.lovasz_softmax(xd, lab.to(dev), from_probs=True) * 3.0 + ops.lovasz_softmax(xd, lab.to(dev), from_probs=True)).backward()
    _close_elementwise(xd.grad, 4.0 * _ref(shape, F32, "plain", False, "present", "probs")[1], 1e-5)
    # and on logits
    x = _logits(shape, F32)[0]
    loss, grad = _run(dev, x, lab, gout=gvec[1])
    _close_l2(grad, -2.5 * _ref(shape, F32, "plain", False, "present", "pattern")[1], False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_runs_are_bit_identical(dev, dtype):
    shape = (2, 4, 30, 70)
    x, lab = _logits(shape, dtype)[0], _labels(shape)
    (la, ga), (lb, gb) = (_run(dev, x, lab) for _ in range(2))
    assert ga.data_ptr() != gb.data_ptr()
    bits = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(ga.view(bits), gb.view(bits))


def test_no_valid_pixel_gives_zero(dev):
    x = _logits((3, 4, 9, 11), F32)[0]
    lab = torch.full((3, 9, 11), 255.0)
    for per_image, classes in COMBOS:
        loss, grad = _run(dev, x, lab, per_image=per_image, classes=classes, ignore_index=255)
        assert loss.item() == 0.0 and bool((grad == 0).all())


def test_refusals(dev):
    x, lab = torch.zeros(2, 4, 5, 6, device=dev), torch.zeros(2, 5, 6, device=dev)
    with pytest.raises(ValueError, match="K"):
        ops.lovasz_softmax(x[:, :1], lab)
    with pytest.raises(ValueError, match="K"):
        ops.lovasz_softmax(torch.zeros(2, 17, 5, 6, device=dev), lab)
    with pytest.raises(ValueError, match="classes"):
        ops.lovasz_softmax(x, lab, classes="foreground")
    with pytest.raises(ValueError, match="classes"):
        losses.LovaszSoftmaxLoss(classes="foreground")
    for bad_x, bad_lab in ((x, lab[:, :4]), (x, lab[:1]), (x[0], lab)):
        with pytest.raises(ValueError, match="expected"):
            ops.lovasz_softmax(bad_x, bad_lab)
    with pytest.raises(ValueError, match="fp32"):
        ops.lovasz_order(torch.zeros(5, device=dev))
    # a workspace four bytes short: the ABI's error, nothing is launched
    ws = torch.empty(kern.lovasz_ws_bytes(2, 4, 5, 6, False) // 4, dtype=torch.int32, device=dev)
    coef, out = torch.full((2, 4, 5, 6), -3.5).to(dev), torch.full((1,), -3.5).to(dev)
    with pytest.raises(RuntimeError, match="cenet_lovasz_fwd_f32 failed with error code 1"):
        kern.lovasz_fwd(x, lab, ws[:-1], coef, out, 2, 4, 5, 6, False, False, None, False)
    with pytest.raises(ValueError, match="sizes"):
        kern.lovasz_fwd(x, lab[:1], ws, coef, out, 2, 4, 5, 6, False, False, None, False)
    with pytest.raises(ValueError, match="alias"):
        kern.lovasz_bwd(x, coef, out, x, 2, 4, 5, 6, False)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert out.item() == -3.5 and bool((coef == -3.5).all())
    with pytest.raises(NotImplementedError, match="focal"):
        losses.Criterion(4, _args("lovasz,focal", "0.5,0.5"))
    with pytest.raises(ValueError, match="lovasz_classes"):
        losses.Criterion(4, _args("dice,lovasz", "0.5,0.5", lovasz_classes="foreground"))


# ---- losses.py -----------------------------------------------------------------------------------------------------------------------
def _args(loss_type, loss_weights, **kw):
    return argparse.Namespace(loss_type=loss_type, loss_weights=loss_weights, **kw)


def _crit_run(d, crit, x, lab):
    xd = x.to(d).clone().requires_grad_(True)
    loss = crit.to(d)(xd, lab.to(d))
    loss.backward()
    return loss.detach(), xd.grad


@pytest.mark.parametrize("dtype", DTYPES)
def test_criterion_adds_the_weighted_term(dev, dtype):
    shape = (2, 4, 30, 70)
    x, lab = _logits(shape, dtype)[0], _labels(shape)
    loss, grad = _crit_run(dev, losses.Criterion(4, _args("dice,ce,lovasz", "0.4,0.4,0.2")), x, lab)
    parts = [_crit_run(dev, m, x, lab) for m in (losses.Criterion(4, _args("dice", "1")), losses.Criterion(4, _args("ce", "1")),
                                                  losses.LovaszSoftmaxLoss())]
    want = sum(w * l.double().item() for w, (l, _) in zip((0.4, 0.4, 0.2), parts))
    print(f"loss {loss.item()!r} weighted sum {want!r}")
    assert abs(loss.item() - want) < 1e-6 * abs(want)
    want_grad = sum(w * g.double().cpu().numpy() for w, (_, g) in zip((0.4, 0.4, 0.2), parts))
    _close_l2(grad, want_grad, dtype == BF16)
    # LovaszSoftmaxLoss is the restatement; the optional attributes reach the op; lovasz alone computes nothing else
    _close_loss(parts[2][0].item(), _ref(shape, dtype, "plain", False, "present", "pattern")[0])
    crit = losses.Criterion(4, _args("lovasz", "1.0", lovasz_per_image=True, lovasz_classes="all", ignore_index=255))
    assert not crit.has_base and crit.lovasz_per_image and crit.lovasz_classes == "all"
    got = _crit_run(dev, crit, x, _labels(shape, "ignore"))[0].item()
    _close_loss(got, lovasz_ref(_logits(shape, dtype)[1], _labels(shape, "ignore"), per_image=True, classes="all",
                                ignore_index=255)[0])


def test_criterion_without_the_name_is_the_path_it_was(dev, monkeypatch):
    shape = (3, 4, 9, 11)
    x, lab = _logits(shape, F32)[0], _labels(shape)
    calls = []
    for owner, name in ((ops, "lovasz_softmax"), (kern, "lovasz_fwd"), (kern, "lovasz_bwd"), (kern, "lovasz_ws_bytes")):
        def wrapper(*a, _real=getattr(owner, name), _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(owner, name, wrapper)
    crit = losses.Criterion(4, _args("dice,ce", "0.5,0.5"))
    assert not crit.has_lovasz
    loss, grad = _crit_run(dev, crit, x, lab)
    xd = x.to(dev).clone().requires_grad_(True)
    direct = ops.dice_ce_loss(xd, lab.to(dev), 0.5, 0.5)
    direct.backward()
    assert calls == []
    assert torch.equal(loss.view(torch.int32), direct.detach().view(torch.int32))
    assert torch.equal(grad.view(torch.int32), xd.grad.view(torch.int32))
    _crit_run(dev, losses.Criterion(4, _args("dice,ce,lovasz", "0.5,0.5,0.5")), x, lab)
    assert calls.count("lovasz_softmax") == 1 and calls.count("lovasz_fwd") == 1 and calls.count("lovasz_bwd") == 1
