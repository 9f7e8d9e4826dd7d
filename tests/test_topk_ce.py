"""The top-k cross-entropy (csrc/topk_ce.hip, ops.topk_ce / ops.topk_mask, losses.TopKCrossEntropyLoss / Criterion) against
tests/topk_ref.py, the float64 restatement of its definition.  Every case runs on the host SIMT checker and, marked gpu, on the
MI355X.

1. The selection alone: ops.topk_mask equals numpy's stable selection argsort(-v, kind="stable")[:m] element for element.
2. Loss and gradient.  The device orders by its fp32 losses, the reference by the float64 ones; a pixel whose loss lies within
   topk_ref.DELTA = 2^-16 of the threshold (the near-tie set N) may fall on either side.  N is capped on the reference BEFORE the
   device runs (|N| <= max(2, n / 500) per segment); then: |loss - ref| < 1e-5 max(1, |ref|); the count of kept pixels per segment
   equals m exactly; every pixel outside N has the reference's kept status; gradient exactly 0 on pixels neither kept nor in N;
   on kept pixels |got - ref| <= 1e-5 |gout| wgt_i per element (wgt_i is the scale of the gradient; absolute because p - 1
   cancels; ten fp32 roundings with a tenfold margin), bf16 adds 2^-8 |ref| for the output rounding; a pixel of N has either
   exact zeros or the kept form within the same bound.
3. k = 100 is the cross-entropy mean.  4. Exact tie blocks go by pixel index; two runs are bit-identical.
5. gout, nothing valid, labels that are no class, m floored to 0, refusals.  6. Criterion."""
import argparse
import functools

import numpy as np
import pytest
import torch

import dist_cases as C
from backend import dev  # noqa: F401
from cenet_amd import kern, losses, ops
from test_lovasz import _order_inputs
from topk_ref import kept_count, topk_ref

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
SHAPES = C.SHAPES + [(2, 2, 96, 96), (1, 9, 64, 64)]
KS = (10.0, 50.0, 100.0)


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ---- 1. the selection alone ----------------------------------------------------------------------------------------------------------
LENGTHS = {"1": lambda t: 1, "5": lambda t: 5, "63": lambda t: 63, "64": lambda t: 64, "65": lambda t: 65,
           "tile-1": lambda t: t - 1, "tile": lambda t: t, "3tiles+1": lambda t: 3 * t + 1}


def _counts(n):
    """m in {1, 2, n / 10 or 1, n - 1 or 1, n}, each within [1, n]"""
    return [min(1, n), min(2, n), max(n // 10, 1), max(n - 1, 1), n]


def _select(v, m):
    ref = np.zeros(v.shape, np.uint8)
    for s in range(v.shape[0]):
        ref[s, np.argsort(-v[s], kind="stable")[:m[s]]] = 1
    return ref


def _check_mask(d, v, m, what):
    got = ops.topk_mask(torch.from_numpy(v).to(d), m)
    assert got.dtype == torch.uint8 and tuple(got.shape) == v.shape
    got, ref = got.cpu().numpy(), _select(v, m)
    assert np.array_equal(got.sum(axis=1), np.asarray(m)), what
    assert np.array_equal(got, ref), what
    return got


@pytest.mark.parametrize("S", [1, 3, 40])
@pytest.mark.parametrize("length", list(LENGTHS))
def test_mask_is_the_stable_selection(dev, length, S):
    """every count with every value family: one segment takes the five counts in turn; several segments take a different count
    each, moved on by one from family to family"""
    n = LENGTHS[length](kern.topk_tile())
    counts = _counts(n)
    for f, (what, v) in enumerate(_order_inputs(S, n, 100 * S + n).items()):
        for j in (range(len(counts)) if S == 1 else [f]):
            m = [counts[(s + j) % len(counts)] for s in range(S)]
            got = _check_mask(dev, v, m, (what, S, n, m))
            if what == "all equal":  # the threshold lies inside the one tie group: the kept ones are the first by index
                for s in range(S):
                    assert got[s, :m[s]].all() and not got[s, m[s]:].any()


def test_mask_with_a_threshold_inside_a_tie_group(dev):
    """eight levels over three tiles and a tile's worth of segments' counts: the kept ties are the first r of their level"""
    n = 3 * kern.topk_tile() + 1
    v = _order_inputs(3, n, 11)["eight levels"]
    m = [n // 10, n // 2, n - 7]
    got = _check_mask(dev, v, m, "eight levels")
    for s in range(3):
        tau = np.sort(v[s])[::-1][m[s] - 1]
        ties = np.flatnonzero(v[s] == tau)
        r = int(got[s, ties].sum())
        assert 1 <= r < ties.size, "the case is meant to cut a tie group"
        assert got[s, ties[:r]].all() and not got[s, ties[r:]].any()


def test_mask_of_values_that_differ_in_the_lowest_byte_only(dev):
    """rounds 0 to 2 of the select each see a single non-empty bin"""
    n = 3 * kern.topk_tile() + 1
    rng = np.random.default_rng(17)
    bits = (np.uint32(0x3F000000) + rng.integers(0, 256, (3, n)).astype(np.uint32))
    v = bits.view(np.float32)
    assert (v > 0).all() and np.unique(bits >> 8).size == 1
    _check_mask(dev, v, [1, n // 10, n - 1], "lowest byte")


def test_mask_over_more_tiles_than_a_scan_step_takes(dev):
    """300 tiles: the scan of the tie counts over the tiles of a segment takes two steps of 64 lanes with four values each"""
    n = 300 * kern.topk_tile() + 3
    rng = np.random.default_rng(5)
    _check_mask(dev, (rng.integers(0, 1000, (1, n)) / 999).astype(np.float32), [n // 10], "thousand levels")


# ---- the cases of 2 and 3 ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _labels(shape, variant="plain"):
    B, K, H, W = shape
    g = torch.Generator().manual_seed(1001 + sum(shape))
    lab = torch.randint(0, K, (B, H, W), generator=g).float()
    if variant == "ignore":  # a fifth of the pixels
        lab[torch.rand(lab.shape, generator=g) < 0.2] = 255
    return lab


@functools.lru_cache(maxsize=None)
def _logits(shape, dtype):
    """2 randn from the shape's seed, and what it is worth in fp32 (seeds 1 + sum(shape) / 1001 + sum(shape): with 0 / 1000 the
    float64 reference of (5, 2, 33, 33) bf16 per_image has 3 near-ties in a segment of 1089, above the cap)"""
    x = (2.0 * torch.randn(shape, generator=torch.Generator().manual_seed(1 + sum(shape)))).to(dtype)
    return x, x.float()


@functools.lru_cache(maxsize=None)
def _ref(shape, dtype, variant, per_image, k):
    return topk_ref(_logits(shape, dtype)[1].numpy(), _labels(shape, variant).numpy(), k, per_image=per_image,
                    ignore_index=255 if variant == "ignore" else None)


def _run(d, x, lab, k=10.0, gout=None, **kw):
    xd = x.to(d).clone().requires_grad_(True)  # (a copy on the checker too: x is shared between the tests)
    loss = ops.topk_ce(xd, lab.to(d), k, **kw)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward(gradient=gout)
    assert xd.grad.dtype == x.dtype and xd.grad.shape == x.shape
    return loss.detach(), xd.grad


def _weights(d, x, lab, k, per_image=False, ignore_index=None):
    """the forward through kern alone: (loss, wgt [B,H,W])"""
    B, K, H, W = x.shape
    ws = torch.empty(kern.topk_ce_ws_bytes(B, H, W, per_image) // 4, dtype=torch.int32, device=d)
    wgt, out = torch.empty(B, H, W, device=d), torch.empty(1, device=d)
    kern.topk_ce_fwd(x.to(d).contiguous(), lab.to(d), torch.tensor([k], dtype=torch.float32).to(d), ws, wgt, out, B, K, H, W,
                     per_image, ignore_index)
    return out[0], wgt.cpu().numpy()


def _close_loss(got, ref):
    print(f"loss {got!r} ref {ref!r} |diff| {abs(got - ref):.3e}")
    assert abs(got - ref) < 1e-5 * max(1.0, abs(ref)), (got, ref)


def _check_against(ref, loss, wgt, grad, bf16, gout=1.0):
    """the conditions of 2 on one result; wgt may be None (then the kept set is read off the gradient's zeros is NOT done: only
    the gradient conditions are checked)"""
    _close_loss(loss, ref.loss * 1.0)
    free = ref.near
    if wgt is not None:
        got_kept = wgt != 0
        for seg, m in zip(ref.segments, ref.m):
            assert int(got_kept.reshape(-1)[seg].sum()) == m, (int(got_kept.reshape(-1)[seg].sum()), m)
        assert np.array_equal(got_kept[~free], ref.kept[~free]), int((got_kept != ref.kept)[~free].sum())
        print(f"near-ties {int(free.sum())}, of which decided otherwise than the reference {int((got_kept != ref.kept)[free].sum())}")
    g = grad.double().cpu().numpy()
    bound = 1e-5 * abs(gout) * ref.scale[:, None] + (2.0 ** -8 * np.abs(ref.kept_form) if bf16 else 0.0)
    err = np.abs(g - ref.kept_form)
    zero = (g == 0).all(axis=1)
    fixed_kept, fixed_out = ref.kept & ~free, ~ref.kept & ~free
    assert zero[fixed_out].all(), int((~zero[fixed_out]).sum())
    within = (err <= bound).all(axis=1)
    assert within[fixed_kept].all(), float((err - bound)[np.broadcast_to(fixed_kept[:, None], err.shape)].max())
    assert (zero | within)[free].all()
    sc = np.broadcast_to(ref.scale[:, None], err.shape)[np.broadcast_to(fixed_kept[:, None], err.shape)]
    rel = err[np.broadcast_to(fixed_kept[:, None], err.shape)] / (abs(gout) * sc)
    print(f"grad max |err| / (|gout| wgt) on kept pixels {float(rel.max()) if rel.size else 0.0:.3e}")


# ---- 2. loss and gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "per_image", "ignore"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_loss_and_gradient(dev, shape, dtype, mode):
    """Observed on the MI355X, the largest over the 27 cases (9 shapes, 3 percentages) of a mode and type:
    |loss - ref|: fp32 4.7e-7 (plain), 3.6e-7 (per_image), 2.7e-7 (ignore_index); bf16 4.3e-7, 2.6e-7, 7.0e-7 (bound 1e-5);
    gradient error on kept pixels over |gout| wgt_i: fp32 2.5e-7, 2.5e-7, 2.6e-7 (bound 1e-5); bf16 3.6e-3 in all three (bound
    1e-5 + 2^-8 |ref| / (|gout| wgt_i), up to 3.9e-3);
    near-ties per segment: fp32 at most 1, bf16 at most 4 (plain), 7 (per_image), 3 (ignore_index) — the device decided every one
    of them as the float64 order does."""
    variant, per_image = "ignore" if mode == "ignore" else "plain", mode == "per_image"
    ignore_index = 255 if mode == "ignore" else None
    x, lab = _logits(shape, dtype)[0], _labels(shape, variant)
    refs = [_ref(shape, dtype, variant, per_image, k) for k in KS]
    for k, ref in zip(KS, refs):  # the cap on the near-ties is a condition on the inputs: before the device runs
        for seg in ref.segments:
            assert int(ref.near.reshape(-1)[seg].sum()) <= max(2, seg.size / 500), (k, int(ref.near.reshape(-1)[seg].sum()))
    for k, ref in zip(KS, refs):
        print(f"case {shape} {dtype} {mode} k={k} m={ref.m}")
        loss, grad = _run(dev, x, lab, k, per_image=per_image, ignore_index=ignore_index)
        loss2, wgt = _weights(dev, x, lab, k, per_image, ignore_index)
        assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32))
        _check_against(ref, loss.item(), wgt, grad, dtype == BF16)
        if mode == "ignore":
            assert bool((grad.cpu()[(lab == 255)[:, None].expand_as(grad)] == 0).all())


# ---- 3. k = 100 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "ignore"])
def test_all_pixels_kept_is_the_cross_entropy_mean(dev, variant):
    shape = (2, 4, 30, 70)
    x, lab = _logits(shape, F32)[0], _labels(shape, variant)
    want = torch.nn.functional.cross_entropy(x.double(), lab.long(), ignore_index=255).item()
    loss, wgt = _weights(dev, x, lab, 100.0, False, 255 if variant == "ignore" else None)
    _close_loss(loss.item(), want)
    valid = (lab != 255).numpy()
    assert (wgt[valid] == np.float32(1.0 / valid.sum())).all() and (wgt[~valid] == 0).all()
    _close_loss(_run(dev, x, lab, 100.0, ignore_index=255 if variant == "ignore" else None)[0].item(), want)


# ---- 4. exact tie blocks ----------------------------------------------------------------------------------------------------------------
def _tiled(shape, dtype, second_every=None):
    """one pixel's logits and label over the whole batch; second_every: every so-manieth pixel of the flattened image is of a
    second population with a larger loss"""
    B, K, H, W = shape
    one = torch.tensor([1.25, -0.5, 0.75, 2.0][:K])
    x = one.view(1, K, 1, 1).expand(B, K, H, W).clone()
    lab = torch.full((B, H, W), 2.0)
    if second_every:
        hard = (torch.arange(H * W) % second_every == 3).view(1, H, W).expand(B, H, W)
        x = torch.where(hard[:, None], torch.tensor([3.0, -1.0, -2.5, 0.5][:K]).view(1, K, 1, 1).expand(B, K, H, W), x)
    else:
        hard = torch.zeros(B, H, W, dtype=torch.bool)
    return x.to(dtype), lab, hard.numpy()


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "per_image"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_ties_go_by_pixel_index(dev, dtype, per_image):
    shape = (2, 4, 30, 70)
    B, n_img = 2, 30 * 70
    for second_every in (None, 5):
        x, lab, hard = _tiled(shape, dtype, second_every)
        (la, ga), (lb, gb) = (_run(dev, x, lab, 30.0, per_image=per_image) for _ in range(2))
        wgt = _weights(dev, x, lab, 30.0, per_image)[1]
        kept = (wgt != 0).reshape(B if per_image else 1, -1)
        hard = hard.reshape(kept.shape)
        for s in range(kept.shape[0]):
            m = kept_count(kept.shape[1], 30.0)
            n_hard = int(hard[s].sum())
            assert n_hard < m, "the threshold is meant to fall into the population with the lower loss"
            want = hard[s].copy()
            want[np.flatnonzero(~hard[s])[:m - n_hard]] = True  # every harder pixel, then the first r of the others by index
            assert np.array_equal(kept[s], want), (second_every, s)
        assert ga.data_ptr() != gb.data_ptr()
        bits = torch.int16 if dtype == BF16 else torch.int32
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(ga.view(bits), gb.view(bits))
        assert np.array_equal((ga.float().cpu().numpy() != 0).any(axis=1).reshape(kept.shape), kept)


# ---- 5. further checks -----------------------------------------------------------------------------------------------------------------
def test_gout_is_honoured(dev):
    """a non-unit gradient of the loss that is a view into the middle of a larger tensor, and the loss used twice in one graph"""
    shape = (3, 4, 9, 11)
    x, lab = _logits(shape, F32)[0], _labels(shape)
    gvec = torch.tensor([9.0, -2.5, 9.0]).to(dev)
    loss, grad = _run(dev, x, lab, 50.0, gout=gvec[1])
    ref = topk_ref(x.numpy(), lab.numpy(), 50.0, gout=-2.5)
    assert not ref.near.any()
    _check_against(ref, loss.item(), None, grad, False, gout=-2.5)
    xd = x.to(dev).clone().requires_grad_(True)
    (ops.topk_ce(xd, lab.to(dev), 50.0) * 3.0 + ops.topk_ce(xd, lab.to(dev), 50.0)).backward()
    _check_against(topk_ref(x.numpy(), lab.numpy(), 50.0, gout=4.0), loss.item(), None, xd.grad, False, gout=4.0)


def test_no_valid_pixel_gives_zero(dev):
    x = _logits((3, 4, 9, 11), F32)[0]
    lab = torch.full((3, 9, 11), 255.0)
    for per_image in (False, True):
        loss, grad = _run(dev, x, lab, per_image=per_image, ignore_index=255)
        assert loss.item() == 0.0 and bool((grad == 0).all())
    # one image without a valid pixel: the mean is over the other two
    lab = _labels((3, 4, 9, 11)).clone()
    lab[1] = 255.0
    loss, grad = _run(dev, x, lab, 50.0, per_image=True, ignore_index=255)
    ref = topk_ref(x.numpy(), lab.numpy(), 50.0, per_image=True, ignore_index=255)
    assert ref.m[1] == 0 and not ref.near.any()
    _check_against(ref, loss.item(), _weights(dev, x, lab, 50.0, True, 255)[1], grad, False)


def test_a_label_that_is_no_class_is_invalid(dev):
    shape = (3, 4, 9, 11)
    x, lab = _logits(shape, F32)[0], _labels(shape).clone()
    lab[0, :3], lab[2, 4:] = -1.0, 4.0
    ref = topk_ref(x.numpy(), lab.numpy(), 50.0)
    assert ref.n_valid[0] == 3 * 99 - 3 * 11 - 5 * 11 and not ref.near.any()
    loss, grad = _run(dev, x, lab, 50.0)
    _check_against(ref, loss.item(), _weights(dev, x, lab, 50.0)[1], grad, False)
    assert bool((grad.cpu()[0, :, :3] == 0).all()) and bool((grad.cpu()[2, :, 4:] == 0).all())


def test_a_count_that_floors_to_zero_becomes_one(dev):
    shape = (1, 2, 1, 5)
    x, lab = _logits(shape, F32)[0], _labels(shape)
    ref = topk_ref(x.numpy(), lab.numpy(), 10.0)
    assert ref.m == [1]
    loss, grad = _run(dev, x, lab, 10.0)
    wgt = _weights(dev, x, lab, 10.0)[1]
    assert int((wgt != 0).sum()) == 1 and wgt.max() == 1.0
    _check_against(ref, loss.item(), wgt, grad, False)


def test_refusals(dev):
    x, lab = torch.zeros(2, 4, 5, 6, device=dev), torch.zeros(2, 5, 6, device=dev)
    with pytest.raises(ValueError, match="K"):
        ops.topk_ce(x[:, :1], lab)
    with pytest.raises(ValueError, match="K"):
        ops.topk_ce(torch.zeros(2, 17, 5, 6, device=dev), lab)
    for bad_x, bad_lab in ((x, lab[:, :4]), (x, lab[:1]), (x[0], lab)):
        with pytest.raises(ValueError, match="expected"):
            ops.topk_ce(bad_x, bad_lab)
    for bad_k in (0.0, -1.0, 100.5):
        with pytest.raises(ValueError, match="percentage"):
            ops.topk_ce(x, lab, bad_k)
    with pytest.raises(ValueError, match="percentage"):
        losses.TopKCrossEntropyLoss(k=0)
    with pytest.raises(ValueError, match="fp32"):
        ops.topk_mask(torch.zeros(5, device=dev), 1)
    # a workspace four bytes short: the ABI's error, nothing is launched
    kp = torch.tensor([10.0]).to(dev)
    ws = torch.empty(kern.topk_ce_ws_bytes(2, 5, 6, False) // 4, dtype=torch.int32, device=dev)
    wgt, out = torch.full((2, 5, 6), -3.5).to(dev), torch.full((1,), -3.5).to(dev)
    with pytest.raises(RuntimeError, match="cenet_topk_ce_fwd_f32 failed with error code 1"):
        kern.topk_ce_fwd(x, lab, kp, ws[:-1], wgt, out, 2, 4, 5, 6, False, None)
    mws = torch.empty(kern.topk_mask_ws_bytes(2, 30) // 4, dtype=torch.int32, device=dev)
    mask = torch.full((2, 30), 7, dtype=torch.uint8).to(dev)
    with pytest.raises(RuntimeError, match="cenet_topk_mask_f32 failed with error code 1"):
        kern.topk_mask(lab.reshape(2, 30), torch.ones(2, dtype=torch.int32).to(dev), mws[:-1], mask, 2, 30)
    with pytest.raises(ValueError, match="sizes"):
        kern.topk_ce_fwd(x, lab[:1], kp, ws, wgt, out, 2, 4, 5, 6, False, None)
    with pytest.raises(ValueError, match="alias"):
        kern.topk_ce_bwd(x, lab, wgt, out, x, 2, 4, 5, 6, None)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert out.item() == -3.5 and bool((wgt == -3.5).all()) and bool((mask == 7).all())
    with pytest.raises(NotImplementedError, match="focal"):
        losses.Criterion(4, _args("topk,focal", "0.5,0.5"))
    with pytest.raises(ValueError, match="topk"):
        losses.Criterion(4, _args("dice,ce", "0.5,0.5")).set_topk_percent(20.0)


# ---- 6. losses.py ----------------------------------------------------------------------------------------------------------------------
def _args(loss_type, loss_weights, **kw):
    return argparse.Namespace(loss_type=loss_type, loss_weights=loss_weights, **kw)


def _crit_run(d, crit, x, lab):
    xd = x.to(d).clone().requires_grad_(True)
    loss = crit.to(d)(xd, lab.to(d))
    loss.backward()
    return loss.detach(), xd.grad


def _close_l2(got, ref, bf16):
    """the gradient bounds of tests/test_lovasz.py"""
    got = got.double().cpu().numpy()
    rel2 = float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
    relmax = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
    print(f"grad rel L2 {rel2:.3e} max |err| / max |ref| {relmax:.3e}")
    if bf16:
        assert rel2 < 1e-2, rel2
    else:
        assert rel2 < 1e-3 and relmax < 2e-3, (rel2, relmax)


@pytest.mark.parametrize("dtype", DTYPES)
def test_criterion_adds_the_weighted_term(dev, dtype):
    shape = (2, 4, 30, 70)
    x, lab = C.logits_as(shape, dtype)[0], torch.from_numpy(C.labels(shape).copy())
    loss, grad = _crit_run(dev, losses.Criterion(4, _args("dice,ce,topk", "0.4,0.4,0.2")), x, lab)
    parts = [_crit_run(dev, m, x, lab) for m in (losses.Criterion(4, _args("dice", "1")), losses.Criterion(4, _args("ce", "1")),
                                                  losses.TopKCrossEntropyLoss())]
    want = sum(w * l.double().item() for w, (l, _) in zip((0.4, 0.4, 0.2), parts))
    print(f"loss {loss.item()!r} weighted sum {want!r}")
    assert abs(loss.item() - want) < 1e-6 * abs(want)
    want_grad = sum(w * g.double().cpu().numpy() for w, (_, g) in zip((0.4, 0.4, 0.2), parts))
    _close_l2(grad, want_grad, dtype == BF16)
    # TopKCrossEntropyLoss is the restatement; the optional attributes reach the op; topk alone computes nothing else
    xr, labr = _logits(shape, dtype), _labels(shape, "ignore")
    _close_loss(_crit_run(dev, losses.TopKCrossEntropyLoss(), xr[0], _labels(shape))[0].item(), _ref(shape, dtype, "plain", False, 10.0).loss)
    crit = losses.Criterion(4, _args("topk", "1.0", topk_percent=50.0, topk_per_image=True, ignore_index=255))
    assert not crit.has_base and crit.topk_per_image and crit.topk_percent.tolist() == [50.0]
    assert "topk_percent" in dict(crit.named_buffers())
    _close_loss(_crit_run(dev, crit, xr[0], labr)[0].item(), _ref(shape, dtype, "ignore", True, 50.0).loss)


def test_set_topk_percent_reaches_the_next_call(dev):
    shape = (2, 4, 30, 70)
    x, lab = _logits(shape, F32)[0], _labels(shape)
    crit = losses.Criterion(4, _args("topk", "1.0"))
    _close_loss(_crit_run(dev, crit, x, lab)[0].item(), _ref(shape, F32, "plain", False, 10.0).loss)
    buf = crit.topk_percent
    crit.set_topk_percent(50)
    assert crit.topk_percent is buf and buf.device.type == dev.type
    _close_loss(_crit_run(dev, crit, x, lab)[0].item(), _ref(shape, F32, "plain", False, 50.0).loss)
    crit.set_topk_percent(torch.tensor(100.0).to(dev))
    _close_loss(_crit_run(dev, crit, x, lab)[0].item(), _ref(shape, F32, "plain", False, 100.0).loss)
    with pytest.raises(ValueError, match="percentage"):
        crit.set_topk_percent(0)


NEW_NAMES = ((ops, "topk_ce"), (ops, "topk_mask"), (kern, "topk_ce_fwd"), (kern, "topk_ce_bwd"), (kern, "topk_ce_ws_bytes"),
             (kern, "topk_mask"), (kern, "topk_mask_ws_bytes"), (kern, "topk_tile"))


def test_criterion_without_the_name_is_the_path_it_was(dev, monkeypatch):
    shape = (3, 4, 9, 11)
    x, lab = C.logits_as(shape, F32)[0], torch.from_numpy(C.labels(shape).copy())
    calls = []
    for owner, name in NEW_NAMES:
        def wrapper(*a, _real=getattr(owner, name), _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(owner, name, wrapper)
    crit = losses.Criterion(4, _args("dice,ce", "0.5,0.5"))
    assert not crit.has_topk and crit.topk_percent is None
    loss, grad = _crit_run(dev, crit, x, lab)
    xd = x.to(dev).clone().requires_grad_(True)
    direct = ops.dice_ce_loss(xd, lab.to(dev), 0.5, 0.5)
    direct.backward()
    assert calls == []
    assert torch.equal(loss.view(torch.int32), direct.detach().view(torch.int32))
    assert torch.equal(grad.view(torch.int32), xd.grad.view(torch.int32))
    _crit_run(dev, losses.Criterion(4, _args("dice,ce,topk", "0.5,0.5,0.5")), x, lab)
    assert calls.count("topk_ce") == 1 and calls.count("topk_ce_fwd") == 1 and calls.count("topk_ce_bwd") == 1
