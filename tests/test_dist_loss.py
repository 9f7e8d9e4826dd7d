"""The distance-map losses (csrc/dist_loss.hip, ops.dist_loss, losses.SurfaceLoss / HausdorffDTLoss / Criterion) against a
float64 restatement of their formulas on scipy's distance maps, gradient by autograd with the maps as constants.  Same cases as
tests/test_dist_maps.py, fp32 and bf16 logits (the restatement consumes the same rounded logits).  Every case runs on the host
SIMT checker and, marked gpu, on the MI355X.

Tolerances: |loss - ref| < 1e-5 max(1, |ref|); fp32 gradient rtol 1e-3 and atol 1e-8 max(1, Dmax), Dmax the largest factor
(|phi| or d2g + d2p) of the case — every addend of the gradient carries one such factor, so its absolute rounding scales with it;
bf16 gradient: relative L2 error < 1e-2, the figure tests/test_bf16_storage.py::test_seg_loss uses."""
import argparse
import functools

import numpy as np
import pytest
import torch

import dist_cases as C
from backend import dev  # noqa: F401
from cenet_amd import _lib, kern, losses, ops

DTYPES = [pytest.param(torch.float32, id="f32"), pytest.param(torch.bfloat16, id="bf16")]
# (w_surface, w_hausdorff, surface present, hausdorff present)
MODES = {"surface": (1.0, 0.0, True, False), "hausdorff": (0.0, 1.0, False, True), "both": (0.7, 0.01, True, True)}


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _terms(x64, lab, d2g, d2p):
    """(L_surf, L_hd, largest |phi|, largest d2g + d2p) in float64; x64 [B,K,H,W], lab [B,H,W], maps [B,K-1,H,W] constants"""
    K = x64.shape[1]
    p = torch.softmax(x64, dim=1)[:, 1:]
    g = torch.stack([lab == c for c in range(1, K)], dim=1)
    dg, dp = d2g.double(), d2p.double()
    phi = torch.where(g, -(dg.sqrt() - 1.0), dg.sqrt())
    n = p.numel()
    return (p * phi).sum() / n, ((p - g.double()) ** 2 * (dg + dp)).sum() / n, float(phi.abs().max()), float((dg + dp).max())


def restate(x_f32, lab, d2g, d2p, ws, wh, surface, hausdorff, gout=1.0):
    """-> (loss, dloss/dlogits * gout as float64 numpy, Dmax)"""
    x = x_f32.double().requires_grad_(True)
    ls, lh, phimax, dmax = _terms(x, lab, d2g, d2p)
    loss = (ws * ls if surface else 0.0) + (wh * lh if hausdorff else 0.0)
    (grad,) = torch.autograd.grad(loss * gout, x)
    return float(loss.detach()), grad.numpy(), max(phimax if surface else 0.0, dmax if hausdorff else 0.0)


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    x, xf = C.logits_as(shape, dtype)
    lab = torch.from_numpy(C.labels(shape).copy())
    return x, xf, lab, torch.from_numpy(C.label_maps(shape).copy()), torch.from_numpy(C.pred_maps(shape, dtype).copy())


@functools.lru_cache(maxsize=None)
def _ref(shape, dtype, mode):
    x, xf, lab, d2g, d2p = _case(shape, dtype)
    return restate(xf, lab, d2g, d2p, *MODES[mode])


def _close_loss(got, ref):
    print(f"loss {got!r} ref {ref!r} |diff| {abs(got - ref):.3e}")
    assert abs(got - ref) < 1e-5 * max(1.0, abs(ref)), (got, ref)


def _close_grad(got, ref, dmax, bf16):
    got = got.double().cpu().numpy()
    err = np.abs(got - ref)
    rel2 = float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
    print(f"grad max |err| {err.max():.3e} rel L2 {rel2:.3e} Dmax {dmax}")
    if bf16:
        assert rel2 < 1e-2, rel2
    else:
        bound = 1e-8 * max(1.0, dmax) + 1e-3 * np.abs(ref)
        assert (err <= bound).all(), float((err - bound).max())


def _lib_loss(d, x, lab, weights, surface, hausdorff, gout=None):
    xd = x.to(d).clone().requires_grad_(True)  # (a copy on the checker too: x is shared between the tests)
    loss = ops.dist_loss(xd, lab.to(d), weights, surface=surface, hausdorff=hausdorff)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward(gradient=gout)
    assert xd.grad.dtype == x.dtype and xd.grad.shape == x.shape
    return loss.detach(), xd.grad


# ---- the cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_loss_and_gradient(dev, shape, dtype, mode):
    x, _, lab, _, _ = _case(shape, dtype)
    ws, wh, surface, hausdorff = MODES[mode]
    ref_loss, ref_grad, dmax = _ref(shape, dtype, mode)
    loss, grad = _lib_loss(dev, x, lab, (ws, wh), surface, hausdorff)
    _close_loss(loss.item(), ref_loss)
    _close_grad(grad, ref_grad, dmax, dtype == torch.bfloat16)


def test_gout_is_honoured(dev):
    """a non-unit gradient of the loss that is a view into the middle of a larger tensor"""
    shape = (3, 4, 9, 11)
    x, xf, lab, d2g, d2p = _case(shape, torch.float32)
    gvec = torch.tensor([9.0, -2.5, 9.0]).to(dev)
    loss, grad = _lib_loss(dev, x, lab, (0.7, 0.01), True, True, gout=gvec[1])
    ref_loss, ref_grad, dmax = restate(xf, lab, d2g, d2p, 0.7, 0.01, True, True, gout=-2.5)
    _close_loss(loss.item(), ref_loss)
    _close_grad(grad, ref_grad, 2.5 * dmax, False)
    # and through a graph that scales and adds it
    xd = x.to(dev).clone().requires_grad_(True)
    (ops.dist_loss(xd, lab.to(dev), (0.7, 0.01)) * 3.0 + ops.dist_loss(xd, lab.to(dev), (0.7, 0.01))).backward()
    _close_grad(xd.grad, 4.0 * _ref(shape, torch.float32, "both")[1], 4.0 * dmax, False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_runs_are_bit_identical(dev, dtype):
    shape = (2, 4, 30, 70)
    x, _, lab, _, _ = _case(shape, dtype)
    (la, ga), (lb, gb) = (_lib_loss(dev, x, lab, (0.7, 0.01), True, True) for _ in range(2))
    assert ga.data_ptr() != gb.data_ptr()
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert torch.equal(ga.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       gb.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))


def test_weights_in_a_device_tensor_are_read_at_every_call(dev):
    shape = (2, 4, 30, 70)
    x, xf, lab, d2g, d2p = _case(shape, torch.float32)
    w = torch.tensor([0.7, 0.01]).to(dev)
    ptr = w.data_ptr()
    loss, grad = _lib_loss(dev, x, lab, w, True, True)
    ref = _ref(shape, torch.float32, "both")
    _close_loss(loss.item(), ref[0])
    _close_grad(grad, ref[1], ref[2], False)
    w.copy_(torch.tensor([0.2, 0.05]))
    assert w.data_ptr() == ptr
    loss2, grad2 = _lib_loss(dev, x, lab, w, True, True)
    ref2 = restate(xf, lab, d2g, d2p, 0.2, 0.05, True, True)
    assert abs(ref2[0] - ref[0]) > 1e-2 * abs(ref[0])
    _close_loss(loss2.item(), ref2[0])
    _close_grad(grad2, ref2[1], ref2[2], False)
    # a pair of floats is uploaded once per pair of values
    xd, ld = x.to(dev), lab.to(dev)
    ops.dist_loss(xd, ld, (0.25, 0.125))
    from cenet_amd.ops import dseb_loss as M
    n = len(M._DIST_WEIGHTS)
    buf = M._DIST_WEIGHTS[(str(xd.device), 0.25, 0.125)]
    ops.dist_loss(xd, ld, (0.25, 0.125))
    assert len(M._DIST_WEIGHTS) == n and M._DIST_WEIGHTS[(str(xd.device), 0.25, 0.125)] is buf
    for bad in (torch.tensor([0.7, 0.01], dtype=torch.float64).to(dev), torch.ones(3).to(dev), (1.0,)):
        with pytest.raises(ValueError, match="weights"):
            ops.dist_loss(xd, ld, bad)


def _counting(monkeypatch, owner, *names):
    """wraps owner.<name> for every name; -> the list the wrappers append their name to at each call"""
    calls = []
    for name in names:
        def wrapper(*a, _real=getattr(owner, name), _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(owner, name, wrapper)
    return calls


def test_without_the_hausdorff_term_no_prediction_map_is_built(dev, monkeypatch):
    shape = (3, 4, 9, 11)
    x, _, lab, _, _ = _case(shape, torch.float32)
    pred, gt = _counting(monkeypatch, kern, "dist_maps_logits"), _counting(monkeypatch, kern, "dist_maps_labels")
    _lib_loss(dev, x, lab, (1.0, 0.0), True, False)
    assert pred == [] and len(gt) == 1
    losses.SurfaceLoss(4)(x.to(dev), lab.to(dev))
    assert pred == [] and len(gt) == 2
    _lib_loss(dev, x, lab, (0.0, 1.0), False, True)
    assert len(pred) == 1 and len(gt) == 3
    losses.HausdorffDTLoss(4)(x.to(dev), lab.to(dev))
    assert len(pred) == 2 and len(gt) == 4


# ---- losses.py -------------------------------------------------------------------------------------------------------------------
def _args(loss_type, loss_weights, **kw):
    return argparse.Namespace(loss_type=loss_type, loss_weights=loss_weights, **kw)


def _crit_run(d, crit, x, lab):
    xd = x.to(d).clone().requires_grad_(True)  # (a copy on the checker too: x is shared between the tests)
    loss = crit.to(d)(xd, lab.to(d))
    loss.backward()
    return loss.detach(), xd.grad


@pytest.mark.parametrize("dtype", DTYPES)
def test_criterion_adds_the_surface_term_to_the_existing_path(dev, dtype):
    shape = (2, 4, 30, 70)
    x, xf, lab, d2g, d2p = _case(shape, dtype)
    loss, grad = _crit_run(dev, losses.Criterion(4, _args("dice,ce,surface", "0.5,0.5,0.1")), x, lab)
    base_loss, base_grad = _crit_run(dev, losses.Criterion(4, _args("dice,ce", "0.5,0.5")), x, lab)
    surf_loss, surf_grad = _crit_run(dev, losses.SurfaceLoss(4), x, lab)
    ref_loss = base_loss.item() + 0.1 * surf_loss.item()
    ref_grad = base_grad.double().cpu().numpy() + 0.1 * surf_grad.double().cpu().numpy()
    _close_loss(loss.item(), ref_loss)
    _close_grad(grad, ref_grad, _ref(shape, dtype, "surface")[2], dtype == torch.bfloat16)
    # SurfaceLoss itself is the restatement's surface term
    _close_loss(surf_loss.item(), _ref(shape, dtype, "surface")[0])
    _close_grad(surf_grad, _ref(shape, dtype, "surface")[1], _ref(shape, dtype, "surface")[2], dtype == torch.bfloat16)


def test_criterion_with_the_distance_terms_alone(dev, monkeypatch):
    shape = (3, 4, 9, 11)
    x, xf, lab, d2g, d2p = _case(shape, torch.float32)
    base = _counting(monkeypatch, ops, "dice_ce_loss", "seg_loss")
    crit = losses.Criterion(4, _args("surface,hausdorff", "0.7,0.01"))
    assert crit.dist_weights.tolist() == pytest.approx([0.7, 0.01]) and "dist_weights" in crit.state_dict()
    loss, grad = _crit_run(dev, crit, x, lab)
    assert crit.dist_weights.device.type == dev.type and base == []
    ref = _ref(shape, torch.float32, "both")
    _close_loss(loss.item(), ref[0])
    _close_grad(grad, ref[1], ref[2], False)
    # HausdorffDTLoss is the restatement's second term; repeated names add up
    hd_loss, hd_grad = _crit_run(dev, losses.HausdorffDTLoss(4), x, lab)
    ref = _ref(shape, torch.float32, "hausdorff")
    _close_loss(hd_loss.item(), ref[0])
    _close_grad(hd_grad, ref[1], ref[2], False)
    twice = losses.Criterion(4, _args("hausdorff,hausdorff", "0.25,0.75"))
    assert twice.dist_weights.tolist() == [0.0, 1.0] and twice.has_hausdorff and not twice.has_surface
    _close_loss(_crit_run(dev, twice, x, lab)[0].item(), ref[0])
    # new weights are written into the same buffer and read by the next call
    ptr = crit.dist_weights.data_ptr()
    crit.set_dist_weights(surface=0.2)
    crit.set_dist_weights(hausdorff=torch.tensor(0.05).to(dev))
    assert crit.dist_weights.data_ptr() == ptr and crit.dist_weights.tolist() == pytest.approx([0.2, 0.05])
    ref2 = restate(xf, lab, d2g, d2p, 0.2, 0.05, True, True)
    loss2, grad2 = _crit_run(dev, crit, x, lab)
    _close_loss(loss2.item(), ref2[0])
    _close_grad(grad2, ref2[1], ref2[2], False)


def test_criterion_without_the_names_launches_nothing_of_this(dev, monkeypatch):
    shape = (3, 4, 9, 11)
    x, _, lab, _, _ = _case(shape, torch.float32)
    base = _counting(monkeypatch, ops, "dice_ce_loss")
    dist = _counting(monkeypatch, kern, "dist_maps_labels", "dist_maps_logits", "dist_loss_fwd", "dist_loss_bwd")
    dist_op = _counting(monkeypatch, ops, "dist_loss")
    crit = losses.Criterion(4, _args("dice,ce", "0.5,0.5"))
    assert crit.dist_weights is None and "dist_weights" not in crit.state_dict()
    _crit_run(dev, crit, x, lab)
    assert base == ["dice_ce_loss"] and dist == [] and dist_op == []
    with pytest.raises(ValueError, match="surface"):
        crit.set_dist_weights(surface=1.0)


def test_refusals(dev):
    for names in ("dice,surface", "hausdorff", "ce,surface,hausdorff"):
        with pytest.raises(NotImplementedError, match="ignore_index"):
            losses.Criterion(4, _args(names, ",".join(["0.5"] * len(names.split(","))), ignore_index=255))
    with pytest.raises(NotImplementedError, match="focal"):
        losses.Criterion(4, _args("surface,focal", "0.5,0.5"))
    x, lab = torch.zeros(2, 4, 5, 6, device=dev), torch.zeros(2, 5, 6, device=dev)
    with pytest.raises(ValueError, match="neither"):
        ops.dist_loss(x, lab, (1.0, 1.0), surface=False, hausdorff=False)
    for bad_x, bad_lab in ((x, lab[:, :4]), (x, lab[:1]), (x[0], lab), (x, lab[0])):
        with pytest.raises(ValueError, match="expected|logits"):
            ops.dist_loss(bad_x, bad_lab, (1.0, 1.0))
    with pytest.raises(ValueError, match="classes|K"):
        ops.dist_loss(x[:, :1], lab, (1.0, 1.0))
    # the launch wrappers hold their tensors to the shape before the library is touched
    w = torch.ones(2, device=dev)
    d2 = torch.zeros(2, 3, 5, 6, dtype=torch.int32, device=dev)
    ws, out = torch.empty(kern.dist_loss_ws_floats(2, 4, 5, 6), device=dev), torch.full((1,), -3.5).to(dev)
    with pytest.raises(ValueError, match="sizes"):
        kern.dist_loss_fwd(x, lab, d2[:, :2], None, w, ws, out, 2, 4, 5, 6, True, False)
    with pytest.raises(ValueError, match="Hausdorff"):
        kern.dist_loss_fwd(x, lab, d2, None, w, ws, out, 2, 4, 5, 6, True, True)
    with pytest.raises(ValueError, match="alias"):
        kern.dist_loss_bwd(x, lab, d2, None, w, out, x, 2, 4, 5, 6, True, False)
    # a workspace one float short: the ABI's error, nothing is launched
    ws9 = torch.empty(kern.dist_loss_ws_floats(2, 9, 33, 33), device=dev)
    assert ws9.numel() == 2 * 2  # one row of two sums per workgroup of 2048 pixels
    with pytest.raises(RuntimeError, match="cenet_dist_loss_fwd_f32 failed with error code 1"):
        kern.dist_loss_fwd(torch.zeros(2, 9, 33, 33, device=dev), torch.zeros(2, 33, 33, device=dev),
                           torch.zeros(2, 8, 33, 33, dtype=torch.int32, device=dev), None, w, ws9[:-1], out, 2, 9, 33, 33, True, False)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert out.item() == -3.5


def test_a_weight_schedule_needs_a_distance_term():
    from cenet_amd import train
    with pytest.raises(ValueError, match="dist_weight_schedule"):
        train.train_acdc(torch.nn.Linear(1, 1), [], device="cpu", dist_weight_schedule=lambda e: (1.0, 1.0))
    with pytest.raises(NotImplementedError, match="ignore_index"):
        train.train_acdc(torch.nn.Linear(1, 1), [], device="cpu", loss_type="dice,surface", ignore_index=255)


def test_host_tensors_are_refused_off_the_checker():
    assert not _lib.is_hostsim()
    x, lab = torch.zeros(2, 4, 3, 4), torch.zeros(2, 3, 4)
    crit = losses.Criterion(4, _args("dice,ce,surface", "0.5,0.5,0.1"))
    for call in (lambda: ops.dist_loss(x, lab, (1.0, 1.0)), lambda: losses.SurfaceLoss(4)(x, lab),
                 lambda: losses.HausdorffDTLoss(4)(x, lab)):
        with pytest.raises(ValueError, match="MI355X"):
            call()
    with pytest.raises((ValueError, RuntimeError), match="MI355X"):
        crit(x, lab)
