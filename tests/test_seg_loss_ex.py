"""The fused loss with options (csrc/seg_loss_ex.hip through ops.seg_loss, losses.DiceLoss / JaccardLoss / Criterion): class
weights for the Dice and cross-entropy terms, ignore_index, the Jaccard term and DiceLoss(softmax=False).

The judge is `restate`: the formulas in torch float64 with gradients by autograd.  With M = [label != ignore_index],
t_c = [label == c] M and sums over the whole batch, I_c = sum M p_c t_c, Z_c = sum M p_c^2, Y_c = sum t_c, S_c = sum M p_c:
  Dice    = 1/K sum_c wd_c (1 - (2 I_c + 1e-5) / (Z_c + Y_c + 1e-5))
  CE      = sum_pix wc_t (-log p_t) / sum_pix wc_t over the pixels with M = 1   (torch's CrossEntropyLoss(weight, ignore_index))
  Jaccard = 1/K sum_c (1 - (I_c + s) / (S_c + Y_c - I_c + s))
  BoundaryDoU as utils/core.py:83-131.
Tolerances are those of tests/test_losses.py (|loss - ref| < 1e-5, gradient rtol 1e-3 / atol 1e-8) and, for bf16 logits against
fp32, of tests/test_bf16_storage.py::test_seg_loss (loss 1e-5 max(1, |loss|), gradient relative L2 < 1e-2)."""
import argparse
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from backend import dev, use_hip  # noqa: F401
from cenet_amd import kern, losses, ops, train

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF = torch.bfloat16
SHAPES = [(2, 12, 12), (3, 37, 61)]  # fewer pixels than one workgroup; 2257 pixels: several workgroups per image, ragged last one
KS = [2, 4, 5, 9, 10, 16]            # each compile-time class bound (4 / 9 / 16) exactly and one predicated case below each


# ---- the float64 restatement ----------------------------------------------------------------------------------------------------
def restate(x, labels, *, w_dice=0., w_ce=0., w_bd=0., w_jac=0., wd=None, wc=None, ignore_index=None, smooth=1.0,
            from_probs=False):
    """x [B,K,H,W] float64 (requires grad), labels [B,H,W] -> loss; a term whose weight is 0 is left out"""
    K = x.shape[1]
    p = x if from_probs else torch.softmax(x, dim=1)
    lab = labels.long()
    M = torch.ones_like(lab, dtype=torch.float64) if ignore_index is None else (lab != ignore_index).double()
    wd = torch.ones(K, dtype=torch.float64) if wd is None else torch.as_tensor(wd, dtype=torch.float64)
    wc = torch.ones(K, dtype=torch.float64) if wc is None else torch.as_tensor(wc, dtype=torch.float64)
    t = torch.stack([(lab == c).double() * M for c in range(K)], dim=1)
    Mp = M[:, None] * p
    I, Z, Y, S = (Mp * t).sum((0, 2, 3)), (Mp * p).sum((0, 2, 3)), t.sum((0, 2, 3)), Mp.sum((0, 2, 3))
    loss = x.new_zeros(())
    if w_dice:
        loss = loss + w_dice * (wd * (1 - (2 * I + 1e-5) / (Z + Y + 1e-5))).sum() / K
    if w_ce:
        safe = lab.clamp(0, K - 1)
        w_pix = wc[safe] * M
        nll = -torch.log(p).gather(1, safe[:, None])[:, 0]
        loss = loss + w_ce * (w_pix * nll).sum() / w_pix.sum()
    if w_bd:
        kernel = torch.tensor([[0., 1, 0], [1, 1, 1], [0, 1, 0]], dtype=torch.float64)[None, None]
        nb = F.conv2d(t.reshape(-1, 1, *t.shape[2:]), kernel, padding=1).reshape(t.shape) * t
        C = ((nb != 0) & (nb != 5)).double().sum((0, 2, 3))
        alpha = torch.clamp(2 * (1 - (C + 1e-5) / (Y + 1e-5)) - 1, max=0.8)
        loss = loss + w_bd * ((Z + Y - 2 * I + 1e-5) / (Z + Y - (1 + alpha) * I + 1e-5)).sum() / K
    if w_jac:
        loss = loss + w_jac * (1 - (I + smooth) / (S + Y - I + smooth)).sum() / K
    return loss


def restate_grad(x32, labels, **kw):
    x = x32.double().requires_grad_(True)
    loss = restate(x, labels, **kw)
    loss.backward()
    return loss.item(), x.grad.numpy()


# ---- inputs and option sets -----------------------------------------------------------------------------------------------------
def blocky(B, K, H, W, seed, absent=None):
    """logits and blocky labels with one class absent (K-1 unless told otherwise)"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, K, H, W, generator=g) * 2
    low = torch.rand(B, 1, 5, 7, generator=g)
    labels = torch.floor(F.interpolate(low, size=(H, W), mode="nearest") * (K - 1)).clamp_(0, max(K - 2, 0))[:, 0]
    if absent is not None and absent != K - 1:
        labels = labels + (labels >= absent).float()
    return logits, labels.contiguous(), g


def weights(K, g):
    return (0.2 + 2.8 * torch.rand(2, K, generator=g)).tolist()  # both vectors in [0.2, 3]


def void(labels, value):
    """the first 9 rows of image 0 and the whole last image carry `value`"""
    labels = labels.clone()
    labels[0, :9] = value
    labels[-1] = value
    return labels


def option_set(name, B, K, H, W, seed=0):
    """-> (input [B,K,H,W] fp32, labels, keyword arguments of `restate`)"""
    # (K = 2 leaves one class present: were it class 0, set (c) would ignore every pixel and its CE would be NaN; there class 0
    # is the absent one and ignore_index=0 masks nothing)
    logits, labels, g = blocky(B, K, H, W, seed + 1000 * K + H, absent=0 if (name == "c" and K == 2) else None)
    wd, wc = weights(K, g)
    if name == "a":
        return logits, void(labels, 255), dict(w_dice=0.4, w_ce=0.3, w_jac=0.3, wd=wd, wc=wc, ignore_index=255)
    if name == "b":
        return logits, void(labels, -100), dict(w_dice=0.4, w_ce=0.3, w_jac=0.3, wd=wd, wc=wc, ignore_index=-100)
    if name == "c":  # a real class is the ignored label
        return logits, labels, dict(w_dice=0.4, w_ce=0.3, w_jac=0.3, wd=wd, wc=wc, ignore_index=0)
    if name == "d":
        return logits, labels, dict(w_dice=0.3, w_ce=0.2, w_bd=0.3, w_jac=0.2, wd=wd, wc=wc)
    if name == "e":
        return torch.softmax(logits, dim=1), labels, dict(w_dice=1.0, wd=wd, from_probs=True)
    raise KeyError(name)


def call(dev, x, labels, *, w_dice=0., w_ce=0., w_bd=0., w_jac=0., wd=None, wc=None, ignore_index=None, smooth=1.0,
         from_probs=False):
    """ops.seg_loss forward + backward -> (loss tensor, gradient tensor), both on the device"""
    x = x.detach().clone().to(dev).requires_grad_(True)  # (a copy: on the host checker .to(dev) is the cached input itself)
    loss = ops.seg_loss(x, labels.to(dev), w_dice=w_dice, w_ce=w_ce, w_boundary=w_bd, w_jaccard=w_jac, dice_class_weights=wd,
                        ce_class_weights=wc, ignore_index=ignore_index, jaccard_smooth=smooth, from_probs=from_probs)
    loss.backward()
    return loss.detach(), x.grad


_REF = {}  # (option set, shape, K) -> (input, labels, options, reference loss, reference gradient), computed once


def case(name, shape, K):
    key = (name, shape, K)
    if key not in _REF:
        B, H, W = shape
        x, labels, kw = option_set(name, B, K, H, W)
        _REF[key] = (x, labels, kw) + restate_grad(x, labels, **kw)
    return _REF[key]


# ---- 1. the float64 restatement over the grid -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_fp64_restatement(dev, shape, K, name):
    x, labels, kw, ref_loss, ref_grad = case(name, shape, K)
    loss, grad = call(dev, x, labels, **kw)
    grad = grad.cpu().numpy()
    print(f"loss {loss.item():.9f} ref {ref_loss:.9f} max|dgrad| {np.abs(grad - ref_grad).max():.3e}")
    assert abs(loss.item() - ref_loss) < 1e-5
    np.testing.assert_allclose(grad, ref_grad, rtol=1e-3, atol=1e-8)
    if kw.get("ignore_index") is not None:
        ignored = (labels == kw["ignore_index"])[:, None].expand_as(x).numpy()
        assert ignored.any() or (name == "c" and K == 2)
        assert (grad[ignored] == 0.0).all()  # exactly zero in every class


@pytest.mark.parametrize("K", [4, 9])
def test_bf16_logits_against_fp32(dev, K):
    x, labels, kw, _, _ = case("a", (3, 37, 61), K)
    x = x.to(BF).float()  # the same inputs for both storage types, fp32 arithmetic in both
    l32, g32 = call(dev, x, labels, **kw)
    l16, g16 = call(dev, x.to(BF), labels, **kw)
    assert g16.dtype == BF
    assert abs(l32.item() - l16.item()) < 1e-5 * max(1.0, abs(l32.item()))
    assert ((g16.float() - g32).norm() / g32.norm()).item() < 1e-2


# ---- 2. goldens: the reference's own DiceLoss / JaccardLoss ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dice_w", "dice_w_probs", "jac255", "jac0"])
@pytest.mark.parametrize("K", [4, 9])
def test_golden(dev, K, name):
    z = np.load(os.path.join(GOLDEN, "loss_ex.npz"))
    logits = torch.from_numpy(z[f"K{K}.logits"])
    labels = torch.from_numpy(z[f"K{K}.labels"].astype(np.float32)).to(dev)
    weight = z[f"K{K}.weight"].tolist()
    if name == "dice_w":
        x = logits.clone().to(dev).requires_grad_(True)
        loss = losses.DiceLoss(K)(x, labels, weight=weight, softmax=True)
    elif name == "dice_w_probs":
        x = torch.softmax(logits.double(), dim=1).float().to(dev).requires_grad_(True)
        loss = losses.DiceLoss(K)(x, labels, weight=weight, softmax=False)
    elif name == "jac255":
        x = logits.clone().to(dev).requires_grad_(True)
        loss = losses.JaccardLoss(255, 1.0)(x, torch.from_numpy(z[f"K{K}.labels255"].astype(np.float32)).to(dev))
    else:
        x = logits.clone().to(dev).requires_grad_(True)
        loss = losses.JaccardLoss(0, 0.5)(x, labels)
    loss.backward()
    assert abs(loss.item() - float(z[f"K{K}.{name}.loss"])) < 1e-5
    np.testing.assert_allclose(x.grad.cpu().numpy(), z[f"K{K}.{name}.grad"], rtol=1e-3, atol=1e-8)


def test_dice_weight_as_device_tensor(dev):
    """DiceLoss.forward(weight=<device tensor>) reads the tensor; new values in it are seen by the next call"""
    x, labels, kw, _, _ = case("e", (2, 12, 12), 5)
    w = torch.tensor(kw["wd"], dtype=torch.float32).to(dev)
    for scale in (1.0, 2.0):
        w.copy_(torch.tensor(kw["wd"]) * scale)
        xd = x.clone().to(dev).requires_grad_(True)
        loss = losses.DiceLoss(5)(xd, labels.to(dev), weight=w, softmax=False)
        ref = restate(x.double(), labels, w_dice=1.0, wd=[v * scale for v in kw["wd"]], from_probs=True).item()
        assert abs(loss.item() - ref) < 1e-5


# ---- 3. neutral options equal the existing path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_neutral_options_equal_dice_ce_loss(dev, bf16):
    K = 5
    logits, labels, _ = blocky(3, K, 37, 61, seed=3)
    if bf16:
        logits = logits.to(BF)
    labels = labels.to(dev)
    xo = logits.clone().to(dev).requires_grad_(True)
    old = ops.dice_ce_loss(xo, labels, 0.3, 0.2, 0.5)
    old.backward()
    xn = logits.clone().to(dev).requires_grad_(True)
    new = ops.seg_loss(xn, labels, w_dice=0.3, w_ce=0.2, w_boundary=0.5, w_jaccard=0.0, dice_class_weights=[1.0] * K,
                       ce_class_weights=[1.0] * K)
    new.backward()
    assert new.dtype == old.dtype and xn.grad.dtype == xo.grad.dtype
    if bf16:
        assert abs(new.item() - old.item()) < 1e-5 * max(1.0, abs(old.item()))
        assert ((xn.grad.float() - xo.grad.float()).norm() / xo.grad.float().norm()).item() < 1e-2
    else:
        assert abs(new.item() - old.item()) < 1e-5
        np.testing.assert_allclose(xn.grad.cpu().numpy(), xo.grad.cpu().numpy(), rtol=1e-3, atol=1e-8)


# ---- 4. bit reproducibility -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 9])
def test_bitwise_reproducible(dev, K):
    """no float atomics: two runs on the same tensors give the same bits (the assertion that matters on the hip backend)"""
    x, labels, kw, _, _ = case("a", (3, 37, 61), K)
    (l1, g1), (l2, g2) = call(dev, x, labels, **kw), call(dev, x, labels, **kw)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    assert bool(torch.isfinite(g1).all()) and g1.abs().max().item() > 0


# ---- 5. the old path is untouched ---------------------------------------------------------------------------------------------------
def _ns(**kw):
    return argparse.Namespace(loss_weights=",".join(["0.5"] * len(kw["loss_type"].split(","))), **kw)


def test_plain_criterion_keeps_the_old_kernels(dev, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("seg_loss_ex reached")
    monkeypatch.setattr(kern, "seg_loss_ex_fwd", boom)
    K = 4
    logits, labels, _ = blocky(2, K, 12, 12, seed=7)
    for args in (_ns(loss_type="dice,ce"), _ns(loss_type="boundary"), train.criterion_args()):
        crit = losses.Criterion(K, args).to(dev)
        assert not crit.extended and not list(crit.buffers())
        x = logits.clone().to(dev).requires_grad_(True)
        loss = crit(x, labels.to(dev))
        loss.backward()
        assert np.isfinite(loss.item()) and x.grad.abs().max().item() > 0
    x = logits.clone().to(dev).requires_grad_(True)
    assert np.isfinite(losses.DiceLoss(K)(x, labels.to(dev), softmax=True).item())
    for extra in (dict(loss_type="dice,jaccard"), dict(loss_type="dice,ce", ignore_index=255), dict(loss_type="ce", jaccard_smooth=0.5),
                  dict(loss_type="dice,ce", ce_class_weights="1,2,3,4"), dict(loss_type="dice", dice_class_weights=[1, 2, 3, 4])):
        crit = losses.Criterion(K, _ns(**extra)).to(dev)
        assert crit.extended
        with pytest.raises(AssertionError, match="seg_loss_ex reached"):
            crit(logits.to(dev), labels.to(dev))
    assert train.criterion_args("dice,ce", "0.5,0.5", ignore_index=255).ignore_index == 255


def test_criterion_equals_the_restatement(dev):
    """comma strings for the weights, `jaccard` in loss_type, weights as a buffer that follows .to()"""
    K = 4
    x, labels, kw, ref_loss, ref_grad = case("a", (3, 37, 61), K)
    args = argparse.Namespace(loss_type="dice,ce,jaccard", loss_weights="0.4,0.3,0.3", ignore_index=255,
                              dice_class_weights=",".join(repr(v) for v in kw["wd"]), ce_class_weights=kw["wc"])
    crit = losses.Criterion(K, args)
    assert crit.class_weights.shape == (2 * K,) and crit.class_weights.device.type == "cpu"
    crit = crit.to(dev)
    assert crit.class_weights.device.type == torch.device(dev).type
    xd = x.clone().to(dev).requires_grad_(True)
    loss = crit(xd, labels.to(dev))
    loss.backward()
    assert abs(loss.item() - ref_loss) < 1e-5
    np.testing.assert_allclose(xd.grad.cpu().numpy(), ref_grad, rtol=1e-3, atol=1e-8)
    with torch.no_grad():  # new values in the buffer take effect at the next call
        crit.class_weights.fill_(1.0)
    ref1 = restate(x.double(), labels, w_dice=0.4, w_ce=0.3, w_jac=0.3, ignore_index=255).item()
    assert abs(crit(x.to(dev), labels.to(dev)).item() - ref1) < 1e-5 and abs(ref1 - ref_loss) > 1e-3


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    K = 4
    logits, labels, _ = blocky(2, K, 12, 12, seed=9)
    x, lab = logits.to(dev), labels.to(dev)
    with pytest.raises(NotImplementedError):
        ops.seg_loss(x, lab, w_boundary=1.0, ignore_index=255)
    with pytest.raises(NotImplementedError):
        losses.Criterion(K, _ns(loss_type="dice,boundary", ignore_index=255))
    for term in ("w_ce", "w_boundary", "w_jaccard"):
        with pytest.raises(ValueError):
            ops.seg_loss(x, lab, w_dice=1.0, from_probs=True, **{term: 0.5})
    with pytest.raises(ValueError):
        ops.seg_loss(x, lab, w_dice=1.0, dice_class_weights=[1.0] * (K + 1))
    with pytest.raises(ValueError):
        ops.seg_loss(x, lab, w_ce=1.0, ce_class_weights=torch.ones(K - 1).to(dev))
    with pytest.raises(ValueError):
        losses.Criterion(K, _ns(loss_type="dice,ce", ce_class_weights="1,2,3"))
    with pytest.raises(NotImplementedError):
        losses.Criterion(K, _ns(loss_type="dice,focal"))
    # a workspace one float short of what the shape needs: the ABI's error, nothing is launched
    n = kern.seg_loss_ex_ws_floats(2, K, 12, 12)
    loss = torch.full((1,), 7.0).to(dev)
    cfg = (1.0, 0.0, 0.0, 0.0, 1.0, None, False)
    with pytest.raises(RuntimeError, match="cenet_seg_loss_ex_fwd_f32 failed with error code 1"):
        kern.seg_loss_ex_fwd(x, lab, None, torch.zeros(n - 1).to(dev), loss, 2, K, 12, 12, *cfg)
    assert loss.item() == 7.0
    kern.seg_loss_ex_fwd(x, lab, None, torch.zeros(n).to(dev), loss, 2, K, 12, 12, *cfg)
    assert 0.0 < loss.item() < 1.0


# ---- 7. a batch whose every pixel is ignored ------------------------------------------------------------------------------------------
def test_all_ignored_batch(dev):
    K = 4
    logits, labels, _ = blocky(2, K, 12, 12, seed=11)
    labels = torch.full_like(labels, 255.0)
    ce, _ = call(dev, logits, labels, w_ce=1.0, ignore_index=255)
    assert torch.isnan(ce).item()
    assert torch.isnan(F.cross_entropy(logits, labels.long(), ignore_index=255)).item()  # as torch's
    dice, grad = call(dev, logits, labels, w_dice=1.0, ignore_index=255)
    ref = restate(logits.double(), labels, w_dice=1.0, ignore_index=255).item()
    assert np.isfinite(dice.item()) and abs(dice.item() - ref) < 1e-5
    assert (grad == 0).all().item()


# ---- 8. graph capture (GPU only) ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_follows_logits_labels_and_weights():
    d = use_hip()
    K, shape = 4, (3, 37, 61)
    x0, lab0, kw0, _, _ = case("a", shape, K)
    x1, lab1, kw1 = option_set("a", *shape[:1], K, *shape[1:], seed=77)
    lab1 = lab1.roll(5, dims=1)  # other pixels ignored than at capture
    opts = dict(w_dice=0.4, w_ce=0.3, w_jaccard=0.3, ignore_index=255)
    sx = x0.to(d).requires_grad_(True)
    slab = lab0.to(d)
    cw = torch.tensor(kw0["wd"] + kw0["wc"], dtype=torch.float32, device=d)

    def step():
        loss = ops.seg_loss(sx, slab, dice_class_weights=cw[:K], ce_class_weights=cw[K:], **opts)
        return loss, torch.autograd.grad(loss, sx)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # eager warm-up on one stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl, gg = step()
    for x, lab, kw in ((x1, lab1, kw1), (x0, lab0, kw0)):
        with torch.no_grad():
            sx.copy_(x.to(d))
            slab.copy_(lab.to(d))
            cw.copy_(torch.tensor(kw["wd"] + kw["wc"]))
        graph.replay()
        torch.cuda.synchronize()
        el, eg = call(d, x, lab, w_dice=0.4, w_ce=0.3, w_jac=0.3, wd=kw["wd"], wc=kw["wc"], ignore_index=255)
        assert torch.equal(gl, el) and torch.equal(gg, eg)
        ref_loss, _ = restate_grad(x, lab, **kw)
        assert abs(gl.item() - ref_loss) < 1e-5
    assert kw0["wd"] != kw1["wd"]


# ---- 9. the training loop (GPU only) --------------------------------------------------------------------------------------------------
class _Toy(torch.utils.data.Dataset):
    """tests/test_train_loop.py's in-memory slices, with a band and a corner of every label set to 255"""

    def __init__(self, n, seed):
        from oracle import cenet_oracle as O
        self.x, self.lab = O.synthetic_batch(n, 1, 4, seed=seed)
        self.lab = self.lab.clone()
        self.lab[:, 100:117] = 255
        self.lab[:, :40, :33] = 255

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return {"image": self.x[i], "label": self.lab[i].long(), "case_name": f"case{i}"}


@pytest.mark.gpu
def test_training_loop_replayed_equals_eager():
    import copy

    from cenet_amd.networks import CENet
    d = use_hip()
    loader = torch.utils.data.DataLoader(_Toy(6, seed=21), batch_size=2, shuffle=False)
    torch.manual_seed(77)
    ref_net = CENet(input_channels=1, num_classes=4, scale_factors=[1.0, 0.5], diffatt_num_heads=[4, 4, 4], out_up_block="upcn")
    ref_net.backbone.reset_drop_path(0.0)
    ref_net = ref_net.to(d)
    runs = []
    for graph in (False, True):
        h = train.train_acdc(copy.deepcopy(ref_net), loader, max_epochs=1, base_lr=0.01, device=d, graph=graph, log_every=1,
                             log=lambda s: None, loss_type="dice,ce,jaccard", loss_weights="0.4,0.3,0.3",
                             dice_class_weights=[0.5, 1.0, 2.0, 1.5], ce_class_weights="0.3,1.0,2.5,1.2", ignore_index=255)
        runs.append(np.array([v for _, v in h["loss"]]))
    le, lg = runs
    assert len(le) == len(lg) == 3 and np.isfinite(le).all()
    assert np.abs(le - lg).max() < 2e-4, (le, lg)
