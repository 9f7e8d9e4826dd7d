"""Test helper: the Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018, Alg. 1) restated in float64 torch from the definition
in include/cenet_hip.h.  The order of a segment comes from torch.sort(-e, stable=True), the increments of the Jaccard loss from
the integer counts in their closed forms, the gradient from autograd with the order held constant."""
import torch


def increments(g_sorted):
    """g_sorted: bool [n] along the sorted order -> float64 [n], J_i - J_{i-1} from the integers"""
    g = g_sorted.long()
    G = int(g.sum())
    F = torch.cumsum(g, 0)
    Z = torch.cumsum(1 - g, 0)
    I, U = (G - F).double(), (G + Z).double()
    inc0 = torch.where(U == 1, torch.ones_like(U), I / (U * (U - 1).clamp(min=1)))
    return torch.where(g_sorted, 1.0 / U, inc0)


def segment_loss(e, g, order_key=None):
    """e float64 [n] (differentiable), g bool [n]; order_key: the values whose stable descending order is used (default e)"""
    key = e.detach() if order_key is None else order_key
    perm = torch.sort(-key, stable=True).indices
    return (e[perm] * increments(g[perm])).sum()


def lovasz_ref(inputs_f32, target, *, per_image=False, classes="present", ignore_index=None, from_probs=False, gout=1.0,
               order="f64"):
    """inputs_f32: fp32 [B,K,H,W] (what the library's input is worth in fp32), target [B,H,W] float -> (loss, dloss/dinputs * gout
    as float64 numpy).  Pixels whose label is ignore_index are removed.  order: "f64" — errors of the float64 probabilities decide
    the order; "f32" — |g - p| computed in fp32 decides it (from_probs: the same single fp32 operation the library does);
    "f32softmax" — torch's fp32 softmax, then the fp32 error."""
    x = inputs_f32.double().requires_grad_(True)
    B, K = x.shape[:2]
    p = x if from_probs else torch.softmax(x, dim=1)
    if order == "f64":
        p32 = None
    elif order == "f32":
        assert from_probs
        p32 = inputs_f32.float()
    else:
        p32 = inputs_f32.float() if from_probs else torch.softmax(inputs_f32.float(), dim=1)
    images = [slice(b, b + 1) for b in range(B)] if per_image else [slice(0, B)]
    total = x.sum() * 0.0
    for sl in images:
        lab = target[sl].reshape(-1)
        valid = torch.ones_like(lab, dtype=torch.bool) if ignore_index is None else lab != ignore_index
        losses = []
        for c in range(K):
            g = (lab == c)[valid]
            if classes == "present" and not bool(g.any()):
                continue
            pc = p[sl, c].reshape(-1)[valid]
            e = (g.double() - pc).abs()
            key = None
            if p32 is not None:
                key = (g.float() - p32[sl, c].reshape(-1)[valid]).abs().double()
            losses.append(segment_loss(e, g, key))
        if losses:
            total = total + sum(losses) / len(losses)
    loss = total / len(images)
    (grad,) = torch.autograd.grad(loss * gout, x, allow_unused=True)
    grad = torch.zeros_like(x) if grad is None else grad
    return float(loss.detach()), grad.numpy()
