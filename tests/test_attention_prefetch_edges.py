"""The register prefetch of the pair-attention kernels (attn_diff.hip) at the edges of its address clamp.  A fetch loads 16 bytes
per chunk slot unconditionally, from the tensor's last row when the tile row lies beyond the tensor, and the fill (zero, the
1e30 of the statistics rows, the hd-4 half swap) is chosen on the landed registers in front of the LDS write.  So the cases are
the row counts at which the clamp and the fill take over: N < 32 (only the prologue stages, every row past N is clamped), an
exact tile (the prefetch of the tile after the last one is clamped whole), a ragged last tile, and a last workgroup whose upper
waves lie wholly past N — for every head dimension the entry point serves (hd 4 / 8 / 16 on the HDP = 16 instances, 32, 40 on
HDP = 48, 64) and for the single-softmax form at C = 64 / 128 (which takes the pair kernels from N = 256 on: 257 and 288).

q, k, v and dU are each the exact tail of their buffer: a load past the tensor's last row would leave the allocation.  Results
are held to the fp64 reference with the per-element bounds of test_attention_bounds.py (c = 4, u = 2^-8) on O, dQ, dK, dV and the
LSE, and a second run must reproduce the first bit for bit (no atomics, the staged bytes do not depend on timing)."""
import pytest
import torch

import attn_ref as R
from backend import use_hip
from cenet_amd import _lib, ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, H = 2, 2
REGIMES = ("randn", "negative")


@pytest.fixture
def hip():
    d = use_hip()
    yield d
    _lib._LIB = None
    _lib._HOSTSIM = False


def tail(t, pad=1024):
    """a copy of t that ends exactly where its buffer ends (pad elements in front of it: the start stays 16-byte aligned)"""
    buf = torch.empty(pad + t.numel(), dtype=t.dtype, device=t.device)
    out = buf[pad:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() + out.numel() * out.element_size() == buf.data_ptr() + buf.numel() * buf.element_size()
    assert out.is_contiguous() and out.data_ptr() % 16 == 0
    return out


def run_pair(q, k, v, dO):
    """ops.diff_attention_heads on canonical q, k [B, 2H, N, hd], v [B, H, N, 2hd]; every tensor the kernels read is a tail"""
    Bq, Hq, N, hd = q.shape
    qp, kp = (tail(t.transpose(1, 2).reshape(Bq, N, Hq * hd)).requires_grad_(True) for t in (q, k))
    vp = tail(v.transpose(1, 2).reshape(Bq, N, H * 2 * hd)).requires_grad_(True)
    U = ops.diff_attention_heads(qp, kp, vp, H)
    assert getattr(U.grad_fn, "pairs", False), "the case did not run on the pair kernels"
    lse = U.grad_fn.saved_tensors[4]
    U.backward(tail(dO.contiguous()))
    return {"O": U, "dQ": qp.grad.view(Bq, N, Hq, hd).transpose(1, 2), "dK": kp.grad.view(Bq, N, Hq, hd).transpose(1, 2),
            "dV": vp.grad.view(Bq, N, H, 2 * hd).transpose(1, 2)}, lse


def run_single(q, k, v, dO):
    """ops.nonlocal_attention on canonical [B, 1, N, C] (theta | phi | g channel-major [B, C, N])"""
    ins = [tail(t[:, 0].transpose(1, 2)).requires_grad_(True) for t in (q, k, v)]
    y = ops.nonlocal_attention(*ins)
    assert y.grad_fn.tok64, "the case did not run on the single-softmax pair kernels"
    lse = y.grad_fn.saved_tensors[4]
    y.backward(tail(dO[:, 0].transpose(1, 2)))
    canon = lambda t: t.transpose(1, 2)[:, None]  # noqa: E731
    return {"O": canon(y), "dQ": canon(ins[0].grad), "dK": canon(ins[1].grad), "dV": canon(ins[2].grad)}, lse


def check(run, regime, Hq, N, hd, Dv, group, dev):
    scale = hd ** -0.5
    q, k, v, dO = (t.to(BF).to(dev) for t in R.make_inputs(regime, B, Hq, N, N, hd, Dv, scale, group, seed=N + hd))
    ref = R.reference(q, k, v, scale, dO, group)
    got, lse = run(q, k, v, dO)
    what = f"prefetch edges B{B} Hq{Hq} N{N} hd{hd} {regime}"
    ratios = R.check_all(got, ref, R.C_BF16, R.U_BF16, what)
    ratios["lse"] = R.assert_within(lse, ref.lse, ref.M_lse, R.C_BF16, R.U_BF16, what=f"{what} lse")
    print(what, {n: round(r, 3) for n, r in ratios.items()})
    again, lse2 = run(q, k, v, dO)
    for n in got:
        assert torch.equal(got[n], again[n]), f"{what}: {n} differs between two runs"
    assert torch.equal(lse, lse2), f"{what}: lse differs between two runs"


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 95])
@pytest.mark.parametrize("hd", [4, 8, 16, 32, 40, 64])
def test_pair_prefetch_edges(hip, hd, N, regime):
    check(run_pair, regime, 2 * H, N, hd, 2 * hd, 2, hip)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("N", [257, 288])
@pytest.mark.parametrize("Cn", [64, 128])
def test_single_softmax_prefetch_edges(hip, Cn, N, regime):
    check(run_single, regime, 1, N, Cn, Cn, 1, hip)
