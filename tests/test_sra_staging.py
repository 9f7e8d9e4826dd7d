"""The four spatial-reduction attention kernels (attn_diff.hip: sra_fwd_kernel, sra_bwd_kernel<1, true, true>, <4, true, false>,
<1, false, true>) at the shapes where their fetches can go wrong, held to the float64 reference of tests/attn_ref.py with the
bf16 bounds of test_attention_bounds.py (check_path, c = 4, u = 2^-8: no tolerance of this file's own).

What the shapes are for: the kernels load the K / V chunks of a (batch, head) and the q / dO / o rows of a 32-query tile
unconditionally from clamped addresses (a row beyond the tensor reads the tensor's last row) and select the fill on the landed
registers; a tile's rows are fetched one trip ahead, on every trip.  So: fewer rows than one tile (Nq 1, 31; Nk 1, 31), exactly one
(32), one more (33), a ragged last tile, every wave busy (128), one query past a workgroup (129: the query-sliced path with a
second workgroup that holds one row), several workgroups (300); on the GPU two tiles per wave (the prefetch crosses a trip that
runs, and one that leaves the loop at once) and the 65 .. 256-key pair of launches.

The path a case takes is asserted with the library's own predicates.  On the GPU every case also runs on q, kv, o and dO that
are the exact tails of their allocations, and the direct path twice: bit-equal."""
import pytest
import torch

import attn_ref as R
from backend import dev, use_hip  # noqa: F401
from cenet_amd import kern, ops
from test_attention_bounds import check_path

BF = torch.bfloat16
REGIMES = ("randn", "staircase")
NQ = (1, 31, 32, 33, 97, 128, 129, 300)
NK = (1, 31, 32, 33, 49, 64)
# (B, H, Nq, Nk, path, more than one tile per wave); path: "direct" / "sliced" (Nk <= 64), "blocks" (65 .. 256 keys)
SMALL = [(2, 2, nq, nk, "direct" if nq <= 128 else "sliced", False) for nq in NQ for nk in NK]
GPU_ONLY = [(25, 4, 400, 49, "sliced", True), (33, 4, 200, 49, "direct", True)] + \
    [(1, 1, nq, nk, "blocks", False) for nq in (33, 300) for nk in (65, 150, 256)]


def _id(c):
    return f"B{c[0]}H{c[1]}-{c[2]}x{c[3]}-{c[4]}"


def _params(cases):
    return [pytest.param(c, r, id=f"{_id(c)}-{r}") for c in cases for r in REGIMES]


def _assert_path(case):
    B, H, Nq, Nk, path, multi = case
    if path == "blocks":
        assert kern.sra_attn_bwd_blocks_supported(64, Nk) and not kern.sra_attn_bwd_supported(64, Nk)
        return
    assert kern.sra_attn_bwd_supported(64, Nk)
    assert kern.sra_attn_bwd_direct_supported(B, H, Nq, Nk) == (path == "direct")
    assert (kern.sra_attn_bwd_tiles(B, H, Nq) > 1) == multi


@pytest.mark.parametrize("case,regime", _params(SMALL))
def test_small_shapes_within_bound(dev, case, regime):
    B, H, Nq, Nk = case[:4]
    _assert_path(case)
    check_path("sra", regime, B, H, Nq, Nk, 64, BF, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", _params(GPU_ONLY))
def test_multi_tile_and_key_block_shapes_within_bound(case, regime):
    device = use_hip()
    B, H, Nq, Nk = case[:4]
    _assert_path(case)
    check_path("sra", regime, B, H, Nq, Nk, 64, BF, device)


def _tail(t):
    """a copy of t whose last byte is the last byte of its allocation (whole 512-byte units, as the caching allocator hands out)"""
    n = t.numel() * t.element_size()
    total = -(-n // 512) * 512 + 512
    buf = torch.empty(total, dtype=torch.uint8, device=t.device)
    v = buf[total - n:].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() + n == buf.data_ptr() + total and v.data_ptr() % 16 == 0
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", _params(SMALL + GPU_ONLY))
def test_tail_buffers_and_direct_path_bit_equal(case, regime):
    device = use_hip()
    B, H, Nq, Nk, path, _ = case
    _assert_path(case)
    hd, Cn, scale = 64, 64 * H, 64 ** -0.5
    q, k, v, dO = (t.to(BF).to(device) for t in R.make_inputs(regime, B, H, Nq, Nk, hd, hd, scale, 1, 0))
    ref = R.reference(q, k, v, scale, dO, 1)
    qp = _tail(q.transpose(1, 2).reshape(B, Nq, Cn))
    kvp = _tail(torch.cat([k.transpose(1, 2).reshape(B, Nk, Cn), v.transpose(1, 2).reshape(B, Nk, Cn)], -1))
    gp = _tail(dO.transpose(1, 2).reshape(B, Nq, Cn))
    if path == "blocks":  # the forward of these problems is the tiled kernel's
        out = ops.sr_attention(qp.clone().requires_grad_(True), kvp, H)
        o, lse = _tail(out.detach()), out.grad_fn.saved_tensors[3]
    else:
        o, lse = _tail(torch.empty_like(qp)), torch.empty((B, H, Nq), dtype=torch.float32, device=device)
        kern.sra_attn_fwd(qp, kvp, o, lse, B, H, Nq, Nk, scale)
    dq = torch.empty_like(qp)
    if path == "direct":
        dkv = torch.empty_like(kvp)
        kern.sra_attn_bwd_direct(qp, kvp, o, gp, lse, dq, dkv, B, H, Nq, Nk, scale)
        dq2, dkv2 = torch.empty_like(qp), torch.empty_like(kvp)
        kern.sra_attn_bwd_direct(qp, kvp, o, gp, lse, dq2, dkv2, B, H, Nq, Nk, scale)
        assert torch.equal(dq.view(torch.int16), dq2.view(torch.int16))
        assert torch.equal(dkv.view(torch.int16), dkv2.view(torch.int16))
    else:
        dkv32 = torch.zeros(kvp.shape, dtype=torch.float32, device=device)
        kern.sra_attn_bwd(qp, kvp, o, gp, lse, dq, dkv32, B, H, Nq, Nk, scale)
        dkv = dkv32.to(BF)

    def canon(t, n):
        return t.reshape(B, n, H, hd).transpose(1, 2)

    got = {"O": canon(o, Nq), "dQ": canon(dq, Nq), "dK": canon(dkv[..., :Cn], Nk), "dV": canon(dkv[..., Cn:], Nk)}
    what = f"sra tails B{B} H{H} Nq{Nq} Nk{Nk} {regime}"
    R.check_all(got, ref, R.C_BF16, R.U_BF16, what)
    R.assert_within(lse, ref.lse, ref.M_lse, R.C_BF16, R.U_BF16, what=f"{what} lse")
