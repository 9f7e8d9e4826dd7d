"""Replay of real code with every GEMM launch checked: kern.gemm and kern.wgrad_group wrapped (gemm_ref.Replay) so that each call
is compared with the float64 interpreter of the ABI in the BOUND regime, with the operands as they occur; atomic and strided
destinations are read before the launch.

* MI355X (`-m gpu`): one bf16 training step per preset at its baseline batch, on the set-up of tests/test_path_census.py.  Every
  GEMM and grouped launch of the step is checked, and the INSTANCE CENSUS is asserted: the instance names the step launches are a
  subset of the names tests/test_gemm_bounds.py covers (COVERED_NAMES, the list its parametrisation is generated from, and the
  grouped plan classes GROUP_COVERED), so a new tile class cannot enter the step without an exact-regime case.  The test prints
  the names seen with their call counts and the worst |err| / bound per instance.
* host checker (CPU): the full step is too slow there; the CPU leg replays the call sites that use col2im, nb_inner and kinner at
  small sizes in both dtypes under the same wrapper: one PVT block (sr 1, sr 2) forward and backward, the patch-embedding
  convolutions (k7s4, k3s2), one CFAM level and the Non-local block.

A failure names the shape key, the instance, the worst element and its 64 x 64 tile."""
import pytest
import torch

import gemm_ref as G
from backend import dev  # noqa: F401
from cenet_amd import kern, ops, optim
from test_gemm_bounds import COVERED_NAMES, GROUP_COVERED

BF = torch.bfloat16
KNOWN = set(COVERED_NAMES) | set(GROUP_COVERED)


def _report(rep, what):
    print(f"== {what}: {rep.calls} GEMM / grouped launches checked")
    for line in rep.table():
        print("   " + line)
    assert rep.calls > 0, f"{what}: no GEMM launch went through the wrapper"
    assert not rep.failures, f"{what}: {len(rep.failures)} launches outside the bound:\n" + "\n".join(rep.failures[:8])
    new = sorted(set(rep.seen) - KNOWN)
    assert not new, f"{what}: instances without an exact-regime case in tests/test_gemm_bounds.py: {new}"


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["acdc", "synapse", "ham512"])
def test_step_replay_and_instance_census(preset):
    from test_path_census import warm_step
    with warm_step(preset) as step:
        with G.Replay() as rep:
            step()
            torch.cuda.synchronize()
    _report(rep, preset)


# ---- CPU leg (and the same on the MI355X): the call sites of col2im, nb_inner and kinner at small sizes ---------------------------
def _train(dev_, dt, module, x, rep_what, **fw):
    """one training forward + backward of `module` under the wrapper"""
    g = torch.Generator().manual_seed(31)
    m = module.to(dev_)
    with torch.no_grad():
        for p in m.parameters():  # (LayerNorm / BatchNorm weights, zero-initialised scales: no operand stays trivially zero)
            p.add_(0.05 * torch.randn(p.shape, generator=g).to(dev_))
    m.train()
    arena = optim.ParamArena(m)
    x = x.to(dt).to(dev_).requires_grad_(True)
    old = kern.set_compute_bf16(dt == BF)
    try:
        with G.Replay() as rep:
            arena.zero_grad()
            y = m(x, **fw)
            y = y[0] if isinstance(y, tuple) else y
            y.backward(torch.randn(y.shape, generator=g).to(y.dtype).to(dev_))
            ops.wgrad_join()
    finally:
        kern.set_compute_bf16(old)
    assert torch.isfinite(x.grad.float()).all()
    _report(rep, rep_what)
    return rep


DTYPES = pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])


class _Fw(torch.nn.Module):
    """module(x, *extra) as module(x)"""

    def __init__(self, inner, *extra):
        super().__init__()
        self.inner, self.extra = inner, extra

    def forward(self, x):
        return self.inner(x, *self.extra)


@DTYPES
@pytest.mark.parametrize("sr", [1, 2])
def test_replay_pvt_block(dev, dt, sr):
    """tokens [B, H W, C] through LN -> q / kv (spatial reduction: a k = stride = sr convolution + LN) -> attention -> proj with the
    residual and DropPath scale in its epilogue -> Mlp; forward and backward"""
    from cenet_amd.networks.cenet.pvtv2 import Block
    torch.manual_seed(3)
    B, H, W, Cn = 2, 6, 10, 32
    blk = Block(Cn, num_heads=2, mlp_ratio=2.0, qkv_bias=True, drop_path=0.1, sr_ratio=sr)
    x = torch.randn(B, H * W, Cn, generator=torch.Generator().manual_seed(4))
    _train(dev, dt, _Fw(blk, H, W), x, f"PVT block sr{sr} {dt}")


@DTYPES
@pytest.mark.parametrize("k,stride,cin", [(7, 4, 3), (3, 2, 16)])
def test_replay_patch_embed(dev, dt, k, stride, cin):
    """the overlapping patch embeddings: im2col forward, col2im data gradient (k > stride: atomic scatter), gathered weight gradient"""
    from cenet_amd.networks.cenet.pvtv2 import OverlapPatchEmbed
    torch.manual_seed(5)
    pe = OverlapPatchEmbed(img_size=24, patch_size=k, stride=stride, in_chans=cin, embed_dim=40)
    x = torch.randn(2, cin, 22, 26, generator=torch.Generator().manual_seed(6))
    _train(dev, dt, pe, x, f"patch embed k{k}s{stride} {dt}")


@DTYPES
def test_replay_cfam_level(dev, dt):
    from cenet_amd.networks.cenet.modules.cfam import CFAModule
    torch.manual_seed(7)
    m = CFAModule(32, mca_rates=[1, 2, 3], init_value=0.5)
    x = torch.randn(2, 32, 7, 7, generator=torch.Generator().manual_seed(8))
    _train(dev, dt, m, x, f"CFAM level {dt}")


@DTYPES
def test_replay_nonlocal_block(dev, dt):
    from cenet_amd.networks.cenet.modules.nlb import Nonlocal
    torch.manual_seed(9)
    m = Nonlocal(32)
    x = torch.randn(2, 32, 9, 7, generator=torch.Generator().manual_seed(10))
    _train(dev, dt, m, x, f"Non-local block {dt}")
