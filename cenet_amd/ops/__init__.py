"""cenet_amd.ops — autograd operators of the CENet hot path, forward AND backward on hand-written HIP kernels.

One module per operator family (round 6: cut out of one 3 100-line module).  Each module imports by name what it uses from the module that
defines it and lists in `__all__` the names it defines: the public ones and the private ones that other modules, tests, tools or
bench.py reach.  This package re-exports exactly those lists, so `from cenet_amd import ops; ops.linear(...)` / `ops._WgradCfg` /
`ops._ZeroWs` read as they always did (torch, os and the like are not among them):
  ops.infra          shared plumbing of the operator modules: tensor allocation helpers, zero-at-rest workspaces, parameter / gradient views into the
  ops.linear         GEMM-backed operators: Linear / MultiLinear in token layout, 1x1 convolutions on NCHW, dense k x k convolutions (implicit GEMM, direct
  ops.norm           LayerNorm over the last dimension and train-mode BatchNorm (+ fused activation)
  ops.depthwise      depthwise 3x3 convolutions (token layout and NCHW) and the fused PVT Mlp half (csrc/pvt_mlp.hip)
  ops.attention      attention operators: spatial-reduction attention, Non-local attention, differential attention heads + combine
  ops.glue           layout / glue operators: token <-> NCHW, concat / split (+ merged depthwise branches), grouped 1x1, add + activation, SiLU product,
  ops.decoder_fused  resampling operators and the channel-local fused chains of the decoder and the head (csrc/chanloc.hip, csrc/res_tail.hip): EUCB front,
  ops.gates          CCU and SRM gates (cfam.py:251-264, 93-101)
  ops.dseb_loss      DSEB combine (dseb.py:40-50,63-76,156-163) and the fused segmentation loss (utils/core.py:44-131,161-188)
"""
import sys

from .infra import *  # noqa: F401,F403
from .linear import *  # noqa: F401,F403
from .norm import *  # noqa: F401,F403
from .depthwise import *  # noqa: F401,F403
from .attention import *  # noqa: F401,F403
from .glue import *  # noqa: F401,F403
from .decoder_fused import *  # noqa: F401,F403
from .gates import *  # noqa: F401,F403
from .dseb_loss import *  # noqa: F401,F403

# (through sys.modules: `ops.linear`, `ops.norm`, ... are what the modules of those names export, not the modules)
__all__ = [n for m in ("infra", "linear", "norm", "depthwise", "attention", "glue", "decoder_fused", "gates", "dseb_loss")
           for n in sys.modules[f"{__name__}.{m}"].__all__]
del sys
