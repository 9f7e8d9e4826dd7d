"""Data-parallel training: one process per GPU, gradients all-reduced over RCCL/xGMI, overlapped with backward.

The reference's only parallelism is in-process `nn.DataParallel` (src/main_acdc.py:178-179): replicas compute BN
statistics per replica and gradients are summed.  Here each rank owns one GPU and a `ParamArena`; the gradient
arena is laid out in reverse-forward segments (cenet_amd.optim.cenet_segments) and each segment is ONE large
all-reduce launched on a side HIP stream as soon as backward has passed the segment's input (tensor hooks placed by
CENet.forward), so communication hides behind the remaining backward.  xGMI is point-to-point (7 links x ~153 GB/s):
five 4-40 MB collectives keep every link busy without the latency cost of 630 small ones.
Semantics (pinned by tests/test_parallel_gloo.py): BN / CCU statistics per rank (no SyncBN), loss per rank on its
shard, gradients averaged (sum here, 1/world folded into the fused SGD kernel's grad_scale).
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.distributed as dist

from .optim import ParamArena


class GradReducer:
    def __init__(self, arena: ParamArena, group=None, force: bool = False, bf16_buckets: bool = False):
        """bf16_buckets: all-reduce each segment as bf16 (half the xGMI bytes: 66.8 instead of 133.5 MB per step); the
        segment is rounded into a staging buffer, summed by RCCL in bf16 and widened back into the fp32 arena.  Off by
        default: the fp32 sum is the one the known-answer test pins to the mean of the per-shard oracle gradients."""
        self.bf16_buckets = bool(bf16_buckets)
        self._stage = {}
        self.arena = arena
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.active = self.world > 1 or (force and dist.is_initialized())  # force: run collectives even on one rank
        self.cuda = arena.grads.is_cuda
        self.side = torch.cuda.Stream() if self.cuda else None
        self._handles: List = []
        self._done = set()

    # ---- one-time state sync -------------------------------------------------------------------------------
    def broadcast_state(self, model: torch.nn.Module, src: int = 0):
        """Initial broadcast of parameters (one flat buffer) and buffers from rank `src`."""
        if not self.active:
            return
        dist.broadcast(self.arena.params, src, group=self.group)
        self.arena.refresh_shadow()  # a bf16 shadow cast before the broadcast (an earlier forward / eval) is stale now
        for b in model.buffers():
            dist.broadcast(b, src, group=self.group)

    # ---- per-step ---------------------------------------------------------------------------------------------
    def segment_ready(self, i: int):
        """Gradient segment i is final: start its all-reduce (idempotent; called from backward hooks)."""
        if not self.active or i in self._done:
            return
        self._done.add(i)
        buf = self.arena.segment_grad(i)
        if buf.numel() == 0:
            return
        from . import ops
        ops.wgrad_flush()  # the segment's recorded (grouped) weight gradients are launched now, ahead of its collective
        if self.cuda:
            # the collective must see the segment's weight gradients, which may still be running on their own stream
            # (ops._wgrad_side): the COMMUNICATION stream waits for that stream and for the compute stream; the compute
            # stream itself is not held up
            wg = ops.wgrad_stream()
            if wg is not None:
                self.side.wait_stream(wg)
            self.side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.side):
                if self.bf16_buckets:
                    st = self._stage.get(i)
                    if st is None:
                        st = self._stage[i] = torch.empty(buf.shape, dtype=torch.bfloat16, device=buf.device)
                    st.copy_(buf)
                    h = dist.all_reduce(st, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
                    h.wait()       # orders the COMMUNICATION stream after the collective (no host block)
                    buf.copy_(st)
                    h = None
                else:
                    h = dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        elif self.bf16_buckets:
            st = buf.to(torch.bfloat16)
            dist.all_reduce(st, op=dist.ReduceOp.SUM, group=self.group)
            buf.copy_(st)
            h = None
        else:
            h = dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        if h is not None:
            self._handles.append(h)

    def hook(self, i: int):
        """tensor hook factory: `t.register_hook(reducer.hook(i))`."""
        def _h(grad):
            self.segment_ready(i)
            return None
        return _h

    def finish(self):
        """After backward: reduce whatever is left, then order the COMPUTE STREAM after all collectives.  Nothing here
        blocks the host on a GPU: for RCCL work objects `wait()` inserts a stream-side wait on the process group's internal
        communication stream (where the collective actually runs; `wait_stream(self.side)` alone would not cover it), so
        the host returns at once and can issue the next step's zero_grad / forward launches.  (gloo: `wait()` is the host
        wait, there is no stream.)"""
        for i in range(len(self.arena.segments)):
            self.segment_ready(i)
        for h in self._handles:
            h.wait()
        if self.cuda:
            torch.cuda.current_stream().wait_stream(self.side)
        self._handles.clear()
        self._done.clear()

    @property
    def grad_scale(self) -> float:
        return 1.0 / self.world


def attach(model: torch.nn.Module, reducer: Optional[GradReducer]):
    """CENet.forward places the segment hooks when a reducer is attached."""
    model._grad_sync = reducer
    return model
