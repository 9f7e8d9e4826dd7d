"""CENet — mirrors reference src/networks/cenet/net.py:8-64 (same ctor signature, attributes and state-dict keys)."""
from __future__ import annotations

import torch
import torch.nn as nn

from ... import kern
from .decoders import Decoder
from .encoder import get_encoder2d
from .out import OutHead


class CENet(nn.Module):
    def __init__(self, input_channels=1, num_classes=1, scale_factors=[0.8, 0.4], diffatt_num_heads=[2, 2, 2],
                 encoder='pvt_v2_b2', enc_pretrain=False, freeze_bb=False, skip_mode="cat", dec_up_block='eucb',
                 out_merge_mode="cat", out_up_block="eucb", out_up_ks=3, writer=None, base_ptdir='.'):
        super().__init__()
        self.writer = writer
        self.backbone, channels = get_encoder2d(input_channels=input_channels, encoder=encoder, pretrain=enc_pretrain,
                                                freeze_bb=freeze_bb, base_ptdir=base_ptdir)
        self.decoder = Decoder(channels=channels, scale_factors=scale_factors, skip_mode=skip_mode,
                               num_heads=diffatt_num_heads, up_block=dec_up_block, writer=writer)
        self.out = OutHead(dec_in_spatial=56, dec_in_channels=channels[-1], x_in_spatial=224,
                           x_in_channels=input_channels, out_channels=num_classes, merge_mode=out_merge_mode,
                           up_block=out_up_block, up_ks=out_up_ks)
        from ... import opaque
        opaque.register(self)

    def __setstate__(self, state):  # (deepcopy / unpickling: the copy is its own module for cenet_amd::forward)
        super().__setstate__(state)
        from ... import opaque
        opaque.register(self)

    def forward(self, x):
        if getattr(self, "_is_replica", False):
            # torch.nn.parallel.replicate marks the per-device copies a multi-device nn.DataParallel makes.  Their "parameters" are
            # Broadcast outputs, not leaves: the kernels here add parameter gradients IN PLACE into param.grad, which would never reach
            # the wrapped module's parameters — training would silently lose every gradient.  Refuse instead (INTEGRATION.md,
            # "nn.DataParallel"): one device works through the wrap; N GPUs = one process per GPU + parallel.GradReducer.
            raise RuntimeError("cenet_amd.CENet was replicated by a multi-device nn.DataParallel (main_acdc.py:178-179). In-process "
                               "replication is not supported: parameter gradients are accumulated in place and would not flow back "
                               "through Broadcast. Use nn.DataParallel(net, device_ids=[one device]) (works unchanged) or launch one "
                               "process per GPU with cenet_amd.parallel.GradReducer (python -m torch.distributed.run ... ; see "
                               "INTEGRATION.md, 'Data-parallel').")
        if torch.jit.is_tracing() or torch.compiler.is_compiling():
            # Tracing callers — utils/utils.py:171-185 (print_param_flops -> fvcore FlopCountAnalysis = torch.jit.trace, called at
            # main_acdc.py:128) and main_acdc.py:188-191 (torch.compile(net, mode='default', fullgraph=True)) — see the forward as ONE
            # opaque operator with a shape function and an autograd formula (cenet_amd/opaque.py): a tracer cannot look inside
            # ctypes launches of hand-written kernels, and has nothing to optimise there
            from ... import opaque
            return opaque.forward(self, x, self._bf16_mode(x))
        return self._forward(x)

    def _bf16_mode(self, x) -> bool:
        return bool(x.dtype == torch.bfloat16 or kern.get_compute_bf16() or (x.is_cuda and torch.is_autocast_enabled("cuda")))

    def _forward(self, x):
        # throughput mode (kern.set_compute_bf16): the whole network runs on bf16 tensors — the input is rounded once here
        # and every kernel downstream follows the element type of its input; logits come back as bf16
        # The reference's AMP switch (main_acdc.py:192-199,243-249: `with autocast('cuda')` + GradScaler) selects the same
        # mode: under an enabled CUDA autocast region the forward runs on bf16 tensors (fp32 islands as in
        # multihead_diffattn.py:108, rms_norm.py:19: softmax / norm statistics / accumulators; parameters stay fp32).  bf16 has
        # fp32's exponent range, so the GradScaler the caller wraps around the step is harmless but not needed.
        amp = x.is_cuda and torch.is_autocast_enabled("cuda")
        if (kern.get_compute_bf16() or amp) and x.dtype == torch.float32:
            x = kern.cast(x, torch.bfloat16)
        # grayscale input: the 3-channel replication of net.py:55 is a zero-stride channel read in patch_embed1
        x1, x2, x3, x4 = self.backbone(x)
        sync = getattr(self, "_grad_sync", None)
        if sync is not None and self.training and x4.requires_grad:
            # gradient-arena segments (cenet_amd.optim.cenet_segments) become final when backward reaches these
            # tensors: head+decoder at x4, stage4 at x3, stage3 at x2, stage2 at x1 (stage1: end of backward)
            for i, t in enumerate((x4, x3, x2, x1)):
                t.register_hook(sync.hook(i))
        dec = self.decoder(x4, [x3, x2, x1])
        return self.out(dec, x)
