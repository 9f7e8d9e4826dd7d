"""Flat parameter/gradient arena, the fused optimizers and the LR schedules.

Mirrors the reference's optimiser plumbing (src/utils/core.py:12-41: `get_optimizer` — torch.optim.SGD(lr, momentum 0.9,
weight_decay), Adam, AdamW — and `get_scheduler` — poly, cosine, exp, step, custom) on top of ONE contiguous fp32 buffer for
parameters, one for gradients and one per optimizer state (momentum; Adam's two moments), so that per step there is one
memset, one fused update kernel and a handful of large all-reduces instead of 630 small ones.
`get_optimizer` / `get_scheduler` here take the reference's arguments and strings.  `torch.optim.SGD(net.parameters())` keeps
working on arena-backed parameters (their `.data` / `.grad` are views), so the reference's `get_optimizer` can also be used
unchanged.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import kern

ALIGN = 64  # elements (256 B)


class ParamArena:
    """Re-homes every trainable parameter of `model` into one flat buffer (and its gradient into another).

    segments: optional ordered list of (name, predicate(param_name) -> bool); parameters are laid out segment by
    segment so that a gradient segment is one contiguous slice (used as an all-reduce bucket). Call AFTER the model
    has been moved to its device.
    """

    def __init__(self, model: nn.Module, segments: Optional[Sequence[Tuple[str, Callable[[str], bool]]]] = None):
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        if not named:
            raise ValueError("no trainable parameters")
        dev = named[0][1].device
        if segments is None:
            segments = [("all", lambda n: True)]
        # parameter groups that a module wants back to back WITHOUT padding between the members (`arena_groups()` on any
        # sub-module: lists of equally shaped parameters, e.g. the same weight of the three dilated branches of a
        # MultiOrderDWConv), so that one kernel launch can address them as one [n, ...] tensor (cenet_amd.ops.merged_param)
        name_of = {id(p): n for n, p in named}
        group_of = {}
        for m in model.modules():
            fn = getattr(m, "arena_groups", None)
            if fn is None:
                continue
            for grp in fn():
                names = [name_of[id(q)] for q in grp if id(q) in name_of]
                if len(names) == len(grp) and len(names) > 1:
                    for n in names:
                        group_of[n] = names
        byname = dict(named)
        order, self.segments = [], []
        taken = set()
        off = 0
        for sname, pred in segments:
            start = off
            for n, p in named:
                if n in taken or not pred(n):
                    continue
                members = group_of.get(n, [n])
                if any(not pred(k) or k in taken for k in members):
                    members = [n]  # a group never straddles a segment
                for k in members:
                    taken.add(k)
                    order.append((k, byname[k], off))
                    off += byname[k].numel()
                off = (off + ALIGN - 1) // ALIGN * ALIGN
            self.segments.append((sname, start, off))
        left = [n for n, _ in named if n not in taken]
        if left:
            raise ValueError(f"parameters not covered by any segment: {left[:5]}")
        self.numel = off
        self.params = torch.zeros(off, device=dev, dtype=torch.float32)
        self.grads = torch.zeros(off, device=dev, dtype=torch.float32)
        self.index = {}
        with torch.no_grad():
            for n, p, o in order:
                view = self.params[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = self.grads[o:o + p.numel()].view(p.shape)
                p._cenet_grad_home = self._home(o, p.numel(), tuple(p.shape))  # ops.grad_buf: re-attach after .grad = None
                self.index[n] = (o, p.numel())
        self._plist = [p for _, p, _ in order]
        self._offs = [o for _, _, o in order]
        # bf16 shadow of the parameters (the GEMM operand of the throughput mode), created on first use by kern.wq
        self.shadow = None
        for p, o in zip(self._plist, self._offs):
            p._cenet_arena_slot = (self, o)

    def enable_shadow(self):
        """One flat bf16 copy of `params`; every parameter's `_cenet_shadow` is a view into it.  The fused optimizers' step rewrites
        it in the same kernel that updates the fp32 master copy."""
        if self.shadow is not None:
            return
        self.shadow = torch.empty(self.numel, device=self.params.device, dtype=torch.bfloat16)
        kern.cast_into(self.params, self.shadow)
        for p, o in zip(self._plist, self._offs):
            p._cenet_shadow = self.shadow[o:o + p.numel()].view(p.shape)
            p._cenet_shadow_ver = p._version

    def refresh_shadow(self):
        """Re-cast the whole bf16 shadow from the fp32 master copy.  Needed after any RAW write to `self.params` (the flat
        broadcast of `GradReducer.broadcast_state`, a checkpoint restored into the arena): `kern.wq` detects stale shadows by
        each parameter's own `_version`, which a write through the flat buffer does not bump."""
        if self.shadow is None:
            return
        kern.cast_into(self.params, self.shadow)
        for p in self._plist:
            p._cenet_shadow_ver = p._version

    def _home(self, o: int, n: int, shape):
        def home():
            g = self.grads[o:o + n]
            kern.zero_(g)  # the slot still holds the previous step's gradient
            return g.view(shape)
        return home

    def zero_grad(self):
        """One memset for all gradients (re-attaches views if a caller set .grad to None)."""
        from . import ops
        ops.wgrad_join()
        kern.zero_(self.grads)
        for p, o in zip(self._plist, self._offs):
            if p.grad is None or p.grad.data_ptr() != self.grads.data_ptr() + 4 * o:
                p.grad = self.grads[o:o + p.numel()].view(p.shape)

    def segment_grad(self, i: int) -> torch.Tensor:
        _, s, e = self.segments[i]
        return self.grads[s:e]


class _HyperStage:
    """Uploads a fused optimizer's hyper-parameters (a few fp32 values) into its device buffer.

    On the GPU the copy is asynchronous from PINNED staging (a pageable temporary could be recycled by the host before the copy
    executes when the host runs ahead of the GPU, e.g. under hipGraph replay).  4 slots rotate; a slot is reused only after the
    copy that last read it has executed (its event), which also bounds how far the host can run ahead of the GPU: 4 steps."""

    def __init__(self, n: int, slots: int = 4):
        self.n, self.slots = n, slots
        self._stage = None

    def upload(self, hyper: torch.Tensor, vals: Sequence[float]):
        if not hyper.is_cuda:
            hyper.copy_(torch.tensor(vals, dtype=torch.float32))
            return
        if self._stage is None:
            self._stage = [torch.zeros(self.n, dtype=torch.float32).pin_memory() for _ in range(self.slots)]
            self._stage_ev = [None] * self.slots
            self._slot = 0
        i = self._slot
        self._slot = (i + 1) % self.slots
        if self._stage_ev[i] is not None:
            self._stage_ev[i].synchronize()
        h = self._stage[i]
        for j, v in enumerate(vals):
            h[j] = v
        hyper.copy_(h, non_blocking=True)
        if self._stage_ev[i] is None:
            self._stage_ev[i] = torch.cuda.Event()
        self._stage_ev[i].record()


class FusedSGD:
    """torch.optim.SGD(momentum, weight_decay, dampening 0, nesterov False) semantics, one kernel launch per step."""

    def __init__(self, arena: ParamArena, lr: float, momentum: float = 0.9, weight_decay: float = 1e-4,
                 grad_scale: float = 1.0):
        self.arena = arena
        # ONE persistent group dict, as torch.optim exposes it: `for g in opt.param_groups: g["lr"] = x` (warm-up code, torch
        # LR schedulers) must take effect.  lr / momentum / weight_decay are read from it at every step.
        self.param_groups = [{"lr": lr, "momentum": momentum, "weight_decay": weight_decay, "params": arena._plist}]
        self.grad_scale = grad_scale
        self.buf = torch.zeros_like(arena.params)
        self.hyper = torch.zeros(5, device=arena.params.device, dtype=torch.float32)
        self._stage = _HyperStage(5)
        self._steps = 0
        self._sync_hyper()

    # lr / momentum / weight_decay live in param_groups[0] (torch.optim idiom); these properties are the short spelling
    lr = property(lambda self: self.param_groups[0]["lr"], lambda self, v: self.param_groups[0].__setitem__("lr", v))
    momentum = property(lambda self: self.param_groups[0]["momentum"],
                        lambda self, v: self.param_groups[0].__setitem__("momentum", v))
    weight_decay = property(lambda self: self.param_groups[0]["weight_decay"],
                            lambda self, v: self.param_groups[0].__setitem__("weight_decay", v))

    def _sync_hyper(self):
        vals = [self.lr, self.momentum, self.weight_decay, self.grad_scale, 1.0 if self._steps == 0 else 0.0]
        self._stage.upload(self.hyper, vals)

    def zero_grad(self, set_to_none: bool = False):
        self.arena.zero_grad()

    def set_lr(self, lr: float):
        self.lr = lr

    def step(self, sync_hyper: bool = True):
        """sync_hyper=False: the caller has uploaded the hyper-parameters already (`prepare()`); needed when the step is
        captured in a HIP graph, where a host->device copy is not allowed inside the captured region."""
        if sync_hyper:
            self._sync_hyper()
        from . import ops
        ops.wgrad_join()  # weight gradients issued on the side stream (ops._wgrad_side) must have landed
        kern.sgd_step(self.arena.params, self.arena.grads, self.buf, self.hyper, self.arena.numel, self.arena.shadow)
        self._steps += 1

    def prepare(self):
        """Upload lr / momentum / wd / grad_scale / first-step flag for the NEXT step (call before a graph replay)."""
        self._sync_hyper()

    def state_dict(self):
        """momentum per parameter NAME (`momentum`: name -> tensor): the flat arena layout (segments, arena groups, padding) is
        an implementation detail that may differ between the run that saved and the run that loads"""
        idx = self.arena.index
        return {"momentum": {n: self.buf[o:o + k].detach().clone() for n, (o, k) in idx.items()}, "steps": self._steps,
                "lr": self.lr}

    def load_state_dict(self, sd):
        if "momentum" in sd:
            idx = self.arena.index
            missing = [n for n in idx if n not in sd["momentum"]]
            if missing:
                raise KeyError(f"momentum missing for parameters {missing[:5]}")
            for n, (o, k) in idx.items():
                self.buf[o:o + k].copy_(sd["momentum"][n].reshape(-1).to(self.buf.device))
        else:
            # (the flat 'buf' of files written before the arena grew groups: the layout is not recorded in the file, and a
            # same-size buffer of another layout would be silently misassigned)
            raise ValueError("training state without per-parameter momentum ('momentum': name -> tensor); re-save it")
        self._steps, self.lr = sd["steps"], sd["lr"]

    def state_buffers(self) -> List[torch.Tensor]:
        """the flat per-parameter state (what a caller snapshots around a capture's warm-up steps)"""
        return [self.buf]


class FusedAdam:
    """torch.optim.Adam (`decoupled=False`) / AdamW (`decoupled=True`) semantics — amsgrad, maximize off — over the arena, one
    kernel launch per step (csrc/adam.hip).  The same contract as FusedSGD: one persistent `param_groups[0]` (lr, betas, eps,
    weight_decay) read at every step, `grad_scale` (GradReducer's 1/world), `prepare()` / `step(sync_hyper=False)` for captured
    steps, `_steps`.  The bias corrections of step t = `_steps + 1` are computed on the host in double when the hyper-parameters
    are uploaded (step() or prepare()), so a graph replay preceded by prepare() advances them."""

    kind = "adam"
    decoupled = False

    def __init__(self, arena: ParamArena, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, grad_scale: float = 1.0, *, amsgrad: bool = False, maximize: bool = False,
                 capturable: bool = False, differentiable: bool = False, foreach: Optional[bool] = None,
                 fused: Optional[bool] = None):
        # options of torch.optim.Adam that the reference never sets are refused, not ignored
        for name, val in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable),
                          ("differentiable", differentiable)):
            if val:
                raise ValueError(f"{type(self).__name__}: {name}=True is not supported")
        for name, val in (("foreach", foreach), ("fused", fused)):
            if val is not None:
                raise ValueError(f"{type(self).__name__}: {name}= selects a torch implementation; the arena has its own kernel")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self.arena = arena
        self.param_groups = [{"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay,
                              "params": arena._plist}]
        self.grad_scale = grad_scale
        self.exp_avg = torch.zeros_like(arena.params)
        self.exp_avg_sq = torch.zeros_like(arena.params)
        self.hyper = torch.zeros(12, device=arena.params.device, dtype=torch.float32)
        self._stage = _HyperStage(12)
        self._steps = 0
        self._sync_hyper()

    lr = property(lambda self: self.param_groups[0]["lr"], lambda self, v: self.param_groups[0].__setitem__("lr", v))
    betas = property(lambda self: self.param_groups[0]["betas"],
                     lambda self, v: self.param_groups[0].__setitem__("betas", tuple(v)))
    eps = property(lambda self: self.param_groups[0]["eps"], lambda self, v: self.param_groups[0].__setitem__("eps", v))
    weight_decay = property(lambda self: self.param_groups[0]["weight_decay"],
                            lambda self, v: self.param_groups[0].__setitem__("weight_decay", v))

    def _sync_hyper(self):
        # torch's _single_tensor_adam: the step counter t, the bias corrections and step_size in Python (double) arithmetic
        lr, (b1, b2), eps, wd = self.lr, self.betas, self.eps, self.weight_decay
        t = float(self._steps + 1)
        bias_correction1 = 1 - b1 ** t
        bias_correction2 = 1 - b2 ** t
        step_size = lr / bias_correction1
        bias_correction2_sqrt = bias_correction2 ** 0.5
        vals = [lr, b1, b2, eps, wd, self.grad_scale, step_size, bias_correction2_sqrt, 1.0 if self.decoupled else 0.0,
                1 - b1, 1 - b2, 1 - lr * wd]
        self._stage.upload(self.hyper, vals)

    def zero_grad(self, set_to_none: bool = False):
        self.arena.zero_grad()

    def set_lr(self, lr: float):
        self.lr = lr

    def step(self, sync_hyper: bool = True):
        """sync_hyper=False: the caller has uploaded the hyper-parameters of this step already (`prepare()`), as a captured step
        must (no host->device copy inside a captured region)."""
        if sync_hyper:
            self._sync_hyper()
        from . import ops
        ops.wgrad_join()  # weight gradients issued on the side stream (ops._wgrad_side) must have landed
        kern.adam_step(self.arena.params, self.arena.grads, self.exp_avg, self.exp_avg_sq, self.hyper, self.arena.numel,
                       self.arena.shadow)
        self._steps += 1

    def prepare(self):
        """Upload lr / betas / eps / wd / grad_scale and the bias corrections of the NEXT step (call before a graph replay)."""
        self._sync_hyper()

    def state_dict(self):
        """`exp_avg` / `exp_avg_sq` per parameter NAME (the flat layout may differ between the saving and the loading run), the
        step counter (the bias corrections continue from it), lr and the optimizer kind"""
        idx = self.arena.index
        return {"kind": self.kind,
                "exp_avg": {n: self.exp_avg[o:o + k].detach().clone() for n, (o, k) in idx.items()},
                "exp_avg_sq": {n: self.exp_avg_sq[o:o + k].detach().clone() for n, (o, k) in idx.items()},
                "steps": self._steps, "lr": self.lr}

    def load_state_dict(self, sd):
        kind = sd.get("kind", "sgd" if "momentum" in sd else None)
        if kind != self.kind:
            raise ValueError(f"{type(self).__name__}.load_state_dict: the state was written by a {kind or 'different'} "
                             f"optimizer, not {self.kind}")
        idx = self.arena.index
        for key, buf in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            missing = [n for n in idx if n not in sd[key]]
            if missing:
                raise KeyError(f"{key} missing for parameters {missing[:5]}")
            for n, (o, k) in idx.items():
                buf[o:o + k].copy_(sd[key][n].reshape(-1).to(buf.device))
        self._steps, self.lr = sd["steps"], sd["lr"]

    def state_buffers(self) -> List[torch.Tensor]:
        return [self.exp_avg, self.exp_avg_sq]


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW: decoupled weight decay (p *= 1 - lr wd before the Adam update); torch's default weight_decay 1e-2"""

    kind = "adamw"
    decoupled = True

    def __init__(self, arena: ParamArena, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, grad_scale: float = 1.0, **kw):
        super().__init__(arena, lr, betas, eps, weight_decay, grad_scale, **kw)


class PolyLR:
    """core.py:31: lr = base * (1 - step / max_iterations) ** 0.9 (LambdaLR semantics: step() after optimizer.step())."""

    def __init__(self, optimizer: FusedSGD, max_iterations: int, power: float = 0.9):
        self.opt, self.max_it, self.power = optimizer, max_iterations, power
        self.base_lr = optimizer.lr
        self.last_epoch = 0

    def get_last_lr(self) -> List[float]:
        return [self.opt.lr]

    def step(self):
        self.last_epoch += 1
        self.opt.set_lr(self.base_lr * (1 - self.last_epoch / self.max_it) ** self.power)


class _FusedLRSchedule:
    """Base of the cosine / exp / step / custom schedules (PolyLR's interface plus a kind-checked state_dict).  step() advances
    `last_epoch` and derives the next lr from the optimizer's present one: cosine, exp and step are the recursive forms of torch
    2.10's `get_lr()`, so long runs agree with torch to the last bit, and a resumed run continues from the lr restored with the
    optimizer's state.  Works on any fused optimizer (anything with `lr` and `set_lr`), stepped once per iteration after
    optimizer.step()."""

    kind = ""

    def __init__(self, optimizer):
        self.opt = optimizer
        self.base_lr = optimizer.lr
        self.last_epoch = 0

    def get_last_lr(self) -> List[float]:
        return [self.opt.lr]

    def step(self):
        self.last_epoch += 1
        self.opt.set_lr(self._next_lr(self.opt.lr))

    def _next_lr(self, lr: float) -> float:
        raise NotImplementedError

    def state_dict(self) -> dict:
        return {"kind": self.kind, "last_epoch": self.last_epoch, "base_lr": self.base_lr}

    def load_state_dict(self, sd: dict):
        if sd.get("kind") != self.kind:
            raise ValueError(f"{type(self).__name__}.load_state_dict: the state was written by a "
                             f"{sd.get('kind') or 'poly'} schedule, not {self.kind}")
        self.last_epoch, self.base_lr = int(sd["last_epoch"]), float(sd["base_lr"])


class CosineLR(_FusedLRSchedule):
    """core.py:28: torch CosineAnnealingLR(T_max=max_iterations), eta_min 0 — its recursive form"""

    kind = "cosine"

    def __init__(self, optimizer, T_max: int, eta_min: float = 0.0):
        super().__init__(optimizer)
        self.T_max, self.eta_min = T_max, eta_min

    def _next_lr(self, lr):
        e, T, lo = self.last_epoch, self.T_max, self.eta_min
        if (e - 1 - T) % (2 * T) == 0:
            return lr + (self.base_lr - lo) * (1 - math.cos(math.pi / T)) / 2
        return (1 + math.cos(math.pi * e / T)) / (1 + math.cos(math.pi * (e - 1) / T)) * (lr - lo) + lo


class ExponentialLR(_FusedLRSchedule):
    """core.py:32: torch ExponentialLR(gamma=0.95): lr *= gamma per step"""

    kind = "exp"

    def __init__(self, optimizer, gamma: float = 0.95):
        super().__init__(optimizer)
        self.gamma = gamma

    def _next_lr(self, lr):
        return lr * self.gamma


class StepLR(_FusedLRSchedule):
    """core.py:34: torch StepLR(step_size=200, gamma=0.5): lr *= gamma every step_size steps"""

    kind = "step"

    def __init__(self, optimizer, step_size: int = 200, gamma: float = 0.5):
        super().__init__(optimizer)
        self.step_size, self.gamma = step_size, gamma

    def _next_lr(self, lr):
        if self.last_epoch == 0 or self.last_epoch % self.step_size != 0:
            return lr
        return lr * self.gamma


class CustomLR(_FusedLRSchedule):
    """core.py:191-212 (CustomLR): a linear ramp from lr_start_high to lr_end_high over the first T_first steps, then a cosine
    from lr_start_low to lr_end_low over max_epochs - T_first steps, in closed form from `last_epoch`.  The reference steps it
    once per ITERATION while get_scheduler feeds it args.max_epochs (core.py:36-37, main_acdc.py:257), so its "epochs" are
    iterations; kept as the reference runs it.  Like any torch scheduler it sets the optimizer's lr to its value at step 0 when
    it is created (lr_start_high, 10x the base lr in get_scheduler)."""

    kind = "custom"

    def __init__(self, optimizer, T_first: int = 3, lr_start_high: float = 0.01, lr_end_high: float = 0.005,
                 lr_start_low: float = 0.001, lr_end_low: float = 0.00001, max_epochs: int = 50):
        super().__init__(optimizer)
        self.T_first, self.max_epochs = T_first, max_epochs
        self.lr_start_high, self.lr_end_high = lr_start_high, lr_end_high
        self.lr_start_low, self.lr_end_low = lr_start_low, lr_end_low
        optimizer.set_lr(self._next_lr(None))

    def _next_lr(self, lr):
        if self.last_epoch < self.T_first:
            progress = self.last_epoch / self.T_first
            return self.lr_start_high - (self.lr_start_high - self.lr_end_high) * progress
        progress = (self.last_epoch - self.T_first) / (self.max_epochs - self.T_first)
        # (numpy's cos, as the reference evaluates it)
        return float(self.lr_start_low - (self.lr_start_low - self.lr_end_low) * (0.5 * (1 - np.cos(np.pi * progress))))


def _arena_of(model: nn.Module) -> Optional[ParamArena]:
    """the ParamArena that already holds every trainable parameter of `model`, None if none does"""
    slots = [getattr(p, "_cenet_arena_slot", None) for p in model.parameters() if p.requires_grad]
    arenas = {id(s[0]): s[0] for s in slots if s is not None}
    if not arenas:
        return None
    if len(arenas) > 1 or any(s is None for s in slots):
        raise ValueError("get_optimizer: the model's parameters are split between arenas (or only partly in one)")
    return next(iter(arenas.values()))


def get_optimizer(model: nn.Module, args):
    """core.py:12-24 on the arena: args.optimizer in {'SGD', 'Adam', 'AdamW'} (any case), args.base_lr, args.weight_decay ->
    FusedSGD(momentum 0.9) / FusedAdam / FusedAdamW (betas (0.9, 0.999), eps 1e-8).  The parameters are re-homed into a
    ParamArena laid out by cenet_segments() (one segment for a model whose parameter names are not CENet's) unless they already
    live in one, which is then used as it is."""
    name = args.optimizer.lower()
    if name not in ("adam", "adamw", "sgd"):
        raise NotImplementedError(f"Optimizer {args.optimizer} not implemented")
    arena = _arena_of(model)
    if arena is None:
        names = [n for n, p in model.named_parameters() if p.requires_grad]
        segs = cenet_segments()
        covered = all(any(pred(n) for _, pred in segs) for n in names)
        arena = ParamArena(model, segs if covered else None)
    if name == "adam":
        return FusedAdam(arena, lr=args.base_lr, weight_decay=args.weight_decay)
    if name == "adamw":
        return FusedAdamW(arena, lr=args.base_lr, weight_decay=args.weight_decay)
    return FusedSGD(arena, lr=args.base_lr, momentum=0.9, weight_decay=args.weight_decay)


def get_scheduler(optimizer, args, max_iterations: int):
    """core.py:27-40: args.scheduler in {'cosine', 'poly', 'exp', 'step', 'custom'} (any case); 'custom' reads args.base_lr and
    args.max_epochs.  Step the result once per iteration after optimizer.step() (main_acdc.py:256-257)."""
    name = args.scheduler.lower()
    if name == "cosine":
        return CosineLR(optimizer, T_max=max_iterations)
    if name == "poly":
        return PolyLR(optimizer, max_iterations=max_iterations)
    if name == "exp":
        return ExponentialLR(optimizer, gamma=0.95)
    if name == "step":
        return StepLR(optimizer, step_size=200, gamma=0.5)
    if name == "custom":
        return CustomLR(optimizer, T_first=5, lr_start_high=10 * args.base_lr, lr_end_high=5 * args.base_lr,
                        lr_start_low=args.base_lr, lr_end_low=0, max_epochs=args.max_epochs)
    raise NotImplementedError(f"Scheduler <{args.scheduler}> not implemented")


def cenet_segments():
    """Arena layout for CENet in reverse-forward order: the gradient of each segment is complete (and can start its
    all-reduce) when backward reaches the segment's input (cenet_amd.parallel)."""
    return [("head+decoder", lambda n: n.startswith(("out.", "decoder."))),
            ("stage4", lambda n: n.startswith(("backbone.patch_embed4", "backbone.block4", "backbone.norm4"))),
            ("stage3", lambda n: n.startswith(("backbone.patch_embed3", "backbone.block3", "backbone.norm3"))),
            ("stage2", lambda n: n.startswith(("backbone.patch_embed2", "backbone.block2", "backbone.norm2"))),
            ("stage1", lambda n: n.startswith(("backbone.patch_embed1", "backbone.block1", "backbone.norm1")))]
