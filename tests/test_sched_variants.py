"""The reference's other LR schedules (src/utils/core.py:27-40: cosine, exp, step, custom) and its get_optimizer /
get_scheduler dispatch, on the fused optimizers: lr sequences against tests/golden/optim_adam_sched.npz
(tools/gen_golden_optim.py, made from the reference itself) and a training-state resume that continues bit-identically."""
import argparse
import os

import numpy as np
import pytest
import torch

from backend import use_sim
from conftest import GOLDEN

SCHEDULES = ["cosine", "exp", "step", "custom"]


@pytest.fixture
def sim():
    from cenet_amd import _lib
    yield use_sim()
    _lib._LIB = None
    _lib._HOSTSIM = False


def _golden():
    return np.load(os.path.join(GOLDEN, "optim_adam_sched.npz"))


def _args(**kw):
    base = dict(optimizer="sgd", base_lr=0.01, weight_decay=1e-4, scheduler="poly", max_epochs=8)
    base.update(kw)
    return argparse.Namespace(**base)


def _vec_module(n=3, dev="cpu"):
    m = torch.nn.Module()
    m.p = torch.nn.Parameter(torch.zeros(n, device=dev))
    return m


@pytest.mark.parametrize("opt_name", ["SGD", "AdamW"])
@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("tag", ["a", "b"])
def test_lr_sequence_matches_the_reference(tag, sched, opt_name):
    """the lr the train loop reads before each scheduler.step() (main_acdc.py:256-257), every iteration of the run; 'b' is
    120 epochs x 96 iterations (the recursive forms over 11 520 steps, 57 StepLR boundaries)"""
    from cenet_amd import optim
    z = _golden()
    args = _args(optimizer=opt_name, base_lr=float(z[f"{tag}.base_lr"]), scheduler=sched,
                 max_epochs=int(z[f"{tag}.max_epochs"]))
    opt = optim.get_optimizer(_vec_module(), args)
    sch = optim.get_scheduler(opt, args, int(z[f"{tag}.max_it"]))
    want = z[f"{tag}.{sched}"]
    got = np.empty_like(want)
    for i in range(len(want)):
        got[i] = sch.get_last_lr()[0]
        sch.step()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert sch.last_epoch == len(want)


def test_get_optimizer_dispatches_on_the_reference_strings():
    from cenet_amd import optim
    for name, cls in (("SGD", optim.FusedSGD), ("sgd", optim.FusedSGD), ("Adam", optim.FusedAdam), ("ADAM", optim.FusedAdam),
                      ("AdamW", optim.FusedAdamW), ("adamw", optim.FusedAdamW)):
        opt = optim.get_optimizer(_vec_module(), _args(optimizer=name, base_lr=0.02, weight_decay=0.3))
        assert type(opt) is cls, name
        assert opt.lr == 0.02 and opt.weight_decay == 0.3
    opt = optim.get_optimizer(_vec_module(), _args(optimizer="adam"))
    assert opt.betas == (0.9, 0.999) and opt.eps == 1e-8
    assert optim.get_optimizer(_vec_module(), _args(optimizer="sgd")).momentum == 0.9
    with pytest.raises(NotImplementedError, match="RMSprop"):
        optim.get_optimizer(_vec_module(), _args(optimizer="RMSprop"))


def test_get_optimizer_keeps_an_existing_arena():
    from cenet_amd import optim
    m = _vec_module(70)
    m.q = torch.nn.Parameter(torch.ones(3))
    arena = optim.ParamArena(m)
    ptr = m.p.data_ptr()
    opt = optim.get_optimizer(m, _args(optimizer="adamw"))
    assert opt.arena is arena and m.p.data_ptr() == ptr


def test_get_optimizer_lays_cenet_out_by_segments():
    from cenet_amd import optim
    from cenet_amd.networks import CENet
    net = CENet(input_channels=1, num_classes=4, scale_factors=[1.0, 0.5], diffatt_num_heads=[4, 4, 4], out_up_block="upcn")
    opt = optim.get_optimizer(net, _args(optimizer="Adam"))
    assert [s[0] for s in opt.arena.segments] == [s[0] for s in optim.cenet_segments()]


def test_get_scheduler_dispatches_on_the_reference_strings():
    from cenet_amd import optim
    for name, cls in (("cosine", optim.CosineLR), ("Cosine", optim.CosineLR), ("poly", optim.PolyLR),
                      ("exp", optim.ExponentialLR), ("STEP", optim.StepLR), ("custom", optim.CustomLR)):
        opt = optim.get_optimizer(_vec_module(), _args(optimizer="adamw"))
        sch = optim.get_scheduler(opt, _args(scheduler=name), 100)
        assert type(sch) is cls, name
        assert sch.base_lr == 0.01 and sch.last_epoch == 0
    with pytest.raises(NotImplementedError, match="linear"):
        optim.get_scheduler(opt, _args(scheduler="linear"), 100)


def _toy(seed):
    torch.manual_seed(seed)
    m = torch.nn.Module()
    m.a = torch.nn.Parameter(torch.randn(5, 7))
    m.b = torch.nn.Parameter(torch.randn(13))
    m.register_buffer("r", torch.zeros(2))
    return m


@pytest.mark.parametrize("opt_name,sched", [("adamw", "cosine"), ("adam", "custom"), ("sgd", "exp"), ("adamw", "step")])
def test_resume_continues_bit_identically(sim, tmp_path, opt_name, sched):
    """3 steps, save_training_state, a fresh net / arena / optimizer / scheduler restored from the file, 3 steps == 6 steps in
    one run (host SIMT checker, injected gradients)"""
    from cenet_amd import checkpoint, optim
    g = torch.Generator().manual_seed(5)
    grads = [{"a": torch.randn(5, 7, generator=g), "b": torch.randn(13, generator=g)} for _ in range(6)]
    args = _args(optimizer=opt_name, base_lr=0.01, weight_decay=0.05, scheduler=sched, max_epochs=4)

    def make(seed):
        net = _toy(seed)
        opt = optim.get_optimizer(net, args)
        return net, opt, optim.get_scheduler(opt, args, 6)

    def step(net, opt, sch, i):
        opt.zero_grad()
        net.a.grad.copy_(grads[i]["a"])
        net.b.grad.copy_(grads[i]["b"])
        opt.step()
        sch.step()

    net, opt, sch = make(0)
    for i in range(6):
        step(net, opt, sch, i)
    net1, opt1, sch1 = make(0)
    for i in range(3):
        step(net1, opt1, sch1, i)
    p = str(tmp_path / "state.pth")
    checkpoint.save_training_state(p, net1, opt1, sch1)
    net2, opt2, sch2 = make(1)  # other initial weights: everything must come from the file
    checkpoint.load_training_state(p, net2, opt2, sch2)
    assert sch2.last_epoch == 3 and opt2._steps == 3
    for i in range(3, 6):
        step(net2, opt2, sch2, i)
    for n in ("a", "b"):
        assert torch.equal(getattr(net2, n).detach(), getattr(net, n).detach()), n
    assert opt2.lr == opt.lr and sch2.last_epoch == sch.last_epoch == 6


def test_training_state_of_another_kind_is_refused(tmp_path):
    from cenet_amd import checkpoint, optim
    net = _toy(0)
    opt = optim.get_optimizer(net, _args(optimizer="adamw"))
    p = str(tmp_path / "state.pth")
    checkpoint.save_training_state(p, net, opt, optim.CosineLR(opt, 10))
    net2 = _toy(0)
    opt2 = optim.get_optimizer(net2, _args(optimizer="adamw"))
    with pytest.raises(ValueError, match="cosine"):
        checkpoint.load_training_state(p, net2, opt2, optim.StepLR(opt2))
    with pytest.raises(ValueError, match="cosine"):
        checkpoint.load_training_state(p, net2, opt2, optim.PolyLR(opt2, 10))
    net3 = _toy(0)
    with pytest.raises(ValueError, match="adamw"):
        checkpoint.load_training_state(p, net3, optim.get_optimizer(net3, _args(optimizer="adam")))
