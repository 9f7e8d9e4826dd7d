"""optim.FusedAdam / FusedAdamW (csrc/adam.hip): one fused launch per step over the parameter arena with torch.optim.Adam /
AdamW arithmetic — against the reference's own get_optimizer('adam' / 'adamw') + get_scheduler('cosine')
(tests/golden/optim_adam_sched.npz, tools/gen_golden_optim.py) and against live torch.optim on odd parameter sizes; grad_scale,
the bf16 shadow, param_groups edits, state_dict round trips and refusals.  Host SIMT checker on CPU, the HIP library with
-m gpu."""
import argparse
import os

import numpy as np
import pytest
import torch

from backend import dev  # noqa: F401  (fixture: host SIMT checker on CPU, the HIP library with -m gpu)
from conftest import GOLDEN


def _golden():
    return np.load(os.path.join(GOLDEN, "optim_adam_sched.npz"))


@pytest.mark.parametrize("name", ["adam", "adamw"])
def test_fused_trajectory_matches_the_reference(dev, name):
    """six steps with the cosine schedule, gradients with exact zeros (a parameter that never gets one, a step without any)"""
    from cenet_amd import optim
    z = _golden()
    m = torch.nn.Module()
    m.p = torch.nn.Parameter(torch.from_numpy(z["traj.p0"]).clone().to(dev))
    args = argparse.Namespace(optimizer=name, base_lr=float(z["traj.base_lr"]), weight_decay=float(z["traj.weight_decay"]),
                              scheduler="cosine", max_epochs=8)
    opt = optim.get_optimizer(m, args)
    assert type(opt) is (optim.FusedAdamW if name == "adamw" else optim.FusedAdam)
    sch = optim.get_scheduler(opt, args, int(z["traj.max_it"]))
    grads = torch.from_numpy(z["traj.grads"]).to(dev)
    for i in range(6):
        opt.zero_grad()
        m.p.grad.copy_(grads[i])
        opt.step()
        sch.step()
        np.testing.assert_allclose(m.p.detach().cpu().numpy(), z[f"traj.{name}"][i], rtol=2e-6, atol=2e-7)
    assert opt._steps == 6


def _odd_module(dev, seed=0):
    torch.manual_seed(seed)
    m = torch.nn.Module()
    m.w = torch.nn.Parameter(torch.randn(3, 5))
    m.b = torch.nn.Parameter(torch.randn(7))
    m.s = torch.nn.Parameter(torch.randn(1))
    m.k = torch.nn.Parameter(torch.randn(2, 3, 11))
    m.e = torch.nn.Parameter(torch.randn(67))
    return m.to(dev)


def _grads(m, steps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [{n: torch.randn(p.shape, generator=g) for n, p in m.named_parameters()} for _ in range(steps)]


def _inject(m, gs, scale=1.0):
    for n, p in m.named_parameters():
        p.grad.copy_(gs[n].to(p.device) * scale)


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_odd_sizes_match_live_torch(dev, decoupled):
    """five parameters of odd sizes (arena padding between them) against torch.optim.Adam / AdamW on the same gradients,
    with the lr changed between steps"""
    from cenet_amd import optim
    m, ref = _odd_module(dev), _odd_module(dev)
    arena = optim.ParamArena(m)
    assert arena.numel > sum(p.numel() for p in m.parameters())  # padding present
    cls, tcls = (optim.FusedAdamW, torch.optim.AdamW) if decoupled else (optim.FusedAdam, torch.optim.Adam)
    opt = cls(arena, lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
    topt = tcls(ref.parameters(), lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
    for i, gs in enumerate(_grads(m, 5)):
        lr = 0.01 * (1 - i / 6)
        opt.param_groups[0]["lr"] = lr
        for g in topt.param_groups:
            g["lr"] = lr
        opt.zero_grad()
        _inject(m, gs)
        opt.step()
        topt.zero_grad()
        for n, p in ref.named_parameters():
            p.grad = gs[n].to(dev).clone()
        topt.step()
        for (n, p), q in zip(m.named_parameters(), ref.parameters()):
            np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=2e-6, atol=2e-7, err_msg=n)
    for n, q in ref.named_parameters():  # (the moments to a few ulps of their largest terms: lerp cancels)
        o, k = arena.index[n]
        st = topt.state[q]
        np.testing.assert_allclose(opt.exp_avg[o:o + k].cpu().numpy(), st["exp_avg"].reshape(-1).cpu().numpy(), rtol=2e-6,
                                   atol=1e-7)
        np.testing.assert_allclose(opt.exp_avg_sq[o:o + k].cpu().numpy(), st["exp_avg_sq"].reshape(-1).cpu().numpy(),
                                   rtol=2e-6, atol=1e-8)


def test_grad_scale_folds_into_the_step(dev):
    """grad_scale = 0.5 on 2 g is the unscaled step on g (GradReducer's 1/world), bit for bit"""
    from cenet_amd import optim
    m1, m2 = _odd_module(dev), _odd_module(dev)
    o1 = optim.FusedAdamW(optim.ParamArena(m1), lr=0.01, weight_decay=0.1)
    o2 = optim.FusedAdamW(optim.ParamArena(m2), lr=0.01, weight_decay=0.1, grad_scale=0.5)
    for gs in _grads(m1, 3):
        for m, o, s in ((m1, o1, 1.0), (m2, o2, 2.0)):
            o.zero_grad()
            _inject(m, gs, s)
            o.step()
    assert torch.equal(o1.arena.params, o2.arena.params)
    assert torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_shadow_is_bf16_of_the_params_after_every_step(dev, decoupled):
    from cenet_amd import optim
    m = _odd_module(dev)
    arena = optim.ParamArena(m)
    arena.enable_shadow()
    opt = (optim.FusedAdamW if decoupled else optim.FusedAdam)(arena, lr=0.01, weight_decay=0.1)
    for gs in _grads(m, 3):
        opt.zero_grad()
        _inject(m, gs)
        opt.step()
        want = arena.params.to(torch.bfloat16)
        assert torch.equal(arena.shadow.view(torch.int16), want.view(torch.int16))


def test_param_groups_edits_take_effect(dev):
    """lr / betas / eps / weight_decay set through param_groups[0] after construction == the same values given at construction"""
    from cenet_amd import optim
    m1, m2 = _odd_module(dev), _odd_module(dev)
    o1 = optim.FusedAdam(optim.ParamArena(m1), lr=0.02, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.3)
    o2 = optim.FusedAdam(optim.ParamArena(m2))
    assert o2.param_groups is o2.param_groups
    for g in o2.param_groups:
        g.update(lr=0.02, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.3)
    for gs in _grads(m1, 3):
        for m, o in ((m1, o1), (m2, o2)):
            o.zero_grad()
            _inject(m, gs)
            o.step()
    assert torch.equal(o1.arena.params, o2.arena.params)
    o3 = optim.FusedAdam(optim.ParamArena(_odd_module(dev)), lr=0.02, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.3)
    assert not torch.equal(o3.arena.params, o1.arena.params)  # (the steps did move the parameters)


def test_state_dict_round_trip_into_another_layout(dev):
    """state saved after 2 steps, loaded into an arena whose segments order the parameters differently: the next 2 steps are
    bit-identical to the uninterrupted run"""
    from cenet_amd import optim
    gs = _grads(_odd_module(dev), 4)
    m1 = _odd_module(dev)
    o1 = optim.FusedAdamW(optim.ParamArena(m1), lr=0.01, weight_decay=0.1)
    for i in range(2):
        o1.zero_grad()
        _inject(m1, gs[i])
        o1.step()
    sd = o1.state_dict()
    assert set(sd) == {"kind", "exp_avg", "exp_avg_sq", "steps", "lr"} and sd["kind"] == "adamw" and sd["steps"] == 2
    m2 = _odd_module(dev, seed=9)
    with torch.no_grad():
        for (_, p), (_, q) in zip(m2.named_parameters(), m1.named_parameters()):
            p.copy_(q)
    a2 = optim.ParamArena(m2, [("tail", lambda n: n in ("e", "s")), ("rest", lambda n: True)])
    assert a2.index["e"][0] != o1.arena.index["e"][0]
    o2 = optim.FusedAdamW(a2, lr=0.5, weight_decay=0.1)
    o2.load_state_dict(sd)
    assert o2._steps == 2 and o2.lr == 0.01
    for i in range(2, 4):
        for m, o in ((m1, o1), (m2, o2)):
            o.zero_grad()
            _inject(m, gs[i])
            o.step()
    for (n, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n


def test_cross_kind_state_and_unsupported_options_are_refused():
    from cenet_amd import optim
    mk = lambda: optim.ParamArena(_odd_module("cpu"))  # noqa: E731
    sgd, adam, adamw = optim.FusedSGD(mk(), lr=0.1), optim.FusedAdam(mk()), optim.FusedAdamW(mk())
    with pytest.raises(ValueError, match="sgd"):
        adamw.load_state_dict(sgd.state_dict())
    with pytest.raises(ValueError, match="adamw"):
        adam.load_state_dict(adamw.state_dict())
    with pytest.raises(ValueError, match="adam"):
        adamw.load_state_dict(adam.state_dict())
    with pytest.raises(ValueError):
        sgd.load_state_dict(adamw.state_dict())
    for kw in ({"amsgrad": True}, {"maximize": True}, {"capturable": True}, {"differentiable": True}, {"foreach": True},
               {"fused": True}, {"lr": -1.0}, {"betas": (1.0, 0.999)}, {"eps": -1e-8}):
        for cls in (optim.FusedAdam, optim.FusedAdamW):
            with pytest.raises(ValueError):
                cls(mk(), **kw)
