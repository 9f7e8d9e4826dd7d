"""The top-k cross-entropy inside cenet_amd.train.train_acdc: the captured step with `topk` in the loss equals the eager loop and
differs from the step without it, and a schedule of the percentage reaches the replayed graph without a recapture.  Network, toy
dataset and loaders are those of tests/test_train_loop.py.  That the capture succeeds at all is the check that nothing in the
select, the tie rank or the weights synchronises or reads back."""
import copy

import numpy as np
import pytest
import torch

from backend import use_hip
from test_train_loop import _net, _Toy


@pytest.mark.gpu
def test_the_replayed_loop_with_topk_equals_the_eager_loop():
    from cenet_amd import train
    from cenet_amd import graph as G
    dev = use_hip()
    loader = torch.utils.data.DataLoader(_Toy(14, seed=21), batch_size=4, shuffle=False)  # 3 full batches + a ragged one of 2
    ref_net = _net(dev)
    captures = []
    real_init = G.GraphedStep.__init__

    def counting_init(self, *a, **k):
        captures.append(1)
        real_init(self, *a, **k)

    def run(graph, loss_type, loss_weights, **kw):
        return train.train_acdc(copy.deepcopy(ref_net), loader, max_epochs=2, base_lr=0.01, device=dev, graph=graph, log_every=1,
                                log=lambda s: None, loss_type=loss_type, loss_weights=loss_weights, **kw)

    he, hg = (run(g, "dice,ce,topk", "0.5,0.5,0.5") for g in (False, True))
    hn = run(True, "dice,ce", "0.5,0.5")
    le, lg, ln = (np.array([v for _, v in h["loss"]]) for h in (he, hg, hn))
    print("eager", le, "replayed", lg, "without topk", ln)
    assert len(le) == len(lg) == len(ln) == 8 and he["lr"] == hg["lr"]
    bound = 2e-4 * np.maximum(1.0, np.abs(le))
    assert (np.abs(le - lg) < bound).all(), (le, lg)
    # (a difference of ten times what the two loops may differ by is no rounding)
    assert (np.abs(lg - ln) > 10 * bound).all(), (lg, ln)
    assert hg["optimizer"]._steps == 8 and he["optimizer"]._steps == 8

    # 100 % in the first epoch, 10 % in the second: the same losses replayed as eager, from ONE captured graph
    schedule = lambda epoch: (100.0, 10.0)[epoch]  # noqa: E731
    se = run(False, "dice,ce,topk", "0.5,0.5,0.5", topk_schedule=schedule)
    G.GraphedStep.__init__ = counting_init
    try:
        sg = run(True, "dice,ce,topk", "0.5,0.5,0.5", topk_schedule=schedule)
    finally:
        G.GraphedStep.__init__ = real_init
    me, mg = (np.array([v for _, v in h["loss"]]) for h in (se, sg))
    print("schedule: eager", me, "replayed", mg)
    assert len(me) == len(mg) == 8
    assert (np.abs(me - mg) < 2e-4 * np.maximum(1.0, np.abs(me))).all(), (me, mg)
    assert len(captures) == 1 and sg["optimizer"]._steps == 8 and se["optimizer"]._steps == 8
    # (the schedule does something: the first epoch, all pixels kept, is not the constant-percentage run's)
    assert (np.abs(mg[:4] - lg[:4]) > 10 * bound[:4]).all(), (mg, lg)
    with pytest.raises(ValueError, match="topk_schedule"):
        run(True, "dice,ce", "0.5,0.5", topk_schedule=schedule)
