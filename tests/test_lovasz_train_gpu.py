"""The Lovasz-Softmax loss inside cenet_amd.train.train_acdc: the captured step with `lovasz` in the loss equals the eager loop and
differs from the step without it.  Network, toy dataset and loaders are those of tests/test_train_loop.py.  That the capture
succeeds at all is the check that nothing in the sort, the ranks or the coefficients synchronises or reads back."""
import copy

import numpy as np
import pytest
import torch

from backend import use_hip
from test_train_loop import _net, _Toy


@pytest.mark.gpu
def test_the_replayed_loop_with_lovasz_equals_the_eager_loop():
    from cenet_amd import train
    dev = use_hip()
    loader = torch.utils.data.DataLoader(_Toy(14, seed=21), batch_size=4, shuffle=False)  # 3 full batches + a ragged one of 2
    ref_net = _net(dev)

    def run(graph, loss_type, loss_weights):
        return train.train_acdc(copy.deepcopy(ref_net), loader, max_epochs=2, base_lr=0.01, device=dev, graph=graph, log_every=1,
                                log=lambda s: None, loss_type=loss_type, loss_weights=loss_weights)

    he, hg = (run(g, "dice,ce,lovasz", "0.5,0.5,0.5") for g in (False, True))
    hn = run(True, "dice,ce", "0.5,0.5")
    le, lg, ln = (np.array([v for _, v in h["loss"]]) for h in (he, hg, hn))
    print("eager", le, "replayed", lg, "without lovasz", ln)
    assert len(le) == len(lg) == len(ln) == 8 and he["lr"] == hg["lr"]
    bound = 2e-4 * np.maximum(1.0, np.abs(le))
    assert (np.abs(le - lg) < bound).all(), (le, lg)
    # (a difference of ten times what the two loops may differ by is no rounding)
    assert (np.abs(lg - ln) > 10 * bound).all(), (lg, ln)
    # one captured graph, eight iterations counted by the optimizer
    assert hg["optimizer"]._steps == 8 and he["optimizer"]._steps == 8
