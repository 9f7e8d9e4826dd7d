"""The distance-map losses inside cenet_amd.train.train_acdc: the captured step with `surface` and `hausdorff` in the loss equals
the eager loop, and a per-epoch weight schedule reaches the replayed graph through the device buffer without a recapture.
Network, toy dataset and loaders are those of tests/test_train_loop.py.  That the capture succeeds at all is the check that
nothing in the maps or the loss synchronises."""
import copy

import numpy as np
import pytest
import torch

from backend import use_hip
from test_train_loop import _net, _Toy


@pytest.mark.gpu
def test_schedule_reaches_the_replayed_graph_and_the_replayed_loop_equals_the_eager_loop():
    from cenet_amd import train
    dev = use_hip()
    loader = torch.utils.data.DataLoader(_Toy(14, seed=21), batch_size=4, shuffle=False)  # 3 full batches + a ragged one of 2
    ref_net = _net(dev)
    schedule = lambda e: (0.05 * (e + 1), 0.001 * (e + 1))  # noqa: E731

    def run(graph, sched):
        return train.train_acdc(copy.deepcopy(ref_net), loader, max_epochs=2, base_lr=0.01, device=dev, graph=graph, log_every=1,
                                log=lambda s: None, loss_type="dice,ce,surface,hausdorff", loss_weights="0.5,0.5,0.05,0.001",
                                dist_weight_schedule=sched)

    he, hg, hn = run(False, schedule), run(True, schedule), run(True, None)
    le, lg, ln = (np.array([v for _, v in h["loss"]]) for h in (he, hg, hn))
    print("eager", le, "replayed", lg, "no schedule", ln)
    assert len(le) == len(lg) == len(ln) == 8 and he["lr"] == hg["lr"]
    assert (np.abs(le - lg) < 2e-4 * np.maximum(1.0, np.abs(le))).all(), (le, lg)
    # epoch 1 runs at the weights of loss_weights either way; in epoch 2 the schedule has doubled the two distance weights
    assert (np.abs(lg[:4] - ln[:4]) < 2e-4 * np.maximum(1.0, np.abs(ln[:4]))).all(), (lg, ln)
    # (a difference of ten times what the two loops may differ by is no rounding)
    assert (np.abs(lg[4:] - ln[4:]) > 2e-3 * np.maximum(1.0, np.abs(ln[4:]))).all(), (lg, ln)
    # one captured graph, eight iterations counted by the optimizer
    assert hg["optimizer"]._steps == 8 and he["optimizer"]._steps == 8
