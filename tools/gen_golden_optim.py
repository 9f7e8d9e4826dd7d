"""Golden vectors for the Adam / AdamW optimizers and the cosine / exp / step / custom LR schedules.

Imports the reference's own `get_optimizer` / `get_scheduler` (src/utils/core.py:12-41, through
oracle.gen_golden.load_reference_losses) and records
  * for each of 'cosine', 'exp', 'step', 'custom': the learning rate the train loop reads before each `scheduler.step()`
    (main_acdc.py:256-257), for a short setting and a long one (120 epochs x 96 iterations: ACDC's 1 902 training slices in
    batches of 20), so that the recursive schedules and StepLR's 200-iteration boundaries are exercised;
  * six steps of get_optimizer('adam') and get_optimizer('adamw'), each with get_scheduler('cosine'), on a 37-element parameter
    vector under a fixed gradient sequence that contains exact zeros (parameters after every step).
Writes tests/golden/optim_adam_sched.npz.  Needs the reference sources; the tests read only the .npz."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import OUT, load_reference_losses  # noqa: E402

SETTINGS = (("a", 0.05, 8, 5), ("b", 0.01, 120, 96))  # tag, base_lr, max_epochs, iterations per epoch
SCHEDULES = ("cosine", "exp", "step", "custom")


def main():
    core = load_reference_losses()
    rec = {}
    for tag, base_lr, max_epochs, per_epoch in SETTINGS:
        max_it = max_epochs * per_epoch
        rec[f"{tag}.base_lr"], rec[f"{tag}.max_epochs"], rec[f"{tag}.max_it"] = (np.float64(base_lr), np.int64(max_epochs),
                                                                                 np.int64(max_it))
        for sch_name in SCHEDULES:
            p = torch.nn.Parameter(torch.zeros(3))
            args = argparse.Namespace(optimizer="sgd", base_lr=base_lr, weight_decay=1e-4, scheduler=sch_name,
                                      max_epochs=max_epochs)
            opt = core.get_optimizer(torch.nn.ParameterList([p]), args)
            sch = core.get_scheduler(opt, args, max_it)
            lrs = []
            for _ in range(max_it):
                opt.step()
                lrs.append(float(sch.get_last_lr()[0]))  # main_acdc.py:256
                sch.step()                                # main_acdc.py:257
            rec[f"{tag}.{sch_name}"] = np.array(lrs, dtype=np.float64)
    g = torch.Generator().manual_seed(123)
    p0 = torch.randn(37, generator=g)
    grads = torch.randn(6, 37, generator=g)
    grads[:, 5] = 0.0       # a parameter that never receives a gradient
    grads[2, :] = 0.0       # a step without any gradient
    grads[::2, 11::7] = 0.0  # scattered zeros
    rec["traj.p0"], rec["traj.grads"] = p0.numpy(), grads.numpy()
    rec["traj.base_lr"], rec["traj.weight_decay"], rec["traj.max_it"] = np.float64(0.01), np.float64(0.05), np.int64(8)
    for name in ("adam", "adamw"):
        p = torch.nn.Parameter(p0.clone())
        args = argparse.Namespace(optimizer=name, base_lr=0.01, weight_decay=0.05, scheduler="cosine", max_epochs=8)
        opt = core.get_optimizer(torch.nn.ParameterList([p]), args)
        sch = core.get_scheduler(opt, args, 8)
        traj = []
        for i in range(6):
            opt.zero_grad()
            p.grad = grads[i].clone()
            opt.step()
            sch.step()
            traj.append(p.detach().clone().numpy())
        rec[f"traj.{name}"] = np.stack(traj)
    np.savez_compressed(os.path.join(OUT, "optim_adam_sched.npz"), **rec)
    print("[golden] optim_adam_sched", {k: rec[f"b.{k}"][-1] for k in SCHEDULES})


if __name__ == "__main__":
    main()
