"""Golden vectors for the loss options of csrc/seg_loss_ex.hip: DiceLoss with class weights (softmax=True and softmax=False)
and JaccardLoss with ignored pixels.

Runs the reference's own `DiceLoss` / `JaccardLoss` (src/utils/core.py:44-80,134-158, loaded by path as
oracle.gen_golden.load_reference_losses does) with the reference's REAL `flatten` (src/utils/utils.py:39-50), which is loaded
at run time from utils/utils.py itself: that file imports plotting / profiling packages at its top that `flatten` does not
use, and the ones that are not installed are stood in for by empty modules while it loads.  (The one-argument stand-in of
oracle.gen_golden is enough for the optimizers and schedules, not for JaccardLoss, which calls flatten(input, target, ignore).)
The reference runs in float64 on the stored float32 inputs.  For K in {4, 9}, B = 2, 24 x 20, sharing one logits / labels pair
per K:
  K{K}.dice_w        DiceLoss(K)(logits, labels, weight=K{K}.weight, softmax=True)
  K{K}.dice_w_probs  DiceLoss(K)(probs, labels, weight=K{K}.weight, softmax=False) on probs = float32(softmax(float64(logits))), which is
                     not stored; gradient with respect to the probabilities
  K{K}.jac255        JaccardLoss(255, 1.0)(logits, K{K}.labels255): a block of rows and scattered pixels carry 255
  K{K}.jac0          JaccardLoss(0, 0.5)(logits, labels): class 0 is the ignored label
each with `.loss` (float64) and `.grad` (float32).  Writes tests/golden/loss_ex.npz.  Needs the reference sources; the tests read
only the .npz."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import OUT, REF_SRC  # noqa: E402

UNUSED_IMPORTS = ("thop", "ptflops", "fvcore", "fvcore.nn", "pandas", "matplotlib", "matplotlib.pyplot")


class _Absent(types.ModuleType):
    """stands in for a package utils/utils.py imports and `flatten` never touches: any name it is asked for is None"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def load_reference_core():
    """utils.core with utils.utils.flatten being the reference's own function"""
    added = []
    for name in UNUSED_IMPORTS:
        if name in sys.modules:
            continue
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = _Absent(name)
            added.append(name)
    pkg = types.ModuleType("utils")
    pkg.__path__ = [os.path.join(REF_SRC, "utils")]
    sys.modules["utils"] = pkg
    mods = {}
    try:
        for short in ("utils", "core"):
            spec = importlib.util.spec_from_file_location(f"utils.{short}", os.path.join(REF_SRC, "utils", f"{short}.py"))
            mods[short] = importlib.util.module_from_spec(spec)
            sys.modules[f"utils.{short}"] = mods[short]
            spec.loader.exec_module(mods[short])
    finally:
        for name in added:
            del sys.modules[name]
    assert mods["core"].flatten is mods["utils"].flatten and mods["utils"].flatten.__code__.co_argcount == 3
    return mods["core"]


def _run(fn, x32):
    x = x32.double().requires_grad_(True)
    loss = fn(x)
    loss.backward()
    return np.float64(loss.item()), x.grad.float().numpy()


def main():
    core = load_reference_core()
    rec = {}
    B, H, W = 2, 24, 20
    for K in (4, 9):
        g = torch.Generator().manual_seed(400 + K)
        logits = torch.randn(B, K, H, W, generator=g) * 2
        low = torch.rand(B, 1, 4, 5, generator=g)
        labels = torch.floor(torch.nn.functional.interpolate(low, size=(H, W), mode="nearest") * K).clamp_(0, K - 1)[:, 0]
        labels = labels.contiguous()
        weight = (0.2 + 2.8 * torch.rand(K, generator=g)).tolist()
        probs = torch.softmax(logits.double(), dim=1).float()
        labels255 = labels.clone()
        labels255[0, :5] = 255
        labels255[torch.rand(B, H, W, generator=g) < 0.1] = 255
        p = f"K{K}."
        rec[p + "logits"], rec[p + "labels"], rec[p + "labels255"] = logits.numpy(), labels.numpy().astype(np.uint8), \
            labels255.numpy().astype(np.uint8)
        rec[p + "weight"] = np.array(weight, dtype=np.float64)
        dice = core.DiceLoss(K)
        cases = {
            "dice_w": (lambda x: dice(x, labels, weight=weight, softmax=True), logits),
            "dice_w_probs": (lambda x: dice(x, labels, weight=weight, softmax=False), probs),
            "jac255": (lambda x: core.JaccardLoss(255, 1.0)(x, labels255), logits),
            "jac0": (lambda x: core.JaccardLoss(0, 0.5)(x, labels), logits),
        }
        for name, (fn, x) in cases.items():
            rec[p + name + ".loss"], rec[p + name + ".grad"] = _run(fn, x)
    path = os.path.join(OUT, "loss_ex.npz")
    np.savez_compressed(path, **rec)
    print("[golden] loss_ex", {k: float(v) for k, v in rec.items() if k.endswith(".loss")}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
