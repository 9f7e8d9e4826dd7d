"""bench.py --dump-outputs: what the last timed step computed, as float32 .npy files that the runs of two builds compare by."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from test_bench_dist import _last_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_large_arrays_at_fixed_positions(tmp_path):
    big = torch.randn(bench.DUMP_CAP + 1000, generator=torch.Generator().manual_seed(3))
    small = torch.randn(2, 3, dtype=torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_CAP,) and np.array_equal(a, b)
    assert np.isin(a, big.numpy()).all()  # a sample of the array's elements, not a transformation of them
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.float().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["replay", "eager", "segmented"])
def test_bench_dump_outputs_are_the_last_timed_step(form, tmp_path):
    """The dumped logits are the ones the dumped loss was computed from (a replayed graph: the capture's static output, rewritten
    by every replay; eager: the last forward), the loss is the one the result line reports, and the parameters and gradients are
    the arena's.  fp32 mode, so that the oracle's criterion on the dumped logits must agree to the last few bits: logits of
    another step (new drop-path draws, updated weights) would miss by far more.  `segmented` is an N > 1 launch form, run with a
    one-rank RCCL group as in tests/test_bench_dist.py."""
    d = tmp_path / "out"
    args = ["--batch", "2", "--steps", "3", "--warmup", "1", "--dtype", "f32", "--no-cpu-baseline", "--no-roofline",
            "--dump-outputs", str(d)]
    if form == "segmented":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
               "127.0.0.1", "--master-port", "29655", "bench.py", "--gpus", "1", "--dist-launch", "segmented"]
        env = dict(os.environ, CENET_FORCE_DIST="1")
    else:
        cmd, env = [sys.executable, "bench.py", "--graph", "on" if form == "replay" else "off"], None
    p = subprocess.run(cmd + args, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    r = _last_json(p.stdout)
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    want = {"replay": "hipGraph replay", "eager": "eager", "segmented": "six hipGraphs"}[form]
    assert r["config"]["launch"].startswith(want), r["config"]["launch"]
    out = {f.stem: np.load(f) for f in d.iterdir()}
    assert set(out) == {"loss", "logits", "params", "grads"} and all(v.dtype == np.float32 for v in out.values())
    assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
    assert out["logits"].shape == (2, 4, 224, 224) and out["params"].shape == out["grads"].shape
    assert abs(float(out["loss"]) - r["config"]["final_loss"]) < 1e-5
    from oracle import cenet_oracle as O
    _, lab = bench.synthetic(2, "cpu", seed=1234)
    ref = O.criterion(torch.from_numpy(out["logits"]), lab, 4).item()
    assert abs(ref - float(out["loss"])) < 1e-4, (ref, float(out["loss"]))
    assert np.isfinite(out["params"]).all() and np.isfinite(out["grads"]).all() and np.abs(out["grads"]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_bench_dump_outputs_repeat_with_the_same_arguments(dtype, tmp_path):
    """Two runs with the same arguments dump the same outputs up to rounding: the last timed step starts from the restored
    start state, so the float-atomic reductions of the earlier steps cannot carry their run-to-run last bits into it.  What
    remains is the dumped step's own reduction order: none in the fp32 forward (logits bit-identical), the split-K
    forward GEMMs of the bf16 mode (a flipped bf16 rounding here and there, a few bf16 ulps on the logits)."""
    extra = ["--graph", "on"] if dtype == "bf16" else ["--dtype", "f32"]
    out = []
    for run in ("a", "b"):
        d = tmp_path / run
        p = subprocess.run([sys.executable, "bench.py", "--steps", "4", "--warmup", "2", "--no-cpu-baseline", "--no-f32",
                            "--no-roofline", "--dump-outputs", str(d)] + extra,
                           cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        out.append({f.stem: np.load(f).astype(np.float64) for f in d.iterdir()})
    a, b = out
    assert set(a) == set(b) == {"loss", "logits", "params", "grads"}
    scale = {k: np.abs(v).max() for k, v in a.items()}
    diff = {k: np.abs(a[k] - b[k]).max() for k in a}
    assert diff["loss"] <= 1e-5 * scale["loss"], diff
    assert diff["params"] <= 1e-6 * scale["params"], diff
    assert diff["grads"] <= 2e-3 * scale["grads"], diff
    if dtype == "f32":
        assert diff["logits"] == 0.0, diff
    else:
        assert diff["logits"] <= 3e-2 * scale["logits"], diff
