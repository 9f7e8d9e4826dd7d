"""The pair-attention kernels (attn_diff.hip) at the edges of their key loop: the loop runs the unmasked tile body over the full
32-key tiles and the masked body once, after it, on the ragged last tile.  Token counts on both sides of every edge: no full
tile (N < 32), no ragged tile (N % 32 == 0), one key past a tile, the last workgroup with a single active wave (the other waves
only stage, and must meet the same barriers), on every instance (HDP 16 / 32 / 48 / 64, the hd-4 pair rows, the single-softmax
form).  Each case goes through check_path of test_attention_bounds.py: fp64 reference, per-element bounds (c = 4, u = 2^-8) on the
forward, all three gradients and the LSE; on the host SIMT checker and, marked gpu, on the device.

`equal` and `large` are in the regime set for the softmax denominator: an exactly uniform softmax over N keys, and logits large
enough that the running maximum is rescaled in many tiles."""
import os

import pytest
import torch

from backend import dev  # noqa: F401
from cenet_amd import kern
from test_attention_bounds import check_path as _check_path

BF = torch.bfloat16


def check_path(monkeypatch, kind, *args, **kw):
    """check_path of test_attention_bounds.py, and the case must have run on attn_diff.hip: exactly one forward and one backward
    call through the pair entry point (kern.diffattn_heads) or the single-softmax one (kern.attn64), and an LSE held to its bound
    (check_path drops that check silently when the path hands none back).  Returns what the entry point saw per call:
    (backward, head dim, tokens, CENET_DATTN_HD40_HDP64 as the C side reads it at that moment)."""
    entry = "diffattn_heads" if kind == "diff" else "attn64"
    other = "attn64" if kind == "diff" else "diffattn_heads"
    calls, stray = [], []
    real = getattr(kern, entry)

    def spy(a, backward):
        calls.append((bool(backward), int(a.hd), int(a.N), os.environ.get("CENET_DATTN_HD40_HDP64")))
        return real(a, backward=backward)

    monkeypatch.setattr(kern, entry, spy)
    monkeypatch.setattr(kern, other, lambda *a_, **k_: stray.append(other))
    ratios = _check_path(kind, *args, **kw)
    assert [c[0] for c in calls] == [False, True], f"{entry} saw {calls}: the case did not run on the kernels of attn_diff.hip"
    assert not stray, stray
    assert "lse" in ratios, "no LSE came back from the attention path"
    return calls


REGIMES = ("staircase", "negative", "peaked", "equal", "large")

# (hd, N): pair kernels, N = Nq = Nk
PAIR = [(16, 31), (16, 32), (16, 33), (16, 64), (16, 95), (16, 160),
        (32, 33), (32, 64),
        (8, 33),
        (4, 33)]


def _bh(hd, N):
    # batch 1-2, heads 1-2: more than one (batch, pair) per launch, every case within seconds on the host checker
    return (2, 1) if N <= 64 else (1, 2) if hd <= 16 and N < 160 else (1, 1)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("hd,N", PAIR, ids=[f"hd{h}-N{n}" for h, n in PAIR])
def test_pair_kernels_at_tile_edges(dev, hd, N, regime, monkeypatch):
    B, H = _bh(hd, N)
    calls = check_path(monkeypatch, "diff", regime, B, H, N, N, hd, BF, dev)
    assert all(c[1:3] == (hd, N) for c in calls), calls


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("hdp64", [False, True], ids=["hdp48", "hdp64"])
@pytest.mark.parametrize("N", [33, 64])
def test_pair_hd40_both_instances_at_tile_edges(dev, N, hdp64, regime, monkeypatch):
    """hd 40 on the HDP = 48 instances and, with CENET_DATTN_HD40_HDP64 (read per call), on the HDP = 64 ones"""
    if hdp64:
        monkeypatch.setenv("CENET_DATTN_HD40_HDP64", "1")
    else:
        monkeypatch.delenv("CENET_DATTN_HD40_HDP64", raising=False)
    calls = check_path(monkeypatch, "diff", regime, 1, 1, N, N, 40, BF, dev)
    # the instance is chosen inside the library from the environment of each call: hd 40 went in, with the switch as set above
    assert all(c[1:] == (40, N, "1" if hdp64 else None) for c in calls), calls


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("joint", [False, True], ids=["split", "joint"])
@pytest.mark.parametrize("Cn,N", [(64, 256), (64, 257), (128, 256), (128, 287)])
def test_single_softmax_form_at_tile_edges(dev, Cn, N, joint, regime, monkeypatch):
    """the single-softmax form of the pair kernels through both Non-local entry points (N >= 256 is the smallest size on this
    path): no ragged tile, one key past a tile, 31 keys past a tile"""
    calls = check_path(monkeypatch, "nl", regime, 1, 1, N, N, Cn, BF, dev, joint=joint)
    assert all(c[1:3] == (Cn, N) for c in calls), calls
