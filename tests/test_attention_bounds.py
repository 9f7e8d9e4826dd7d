"""Every attention path of the product held to a float64 reference with PER-ELEMENT bounds (tests/attn_ref.py):
|got - ref| <= c u M + floor, where M is the magnitude the formula itself produces at that element (P|V| for the output, ...).
bf16 paths: u = 2^-8, c = 4; fp32 (parity) paths: u = 2^-24 (sqrt(Nk) + max|scale s|), c = 16.  (The logit term of the fp32 unit:
an fp32 score, the stored fp32 LSE and the hardware exp each carry an absolute error of ~|scale s| 2^-24 in the logit, which is
that relative error in P; at logits of 160 it is 11x the sqrt(Nk) term of a 196-key problem.  In bf16 it is far below 2^-8.)

Measured on the MI355X, max over the cases of each path of (|err| - floor) / (u M) over O, dQ, dK, dV and the LSE:
    path                      c   randn  peaked  staircase  negative  equal  large
    pair kernels bf16         4   0.72   1.68    1.66       1.07      0.17   1.46
    single-softmax pair bf16  4   0.58   -       1.33       0.54      -      1.31
    tiled bf16                4   0.89   1.48    1.55       1.00      0.24   1.29
    SRA resident bf16         4   1.08   1.67    1.48       1.42      -      1.77
    SRA key blocks bf16       4   0.60   -       1.43       0.79      0.12   -
    materialised bf16         4   1.22   2.41    2.27       1.46      -      1.85
    tiled fp32               16   0.87   1.57    1.94       2.77      0.67   2.82
    materialised fp32        16   0.93   -       1.89       2.74      -      7.04

Part 1 (CPU only, no kernel): the bound itself is tested.  fp64 emulations of plausible kernel bugs (a padded key in the ragged
key tile, the last key dropped, a missed rescale of the accumulators, a query tile off by 5 %, dK / dV of softmax head 1 built
with head 0's P, delta over half the value columns) must be REJECTED on the input regime built to expose each one; an honest
emulation (fp64 with P, dS and the outputs rounded to bf16) must PASS on every regime.

Part 2: the product's kernels, forward and all three input gradients (and the LSE where the entry point writes one), in the
regimes of attn_ref.make_inputs: `sim` runs small shapes on the host SIMT checker, `hip` (marker gpu) runs them and the
production shapes (benched batch 32 / 24: every (batch, head) is checked) on the MI355X.

Part 3: the fp32 parity mode on overflowing scores (multihead_diffattn.py:95,106, torch.nan_to_num of the scores) in both
directions, on the tiled kernels (hd 16) and the materialised path (hd 80), against the reference formula under autograd."""
import json
import math
import os

import pytest
import torch

import attn_ref as R
from backend import dev  # noqa: F401
from cenet_amd import ops

BF, F32 = torch.bfloat16, torch.float32
gpu = pytest.mark.gpu


def _log(what, ratios):
    # CENET_BOUNDS_LOG=<file>: append the measured max |err| / (u M) of every check (the table of the PR / DESIGN numbers)
    path = os.environ.get("CENET_BOUNDS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": what, **{k: round(v, 4) for k, v in ratios.items()}}) + "\n")


# =====================================================================================================================
# part 1: mutation self-test of the bound (fp64 emulation, CPU)
# =====================================================================================================================
def _rb(x):
    """round to bf16 and back (the honest kernel's storage rounding)"""
    return x.to(BF).double()


def emulate(q, k, v, dO, scale, group, bug=None):
    """a bf16 pair kernel in fp64: online softmax over 32-key tiles (P rounded to bf16 before PV, O stored bf16), backward from
    the LSE (dS rounded to bf16, gradients stored bf16); `bug` plants one plausible kernel bug."""
    q, k, v, dO = (t.double() for t in (q, k, v, dO))
    B, Hq, Nq, D = q.shape
    Nk, Dv = k.shape[2], v.shape[3]
    T = R.TILE
    nt = (Nk + T - 1) // T
    pad = nt * T - Nk
    kp = torch.cat([k, k.new_zeros(B, Hq, pad, D)], 2)
    vx = v[:, torch.arange(Hq) // group]
    vp = torch.cat([vx, vx.new_zeros(B, Hq, pad, Dv)], 2)
    valid = torch.arange(nt * T) < Nk
    if bug == "pad_key":
        valid = torch.arange(nt * T) >= 0  # the padded keys (k = 0: score 0) enter the softmax
    if bug == "drop_last":
        valid = torch.arange(nt * T) < Nk - 1
    m = torch.full((B, Hq, Nq, 1), -math.inf, dtype=torch.float64)
    l = torch.zeros_like(m)
    acc = torch.zeros(B, Hq, Nq, Dv, dtype=torch.float64)
    for t in range(nt):
        sl = slice(T * t, T * t + T)
        S = scale * q @ kp[:, :, sl].transpose(-1, -2)
        S = S.masked_fill(~valid[sl], -math.inf)
        mnew = torch.maximum(m, S.amax(-1, keepdim=True))
        alpha = torch.exp(m - mnew)
        p = torch.exp(S - mnew)
        l = l * alpha + p.sum(-1, keepdim=True)
        if bug == "no_rescale" and t >= 1:
            pass  # the running max rose in a late tile but the accumulators keep their old scale
        elif bug == "no_rescale_half" and t >= 1:
            acc = torch.cat([acc[..., :32], acc[..., 32:] * alpha], -1)  # only the second 32-column half is rescaled
        else:
            acc = acc * alpha
        acc = acc + _rb(p) @ vp[:, :, sl]
        m = mnew
    O = acc / l
    lse = (m + torch.log(l))[..., 0]
    if bug == "tile_off":
        last = (Nq - 1) // T * T
        O[:, :, last:] *= 1.05
    O = _rb(O)
    # backward
    S = scale * q @ kp.transpose(-1, -2)
    P = torch.exp(S - lse[..., None]).masked_fill(~valid, 0.0)
    dP = dO @ vp.transpose(-1, -2)
    delta = (dO[..., : Dv // 2] * O[..., : Dv // 2] if bug == "half_delta" else dO * O).sum(-1, keepdim=True)
    dS = _rb(P * (dP - delta))
    Pb = _rb(P)
    if bug == "wrong_head_p":  # softmax head s = 1 of each pair takes head 0's P for dK / dV
        Pk = Pb.clone()
        Pk[:, 1::2] = Pb[:, 0::2]
        dSk = _rb(Pk * (dP - delta))
    else:
        Pk, dSk = Pb, dS
    dQ = _rb(scale * dS @ kp)
    dK = _rb(scale * dSk.transpose(-1, -2) @ q)[:, :, :Nk]
    dVh = (Pk.transpose(-1, -2) @ dO)[:, :, :Nk]
    dV = _rb(dVh.view(B, Hq // group, group, Nk, Dv).sum(2))
    return {"O": O, "dQ": dQ, "dK": dK, "dV": dV, "lse": lse}


# (bug, regime that exposes it, N, hd): differential pairs, one value head (group 2)
MUTANTS = [
    ("pad_key", "negative", 70, 16),
    ("drop_last", "staircase", 100, 16),
    ("no_rescale", "staircase", 100, 16),
    ("no_rescale_half", "staircase", 100, 32),
    ("tile_off", "peaked", 70, 16),
    ("wrong_head_p", "peaked", 70, 16),
    ("half_delta", "randn", 70, 16),
]


def _emul_case(regime, N, hd, bug, seed=3):
    scale = hd ** -0.5
    q, k, v, dO = (t.to(BF).double() for t in R.make_inputs(regime, 1, 2, N, N, hd, 2 * hd, scale, group=2, seed=seed))
    ref = R.reference(q, k, v, scale, dO, group=2)
    return emulate(q, k, v, dO, scale, 2, bug), ref


@pytest.mark.parametrize("bug,regime,N,hd", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_bound_rejects_mutant(bug, regime, N, hd):
    got, ref = _emul_case(regime, N, hd, bug)
    with pytest.raises(AssertionError, match="outside"):
        R.check_all(got, ref, R.C_BF16, R.U_BF16, f"mutant {bug}")


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("N,hd", [(70, 16), (100, 32), (20, 8)])
def test_bound_accepts_honest_bf16_emulation(regime, N, hd):
    got, ref = _emul_case(regime, N, hd, None)
    r = R.check_all(got, ref, R.C_BF16, R.U_BF16, f"honest {regime}")
    r["lse"] = R.assert_within(got["lse"], ref.lse, ref.M_lse, R.C_BF16, R.U_BF16, what="honest lse")
    _log(f"emulation honest N{N} hd{hd} {regime}", r)


def test_failure_report_names_the_tile():
    got, ref = _emul_case("peaked", 70, 16, "tile_off")
    with pytest.raises(AssertionError, match=r"row tile 2 of 3 \(the ragged last tile\)"):
        R.assert_within(got["O"], ref.O, ref.M_O, R.C_BF16, R.U_BF16, what="O")


# =====================================================================================================================
# part 2: the product's kernels
# =====================================================================================================================
def run_diff(q, k, v, dO, H):
    """ops.diff_attention_heads on canonical q, k [B, 2H, N, hd], v [B, H, N, 2hd]"""
    B, Hq, N, hd = q.shape
    qp, kp = (t.transpose(1, 2).reshape(B, N, Hq * hd).contiguous().requires_grad_(True) for t in (q, k))
    vp = v.transpose(1, 2).reshape(B, N, H * 2 * hd).contiguous().requires_grad_(True)
    U = ops.diff_attention_heads(qp, kp, vp, H)
    ctx = U.grad_fn
    lse = ctx.saved_tensors[4] if (getattr(ctx, "pairs", False) or getattr(ctx, "kind", None) == "flash") else None
    U.backward(dO.contiguous())
    return {"O": U, "dQ": qp.grad.view(B, N, Hq, hd).transpose(1, 2), "dK": kp.grad.view(B, N, Hq, hd).transpose(1, 2),
            "dV": vp.grad.view(B, N, H, 2 * hd).transpose(1, 2)}, lse


def run_sra(q, k, v, dO, H):
    """ops.sr_attention on canonical q [B, H, Nq, 64], k / v [B, H, Nk, 64] (kv packed as [k | v])"""
    B, _, N, hd = q.shape
    Nk, Cn = k.shape[2], H * hd
    qp = q.transpose(1, 2).reshape(B, N, Cn).contiguous().requires_grad_(True)
    kvp = torch.cat([k.transpose(1, 2).reshape(B, Nk, Cn), v.transpose(1, 2).reshape(B, Nk, Cn)], -1).contiguous()
    kvp.requires_grad_(True)
    o = ops.sr_attention(qp, kvp, H)
    ctx = o.grad_fn
    lse = ctx.saved_tensors[3] if ctx.kind == "flash" else None
    o.backward(dO.transpose(1, 2).reshape(B, N, Cn).contiguous())
    dkv = kvp.grad

    def canon(t, n):
        return t.reshape(B, n, H, hd).transpose(1, 2)

    return {"O": canon(o, N), "dQ": canon(qp.grad, N), "dK": canon(dkv[..., :Cn], Nk), "dV": canon(dkv[..., Cn:], Nk)}, lse


def run_nonlocal(q, k, v, dO, joint=False):
    """ops.nonlocal_attention (or the joint form) on canonical [B, 1, N, C]: theta | phi | g channel-major [B, C, N]"""
    th, ph, gx = (t[:, 0].transpose(1, 2).contiguous() for t in (q, k, v))
    go = dO[:, 0].transpose(1, 2).contiguous()
    if joint:
        tpg = torch.cat([th, ph, gx], 1).requires_grad_(True)
        y = ops.nonlocal_attention_joint(tpg)
        ctx = y.grad_fn
        lse = ctx.saved_tensors[2] if ctx.tok64 else (ctx.saved_tensors[2] if ctx.kind == "flash" else None)
        y.backward(go)
        C = th.shape[1]
        grads = [tpg.grad[:, i * C:(i + 1) * C] for i in range(3)]
    else:
        ins = [t.requires_grad_(True) for t in (th, ph, gx)]
        y = ops.nonlocal_attention(*ins)
        ctx = y.grad_fn
        lse = ctx.saved_tensors[4] if (ctx.tok64 or ctx.kind == "flash") else None
        y.backward(go)
        grads = [t.grad for t in ins]

    def canon(t):
        return t.transpose(1, 2)[:, None]

    return {"O": canon(y), "dQ": canon(grads[0]), "dK": canon(grads[1]), "dV": canon(grads[2])}, lse


def check_path(kind, regime, B, H, Nq, Nk, hd, dtype, device, seed=0, joint=False):
    """one case: inputs of `regime`, rounded to dtype; the kernel's O / dQ / dK / dV (and LSE) against the fp64 reference"""
    if kind == "diff":
        Hq, Dv, group, scale = 2 * H, 2 * hd, 2, hd ** -0.5
    else:
        Hq, Dv, group, scale = H, hd, 1, hd ** -0.5
    q, k, v, dO = (t.to(dtype).to(device) for t in R.make_inputs(regime, B, Hq, Nq, Nk, hd, Dv, scale, group, seed))
    ref = R.reference(q, k, v, scale, dO, group)
    if kind == "diff":
        got, lse = run_diff(q, k, v, dO, H)
    elif kind == "sra":
        got, lse = run_sra(q, k, v, dO, H)
    else:
        got, lse = run_nonlocal(q, k, v, dO, joint)
    if dtype == BF:
        c, u = R.C_BF16, R.U_BF16
        assert got["O"].dtype == BF
    else:
        c, u = R.C_FP32, R.u_fp32(Nk, ref.logit_max)
        assert got["O"].dtype == F32
    what = f"{kind}{'-joint' if joint else ''} {str(dtype)[6:]} B{B} H{H} Nq{Nq} Nk{Nk} hd{hd} {regime}"
    ratios = R.check_all(got, ref, c, u, what)
    if lse is not None:
        ratios["lse"] = R.assert_within(lse, ref.lse, ref.M_lse, c, u, what=f"{what} lse")
    _log(what, ratios)
    return ratios


# ---- host SIMT checker and GPU: small shapes ------------------------------------------------------------------------------
# (kind, B, H, Nq, Nk, hd, dtype, regimes)
ALL = R.REGIMES
SMALL = [
    # pair kernels (attn_diff.hip), every head dim; N < 32 and ragged N
    ("diff", 2, 1, 70, 70, 16, BF, ALL),
    ("diff", 1, 2, 20, 20, 8, BF, ("randn", "staircase", "negative")),
    ("diff", 1, 2, 49, 49, 4, BF, ("peaked", "staircase", "negative")),
    ("diff", 1, 1, 100, 100, 32, BF, ("randn", "staircase", "negative", "large")),
    ("diff", 1, 1, 49, 49, 40, BF, ("peaked", "staircase")),
    ("diff", 1, 1, 70, 70, 64, BF, ("randn", "staircase", "negative")),
    # bf16 tiled kernels (attn_bf16.hip): head dims outside the pair set
    ("diff", 1, 1, 70, 70, 10, BF, ("randn", "staircase", "negative", "large")),
    ("diff", 1, 1, 100, 100, 20, BF, ("peaked", "equal")),
    # fp32 tiled kernels (attn.hip, parity mode: finite_scores on)
    ("diff", 1, 1, 70, 70, 16, F32, ALL),
    ("diff", 1, 1, 49, 49, 64, F32, ("randn", "staircase", "negative")),
    ("diff", 1, 2, 20, 20, 4, F32, ("peaked", "negative")),
    # materialised path (head dim > 64): score GEMM, softmax_rows_*, fp32 and bf16 (atomic=2 score GEMM)
    ("diff", 1, 1, 49, 49, 80, F32, ("randn", "staircase", "negative", "large")),
    ("diff", 1, 1, 49, 49, 80, BF, ("randn", "staircase", "negative", "large")),
    # spatial-reduction attention: resident forward + fused backward (49 keys), key blocks (65..256), > 256 keys (tiled)
    ("sra", 2, 2, 100, 49, 64, BF, ("randn", "staircase", "negative")),
    ("sra", 1, 1, 300, 49, 64, BF, ("peaked", "staircase")),
    ("sra", 1, 1, 97, 150, 64, BF, ("randn", "staircase", "negative")),
    ("sra", 1, 1, 40, 300, 64, BF, ("randn", "negative")),
    ("sra", 1, 2, 100, 49, 64, F32, ("randn", "staircase", "large")),
    # Non-local: materialised (C > 64), fp32 tiled (C <= 64)
    ("nl", 2, 1, 49, 49, 96, BF, ("randn", "staircase", "negative")),
    ("nl", 1, 1, 49, 49, 96, F32, ("randn", "negative")),
    ("nl", 1, 1, 49, 49, 32, F32, ("randn", "staircase")),
]
SMALL_CASES = [pytest.param(c[:7] + (r,), id=f"{c[0]}-{str(c[6])[6:]}-B{c[1]}H{c[2]}-{c[3]}x{c[4]}-hd{c[5]}-{r}")
               for c in SMALL for r in c[7]]


@pytest.mark.parametrize("case", SMALL_CASES)
def test_small_shapes_within_bound(dev, case):
    kind, B, H, Nq, Nk, hd, dtype, regime = case
    check_path(kind, regime, B, H, Nq, Nk, hd, dtype, dev)


@pytest.mark.parametrize("regime", ("randn", "staircase", "negative"))
def test_pair_hd40_hdp64_instances(dev, regime, monkeypatch):
    """hd 40 on the HDP = 64 instances (CENET_DATTN_HD40_HDP64 is read per call) as well as the default HDP = 48"""
    monkeypatch.setenv("CENET_DATTN_HD40_HDP64", "1")
    check_path("diff", regime, 1, 1, 70, 70, 40, BF, dev)


@pytest.mark.parametrize("regime", ("randn", "staircase"))
def test_nonlocal_joint_materialised(dev, regime):
    check_path("nl", regime, 1, 1, 49, 49, 96, BF, dev, joint=True)


# ---- GPU: production shapes -----------------------------------------------------------------------------------------------
GPU_REGIMES = ("randn", "peaked", "staircase", "negative", "large")
# (kind, B, H, Nq, Nk, hd, dtype, regimes); ACDC batch 32, Synapse batch 24
PROD = [
    # ACDC DSEB1 / DSEB2 (pair kernels), DSEB3 (hd 80, materialised)
    ("diff", 32, 4, 3136, 3136, 16, BF, GPU_REGIMES),
    ("diff", 32, 4, 784, 784, 32, BF, GPU_REGIMES),
    ("diff", 32, 4, 196, 196, 80, BF, GPU_REGIMES),
    # Synapse DSEB1 / DSEB2 / DSEB3
    ("diff", 24, 16, 3136, 3136, 8, BF, ("randn", "staircase", "negative")),
    ("diff", 24, 8, 784, 784, 16, BF, ("randn", "staircase", "negative")),
    ("diff", 24, 8, 196, 196, 20, BF, ("randn", "staircase", "negative")),
    ("diff", 24, 4, 196, 196, 40, BF, ("randn", "staircase", "negative")),
    # skip_mode='add' head dims; HAM levels; >= 1024 tokens; the 64-query form (hd 64) at 4096
    ("diff", 8, 4, 3136, 3136, 4, BF, ("randn", "staircase", "negative")),
    ("diff", 2, 2, 784, 784, 64, BF, ("randn", "staircase", "negative", "large")),
    ("diff", 2, 2, 4096, 4096, 64, BF, ("randn", "staircase")),
    ("diff", 4, 2, 1024, 1024, 32, BF, ("randn", "staircase", "negative")),
    ("diff", 2, 2, 196, 196, 160, BF, ("randn", "staircase", "negative")),
    ("diff", 2, 2, 1024, 1024, 160, BF, ("randn", "staircase")),
    ("diff", 4, 2, 3136, 3136, 10, BF, ("randn", "staircase", "negative")),
    # fp32 parity mode: tiled kernels at every head-dim class, the materialised path
    ("diff", 4, 4, 784, 784, 16, F32, GPU_REGIMES),
    ("diff", 2, 2, 196, 196, 32, F32, ("randn", "staircase", "negative")),
    ("diff", 2, 2, 196, 196, 64, F32, ("randn", "staircase", "negative")),
    ("diff", 2, 2, 196, 196, 80, F32, ("randn", "staircase", "negative", "large")),
    ("diff", 2, 2, 1024, 1024, 160, F32, ("randn", "staircase")),
    # spatial-reduction attention at batch 32: 1 / 2 / 5 / 8 heads at 3136 / 784 / 196 / 49 queries (sra_tiles > 1)
    ("sra", 32, 1, 3136, 49, 64, BF, GPU_REGIMES),
    ("sra", 32, 2, 784, 49, 64, BF, GPU_REGIMES),
    ("sra", 32, 5, 196, 49, 64, BF, ("randn", "staircase", "negative")),
    ("sra", 32, 8, 49, 49, 64, BF, ("randn", "staircase", "negative")),
    ("sra", 2, 1, 4096, 256, 64, BF, ("randn", "staircase", "negative")),
    ("sra", 2, 1, 1024, 300, 64, BF, ("randn", "staircase")),
    ("sra", 4, 2, 1024, 49, 64, F32, ("randn", "staircase", "negative")),  # query-sliced dK / dV (few keys)
    # Non-local: the single-softmax pair form (C = 64 @ 3136, 128 @ 784) and the materialised path at 14^2 / 7^2
    ("nl", 32, 1, 3136, 3136, 64, BF, ("randn", "staircase", "negative")),
    ("nl", 32, 1, 784, 784, 128, BF, ("randn", "staircase", "negative", "large")),
    ("nl", 32, 1, 196, 196, 320, BF, ("randn", "staircase")),
    ("nl", 32, 1, 49, 49, 512, BF, ("randn", "negative")),
    ("nl", 4, 1, 196, 196, 320, F32, ("randn", "staircase")),
]
PROD_CASES = [pytest.param(c[:7] + (r,), id=f"{c[0]}-{str(c[6])[6:]}-B{c[1]}H{c[2]}-{c[3]}x{c[4]}-hd{c[5]}-{r}")
              for c in PROD for r in c[7]]


@gpu
@pytest.mark.parametrize("case", PROD_CASES)
def test_production_shapes_within_bound(case):
    from backend import use_hip
    device = use_hip()
    kind, B, H, Nq, Nk, hd, dtype, regime = case
    check_path(kind, regime, B, H, Nq, Nk, hd, dtype, device)


@gpu
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("Cn,N", [(64, 3136), (128, 784)])
def test_nonlocal_single_softmax_pair_form(Cn, N, joint):
    """kern.attn64 (the single-softmax form of the pair kernels) through both Non-local entry points"""
    from backend import use_hip
    device = use_hip()
    for regime in ("randn", "staircase", "negative"):
        check_path("nl", regime, 8, 1, N, N, Cn, BF, device, joint=joint)


@gpu
def test_all_equal_softmax_over_16k_keys():
    """q = 0: an exactly uniform softmax over 16 384 keys (the tiled bf16 kernels: hd 20; the pair kernels: hd 16)"""
    from backend import use_hip
    device = use_hip()
    check_path("diff", "equal", 1, 1, 16384, 16384, 16, BF, device)
    check_path("diff", "equal", 1, 1, 16384, 16384, 20, BF, device)
    check_path("sra", "equal", 1, 1, 16384, 256, 64, BF, device)


# =====================================================================================================================
# part 3: fp32 parity mode on overflowing scores
# =====================================================================================================================
def _reference_diffattn_core(q, k, v, H, scale):
    """multihead_diffattn.py:95-109 restated: q scaled first, scores through torch.nan_to_num, softmax, shared value head"""
    B, N, E = q.shape
    hd = E // H // 2
    q = q * scale
    qh = q.view(B, N, 2 * H, hd).transpose(1, 2)
    kh = k.view(B, N, 2 * H, hd).transpose(1, 2)
    vh = v.view(B, N, H, 2 * hd).transpose(1, 2).repeat_interleave(2, dim=1)
    s = torch.nan_to_num(qh @ kh.transpose(-1, -2))
    return torch.softmax(s, dim=-1) @ vh


@pytest.mark.parametrize("hd", [16, 80])
def test_parity_mode_overflowing_scores_both_directions(dev, hd):
    """scores that overflow fp32 (+-inf) in some rows while the reference's output and gradients stay finite: the tiled kernels
    (hd 16) and the materialised path (hd 80) clamp the scores like nan_to_num and give them zero gradient"""
    B, H, N = 1, 1, 40
    E = 2 * H * hd
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B, N, E, generator=g) for _ in range(3))
    # feature 0 of softmax head 0: query 3 at 4e36 (finite after q *= scale), keys 17 / 21 at +-400, every other token 0 there.
    # Row 3 then has the scores +inf (key 17) and -inf (key 21): nan_to_num makes them +-FLT_MAX, the row is one-hot and its
    # gradient zero; the other rows stay ordinary.
    q[0, :, 0] = 0.0
    k[0, :, 0] = 0.0
    q[0, 3, 0] = 4e36
    k[0, 17, 0] = 400.0
    k[0, 21, 0] = -400.0
    dO = torch.randn(B, 2 * H, N, 2 * hd, generator=g)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = _reference_diffattn_core(qr, kr, vr, H, hd ** -0.5)
    assert torch.isfinite(ref).all()
    ref.backward(dO)
    for t in (qr, kr, vr):
        assert torch.isfinite(t.grad).all()
    qs, ks, vs = (t.clone().to(dev).requires_grad_(True) for t in (q, k, v))
    out = ops.diff_attention_heads(qs, ks, vs, H)
    out.backward(dO.to(dev))
    got = [out, qs.grad, ks.grad, vs.grad]
    for name, a, b in zip(("out", "dq", "dk", "dv"), got, (ref, qr.grad, kr.grad, vr.grad)):
        a = a.detach().cpu()
        assert torch.isfinite(a).all(), name
        b = b.detach()
        torch.testing.assert_close(a, b, rtol=1e-3, atol=2e-4 * max(1.0, float(b.abs().max())), msg=name)
