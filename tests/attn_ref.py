"""Attention reference for the bound tests (tests/test_attention_bounds.py): float64 evaluation, per-element error magnitudes,
the element-wise bound, and input regimes that expose the ways attention kernels go wrong.  Plain helper module: no fixtures.

Every attention form of the product is written in one canonical layout:
    q [B, Hq, Nq, D], k [B, Hq, Nk, D], v [B, Hq // group, Nk, Dv];   softmax head h reads value head h // group
    O[b, h] = softmax(scale q k^T) v[b, h // group]                    ([B, Hq, Nq, Dv]), lse = natural-log LSE ([B, Hq, Nq])
group = 2: differential attention (multihead_diffattn.py:83-109, two softmax heads share one value head); group = 1: single
softmax, spatial-reduction attention with a packed kv (pvtv2.py:88-109), channel-major Non-local (nlb.py:117-138).  The tests map
the product's layouts onto this one.

Magnitudes.  The same formulas re-evaluated with every operand replaced by its absolute value and every subtraction turned into an
addition bound what rounding can do to each element (P = softmax(scale q k^T), delta = rowsum(dO o O)):
    M_O = P |V|      M_dS = P o (|dO| |V|^T + rowsum(|dO| o |O|))      M_dV = P^T |dO|  (summed over the softmax heads of a group)
    M_dQ = scale M_dS |K|      M_dK = scale M_dS^T |Q|      M_lse = 1 + rowsum(P o |scale q k^T|)
A kernel that rounds its operands / outputs to a unit u stays within a small multiple of u M of the exact result; a kernel that
mixes up an index, drops a key or forgets a rescale does not (tests/test_attention_bounds.py, mutation self-test)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

U_BF16 = 2.0 ** -8
C_BF16 = 4.0
C_FP32 = 16.0
TILE = 32  # rows of the tiles the failure report names (the pair kernels' query / key tiles)


def u_fp32(Nk: int, logit_max: float = 0.0) -> float:
    """unit of the fp32 paths: 2^-24 per accumulated term (sqrt(Nk) of them), plus the absolute rounding of a logit of size
    logit_max (fp32 scores, the stored fp32 LSE and a hardware exp see |scale s| 2^-24 of absolute error, i.e. that relative
    error in every probability)"""
    return 2.0 ** -24 * (math.sqrt(Nk) + logit_max)


def _chunks(n_bh, Nq, Nk, budget=1 << 25):
    step = max(1, budget // max(1, Nq * Nk))
    for s in range(0, n_bh, step):
        yield s, min(n_bh, s + step)


def reference(q, k, v, scale, dO=None, group=1):
    """float64 attention on the tensors' device, per (batch, head) chunk.  Returns a namespace with O, lse, M_O, M_lse,
    logit_max and, given dO, dQ / dK / dV with M_dQ / M_dK / M_dV (all float64, canonical layout)."""
    B, Hq, Nq, D = q.shape
    Nk, Dv = k.shape[2], v.shape[3]
    Hv = v.shape[1]
    assert Hq == Hv * group and k.shape == (B, Hq, Nk, D) and v.shape == (B, Hv, Nk, Dv)
    dev = q.device
    q64, k64 = q.double().reshape(B * Hq, Nq, D), k.double().reshape(B * Hq, Nk, D)
    vh = torch.arange(Hq, device=dev) // group
    v64 = v.double()[:, vh].reshape(B * Hq, Nk, Dv)
    g64 = dO.double().reshape(B * Hq, Nq, Dv) if dO is not None else None
    O = torch.empty(B * Hq, Nq, Dv, dtype=torch.float64, device=dev)
    MO, lse = torch.empty_like(O), torch.empty(B * Hq, Nq, dtype=torch.float64, device=dev)
    Mlse = torch.empty_like(lse)
    logit_max = 0.0
    if dO is not None:
        dQ, MdQ = torch.empty_like(q64), torch.empty_like(q64)
        dK, MdK = torch.empty_like(k64), torch.empty_like(k64)
        dVh, MdVh = torch.empty_like(v64), torch.empty_like(v64)
    for s, e in _chunks(B * Hq, Nq, Nk):
        qc, kc, vc = q64[s:e], k64[s:e], v64[s:e]
        S = scale * (qc @ kc.transpose(1, 2))
        logit_max = max(logit_max, float(S.abs().max()))
        L = torch.logsumexp(S, dim=-1)
        P = torch.exp(S - L[..., None])
        O[s:e] = P @ vc
        MO[s:e] = P @ vc.abs()
        lse[s:e] = L
        Mlse[s:e] = 1.0 + (P * S.abs()).sum(-1)
        if dO is None:
            continue
        gc = g64[s:e]
        delta = (gc * O[s:e]).sum(-1, keepdim=True)
        dS = P * (gc @ vc.transpose(1, 2) - delta)
        MdS = P * (gc.abs() @ vc.abs().transpose(1, 2) + (gc.abs() * O[s:e].abs()).sum(-1, keepdim=True))
        dQ[s:e] = scale * (dS @ kc)
        MdQ[s:e] = scale * (MdS @ kc.abs())
        dK[s:e] = scale * (dS.transpose(1, 2) @ qc)
        MdK[s:e] = scale * (MdS.transpose(1, 2) @ qc.abs())
        dVh[s:e] = P.transpose(1, 2) @ gc
        MdVh[s:e] = P.transpose(1, 2) @ gc.abs()
    r = SimpleNamespace(O=O.view(B, Hq, Nq, Dv), M_O=MO.view(B, Hq, Nq, Dv), lse=lse.view(B, Hq, Nq),
                        M_lse=Mlse.view(B, Hq, Nq), logit_max=logit_max)
    if dO is not None:
        r.dQ, r.M_dQ = dQ.view(B, Hq, Nq, D), MdQ.view(B, Hq, Nq, D)
        r.dK, r.M_dK = dK.view(B, Hq, Nk, D), MdK.view(B, Hq, Nk, D)
        # the softmax heads of a group add into their shared value head
        r.dV = dVh.view(B, Hv, group, Nk, Dv).sum(2)
        r.M_dV = MdVh.view(B, Hv, group, Nk, Dv).sum(2)
    return r


def assert_within(got, ref, M, c, u, floor=None, what=""):
    """|got - ref| <= c u M + floor element-wise (floor = 1e-3 u max(M) unless given).  got / ref / M: [B, H, rows(, cols)].
    Returns the measured max (|err| - floor) / (u M): the smallest c that passes.  On failure names the worst element as (batch, head,
    row, column), its 32-row tile and whether that tile is the ragged last one."""
    got = got.detach().to(ref.device, torch.float64)
    ref, M = ref.to(torch.float64), M.to(torch.float64)
    assert got.shape == ref.shape == M.shape, (what, tuple(got.shape), tuple(ref.shape), tuple(M.shape))
    if got.dim() == 3:
        got, ref, M = got[..., None], ref[..., None], M[..., None]
    mmax = float(M.max()) if M.numel() else 0.0
    if floor is None:
        floor = 1e-3 * u * mmax
    assert floor <= 1e-3 * u * mmax + 1e-300, f"{what}: floor {floor} above 1e-3 u max(M)"
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf))
    bound = c * u * M + floor
    ratio = err / (u * M).clamp_min(1e-300)
    # measured: the c this element needs once the floor has taken its share
    need = (err - floor).clamp_min(0.0) / (u * M).clamp_min(1e-300)
    measured = float(need[M > 0].max()) if bool((M > 0).any()) else 0.0
    bad = err > bound
    if bool(bad.any()):
        excess = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        flat = int(torch.argmax(excess.flatten()))
        B, H, R, Cc = got.shape
        b, rem = divmod(flat, H * R * Cc)
        h, rem = divmod(rem, R * Cc)
        row, col = divmod(rem, Cc)
        tile, ntile = row // TILE, (R + TILE - 1) // TILE
        ragged = R % TILE != 0 and tile == ntile - 1
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside |err| <= {c} u M + floor (u = {u:.3g}); worst at "
            f"(batch {b}, head {h}, row {row}, column {col}), row tile {tile} of {ntile}{' (the ragged last tile)' if ragged else ''}: "
            f"got {float(got[b, h, row, col]):.6g}, reference {float(ref[b, h, row, col]):.6g}, |err| / (u M) = "
            f"{float(ratio[b, h, row, col]):.3g}, M = {float(M[b, h, row, col]):.3g}")
    return measured


# ---- input regimes ----------------------------------------------------------------------------------------------------------
REGIMES = ("randn", "peaked", "staircase", "negative", "equal", "large")


def _unit(D, g, dev):
    e = torch.randn(D, generator=g)
    return (e / e.norm()).to(dev)


def make_inputs(regime, B, Hq, Nq, Nk, D, Dv, scale, group=1, seed=0, device="cpu"):
    """canonical fp32 q [B, Hq, Nq, D], k [B, Hq, Nk, D], v [B, Hq // group, Nk, Dv], dO [B, Hq, Nq, Dv]:
      randn      every element N(0, 1)
      peaked     q x 6: score standard deviation >= 6
      staircase  query i's dominant key sits in the first key tile, a late one or the ragged last one (i mod 3): the running
                 maximum rises late, and in only some lanes of a wave
      negative   k along -q: every real score <= -20, so a padded or masked key that leaks in (score 0) dominates
      equal      q = 0: an exactly uniform softmax
      large      q, k along one direction: |scale s| up to ~160 (anything that skips the max subtraction overflows)"""
    g = torch.Generator().manual_seed(seed)
    Hv = Hq // group

    def rn(*s):
        return torch.randn(*s, generator=g)

    v, dO = rn(B, Hv, Nk, Dv), rn(B, Hq, Nq, Dv)
    if regime == "randn":
        q, k = rn(B, Hq, Nq, D), rn(B, Hq, Nk, D)
    elif regime == "peaked":
        q, k = 6.0 * rn(B, Hq, Nq, D), rn(B, Hq, Nk, D)
    elif regime == "equal":
        q, k = torch.zeros(B, Hq, Nq, D), rn(B, Hq, Nk, D)
    elif regime == "staircase":
        k = 0.5 * rn(B, Hq, Nk, D)
        nt = (Nk + TILE - 1) // TILE
        i = torch.arange(Nq)
        first = i % min(TILE, Nk)
        late = TILE * max(nt - 2, 0) + i % min(TILE, Nk - TILE * max(nt - 2, 0))
        last_len = Nk - TILE * (nt - 1)
        last = Nk - 1 - i % last_len
        tgt = torch.where(i % 3 == 0, first, torch.where(i % 3 == 1, late, last))
        hot = torch.zeros(Nk, dtype=torch.bool)
        hot[tgt] = True
        k[:, :, hot] *= 3.0
        kt = k[:, :, tgt]  # [B, Hq, Nq, D]
        # scale q_i . k_t = 12 for the target key
        q = 12.0 * kt / (scale * (kt * kt).sum(-1, keepdim=True).clamp_min(1e-6)) + 0.05 * rn(B, Hq, Nq, D)
    elif regime == "negative":
        e = _unit(D, g, "cpu")
        alpha = math.sqrt(25.0 / scale)
        a = alpha * (1.0 + 0.5 * torch.rand(B, Hq, Nq, 1, generator=g))
        b = alpha * (1.0 + 0.5 * torch.rand(B, Hq, Nk, 1, generator=g))
        noise = 0.02 * math.sqrt(1.0 / scale)
        q = a * e + noise * rn(B, Hq, Nq, D)
        k = -b * e + noise * rn(B, Hq, Nk, D)
    elif regime == "large":
        e = _unit(D, g, "cpu")
        alpha = math.sqrt(160.0 / scale)
        a = alpha * (0.5 + 0.5 * torch.rand(B, Hq, Nq, 1, generator=g))
        b = alpha * (2.0 * torch.rand(B, Hq, Nk, 1, generator=g) - 1.0)
        q = a * e + 0.1 * rn(B, Hq, Nq, D)
        k = b * e + 0.1 * rn(B, Hq, Nk, D)
    else:
        raise ValueError(regime)
    return tuple(t.to(device) for t in (q, k, v, dO))


def check_all(got, ref, c, u, what, keys=("O", "dQ", "dK", "dV")):
    """assert_within on each named tensor of `got` (a dict) against `ref`; returns {name: measured ratio}"""
    out = {}
    for n in keys:
        if n in got:
            out[n] = assert_within(got[n], getattr(ref, n), getattr(ref, "M_" + n), c, u, what=f"{what} {n}")
    return out
