"""Reference for the convolutions that do not go through the GEMM (conv_direct.hip, conv_c1.hip, dwconv.hip), for
tests/test_conv_bounds.py: float64 evaluations of what include/cenet_hip.h says each entry point means, the per-element magnitude
that goes with each, and the two acceptance rules of tests/gemm_ref.py (whose `round_once`, `ints`, `reals`, `bound_of`, constants
and `_act64` are imported, not copied).  Plain helper module: no fixtures.  Written from the header text, not from the kernels.

Operands are passed as strided VIEWS (`view()`) of the buffers the kernel is given, so batch strides, lead offsets and padded planes
are honoured by construction; a formula returns (value, Mag) over the logical output, Mag being the same formula with every operand
replaced by its absolute value, and `expect()` scatters them through the index map of the destination into the WHOLE destination
buffer: elements the call does not own keep their previous value ("ADDED into": previous + value, Mag + |previous|).

    conv (conv_direct, conv_c1)   y[b,o,y,x]  = sum_{i,ky,kx} w[o,i,ky,kx] x[b,i,y+ky-p,x+kx-p]          p = k/2, zero outside
    conv_direct dgrad = 1         dX[b,o,y,x] = sum_{i,ky,kx} w[i,o,ky,kx] dY[b,i,y-ky+p,x-kx+p]         w: the forward weight
    weight gradient               dw[o,i,ky,kx] += sum_{b,y,x} dY[b,o,y,x] x[b,i,y+ky-p,x+kx-p]
    pw_small                      y[b,jG+o,p] = sum_i W[j][o][i] x[b,jG+i,p]        (transpose: W[j][i][o])
    pw_fewout                     y[b,o,p] = bias[o] + sum_i W[o,i] x[b,i,p];  dx[b,i,p] = sum_o W[o,i] dy[b,o,p];
                                  dW[o,i] += sum_{b,p} dy[b,o,p] x[b,i,p];  dbias[o] += sum_{b,p} dy[b,o,p]
    depthwise (NCHW and tokens)   y[b,c,y,x] = bias[c] + sum_{ky,kx} w[c, flip ? 8-t : t] x[b,c,y+(ky-1)dil,x+(kx-1)dil], t = 3ky+kx;
                                  a = act(y);  dw[c,t] += sum dy[b,c,y,x] x[b,c,y+(ky-1)dil,x+(kx-1)dil];  dbias[c] += sum dy
    tok_bwd_pre                   gu = g act'(conv(x) + bias);  dw, dbias from gu as above

Weight precision (what the kernels do with the fp32 master weight; the reference takes `wq="bf16"` where the kernel rounds once):
    conv_direct fwd / dgrad       rounded to bf16 once per workgroup (MFMA operand)
    conv_c1 stencils (fwd)        fp32 weights
    conv_c1 forward, MFMA form    rounded to bf16 once (k = 5 and W % 16 == 0): the SAME op uses bf16 or fp32 weights depending on
                                  W % 16 -- recorded as a finding in DESIGN.md, not a failure
    pw_small / pw_fewout          the caller passes the bf16 shadow of the weight; widened exactly, fp32 products
    depthwise                     fp32 weights and bias
The test matrix feeds bf16-exact weights (both regimes), where the forms agree; `wq` is exercised by one conv_direct case.

Acceptance rules: the two regimes of gemm_ref.
  EXACT  operands, bias, previous accumulator contents and cotangents are integers in [-4, 4], activations none / relu / lrelu with
         slope 1/4, max Mag < 2^24 (asserted): the output equals the float64 result rounded once; no tolerance; everything outside
         the footprint is unchanged bit for bit.
  BOUND  bf16-rounded normals (and a run with a common +1 offset):
             |y - ref| <= C_OUT u_out |ref| + L_act C_ACC 2^-24 sqrt(K_tot) Mag
         K_tot = terms of one output (Cin k^2; 9; B H W for a weight gradient), u_out = 2^-8 (bf16 store) or 2^-24 (fp32).

Constants: measured on the HOST, never on the kernels.  `measure_constants()` evaluates the conv shapes of the case matrix in plain
fp32 on the CPU (one fp32 partial sum per tap, the taps -- and for weight gradients the images -- added in a shuffled order)
against float64, in both operand regimes:
    accumulation: largest |y32 - ref| / (2^-24 sqrt(K_tot) Mag)                 measured 0.484  -> x 4 = 1.94 < 2.3: C_ACC stays 2.3
    store:        largest (|bf16(y32) - ref| - |y32 - ref|) / (2^-8 |ref|)      measured 0.9959 -> C_OUT stays 1.0
    gelu' sensitivity: largest |gelu'(z + d) - gelu'(z)| / |d| in float64       measured 0.7979 (= 2 phi(0)) -> L_DGELU = 0.8
(the values are the module constants below, pinned by test_conv_constants_are_the_host_measurement).  L_DGELU is the Lipschitz
factor of g gelu'(z) in z per unit |g|: an error e in the recomputed pre-activation moves gu by at most |g| L_DGELU e, and e is
bounded by the accumulation term (whose C_ACC already carries the factor 4 for summation order).
These constants are not widened to make a kernel pass: a kernel that needs more is a finding."""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from gemm_ref import (ACT_LIPSCHITZ, BF, C_ACC, C_OUT, EXACT_LIMIT, U_BF16, U_FP32, _act64, bound_of, ints, reals,  # noqa: F401
                      round_once)

MEASURED_ACC, MEASURED_OUT, MEASURED_DGELU = 0.484, 0.9959, 0.7979  # measure_constants() over the case matrix (pinned by a test)
L_DGELU = 0.8  # measured 0.7979, rounded up


# ---- views and the whole-buffer expectation ----------------------------------------------------------------------------------
def view(buf, off, shape, strides):
    """logical tensor `shape` at element offset `off` of the flat buffer `buf` with element strides `strides`"""
    return buf.as_strided(tuple(shape), tuple(strides), buf.storage_offset() + off)


def index_map(off, shape, strides, device):
    """flat buffer address of every logical element"""
    idx = torch.full((), off, dtype=torch.int64, device=device)
    for d, (n, s) in enumerate(zip(shape, strides)):
        sh = [1] * len(shape)
        sh[d] = n
        idx = idx + (torch.arange(n, device=device, dtype=torch.int64) * s).view(sh)
    return idx.expand(tuple(shape))


def expect(buf, off, shape, strides, val, mag, K_tot, *, add=False, lip=1.0, dims=("image", "channel", "y", "x"), tile=None,
           kernel=""):
    """What a call must leave in the flat destination `buf`, given its contents NOW: `val` / `mag` (float64, logical `shape`) at
    offset / strides; add: "ADDED into".  tile = (th, tw): the kernel's output tile over the last two dims, for the failure report."""
    flat = buf.reshape(-1)
    idx = index_map(off, shape, strides, flat.device)
    C, Mag = flat.double().clone(), torch.zeros(flat.numel(), dtype=torch.float64, device=flat.device)
    own = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
    fi = idx.reshape(-1)
    if add:
        prev = C[fi]
        C[fi], Mag[fi] = prev + val.reshape(-1), prev.abs() + mag.reshape(-1)
    else:
        C[fi], Mag[fi] = val.reshape(-1), mag.reshape(-1)
    own[fi] = True
    return SimpleNamespace(C=C, Mag=Mag, own=own, prev_raw=flat.clone(), idx=idx, out_dtype=flat.dtype,
                           u_out=U_BF16 if flat.dtype == BF else U_FP32, K_tot=K_tot, lip=lip, dims=dims, tile=tile, kernel=kernel)


def _locate(exp, flat, what):
    hit = (exp.idx == flat).nonzero()
    if not len(hit):
        return f"{what} [{exp.kernel}]: buffer element {flat} (outside the call's footprint)"
    pos = tuple(int(v) for v in hit[0])
    s = f"{what} [{exp.kernel}]: output (" + ", ".join(f"{n} {p}" for n, p in zip(exp.dims, pos)) + ")"
    if exp.tile is not None and len(pos) >= 2:
        th, tw = exp.tile
        s += f", {th} x {tw} tile ({pos[-2] // th}, {pos[-1] // tw}), row {pos[-2] % th} column {pos[-1] % tw} of it"
    return s


def _outside(got, exp, what):
    bits = torch.int16 if got.element_size() == 2 else torch.int32
    out = ~exp.own & (got.view(bits) != exp.prev_raw.view(bits))
    if bool(out.any()):
        flat = int(out.nonzero()[0])
        raise AssertionError(f"{what} [{exp.kernel}]: buffer element {flat} outside the footprint changed: {float(got[flat])!r} "
                             f"(was {float(exp.prev_raw[flat])!r}); {int(out.sum())} such elements")


def assert_exact(got, exp, what=""):
    """every own element equals the float64 expectation rounded once; everything else is unchanged bit for bit"""
    got = got.reshape(-1)
    assert float(exp.Mag.max()) < EXACT_LIMIT, f"{what}: magnitude {float(exp.Mag.max())} is outside the exact regime"
    _outside(got, exp, what)
    want = round_once(torch.where(exp.own, exp.C, torch.zeros_like(exp.C)), exp.out_dtype)
    bad = exp.own & ~((got == want) & torch.isfinite(got))
    if bool(bad.any()):
        flat = int(bad.nonzero()[0])
        raise AssertionError(f"{_locate(exp, flat, what)}: got {float(got[flat])!r}, expected {float(want[flat])!r}; "
                             f"{int(bad.sum())} of {int(exp.own.sum())} outputs wrong")


def assert_bound(got, exp, what=""):
    """|got - ref| <= C_OUT u_out |ref| + lip C_ACC 2^-24 sqrt(K_tot) Mag on the own elements; the rest unchanged.  Returns the
    worst |err| / bound."""
    got = got.reshape(-1)
    _outside(got, exp, what)
    g64 = got.double()
    err = (g64 - exp.C).abs()
    err = torch.where(torch.isfinite(g64), err, torch.full_like(err, math.inf))
    bound = bound_of(exp.C, exp.Mag, exp.u_out, exp.K_tot, c_acc=C_ACC * exp.lip)
    ratio = torch.where(exp.own, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max())
    if worst > 1.0:
        flat = int(torch.argmax(ratio))
        raise AssertionError(f"{_locate(exp, flat, what)}: got {float(got[flat]):.9g}, reference {float(exp.C[flat]):.9g}, |err| = "
                             f"{float(err[flat]):.3g} = {worst:.3g} x bound (u_out = {exp.u_out:.3g}, K_tot = {exp.K_tot}, Mag = "
                             f"{float(exp.Mag[flat]):.3g}); {int((ratio > 1).sum())} of {int(exp.own.sum())} outputs outside")
    return worst


# ---- formulas ------------------------------------------------------------------------------------------------------------------
def _shift(x, dy, dx):
    """z[..., y, x] = x[..., y + dy, x + dx], zero outside the image"""
    H, W = x.shape[-2:]
    z = torch.zeros_like(x)
    ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        z[..., ys:ye, xs:xe] = x[..., ys + dy:ye + dy, xs + dx:xe + dx]
    return z


def _wq(w, wq):
    w = w.detach()
    return (w.float().to(BF) if wq == "bf16" else w).double()


def _both(fn, *ops):
    """(formula on the operands, the same formula on their absolute values)"""
    return fn(*ops), fn(*[o.abs() for o in ops])


def conv_same(x, w, k, dgrad=False, wq="fp32"):
    """x [B, Cin, H, W], w [Cout, Cin, k, k] (dgrad: the forward weight [Cin, Cout, k, k]) -> (y, Mag) [B, Cout, H, W], K_tot"""
    p = k // 2

    def f(x, w):
        y = 0
        for ky in range(k):
            for kx in range(k):
                if dgrad:
                    y = y + torch.einsum("io,bihw->bohw", w[:, :, ky, kx], _shift(x, p - ky, p - kx))
                else:
                    y = y + torch.einsum("oi,bihw->bohw", w[:, :, ky, kx], _shift(x, ky - p, kx - p))
        return y
    return (*_both(f, x.double(), _wq(w, wq)), x.shape[1] * k * k)


def conv_wgrad(x, dy, k):
    """-> (dw, Mag) [Cout, Cin, k, k] (the sum, to be ADDED), K_tot = B H W"""
    p = k // 2

    def f(x, dy):
        taps = [torch.einsum("bohw,bihw->oi", dy, _shift(x, ky - p, kx - p)) for ky in range(k) for kx in range(k)]
        return torch.stack(taps, -1).view(dy.shape[1], x.shape[1], k, k)
    return (*_both(f, x.double(), dy.double()), x.shape[0] * x.shape[2] * x.shape[3])


def pw_small(x, W, G, transpose):
    """x [B, groups, G, HW], W [groups, G, G] -> [B, groups, G, HW]"""
    f = (lambda x, W: torch.einsum("jio,bjip->bjop", W, x)) if transpose else (lambda x, W: torch.einsum("joi,bjip->bjop", W, x))
    return (*_both(f, x.double(), W.double()), G)


def pw_fewout_fwd(x, W, bias):
    b = bias.double() if bias is not None else torch.zeros(W.shape[0], dtype=torch.float64, device=W.device)
    return (*_both(lambda x, W, b: torch.einsum("oi,bip->bop", W, x) + b[None, :, None], x.double(), W.double(), b), W.shape[1])


def pw_fewout_dgrad(dy, W):
    return (*_both(lambda dy, W: torch.einsum("oi,bop->bip", W, dy), dy.double(), W.double()), W.shape[0])


def pw_fewout_wgrad(x, dy):
    """-> (dW [Cout, Cin], Mag), (dbias [Cout], Mag), K_tot"""
    x, dy = x.double(), dy.double()
    return (_both(lambda x, dy: torch.einsum("bop,bip->oi", dy, x), x, dy), (dy.sum((0, 2)), dy.abs().sum((0, 2))),
            x.shape[0] * x.shape[2])


def dw3x3(x, w, bias, dil=1, flip=False):
    """x [B, C, H, W] (a view in any layout), w [C, 9], bias [C] or None -> (y, Mag), K_tot = 9"""
    b = bias.double() if bias is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)

    def f(x, w, b):
        y = b[None, :, None, None].expand(x.shape).clone()
        for t in range(9):
            ky, kx = divmod(t, 3)
            y = y + w[None, :, 8 - t if flip else t, None, None] * _shift(x, (ky - 1) * dil, (kx - 1) * dil)
        return y
    return (*_both(f, x.double(), w.reshape(-1, 9).double(), b), 9)


def dw3x3_wgrad(x, dy, dil=1):
    """-> (dw [C, 9], Mag), (dbias [C], Mag), K_tot = B H W"""
    def f(x, dy):
        return torch.stack([(dy * _shift(x, (t // 3 - 1) * dil, (t % 3 - 1) * dil)).sum((0, 2, 3)) for t in range(9)], -1)
    x, dy = x.double(), dy.double()
    return _both(f, x, dy), (dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))), x.shape[0] * x.shape[2] * x.shape[3]


def _dact64(v, act, slope):
    if act == "none":
        return torch.ones_like(v)
    if act == "relu":
        return (v > 0).double()
    if act == "lrelu":
        return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, slope))
    if act == "gelu":
        return 0.5 * (1.0 + torch.erf(v * 0.7071067811865476)) + v * torch.exp(-0.5 * v * v) * 0.3989422804014327
    raise ValueError(act)


DACT_MAX = {"none": 1.0, "relu": 1.0, "lrelu": 1.0, "gelu": 1.13}   # sup |act'|
DACT_LIP = {"none": 0.0, "relu": 0.0, "lrelu": 0.0, "gelu": L_DGELU}  # Lipschitz factor of act' (away from the kink of relu / lrelu)


def dw_bwd_pre(x, g, w, bias, act, slope):
    """gu = g act'(conv(x) + bias) -> (gu, the magnitude whose accumulation term bounds gu's error: |g| Mag_u, to be used with
    lip = DACT_LIP[act]), u, Mag_u"""
    u, mu, _ = dw3x3(x, w, bias)
    g = g.double()
    return g * _dact64(u, act, slope), g.abs() * mu, u, mu


# ---- host measurement of the constants ---------------------------------------------------------------------------------------
def measure_constants(conv_shapes, wgrad_shapes, seed=0):
    """conv_shapes: (Cin, Cout, k, H, W); wgrad_shapes: (B, Cin, Cout, k, H, W).  Plain fp32 on the CPU -- one fp32 partial sum per
    tap (per tap and image for a weight gradient), added in a shuffled order -- against float64, operands normal and normal + 1.
    Returns (accumulation ratio, store ratio, gelu' sensitivity)."""
    g = torch.Generator().manual_seed(seed)
    r_acc = r_out = 0.0
    for (Ci, Co, k, H, W) in conv_shapes:
        for off in (0.0, 1.0):
            x, w = reals((1, Ci, H, W), g, off).to(BF).float(), reals((Co, Ci, k, k), g, off).to(BF).float()
            ref, mag, K = conv_same(x, w, k)
            parts = [torch.einsum("oi,bihw->bohw", w[:, :, t // k, t % k], _shift(x, t // k - k // 2, t % k - k // 2)) for t in range(k * k)]
            y = torch.zeros_like(parts[0])
            for i in torch.randperm(len(parts), generator=g).tolist():
                y = y + parts[i]
            e32 = (y.double() - ref).abs()
            r_acc = max(r_acc, float((e32 / (U_FP32 * math.sqrt(K) * mag)).max()))
            e16 = (y.to(BF).double() - ref).abs()
            r_out = max(r_out, float(((e16 - e32) / (U_BF16 * ref.abs()).clamp_min(1e-300)).max()))
    for (B, Ci, Co, k, H, W) in wgrad_shapes:
        for off in (0.0, 1.0):
            x, dy = reals((B, Ci, H, W), g, off).to(BF).float(), reals((B, Co, H, W), g, off).to(BF).float()
            ref, mag, K = conv_wgrad(x, dy, k)
            parts = [torch.stack([torch.einsum("ohw,ihw->oi", dy[b], _shift(x[b], t // k - k // 2, t % k - k // 2)) for t in range(k * k)],
                                 -1).view(Co, Ci, k, k) for b in range(B)]
            y = torch.zeros_like(parts[0])
            for i in torch.randperm(B, generator=g).tolist():
                y = y + parts[i]
            r_acc = max(r_acc, float(((y.double() - ref).abs() / (U_FP32 * math.sqrt(K) * mag)).max()))
    z = torch.linspace(-8.0, 8.0, 160001, dtype=torch.float64)
    d = _dact64(z, "gelu", 0.0)
    r_dg = float(((d[1:] - d[:-1]).abs() / (z[1:] - z[:-1])).max())
    return r_acc, r_out, r_dg
