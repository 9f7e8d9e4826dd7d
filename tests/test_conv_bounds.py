"""The convolutions that do not go through the GEMM (conv_direct.hip, conv_c1.hip, dwconv.hip), kernel by kernel, held per element
to the float64 reference of tests/conv_ref.py.

* CASES: one case per kernel name `kern.last_conv_kernel()` can report (the dispatchers are host code: the name is asserted on the
  host checker as on the MI355X), at the smallest shape that selects it, plus the shapes that reach the loops only a big batch
  reaches otherwise: the multi-tile walk of conv_direct (CENET_CONV_DIRECT_GRID, and naturally with > 512 / > 256 tiles on the
  GPU), several planes per workgroup in the NCHW depthwise plane kernels (B C >= 2047), rows_per_wg > 8 in conv_c1's weight
  gradient (CENET_C1_WGS), two tiles per workgroup in tok_bwd_pre, several passes in dw3x3_wgrad_nchw_chan_kernel.  Every case
  runs the exact regime (integers: the output equals the reference, no tolerance) and, where a bf16 store, a transcendental
  activation or a deep fp32 sum is involved, the bound regime.  Operands sit in NaN-filled buffers, destinations in sentinel-filled
  ones with a lead offset and padded batch strides where the ABI takes them: nothing outside the footprint may change (bitwise).
  The set of covered names is held equal to what the dispatcher rules can produce (`_nameable`).
* mutation self-test (no kernel): deliberately wrong REFERENCES must be rejected by the rules.
      mutation                                                  exact   bound (normal + 1 operands)
      one tap dropped at the ragged right column                yes     yes (one of 9 same-sign terms against u_out = 0.4 %)
      halo of the neighbouring tile for one tile                yes     yes
      weight of channel c + 1 for one plane (ppw > 1 shape)     yes     yes
      flip ignored                                              yes     yes
      dilation off by one in y only                             yes     yes
      bias skipped on the last channel                          yes     yes
      one weight-gradient tile counted twice                    yes     yes
      dw_acc overwritten instead of added to                    yes     yes
      truncation instead of round-to-nearest (bf16)             yes     yes (up to 2 u_out: C_OUT may not reach 2)
`sim` = the kernel sources on the host SIMT checker (CPU); `hip` = the gfx950 library (marker gpu)."""
import math

import pytest
import torch

import conv_ref as R
from backend import dev  # noqa: F401
from cenet_amd import _lib, kern

BF, F32 = torch.bfloat16, torch.float32
SENTINEL = 12288.0  # exact in bf16
NAN = float("nan")


def _sync(d):
    if d.type == "cuda":
        torch.cuda.synchronize()


def _vals(shape, g, regime):
    if regime == "exact":
        return R.ints(shape, g)
    return R.reals(shape, g, 1.0 if regime == "offset" else 0.0).to(BF).float()


def _put(x, d, dtype=BF, lead=8, pad=0, fill=NAN):
    """x [B, ...] -> (flat buffer, element offset, batch stride): images `pad` elements apart, the lot surrounded by `fill`"""
    B, n = x.shape[0], x[0].numel()
    sb = n + pad
    buf = torch.full((lead + B * sb + 16,), fill, dtype=F32)
    buf[lead:lead + B * sb].view(B, sb)[:, :n] = x.reshape(B, n)
    return buf.to(dtype).to(d), lead, sb


def _dest(shape, d, dtype=BF, lead=8, pad=0):
    return _put(torch.full(shape, SENTINEL), d, dtype, lead, pad, fill=SENTINEL)


def _acc(shape, d, g, regime, lead=4):
    """an fp32 accumulator ("ADDED into") with previous contents, inside a sentinel-filled buffer"""
    prev = R.ints(shape, g) if regime == "exact" else torch.full(shape, 0.75)
    buf, off, _ = _put(prev[None], d, F32, lead, 0, fill=SENTINEL)
    return buf, off


def _nchw(shape, sb):
    B, C, H, W = shape
    return (sb, H * W, W, 1)


def _check(regime, checks, what):
    worst = 0.0
    for got, exp in checks:
        if regime == "exact":
            R.assert_exact(got, exp, what)
        else:
            worst = max(worst, R.assert_bound(got, exp, what))
    if regime != "exact":
        print(f"BOUND {what} [{regime}]: worst |err| / bound = {worst:.3f}")
    return worst


def _named(expected):
    got = kern.last_conv_kernel()
    assert got == expected, (got, expected)
    return got


# ---- conv_direct ---------------------------------------------------------------------------------------------------------------
DIRECT = {(32, 32, 5): 4, (64, 64, 3): 8, (64, 32, 3): 8, (32, 64, 3): 4}  # (Cin, Cout, k): waves


def run_direct(d, regime, Cin, Cout, k, B, H, W, dgrad, grid, wq=False, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = _vals((B, Cin, H, W), g, regime)
    w = _vals((Cin, Cout, k, k) if dgrad else (Cout, Cin, k, k), g, regime)
    if wq:  # fp32 master weights that are NOT bf16 values: the kernel rounds them once, and so does the reference
        w = w + R.reals(tuple(w.shape), g) * 2.0 ** -10
    xb, xo, sx = _put(x, d, BF, lead=3)
    yb, yo, sy = _dest((B, Cout, H, W), d, BF, lead=4)
    wd = w.to(d)
    ref, mag, K = R.conv_same(R.view(xb, xo, x.shape, _nchw(x.shape, sx)), wd, k, dgrad=dgrad, wq="bf16")
    ntiles = B * -(-H // 8) * -(-W // 32)
    name = f"conv_direct_bf16_kernel<{Cin}, {Cout}, {k}, {DIRECT[(Cin, Cout, k)]}> dgrad={int(dgrad)} grid={grid} ntiles={ntiles}"
    exp = R.expect(yb, yo, (B, Cout, H, W), _nchw((B, Cout, H, W), sy), ref, mag, K, tile=(8, 32), kernel=name)
    kern.conv_direct(xb[xo:], wd, yb[yo:], B, Cin, Cout, H, W, k, dgrad)
    _sync(d)
    _named(name)
    return _check(regime, [(yb, exp)], name)


def run_wgrad_direct(d, regime, Cin, Cout, k, B, H, W, lead, vec, grid, seed=2):
    g = torch.Generator().manual_seed(seed)
    x, dy = _vals((B, Cin, H, W), g, regime), _vals((B, Cout, H, W), g, regime)
    xb, xo, sx = _put(x, d, BF, lead=lead)
    gb, go, sg = _put(dy, d, BF, lead=lead)
    db, do = _acc((Cout, Cin, k, k), d, g, regime)
    ref, mag, K = R.conv_wgrad(R.view(xb, xo, x.shape, _nchw(x.shape, sx)), R.view(gb, go, dy.shape, _nchw(dy.shape, sg)), k)
    th = 8 if k == 5 else 4
    ntiles = B * -(-H // th) * -(-W // 32)
    inst = {(32, 32, 5): "32, 32, 5, 8, 8, 2", (64, 64, 3): "64, 64, 3, 4, 8", (64, 32, 3): "64, 32, 3, 4, 4"}[(Cin, Cout, k)]
    name = f"conv_wgrad_direct_kernel<{inst}> vec={vec} grid={grid} ntiles={ntiles}"
    exp = R.expect(db, do, (Cout, Cin, k, k), (Cin * k * k, k * k, k, 1), ref, mag, K, add=True, dims=("co", "ci", "ky", "kx"),
                   kernel=name)
    kern.conv_wgrad_direct(xb[xo:], gb[go:], db[do:], B, Cin, Cout, H, W, k)
    _sync(d)
    _named(name)
    return _check(regime, [(db, exp)], name)


# ---- conv_c1 -------------------------------------------------------------------------------------------------------------------
def run_c1_fwd(d, regime, k, B, Cout, H, W, mfma, ylead=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    x, w = _vals((B, 1, H, W), g, regime), _vals((Cout, 1, k, k), g, regime)
    xb, xo, sx = _put(x, d, BF, lead=3)
    yb, yo, sy = _dest((B, Cout, H, W), d, BF, lead=ylead)
    wd = w.to(d)
    ref, mag, K = R.conv_same(R.view(xb, xo, x.shape, _nchw(x.shape, sx)), wd, k, wq="bf16" if mfma else "fp32")
    name = "conv_c1_fwd_mfma5_kernel rows_per_wg=8" if mfma else f"conv_c1_fwd_kernel<{k}> rows_per_wg=8"
    exp = R.expect(yb, yo, (B, Cout, H, W), _nchw((B, Cout, H, W), sy), ref, mag, K, tile=(8, 128), kernel=name)
    kern.conv_c1_fwd(xb[xo:], wd, yb[yo:], B, Cout, H, W, k)
    _sync(d)
    _named(name)
    return _check(regime, [(yb, exp)], name)


def run_c1_wgrad(d, regime, k, B, Cout, H, W, mfma, rows, glead=8, seed=4):
    g = torch.Generator().manual_seed(seed)
    x, dy = _vals((B, 1, H, W), g, regime), _vals((B, Cout, H, W), g, regime)
    xb, xo, sx = _put(x, d, BF, lead=3)
    gb, go, sg = _put(dy, d, BF, lead=glead)
    db, do = _acc((Cout, 1, k, k), d, g, regime)
    ref, mag, K = R.conv_wgrad(R.view(xb, xo, x.shape, _nchw(x.shape, sx)), R.view(gb, go, dy.shape, _nchw(dy.shape, sg)), k)
    name = f"conv_c1_wgrad_mfma5_kernel rows_per_wg={rows}" if mfma else f"conv_c1_wgrad_kernel<{k}> rows_per_wg={rows}"
    exp = R.expect(db, do, (Cout, 1, k, k), (k * k, k * k, k, 1), ref, mag, K, add=True, dims=("co", "ci", "ky", "kx"), kernel=name)
    kern.conv_c1_wgrad(xb[xo:], gb[go:], db[do:], B, Cout, H, W, k)
    _sync(d)
    _named(name)
    return _check(regime, [(db, exp)], name)


# ---- pointwise -----------------------------------------------------------------------------------------------------------------
def run_pw_small(d, regime, G, tr, groups, HW, B=2, seed=5):
    g = torch.Generator().manual_seed(seed)
    x, W = _vals((B, groups * G, HW), g, regime), _vals((groups, G, G), g, regime)
    xb, xo, sx = _put(x, d, BF, lead=2)
    yb, yo, sy = _dest((B, groups * G, HW), d, BF, lead=2)
    Wd = W.to(BF).to(d)
    shape, st = (B, groups, G, HW), (sx, G * HW, HW, 1)
    ref, mag, K = R.pw_small(R.view(xb, xo, shape, st), Wd, G, tr)
    name = f"pw_small_kernel<{G}, {'true' if tr else 'false'}> even={int(HW % 2 == 0)}"
    exp = R.expect(yb, yo, shape, st, ref, mag, K, dims=("image", "group", "channel", "pixel"), kernel=name)
    kern.pw_small(xb[xo:], Wd, yb[yo:], B, groups, G, HW, transpose=tr)
    _sync(d)
    _named(name)
    return _check(regime, [(yb, exp)], name)


def run_pwf(d, regime, kind, Cout, HW, extra, B=2, seed=6):
    """kind fwd (extra: bias) / dgrad / wgrad (extra: dbias)"""
    g = torch.Generator().manual_seed(seed)
    even = int(HW % 2 == 0)
    x, dy, W = _vals((B, 64, HW), g, regime), _vals((B, Cout, HW), g, regime), _vals((Cout, 64), g, regime)
    xb, xo, sx = _put(x, d, BF, lead=2)
    gb, go, sg = _put(dy, d, BF, lead=2)
    Wd = W.to(BF).to(d)
    xv, gv = R.view(xb, xo, x.shape, (sx, HW, 1)), R.view(gb, go, dy.shape, (sg, HW, 1))
    dims = ("image", "channel", "pixel")
    if kind == "fwd":
        bias = _vals((Cout,), g, regime).to(d) if extra else None
        yb, yo, sy = _dest((B, Cout, HW), d, BF, lead=2)
        name = f"pw_fewout_fwd_kernel CO={Cout} even={even}"
        ref, mag, K = R.pw_fewout_fwd(xv, Wd, bias)
        exp = [(yb, R.expect(yb, yo, (B, Cout, HW), (sy, HW, 1), ref, mag, K, dims=dims, kernel=name))]
        kern.pw_fewout_fwd(xb[xo:], Wd, bias, yb[yo:], B, 64, Cout, HW)
    elif kind == "dgrad":
        yb, yo, sy = _dest((B, 64, HW), d, BF, lead=2)
        name = f"pw_fewout_dgrad_kernel<{2 if Cout <= 2 else 4 if Cout <= 4 else 9 if Cout <= 9 else 16}> even={even}"
        ref, mag, K = R.pw_fewout_dgrad(gv, Wd)
        exp = [(yb, R.expect(yb, yo, (B, 64, HW), (sy, HW, 1), ref, mag, K, dims=dims, kernel=name))]
        kern.pw_fewout_dgrad(gb[go:], Wd, yb[yo:], B, 64, Cout, HW)
    else:
        wb, wo = _acc((Cout, 64), d, g, regime)
        name = f"pw_fewout_wgrad_kernel<{Cout}> even={even}"
        (rw, mw), (rb, mb), K = R.pw_fewout_wgrad(xv, gv)
        exp = [(wb, R.expect(wb, wo, (Cout, 64), (64, 1), rw, mw, K, add=True, dims=("co", "ci"), kernel=name))]
        bb = None
        if extra:
            bb, bo = _acc((Cout,), d, g, regime)
            exp.append((bb, R.expect(bb, bo, (Cout,), (1,), rb, mb, K, add=True, dims=("co",), kernel=name + " dbias")))
        kern.pw_fewout_wgrad(xb[xo:], gb[go:], wb[wo:], bb[bo:] if extra else None, B, 64, Cout, HW)
    _sync(d)
    _named(name)
    return _check(regime, exp, name)


# ---- depthwise, NCHW -----------------------------------------------------------------------------------------------------------
def _chan_weights(C, g, regime):
    """per-channel DISTINCT weights and biases (a wrong channel index fails the exact regime): integers in [-4, 4] whose pattern
    over the nine taps differs from channel to channel"""
    if regime != "exact":
        return _vals((C, 9), g, regime), _vals((C,), g, regime)
    c = torch.arange(C)
    w = torch.stack([((c // 9 ** (t % 4) + t * (c % 7 + 1)) % 9 - 4) for t in range(9)], -1).float()
    return w, ((c * 5 + c // 9) % 9 - 4).float()


def run_dw_nchw(d, regime, name, B, C, H, W, dil=1, flip=False, act="none", want="ya", bias=True, f32=False, pad=0, lead=8, seed=7):
    g = torch.Generator().manual_seed(seed)
    dt = F32 if f32 else BF
    x = _vals((B, C, H, W), g, regime)
    w, bv = _chan_weights(C, g, regime)
    xb, xo, sx = _put(x, d, dt, lead=lead, pad=pad)
    wd, bd = w.to(d), (bv.to(d) if bias else None)
    ref, mag, K = R.dw3x3(R.view(xb, xo, x.shape, _nchw(x.shape, sx)), wd, bd, dil, flip)
    checks, yb, ab, yo, sy, sa = [], None, None, 0, 0, 0
    if "y" in want:
        yb, yo, sy = _dest((B, C, H, W), d, dt, lead=lead, pad=pad)
        checks.append((yb, R.expect(yb, yo, x.shape, _nchw(x.shape, sy), ref, mag, K, kernel=name)))
    if "a" in want:
        ab, ao, sa = _dest((B, C, H, W), d, dt, lead=lead, pad=2 * pad)
        checks.append((ab, R.expect(ab, ao, x.shape, _nchw(x.shape, sa), R._act64(ref, act, 0.25), mag, K, lip=R.ACT_LIPSCHITZ[act],
                                    kernel=name + " a")))
    kern.dw_nchw(xb, sx, wd, bd, yb, sy, ab[ao:] if ab is not None else None, sa, B, C, H, W, dil, flip, act=act, slope=0.25,
                 x_off=xo, y_off=yo)
    _sync(d)
    _named(name)
    return _check(regime, checks, name)


def run_dw_wgrad_nchw(d, regime, name, B, C, H, W, dil=1, dbias=True, f32=False, pad=0, lead=8, seed=8):
    g = torch.Generator().manual_seed(seed)
    dt = F32 if f32 else BF
    x, dy = _vals((B, C, H, W), g, regime), _vals((B, C, H, W), g, regime)
    xb, xo, sx = _put(x, d, dt, lead=lead, pad=pad)
    gb, go, sg = _put(dy, d, dt, lead=lead, pad=2 * pad)
    wb, wo = _acc((C, 9), d, g, regime)
    bb, bo = _acc((C,), d, g, regime)
    (rw, mw), (rb, mb), K = R.dw3x3_wgrad(R.view(xb, xo, x.shape, _nchw(x.shape, sx)), R.view(gb, go, x.shape, _nchw(x.shape, sg)), dil)
    checks = [(wb, R.expect(wb, wo, (C, 9), (9, 1), rw, mw, K, add=True, dims=("channel", "tap"), kernel=name))]
    if dbias:
        checks.append((bb, R.expect(bb, bo, (C,), (1,), rb, mb, K, add=True, dims=("channel",), kernel=name + " dbias")))
    kern.dw_wgrad_nchw(xb, sx, gb, sg, wb[wo:], bb[bo:] if dbias else None, B, C, H, W, dil, x_off=xo, g_off=go)
    _sync(d)
    _named(name)
    return _check(regime, checks, name)


def run_dw_multi(d, regime, wgrad, B, H, W, Cs, dils, ppws, flip=False, seed=9):
    """the branches are channel slices of ONE tensor (batch stride = all the channels), as the CFAM block passes them"""
    g = torch.Generator().manual_seed(seed)
    Ct, HW = sum(Cs), H * W
    x, dy = _vals((B, Ct, H, W), g, regime), _vals((B, Ct, H, W), g, regime)
    xb, xo, sx = _put(x, d, BF, lead=8, pad=8)
    kname = "dw3x3_wgrad_nchw_plane_multi_kernel" if wgrad else "dw3x3_nchw_plane_multi_kernel"
    name = f"{kname} ppw={','.join(str(p) for p in ppws)}"
    branches, checks, c0 = [], [], 0
    if wgrad:
        gb, go, sg = _put(dy, d, BF, lead=8, pad=8)
    else:
        yb, yo, sy = _dest((B, Ct, H, W), d, BF, lead=8, pad=8)
        ycur = None
    for i, (C, dil) in enumerate(zip(Cs, dils)):
        shape = (B, C, H, W)
        xv = R.view(xb, xo + c0 * HW, shape, _nchw(shape, sx))
        if wgrad:
            wb, wo = _acc((C, 9), d, g, regime)
            (rw, mw), _, K = R.dw3x3_wgrad(xv, R.view(gb, go + c0 * HW, shape, _nchw(shape, sg)), dil)
            checks.append((wb, R.expect(wb, wo, (C, 9), (9, 1), rw, mw, K, add=True, dims=("channel", "tap"), kernel=f"{name} branch {i}")))
            branches.append((xb, xo + c0 * HW, sx, gb, go + c0 * HW, sg, wb[wo:], C, dil))
        else:
            w, _ = _chan_weights(C, g, regime)
            wd = w.roll(i + 1, 0).contiguous().to(d)
            ref, mag, K = R.dw3x3(xv, wd, None, dil, flip)
            e = R.expect(yb, yo + c0 * HW, shape, _nchw(shape, sy), ref, mag, K, kernel=f"{name} branch {i}")
            if ycur is None:
                ycur = e
            else:  # one destination buffer for all branches: fold the branch into the running expectation
                ycur.C, ycur.Mag = torch.where(e.own, e.C, ycur.C), torch.where(e.own, e.Mag, ycur.Mag)
                ycur.own = ycur.own | e.own
                ycur.idx = torch.cat([ycur.idx.reshape(-1), e.idx.reshape(-1)])
                ycur.dims, ycur.tile = ("output",), None
            branches.append((xb, xo + c0 * HW, sx, wd, yb, yo + c0 * HW, sy, C, dil))
        c0 += C
    if wgrad:
        assert kern.dw_wgrad_nchw_multi(branches, B, H, W)
    else:
        assert kern.dw_nchw_multi(branches, B, H, W, flip)
        checks.append((yb, ycur))
    _sync(d)
    _named(name)
    return _check(regime, checks, name)


# ---- depthwise, tokens ---------------------------------------------------------------------------------------------------------
def _tok(shape):
    B, C, H, W = shape
    return (H * W * C, 1, W * C, C)


def _to_tok(x):
    return x.permute(0, 2, 3, 1).contiguous()


def run_dw_tok(d, regime, name, B, C, H, W, flip=False, act="none", want="ya", bias=True, f32=False, lead=8, seed=10):
    g = torch.Generator().manual_seed(seed)
    dt = F32 if f32 else BF
    shape = (B, C, H, W)
    x = _vals(shape, g, regime)
    w, bv = _chan_weights(C, g, regime)
    xb, xo, _ = _put(_to_tok(x), d, dt, lead=lead)
    wd, bd = w.to(d), (bv.to(d) if bias else None)
    ref, mag, K = R.dw3x3(R.view(xb, xo, shape, _tok(shape)), wd, bd, 1, flip)
    checks, yb, ab, yo, ao = [], None, None, 0, 0
    if "y" in want:
        yb, yo, _ = _dest((B, H, W, C), d, dt, lead=lead)
        checks.append((yb, R.expect(yb, yo, shape, _tok(shape), ref, mag, K, kernel=name)))
    if "a" in want:
        ab, ao, _ = _dest((B, H, W, C), d, dt, lead=lead)
        checks.append((ab, R.expect(ab, ao, shape, _tok(shape), R._act64(ref, act, 0.25), mag, K, lip=R.ACT_LIPSCHITZ[act],
                                    kernel=name + " a")))
    kern.dw_tok(xb[xo:], wd, bd, yb[yo:] if yb is not None else None, ab[ao:] if ab is not None else None, B, C, H, W, flip,
                act=act, slope=0.25)
    _sync(d)
    _named(name)
    return _check(regime, checks, name)


def run_dw_wgrad_tok(d, regime, name, B, C, H, W, f32=False, lead=8, seed=11):
    g = torch.Generator().manual_seed(seed)
    dt = F32 if f32 else BF
    shape = (B, C, H, W)
    x, dy = _vals(shape, g, regime), _vals(shape, g, regime)
    xb, xo, _ = _put(_to_tok(x), d, dt, lead=lead)
    gb, go, _ = _put(_to_tok(dy), d, dt, lead=lead)
    wb, wo = _acc((C, 9), d, g, regime)
    bb, bo = _acc((C,), d, g, regime)
    (rw, mw), (rb, mb), K = R.dw3x3_wgrad(R.view(xb, xo, shape, _tok(shape)), R.view(gb, go, shape, _tok(shape)), 1)
    checks = [(wb, R.expect(wb, wo, (C, 9), (9, 1), rw, mw, K, add=True, dims=("channel", "tap"), kernel=name)),
              (bb, R.expect(bb, bo, (C,), (1,), rb, mb, K, add=True, dims=("channel",), kernel=name + " dbias"))]
    kern.dw_wgrad_tok(xb[xo:], gb[go:], wb[wo:], bb[bo:], B, C, H, W)
    _sync(d)
    _named(name)
    return _check(regime, checks, name)


def run_dw_bwd_pre(d, regime, name, B, C, H, W, act, seed=12):
    g = torch.Generator().manual_seed(seed)
    shape = (B, C, H, W)
    x, gr = _vals(shape, g, regime), _vals(shape, g, regime)
    w, bv = _chan_weights(C, g, regime)
    if regime == "exact" and act != "none":  # keep the pre-activation off the kink: odd integers + an even bias never sum to ... 0
        bv = bv * 0 + 0.5                    # (u = integer + 1/2 is never 0; exact in bf16 and in the fp32 sum)
    xb, xo, _ = _put(_to_tok(x), d, BF, lead=8)
    gb, go, _ = _put(_to_tok(gr), d, BF, lead=8)
    ub, uo, _ = _dest((B, H, W, C), d, BF, lead=8)
    wb, wo = _acc((C, 9), d, g, regime)
    bb, bo = _acc((C,), d, g, regime)
    wd, bd = w.to(d), bv.to(d)
    xv = R.view(xb, xo, shape, _tok(shape))
    gu, gmag, u, mu = R.dw_bwd_pre(xv, R.view(gb, go, shape, _tok(shape)), wd, bd, act, 0.25)
    th, tw = (8, 14) if W % 14 == 0 else ((8, 8) if W <= 8 and H <= 8 else (8, 16))
    # gu: one rounding of g act'(u) + the recomputed pre-activation's error through act' (lip = its Lipschitz factor)
    e_gu = R.expect(ub, uo, shape, _tok(shape), gu, gmag, 9, lip=R.DACT_LIP[act], tile=(th, tw), kernel=name + " gu")
    (rw, mw), (rb, mb), K = R.dw3x3_wgrad(xv, gu)
    mw = R.dw3x3_wgrad(xv, gr.to(d).double().abs() * R.DACT_MAX[act])[0][1]  # magnitude from |g| sup|act'|, not from a cancelling gu
    mb = (gr.to(d).double().abs() * R.DACT_MAX[act]).sum((0, 2, 3))
    checks = [(ub, e_gu), (wb, R.expect(wb, wo, (C, 9), (9, 1), rw, mw, K, add=True, dims=("channel", "tap"), kernel=name + " dw")),
              (bb, R.expect(bb, bo, (C,), (1,), rb, mb, K, add=True, dims=("channel",), kernel=name + " dbias"))]
    kern.dw_tok_bwd_pre(xb[xo:], gb[go:], wd, bd, ub[uo:], wb[wo:], bb[bo:], B, C, H, W, act, slope=0.25)
    _sync(d)
    _named(name)
    return _check(regime, checks, name)


# ---- the case matrix -----------------------------------------------------------------------------------------------------------
CASES = []   # dicts: id, name (as the reporter spells it), fn(dev, regime), bound, slow, gpu_only, env


def _add(cid, name, fn, bound=False, slow=False, gpu_only=False, env=None, exact=True):
    CASES.append(dict(id=cid, name=name, fn=fn, bound=bound, slow=slow, gpu_only=gpu_only, env=env or {}, exact=exact))


for (ci, co, k), nw in DIRECT.items():
    for dg in (0, 1):
        inst = f"conv_direct_bf16_kernel<{ci}, {co}, {k}, {nw}> dgrad={dg}"
        big = ci + co == 128
        _add(f"direct-{ci}-{co}-k{k}-d{dg}-ragged", inst, lambda d, r, a=(ci, co, k), dg=dg: run_direct(d, r, *a, 2, 11, 70, dg, 12),
             bound=True, slow=big)
        _add(f"direct-{ci}-{co}-k{k}-d{dg}-full", inst, lambda d, r, a=(ci, co, k), dg=dg: run_direct(d, r, *a, 1, 16, 64, dg, 4),
             slow=True)
        _add(f"direct-{ci}-{co}-k{k}-d{dg}-walk", inst, lambda d, r, a=(ci, co, k), dg=dg: run_direct(d, r, *a, 2, 19, 104, dg, 5),
             env={"CENET_CONV_DIRECT_GRID": "5"}, bound=dg == 0, slow=big or dg == 1)
_add("direct-32-32-k5-natural", "conv_direct_bf16_kernel<32, 32, 5, 4> dgrad=0",
     lambda d, r: run_direct(d, r, 32, 32, 5, 1, 136, 1000, 0, 512), bound=True, gpu_only=True)
_add("direct-64-64-k3-natural", "conv_direct_bf16_kernel<64, 64, 3, 8> dgrad=1",
     lambda d, r: run_direct(d, r, 64, 64, 3, 1, 72, 1000, 1, 256), bound=True, gpu_only=True)
_add("direct-64-32-k3-wq", "conv_direct_bf16_kernel<64, 32, 3, 8> dgrad=0",
     lambda d, r: run_direct(d, r, 64, 32, 3, 1, 9, 33, 0, 4, wq=True), bound=True, exact=False)

for (ci, co, k) in [(32, 32, 5), (64, 64, 3), (64, 32, 3)]:
    inst = {5: "32, 32, 5, 8, 8, 2"}.get(k, "64, 64, 3, 4, 8" if co == 64 else "64, 32, 3, 4, 4")
    H = 10 if k == 5 else 6  # not a multiple of the tile height (8 / 4)
    _add(f"wgrad-direct-{ci}-{co}-vec", f"conv_wgrad_direct_kernel<{inst}> vec=1",
         lambda d, r, a=(ci, co, k), H=H: run_wgrad_direct(d, r, *a, 2, H, 40, 8, 1, 3), env={"CENET_WGRAD_GRID": "3"}, bound=True,
         slow=co == 64)
    _add(f"wgrad-direct-{ci}-{co}-novec", f"conv_wgrad_direct_kernel<{inst}> vec=0",
         lambda d, r, a=(ci, co, k), H=H: run_wgrad_direct(d, r, *a, 2, H, 33, 2, 0, 3), env={"CENET_WGRAD_GRID": "3"},
         slow=co == 64)

for k in (1, 3, 5):
    for (H, W, Co) in [(7, 9, 12), (19, 30, 32), (7, 132, 12)]:
        _add(f"c1-fwd-k{k}-{H}x{W}", f"conv_c1_fwd_kernel<{k}>", lambda d, r, k=k, s=(H, W, Co): run_c1_fwd(d, r, k, 2, s[2], s[0], s[1], False),
             bound=W == 30)
        _add(f"c1-wgrad-k{k}-{H}x{W}", f"conv_c1_wgrad_kernel<{k}>",
             lambda d, r, k=k, s=(H, W, Co): run_c1_wgrad(d, r, k, 2, s[2], s[0], s[1], False, 8), bound=W == 30)
for (W, Co) in [(16, 24), (160, 32)]:
    _add(f"c1-fwd-mfma-{W}", "conv_c1_fwd_mfma5_kernel", lambda d, r, s=(W, Co): run_c1_fwd(d, r, 5, 2, s[1], 11, s[0], True), bound=True)
for (W, Co) in [(32, 24), (160, 32)]:
    _add(f"c1-wgrad-mfma-{W}", "conv_c1_wgrad_mfma5_kernel", lambda d, r, s=(W, Co): run_c1_wgrad(d, r, 5, 2, s[1], 11, s[0], True, 8),
         bound=True)
_add("c1-wgrad-mfma-misaligned-dy", "conv_c1_wgrad_kernel<5>", lambda d, r: run_c1_wgrad(d, r, 5, 1, 24, 9, 32, False, 8, glead=4))
for H in (30, 27):  # CENET_C1_WGS=2: the row-group loop grows to 32 rows, staged 8 at a time (H = 27: a ragged last stage)
    _add(f"c1-wgrad-rows-k5-H{H}", "conv_c1_wgrad_kernel<5>", lambda d, r, H=H: run_c1_wgrad(d, r, 5, 2, 12, H, 30, False, 32),
         env={"CENET_C1_WGS": "2"})
    _add(f"c1-wgrad-rows-mfma-H{H}", "conv_c1_wgrad_mfma5_kernel", lambda d, r, H=H: run_c1_wgrad(d, r, 5, 2, 24, H, 32, True, 32),
         env={"CENET_C1_WGS": "2"})
_add("c1-wgrad-rows-k3-two-groups", "conv_c1_wgrad_kernel<3>", lambda d, r: run_c1_wgrad(d, r, 3, 2, 12, 27, 30, False, 16),
     env={"CENET_C1_WGS": "4"})

for G in (4, 8, 20, 32, 40):
    for tr in (False, True):
        for HW, groups in ((49, 3), (64, 1)):
            _add(f"pw-small-G{G}-t{int(tr)}-HW{HW}", f"pw_small_kernel<{G}, {'true' if tr else 'false'}> even={int(HW % 2 == 0)}",
                 lambda d, r, a=(G, tr, groups, HW): run_pw_small(d, r, *a), bound=G in (4, 40))
for Co in (1, 2, 3, 4, 9, 16):
    HW = 49 if Co % 2 else 64
    _add(f"pwf-fwd-{Co}", f"pw_fewout_fwd_kernel even={int(HW % 2 == 0)}", lambda d, r, a=(Co, HW): run_pwf(d, r, "fwd", *a, Co != 3),
         bound=Co in (1, 16))
_add("pwf-fwd-513", "pw_fewout_fwd_kernel even=0", lambda d, r: run_pwf(d, r, "fwd", 4, 513, True, B=1))
for Co, cls in ((2, 2), (3, 4), (9, 9), (12, 16)):
    for HW in (49, 64):
        _add(f"pwf-dgrad-{Co}-HW{HW}", f"pw_fewout_dgrad_kernel<{cls}> even={int(HW % 2 == 0)}",
             lambda d, r, a=(Co, HW): run_pwf(d, r, "dgrad", *a, None), bound=HW == 49)
_add("pwf-dgrad-513", "pw_fewout_dgrad_kernel<4> even=0", lambda d, r: run_pwf(d, r, "dgrad", 4, 513, None, B=1))
for Co in (2, 4, 9):
    for HW in (49, 64):
        _add(f"pwf-wgrad-{Co}-HW{HW}", f"pw_fewout_wgrad_kernel<{Co}> even={int(HW % 2 == 0)}",
             lambda d, r, a=(Co, HW): run_pwf(d, r, "wgrad", *a, HW == 49), bound=HW == 64)
_add("pwf-wgrad-2050", "pw_fewout_wgrad_kernel<2> even=1", lambda d, r: run_pwf(d, r, "wgrad", 2, 2050, True, B=1))

# NCHW depthwise: (instance, shape B C H W, keywords)
PL, V4, SC = "dw3x3_nchw_plane_kernel<%s> ppw=%d", "dw3x3_nchw_v4_kernel<%s, %s>", "dw3x3_nchw_kernel<%s>"
for cid, nm, shape, kw, bound in [
        ("plane-none", PL % ("ACT_NONE", 1), (2, 3, 8, 8), dict(want="y", dil=1), True),
        ("plane-none-a", PL % ("ACT_NONE", 1), (2, 3, 8, 8), dict(want="a", dil=2, act="none", bias=False), False),
        ("plane-gelu", PL % ("ACT_GELU", 1), (2, 3, 8, 8), dict(act="gelu", dil=3, pad=4, lead=12), True),
        ("plane-lrelu", PL % ("-1", 1), (2, 3, 8, 8), dict(act="lrelu", dil=5, pad=4), True),
        ("plane-flip", PL % ("ACT_NONE", 1), (2, 3, 6, 14), dict(want="y", flip=True, bias=False, dil=2), False),
        ("plane-ppw4", PL % ("ACT_NONE", 4), (2, 2050, 4, 4), dict(want="y"), True),
        ("plane-ppw4-lrelu", PL % ("-1", 4), (2, 2050, 4, 4), dict(act="lrelu", flip=True), False),
        ("v4-none", V4 % ("bf16_t", "ACT_NONE"), (1, 2, 64, 68), dict(want="y", dil=2), True),
        ("v4-gelu", V4 % ("bf16_t", "ACT_GELU"), (1, 2, 64, 68), dict(act="gelu", dil=2), True),
        ("v4-lrelu", V4 % ("bf16_t", "-1"), (1, 2, 64, 68), dict(act="lrelu", dil=2, flip=True), False),
        ("v4-f32", V4 % ("float", "-1"), (2, 3, 6, 8), dict(act="lrelu", dil=2, f32=True, pad=4, lead=4), True),
        ("scalar", SC % "bf16_t", (2, 3, 7, 7), dict(act="lrelu", dil=2, pad=3, lead=3), True),
        ("scalar-f32", SC % "float", (2, 3, 7, 7), dict(act="gelu", dil=3, f32=True), True)]:
    gelu = kw.get("act") == "gelu"
    _add("dw-nchw-" + cid, nm, lambda d, r, nm=nm, s=shape, kw=kw: run_dw_nchw(d, r, nm, *s, **kw), bound=bound, exact=not gelu,
         slow=shape[1] > 1000 and kw.get("act") == "lrelu")
WC = "dw3x3_wgrad_nchw_chan_kernel<%s> np=%d ipg=%d groups=%d"
for cid, nm, shape, kw in [
        ("chan-one-pass", WC % ("true", 5, 5, 1), (5, 6, 8, 8), dict()),
        ("chan-two-groups", WC % ("true", 5, 5, 2), (9, 3, 28, 28), dict()),   # image groups of 5 + 4: a partial last pass
        ("chan-two-passes", WC % ("true", 4, 8, 1), (5, 1025, 32, 32), dict()),  # C > 1024: ONE group walks 5 images in passes of 4 + 1
        ("chan-np-by-lds", WC % ("true", 1, 1, 4), (4, 2, 56, 56), dict(pad=4)),
        ("chan-ng1", WC % ("false", 7, 7, 1), (7, 1100, 4, 4), dict(dil=2)),
        ("plane", "dw3x3_wgrad_nchw_plane_kernel ppw=1", (2, 3, 8, 8), dict(dil=2, pad=4)),
        ("plane-14", "dw3x3_wgrad_nchw_plane_kernel ppw=1", (5, 3, 14, 14), dict(dbias=False)),
        ("plane-ppw4", "dw3x3_wgrad_nchw_plane_kernel ppw=4", (2, 2050, 4, 4), dict()),
        ("v4", "dw3x3_wgrad_nchw_v4_kernel<bf16_t>", (1, 2, 64, 68), dict(dil=2)),
        ("v4-f32", "dw3x3_wgrad_nchw_v4_kernel<float>", (2, 3, 6, 8), dict(dil=3, f32=True, lead=4)),
        ("scalar", "dw3x3_wgrad_nchw_kernel<bf16_t>", (2, 3, 7, 7), dict(dil=2, pad=3, lead=3)),
        ("scalar-f32", "dw3x3_wgrad_nchw_kernel<float>", (2, 3, 7, 7), dict(dil=5, f32=True, lead=3))]:
    _add("dw-wgrad-nchw-" + cid, nm, lambda d, r, nm=nm, s=shape, kw=kw: run_dw_wgrad_nchw(d, r, nm, *s, **kw), bound=shape[1] < 1000,
         slow=shape[1] * shape[2] > 8000)
_add("dw-nchw-multi", "dw3x3_nchw_plane_multi_kernel", lambda d, r: run_dw_multi(d, r, False, 2, 4, 4, (2050, 1500, 1030), (1, 2, 3), (4, 2, 2)))
_add("dw-nchw-multi-flip", "dw3x3_nchw_plane_multi_kernel", lambda d, r: run_dw_multi(d, r, False, 2, 8, 8, (5, 3), (2, 1), (1, 1), flip=True),
     bound=True)
_add("dw-wgrad-nchw-multi", "dw3x3_wgrad_nchw_plane_multi_kernel",
     lambda d, r: run_dw_multi(d, r, True, 2, 4, 4, (2050, 1500, 1030), (1, 2, 3), (4, 2, 2)), bound=True)

# token layout
ACTS = {"ACT_NONE": "none", "ACT_GELU": "gelu", "-1": "lrelu"}
TILES = {(8, 14): [(1, 8, 14, 14), (2, 136, 9, 28)], (8, 8): [(2, 136, 7, 8)], (8, 16): [(2, 8, 11, 19), (1, 136, 9, 16)]}
for (th, tw), shapes in TILES.items():
    for B, C, H, W in shapes:
        for an, act in ACTS.items():
            nm = f"dw3x3_tok_tile_kernel<{th}, {tw}, 0, {an}> tpw=1"
            _add(f"tok-tile-{th}x{tw}-m0-{act}-C{C}-{H}x{W}", nm,
                 lambda d, r, nm=nm, s=(B, C, H, W), act=act: run_dw_tok(d, r, nm, *s, act=act, want="a" if act == "none" else "ya"),
                 bound=C == 8, exact=act != "gelu")
            nm = f"dw3x3_tok_tile_kernel<{th}, {tw}, 2, {an}> tpw=1"
            _add(f"tok-tile-{th}x{tw}-m2-{act}-C{C}-{H}x{W}", nm, lambda d, r, nm=nm, s=(B, C, H, W), act=act: run_dw_bwd_pre(d, r, nm, *s, act),
                 bound=C == 8, exact=act != "gelu")
        nm = f"dw3x3_tok_tile_kernel<{th}, {tw}, 1, ACT_NONE> tpw=1"
        _add(f"tok-tile-{th}x{tw}-m1-C{C}-{H}x{W}", nm,
             lambda d, r, nm=nm, s=(B, C, H, W): run_dw_tok(d, r, nm, *s, flip=True, bias=False, want="y"), bound=C == 8)
_add("tok-tile-tpw2", "dw3x3_tok_tile_kernel<8, 14, 2, -1> tpw=2",
     lambda d, r: run_dw_bwd_pre(d, r, "dw3x3_tok_tile_kernel<8, 14, 2, -1> tpw=2", 1, 8, 64, 28, "lrelu"), bound=True)
_add("tok-tile-tpw3-aid", "dw3x3_tok_tile_kernel<8, 16, 2, ACT_NONE> tpw=3",
     lambda d, r: run_dw_bwd_pre(d, r, "dw3x3_tok_tile_kernel<8, 16, 2, ACT_NONE> tpw=3", 2, 8, 11, 35, "none"), env={"CENET_DW_TPW": "3"})
for hw in (14, 7):
    for C in (64, 128):
        for an, act in ACTS.items():
            if (C == 128) != (act == "lrelu"):
                continue
            nm = f"dw3x3_tok_plane_kernel<{hw}, 0, {an}>"
            _add(f"tok-plane-{hw}-m0-{act}", nm, lambda d, r, nm=nm, s=(2, C, hw, hw), act=act: run_dw_tok(d, r, nm, *s, act=act),
                 bound=True, exact=act != "gelu")
            nm = f"dw3x3_tok_plane_kernel<{hw}, 2, {an}>"
            _add(f"tok-plane-{hw}-m2-{act}", nm, lambda d, r, nm=nm, s=(2, C, hw, hw), act=act: run_dw_bwd_pre(d, r, nm, *s, act),
                 bound=True, exact=act != "gelu")
    nm = f"dw3x3_tok_plane_kernel<{hw}, 1, ACT_NONE>"
    _add(f"tok-plane-{hw}-m1", nm, lambda d, r, nm=nm, hw=hw: run_dw_tok(d, r, nm, 2, 64, hw, hw, flip=True, bias=False, want="y"))
for tn, f32 in (("bf16_t", False), ("float", True)):
    for sr, H in ((4, 29), (2, 9)):
        for cp, C in ((2, 6), (1, 5)):
            if f32 and cp == 2:
                continue
            nm = f"dw3x3_tok_kernel<{tn}, {sr}, {cp}>"
            _add(f"tok-strip-{tn}-sr{sr}-cp{cp}", nm,
                 lambda d, r, nm=nm, s=(2, C, H, 11), f32=f32: run_dw_tok(d, r, nm, *s, act="lrelu", f32=f32, flip=s[1] == 5, lead=2),
                 bound=not f32)
    _add(f"tok-wgrad-v4-{tn}", f"dw3x3_wgrad_tok_v4_kernel<{tn}>",
         lambda d, r, tn=tn, f32=f32: run_dw_wgrad_tok(d, r, f"dw3x3_wgrad_tok_v4_kernel<{tn}>", 2, 12, 9, 11, f32=f32, lead=8), bound=True)
    _add(f"tok-wgrad-scalar-{tn}", f"dw3x3_wgrad_tok_kernel<{tn}>",
         lambda d, r, tn=tn, f32=f32: run_dw_wgrad_tok(d, r, f"dw3x3_wgrad_tok_kernel<{tn}>", 2, 5, 9, 11, f32=f32, lead=3), bound=True)

RUNTIME = (" grid=", " ntiles=", " rows_per_wg=", " ppw=", " np=", " ipg=", " groups=", " tpw=", " CO=")


def _class(name):
    """a reported name without its run-time numbers (grid, ntiles, rows_per_wg, ppw, np, ipg, groups, tpw, CO)"""
    out = []
    for tok in name.split(" "):
        if not any(tok.startswith(r.strip()) for r in RUNTIME):
            out.append(tok)
    return " ".join(out)


def _nameable():
    """every name the dispatcher rules of the three files can produce, without run-time numbers"""
    n = set()
    for (ci, co, k), nw in DIRECT.items():
        n |= {f"conv_direct_bf16_kernel<{ci}, {co}, {k}, {nw}> dgrad={dg}" for dg in (0, 1)}
    for inst in ("32, 32, 5, 8, 8, 2", "64, 64, 3, 4, 8", "64, 32, 3, 4, 4"):
        n |= {f"conv_wgrad_direct_kernel<{inst}> vec={v}" for v in (0, 1)}
    for k in (1, 3, 5):
        n |= {f"conv_c1_fwd_kernel<{k}>", f"conv_c1_wgrad_kernel<{k}>"}
    n |= {"conv_c1_fwd_mfma5_kernel", "conv_c1_wgrad_mfma5_kernel"}
    for ev in (0, 1):
        n |= {f"pw_small_kernel<{G}, {t}> even={ev}" for G in (4, 8, 20, 32, 40) for t in ("true", "false")}
        n |= {f"pw_fewout_fwd_kernel even={ev}"}
        n |= {f"pw_fewout_dgrad_kernel<{c}> even={ev}" for c in (2, 4, 9, 16)}
        n |= {f"pw_fewout_wgrad_kernel<{c}> even={ev}" for c in (2, 4, 9)}
    acts = ("ACT_NONE", "ACT_GELU", "-1")
    n |= {f"dw3x3_nchw_plane_kernel<{a}>" for a in acts} | {f"dw3x3_nchw_v4_kernel<bf16_t, {a}>" for a in acts}
    n |= {"dw3x3_nchw_v4_kernel<float, -1>", "dw3x3_nchw_kernel<bf16_t>", "dw3x3_nchw_kernel<float>"}
    n |= {"dw3x3_wgrad_nchw_chan_kernel<true>", "dw3x3_wgrad_nchw_chan_kernel<false>", "dw3x3_wgrad_nchw_plane_kernel"}
    n |= {f"dw3x3_wgrad_nchw{v}_kernel<{t}>" for v in ("_v4", "") for t in ("bf16_t", "float")}
    n |= {"dw3x3_nchw_plane_multi_kernel", "dw3x3_wgrad_nchw_plane_multi_kernel"}
    modes = [(0, a) for a in acts] + [(1, "ACT_NONE")] + [(2, a) for a in acts]
    n |= {f"dw3x3_tok_tile_kernel<{th}, {tw}, {m}, {a}>" for (th, tw) in ((8, 14), (8, 8), (8, 16)) for m, a in modes}
    n |= {f"dw3x3_tok_plane_kernel<{hw}, {m}, {a}>" for hw in (14, 7) for m, a in modes}
    n |= {f"dw3x3_tok_kernel<bf16_t, {sr}, {cp}>" for sr in (4, 2) for cp in (2, 1)} | {f"dw3x3_tok_kernel<float, {sr}, 1>" for sr in (4, 2)}
    n |= {f"dw3x3_wgrad_tok{v}_kernel<{t}>" for v in ("_v4", "") for t in ("bf16_t", "float")}
    return n


def test_every_nameable_conv_kernel_has_a_case():
    covered = {_class(c["name"]) for c in CASES}
    assert covered == _nameable(), (sorted(_nameable() - covered), sorted(covered - _nameable()))


def test_big_batch_loops_have_a_case():
    """the loops only the benchmark's batch reached before: each has a case whose NAME (asserted against the reporter in run_*)
    says so"""
    ids = {c["id"] for c in CASES}
    assert {"direct-32-32-k5-d0-walk", "direct-64-64-k3-d1-walk", "dw-nchw-plane-ppw4", "dw-wgrad-nchw-plane-ppw4", "dw-nchw-multi",
            "dw-wgrad-nchw-multi", "c1-wgrad-rows-k5-H27", "c1-wgrad-rows-mfma-H30", "tok-tile-tpw2", "dw-wgrad-nchw-chan-two-passes"} <= ids


def _params(cases):
    return [pytest.param(c, id=c["id"], marks=[pytest.mark.slow] if c["slow"] else []) for c in cases]


def _run(dev_, case, regime, monkeypatch):
    for k in ("CENET_CONV_DIRECT_GRID", "CENET_WGRAD_GRID", "CENET_C1_WGS", "CENET_DW_TPW"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    case["fn"](dev_, regime)


@pytest.mark.parametrize("case", _params([c for c in CASES if c["exact"] and not c["gpu_only"]]))
def test_conv_exact(dev, case, monkeypatch):
    _run(dev, case, "exact", monkeypatch)


@pytest.mark.parametrize("regime", ["normal", "offset"])
@pytest.mark.parametrize("case", _params([c for c in CASES if c["bound"] and not c["gpu_only"]]))
def test_conv_bound(dev, case, regime, monkeypatch):
    _run(dev, case, regime, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["exact", "offset"])
@pytest.mark.parametrize("case", _params([c for c in CASES if c["gpu_only"]]))
def test_conv_direct_natural_multi_tile_walk(case, regime, monkeypatch):
    """more tiles than workgroup slots (512; 256 for 64 -> 64) without the aid: the MI355X only (minutes on the host checker)"""
    from backend import use_hip
    try:
        _run(use_hip(), case, regime, monkeypatch)
    finally:
        _lib._LIB, _lib._HOSTSIM = None, False


# ---- argument contracts --------------------------------------------------------------------------------------------------------
def test_conv_direct_refuses_a_misaligned_output(dev):
    x = torch.zeros(2 * 32 * 8 * 32 + 8, dtype=BF, device=dev)
    y = torch.zeros_like(x)
    w = torch.zeros(32, 32, 5, 5, device=dev)
    assert _lib.lib().cenet_conv_direct_bf16(kern.P(x), kern.P(w), kern.P(y[2:]), 1, 32, 32, 8, 32, 5, 0, kern.stream()) == 1  # CENET_EINVAL


def test_tiled_tok_refuses_flip_with_bias_or_activation(dev):
    x = torch.zeros(1, 49, 8, dtype=BF, device=dev)
    y, a = torch.zeros_like(x), torch.zeros_like(x)
    w, b = torch.zeros(8, 9, device=dev), torch.zeros(8, device=dev)
    args = lambda bias, act_out: (kern.P(x), kern.P(w), kern.P(bias), kern.P(y), kern.P(act_out), 1, 8, 7, 7, 1, 0,  # noqa: E731
                                  0.0, kern.stream())
    assert _lib.lib().cenet_dwconv3x3_tok_bf16(*args(b, None)) == 2      # CENET_EUNSUPPORTED
    assert _lib.lib().cenet_dwconv3x3_tok_bf16(*args(None, a)) == 2
    assert _lib.lib().cenet_dwconv3x3_tok_bf16(*args(None, None)) == 0


# ---- mutation self-test: no kernel involved ------------------------------------------------------------------------------------
def _trunc_bf16(x64):
    return (x64.float().view(torch.int32) & -65536).view(torch.float32).to(BF)


def _as_output(wrong64, exp, truncate=False):
    conv = _trunc_bf16 if truncate else (lambda v: v.float().to(exp.out_dtype))
    return torch.where(exp.own, conv(wrong64), exp.prev_raw)


def _scatter(exp, val):
    C = exp.C.clone()
    C[exp.idx.reshape(-1)] = val.reshape(-1)
    return C


def _mut_dw(regime, B=2, C=6, H=7, W=10, dil=2, flip=True, seed=31):
    g = torch.Generator().manual_seed(seed)
    x = _vals((B, C, H, W), g, regime)
    w, bv = _chan_weights(C, g, regime)
    if regime != "exact":
        bv = bv + 4.0
    yb, yo, sy = _dest((B, C, H, W), torch.device("cpu"), BF, lead=8, pad=4)
    ref, mag, K = R.dw3x3(x, w, bv, dil, flip)
    return x, w, bv, R.expect(yb, yo, x.shape, _nchw(x.shape, sy), ref, mag, K), ref


def _mut_ppw(regime):
    """the ppw > 1 shape: workgroup 512 holds channels 2048, 2049 of image 0 and 0, 1 of image 1"""
    return _mut_dw(regime, B=2, C=2050, H=4, W=4, dil=1, flip=False)


def _mutated(name, regime):
    """-> (expectation, what a kernel with the defect would have left in the buffer)"""
    cpu = torch.device("cpu")
    if name in ("drop_tap_ragged_column", "flip_ignored", "dilation_y_off_by_one", "bias_last_channel"):
        x, w, bv, exp, ref = _mut_dw(regime)
        wrong = ref.clone()
        if name == "drop_tap_ragged_column":  # tap (ky 1, kx 0) of the last column: reads x - dil, inside the image
            wrong[..., -1] -= (w[None, :, 8 - 3, None, None] * R._shift(x.double(), 0, -2))[..., -1]
        elif name == "flip_ignored":
            wrong = R.dw3x3(x, w, bv, 2, False)[0]
        elif name == "dilation_y_off_by_one":
            wrong = bv.double()[None, :, None, None].expand(x.shape).clone()
            for t in range(9):
                wrong = wrong + w.double()[None, :, 8 - t, None, None] * R._shift(x.double(), (t // 3 - 1) * 3, (t % 3 - 1) * 2)
        elif name == "bias_last_channel":
            wrong[:, -1] -= bv[-1].double()
        return exp, _as_output(_scatter(exp, wrong), exp)
    if name == "weight_of_next_channel":
        x, w, bv, exp, ref = _mut_ppw(regime)
        w2 = w.clone()
        w2[2048] = w[2049]
        wrong = ref.clone()
        wrong[0, 2048] = R.dw3x3(x[:1, 2048:2049], w2[2048:2049], bv[2048:2049], 1, False)[0][0, 0]
        return exp, _as_output(_scatter(exp, wrong), exp)
    g = torch.Generator().manual_seed(37)
    if name in ("halo_of_neighbouring_tile", "truncate"):  # (800-term sums: most need rounding to bf16 in the exact regime too)
        x, w = _vals((1, 32, 11, 70), g, regime), _vals((32, 32, 5, 5), g, regime)
        yb, yo, sy = _dest((1, 32, 11, 70), cpu, BF, lead=4)
        ref, mag, K = R.conv_same(x, w, 5)
        exp = R.expect(yb, yo, x.shape, _nchw(x.shape, sy), ref, mag, K, tile=(8, 32))
        wrong = ref.clone()
        if name == "truncate":
            return exp, _as_output(exp.C, exp, truncate=True)
        wrong[..., :8, 32:64] = ref[..., :8, 0:32]  # tile (0, 1) computed from the halo staged for tile (0, 0)
        return exp, _as_output(_scatter(exp, wrong), exp)
    x, dy = _vals((2, 32, 10, 40), g, regime), _vals((2, 32, 10, 40), g, regime)
    db, do = _acc((32, 32, 5, 5), cpu, g, regime)
    ref, mag, K = R.conv_wgrad(x, dy, 5)
    exp = R.expect(db, do, (32, 32, 5, 5), (800, 25, 5, 1), ref, mag, K, add=True, dims=("co", "ci", "ky", "kx"))
    prev = db[do:do + ref.numel()].view(ref.shape).double()
    if name == "wgrad_tile_twice":
        dy2 = torch.zeros_like(dy)
        dy2[1, :, 8:, 32:] = dy[1, :, 8:, 32:]  # the last (ragged) tile once more
        wrong = prev + ref + R.conv_wgrad(x, dy2, 5)[0]
    else:
        assert name == "overwrite_instead_of_add"
        wrong = ref
    return exp, _as_output(_scatter(exp, wrong), exp)


MUTATIONS = ["drop_tap_ragged_column", "halo_of_neighbouring_tile", "weight_of_next_channel", "flip_ignored", "dilation_y_off_by_one",
             "bias_last_channel", "wgrad_tile_twice", "overwrite_instead_of_add", "truncate"]


@pytest.mark.parametrize("name", MUTATIONS)
def test_conv_mutations_are_rejected(name):
    """the acceptance rules fed deliberately wrong references: both regimes reject every one of the table in the module docstring,
    and both accept the unmutated reference"""
    exp, got = _mutated(name, "exact")
    R.assert_exact(_as_output(exp.C, exp), exp, "unmutated")
    with pytest.raises(AssertionError):
        R.assert_exact(got, exp, name)
    exp, got = _mutated(name, "offset")
    assert R.assert_bound(_as_output(exp.C, exp), exp, "unmutated") <= 1.0
    with pytest.raises(AssertionError):
        R.assert_bound(got, exp, name)


def test_failure_report_names_element_and_tile():
    exp, got = _mutated("halo_of_neighbouring_tile", "exact")
    with pytest.raises(AssertionError, match=r"image 0, channel \d+, y \d+, x 3\d\), 8 x 32 tile \(0, 1\)"):
        R.assert_exact(got, exp, "report")


CONV_SHAPES = [(32, 32, 5, 11, 70), (64, 64, 3, 11, 70), (64, 32, 3, 19, 104), (32, 64, 3, 16, 64), (1, 32, 5, 19, 30), (1, 12, 3, 7, 9),
               (1, 12, 1, 7, 9), (64, 16, 1, 7, 7), (40, 40, 1, 8, 8), (1, 1, 3, 64, 68)]
WGRAD_SHAPES = [(2, 32, 32, 5, 10, 40), (2, 64, 32, 3, 6, 33), (2, 1, 32, 5, 27, 30), (9, 1, 3, 3, 28, 28), (2, 1, 12, 1, 19, 30),
                (1, 64, 2, 1, 41, 50)]


def test_conv_constants_are_the_host_measurement():
    """C_ACC / C_OUT stay gemm_ref's because the host measurement over the conv shapes of this matrix, x 4, stays under them; the
    values conv_ref records are pinned: the measurement must reproduce them.  Never measured on a kernel."""
    r_acc, r_out, r_dg = R.measure_constants(CONV_SHAPES, WGRAD_SHAPES)
    print(f"measured on the host: accumulation {r_acc:.3f}, store {r_out:.4f}, gelu' sensitivity {r_dg:.4f}")
    assert r_acc == pytest.approx(R.MEASURED_ACC, abs=0.01) and r_out == pytest.approx(R.MEASURED_OUT, abs=0.0005)
    assert r_dg == pytest.approx(R.MEASURED_DGELU, abs=0.0005) and r_dg == pytest.approx(2.0 / math.sqrt(2.0 * math.pi), abs=1e-4)
    assert 4.0 * R.MEASURED_ACC < R.C_ACC == 2.3 and R.MEASURED_OUT <= R.C_OUT == 1.0 < 2.0
    assert R.MEASURED_DGELU <= R.L_DGELU == 0.8
