"""LayerNorm and train-mode BatchNorm (norm.hip), kernel by kernel, held per element to the float64 reference of tests/norm_ref.py.

* CASES: one case per name `kern.last_norm_kernel()` can report (the dispatchers are host code: the name is asserted on the host checker
  as on the MI355X), fp32 and bf16, at the smallest shape that selects it, plus the branches no other test reaches: steps = 2 in the
  16-byte LayerNorm kernels, S > 1 splits and chunks > 1 in the BatchNorm kernels, misaligned pointers that must fall out of the vector
  forms, padded batch strides and channel slices of a wider tensor.  Destinations sit in sentinel-filled buffers with a lead offset (and
  the other channels of the wider tensor around a slice), operands in NaN-filled ones: nothing outside the footprint may change
  (bitwise).  The set of covered names is held equal to what the dispatcher rules can produce (`_nameable`).
* data regimes, each on every case: normal 0.3 + 1.5 N; offset 8 + 0.25 N; constant (one row / channel constant: var = 0; integer
  cotangents and integer previous dbeta, so that dbeta is EXACT where there is no activation); and, for the forms that compute batch
  statistics, outlier-first: the offset regime with x[0, c, 0] = 0 -- the element the one-pass kernels used to shift their sums by.
* mutation self-test (no kernel): deliberately wrong REFERENCES must be rejected by the rule, in the normal and the offset regime.
      mutation                                            rejected by
      unbiased instead of biased batch variance           var bound (1 / n of var against 2^-24 sqrt(n) var)
      running variance without n / (n - 1)                running-variance bound (m var / n against m n/(n-1) b_var)
      momentum applied to the wrong operand               running-mean bound
      eps dropped on the constant channel                 y: not finite
      statistics from the first split only                mean bound (sigma / sqrt(n) against 2^-24 sqrt(n) E|x|)
      mean(g) term dropped from dx                        dx bound
      mean(g xh) term dropped for one ragged chunk        dx bound on the chunk's elements (fp32 destination)
      dgamma overwritten instead of added to              dgamma bound (the previous contents are part of the reference)
      act' taken from the wrong side for lrelu            dx bound (and dbeta, dgamma)
      dx_add ignored                                      dx bound
      one LayerNorm row normalised with its neighbour's rstd      y bound on that row
      truncation instead of round-to-nearest (bf16)       y bound (up to 2 u_out: C_OUT may not reach 2)
`sim` = the kernel sources on the host SIMT checker (CPU); `hip` = the gfx950 library (marker gpu)."""
import math

import pytest
import torch

import norm_ref as R
from backend import dev  # noqa: F401
from cenet_amd import _lib, kern

BF, F32 = torch.bfloat16, torch.float32
SENTINEL = 12288.0  # exact in bf16
NAN = float("nan")
LN_EPS, BN_EPS, SLOPE, MOM = 1e-6, 1e-5, 0.25, 0.1


def _sync(d):
    if d.type == "cuda":
        torch.cuda.synchronize()


def _tn(dt):
    return "bf16_t" if dt == BF else "float"


# ---- data ------------------------------------------------------------------------------------------------------------------------
def _data(shape, g, regime, const_dim):
    """bf16-exact values; constant: index 1 (0 if there is one only) along `const_dim` is 1.75 everywhere; outlier: the first element
    of every plane of image 0 (the offset regime otherwise) is 0"""
    m, s = (8.0, 0.25) if regime in ("offset", "outlier") else (0.3, 1.5)
    x = (m + s * R.reals(shape, g)).to(BF).float()
    if regime == "constant":
        x.select(const_dim, min(1, shape[const_dim] - 1)).fill_(1.75)
    if regime == "outlier":
        x[0, :, 0] = 0.0
    return x


def _cot(shape, g, regime):
    return R.ints(shape, g) if regime == "constant" else R.reals(shape, g).to(BF).float()


def _affine(C, g):
    """gamma of both signs away from 0, beta away from 0 (beta = 0 with symmetric data would put relu's kink in the data's middle)"""
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 2, -1.0, 1.0)
    beta = 0.3 + 0.2 * R.reals((C,), g)
    return gamma, beta


def _buf(x, d, dtype, lead, fill, sb=None, tail=16):
    """x [B, n] -> (flat buffer, lead): images `sb` elements apart (default n), surrounded by `fill`"""
    B, n = x.shape
    sb = n if sb is None else sb
    buf = torch.full((lead + B * sb + tail,), fill, dtype=F32)
    buf[lead:lead + B * sb].view(B, sb)[:, :n] = x
    return buf.to(dtype).to(d)


def _acc(prev, d, lead=4):
    """an fp32 accumulator ("ADDED into") with previous contents inside a sentinel-filled buffer"""
    return _buf(prev.reshape(1, -1), d, F32, lead, SENTINEL), lead


def _prev(C, g, regime):
    return R.ints((C,), g) if regime == "constant" else torch.full((C,), 0.75)


def _report(name, regime, worst, worst32):
    """(bf16 destinations sit at ~0.99 by construction: the store's half ulp against C_OUT u_out |ref|; the fp32 ones show the sums)"""
    print(f"BOUND {name} [{regime}]: worst |err| / bound = {worst:.3f}, fp32 outputs {worst32:.3f}")


def _named(expected, cls):
    got = kern.last_norm_kernel()
    assert got == expected, (got, expected)
    assert _class(got) == cls, (_class(got), cls)


RUNTIME = ("S=", "threads=", "chunks=", "steps=", "items=")


def _class(name):
    """a reported name without its run-time numbers (S, threads, chunks, steps, items)"""
    return "+".join(" ".join(t for t in part.split(" ") if not t.startswith(RUNTIME)) for part in name.split("+"))


# ---- LayerNorm: the dispatcher rules ---------------------------------------------------------------------------------------------
def _ln_steps(rows, rps, target):
    return max(1, min(8, rows // (rps * target)))


def _ln_fwd_name(dt, rows, C, aligned):
    if C % 4 == 0 and C <= 512 and aligned:
        lpr, np_ = (16, 1) if C <= 64 else (32, 1) if C <= 128 else (64, 1) if C <= 256 else (64, 2)
        return f"ln_fwd_v4_kernel<{_tn(dt)}, {lpr}, {np_}> steps={_ln_steps(rows, 256 // lpr, 1024)}"
    return f"layernorm_fwd_kernel<{_tn(dt)}>"


def _ln_bwd_name(dt, rows, C, aligned16, aligned_quad):
    """aligned16: dy, x, dx, dx_add 16-byte aligned (the 8-channel form); aligned_quad: to four elements (the quad form)"""
    if dt == BF and C % 8 == 0 and aligned16:
        lpr = 8 if C <= 64 else 16 if C <= 128 else 32 if C <= 256 else 64
        return f"ln_bwd_v8_kernel<{lpr}, 1> steps={_ln_steps(rows, 256 // lpr, 256)}"
    if C % 4 == 0 and aligned_quad:
        lpr, np_ = (16, 1) if C <= 64 else (32, 1) if C <= 128 else (64, 1) if C <= 256 else (64, 2)
        return f"ln_bwd_v4_kernel<{_tn(dt)}, {lpr}, {np_}> steps={_ln_steps(rows, 256 // lpr, 256 if dt == BF else 1024)}"
    mj, rp = (1, 4) if C <= 64 else (2, 4) if C <= 128 else (4, 2) if C <= 256 else (8, 1)
    return f"layernorm_bwd_kernel<{_tn(dt)}, {mj}, {rp}>"


def _ln_part_name(rows, C, dxs):
    lpr = 8 if C <= 64 else 16 if C <= 128 else 32 if C <= 256 else 64
    return f"ln_bwd_v8_kernel<{lpr}, 1> part dxs={int(dxs)} steps={_ln_steps(rows, 256 // lpr, 1024)}"


def _rows_ok(exp_list, regime, name):
    worst = worst32 = 0.0
    for got, exp in exp_list:
        w = R.assert_bound(got, exp, name)
        worst = max(worst, w)
        if exp.out_dtype == F32:
            worst32 = max(worst32, w)
    _report(name, regime, worst, worst32)
    return worst


def run_ln_fwd(d, regime, cls, dt, rows, C, xlead=8, has=()):
    g = torch.Generator().manual_seed(rows * 1000 + C)
    x = _data((rows, C), g, regime, 0)
    gamma, beta = _affine(C, g)
    xb = _buf(x.reshape(1, -1), d, dt, xlead, NAN)
    yb = _buf(torch.full((1, rows * C), SENTINEL), d, dt, 8, SENTINEL)
    mb, rb = (_buf(torch.full((1, rows), SENTINEL), d, F32, 4, SENTINEL) for _ in range(2))
    gd, bd = gamma.to(d), beta.to(d)
    o = R.ln_fwd(R.view(xb, xlead, (rows, C), (C, 1)), gd, bd, LN_EPS)
    name = _ln_fwd_name(dt, rows, C, xlead % 4 == 0)
    assert all(h in name for h in has), (name, has)
    exps = [(yb, R.as_exp(yb, 8, (rows, C), (C, 1), o["y"], kernel=name)),
            (mb, R.as_exp(mb, 4, (rows,), (1,), o["mean"], dims=("row",), kernel=name + " mean")),
            (rb, R.as_exp(rb, 4, (rows,), (1,), o["rstd"], dims=("row",), kernel=name + " rstd"))]
    kern.layernorm_fwd(xb[xlead:], gd, bd, yb[8:], mb[4:], rb[4:], rows, C, LN_EPS)
    _sync(d)
    _named(name, cls)
    return _rows_ok(exps, regime, name)


def _ln_operands(d, regime, dt, rows, C, g, add, alead):
    x = _data((rows, C), g, regime, 0)
    dy = _cot((rows, C), g, regime)
    gamma, _ = _affine(C, g)
    st = R.stats(x.double(), (1,))
    mean, rstd = st.mu[:, 0].float().to(d), ((st.var[:, 0] + LN_EPS) ** -0.5).float().to(d)  # operands of the backward: given
    xb, gb = _buf(x.reshape(1, -1), d, dt, 8, NAN), _buf(dy.reshape(1, -1), d, dt, 8, NAN)
    ab = _buf(R.reals((1, rows * C), g).to(BF).float(), d, dt, alead, NAN) if add else None
    dxb = _buf(torch.full((1, rows * C), SENTINEL), d, dt, 8, SENTINEL)
    v = lambda b, lead: R.view(b, lead, (rows, C), (C, 1))  # noqa: E731
    o = R.ln_bwd(v(gb, 8), v(xb, 8), gamma.to(d), mean, rstd, v(ab, alead) if add else None)
    return xb, gb, ab, dxb, gamma.to(d), mean, rstd, o


def _exact_dbeta(got, prev, o, regime, what):
    if regime == "constant":
        want = prev.double().to(o.ref.device) + o.ref
        assert float(o.mag.max()) + float(prev.abs().max()) < R.EXACT_LIMIT
        assert torch.equal(got.double(), want), f"{what}: dbeta of integer cotangents is not the exact sum"


def run_ln_bwd(d, regime, cls, dt, rows, C, add=False, alead=8, has=()):
    g = torch.Generator().manual_seed(rows * 1000 + C + 7)
    xb, gb, ab, dxb, gamma, mean, rstd, o = _ln_operands(d, regime, dt, rows, C, g, add, alead)
    pg, pb = _prev(C, g, regime), _prev(C, g, regime)
    (dgb, gl), (dbb, bl) = _acc(pg, d), _acc(pb, d)
    name = _ln_bwd_name(dt, rows, C, alead * (2 if dt == BF else 4) % 16 == 0, alead % 4 == 0)
    assert all(h in name for h in has), (name, has)
    exps = [(dxb, R.as_exp(dxb, 8, (rows, C), (C, 1), o["dx"], kernel=name)),
            (dgb, R.as_exp(dgb, gl, (C,), (1,), o["dgamma"], add=True, dims=("column",), kernel=name + " dgamma")),
            (dbb, R.as_exp(dbb, bl, (C,), (1,), o["dbeta"], add=True, dims=("column",), kernel=name + " dbeta"))]
    kern.layernorm_bwd(gb[8:], xb[8:], gamma, mean, rstd, dxb[8:], dgb[gl:], dbb[bl:], rows, C, dx_add=ab[alead:] if add else None)
    _sync(d)
    _named(name, cls)
    _exact_dbeta(dbb[bl:bl + C].cpu(), pb, R.Out(o["dbeta"].ref.cpu(), o["dbeta"].mag.cpu(), rows), regime, name)
    return _rows_ok(exps, regime, name)


def run_ln_part(d, regime, cls, rows, C, add, scaled, rows2=0, C2=0, has=()):
    """the deferred form: dx (+ dxs) and a partial buffer per item, then ONE fold for all items (a second item of another shape)"""
    g = torch.Generator().manual_seed(rows * 1000 + C + 13)
    items, exps, names = [], [], []
    for (r_, c_) in ((rows, C), (rows2, C2)):
        if r_ == 0:
            continue
        xb, gb, ab, dxb, gamma, mean, rstd, o = _ln_operands(d, regime, BF, r_, c_, g, add, 8)
        assert kern.layernorm_bwd_part_supported(gb[8:], xb[8:], c_)
        name = _ln_part_name(r_, c_, scaled)
        nsamp = 2 if r_ % 2 == 0 else 1
        bscale = torch.tensor([0.5, 1.25][:nsamp]).to(d) if scaled else None
        dxs = _buf(torch.full((1, r_ * c_), SENTINEL), d, BF, 8, SENTINEL) if scaled else None
        dxs0 = dxs.clone() if scaled else None
        part = kern.layernorm_bwd_part(gb[8:], xb[8:], gamma, mean, rstd, dxb[8:], r_, c_, dx_add=ab[8:] if add else None,
                                       bscale=bscale, dxs=dxs[8:] if scaled else None)
        _sync(d)
        _named(name, cls if not names else _class(name))
        exps.append((dxb, R.as_exp(dxb, 8, (r_, c_), (c_, 1), o["dx"], kernel=name)))
        if scaled:  # dxs = bscale[sample] * the STORED dx, rounded once
            stored = dxb[8:8 + r_ * c_].view(r_, c_).double() * bscale.double().repeat_interleave(r_ // nsamp)[:, None]
            exps.append((dxs, R.as_exp(dxs0, 8, (r_, c_), (c_, 1), R.Out(stored, stored.abs(), 1), kernel=name + " dxs")))
        pg, pb = _prev(c_, g, regime), _prev(c_, g, regime)
        (dgb, gl), (dbb, bl) = _acc(pg, d), _acc(pb, d)
        fg, fb = R.ln_fold(part, c_)  # the fold alone, from the partial rows the kernel wrote
        items.append((part, dgb, gl, dbb, bl, pb, o, c_, r_, name,
                      R.as_exp(dgb, gl, (c_,), (1,), fg, add=True, dims=("column",), kernel="fold dgamma"),
                      R.as_exp(dbb, bl, (c_,), (1,), fb, add=True, dims=("column",), kernel="fold dbeta"),
                      R.as_exp(dgb, gl, (c_,), (1,), o["dgamma"], add=True, dims=("column",), kernel=name + " dgamma"),
                      R.as_exp(dbb, bl, (c_,), (1,), o["dbeta"], add=True, dims=("column",), kernel=name + " dbeta")))
        names.append(name)
    assert all(h in names[0] for h in has), (names, has)
    kern.ln_fold_group([(it[0], it[1][it[2]:it[2] + it[7]], it[3][it[4]:it[4] + it[7]]) for it in items])
    _sync(d)
    assert kern.last_norm_kernel() == f"ln_fold_group_kernel items={len(items)}"
    for (part, dgb, gl, dbb, bl, pb, o, c_, r_, name, e1, e2, e3, e4) in items:
        exps += [(dgb, e1), (dbb, e2), (dgb, e3), (dbb, e4)]
        _exact_dbeta(dbb[bl:bl + c_].cpu(), pb, R.Out(o["dbeta"].ref.cpu(), o["dbeta"].mag.cpu(), r_), regime, name)
    return _rows_ok(exps, regime, names[0])


def run_ln_acc(d, regime, cls, rows, C, bias):
    g = torch.Generator().manual_seed(rows * 1000 + C + 17)
    acc = _data((rows, C), g, regime, 0) + (R.reals((rows, C), g) * 2.0 ** -9 if regime != "constant" else 0.0)  # not bf16 values
    bv = (0.5 * R.reals((C,), g)).to(d) if bias else None
    if regime == "constant" and bias:
        bv = torch.full((C,), 0.25).to(d)
    gamma, beta = _affine(C, g)
    accb = _buf(acc.reshape(1, -1), d, F32, 4, SENTINEL)
    xpb, yb = (_buf(torch.full((1, rows * C), SENTINEL), d, BF, 4, SENTINEL) for _ in range(2))
    mb, rb = (_buf(torch.full((1, rows), SENTINEL), d, F32, 4, SENTINEL) for _ in range(2))
    pre = R.ln_acc_pre(R.view(accb, 4, (rows, C), (C, 1)), bv)
    e_pre = R.as_exp(xpb, 4, (rows, C), (C, 1), pre, kernel="ln_fwd_acc_kernel xpre")
    acc_before, yb0, mb0, rb0 = accb.clone(), yb.clone(), mb.clone(), rb.clone()  # (what "unchanged" means for the outputs checked below)
    kern.layernorm_fwd_acc(accb[4:], bv, xpb[4:], gamma.to(d), beta.to(d), yb[4:], mb[4:], rb[4:], rows, C, LN_EPS)
    _sync(d)
    _named("ln_fwd_acc_kernel", cls)
    own = torch.zeros(accb.numel(), dtype=torch.bool, device=d)
    own[4:4 + rows * C] = True
    bits, before = accb.view(torch.int32), acc_before.view(torch.int32)
    assert bool((bits[own] == 0).all()), "the accumulator is not all +0 after the call"
    assert torch.equal(bits[~own], before[~own]), "elements around the accumulator changed"
    o = R.ln_fwd(R.view(xpb, 4, (rows, C), (C, 1)), gamma.to(d), beta.to(d), LN_EPS)  # statistics of the ROUNDED rows the kernel stored
    exps = [(xpb, e_pre), (yb, R.as_exp(yb0, 4, (rows, C), (C, 1), o["y"], kernel="ln_fwd_acc_kernel y")),
            (mb, R.as_exp(mb0, 4, (rows,), (1,), o["mean"], dims=("row",), kernel="ln_fwd_acc_kernel mean")),
            (rb, R.as_exp(rb0, 4, (rows,), (1,), o["rstd"], dims=("row",), kernel="ln_fwd_acc_kernel rstd"))]
    return _rows_ok(exps, regime, "ln_fwd_acc_kernel")


# ---- BatchNorm: the dispatcher rules ---------------------------------------------------------------------------------------------
def _splits_v4(C, quads):
    return max(1, min(2048 // C, (quads + 1023) // 1024, 255))


def _splits(C, total):
    return max(1, min(max(1, 1024 // C), (total + 2047) // 2048, 255))


def _plane(nq):
    th = 64 if nq <= 64 else 128 if nq <= 128 else 256
    return th, max(1, min(16, -(-nq // (th * 2))))


def _quad(HW, *off_stride):
    return HW % 4 == 0 and all(o % 4 == 0 and s % 4 == 0 for o, s in off_stride)


def _partial_name(dt, B, C, HW, xo, sxb):
    if _quad(HW, (xo, sxb)):
        return f"bn_partial_v4_kernel<{_tn(dt)}> S={_splits_v4(C, B * HW // 4)}"
    if dt == BF and HW <= 1024:
        return f"bn_partial_flat_kernel<bf16_t> S={_splits(C, B * HW)}"
    return f"bn_partial_kernel<{_tn(dt)}> S={_splits(C, B * HW)}"


def _apply_name(dt, B, C, HW, xo, sxb, yo, syb, fin):
    v4 = _quad(HW, (xo, sxb), (yo, syb))
    if dt == BF and HW <= 1024 and sxb == C * HW and syb == C * HW:
        return f"bn_apply_flat_kernel<bf16_t, {4 if v4 else 1}> fin={fin}"
    if v4:
        th, ch = _plane(HW // 4)
        return f"bn_apply_v4_kernel<{_tn(dt)}> fin={fin} threads={th} chunks={ch}"
    return f"bn_apply_kernel<{_tn(dt)}> fin={fin} chunks={min(64, -(-HW // 1024))}"


def _train_name(dt, B, C, HW, xo, sxb, yo, syb):
    if dt == BF and 2 <= B * HW <= 2048:
        return "bn_train_fwd_1k_kernel"
    if dt == BF:
        return _partial_name(dt, B, C, HW, xo, sxb) + "+" + _apply_name(dt, B, C, HW, xo, sxb, yo, syb, 1)
    return _partial_name(dt, B, C, HW, xo, sxb) + "+bn_finalize_kernel<float>+" + _apply_name(dt, B, C, HW, xo, sxb, yo, syb, 0)


def _bwd_name(dt, B, C, HW, go, sgb, xo, sxb, do, sdb, ao=None, sab=0):
    if dt == BF and B * HW <= 2048:
        return "bn_bwd_1k_kernel"
    v4 = _quad(HW, (go, sgb), (xo, sxb), (do, sdb), (ao or 0, sab))
    t = _tn(dt)
    if dt == BF and HW <= 1024 and sgb == sxb == sdb == C * HW and (ao is None or sab == C * HW):
        S = _splits_v4(C, B * HW // 4) if v4 else _splits(C, B * HW)
        return f"bn_bwd_partial_{'v4' if v4 else 'flat'}_kernel<bf16_t> S={S}+bn_bwd_apply_flat_kernel<bf16_t, {4 if v4 else 1}>"
    if v4:
        th, ch = _plane(HW // 4)
        return f"bn_bwd_partial_v4_kernel<{t}> S={_splits_v4(C, B * HW // 4)}+bn_bwd_apply_v4_kernel<{t}> threads={th} chunks={ch}"
    return f"bn_bwd_partial_kernel<{t}> S={_splits(C, B * HW)}+bn_bwd_apply_kernel<{t}> chunks={min(64, -(-HW // 1024))}"


def _wide(x, d, dt, lead, Ctot, c0, pad, fill):
    """x [B, C, HW] as channels [c0, c0 + C) of a [B, Ctot, HW] tensor whose images lie Ctot HW + pad apart, at `lead` of a buffer
    filled with `fill` -> (buffer, offset of x[0, 0, 0], batch stride)"""
    B, C, HW = x.shape
    sb = Ctot * HW + pad
    buf = torch.full((lead + B * sb + 16,), fill, dtype=F32)
    buf[lead:lead + B * sb].view(B, sb)[:, c0 * HW:(c0 + C) * HW] = x.reshape(B, C * HW)
    return buf.to(dt).to(d), lead + c0 * HW, sb


def _vecdest(C, d, prev=None):
    p = torch.full((C,), SENTINEL) if prev is None else prev
    return _buf(p.reshape(1, -1), d, F32, 4, SENTINEL)


def _ws(C, d):
    """CENET_BN_WS_FLOATS(C) floats of scratch (NaN: nothing may be read before it is written) and a guarded tail"""
    ws = torch.full((2 * C * 256 + 16,), NAN)
    ws[2 * C * 256:] = SENTINEL
    return ws.to(d)


def _ws_tail_ok(ws, C):
    assert bool((ws[2 * C * 256:] == SENTINEL).all()), "the workspace was written beyond CENET_BN_WS_FLOATS(C)"


def run_bn_fwd(d, regime, cls, dt, B, C, HW, act="none", xlead=8, ylead=8, Ctot=None, c0=0, pad=0, entry="train", running=True,
               nbt_n=1, has=()):
    """entry train: cenet_bn_train_fwd; split: cenet_bn_stats, then cenet_bn_apply on the statistics of the reference"""
    g = torch.Generator().manual_seed(B * 100003 + C * 1009 + HW)
    Ctot = C if Ctot is None else Ctot
    x = _data((B, C, HW), g, regime, 1)
    gamma, beta = _affine(C, g)
    xb, xo, sxb = _wide(x, d, dt, xlead, Ctot, c0, pad, NAN)
    yb, yo, syb = _wide(torch.full((B, C, HW), SENTINEL), d, dt, ylead, Ctot, c0, pad, SENTINEL)
    shape, xs, ys = (B, C, HW), (sxb, HW, 1), (syb, HW, 1)
    xv = R.view(xb, xo, shape, xs)
    prm, prv = 0.2 * R.reals((C,), g), torch.rand(C, generator=g) + 0.5
    mb, vb = _vecdest(C, d), _vecdest(C, d)
    rmb, rvb = (_vecdest(C, d, prm), _vecdest(C, d, prv)) if running else (None, None)
    nbt = torch.tensor([3, 5, 7, 11][:nbt_n + 1], dtype=torch.int64).to(d) if running else None
    ws = _ws(C, d)
    gd, bd = gamma.to(d), beta.to(d)
    st = R.bn_stats(xv, prm.to(d) if running else None, prv.to(d) if running else None, MOM)
    dims = ("image", "channel", "pixel")
    stat_exps = [(mb, R.as_exp(mb, 4, (C,), (1,), st["mean"], dims=("channel",), kernel="mean")),
                 (vb, R.as_exp(vb, 4, (C,), (1,), st["var"], dims=("channel",), kernel="var"))]
    if running:
        stat_exps += [(rmb, R.as_exp(rmb, 4, (C,), (1,), st["rmean"], dims=("channel",), kernel="running mean")),
                      (rvb, R.as_exp(rvb, 4, (C,), (1,), st["rvar"], dims=("channel",), kernel="running var"))]
    sq = lambda t: t[0, :, 0]  # noqa: E731
    rm_, rv_ = (rmb[4:], rvb[4:]) if running else (None, None)
    if entry == "train":
        name = _train_name(dt, B, C, HW, xo, sxb, yo, syb)
        y, _, _ = R.bn_fwd(xv, sq(st["st"].mu), sq(st["st"].var), gd, bd, BN_EPS, act, SLOPE, st["st"].b_mu, st["st"].b_var)
        exps = stat_exps + [(yb, R.as_exp(yb, yo, shape, ys, y, dims=dims, kernel=name))]
        kern.bn_train_fwd(xb[xo:], sxb, yb[yo:], syb, ws, mb[4:], vb[4:], rm_, rv_, MOM, nbt[:nbt_n] if running else None, BN_EPS, gd,
                          bd, act, SLOPE, B, C, HW)
        _sync(d)
        _named(name, cls)
    else:
        assert nbt_n == 1
        name = _partial_name(dt, B, C, HW, xo, sxb) + f"+bn_finalize_kernel<{_tn(dt)}>"
        kern.bn_stats(xb[xo:], sxb, B, C, HW, ws, mb[4:], vb[4:], rm_, rv_, MOM, nbt[:1] if running else None)
        _sync(d)
        _named(name, cls.split("|")[0])
        mean, var = sq(st["st"].mu).float(), sq(st["st"].var).float()  # operands of cenet_bn_apply: given
        y, _, _ = R.bn_fwd(xv, mean, var, gd, bd, BN_EPS, act, SLOPE)
        name2 = _apply_name(dt, B, C, HW, xo, sxb, yo, syb, 0)
        exps = stat_exps + [(yb, R.as_exp(yb, yo, shape, ys, y, dims=dims, kernel=name2))]
        kern.bn_apply(xb[xo:], sxb, yb[yo:], syb, mean, var, BN_EPS, gd, bd, act, SLOPE, B, C, HW)
        _sync(d)
        _named(name2, cls.split("|")[1])
        name = name + "|" + name2
    assert all(h in name for h in has), (name, has)
    if running:
        assert nbt.cpu().tolist() == [v + (i < nbt_n) for i, v in enumerate([3, 5, 7, 11][:nbt_n + 1])], nbt
    _ws_tail_ok(ws, C)
    return _rows_ok(exps, regime, name)


def _amb_ok(o, what):
    frac = float(o["amb"].double().mean())
    assert frac <= 0.01, f"{what}: {frac:.3%} of the elements are ambiguous for the activation's derivative"


def run_bn_bwd(d, regime, cls, dt, B, C, HW, act="none", lead=8, dlead=8, Ctot=None, c0=0, pad=0, add=None, has=()):
    """add: None / "tight" (dx_add contiguous: batch stride C HW) / "wide" (one more channel between the images)"""
    g = torch.Generator().manual_seed(B * 100003 + C * 1009 + HW + 5)
    Ctot = C if Ctot is None else Ctot
    x, dy = _data((B, C, HW), g, regime, 1), _cot((B, C, HW), g, regime)
    gamma, beta = _affine(C, g)
    xb, xo, sxb = _wide(x, d, dt, lead, Ctot, c0, pad, NAN)
    gb, go, sgb = _wide(dy, d, dt, lead, Ctot, c0, pad, NAN)
    dxb, do, sdb = _wide(torch.full((B, C, HW), SENTINEL), d, dt, dlead, Ctot, c0, pad, SENTINEL)
    shape = (B, C, HW)
    ab = ao = None
    sab = 0
    if add:
        ab, ao, sab = _wide(R.reals(shape, g).to(BF).float(), d, dt, 8, C + (add == "wide"), 0, 0, NAN)
    xv = R.view(xb, xo, shape, (sxb, HW, 1))
    st = R.stats(xv.double(), (0, 2))
    mean, var = st.mu[0, :, 0].float(), st.var[0, :, 0].float()  # operands of the backward: given
    gd, bd = gamma.to(d), beta.to(d)
    o = R.bn_bwd(R.view(gb, go, shape, (sgb, HW, 1)), xv, mean, var, gd, bd, BN_EPS, act, SLOPE,
                 R.view(ab, ao, shape, (sab, HW, 1)) if add else None)
    _amb_ok(o, cls)
    pg, pb = _prev(C, g, regime), _prev(C, g, regime)
    (dgb, gl), (dbb, bl) = _acc(pg, d), _acc(pb, d)
    ws = _ws(C, d)
    name = _bwd_name(dt, B, C, HW, go, sgb, xo, sxb, do, sdb, ao, sab)
    assert all(h in name for h in has), (name, has)
    exps = [(dxb, R.as_exp(dxb, do, shape, (sdb, HW, 1), o["dx"], dims=("image", "channel", "pixel"), kernel=name)),
            (dgb, R.as_exp(dgb, gl, (C,), (1,), o["dgamma"], add=True, dims=("channel",), kernel=name + " dgamma")),
            (dbb, R.as_exp(dbb, bl, (C,), (1,), o["dbeta"], add=True, dims=("channel",), kernel=name + " dbeta"))]
    if add == "wide":  # (kern.bn_bwd takes a contiguous dx_add: the strided one goes through the entry point itself)
        kern._call("cenet_bn_bwd_add_acc_f32", kern.Ptr(gb, go), sgb, kern.Ptr(xb, xo), sxb, kern.Ptr(dxb, do),
                   sdb, kern.Ptr(ab, ao), sab, mean, var, BN_EPS, gd, bd, kern.ACT[act], SLOPE, B, C, HW, ws,
                   kern.Ptr(dgb, gl), kern.Ptr(dbb, bl))
    else:
        kern.bn_bwd(gb[go:], sgb, xb[xo:], sxb, dxb[do:], sdb, mean, var, BN_EPS, gd, bd, act, SLOPE, B, C, HW, ws, dgb[gl:], dbb[bl:],
                    dx_add=ab[ao:] if add else None)
    _sync(d)
    _named(name, cls)
    if act == "none":
        _exact_dbeta(dbb[bl:bl + C].cpu(), pb, R.Out(o["dbeta"].ref.cpu(), o["dbeta"].mag.cpu(), B * HW), regime, name)
    _ws_tail_ok(ws, C)
    return _rows_ok(exps, regime, name)


def run_bn1d(d, regime, cls, B, C, running=True):
    g = torch.Generator().manual_seed(B * 1009 + C)
    z = _data((B, C, 1), g, regime, 1)
    gamma, beta = _affine(C, g)
    zb = _buf(z.reshape(1, -1), d, F32, 4, NAN)
    shape, strides = (B, C, 1), (C, 1, 1)
    zv = R.view(zb, 4, shape, strides)
    prm, prv = 0.2 * R.reals((C,), g), torch.rand(C, generator=g) + 0.5
    znb = _buf(torch.full((1, B * C), SENTINEL), d, F32, 4, SENTINEL)
    mb, vb = _vecdest(C, d), _vecdest(C, d)
    rmb, rvb = (_vecdest(C, d, prm), _vecdest(C, d, prv)) if running else (None, None)
    nbt = torch.tensor([3, 5], dtype=torch.int64).to(d) if running else None
    gd, bd = gamma.to(d), beta.to(d)
    st = R.bn_stats(zv, prm.to(d) if running else None, prv.to(d) if running else None, MOM)
    sq = lambda t: t[0, :, 0]  # noqa: E731
    y, _, _ = R.bn_fwd(zv, sq(st["st"].mu), sq(st["st"].var), gd, bd, BN_EPS, "none", 0.0, st["st"].b_mu, st["st"].b_var)
    dims = ("row", "channel", "-")
    exps = [(znb, R.as_exp(znb, 4, shape, strides, y, dims=dims, kernel="bn1d_train_fwd_kernel")),
            (mb, R.as_exp(mb, 4, (C,), (1,), st["mean"], dims=("channel",), kernel="bn1d mean")),
            (vb, R.as_exp(vb, 4, (C,), (1,), st["var"], dims=("channel",), kernel="bn1d var"))]
    if running:
        exps += [(rmb, R.as_exp(rmb, 4, (C,), (1,), st["rmean"], dims=("channel",), kernel="bn1d running mean")),
                 (rvb, R.as_exp(rvb, 4, (C,), (1,), st["rvar"], dims=("channel",), kernel="bn1d running var"))]
    kern.bn1d_train_fwd(zb[4:], znb[4:], mb[4:], vb[4:], rmb[4:] if running else None, rvb[4:] if running else None, MOM,
                        nbt[:1] if running else None, BN_EPS, gd, bd, B, C)
    _sync(d)
    _named("bn1d_train_fwd_kernel", cls)
    if running:
        assert nbt.cpu().tolist() == [4, 5]
    worst = _rows_ok(exps, regime, "bn1d_train_fwd_kernel")
    # backward, on the statistics of the reference
    dy = _cot((B, C, 1), g, regime)
    gb = _buf(dy.reshape(1, -1), d, F32, 4, NAN)
    mean, var = sq(st["st"].mu).float(), sq(st["st"].var).float()
    o = R.bn_bwd(R.view(gb, 4, shape, strides), zv, mean, var, gd, None, BN_EPS, "none", 0.0)
    dzb = _buf(torch.full((1, B * C), SENTINEL), d, F32, 4, SENTINEL)
    pg, pb = _prev(C, g, regime), _prev(C, g, regime)
    (dgb, gl), (dbb, bl) = _acc(pg, d), _acc(pb, d)
    exps = [(dzb, R.as_exp(dzb, 4, shape, strides, o["dx"], dims=dims, kernel="bn1d_bwd_kernel"))]
    if running:  # (the run without running buffers is also the run without parameter gradients: both are optional)
        exps += [(dgb, R.as_exp(dgb, gl, (C,), (1,), o["dgamma"], add=True, dims=("channel",), kernel="bn1d_bwd_kernel dgamma")),
                 (dbb, R.as_exp(dbb, bl, (C,), (1,), o["dbeta"], add=True, dims=("channel",), kernel="bn1d_bwd_kernel dbeta"))]
    else:
        zero = R.Out(torch.zeros(C, dtype=torch.float64, device=d), torch.zeros(C, dtype=torch.float64, device=d), 1)
        exps += [(dgb, R.as_exp(dgb, gl, (C,), (1,), zero, add=True, dims=("channel",), kernel="bn1d_bwd_kernel dgamma (NULL)")),
                 (dbb, R.as_exp(dbb, bl, (C,), (1,), zero, add=True, dims=("channel",), kernel="bn1d_bwd_kernel dbeta (NULL)"))]
    kern.bn1d_bwd(gb[4:], zb[4:], dzb[4:], mean, var, BN_EPS, gd, dgb[gl:] if running else None, dbb[bl:] if running else None, B, C)
    _sync(d)
    _named("bn1d_bwd_kernel", "bn1d_bwd_kernel")
    if running:
        _exact_dbeta(dbb[bl:bl + C].cpu(), pb, R.Out(o["dbeta"].ref.cpu(), o["dbeta"].mag.cpu(), B), regime, "bn1d_bwd_kernel")
    return max(worst, _rows_ok(exps, regime, "bn1d_bwd_kernel"))


# ---- the case matrix -------------------------------------------------------------------------------------------------------------
CASES = []


def _add(cid, cls, fn, stats=False, big=False):
    """cls: the reported name without run-time numbers; stats: the form computes batch statistics (outlier-first applies);
    big: a steps = 2 shape (rows = 2 x rows per step x target + 5, at the narrowest width of the class)"""
    CASES.append(dict(id=cid, cls=cls, fn=fn, stats=stats, big=big))


for dt in (F32, BF):
    t = _tn(dt)
    # LayerNorm forward: the four width classes at their widest and at a ragged width, the scalar fallback, 1 / 37 rows, steps = 2
    for (lpr, np_), (Ca, Cb, Cs) in {(16, 1): (64, 60, 8), (32, 1): (128, 68, 68), (64, 1): (256, 132, 132), (64, 2): (512, 260, 260)}.items():
        cls = f"ln_fwd_v4_kernel<{t}, {lpr}, {np_}>"
        _add(f"ln-fwd-{t}-C{Ca}", cls, lambda d, r, cls=cls, dt=dt, C=Ca: run_ln_fwd(d, r, cls, dt, 37, C, has=("steps=1",)))
        _add(f"ln-fwd-{t}-C{Cb}-row1", cls, lambda d, r, cls=cls, dt=dt, C=Cb: run_ln_fwd(d, r, cls, dt, 1, C))
        rows2 = 2 * (256 // lpr) * 1024 + 5
        _add(f"ln-fwd-{t}-C{Cs}-steps2", cls, lambda d, r, cls=cls, dt=dt, C=Cs, n=rows2: run_ln_fwd(d, r, cls, dt, n, C, has=("steps=2",)),
             big=True)
    cls = f"layernorm_fwd_kernel<{t}>"
    _add(f"ln-fwd-{t}-C50", cls, lambda d, r, cls=cls, dt=dt: run_ln_fwd(d, r, cls, dt, 37, 50))
    _add(f"ln-fwd-{t}-C516", cls, lambda d, r, cls=cls, dt=dt: run_ln_fwd(d, r, cls, dt, 5, 516))
    _add(f"ln-fwd-{t}-C64-offset-by-one", cls, lambda d, r, cls=cls, dt=dt: run_ln_fwd(d, r, cls, dt, 37, 64, xlead=9))
    # LayerNorm backward: quad form (fp32: C % 4 == 0; bf16: C % 4 == 0 but not % 8), scalar form, each with and without dx_add
    quad = {(16, 1): (64, 60), (32, 1): (128, 68), (64, 1): (256, 132), (64, 2): (512, 260)} if dt == F32 else \
        {(16, 1): (44, 44), (32, 1): (68, 68), (64, 1): (132, 132), (64, 2): (260, 260)}
    for (lpr, np_), Cs in quad.items():
        cls = f"ln_bwd_v4_kernel<{t}, {lpr}, {np_}>"
        for i, C in enumerate(sorted(set(Cs))):
            for add in (False, True):
                if len(set(Cs)) == 2 and add != bool(i):
                    continue
                _add(f"ln-bwd-v4-{t}-C{C}{'-add' if add else ''}", cls,
                     lambda d, r, cls=cls, dt=dt, C=C, add=add: run_ln_bwd(d, r, cls, dt, 37, C, add=add, has=("steps=1",)))
    cls = f"ln_bwd_v4_kernel<{t}, 16, 1>"
    rows2 = 2 * 16 * (256 if dt == BF else 1024) + 5
    _add(f"ln-bwd-v4-{t}-steps2", cls, lambda d, r, cls=cls, dt=dt, n=rows2: run_ln_bwd(d, r, cls, dt, n, 4, add=True, has=("steps=2",)), big=True)
    # (C = 100 is a multiple of 4: with aligned rows it belongs to the quad form, so the <2, 4> scalar instance is taken at C = 102 and
    # C = 100 is held to the quad form it selects)
    cls = f"ln_bwd_v4_kernel<{t}, 32, 1>"
    _add(f"ln-bwd-v4-{t}-C100", cls, lambda d, r, cls=cls, dt=dt: run_ln_bwd(d, r, cls, dt, 67, 100))
    for (mj, rp), C in {(1, 4): 50, (2, 4): 102, (4, 2): 250, (8, 1): 510}.items():
        cls = f"layernorm_bwd_kernel<{t}, {mj}, {rp}>"
        for add in (False, True):
            _add(f"ln-bwd-scalar-{t}-C{C}{'-add' if add else ''}", cls,
                 lambda d, r, cls=cls, dt=dt, C=C, add=add: run_ln_bwd(d, r, cls, dt, 67, C, add=add))
    cls = f"layernorm_bwd_kernel<{t}, 1, 4>"
    _add(f"ln-bwd-{t}-C64-add-offset-by-one", cls, lambda d, r, cls=cls, dt=dt: run_ln_bwd(d, r, cls, dt, 37, 64, add=True, alead=9))
# the 8-channel form (bf16 only), accumulating and deferred (part + fold), and the split-K accumulator form
for lpr, (Ca, Cb) in {8: (64, 40), 16: (128, 72), 32: (256, 136), 64: (512, 264)}.items():
    cls = f"ln_bwd_v8_kernel<{lpr}, 1>"
    _add(f"ln-bwd-v8-C{Ca}", cls, lambda d, r, cls=cls, C=Ca: run_ln_bwd(d, r, cls, BF, 37, C, has=("steps=1",)))
    _add(f"ln-bwd-v8-C{Cb}-add", cls, lambda d, r, cls=cls, C=Cb: run_ln_bwd(d, r, cls, BF, 37, C, add=True))
    _add(f"ln-part-C{Ca}-scaled", cls + " part dxs=1",
         lambda d, r, cls=cls, C=Ca: run_ln_part(d, r, cls + " part dxs=1", 38, C, True, True, has=("steps=1",)))
    _add(f"ln-part-C{Cb}+fold-two-items", cls + " part dxs=0",
         lambda d, r, cls=cls, C=Cb: run_ln_part(d, r, cls + " part dxs=0", 37, C, False, False, rows2=70, C2=24))
_add("ln-bwd-v8-steps2", "ln_bwd_v8_kernel<8, 1>", lambda d, r: run_ln_bwd(d, r, "ln_bwd_v8_kernel<8, 1>", BF, 2 * 32 * 256 + 5, 8, has=("steps=2",)),
     big=True)
_add("ln-part-steps2", "ln_bwd_v8_kernel<8, 1> part dxs=0",
     lambda d, r: run_ln_part(d, r, "ln_bwd_v8_kernel<8, 1> part dxs=0", 2 * 32 * 1024 + 5, 8, True, False, has=("steps=2",)), big=True)
for C in (64, 320):
    for bias in (False, True):
        _add(f"ln-acc-C{C}{'-bias' if bias else ''}", "ln_fwd_acc_kernel", lambda d, r, C=C, bias=bias: run_ln_acc(d, r, "ln_fwd_acc_kernel", 37, C, bias))

# BatchNorm forward, fp32: the three-launch form
FIN = "+bn_finalize_kernel<float>+"
PV4, PSC, AV4, ASC = "bn_partial_v4_kernel<float>", "bn_partial_kernel<float>", "bn_apply_v4_kernel<float> fin=0", "bn_apply_kernel<float> fin=0"


def _fwd(cid, cls, dt, B, C, HW, **kw):
    _add(cid, cls, lambda d, r: run_bn_fwd(d, r, cls, dt, B, C, HW, **kw), stats=True)


_fwd("bn-f32-HW196-wg64", PV4 + FIN + AV4, F32, 3, 5, 196, act="relu", has=("threads=64", "S=1"))
_fwd("bn-f32-HW400-wg128", PV4 + FIN + AV4, F32, 2, 3, 400, act="lrelu", has=("threads=128",), nbt_n=3)
_fwd("bn-f32-HW784-wg256", PV4 + FIN + AV4, F32, 2, 3, 784, has=("threads=256", "chunks=1"))
_fwd("bn-f32-HW49-scalar", PSC + FIN + ASC, F32, 4, 3, 49, act="relu", has=("chunks=1",))
_fwd("bn-f32-HW196-stride-not-quad", PSC + FIN + ASC, F32, 3, 5, 196, pad=2)
_fwd("bn-f32-HW196-x-offset-by-one", PSC + FIN + ASC, F32, 3, 5, 196, xlead=9)
_fwd("bn-f32-HW196-y-offset-by-one", PV4 + FIN + ASC, F32, 3, 5, 196, ylead=9, act="lrelu")
_fwd("bn-f32-v4-S2", PV4 + FIN + AV4, F32, 2, 2, 4096, has=("S=2", "chunks=2"))
_fwd("bn-f32-scalar-S2", PSC + FIN + ASC, F32, 1, 2, 2049, has=("S=2", "chunks=3"), running=False)
_fwd("bn-f32-HW2052-chunks2", PV4 + FIN + AV4, F32, 2, 3, 2052, act="relu", has=("chunks=2",))
_fwd("bn-f32-HW1025-chunks2", PSC + FIN + ASC, F32, 2, 3, 1025, act="lrelu", has=("chunks=2",))
_fwd("bn-f32-slice", PV4 + FIN + AV4, F32, 2, 4, 196, Ctot=6, c0=1, act="relu")
_fwd("bn-f32-split-v4", PV4 + "+bn_finalize_kernel<float>|" + AV4, F32, 2, 4, 196, Ctot=6, c0=1, act="lrelu", entry="split")
_fwd("bn-f32-split-scalar", PSC + "+bn_finalize_kernel<float>|" + ASC, F32, 4, 3, 49, act="relu", entry="split")
# BatchNorm forward, bf16
BV4, BFL, BSC = "bn_partial_v4_kernel<bf16_t>", "bn_partial_flat_kernel<bf16_t>", "bn_partial_kernel<bf16_t>"
_fwd("bn-bf16-1k-n2", "bn_train_fwd_1k_kernel", BF, 2, 3, 1, act="relu")
_fwd("bn-bf16-1k-n147", "bn_train_fwd_1k_kernel", BF, 3, 5, 49, act="lrelu", nbt_n=2)
_fwd("bn-bf16-1k-n2048-slice", "bn_train_fwd_1k_kernel", BF, 2, 2, 1024, Ctot=3, c0=1)
_fwd("bn-bf16-n2049-leaves-1k", BSC + "+bn_apply_kernel<bf16_t> fin=1", BF, 1, 2, 2049, act="relu", has=("S=2", "chunks=3"))
_fwd("bn-bf16-flat4-HW784", BV4 + "+bn_apply_flat_kernel<bf16_t, 4> fin=1", BF, 3, 3, 784, act="relu", has=("S=1",))
_fwd("bn-bf16-flat4-S2", BV4 + "+bn_apply_flat_kernel<bf16_t, 4> fin=1", BF, 9, 2, 1024, act="lrelu", has=("S=3",))
_fwd("bn-bf16-flat1-HW63", BFL + "+bn_apply_flat_kernel<bf16_t, 1> fin=1", BF, 33, 2, 63, act="relu")
_fwd("bn-bf16-flat1-S2", BFL + "+bn_apply_flat_kernel<bf16_t, 1> fin=1", BF, 5, 2, 1023, has=("S=3",))
_fwd("bn-bf16-flat1-y-offset-by-one", BV4 + "+bn_apply_flat_kernel<bf16_t, 1> fin=1", BF, 3, 3, 784, ylead=9, act="lrelu")
_fwd("bn-bf16-v4-HW1600", BV4 + "+bn_apply_v4_kernel<bf16_t> fin=1", BF, 2, 3, 1600, act="relu", has=("threads=256", "chunks=1"))
_fwd("bn-bf16-v4-slice", BV4 + "+bn_apply_v4_kernel<bf16_t> fin=1", BF, 3, 3, 784, Ctot=5, c0=2, act="lrelu", nbt_n=3)
_fwd("bn-bf16-v4-y-offset-by-one", BV4 + "+bn_apply_kernel<bf16_t> fin=1", BF, 2, 3, 1600, ylead=9)
_fwd("bn-bf16-scalar-HW1025", BSC + "+bn_apply_kernel<bf16_t> fin=1", BF, 2, 3, 1025, act="lrelu", has=("chunks=2",), running=False)
_fwd("bn-bf16-flat-partial-strided", BFL + "+bn_apply_kernel<bf16_t> fin=1", BF, 33, 2, 63, pad=1, act="relu")
_fwd("bn-bf16-split-v4-flat4", BV4 + "+bn_finalize_kernel<bf16_t>|bn_apply_flat_kernel<bf16_t, 4> fin=0", BF, 3, 3, 784, act="relu", entry="split")
_fwd("bn-bf16-split-flat-flat1", BFL + "+bn_finalize_kernel<bf16_t>|bn_apply_flat_kernel<bf16_t, 1> fin=0", BF, 3, 2, 63, act="lrelu", entry="split")
_fwd("bn-bf16-split-scalar", BSC + "+bn_finalize_kernel<bf16_t>|bn_apply_kernel<bf16_t> fin=0", BF, 2, 3, 1025, entry="split")
_fwd("bn-bf16-split-v4-v4", BV4 + "+bn_finalize_kernel<bf16_t>|bn_apply_v4_kernel<bf16_t> fin=0", BF, 2, 2, 196, Ctot=3, act="relu", entry="split")


def _bwd(cid, cls, dt, B, C, HW, **kw):
    _add(cid, cls, lambda d, r: run_bn_bwd(d, r, cls, dt, B, C, HW, **kw))


for dt in (F32, BF):
    t = _tn(dt)
    v4 = f"bn_bwd_partial_v4_kernel<{t}>+bn_bwd_apply_v4_kernel<{t}>"
    sc = f"bn_bwd_partial_kernel<{t}>+bn_bwd_apply_kernel<{t}>"
    big = dt == BF  # bf16 leaves the one-kernel form above B HW = 2048 only
    _bwd(f"bn-bwd-{t}-v4-slice-wg64", v4, dt, 11 if big else 3, 3, 196, Ctot=5, c0=1, act="relu", has=("threads=64",))
    _bwd(f"bn-bwd-{t}-v4-wg128-add", v4, dt, 6 if big else 2, 3, 400, pad=4, act="lrelu", add="tight", has=("threads=128",))
    _bwd(f"bn-bwd-{t}-v4-S2-chunks2", v4, dt, 2, 2, 4096, pad=4 if big else 0, has=("S=2", "chunks=2"))
    _bwd(f"bn-bwd-{t}-scalar-HW1025", sc, dt, 2, 3, 1025, act="relu", add="tight", has=("chunks=2",))
    _bwd(f"bn-bwd-{t}-scalar-S2", sc, dt, 1, 2, 2049, act="lrelu", has=("S=2", "chunks=3"))
    _bwd(f"bn-bwd-{t}-dx-offset-by-one", sc, dt, 11 if big else 3, 3, 196, pad=4 if big else 0, dlead=9, act="relu")
_bwd("bn-bwd-bf16-1k-n147", "bn_bwd_1k_kernel", BF, 3, 5, 49, act="relu", add="tight")
_bwd("bn-bwd-bf16-1k-n2048-slice", "bn_bwd_1k_kernel", BF, 2, 2, 1024, Ctot=3, c0=1, act="lrelu")
_bwd("bn-bwd-bf16-1k-n2", "bn_bwd_1k_kernel", BF, 2, 3, 1)
FL4 = "bn_bwd_partial_v4_kernel<bf16_t>+bn_bwd_apply_flat_kernel<bf16_t, 4>"
FL1 = "bn_bwd_partial_flat_kernel<bf16_t>+bn_bwd_apply_flat_kernel<bf16_t, 1>"
_bwd("bn-bwd-bf16-flat4-add", FL4, BF, 3, 3, 784, act="relu", add="tight")
_bwd("bn-bwd-bf16-flat4-S3", FL4, BF, 9, 2, 1024, act="lrelu", has=("S=3",))
_bwd("bn-bwd-bf16-add-wide-leaves-flat", "bn_bwd_partial_v4_kernel<bf16_t>+bn_bwd_apply_v4_kernel<bf16_t>", BF, 3, 3, 784, act="relu", add="wide")
_bwd("bn-bwd-bf16-flat1-HW63", FL1, BF, 33, 2, 63, act="lrelu", add="tight")
_bwd("bn-bwd-bf16-flat1-S3", FL1, BF, 5, 2, 1023, has=("S=3",))
for B in (2, 3, 63, 64):
    for C in (1, 64, 65, 130):
        if (B in (3, 63)) == (C in (1, 130)):
            run = (B + C) % 2 == 0
            _add(f"bn1d-B{B}-C{C}{'' if run else '-no-running'}", "bn1d_train_fwd_kernel",
                 lambda d, r, B=B, C=C, run=run: run_bn1d(d, r, "bn1d_train_fwd_kernel", B, C, running=run), stats=True)


def _nameable():
    """every name the dispatcher rules of norm.hip can produce, without run-time numbers ('|': two calls of one case)"""
    n = {"ln_fwd_acc_kernel", "bn_train_fwd_1k_kernel", "bn_bwd_1k_kernel", "bn1d_train_fwd_kernel"}  # (bn1d_bwd: in the bn1d cases)
    widths = ((16, 1), (32, 1), (64, 1), (64, 2))
    for t in ("float", "bf16_t"):
        n |= {f"ln_fwd_v4_kernel<{t}, {a}, {b}>" for a, b in widths} | {f"layernorm_fwd_kernel<{t}>"}
        n |= {f"ln_bwd_v4_kernel<{t}, {a}, {b}>" for a, b in widths}
        n |= {f"layernorm_bwd_kernel<{t}, {a}, {b}>" for a, b in ((1, 4), (2, 4), (4, 2), (8, 1))}
        # plane forms: a quad partial goes with either apply (the destination may be misaligned on its own), a scalar partial with the
        # scalar apply only (what keeps x from the quad form keeps the apply from it)
        partials = [f"bn_partial_v4_kernel<{t}>", f"bn_partial_kernel<{t}>"]
        plane = [(partials[0], f"bn_apply_v4_kernel<{t}>"), (partials[0], f"bn_apply_kernel<{t}>"), (partials[1], f"bn_apply_kernel<{t}>")]
        if t == "float":
            n |= {f"{p}+bn_finalize_kernel<float>+{a} fin=0" for p, a in plane}
            n |= {f"{p}+bn_finalize_kernel<float>|{a} fin=0" for p, a in (plane[0], plane[2])}
        else:
            fl = "bn_partial_flat_kernel<bf16_t>"
            n |= {f"{p}+{a} fin=1" for p, a in plane} | {f"{fl}+bn_apply_kernel<bf16_t> fin=1"}
            n |= {f"{partials[0]}+bn_apply_flat_kernel<bf16_t, 4> fin=1", f"{partials[0]}+bn_apply_flat_kernel<bf16_t, 1> fin=1",
                  f"{fl}+bn_apply_flat_kernel<bf16_t, 1> fin=1"}
            fz = "+bn_finalize_kernel<bf16_t>|"
            n |= {f"{partials[0]}{fz}bn_apply_flat_kernel<bf16_t, 4> fin=0", f"{fl}{fz}bn_apply_flat_kernel<bf16_t, 1> fin=0",
                  f"{partials[1]}{fz}bn_apply_kernel<bf16_t> fin=0", f"{partials[0]}{fz}bn_apply_v4_kernel<bf16_t> fin=0"}
            n |= {"bn_bwd_partial_v4_kernel<bf16_t>+bn_bwd_apply_flat_kernel<bf16_t, 4>",
                  "bn_bwd_partial_flat_kernel<bf16_t>+bn_bwd_apply_flat_kernel<bf16_t, 1>"}
        n |= {f"bn_bwd_partial_v4_kernel<{t}>+bn_bwd_apply_v4_kernel<{t}>", f"bn_bwd_partial_kernel<{t}>+bn_bwd_apply_kernel<{t}>"}
    for lpr in (8, 16, 32, 64):
        n |= {f"ln_bwd_v8_kernel<{lpr}, 1>", f"ln_bwd_v8_kernel<{lpr}, 1> part dxs=0", f"ln_bwd_v8_kernel<{lpr}, 1> part dxs=1"}
    return n


def test_every_nameable_norm_kernel_has_a_case():
    """(each run_* asserts the reporter's name against the case's class, so a class listed here is a class that ran)"""
    covered = {c["cls"] for c in CASES}
    assert covered == _nameable(), (sorted(_nameable() - covered), sorted(covered - _nameable()))


def test_branches_no_other_test_reaches_have_a_case():
    ids = {c["id"] for c in CASES}
    assert {"ln-fwd-float-C8-steps2", "ln-fwd-bf16_t-C260-steps2", "ln-bwd-v8-steps2", "ln-bwd-v4-float-steps2", "ln-bwd-v4-bf16_t-steps2",
            "ln-part-steps2", "bn-f32-v4-S2", "bn-f32-scalar-S2", "bn-f32-HW2052-chunks2", "bn-f32-HW1025-chunks2", "bn-bf16-flat4-S2",
            "bn-bwd-float-v4-S2-chunks2", "bn-bwd-bf16_t-scalar-S2", "ln-fwd-float-C64-offset-by-one", "bn-f32-HW196-x-offset-by-one",
            "ln-bwd-bf16_t-C64-add-offset-by-one", "bn-bwd-bf16-add-wide-leaves-flat", "bn-bf16-n2049-leaves-1k"} <= ids, sorted(ids)


def _params(cases):
    return [pytest.param(c, id=c["id"]) for c in cases]


@pytest.mark.parametrize("regime", ["normal", "offset", "constant"])
@pytest.mark.parametrize("case", _params(CASES))
def test_norm_bound(dev, case, regime):
    case["fn"](dev, regime)


@pytest.mark.parametrize("case", _params([c for c in CASES if c["stats"]]))
def test_norm_bound_outlier_first(dev, case):
    """the offset regime with x[0, c, 0] = 0: the batch variance may not depend on one element"""
    case["fn"](dev, "outlier")


# ---- argument contracts --------------------------------------------------------------------------------------------------------
def test_layernorm_backward_refuses_wide_rows(dev):
    x = torch.zeros(2 * 516, device=dev)
    v = torch.zeros(516, device=dev)
    rc = _lib.lib().cenet_layernorm_bwd_add_acc_f32(kern.P(x), kern.P(x), kern.P(v), kern.P(v), kern.P(v), None, kern.P(x),
                                                    kern.P(v), kern.P(v), 2, 516, kern.stream())
    assert rc == 2  # CENET_EUNSUPPORTED


def test_bn1d_supported_range(dev):
    assert [kern.bn1d_supported(B) for B in (1, 2, 64, 65)] == [False, True, True, False]


def test_layernorm_bwd_part_supported(dev):
    xb, xf = torch.zeros(8 * 64 + 8, dtype=BF, device=dev), torch.zeros(8 * 64, device=dev)
    assert kern.layernorm_bwd_part_supported(xb, xb, 64)
    assert not kern.layernorm_bwd_part_supported(xf, xf, 64)          # fp32 rows
    assert not kern.layernorm_bwd_part_supported(xb, xb, 68)          # C % 8
    assert not kern.layernorm_bwd_part_supported(xb, xb, 520)         # C > 512
    assert not kern.layernorm_bwd_part_supported(xb[4:], xb, 64)      # 16-byte alignment


# ---- mutation self-test: no kernel involved ------------------------------------------------------------------------------------
def _trunc_bf16(x64):
    return (x64.float().view(torch.int32) & -65536).view(torch.float32).to(BF)


def _as_output(wrong64, exp, truncate=False):
    conv = _trunc_bf16 if truncate else (lambda v: v.float().to(exp.out_dtype))
    return torch.where(exp.own, conv(wrong64), exp.prev_raw)


def _scatter(exp, val):
    C = exp.C.clone()
    C[exp.idx.reshape(-1)] = val.reshape(-1).double()
    return C


def _mut_bn(regime, dt=BF, B=2, C=4, HW=49, act="lrelu", seed=41):
    g = torch.Generator().manual_seed(seed)
    x = _data((B, C, HW), g, regime, 1)
    x[:, 1] = 1.75  # a constant channel in every regime
    dy, add = _cot((B, C, HW), g, "normal"), R.reals((B, C, HW), g).to(BF).float()
    gamma, beta = _affine(C, g)
    return x, dy, add, gamma, beta, 0.2 * R.reals((C,), g), torch.rand(C, generator=g) + 0.5


def _mutated(name, regime):
    """-> (expectation, what a kernel with the defect would have left in the buffer)"""
    cpu = torch.device("cpu")
    B, C, HW = (2, 4, 1025) if name == "ragged_chunk_without_m2" else (2, 4, 49)
    dt = F32 if name == "ragged_chunk_without_m2" else BF
    x, dy, add, gamma, beta, prm, prv = _mut_bn(regime, dt, B, C, HW)
    n = B * HW
    st = R.bn_stats(x, prm, prv, MOM)
    mu, var = st["st"].mu[0, :, 0], st["st"].var[0, :, 0]

    def vec(key, wrong):
        buf = _vecdest(C, cpu, {"rmean": prm, "rvar": prv}.get(key))
        exp = R.as_exp(buf, 4, (C,), (1,), st[key], dims=("channel",))
        return exp, _as_output(_scatter(exp, wrong), exp)
    if name == "unbiased_variance":
        return vec("var", var * n / (n - 1))
    if name == "running_var_biased":
        return vec("rvar", (1 - MOM) * prv.double() + MOM * var)
    if name == "momentum_on_wrong_operand":
        return vec("rmean", MOM * prm.double() + (1 - MOM) * mu)
    if name == "first_split_only":
        return vec("mean", x[:1].double().mean((0, 2)))
    shape, strides = (B, C, HW), (C * HW, HW, 1)
    if name in ("eps_dropped_on_constant_channel", "truncate"):
        yb = _buf(torch.full((1, B * C * HW), SENTINEL), cpu, BF, 8, SENTINEL)
        y, _, _ = R.bn_fwd(x, mu, var, gamma, beta, BN_EPS, "lrelu", SLOPE, st["st"].b_mu, st["st"].b_var)
        exp = R.as_exp(yb, 8, shape, strides, y)
        if name == "truncate":
            return exp, _as_output(exp.C, exp, truncate=True)
        wrong = R.bn_fwd(x, mu, var, gamma, beta, 0.0, "lrelu", SLOPE)[0].ref
        return exp, _as_output(_scatter(exp, wrong), exp)
    if name == "ln_row_with_neighbours_rstd":
        rows, Cn = 6, 64
        g = torch.Generator().manual_seed(43)
        xl = _data((rows, Cn), g, regime, 0)
        gm, bt = _affine(Cn, g)
        o = R.ln_fwd(xl, gm, bt, LN_EPS)
        yb = _buf(torch.full((1, rows * Cn), SENTINEL), cpu, BF, 8, SENTINEL)
        exp = R.as_exp(yb, 8, (rows, Cn), (Cn, 1), o["y"])
        wrong = o["y"].ref.clone()
        wrong[2] = (xl[2].double() - o["st"].mu[2]) * o["rstd"].ref[3] * gm.double() + bt.double()
        return exp, _as_output(_scatter(exp, wrong), exp)
    # backward
    mean, varf = mu.float(), var.float()
    o = R.bn_bwd(dy, x, mean, varf, gamma, beta, BN_EPS, "lrelu", SLOPE, add)
    r = (varf.double() + BN_EPS)[None, :, None] ** -0.5
    xh = (x.double() - mean.double()[None, :, None]) * r
    pre = xh * gamma.double()[None, :, None] + beta.double()[None, :, None]
    gd = dy.double() * R._dact64(pre, "lrelu", SLOPE)
    gr = gamma.double()[None, :, None] * r
    m1, m2 = gd.mean((0, 2), keepdim=True), (gd * xh).mean((0, 2), keepdim=True)
    if name == "dgamma_overwritten":
        buf, lead = _acc(torch.full((C,), 0.75), cpu)
        exp = R.as_exp(buf, lead, (C,), (1,), o["dgamma"], add=True, dims=("channel",))
        return exp, _as_output(_scatter(exp, o["dgamma"].ref), exp)
    dxb = _buf(torch.full((1, B * C * HW), SENTINEL), cpu, dt, 8, SENTINEL)
    exp = R.as_exp(dxb, 8, shape, strides, o["dx"])
    if name == "mean_g_dropped":
        wrong = gr * (gd - xh * m2) + add.double()
    elif name == "ragged_chunk_without_m2":
        wrong = o["dx"].ref.clone()
        wrong[:, :, 1024:] = (gr * (gd - m1) + add.double())[:, :, 1024:]
    elif name == "lrelu_derivative_from_wrong_side":
        g2 = dy.double() * torch.where(pre > 0, torch.full_like(pre, SLOPE), torch.ones_like(pre))
        wrong = gr * (g2 - g2.mean((0, 2), keepdim=True) - xh * (g2 * xh).mean((0, 2), keepdim=True)) + add.double()
    else:
        assert name == "dx_add_ignored"
        wrong = o["dx"].ref - add.double()
    return exp, _as_output(_scatter(exp, wrong), exp)


MUTATIONS = ["unbiased_variance", "running_var_biased", "momentum_on_wrong_operand", "eps_dropped_on_constant_channel", "first_split_only",
             "mean_g_dropped", "ragged_chunk_without_m2", "dgamma_overwritten", "lrelu_derivative_from_wrong_side", "dx_add_ignored",
             "ln_row_with_neighbours_rstd", "truncate"]


@pytest.mark.parametrize("regime", ["normal", "offset"])
@pytest.mark.parametrize("name", MUTATIONS)
def test_norm_mutations_are_rejected(name, regime):
    """the acceptance rule fed deliberately wrong references rejects every one of the table in the module docstring, and accepts the
    unmutated reference"""
    exp, got = _mutated(name, regime)
    assert R.assert_bound(_as_output(exp.C, exp), exp, "unmutated") <= 1.0
    with pytest.raises(AssertionError):
        R.assert_bound(got, exp, name)


def test_reference_agrees_with_autograd():
    """the float64 formulas against torch's own float64 batch_norm / layer_norm and autograd (the reference's reference)"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    x, dy = R.reals((3, 4, 10), g).double().requires_grad_(True), R.reals((3, 4, 10), g).double()
    gm, bt = (t.double().requires_grad_(True) for t in _affine(4, g))
    rm, rv = torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    rm0, rv0 = rm.clone(), rv.clone()
    y = F.leaky_relu(F.batch_norm(x, rm, rv, gm, bt, True, MOM, BN_EPS), SLOPE)
    y.backward(dy)
    st = R.bn_stats(x.detach(), rm0, rv0, MOM)
    mu, var = st["st"].mu[0, :, 0], st["st"].var[0, :, 0]
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-12)  # noqa: E731
    close(st["rmean"].ref, rm), close(st["rvar"].ref, rv)
    close(R.bn_fwd(x.detach(), mu, var, gm.detach(), bt.detach(), BN_EPS, "lrelu", SLOPE)[0].ref, y.detach())
    o = R.bn_bwd(dy, x.detach(), mu, var, gm.detach(), bt.detach(), BN_EPS, "lrelu", SLOPE)
    close(o["dx"].ref, x.grad), close(o["dgamma"].ref, gm.grad), close(o["dbeta"].ref, bt.grad)
    xl, dyl = R.reals((5, 12), g).double().requires_grad_(True), R.reals((5, 12), g).double()
    gl, bl = (t.double().requires_grad_(True) for t in _affine(12, g))
    yl = F.layer_norm(xl, (12,), gl, bl, LN_EPS)
    yl.backward(dyl)
    f = R.ln_fwd(xl.detach(), gl.detach(), bl.detach(), LN_EPS)
    close(f["y"].ref, yl.detach())
    o = R.ln_bwd(dyl, xl.detach(), gl.detach(), f["mean"].ref, f["rstd"].ref)
    close(o["dx"].ref, xl.grad), close(o["dgamma"].ref, gl.grad), close(o["dbeta"].ref, bl.grad)


NS = [2, 3, 8, 40, 64, 132, 147, 260, 512, 1568, 2048, 2352, 4098, 8192]  # row lengths and channel populations of the case matrix


def test_norm_constants_are_the_host_measurement():
    """C_ACC stays gemm_ref's because the host measurement over the n of this matrix, x 4, stays under it; the values norm_ref records
    are pinned: the measurement must reproduce them.  Never measured on a kernel."""
    r_mu, r_var, r_sum = R.measure_constants(NS)
    print(f"measured on the host: mean {r_mu:.3f}, variance {r_var:.3f}, sum of products {r_sum:.3f}")
    assert r_mu == pytest.approx(R.MEASURED_MEAN, abs=0.01) and r_var == pytest.approx(R.MEASURED_VAR, abs=0.01)
    assert r_sum == pytest.approx(R.MEASURED_SUM, abs=0.01)
    assert 4.0 * max(R.MEASURED_MEAN, R.MEASURED_SUM) < R.C_ACC == 2.3 and R.C_OUT == 1.0 < 2.0
    assert R.C_ACC < 4.0 * R.MEASURED_VAR <= R.C_VAR == 5.6  # the variance's own constant: C_ACC does not cover its measurement
