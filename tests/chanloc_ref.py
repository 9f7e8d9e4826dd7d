"""Reference for the channel-local fused chains (chanloc.hip), for tests/test_chanloc_bounds.py: float64 evaluations of what
include/cenet_hip.h says each entry point means, step by step, under the acceptance rule of tests/gemm_ref.py and tests/norm_ref.py
    |got - ref| <= C_OUT u_out |ref| + C_ACC 2^-24 sqrt(K) Mag + extra                                   (u_out = 2^-8 bf16, 2^-24 fp32)
Plain helper module: no fixtures.  Written from the header text and PyTorch's float64 ops (F.interpolate, F.adaptive_avg_pool2d,
erf), not from the kernels.  `stats`, `rsqrt_of`, `normalise`, `as_exp`, `Out`, `acc_term` are norm_ref's, `dw3x3`, `dw3x3_wgrad`, `expect`,
`assert_bound`, the footprint check and `_dact64` conv_ref's, `ints`, `reals`, `_act64` and the constants gemm_ref's (imported, not copied).

A CHAIN's bound is the first-order propagation of its steps' bounds (as norm_ref does for statistics -> rstd -> y).  A step returns
its float64 value and `e`, the bound of its fp32 evaluation BEFORE the store rounding; the next step adds |its derivative| e:
    conv                      Mag = sum |w| |x| over the taps inside the plane, K = 9:  e_u = C_ACC u sqrt(9) Mag
    a value the chain goes on with AS STORED (the header says where: dwbn's conv output, cfam_mid's x1 and d x1): `stored()` -- the
                              reference rounds to bf16 too, and only where a rounding boundary lies within e of the float64 value does
                              the bound become the distance of the two candidates (one bf16 ulp), else 0
    statistics of computed u  b_mu = norm_ref's + E e_u;   b_var = norm_ref's + 2 sqrt(var E e_u^2) + E e_u^2  (Cauchy-Schwarz on
                              d var = 2 E[(u - mu) du])
    normalise                 norm_ref.normalise + |gamma| r e_u; relu / lrelu are 1-Lipschitz
    BatchNorm backward        norm_ref's formulas with e_xh += r e_u (+ RS_REL |xh|: the backward forms r itself) and an error e_dy of the
                              incoming gradient carried into every sum
    transposed conv / folds   linear maps: Mag the map of |.|, e the map of e through |w|
relu / lrelu in a backward pass: an element whose float64 pre-activation lies within its own bound of 0 is AMBIGUOUS.  Its gradient may
take either slope: |dy| (1 - slope) goes to that element's own bound (so it, and the dx its conv spreads it to, are in effect left out),
and through the channel's sums to dbeta, dgamma and every dx of the channel.  The test asserts on the reference alone that at most
1 % of a case is ambiguous.

Constants: C_ACC, C_OUT (gemm_ref), C_VAR, RS_REL, K_ELEM (norm_ref) as they are.  New ones are measured on the HOST, never on a kernel
(`measure_constants()`: the header's formula in plain fp32 on the CPU against float64 over |u| <= 24, the range of the case matrix), x 4
as norm_ref.measure_constants does, rounded up:
    GELU      0.5 u (1 + erf(u / sqrt 2))           |err| / (2^-24 |u|)   measured 1.712   -> C_GELU  = 6.9
    GELU'     Phi(u) + u phi(u)                     |err| / 2^-24         measured 2.185   -> C_DGELU = 8.8
    sigmoid   1 / (1 + exp(-v))                     |err| / 2^-24         measured 1.497   -> C_SIGM  = 6.0
    pooled branch's composed maps RH / RW (ops' host builder, fp32 coordinates) against the float64 F.interpolate chain:
              largest |R32 - R64| / 2^-24 over the H, W of the matrix     measured 5.333   -> C_MAP   = 21.4 (per axis; rows sum to 1)
bf16 storage: the dwact kernels evaluate erf by Abramowitz & Stegun 7.1.26; the header states |gelu_as(u) - gelu(u)| <= AS_H |u| and
|gelu_as_grad(u) - gelu'(u)| <= AS_DG with their derivation, and the reference uses the stated figures (AS_H = 6e-7, AS_DG = 7e-7: a
four-hundredth of a bf16 ulp).  Not widened to make a kernel pass."""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn.functional as F

from conv_ref import DACT_LIP, DACT_MAX, dw3x3, dw3x3_wgrad  # noqa: F401
from gemm_ref import ACT_LIPSCHITZ
from norm_ref import (BF, C_ACC, C_OUT, C_VAR, K_ELEM, RS_REL, U_BF16, U_FP32, Out, _act64, _dact64, _outside, acc_term,  # noqa: F401
                      as_exp, assert_bound, bound_of, expect, index_map, ints, normalise, reals, rsqrt_of, stats, view)

MEASURED_GELU, MEASURED_DGELU, MEASURED_SIGM, MEASURED_MAP = 1.712, 2.185, 1.497, 5.333  # measure_constants() (pinned by a test)
C_GELU, C_DGELU, C_SIGM, C_MAP = 6.9, 8.8, 6.0, 21.4
AS_H, AS_DG = 6e-7, 7e-7  # include/cenet_hip.h: stated error of the bf16 instances' erf approximation
U_RANGE = 24.0
MAP_SIZES = (4, 7, 9, 10, 20, 64)


def ch(t, like):
    """a per-channel vector against [B, C, ...]"""
    return t.double().reshape((1, -1) + (1,) * (like.dim() - 2))


def _dims(u):
    return tuple(d for d in range(u.dim()) if d != 1)


def stored(u, e, dt):
    """an intermediate the chain goes on with AS STORED in the tensor type -> (value, bound).  fp32: the value computed is the value
    stored.  bf16: the reference rounds too; rounding is monotone, so the fp32 value v of a kernel, |v - u| <= e, rounds to the same
    bf16 number unless a rounding boundary lies within e of u: there the bound is the distance of the two candidates (one bf16
    ulp: the first-order term of one such rounding), everywhere else 0"""
    e = e + torch.zeros_like(u)
    if dt != BF:
        return u, e
    rb = lambda t: t.float().to(BF).double()  # noqa: E731
    return rb(u), (rb(u + e) - rb(u - e)).abs()


# ---- BatchNorm steps of a chain --------------------------------------------------------------------------------------------
def chan_stats(u, e_u, rmean=None, rvar=None, momentum=0.1):
    """batch statistics per channel of a COMPUTED float64 tensor u [B, C, ...] whose fp32 evaluation is within e_u ->
    mu, var, b_mu, b_var ([1, C, 1...]) and the Outs mean, var (and rmean, rvar)"""
    dims = _dims(u)
    st = stats(u, dims)
    e_u = e_u + torch.zeros_like(u)
    e1, e2 = e_u.mean(dims, keepdim=True), (e_u ** 2).mean(dims, keepdim=True)
    b_mu = st.b_mu + e1
    d_var = 2.0 * (st.var * e2).sqrt() + e2
    b_var = st.b_var - st.b_mu ** 2 + b_mu ** 2 + d_var
    sq = lambda t: t.reshape(-1)  # noqa: E731
    outs = dict(mean=Out(sq(st.mu), sq(st.ax), st.n, sq(e1)),
                var=Out(sq(st.var), sq(st.var) * (C_VAR / C_ACC), st.n + K_ELEM, sq(b_mu ** 2 + d_var)))
    if rmean is not None:
        m, unb = momentum, st.n / (st.n - 1.0)
        rm, rv = rmean.double(), rvar.double()
        outs["rmean"] = Out((1 - m) * rm + m * sq(st.mu), (1 - m) * rm.abs() + m * sq(st.mu).abs(), K_ELEM, m * sq(b_mu))
        outs["rvar"] = Out((1 - m) * rv + m * sq(st.var) * unb, (1 - m) * rv.abs() + m * sq(st.var) * unb, K_ELEM, m * unb * sq(b_var))
    return SimpleNamespace(mu=st.mu, var=st.var, b_mu=b_mu, b_var=b_var, n=st.n, outs=outs)


def bn_apply(u, e_u, st, gamma, beta, eps):
    """gamma (u - mu) / sqrt(var + eps) + beta on the statistics `st` of the same call -> (pre, bound)"""
    r, b_r = rsqrt_of(st.var, st.b_var, eps)
    g = ch(gamma, u)
    pre, e = normalise(u, st.mu, st.b_mu, r, b_r, g, ch(beta, u))
    return pre, e + g.abs() * r * e_u


def bn_back(dy, u, e_u, mean, var, gamma, beta, eps, act, slope, e_dy=0.0):
    """BatchNorm (+ activation) backward over [B, C, ...] with mean / var GIVEN (operands of the entry point): the gradient du of
    the BatchNorm's input with its bound, the Outs dgamma / dbeta (sums, to be ADDED) and the ambiguous elements"""
    dims = _dims(u)
    n = 1
    for d in dims:
        n *= u.shape[d]
    dy = dy.double()
    e_dy = e_dy + torch.zeros_like(dy)
    mu, g = ch(mean, u), ch(gamma, u)
    b = ch(beta, u) if beta is not None else torch.zeros_like(g)
    r = (ch(var, u) + eps) ** -0.5
    xh, Xh = (u - mu) * r, (u.abs() + mu.abs()) * r
    e_xh = acc_term(Xh, K_ELEM) + RS_REL * xh.abs() + r * e_u
    pre = xh * g + b
    if act == "none":
        amb = torch.zeros_like(pre, dtype=torch.bool)
        flip = torch.zeros_like(pre)
    else:
        amb = pre.abs() <= acc_term(Xh * g.abs() + b.abs(), K_ELEM) + g.abs() * (RS_REL * Xh + r * e_u)
        flip = dy.abs() * (1.0 - (slope if act == "lrelu" else 0.0)) * amb
    gd = dy * _dact64(pre, act, slope)
    m1, m2 = gd.mean(dims, keepdim=True), (gd * xh).mean(dims, keepdim=True)
    s_b = (flip + e_dy).sum(dims, keepdim=True)
    s_g = ((flip + e_dy) * xh.abs() + gd.abs() * e_xh).sum(dims, keepdim=True)
    e_m1 = acc_term(gd.abs().mean(dims, keepdim=True), n) + s_b / n
    e_m2 = acc_term((gd * xh).abs().mean(dims, keepdim=True), n) + s_g / n
    s = g * r
    du = s * (gd - m1 - xh * m2)
    mag = s.abs() * (gd.abs() + m1.abs() + (xh * m2).abs())
    e_du = acc_term(mag, K_ELEM) + RS_REL * du.abs() + s.abs() * (flip + e_dy + e_m1 + xh.abs() * e_m2 + m2.abs() * e_xh)
    sq = lambda t: t.reshape(-1)  # noqa: E731
    return SimpleNamespace(du=du, e_du=e_du, amb=amb,
                           dgamma=Out(sq((gd * xh).sum(dims, keepdim=True)), sq((gd * xh).abs().sum(dims, keepdim=True)), n, sq(s_g)),
                           dbeta=Out(sq(gd.sum(dims, keepdim=True)), sq(gd.abs().sum(dims, keepdim=True)), n, sq(s_b)))


def _final(val, e):
    """an output whose bound is its store rounding plus the propagated e"""
    return Out(val, torch.zeros_like(val), 1, e + torch.zeros_like(val))


# ---- depthwise pieces ----------------------------------------------------------------------------------------------------------
def conv_dw(x, w, dil=1, bias=None):
    """-> (u, e_u): depthwise 3x3, zero outside the plane; Mag = sum |w| |x| over the taps inside"""
    u, mag, K = dw3x3(x, w, bias, dil)
    return u, acc_term(mag, K)


def conv_dw_T(du, e_du, w, dil=1, add=None):
    """data gradient of conv_dw (correlation with the flipped taps) (+ add) -> (dx, e_dx)"""
    dx, mag, K = dw3x3(du, w, None, dil, flip=True)
    e = dw3x3(e_du, w.abs(), None, dil, flip=True)[0]
    if add is not None:
        dx, mag, K = dx + add.double(), mag + add.double().abs(), K + 1
    return dx, acc_term(mag, K) + e


def conv_dw_wgrad(x, du, e_du, dil=1):
    """-> Out dw [C, 9] (the sum, to be ADDED)"""
    (dw, mag), _, K = dw3x3_wgrad(x, du, dil)
    return Out(dw, mag, K, dw3x3_wgrad(x.abs(), e_du, dil)[0][0])


def up2(x):
    return x.repeat_interleave(2, -2).repeat_interleave(2, -1)


def fold2(y):
    B, C, H2, W2 = y.shape
    return y.reshape(B, C, H2 // 2, 2, W2 // 2, 2).sum((3, 5))


# ---- EUCB front: y = LeakyReLU(BatchNorm_train(DW3x3(nearest_x2(x)))) ----------------------------------------------------------
def eucb_fwd(x, w, gamma, beta, eps, slope, rmean=None, rvar=None, momentum=0.1):
    u, e_u = conv_dw(up2(x.double()), w)
    st = chan_stats(u, e_u, rmean, rvar, momentum)
    pre, e = bn_apply(u, e_u, st, gamma, beta, eps)
    return dict(y=_final(_act64(pre, "lrelu", slope), e), **st.outs)


def eucb_bwd(g, x, w, gamma, beta, eps, slope, mean, var):
    xu = up2(x.double())
    u, e_u = conv_dw(xu, w)
    bb = bn_back(g, u, e_u, mean, var, gamma, beta, eps, "lrelu", slope)
    dxu, mag, _ = dw3x3(bb.du, w, None, 1, flip=True)
    e = dw3x3(bb.e_du, w.abs(), None, 1, flip=True)[0]
    return dict(dx=Out(fold2(dxu), fold2(mag), 36, fold2(e)), dw=conv_dw_wgrad(xu, bb.du, bb.e_du), dgamma=bb.dgamma, dbeta=bb.dbeta,
                amb=bb.amb)


# ---- dilated depthwise branches + BatchNorm + ReLU, and the pooled slice's copy ------------------------------------------------
def _dwbn_u(x, ws, dils, g, dt):
    """the conv outputs of the nb branches [B, nb g, H, W]; the header: STORED in the tensor type, statistics of the stored values"""
    us, es = [], []
    for j, (w, dil) in enumerate(zip(ws, dils)):
        u, e = conv_dw(x[:, j * g:(j + 1) * g].double(), w, dil)
        u, e = stored(u, e, dt)
        us.append(u), es.append(e)
    return torch.cat(us, 1), torch.cat(es, 1)


def dwbn_fwd(x, ws, dils, g, p, gamma, beta, eps, rmean, rvar, momentum, dt):
    nb = len(ws)
    u, e_u = _dwbn_u(x, ws, dils, g, dt)
    st = chan_stats(u, e_u, rmean, rvar, momentum)
    pre, e = bn_apply(u, e_u, st, gamma, beta, eps)
    out = dict(v=_final(_act64(pre, "relu", 0.0), e), **st.outs)
    if p:
        out["rest"] = x[:, nb * g:nb * g + p].double()  # a copy: exact
    return out


def dwbn_bwd(g_v, g_rest, g_add, x, ws, dils, g, p, gamma, beta, eps, mean, var, dt):
    nb = len(ws)
    u, e_u = _dwbn_u(x, ws, dils, g, dt)
    bb = bn_back(g_v, u, e_u, mean, var, gamma, beta, eps, "relu", 0.0)
    dxs, es, dws = [], [], []
    for j, (w, dil) in enumerate(zip(ws, dils)):
        sl = slice(j * g, (j + 1) * g)
        dx, e = conv_dw_T(bb.du[:, sl], bb.e_du[:, sl], w, dil, g_add[:, sl] if g_add is not None else None)
        dxs.append(dx), es.append(e)
        dws.append(conv_dw_wgrad(x[:, sl].double(), bb.du[:, sl], bb.e_du[:, sl], dil))
    if p:
        r = g_rest.double()
        a = g_add[:, nb * g:].double() if g_add is not None else torch.zeros_like(r)
        dxs.append(r + a), es.append(acc_term(r.abs() + a.abs(), 1))
    return dict(dx=_final(torch.cat(dxs, 1), torch.cat(es, 1)), dw=dws, dgamma=bb.dgamma, dbeta=bb.dbeta, amb=bb.amb)


# ---- depthwise 3x3 (+ bias) + activation ----------------------------------------------------------------------------------------
def _act_eval_err(u, act, dt):
    if act != "gelu":
        return torch.zeros_like(u)
    return (C_GELU * U_FP32 + (AS_H if dt == BF else 0.0)) * u.abs()


def _dact_eval_err(u, act, dt):
    if act != "gelu":
        return torch.zeros_like(u)
    return torch.full_like(u, C_DGELU * U_FP32 + (AS_DG if dt == BF else 0.0))


def dwact_fwd(x, w, bias, act, slope, dil, dt):
    u, e_u = conv_dw(x.double(), w, dil, bias)
    return dict(y=_final(_act64(u, act, slope), ACT_LIPSCHITZ[act] * e_u + _act_eval_err(u, act, dt)))


def dwact_bwd(g, x, w, bias, act, slope, dil, dt):
    x, g = x.double(), g.double()
    u, e_u = conv_dw(x, w, dil, bias)
    d = g * _dact64(u, act, slope)
    if act in ("relu", "lrelu"):
        amb = u.abs() <= e_u
        flip = g.abs() * (1.0 - (slope if act == "lrelu" else 0.0)) * amb
    else:
        amb, flip = torch.zeros_like(u, dtype=torch.bool), 0.0
    e_d = acc_term(g.abs() * DACT_MAX[act], 2) + g.abs() * (DACT_LIP[act] * e_u + _dact_eval_err(u, act, dt)) + flip
    dx, e_dx = conv_dw_T(d, e_d, w, dil)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    return dict(dx=_final(dx, e_dx), dw=conv_dw_wgrad(x, d, e_d, dil), amb=amb,
                db=Out(d.sum((0, 2, 3)), d.abs().sum((0, 2, 3)), n, e_d.sum((0, 2, 3))))


# ---- CFAM mid: p = BN_nl(p_raw); z = (1 - w) m + w p; x1 = x0 + ls z; y2 = BN_2(x1 as stored) -------------------------------------
def _mid_x1(p_raw, m, x0, pn, mag_p, e_pn, w, ls):
    w, l = float(w), ch(ls, p_raw)
    z = (1 - w) * m + w * pn
    mag_z = abs(1 - w) * m.abs() + abs(w) * mag_p
    e_z = acc_term(mag_z, K_ELEM) + abs(w) * e_pn
    x1 = x0 + l * z
    mag = x0.abs() + l.abs() * mag_z
    return x1, acc_term(mag, K_ELEM) + l.abs() * abs(w) * e_pn, z, mag_z, e_z


def cfam_mid_fwd(p_raw, m, x0, gp, bp, epsp, w, ls, g2, b2, eps2, rmp, rvp, momp, rm2, rv2, mom2, dt):
    p_raw, m, x0 = p_raw.double(), m.double(), x0.double()
    stp = chan_stats(p_raw, 0.0, rmp, rvp, momp)
    pn, e_pn = bn_apply(p_raw, 0.0, stp, gp, bp, epsp)
    rp = (stp.var + epsp) ** -0.5
    mag_p = ch(gp, p_raw).abs() * rp * (p_raw.abs() + stp.mu.abs()) + ch(bp, p_raw).abs()
    x1, e_x1, *_ = _mid_x1(p_raw, m, x0, pn, mag_p, e_pn, w, ls)
    x1s, e_st = stored(x1, e_x1, dt)  # the header: BatchNorm_2 takes the statistics of x1 AS STORED
    st2 = chan_stats(x1s, e_st, rm2, rv2, mom2)
    y2, e_y2 = bn_apply(x1s, e_st, st2, g2, b2, eps2)
    out = dict(x1=_final(x1, e_x1), y2=_final(y2, e_y2))
    out.update({k + "_p": v for k, v in stp.outs.items()})
    out.update({k + "_2": v for k, v in st2.outs.items()})
    return out


def cfam_mid_bwd(g_y2, g_x1, p_raw, m, x1, gp, bp, epsp, meanp, varp, w, ls, g2, eps2, mean2, var2, dt):
    p_raw, m, x1 = p_raw.double(), m.double(), x1.double()
    dims, C = _dims(p_raw), p_raw.shape[1]
    n = p_raw.numel() // C
    bb2 = bn_back(g_y2, x1, 0.0, mean2, var2, g2, None, eps2, "none", 0.0)
    gx = g_x1.double() if g_x1 is not None else torch.zeros_like(x1)
    d0 = bb2.du + gx
    e_d = bb2.e_du + acc_term(bb2.du.abs() + gx.abs(), 1)
    d, e_ds = stored(d0, e_d, dt)  # (the header: the chain below d x1 goes on with the value d_x0 stores)
    mup, g_, b_ = ch(meanp, p_raw), ch(gp, p_raw), ch(bp, p_raw)
    rp = (ch(varp, p_raw) + epsp) ** -0.5
    pn = (p_raw - mup) * rp * g_ + b_
    mag_p = g_.abs() * rp * (p_raw.abs() + mup.abs()) + b_.abs()
    e_pn = acc_term(mag_p, K_ELEM) + RS_REL * mag_p
    wv, l = float(w), ch(ls, p_raw)
    _, _, z, mag_z, e_z = _mid_x1(p_raw, m, torch.zeros_like(m), pn, mag_p, e_pn, wv, ls)
    sq = lambda t: t.sum(dims)  # noqa: E731
    dls = Out(sq(d * z), sq(d.abs() * mag_z), n, sq(e_ds * z.abs() + d.abs() * e_z))
    t = d * l * (pn - m)
    dw = Out(t.sum().reshape(1), (d.abs() * l.abs() * (mag_p + m.abs())).sum().reshape(1), n * C,
             (e_ds * l.abs() * (pn - m).abs() + d.abs() * l.abs() * (e_pn + acc_term(mag_p + m.abs(), K_ELEM))).sum().reshape(1))
    dm = d * l * (1 - wv)
    dpn = d * l * wv
    e_dpn = e_ds * (l * wv).abs() + acc_term(dpn.abs(), 2)
    bbp = bn_back(dpn, p_raw, 0.0, meanp, varp, gp, bp, epsp, "none", 0.0, e_dy=e_dpn)
    return dict(d_x0=_final(d0, e_d), d_m=_final(dm, e_ds * (l * (1 - wv)).abs() + acc_term(dm.abs(), 3)), d_p=_final(bbp.du, bbp.e_du),
                dgp=bbp.dgamma, dbp=bbp.dbeta, dg2=bb2.dgamma, db2=bb2.dbeta, dls=dls, dw=dw)


# ---- CFAM front: y1 = BN_1(x0); u = [max, mean, std] of y1 as stored; z = fc2 . relu(fc1 u); zn = BN1d(z); xs = y1 sigmoid(zn) -----
def _plane_stats(y, e_y):
    """[max, mean, biased std] over the plane of y [B, C, H, W] within e_y -> (u [B, C, 3], e_u, var-zero mask)"""
    st = stats(y, (2, 3))
    e1, e2 = e_y.mean((2, 3), keepdim=True), (e_y ** 2).mean((2, 3), keepdim=True)
    b_mu = st.b_mu + e1
    b_var = st.b_var - st.b_mu ** 2 + b_mu ** 2 + 2.0 * (st.var * e2).sqrt() + e2
    sd = st.var.sqrt()
    e_sd = torch.minimum(b_var / sd.clamp_min(1e-300), b_var.sqrt()) + RS_REL * sd  # |sqrt a - sqrt v| <= |a - v| / sqrt v, <= sqrt |a - v|
    const = y.amax((2, 3)) == y.amin((2, 3))  # a constant plane: mean and std = 0 exactly, whatever the float64 sums round to
    u = torch.stack([y.amax((2, 3)), torch.where(const, y.amax((2, 3)), st.mu[..., 0, 0]),
                     torch.where(const, torch.zeros_like(sd[..., 0, 0]), sd[..., 0, 0])], -1)
    e_u = torch.stack([e_y.amax((2, 3)), b_mu[..., 0, 0], e_sd[..., 0, 0]], -1)
    return u, e_u


def _gate_mlp(u, e_u, fc1, fc2):
    """z = fc2 . relu(fc1 u) per (image, channel) -> (z, e_z, hidden, its ambiguity mask, hidden's magnitude)"""
    f1, f2 = fc1.double()[None], fc2.double()[None]            # [1, C, 3, 3], [1, C, 3]
    h = (f1 * u[:, :, None, :]).sum(-1)
    mag_h = (f1.abs() * u.abs()[:, :, None, :]).sum(-1)
    e_h = acc_term(mag_h, 3) + (f1.abs() * e_u[:, :, None, :]).sum(-1)
    amb = h.abs() <= e_h
    hr = h.clamp_min(0.0)
    z = (f2 * hr).sum(-1)
    e_z = acc_term((f2.abs() * mag_h).sum(-1), 3) + (f2.abs() * e_h).sum(-1)
    return z, e_z, h, amb, mag_h


def cfam_front_fwd(x0, g1, b1, eps1, rm1, rv1, mom1, fc1, fc2, gd, bd, epsd, rmd, rvd, momd, dt):
    """-> Outs y1, xs [B, C, H, W], u [B, C, 3], z, zn [B, C], the statistics of both BatchNorms, and for amax: `y1s` (float64 y1 as
    stored), `e_y1s`; `hidden_amb`: the hidden units within their bound of relu's kink"""
    x0 = x0.double()
    st1 = chan_stats(x0, 0.0, rm1, rv1, mom1)
    y1, e_y1 = bn_apply(x0, 0.0, st1, g1, b1, eps1)
    y1s, e_s = stored(y1, e_y1, dt)  # the header: the per-image statistics and the gate use y1 AS STORED
    u, e_u = _plane_stats(y1s, e_s)
    z, e_z, _, amb, _ = _gate_mlp(u, e_u, fc1, fc2)
    out = dict(y1=_final(y1, e_y1), u=_final(u, e_u), z=_final(z, e_z), y1s=y1s, e_y1s=e_s, hidden_amb=amb)
    out.update({k + "1": v for k, v in st1.outs.items()})
    if gd is not None:
        std = chan_stats(z[:, :, None], e_z[:, :, None], rmd, rvd, momd)
        zn, e_zn = bn_apply(z[:, :, None], e_z[:, :, None], std, gd, bd, epsd)
        zn, e_zn = zn[:, :, 0], e_zn[:, :, 0]
        out.update({k + "d": v for k, v in std.outs.items()})
    else:
        zn, e_zn = z, e_z
    gate = torch.sigmoid(zn)[:, :, None, None]
    e_gate = (0.25 * e_zn + C_SIGM * U_FP32)[:, :, None, None]
    xs = y1s * gate
    out.update(zn=_final(zn, e_zn), xs=_final(xs, gate * e_s + y1s.abs() * e_gate + acc_term(xs.abs(), 1)))
    return out


def cfam_front_bwd(g_xs, g_y1, g_tap, x0, g1, b1, eps1, mean1, var1, fc1, fc2, gd, epsd, mean_d, var_d, u, amax, z, zn, dt):
    """mean1 / var1, mean_d / var_d, u, amax, z, zn: as given to the entry point"""
    x0, g_xs = x0.double(), g_xs.double()
    B, C, H, W = x0.shape
    HW = H * W
    mu, g, b = ch(mean1, x0), ch(g1, x0), ch(b1, x0)
    r = (ch(var1, x0) + eps1) ** -0.5
    y1 = (x0 - mu) * r * g + b
    mag_y = g.abs() * r * (x0.abs() + mu.abs()) + b.abs()
    y1s, e_y = stored(y1, acc_term(mag_y, K_ELEM) + RS_REL * mag_y, dt)  # (y1 as the forward stored it)
    u, zn = u.double(), zn.double()
    sg = torch.sigmoid(zn)
    e_sg = C_SIGM * U_FP32
    q = (g_xs * y1s).sum((2, 3))
    e_q = acc_term((g_xs * y1s).abs().sum((2, 3)), HW) + (g_xs.abs() * e_y).sum((2, 3))
    dzn = q * sg * (1 - sg)
    e_dzn = 0.25 * e_q + q.abs() * e_sg + acc_term(dzn.abs(), 3)
    out = {}
    if gd is not None:
        bbd = bn_back(dzn[:, :, None], z.double()[:, :, None], 0.0, mean_d, var_d, gd, None, epsd, "none", 0.0, e_dy=e_dzn[:, :, None])
        gz, e_gz = bbd.du[:, :, 0], bbd.e_du[:, :, 0]
        out.update(dgd=bbd.dgamma, dbd=bbd.dbeta)
    else:
        gz, e_gz = dzn, e_dzn
    _, _, h, amb, mag_h = _gate_mlp(u, torch.zeros_like(u), fc1, fc2)
    f1, f2 = fc1.double()[None], fc2.double()[None]
    on = (h > 0).double()
    hr = h.clamp_min(0.0)
    out["dfc2"] = Out((gz[:, :, None] * hr).sum(0), (gz.abs()[:, :, None] * hr).sum(0), B,
                      (e_gz[:, :, None] * hr + gz.abs()[:, :, None] * acc_term(mag_h, 3)).sum(0))
    gh = gz[:, :, None] * f2 * on                                   # [B, C, 3]
    e_gh = (e_gz[:, :, None] * f2.abs() + acc_term(gh.abs(), 1)) * on
    out["dfc1"] = Out((gh[..., None] * u[:, :, None, :]).sum(0), (gh.abs()[..., None] * u.abs()[:, :, None, :]).sum(0), B,
                      (e_gh[..., None] * u.abs()[:, :, None, :]).sum(0))
    du = (gh[..., None] * f1).sum(2)                                 # [B, C, 3]
    mag_du = (gh.abs()[..., None] * f1.abs()).sum(2)
    e_du = acc_term(mag_du, 3) + (e_gh[..., None] * f1.abs()).sum(2)
    sd = u[..., 2]
    live = sd > 0                                                    # aten::std_backward masks the 0 / 0 of a constant plane to 0
    dmax, dmean = du[..., 0], du[..., 1] / HW
    dstd = torch.where(live, du[..., 2] / (HW * sd.clamp_min(1e-300)), torch.zeros_like(sd))
    e_dstd = torch.where(live, e_du[..., 2] / (HW * sd.clamp_min(1e-300)), torch.zeros_like(sd)) + 2 * U_FP32 * dstd.abs()
    e_dmean = e_du[..., 1] / HW + U_FP32 * dmean.abs()
    pl = lambda t: t[:, :, None, None]  # noqa: E731
    at = torch.zeros(B, C, HW, dtype=torch.bool, device=x0.device)
    at.scatter_(2, amax.long()[:, :, None], True)
    at = at.reshape(B, C, H, W).double()
    gy = g_y1.double() if g_y1 is not None else torch.zeros_like(x0)
    d = g_xs * pl(sg) + pl(dmean) + pl(dstd) * (y1s - pl(u[..., 1])) + gy + at * pl(dmax)
    mag_d = g_xs.abs() * pl(sg) + pl(dmean).abs() + pl(dstd).abs() * (y1s.abs() + pl(u[..., 1]).abs()) + gy.abs() + at * pl(dmax).abs()
    e_d = (acc_term(mag_d, K_ELEM) + g_xs.abs() * e_sg + pl(e_dmean) + pl(e_dstd) * (y1s - pl(u[..., 1])).abs() + pl(dstd).abs() * e_y +
           at * pl(e_du[..., 0]))
    bb = bn_back(d, x0, 0.0, mean1, var1, g1, b1, eps1, "none", 0.0, e_dy=e_d)
    gt = g_tap.double() if g_tap is not None else torch.zeros_like(x0)
    out.update(dx0=_final(bb.du + gt, bb.e_du + acc_term(bb.du.abs() + gt.abs(), 1)), dg1=bb.dgamma, db1=bb.dbeta, hidden_amb=amb)
    return out


# ---- pooled branch: AdaptiveAvgPool(7) -> 1x1 conv -> BatchNorm -> LeakyReLU -> x7 (align_corners) -> (H, W) ------------------
def resample(z, H, W):
    """the float64 chain itself"""
    z = F.interpolate(z, scale_factor=7, mode="bilinear", align_corners=True)
    return F.interpolate(z, size=(H, W), mode="bilinear", align_corners=False)


def _adjoint(fn, x_like, g):
    """the transpose of the linear map fn at cotangent g (float64 autograd)"""
    x = torch.zeros_like(x_like, requires_grad=True)
    return torch.autograd.grad(fn(x), x, g)[0]


def _win(n):
    """largest adaptive-pool window along an axis of n"""
    return max(-(-(o + 1) * n // 7) - (o * n) // 7 for o in range(7))


def _taps(n):
    """rows of the composed map that can touch one of the 7 sources along an axis of n"""
    return min(n, 2 * -(-n // 7) + 2)


def pool_fwd(x, wc, gamma, beta, eps, slope, rmean, rvar, momentum):
    x, wc = x.double(), wc.double()
    B, P, H, W = x.shape
    pooled = F.adaptive_avg_pool2d(x, 7)
    mag_p = F.adaptive_avg_pool2d(x.abs(), 7)
    e_p = acc_term(mag_p, _win(H) * _win(W) + 1)
    t = torch.einsum("oi,bihw->bohw", wc, pooled)
    mag_t = torch.einsum("oi,bihw->bohw", wc.abs(), mag_p)
    e_t = acc_term(mag_t, P) + torch.einsum("oi,bihw->bohw", wc.abs(), e_p)
    st = chan_stats(t, e_t, rmean, rvar, momentum)
    pre, e = bn_apply(t, e_t, st, gamma, beta, eps)
    z = _act64(pre, "lrelu", slope)
    y = resample(z, H, W)
    mag_y = resample(z.abs(), H, W)
    e_y = acc_term(mag_y, 49) + 2 * C_MAP * U_FP32 * mag_y + resample(e + torch.zeros_like(z), H, W)
    return dict(y=_final(y, e_y), pooled=Out(pooled.reshape(B, P, 49), mag_p.reshape(B, P, 49), _win(H) * _win(W) + 1),
                t=Out(t.reshape(B, P, 49), mag_t.reshape(B, P, 49), P, e_t.reshape(B, P, 49) - acc_term(mag_t, P).reshape(B, P, 49)), **st.outs)


def pool_bwd(g, wc, gamma, beta, eps, slope, pooled, t, mean, var, H, W):
    """pooled, t [B, P, 49], mean, var: as given to the entry point"""
    g, wc = g.double(), wc.double()
    B, P = g.shape[:2]
    t4, p4 = t.double().reshape(B, P, 7, 7), pooled.double().reshape(B, P, 7, 7)
    up = lambda z: resample(z, H, W)  # noqa: E731
    dz = _adjoint(up, t4, g)
    mag = _adjoint(up, t4, g.abs())
    e_dz = acc_term(mag, _taps(H) * _taps(W)) + 2 * C_MAP * U_FP32 * mag
    bb = bn_back(dz, t4, 0.0, mean, var, gamma, beta, eps, "lrelu", slope, e_dy=e_dz)
    dwc = Out(torch.einsum("bohw,bihw->oi", bb.du, p4), torch.einsum("bohw,bihw->oi", bb.du.abs(), p4.abs()), B * 49,
              torch.einsum("bohw,bihw->oi", bb.e_du, p4.abs()))
    dp = torch.einsum("oi,bohw->bihw", wc, bb.du)
    mag_dp = torch.einsum("oi,bohw->bihw", wc.abs(), bb.du.abs())
    e_dp = acc_term(mag_dp, P + 1) + torch.einsum("oi,bohw->bihw", wc.abs(), bb.e_du)
    pool = lambda x: F.adaptive_avg_pool2d(x, 7)  # noqa: E731
    like = torch.zeros(B, P, H, W, dtype=torch.float64, device=g.device)
    dx, mag_dx = _adjoint(pool, like, dp), _adjoint(pool, like, mag_dp)
    return dict(dx=Out(dx, mag_dx, 4, _adjoint(pool, like, e_dp)), dwc=dwc, dgamma=bb.dgamma, dbeta=bb.dbeta, amb=bb.amb)


# ---- host measurement of the constants ---------------------------------------------------------------------------------------
def map64(n):
    """[n, 7] float64: one axis of the chain, from F.interpolate on the identity"""
    eye = torch.eye(7, dtype=torch.float64).reshape(7, 1, 7, 1).expand(7, 1, 7, 7).contiguous()
    return resample(eye, n, 7)[:, 0, :, 0].t().contiguous()


def measure_constants():
    """-> (gelu, gelu', sigmoid, map) ratios as the module docstring defines them: plain fp32 on the CPU against float64"""
    u = torch.linspace(-U_RANGE, U_RANGE, 2_000_001, dtype=torch.float64).float()
    u = u[u != 0]
    u64 = u.double()
    gelu32 = 0.5 * u * (1.0 + torch.erf(u * 0.70710678118654752))
    r_g = float(((gelu32.double() - _act64(u64, "gelu", 0.0)).abs() / (U_FP32 * u64.abs())).max())
    dg32 = 0.5 * (1.0 + torch.erf(u * 0.70710678118654752)) + u * (0.3989422804014327 * torch.exp(-0.5 * u * u))
    r_dg = float(((dg32.double() - _dact64(u64, "gelu", 0.0)).abs() / U_FP32).max())
    sg32 = 1.0 / (1.0 + torch.exp(-u))
    r_s = float(((sg32.double() - torch.sigmoid(u64)).abs() / U_FP32).max())
    from cenet_amd.ops import decoder_fused as DF
    r_m = 0.0
    for n in MAP_SIZES:
        r32 = DF._pool_matrices(n, n, "cpu")[0].double()
        r_m = max(r_m, float((r32 - map64(n)).abs().max() / U_FP32))
    return r_g, r_dg, r_s, r_m
