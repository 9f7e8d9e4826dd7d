"""Reference for LayerNorm and train-mode BatchNorm (norm.hip), for tests/test_norm_bounds.py: float64 evaluations of what
include/cenet_hip.h says each entry point means, with a magnitude `Mag` and a term count `K` per output, under the acceptance rule of
tests/gemm_ref.py.  Plain helper module: no fixtures.  Written from the header text, not from the kernels; `view`, `index_map`,
`expect`, the outside-the-footprint check and `_dact64` are conv_ref's, `round_once`, `ints`, `reals`, `bound_of` and the constants
gemm_ref's (imported, not copied).

Operands are strided VIEWS of the buffers the kernel is given.  A formula returns `Out(ref, mag, K, extra)`; an output is accepted when
    |got - ref| <= C_OUT u_out |ref| + C_ACC 2^-24 sqrt(K) Mag + extra                                   (u_out = 2^-8 bf16, 2^-24 fp32)
`extra` being the bounds of the statistics the output is computed from, propagated to first order (it is itself made of terms of the
same form; `as_exp` folds it into Mag so that conv_ref.assert_bound applies unchanged, footprint check included).

Magnitudes (n = elements of a row / of a channel over the batch, E = mean over them, u = 2^-24):
    mean        Mag = E|x|, K = n                                            b_mu  = C_OUT u |mu| + C_ACC u sqrt(n) E|x|
    var         Mag = var, K = n + K_ELEM, extra = b_mu^2                    b_var = C_OUT u var + C_VAR u sqrt(n + K_ELEM) var + b_mu^2
                (the mean of (x - m)^2 is var + (m - mu)^2 exactly: the square of the mean's own bound is what a two-pass form owes
                to its mean, and it keeps the bound of a constant row or plane above zero.  The bound holds for ANY data: a one-pass
                kernel has to shift its sums by something close to the mean to meet it)
    rstd, 1/sqrt(var + eps)       b_r = 1/2 r^3 b_var + RS_REL r             RS_REL = 3 u: the add var + eps (half an ulp, a quarter
                                                                             on the root) and a reciprocal root good to one ulp (2^-23)
    y = gamma (x - mu) r + beta   Mag = |gamma| r (|x| + |mu|) + |beta|, K = K_ELEM (not |x - mu|: x sc + (beta - mu sc) is a legitimate
                                  evaluation), extra = |gamma| r b_mu + |gamma| |x - mu| b_r; activations none / relu / lrelu are
                                  1-Lipschitz, so the bound of the pre-activation is the bound of act(pre)
    running statistics            (1 - m) old + m new: Mag the same with absolute values, K = K_ELEM, extra = m b_mu, m n/(n-1) b_var
    backward (mean and rstd / var are OPERANDS of the backward entry points: taken as given, no statistics bound)
        xh = (x - mu) r, Xh = (|x| + |mu|) r (x r - mu r is a legitimate evaluation: e_xh = C_ACC u sqrt(K_ELEM) Xh);
        LayerNorm: g = dy gamma, sums over the n = C columns of a row;   BatchNorm: g = dy act'(gamma xh + beta), sums over n = B HW
        m1 = E g:       e_m1 = C_ACC u sqrt(n) E|g|
        m2 = E(g xh):   e_m2 = C_ACC u sqrt(n) E|g xh| + C_ACC u sqrt(K_ELEM) E(|g| Xh)       (the sum; each term's own roundings)
        dx = s (g - m1 - xh m2) + dx_add, s = r [gamma r]:  Mag = |s| (|g| + |m1| + |xh m2|) + |dx_add|, K = K_ELEM,
                                                            extra = |s| (e_m1 + |xh| e_m2 + |m2| e_xh)
        dgamma  += sum dy xh  [sum g xh]:  Mag = sum |dy xh| + |previous|, K = rows [n], extra = C_ACC u sqrt(K_ELEM) sum |dy| Xh
        dbeta   += sum dy     [sum g]:     Mag = sum |dy| + |previous|,    K = rows [n]
    K_ELEM = 8: the fp32 operations of one output besides its sums.
relu / lrelu in the backward: an element whose float64 pre-activation lies within its own bound (the y bound above, statistics given)
of 0 is AMBIGUOUS: it is left out of the dx comparison, its |dy| goes to the channel's dbeta bound and its |dy xh| to the dgamma bound,
and, because E g and E(g xh) move with them, |gamma| r (that / n) and |gamma| r |xh| (that / n) go to every dx of the channel.  The
test asserts, on the reference alone, that at most 1 % of a case is ambiguous.

Constants: measured on the HOST, never on a kernel.  `measure_constants()` evaluates mean, two-pass variance and a column sum of
products in plain fp32 on the CPU (256 lane partials over a shuffled order, then the lanes) against float64, bf16-rounded operands,
in the normal (0.3 + 1.5 N) and offset (8 + 0.25 N) regimes, at the n of the case matrix:
    mean 0.384, sum of products 0.538 (in units of 2^-24 sqrt(n) Mag)  -> x 4 = 2.15 < 2.3: C_ACC stays gemm_ref's 2.3
    variance 1.387 (in units of 2^-24 sqrt(n + K_ELEM) var) -> x 4 = 5.55: C_ACC does not cover it, the variance gets C_VAR = 5.6.
    (The largest ratios come from n = 8, one element far from the rest: its square carries the sum, and the roundings on its way
    through a 256-lane reduction tree -- as deep for 8 elements as for 8000 -- all count in full; from n = 40 on the ratio is under 0.4.)
    bf16 store: gemm_ref's C_OUT = 1.0 (measured there 0.996)
(module constants below, pinned by test_norm_constants_are_the_host_measurement).  Not widened to make a kernel pass."""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from conv_ref import _dact64, _outside, assert_bound, expect, index_map, view  # noqa: F401
from gemm_ref import (BF, C_ACC, C_OUT, EXACT_LIMIT, U_BF16, U_FP32, _act64, bound_of, ints, reals, round_once)  # noqa: F401

MEASURED_MEAN, MEASURED_VAR, MEASURED_SUM = 0.384, 1.387, 0.538  # measure_constants() over the case matrix (pinned by a test)
C_VAR = 5.6  # 4 x MEASURED_VAR, rounded up: the variance's own constant
RS_REL = 3 * U_FP32
K_ELEM = 8


def Out(ref, mag, K, extra=0.0):
    return SimpleNamespace(ref=ref, mag=mag, K=K, extra=extra)


def acc_term(mag, K):
    return C_ACC * U_FP32 * math.sqrt(K) * mag


def as_exp(buf, off, shape, strides, o, *, add=False, dims=("row", "column"), kernel=""):
    """conv_ref.expect for an Out: `extra` becomes magnitude (extra / (C_ACC 2^-24 sqrt(K))), so that assert_bound's rule is the one above"""
    mag = (o.mag + o.extra / (C_ACC * U_FP32 * math.sqrt(o.K))) + torch.zeros_like(o.ref)
    return expect(buf, off, shape, strides, o.ref.expand(shape), mag.expand(shape), o.K, add=add, dims=dims, kernel=kernel)


# ---- statistics ----------------------------------------------------------------------------------------------------------------
def stats(x, dims):
    """mean / biased variance of a float64 tensor over `dims` (kept), with their bounds"""
    n = 1
    for d in dims:
        n *= x.shape[d]
    mu = x.mean(dims, keepdim=True)
    ax = x.abs().mean(dims, keepdim=True)
    var = ((x - mu) ** 2).mean(dims, keepdim=True)
    b_mu = bound_of(mu, ax, U_FP32, n)
    b_var = bound_of(var, var, U_FP32, n + K_ELEM, c_acc=C_VAR) + b_mu ** 2
    return SimpleNamespace(n=n, mu=mu, var=var, ax=ax, b_mu=b_mu, b_var=b_var)


def rsqrt_of(var, b_var, eps):
    r = (var + eps) ** -0.5
    return r, 0.5 * r ** 3 * b_var + RS_REL * r


def normalise(x, mu, b_mu, r, b_r, gamma, beta):
    """gamma (x - mu) r + beta (operands broadcast against x) -> (pre, bound of pre without a store rounding)"""
    pre = (x - mu) * r * gamma + beta
    mag = gamma.abs() * r * (x.abs() + mu.abs()) + beta.abs()
    return pre, acc_term(mag, K_ELEM) + gamma.abs() * r * b_mu + gamma.abs() * (x - mu).abs() * b_r


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------
def ln_fwd(x, gamma, beta, eps):
    """x [rows, C] -> dict of Outs: mean, rstd [rows], y [rows, C]"""
    x, g, b = x.double(), gamma.double()[None], beta.double()[None]
    st = stats(x, (1,))
    r, b_r = rsqrt_of(st.var, st.b_var, eps)
    y, e_y = normalise(x, st.mu, st.b_mu, r, b_r, g, b)
    return dict(mean=Out(st.mu[:, 0], st.ax[:, 0], st.n), rstd=Out(r[:, 0], torch.zeros_like(r[:, 0]), 1, b_r[:, 0]),
                y=Out(y, torch.zeros_like(y), 1, e_y), st=st)


def ln_bwd(dy, x, gamma, mean, rstd, dx_add=None):
    """mean / rstd [rows] as given to the kernel -> dx [rows, C], dgamma / dbeta [C] (the sums, to be ADDED)"""
    dy, x, g = dy.double(), x.double(), gamma.double()[None]
    mu, r = mean.double()[:, None], rstd.double()[:, None]
    rows, C = x.shape
    xh, Xh = (x - mu) * r, (x.abs() + mu.abs()) * r
    gg = dy * g
    s1, s2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    dx, mag, extra = _dx(r, gg, xh, Xh, s1, s2, (1,), dx_add)
    return dict(dx=Out(dx, mag, K_ELEM, extra), dbeta=Out(dy.sum(0), dy.abs().sum(0), rows),
                dgamma=Out((dy * xh).sum(0), (dy * xh).abs().sum(0), rows, acc_term((dy.abs() * Xh).sum(0), K_ELEM)))


def _dx(s, g, xh, Xh, m1, m2, dims, dx_add):
    """s (g - m1 - xh m2) + dx_add with its magnitude and the propagated bounds of m1, m2 and xh (module docstring)"""
    n = 1
    for d in dims:
        n *= g.shape[d]
    e_m1 = acc_term(g.abs().mean(dims, keepdim=True), n)
    e_m2 = acc_term((g * xh).abs().mean(dims, keepdim=True), n) + acc_term((g.abs() * Xh).mean(dims, keepdim=True), K_ELEM)
    dx = s * (g - m1 - xh * m2)
    mag = s.abs() * (g.abs() + m1.abs() + (xh * m2).abs())
    extra = s.abs() * (e_m1 + xh.abs() * e_m2 + m2.abs() * acc_term(Xh, K_ELEM))
    if dx_add is not None:
        dx, mag = dx + dx_add.double(), mag + dx_add.double().abs()
    return dx, mag, extra


def ln_fold(part, C):
    """part [nrows, 2 C] -> the column sums that go to dgamma, dbeta"""
    p = part.double()
    s, a = p.sum(0), p.abs().sum(0)
    return Out(s[:C], a[:C], p.shape[0]), Out(s[C:], a[C:], p.shape[0])


def ln_acc_pre(acc, bias):
    """xpre = bf16(acc + bias): the sum before its one rounding"""
    a = acc.double()
    b = bias.double()[None] if bias is not None else torch.zeros_like(a)
    return Out(a + b, a.abs() + b.abs(), 1)


# ---- BatchNorm: x [B, C, HW] (BatchNorm1d: HW = 1) -------------------------------------------------------------------------------
def bn_stats(x, rmean=None, rvar=None, momentum=0.1):
    """-> dict of Outs over [C]: mean, var (biased), and with running buffers rmean, rvar (variance times n / (n - 1))"""
    st = stats(x.double(), (0, 2))
    sq = lambda t: t[0, :, 0]  # noqa: E731
    out = dict(mean=Out(sq(st.mu), sq(st.ax), st.n), var=Out(sq(st.var), sq(st.var) * (C_VAR / C_ACC), st.n + K_ELEM, sq(st.b_mu) ** 2), st=st)
    if rmean is not None:
        m, n = momentum, st.n
        rm, rv = rmean.double(), rvar.double()
        unb = n / (n - 1.0)
        out["rmean"] = Out((1 - m) * rm + m * sq(st.mu), (1 - m) * rm.abs() + m * sq(st.mu).abs(), K_ELEM, m * sq(st.b_mu))
        out["rvar"] = Out((1 - m) * rv + m * sq(st.var) * unb, (1 - m) * rv.abs() + m * sq(st.var) * unb, K_ELEM, m * unb * sq(st.b_var))
    return out


def _ch(t):
    return t.double()[None, :, None]


def bn_fwd(x, mean, var, gamma, beta, eps, act, slope, b_mu=0.0, b_var=0.0):
    """y = act(gamma (x - mean) / sqrt(var + eps) + beta); mean / var [C]: given to the kernel (bounds 0) or the batch statistics of
    the same call (their bounds) -> Out y, pre, bound of pre"""
    x = x.double()
    r, b_r = rsqrt_of(_ch(var), b_var, eps)
    pre, e = normalise(x, _ch(mean), b_mu, r, b_r, _ch(gamma), _ch(beta))
    y = _act64(pre, act, slope)
    return Out(y, torch.zeros_like(y), 1, e), pre, e


def bn_bwd(dy, x, mean, var, gamma, beta, eps, act, slope, dx_add=None):
    """mean / var [C] as given -> dict: dx [B, C, HW], dgamma / dbeta [C] (sums, to be ADDED), amb (the ambiguous elements)"""
    dy, x = dy.double(), x.double()
    mu, g, b = _ch(mean), _ch(gamma), (_ch(beta) if beta is not None else 0.0)
    r, _ = rsqrt_of(_ch(var), 0.0, eps)
    n = x.shape[0] * x.shape[2]
    xh, Xh = (x - mu) * r, (x.abs() + mu.abs()) * r
    pre = xh * g + b
    if act == "none":
        amb = torch.zeros_like(pre, dtype=torch.bool)
    else:
        amb = pre.abs() <= acc_term(Xh * g.abs() + abs(b), K_ELEM) + RS_REL * Xh * g.abs()
    gd = dy * _dact64(pre, act, slope)
    ag = gd.abs()
    m1, m2 = gd.mean((0, 2), keepdim=True), (gd * xh).mean((0, 2), keepdim=True)
    amb_b = (dy.abs() * amb).sum((0, 2), keepdim=True)
    amb_g = ((dy * xh).abs() * amb).sum((0, 2), keepdim=True)
    dx, mag, extra = _dx(g * r, gd, xh, Xh, m1, m2, (0, 2), dx_add)
    extra = extra + g.abs() * r * (amb_b / n + xh.abs() * amb_g / n)
    extra = torch.where(amb, torch.full_like(extra, math.inf), extra)
    return dict(dx=Out(dx, mag, K_ELEM, extra), amb=amb,
                dgamma=Out((gd * xh).sum((0, 2)), (gd * xh).abs().sum((0, 2)), n,
                           amb_g[0, :, 0] + acc_term((ag * Xh).sum((0, 2)), K_ELEM)),
                dbeta=Out(gd.sum((0, 2)), ag.sum((0, 2)), n, amb_b[0, :, 0]))


# ---- host measurement of the constants ---------------------------------------------------------------------------------------
def _lanes32(v, g):
    """plain fp32 sum: a shuffled order dealt to 256 lane partials, then the lanes"""
    v = v[torch.randperm(v.numel(), generator=g)]
    pad = (-v.numel()) % 256
    v = torch.cat([v, torch.zeros(pad)]).view(-1, 256)
    lanes = torch.zeros(256)
    for row in v:
        lanes = lanes + row
    return lanes.sum()


def measure_constants(ns, seed=0, draws=20):
    """ns: the element counts n of the case matrix.  fp32 mean, two-pass variance and sum of products on the CPU against float64,
    bf16-rounded operands in both regimes -> (mean, variance, sum-of-products) ratios in units of 2^-24 sqrt(n) Mag"""
    g = torch.Generator().manual_seed(seed)
    r_mu = r_var = r_sum = 0.0
    for n in ns:
        for (m, s) in ((0.3, 1.5), (8.0, 0.25)):
            for _ in range(draws):
                x = (m + s * reals((n,), g)).to(BF).float()
                dy = reals((n,), g).to(BF).float()
                st = stats(x.double()[None], (1,))
                mu32 = _lanes32(x, g) / n
                var32 = _lanes32((x - mu32) * (x - mu32), g) / n
                sq = math.sqrt(n) * U_FP32
                r_mu = max(r_mu, abs(float(mu32) - float(st.mu)) / (sq * float(st.ax)))
                sv = math.sqrt(n + K_ELEM) * U_FP32
                r_var = max(r_var, abs(float(var32) - float(st.var)) / (sv * float(st.var) + float(st.b_mu) ** 2))
                ref = float((x.double() * dy.double()).sum())
                r_sum = max(r_sum, abs(float(_lanes32(x * dy, g)) - ref) / (sq * float((x.double() * dy.double()).abs().sum())))
    return r_mu, r_var, r_sum
