"""Reference for the fused PVT MLP kernels (pvt_mlp.hip), for tests/test_pvt_mlp_bounds.py: float64 evaluations of what
include/cenet_hip.h says cenet_pvt_mlp_fwd_bf16 / cenet_pvt_mlp_bwd_bf16 mean, STAGE BY STAGE, under the acceptance rule of
tests/gemm_ref.py, tests/norm_ref.py and tests/chanloc_ref.py
    |got - ref| <= C_OUT u_out |ref| + C_ACC 2^-24 sqrt(K) Mag + extra                                   (u_out = 2^-8 bf16, 2^-24 fp32)
Plain helper module: no fixtures.  Written from the header text and PyTorch's float64 ops, not from the kernels.  `expect`,
`assert_bound`, `dw3x3`, `dw3x3_wgrad` are conv_ref's, `Out`, `acc_term`, `as_exp`, `ln_fwd`, `ln_bwd`, `ln_fold` norm_ref's, `stored`
chanloc_ref's (imported, not copied), and so is every constant.

Each stage is checked against the reference applied to the kernel's OWN STORED output of the stage before it (`got`), so every bound
is that of one LayerNorm, GEMM or conv step and nothing compounds; by induction the whole chain is held.
    forward   xn, mean, rstd   norm_ref.ln_fwd(x)
              h                got xn @ w1^T + b1                      K = C,  Mag = |xn| |w1|^T + |b1|
              a                s_b GELU(u), u = DW3x3(got h) + bd      e_u = C_ACC u sqrt(9) Mag_u; e_a = L_gelu e_u + (C_GELU 2^-24 + AS_H) |u|;
                               rounded ONCE from fp32 (the scale is one more fp32 product: K = 1 on |s_b a|)
              y                bscale NULL or s_b = 1: x + (got a @ w2^T + b2), K = HD
                               s_b = 0: x, bit for bit (`y_exact_rows`)
                               otherwise got a carries the scale and a second rounding: a = stored(GELU(u)) -- the reference rounds
                               too, and only where a bf16 rounding boundary lies within e_a of the float64 value is the bound the
                               distance of the two candidates -- and |s_b| e_a |w2|^T goes into y's bound.  Nothing is left out.
    backward  (h, x, mean, rstd, g: operands of the entry point)
              gu               da GELU'(u), da = stored(s_b (g @ w2)) (K = C; the header: rounded to bf16 BEFORE the multiply),
                               e_d = L_DGELU e_u + C_DGELU 2^-24 + AS_DG
              dwd, dbd         sums of the UNROUNDED da GELU' against the windows of h (the header), K = B H W, any order
              dh               DW3x3 with the mirrored taps of got gu, K = 9
              dx               g + ln_bwd(t), t = got dh @ w1 (K = HD; its bound e_t carried through the LayerNorm backward)
              dln_g, dln_b     column sums of t xhat and of t (norm_ref.ln_bwd's, + the sums of e_t |xhat|, e_t)
              db2              column sums of s_b g, K = B H W
              dxs              bf16(up_scale_b * float(dx as stored)): exact (`dxs_exact`, fp32 on the host: one IEEE product, one rounding)
Constants, all as they are: C_ACC, C_OUT (gemm_ref, measured 0.563 x 4 / 0.996), C_VAR, RS_REL, K_ELEM (norm_ref), L_gelu = 1.13
(gemm_ref.ACT_LIPSCHITZ), L_DGELU = 0.8 (conv_ref, measured 0.7979), C_GELU, C_DGELU (chanloc_ref.measure_constants: 1.712, 2.185 x 4),
AS_H, AS_DG (stated in the header), U_RANGE = 24 (the range C_GELU / C_DGELU were measured over: the tests assert |u| <= U_RANGE on
the reference).  Nothing new, nothing measured on a kernel, nothing widened to make a kernel pass."""
from __future__ import annotations

import torch

from chanloc_ref import AS_DG, AS_H, C_DGELU, C_GELU, U_RANGE, stored  # noqa: F401
from conv_ref import L_DGELU, assert_bound, dw3x3, dw3x3_wgrad, expect  # noqa: F401
from gemm_ref import ACT_LIPSCHITZ, BF, U_BF16, U_FP32, _act64  # noqa: F401
from norm_ref import (C_ACC, C_OUT, C_VAR, K_ELEM, RS_REL, Out, _dact64, acc_term, as_exp, bound_of, ln_bwd, ln_fold, ln_fwd)  # noqa: F401


def _planes(t, B, H, W):
    """[B, H W, HD] tokens -> float64 [B, HD, H, W]"""
    return t.double().reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _tokens(p):
    """[B, HD, H, W] -> [B, H W, HD]"""
    B, HD, H, W = p.shape
    return p.permute(0, 2, 3, 1).reshape(B, H * W, HD)


def _scale(bscale, B, like):
    """s_b per sample as float64 [B, 1, 1] (1 where there is no DropPath scale)"""
    s = torch.ones(B, dtype=torch.float64, device=like.device) if bscale is None else bscale.double()
    return s.reshape(B, 1, 1)


def preact(h, wd, bd, B, H, W):
    """u = DW3x3(h) + bd of tokens h [B, H W, HD] -> (u, e_u) as tokens"""
    u, mag, K = dw3x3(_planes(h, B, H, W), wd.reshape(-1, 9), bd)
    return _tokens(u), _tokens(acc_term(mag, K))


def gelu_of(u, e_u):
    """-> (GELU(u), bound of its fp32 evaluation by the bf16 instances' form, before the store)"""
    return _act64(u, "gelu", 0.0), ACT_LIPSCHITZ["gelu"] * e_u + (C_GELU * U_FP32 + AS_H) * u.abs()


def dgelu_of(u, e_u):
    return _dact64(u, "gelu", 0.0), L_DGELU * e_u + C_DGELU * U_FP32 + AS_DG


def _final(val, e, mag=None, K=1):
    return Out(val, torch.zeros_like(val) if mag is None else mag, K, e + torch.zeros_like(val))


# ---- forward -------------------------------------------------------------------------------------------------------------------
def fwd(x, ln_g, ln_b, eps, w1, b1, wd, bd, w2, b2, bscale, got, B, H, W):
    """x [B, H W, C] bf16; w1 [HD, C], w2 [C, HD] the bf16 operands; got: the kernel's stored xn, h, a -> dict of Outs xn, mean, rstd
    [B H W (, C)], h, a [B, H W, HD], y [B, H W, C], `u` (float64 pre-activation, for the range assertion) and `y_exact_rows` (bool [B]:
    the samples whose y must equal x bit for bit)"""
    C, HD = x.shape[-1], w1.shape[0]
    x2 = x.double().reshape(-1, C)
    ln = ln_fwd(x2, ln_g, ln_b, eps)
    out = dict(xn=ln["y"], mean=ln["mean"], rstd=ln["rstd"])
    xn, w1d, w2d = got["xn"].double().reshape(-1, C), w1.double(), w2.double()
    out["h"] = Out((xn @ w1d.t() + b1.double()).reshape(B, H * W, HD), (xn.abs() @ w1d.abs().t() + b1.double().abs()).reshape(B, H * W, HD), C)
    u, e_u = preact(got["h"], wd, bd, B, H, W)
    a, e_a = gelu_of(u, e_u)
    s = _scale(bscale, B, x)
    out["a"] = _final(s * a, s.abs() * e_a, (s * a).abs() if bscale is not None else None, 1)
    out["u"] = u
    # y from the kernel's a where a is recoverable from it (s_b = 1), from the reference's own rounded a elsewhere
    ak, b2d, xd = got["a"].double(), b2.double(), x.double()
    y1 = xd + (ak @ w2d.t() + b2d)
    m1 = xd.abs() + (ak.abs() @ w2d.abs().t() + b2d.abs())
    if bscale is None:
        out["y"], out["y_exact_rows"] = Out(y1, m1, HD), torch.zeros(B, dtype=torch.bool, device=x.device)
        return out
    ar, e_ar = stored(a, e_a, BF)
    ys = xd + s * (ar @ w2d.t() + b2d)
    ms = xd.abs() + s.abs() * (ar.abs() @ w2d.abs().t() + b2d.abs())
    es = s.abs() * (e_ar @ w2d.abs().t())
    one = s == 1.0
    out["y"] = Out(torch.where(one, y1, ys), torch.where(one, m1, ms), HD, torch.where(one, torch.zeros_like(es), es))
    out["y_exact_rows"] = (s == 0.0).reshape(B)
    return out


# ---- backward ------------------------------------------------------------------------------------------------------------------
def bwd(g, bscale, w1, w2, wd, bd, h, x, ln_g, mean, rstd, got, B, H, W):
    """operands as given to the entry point; got: the kernel's stored gu, dh -> dict of Outs gu, dh [B, H W, HD], dx [B, H W, C], and the
    sums (to be ADDED) dwd [HD, 9], dbd [HD], dln_g, dln_b, db2 [C]; `u` the float64 pre-activation"""
    C, HD = x.shape[-1], w1.shape[0]
    gd, w1d, w2d = g.double(), w1.double(), w2.double()
    s = _scale(bscale, B, x)
    da0 = s * (gd @ w2d)
    mag_da = s.abs() * (gd.abs() @ w2d.abs())
    da, e_da = stored(da0, acc_term(mag_da, C) + acc_term(da0.abs(), 1), BF)  # (the header: da is rounded to bf16 before the multiply)
    u, e_u = preact(h, wd, bd, B, H, W)
    d, e_d = dgelu_of(u, e_u)
    p = da * d                                                                 # the fp32 product: what dwd / dbd sum, what gu rounds
    e_p = e_da * d.abs() + da.abs() * e_d + acc_term(p.abs(), 1)
    out = dict(gu=_final(p, e_p), u=u)
    hp, pp, ep = _planes(h, B, H, W), _planes(p, B, H, W), _planes(e_p, B, H, W)
    (dw, mag_w), (db, mag_b), K = dw3x3_wgrad(hp, pp)
    out["dwd"] = Out(dw, mag_w, K, dw3x3_wgrad(hp.abs(), ep)[0][0])
    out["dbd"] = Out(db, mag_b, K, ep.sum((0, 2, 3)))
    # dh from the kernel's gu: the transposed conv is the conv with the mirrored taps
    dh, mag_h, K9 = dw3x3(_planes(got["gu"], B, H, W), wd.reshape(-1, 9), None, 1, flip=True)
    out["dh"] = Out(_tokens(dh), _tokens(mag_h), K9)
    # dx, dln_g, dln_b from the kernel's dh
    dhk = got["dh"].double().reshape(-1, HD)
    t, e_t = dhk @ w1d, acc_term(dhk.abs() @ w1d.abs(), HD)
    x2, g2 = x.double().reshape(-1, C), gd.reshape(-1, C)
    lb = ln_bwd(t, x2, ln_g, mean, rstd, dx_add=g2)
    gam, r = ln_g.double()[None].abs(), rstd.double()[:, None].abs()
    xh = ((x2 - mean.double()[:, None]) * rstd.double()[:, None]).abs()
    eg = gam * e_t
    e_dx = r * (eg + eg.mean(1, keepdim=True) + xh * (eg * xh).mean(1, keepdim=True))
    o = lb["dx"]
    out["dx"] = Out(o.ref.reshape(B, H * W, C), o.mag.reshape(B, H * W, C), o.K, (o.extra + e_dx).reshape(B, H * W, C))
    o = lb["dgamma"]
    out["dln_g"] = Out(o.ref, o.mag, o.K, o.extra + (e_t * xh).sum(0))
    o = lb["dbeta"]
    out["dln_b"] = Out(o.ref, o.mag, o.K, o.extra + e_t.sum(0))
    sg = (s * gd).reshape(-1, C)
    out["db2"] = Out(sg.sum(0), sg.abs().sum(0), sg.shape[0])
    return out


def dxs_exact(dx, up_scale):
    """what dxs must hold, bit for bit: bf16(up_scale_b * float(dx as stored)), one fp32 product and one rounding"""
    return (up_scale.float().reshape(-1, 1, 1) * dx.float()).to(BF)
