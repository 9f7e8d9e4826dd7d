"""The channel-local fused chains (chanloc.hip), entry point by entry point, held per element to the float64 reference of
tests/chanloc_ref.py: eucb, cfam_mid, dwbn, cfam_front, dwact and pool_branch, forward and backward, fp32 and bf16 storage.

* The reference is the header's meaning of each entry point evaluated step by step in float64 (chanloc_ref), NOT the launch chain the
  fused form replaces (tests/test_chanloc.py compares those two: both are code under test).
* Destinations sit in sentinel-filled buffers with a lead offset, operands in NaN-filled ones; nothing outside the footprint may change
  (bitwise).  Every entry point that takes batch strides runs at least one case as a channel slice of a wider, padded tensor.
  Accumulated outputs (dw, dgamma, dbeta, dls, dwc, dbias) are checked as += onto a non-zero previous value; running statistics and
  batch counters are compared too.  The backward entry points take mean / var as operands: the reference's, rounded to fp32.
* data regimes, each on every case (bf16-exact values): normal 0.3 + 1.5 N; offset 8 + 0.25 N; constant (channel 1 constant -- for the
  conv chains constant in the plane interior --, integer cotangents and previous values: dbeta is compared EXACTLY where no element of the
  channel is ambiguous); outlier / outlier3: the offset regime with the sample the one-pass statistics used to shift by, and its 3x3
  neighbourhood, set to 0 (the channel's first element for cfam_mid, cfam_front and pool, the input pixels that feed the conv output at
  (H/2, W/2) of image 0 for eucb and dwbn).
* relu / lrelu in a backward pass: chanloc_ref's ambiguity rule; at most 1 % of a case may be ambiguous, asserted on the reference alone
  before any kernel runs (test_ambiguity_cap_on_the_reference checks every case and regime without a kernel).
* CASES: the smallest shapes at which each form can still go wrong; the class each row is meant for is re-derived from the host code
  (own_pick, cfam_mid_launch, dwact_launch, dwbn_launch, eucb_bwd_group, dwact_bordered, pool_ok) in the comment on the row.
* mutation self-test (no kernel): deliberately wrong references must be rejected by the rule in the normal and the offset regime.
`sim` = the kernel sources on the host SIMT checker (CPU); `hip` = the gfx950 library (marker gpu)."""
import pytest
import torch

import chanloc_ref as R
from norm_ref import EXACT_LIMIT
from backend import dev  # noqa: F401
from cenet_amd import kern
from cenet_amd.ops import decoder_fused as DF
from test_norm_bounds import NAN, SENTINEL, _acc, _affine, _cot, _prev, _sync, _vecdest, _wide

BF, F32 = torch.bfloat16, torch.float32
EPS, SLOPE, MOM = 1e-5, 0.25, 0.1
REGIMES = ("normal", "offset", "constant", "outlier", "outlier3")
WORST = {}


# ---- data ----------------------------------------------------------------------------------------------------------------------
def _x(shape, g, regime, at):
    """[B, C, H, W] bf16-exact; at = (i, j, dil): the outlier's pixel of image 0 (and its 3x3 neighbourhood at that dilation)"""
    m, s = (0.3, 1.5) if regime == "normal" else (8.0, 0.25)
    if regime == "constant":
        m, s = 0.3, 1.5
    x = (m + s * R.reals(shape, g)).to(BF).float()
    H, W = shape[-2:]
    if regime == "constant":
        x[:, min(1, shape[1] - 1)] = 1.75
    if regime in ("outlier", "outlier3"):
        i, j, dil = at
        k = 1 if regime == "outlier3" else 0
        for di in range(-k, k + 1):
            for dj in range(-k, k + 1):
                ii, jj = i + di * dil, j + dj * dil
                if 0 <= ii < H and 0 <= jj < W:
                    x[0, :, ii, jj] = 0.0
    return x


def _w(shape, g, scale=0.3):
    return (scale * R.reals(shape, g)).to(BF).float()


def _src(x, d, dt, strided, fill=NAN):
    """x [B, C, H, W] -> (buffer, offset, batch stride, float64-able view): contiguous at a lead offset, or channels [1, 1 + C) of a
    [B, C + 2, H, W] tensor whose images lie 8 elements further apart"""
    B, C, H, W = x.shape
    buf, off, sb = _wide(x.reshape(B, C, H * W), d, dt, 8, C + 2 if strided else C, 1 if strided else 0, 8 if strided else 0, fill)
    return buf, off, sb, R.view(buf, off, (B, C, H, W), (sb, H * W, W, 1))


def _dst(shape, d, dt, strided):
    return _src(torch.full(shape, SENTINEL), d, dt, strided, SENTINEL)[:3]


def _st4(sb, H, W):
    return (sb, H * W, W, 1)


def _vexp(o, d, name, prev=None, add=False):
    """a [n] fp32 destination (previous contents `prev`) inside a sentinel-filled buffer -> (buffer, expectation)"""
    n = o.ref.numel()
    buf = _vecdest(n, d, prev)
    return buf, R.as_exp(buf, 4, (n,), (1,), o, add=add, dims=("entry",), kernel=name)


def _stat_dests(o, d, C, g, sfx=""):
    """mean / var / running statistics destinations of a forward chain -> (exps, pointers dict)"""
    exps, ptr = [], {}
    for k in ("mean", "var", "rmean", "rvar"):
        buf, e = _vexp(o[k + sfx], d, k + sfx, prev=o["_prev_" + k + sfx] if k.startswith("r") else None)
        exps.append((buf, e))
        ptr[k] = buf[4:]
    return exps, ptr


def _running(C, g, d):
    return (0.2 * R.reals((C,), g)).to(d), (torch.rand(C, generator=g) + 0.5).to(d)


def _accs(o, d, g, regime, names):
    """accumulators with non-zero previous contents for the Outs `names` -> (exps, pointers dict, previous values dict)"""
    exps, ptr, prevs = [], {}, {}
    for k in names:
        n = o[k].ref.numel()
        prev = _prev(n, g, regime)
        buf, lead = _acc(prev, d)
        exps.append((buf, R.as_exp(buf, lead, o[k].ref.shape, _contig(o[k].ref.shape), o[k], add=True,
                                   dims=tuple(f"d{i}" for i in range(o[k].ref.dim())), kernel=k)))
        ptr[k], prevs[k] = buf[lead:], prev
    return exps, ptr, prevs


def _contig(shape):
    st, s = [], 1
    for n in reversed(shape):
        st.append(s)
        s *= n
    return tuple(reversed(st))


def _amb_ok(amb, what):
    frac = float(amb.double().mean())
    assert frac <= 0.01, f"{what}: {frac:.3%} of the elements are ambiguous for the activation's derivative"


def _exact_dbeta(got, prev, o, amb, regime, what):
    """constant regime: integer cotangents, slope 1/4, integer previous value -> the sum is exact in any order, for the channels
    without an ambiguous element"""
    if regime != "constant":
        return
    clean = ~amb.transpose(0, 1).reshape(amb.shape[1], -1).any(1).cpu()
    want = prev.double() + o.ref.cpu()
    assert float(o.mag.max()) + float(prev.abs().max()) < EXACT_LIMIT
    assert torch.equal(got.cpu().double()[clean], want[clean]), f"{what}: dbeta of integer cotangents is not the exact sum"


def _check(exps, kernel, regime, d):
    worst = 0.0
    for got, exp in exps:
        worst = max(worst, R.assert_bound(got, exp, f"{kernel} [{regime}]"))
    key = (kernel, regime, d.type)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"BOUND {kernel} [{regime}]: worst |err| / bound = {WORST[key]:.3f} (this case {worst:.3f})")
    return worst


def _tn(dt):
    return "bf16" if dt == BF else "f32"


def _gen(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ---- eucb ----------------------------------------------------------------------------------------------------------------------
def eucb_ref(d, regime, dt, B, H, W, strided, C=3):
    g = _gen(1, B, H, W)
    x = _x((B, C, H, W), g, regime, (H // 2, W // 2, 1))
    w, (gamma, beta) = _w((C, 9), g).to(d), _affine(C, g)
    cot = _cot((B, C, 2 * H, 2 * W), g, regime)
    rm, rv = _running(C, g, d)
    xs = _src(x, d, dt, strided)
    gs = _src(cot, d, dt, strided)
    gamma, beta = gamma.to(d), beta.to(d)
    of = R.eucb_fwd(xs[3], w, gamma, beta, EPS, SLOPE, rm, rv, MOM)
    mean, var = of["mean"].ref.float(), of["var"].ref.float()
    ob = R.eucb_bwd(gs[3], xs[3], w, gamma, beta, EPS, SLOPE, mean, var)
    _amb_ok(ob["amb"], f"eucb {B, H, W} {regime}")
    return dict(g=g, xs=xs, gs=gs, w=w, gamma=gamma, beta=beta, rm=rm, rv=rv, of=of, ob=ob, mean=mean, var=var, C=C)


def run_eucb(d, regime, dt, B, H, W, strided=False):
    r = eucb_ref(d, regime, dt, B, H, W, strided)
    C, of, ob, g = r["C"], r["of"], r["ob"], r["g"]
    (xb, xo, sxb, _), (gb, go, sgb, _) = r["xs"], r["gs"]
    of.update(_prev_rmean=r["rm"].cpu(), _prev_rvar=r["rv"].cpu())
    yb, yo, syb = _dst((B, C, 2 * H, 2 * W), d, dt, strided)
    exps, sp = _stat_dests(of, d, C, g)
    exps.append((yb, R.as_exp(yb, yo, (B, C, 2 * H, 2 * W), _st4(syb, 2 * H, 2 * W), of["y"], dims=("image", "channel", "y", "x"), kernel="y")))
    nbt = torch.tensor([3, 5], dtype=torch.int64).to(d)
    if strided:
        kern._call("cenet_eucb_fwd_f32", kern.Ptr(xb, xo), sxb, r["w"], r["gamma"], r["beta"], EPS, SLOPE, kern.Ptr(yb, yo), syb,
                   sp["mean"], sp["var"], sp["rmean"], sp["rvar"], MOM, nbt, B, C, H, W)
    else:
        kern.eucb_fwd(xb[xo:], r["w"], r["gamma"], r["beta"], EPS, SLOPE, yb[yo:], sp["mean"], sp["var"], sp["rmean"], sp["rvar"], MOM,
                      nbt, B, C, H, W)
    _sync(d)
    assert nbt.cpu().tolist() == [4, 5]
    _check(exps, f"eucb_fwd<{_tn(dt)}>", regime, d)
    dxb, do, sdb = _dst((B, C, H, W), d, dt, strided)
    exps, ap, prevs = _accs(ob, d, g, regime, ("dw", "dgamma", "dbeta"))
    exps.append((dxb, R.as_exp(dxb, do, (B, C, H, W), _st4(sdb, H, W), ob["dx"], dims=("image", "channel", "y", "x"), kernel="dx")))
    if strided:
        kern._call("cenet_eucb_bwd_acc_f32", kern.Ptr(gb, go), sgb, kern.Ptr(xb, xo), sxb, r["w"], r["gamma"], r["beta"], EPS, SLOPE,
                   r["mean"], r["var"], kern.Ptr(dxb, do), sdb, ap["dw"], ap["dgamma"], ap["dbeta"], B, C, H, W)
    else:
        kern.eucb_bwd(gb[go:], xb[xo:], r["w"], r["gamma"], r["beta"], EPS, SLOPE, r["mean"], r["var"], dxb[do:], ap["dw"], ap["dgamma"],
                      ap["dbeta"], B, C, H, W)
    _sync(d)
    _exact_dbeta(ap["dbeta"][:C], prevs["dbeta"], ob["dbeta"], ob["amb"], regime, "eucb_bwd")
    _check(exps, f"eucb_bwd<{_tn(dt)}>", regime, d)


# forward: B (H + 2)(W + 2) 4 bytes <= 48 KB -> 512 threads / 48 KB, else 1024 threads / 152 KB.  backward: G = (LDS - source
# planes) / (4 (2H + 2)(2W + 2)) images per group, 48 KB if G >= 4 or G == B, else 152 KB (eucb_bwd_group)
EUCB_CASES = [
    (2, 4, 4, False),     # smallest supported (HW = 16); backward 48 KB, G = B: one group
    (2, 5, 6, True),      # odd, non-square plane; batch strides of a channel slice
    (3, 6, 11, False),    # W odd
    (12, 14, 14, False),  # 48 KB both ways; backward G = (49152 - 12288) / 3600 = 10: groups of 10 + 2
    (4, 28, 28, False),   # forward 14400 B: 48 KB; backward 48 KB G = 2 < 4 -> 152 KB, G = 4 = B: one group
    (14, 28, 28, True),   # forward 50400 B > 48 KB: 1024 threads, 152 KB; backward (155648 - 50400) / 13456 = 7: groups of 7 + 7
    (6, 40, 40, False),   # forward 42336 B: 48 KB; backward 48 KB G = 0 -> 152 KB, (155648 - 42336) / 26896 = 4: groups of 4 + 2
]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", EUCB_CASES, ids=lambda c: "x".join(str(v) for v in c[:3]) + ("-slice" if c[3] else ""))
def test_eucb_bounds(dev, case, regime):
    for dt in (F32, BF):
        run_eucb(dev, regime, dt, *case)


# ---- cfam_mid ------------------------------------------------------------------------------------------------------------------
def run_mid(d, regime, dt, B, H, W, C=3):
    HW = H * W
    g = _gen(2, B, H, W)
    p_raw = _x((B, C, H, W), g, regime, (0, 0, 1))
    m, x0 = _x((B, C, H, W), g, "normal", None), _x((B, C, H, W), g, "offset" if regime != "normal" else "normal", None)
    cy, cx = _cot((B, C, H, W), g, regime), _cot((B, C, H, W), g, regime)
    (gp, bp), (g2, b2) = _affine(C, g), _affine(C, g)
    gp, bp, g2, b2 = gp.to(d), bp.to(d), g2.to(d), b2.to(d)
    wv, ls = torch.tensor([0.625]).to(d), (0.5 + 0.25 * torch.arange(C)).to(d)
    (rmp, rvp), (rm2, rv2) = _running(C, g, d), _running(C, g, d)
    ps, ms, xs, ys, gxs = (_src(t, d, dt, False) for t in (p_raw, m, x0, cy, cx))
    of = R.cfam_mid_fwd(ps[3], ms[3], xs[3], gp, bp, EPS, wv, ls, g2, b2, 1e-3, rmp, rvp, MOM, rm2, rv2, 0.2, dt)
    of.update(_prev_rmean_p=rmp.cpu(), _prev_rvar_p=rvp.cpu(), _prev_rmean_2=rm2.cpu(), _prev_rvar_2=rv2.cpu())
    x1b, _, _ = _dst((B, C, H, W), d, dt, False)
    y2b, _, _ = _dst((B, C, H, W), d, dt, False)
    sh, st = (B, C, H, W), _st4(C * HW, H, W)
    dims = ("image", "channel", "y", "x")
    e1, sp = _stat_dests(of, d, C, g, "_p")
    e2, s2 = _stat_dests(of, d, C, g, "_2")
    exps = e1 + e2 + [(x1b, R.as_exp(x1b, 8, sh, st, of["x1"], dims=dims, kernel="x1")),
                      (y2b, R.as_exp(y2b, 8, sh, st, of["y2"], dims=dims, kernel="y2"))]
    nbp, nb2 = torch.tensor([3, 5], dtype=torch.int64).to(d), torch.tensor([7, 11], dtype=torch.int64).to(d)
    kern.cfam_mid_fwd(ps[0][8:], ms[0][8:], xs[0][8:], x1b[8:], y2b[8:], gp, bp, EPS, sp["mean"], sp["var"], sp["rmean"], sp["rvar"], MOM,
                      nbp, wv, ls, g2, b2, 1e-3, s2["mean"], s2["var"], s2["rmean"], s2["rvar"], 0.2, nb2, B, C, HW)
    _sync(d)
    assert nbp.cpu().tolist() == [4, 5] and nb2.cpu().tolist() == [8, 11]
    _check(exps, f"cfam_mid_fwd<{_tn(dt)}>", regime, d)
    # backward on the reference's statistics and the reference's x1 rounded to the storage type (operands: given)
    x1 = of["x1"].ref.float().to(dt).float()
    x1s = _src(x1.cpu(), d, dt, False)
    meanp, varp = of["mean_p"].ref.float(), of["var_p"].ref.float()
    st2 = R.stats(x1s[3].double(), (0, 2, 3))
    mean2, var2 = st2.mu.reshape(-1).float(), st2.var.reshape(-1).float()
    for tap in (True, False):
        ob = R.cfam_mid_bwd(ys[3], gxs[3] if tap else None, ps[3], ms[3], x1s[3], gp, bp, EPS, meanp, varp, wv, ls, g2, 1e-3, mean2, var2, dt)
        names = ("dgp", "dbp", "dw", "dls", "dg2", "db2")
        exps, ap, prevs = _accs(ob, d, g, regime, names)
        outs = {}
        for k in ("d_p", "d_m", "d_x0"):
            outs[k] = _dst(sh, d, dt, False)[0]
            exps.append((outs[k], R.as_exp(outs[k], 8, sh, st, ob[k], dims=dims, kernel=k)))
        kern.cfam_mid_bwd(ys[0][8:], gxs[0][8:] if tap else None, ps[0][8:], ms[0][8:], x1s[0][8:], outs["d_p"][8:], outs["d_m"][8:],
                          outs["d_x0"][8:], gp, bp, EPS, meanp, varp, wv, ls, g2, 1e-3, mean2, var2, ap["dgp"], ap["dbp"], ap["dw"],
                          ap["dls"], ap["dg2"], ap["db2"], B, C, HW)
        _sync(d)
        none = torch.zeros((1, C, 1), dtype=torch.bool)
        _exact_dbeta(ap["db2"][:C], prevs["db2"], ob["db2"], none, regime, "cfam_mid_bwd db2")
        _check(exps, f"cfam_mid_bwd<{_tn(dt)}>", regime, d)


# own_pick(B, HW, maxE): Rr = ceil(HW / 64) rows per image; the fewest waves nw in {4, 8, 16} with ceil(B / nw) Rr <= maxE elements per
# thread; instances of 2, 4, 8 (and, maxE = 16: cfam_mid, cfam_front) 16 elements
OWN_CASES = [
    (3, 4, 4),     # HW = 16, the smallest supported: need 1 -> 2 elements, 4 waves, wave 3 idle
    (5, 7, 7),     # need 2 -> 2 elements; B not a multiple of the 4 waves: the last slot is ragged
    (13, 7, 7),    # need 4 -> 4 elements
    (30, 7, 7),    # need 8 -> 8 elements, 4 waves
    (35, 7, 7),    # maxE = 8: 9 > 8 at 4 waves -> 8 waves, need 5 -> 8 elements; maxE = 16: 4 waves, 16 elements
    (70, 5, 5),    # maxE = 8: 16 waves, need 5; maxE = 16: 8 waves, need 9 -> 16 elements
    (3, 14, 14),   # Rr = 4: four pixel rows per lane, the last row 196 - 192 = 4 lanes wide; need 4
    (2, 9, 13),    # W odd: pix_ij divides by a float reciprocal of W; Rr = 2, need 2
    (5, 16, 16),   # HW = 256, an exact multiple of 64: Rr = 4, need 8
]
MID_CASES = OWN_CASES + [
    (10, 28, 28),  # Rr = 13: 16 waves, need 13 -> the 16-element instance (the model never reaches it: chanloc_supported gates at 8)
    (140, 7, 7),   # 16 waves, need 9 -> 16 elements
]
_cid = lambda c: "x".join(str(v) for v in c)  # noqa: E731


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", MID_CASES, ids=_cid)
def test_cfam_mid_bounds(dev, case, regime):
    for dt in (F32, BF):
        run_mid(dev, regime, dt, *case)


# ---- cfam_front ----------------------------------------------------------------------------------------------------------------
def front_ref(d, regime, dt, B, H, W, bn1d=True, C=3):
    """the seed is the first of eight for which the REFERENCE has no hidden unit of the gate (3 B C values) within its bound of relu's
    kink, in either storage type: chosen on the reference alone, the same for both backends"""
    for k in range(8):
        if all(not bool(_front_ref(d, regime, t, B, H, W, bn1d, C, k)["of"]["hidden_amb"].any()) for t in (F32, BF) if t != dt):
            r = _front_ref(d, regime, dt, B, H, W, bn1d, C, k)
            if not bool(r["of"]["hidden_amb"].any()):
                return r
    raise AssertionError(f"cfam_front {B, H, W} {regime}: a hidden unit of the gate lies within its bound of relu's kink for every seed")


def _front_ref(d, regime, dt, B, H, W, bn1d, C, k):
    g = _gen(6, B, H, W, k)
    x0 = _x((B, C, H, W), g, regime, (0, 0, 1))
    (g1, b1), (gd, bd) = _affine(C, g), _affine(C, g)
    g1, b1, gd, bd = g1.to(d), b1.to(d), gd.to(d), bd.to(d)
    fc1, fc2 = _w((C, 3, 3), g, 0.5).to(d), _w((C, 3), g, 0.5).to(d)
    (rm1, rv1), (rmd, rvd) = _running(C, g, d), _running(C, g, d)
    xs = _src(x0, d, dt, False)
    cots = [_src(_cot((B, C, H, W), g, regime), d, dt, False) for _ in range(3)]
    of = R.cfam_front_fwd(xs[3], g1, b1, EPS, rm1, rv1, MOM, fc1, fc2, gd if bn1d else None, bd, 1e-3, rmd, rvd, 0.2, dt)
    return dict(g=g, xs=xs, cots=cots, g1=g1, b1=b1, gd=gd if bn1d else None, bd=bd, fc1=fc1, fc2=fc2, rm1=rm1, rv1=rv1, rmd=rmd, rvd=rvd,
                of=of, C=C)


def run_front(d, regime, dt, B, H, W, bn1d=True):
    r = front_ref(d, regime, dt, B, H, W, bn1d)
    C, of, g, HW = r["C"], r["of"], r["g"], H * W
    of.update(_prev_rmean1=r["rm1"].cpu(), _prev_rvar1=r["rv1"].cpu(), _prev_rmeand=r["rmd"].cpu(), _prev_rvard=r["rvd"].cpu())
    sh, st, dims = (B, C, H, W), _st4(C * HW, H, W), ("image", "channel", "y", "x")
    y1b, xsb = _dst(sh, d, dt, False)[0], _dst(sh, d, dt, False)[0]
    exps, s1 = _stat_dests(of, d, C, g, "1")
    sd_ = dict(mean=None, var=None, rmean=None, rvar=None)
    if bn1d:
        ed, sd_ = _stat_dests(of, d, C, g, "d")
        exps += ed
    exps += [(y1b, R.as_exp(y1b, 8, sh, st, of["y1"], dims=dims, kernel="y1")), (xsb, R.as_exp(xsb, 8, sh, st, of["xs"], dims=dims, kernel="xs"))]
    small = {}
    for k, n in (("u", 3 * B * C), ("z", B * C), ("zn", B * C)):
        small[k] = torch.full((n + 8,), SENTINEL).to(d)
        exps.append((small[k], R.as_exp(small[k], 4, of[k].ref.shape, _contig(of[k].ref.shape), of[k], dims=("image", "channel", "k")[:of[k].ref.dim()],
                                        kernel=k)))
    am = torch.full((B * C + 8,), -7, dtype=torch.int32).to(d)
    nb1, nbd = torch.tensor([3, 5], dtype=torch.int64).to(d), torch.tensor([7, 11], dtype=torch.int64).to(d)
    kern.cfam_front_fwd(r["xs"][0][8:], y1b[8:], xsb[8:], r["g1"], r["b1"], EPS, s1["mean"], s1["var"], s1["rmean"], s1["rvar"], MOM, nb1,
                        r["fc1"], r["fc2"], r["gd"], r["bd"] if bn1d else None, 1e-3, sd_["mean"], sd_["var"], sd_["rmean"], sd_["rvar"],
                        0.2, nbd if bn1d else None, small["u"][4:], am[4:], small["z"][4:], small["zn"][4:], B, C, HW)
    _sync(d)
    assert nb1.cpu().tolist() == [4, 5] and nbd.cpu().tolist() == ([8, 11] if bn1d else [7, 11])
    # amax: accepted if the float64 y1 (as stored) at that index is within its bound of the plane's maximum
    assert bool((am[:4] == -7).all()) and bool((am[4 + B * C:] == -7).all()), "amax written outside [B, C]"
    idx = am[4:4 + B * C].reshape(B, C).long()
    assert bool(((idx >= 0) & (idx < HW)).all()), "amax out of the plane"
    y1s, e1s = of["y1s"].reshape(B, C, HW), of["e_y1s"].reshape(B, C, HW)
    gap = of["u"].ref[..., 0] - y1s.gather(2, idx[:, :, None])[:, :, 0]
    assert bool((gap <= e1s.gather(2, idx[:, :, None])[:, :, 0] + of["u"].extra[..., 0]).all()), "amax is not at the plane's maximum"
    _check(exps, f"cfam_front_fwd<{_tn(dt)}>", regime, d)
    # backward on the reference's saved tensors (operands: given)
    mean1, var1 = of["mean1"].ref.float(), of["var1"].ref.float()
    meand, vard = (of["meand"].ref.float(), of["vard"].ref.float()) if bn1d else (None, None)
    u, z, zn = (of[k].ref.float().contiguous() for k in ("u", "z", "zn"))
    amax = y1s.argmax(2).to(torch.int32).contiguous()
    (gxs, gy1, gtap) = r["cots"]
    for taps in (True, False):
        ob = R.cfam_front_bwd(gxs[3], gy1[3] if taps else None, gtap[3] if taps else None, r["xs"][3], r["g1"], r["b1"], EPS, mean1, var1,
                              r["fc1"], r["fc2"], r["gd"], 1e-3, meand, vard, u, amax, z, zn, dt)
        assert not bool(ob["hidden_amb"].any())
        exps, ap, prevs = _accs(ob, d, g, regime, ("dg1", "db1", "dfc1", "dfc2") + (("dgd", "dbd") if bn1d else ()))
        dxb = _dst(sh, d, dt, False)[0]
        exps.append((dxb, R.as_exp(dxb, 8, sh, st, ob["dx0"], dims=dims, kernel="dx0")))
        kern.cfam_front_bwd(gxs[0][8:], gy1[0][8:] if taps else None, gtap[0][8:] if taps else None, r["xs"][0][8:], dxb[8:], r["g1"], r["b1"],
                            EPS, mean1, var1, r["fc1"], r["fc2"], r["gd"], 1e-3, meand, vard, u, amax, z, zn, ap["dg1"], ap["db1"],
                            ap["dfc1"], ap["dfc2"], ap["dgd"] if bn1d else None, ap["dbd"] if bn1d else None, B, C, HW)
        _sync(d)
        assert bool(torch.isfinite(dxb[8:8 + B * C * HW].float()).all()), "std = 0 planes must give finite gradients"
        _check(exps, f"cfam_front_bwd<{_tn(dt)}>", regime, d)


# (B, H, W, BatchNorm1d): OWN_CASES and the two 16-element shapes; gamma_d = NULL (zn = z) on one of them.  Backward: <= 512 threads
# take the 512-thread instance (256 registers), 16 waves the 1024-thread one
FRONT_CASES = [c + (True,) for c in MID_CASES] + [(5, 7, 7, False)]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", FRONT_CASES, ids=lambda c: _cid(c[:3]) + ("" if c[3] else "-nobn1d"))
def test_cfam_front_bounds(dev, case, regime):
    for dt in (F32, BF):
        run_front(dev, regime, dt, *case)


# ---- dwbn ----------------------------------------------------------------------------------------------------------------------
def dwbn_ref(d, regime, dt, B, H, W, dils, gch, p, strided, gadd):
    nb = len(dils)
    Cb, Ct = nb * gch, nb * gch + p
    g = _gen(3, B, H, W, nb, gch, p)
    x = _x((B, Ct, H, W), g, regime, (H // 2, W // 2, dils[0]))
    ws = [_w((gch, 9), g).to(d) for _ in dils]
    gamma, beta = _affine(Cb, g)
    gamma, beta = gamma.to(d), beta.to(d)
    rm, rv = _running(Cb, g, d)
    xs = _src(x, d, dt, strided)
    gv = _src(_cot((B, Cb, H, W), g, regime), d, dt, strided)
    gr = _src(_cot((B, p, H, W), g, regime), d, dt, strided) if p else None
    ga = _src(_cot((B, Ct, H, W), g, regime), d, dt, strided) if gadd else None
    of = R.dwbn_fwd(xs[3], ws, dils, gch, p, gamma, beta, EPS, rm, rv, MOM, dt)
    mean, var = of["mean"].ref.float(), of["var"].ref.float()
    ob = R.dwbn_bwd(gv[3], gr[3] if p else None, ga[3] if gadd else None, xs[3], ws, dils, gch, p, gamma, beta, EPS, mean, var, dt)
    _amb_ok(ob["amb"], f"dwbn {B, H, W, dils, gch, p} {regime}")
    return dict(g=g, xs=xs, gv=gv, gr=gr, ga=ga, ws=ws, gamma=gamma, beta=beta, rm=rm, rv=rv, of=of, ob=ob, mean=mean, var=var)


def run_dwbn(d, regime, dt, B, H, W, dils, gch, p, strided=False, gadd=False):
    nb = len(dils)
    Cb, Ct, HW = nb * gch, nb * gch + p, H * W
    r = dwbn_ref(d, regime, dt, B, H, W, dils, gch, p, strided, gadd)
    of, ob, g, ws = r["of"], r["ob"], r["g"], r["ws"]
    xb, xo, sxb, xv = r["xs"]
    of.update(_prev_rmean=r["rm"].cpu(), _prev_rvar=r["rv"].cpu())
    dims = ("image", "channel", "y", "x")
    vb, vo, svb = _dst((B, Cb, H, W), d, dt, strided)
    exps, sp = _stat_dests(of, d, Cb, g)
    exps.append((vb, R.as_exp(vb, vo, (B, Cb, H, W), _st4(svb, H, W), of["v"], dims=dims, kernel="v")))
    rb, ro, srb = _dst((B, max(p, 1), H, W), d, dt, strided)
    if p:
        exps.append((rb, R.as_exp(rb, ro, (B, p, H, W), _st4(srb, H, W), R.Out(of["rest"], of["rest"].abs(), 1), dims=dims, kernel="rest")))
    nbt = torch.tensor([3, 5, 7, 11][:nb + 1], dtype=torch.int64).to(d)
    wp, dl = kern._ptr_arr([w.data_ptr() for w in ws]), (kern.C.c_int * nb)(*dils)
    if strided:
        kern._call("cenet_dwbn_fwd_f32", kern.Ptr(xb, xo), sxb, wp, dl, nb, gch, p, kern.Ptr(vb, vo), svb, kern.Ptr(rb, ro) if p else None,
                   srb, r["gamma"], r["beta"], EPS, sp["mean"], sp["var"], sp["rmean"], sp["rvar"], MOM, nbt, B, H, W)
    else:
        kern.dwbn_fwd(xb[xo:], ws, dils, gch, p, vb[vo:], rb[ro:] if p else None, r["gamma"], r["beta"], EPS, sp["mean"], sp["var"],
                      sp["rmean"], sp["rvar"], MOM, nbt, B, H, W)
    _sync(d)
    assert nbt.cpu().tolist() == [v + (i < nb) for i, v in enumerate([3, 5, 7, 11][:nb + 1])], nbt  # one counter per branch
    if p:  # a copy is exact
        assert torch.equal(R.view(rb, ro, (B, p, H, W), _st4(srb, H, W)).double(), of["rest"])
    _check(exps, f"dwbn_fwd<{_tn(dt)}>", regime, d)
    dxb, do, sdb = _dst((B, Ct, H, W), d, dt, strided)
    obf = dict(ob, **{f"dw{j}": o for j, o in enumerate(ob["dw"])})
    exps, ap, prevs = _accs(obf, d, g, regime, tuple(f"dw{j}" for j in range(nb)) + ("dgamma", "dbeta"))
    exps.append((dxb, R.as_exp(dxb, do, (B, Ct, H, W), _st4(sdb, H, W), ob["dx"], dims=dims, kernel="dx")))
    gvb, gvo, sgb, _ = r["gv"]
    if strided or gadd:
        dwp = kern._ptr_arr([ap[f"dw{j}"].data_ptr() for j in range(nb)])
        kern._call("cenet_dwbn_bwd_acc_f32", kern.Ptr(gvb, gvo), sgb, kern.Ptr(r["gr"][0], r["gr"][1]) if p else None,
                   r["gr"][2] if p else 0, kern.Ptr(r["ga"][0], r["ga"][1]) if gadd else None, r["ga"][2] if gadd else 0,
                   kern.Ptr(xb, xo), sxb, wp, dl, nb, gch, p, r["gamma"], r["beta"], EPS, r["mean"], r["var"], kern.Ptr(dxb, do), sdb, dwp,
                   ap["dgamma"], ap["dbeta"], B, H, W)
    else:
        kern.dwbn_bwd(gvb[gvo:], r["gr"][0][r["gr"][1]:] if p else None, xb[xo:], ws, dils, gch, p, r["gamma"], r["beta"], EPS, r["mean"],
                      r["var"], dxb[do:], [ap[f"dw{j}"] for j in range(nb)], ap["dgamma"], ap["dbeta"], B, H, W)
    _sync(d)
    _exact_dbeta(ap["dbeta"][:Cb], prevs["dbeta"], ob["dbeta"], ob["amb"], regime, "dwbn_bwd")
    _check(exps, f"dwbn_bwd<{_tn(dt)}>", regime, d)


# (B, H, W, dilations, channels per branch g, pooled channels p, batch strides, g_add): the own-elements classes at maxE = 8, with
# nb = 1, 2, 3, mixed dilations, g = 1 and 2, p = 0 and > 0, g_add / g_rest present and NULL spread over them
DWBN_CASES = [
    (3, 4, 4, (1, 2, 3), 1, 1, False, False),    # 2 elements, wave 3 idle; dilation 3 on 4x4: only the centre tap lands inside
    (5, 7, 7, (1, 2, 3), 2, 2, True, True),      # 2 elements, ragged slot; slices of wider tensors; g_add
    (13, 7, 7, (2,), 2, 0, False, False),        # 4 elements; nb = 1, p = 0: rest / g_rest NULL
    (30, 7, 7, (1, 3), 1, 1, False, True),       # 8 elements, 4 waves; nb = 2
    (35, 7, 7, (3, 1), 1, 0, False, True),       # 8 waves; p = 0 with g_add
    (70, 5, 5, (1, 2), 1, 1, True, False),       # 16 waves
    (3, 14, 14, (1, 2, 3), 1, 2, False, False),  # four rows per lane, the last 4 lanes wide
    (2, 9, 13, (2, 1), 2, 1, True, True),        # W odd: pix_ij
    (5, 16, 16, (3,), 1, 1, False, False),       # HW a multiple of 64; 8 elements
]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", DWBN_CASES, ids=lambda c: _cid(c[:3]) + "-d" + "".join(map(str, c[3])) + f"-g{c[4]}p{c[5]}" +
                         ("-slice" if c[6] else "") + ("-add" if c[7] else ""))
def test_dwbn_bounds(dev, case, regime):
    for dt in (F32, BF):
        run_dwbn(dev, regime, dt, *case)


# ---- dwact ---------------------------------------------------------------------------------------------------------------------
def dwact_ref(d, regime, dt, B, H, W, dil, act, has_bias, C=2):
    g = _gen(4, B, H, W, dil, len(act))
    x = _x((B, C, H, W), g, regime, (0, 0, 1))
    w = _w((C, 9), g).to(d)
    bias = (0.3 + _w((C,), g, 0.2)).to(d) if has_bias else None
    xs = _src(x, d, dt, False)
    gs = _src(_cot((B, C, H, W), g, regime), d, dt, False)
    of = R.dwact_fwd(xs[3], w, bias, act, SLOPE, dil, dt)
    ob = R.dwact_bwd(gs[3], xs[3], w, bias, act, SLOPE, dil, dt)
    _amb_ok(ob["amb"], f"dwact {B, H, W, dil, act} {regime}")
    return dict(g=g, xs=xs, gs=gs, w=w, bias=bias, of=of, ob=ob, C=C)


def run_dwact(d, regime, dt, B, H, W, dil, act, has_bias):
    r = dwact_ref(d, regime, dt, B, H, W, dil, act, has_bias)
    C, of, ob, g = r["C"], r["of"], r["ob"], r["g"]
    sh, st, dims = (B, C, H, W), _st4(C * H * W, H, W), ("image", "channel", "y", "x")
    yb = _dst(sh, d, dt, False)[0]
    exps = [(yb, R.as_exp(yb, 8, sh, st, of["y"], dims=dims, kernel="y"))]
    kern.dwact_fwd(r["xs"][0][8:], r["w"], r["bias"], yb[8:], act, SLOPE, dil, B, C, H, W)
    _sync(d)
    _check(exps, f"dwact_fwd<{_tn(dt)}, {act}>", regime, d)
    dxb = _dst(sh, d, dt, False)[0]
    exps, ap, prevs = _accs(ob, d, g, regime, ("dw", "db") if has_bias else ("dw",))
    exps.append((dxb, R.as_exp(dxb, 8, sh, st, ob["dx"], dims=dims, kernel="dx")))
    kern.dwact_bwd(r["gs"][0][8:], r["xs"][0][8:], r["w"], r["bias"], dxb[8:], ap["dw"], ap["db"] if has_bias else None, act, SLOPE, dil,
                   B, C, H, W)
    _sync(d)
    _check(exps, f"dwact_bwd<{_tn(dt)}, {act}>", regime, d)


# (B, H, W, dil, act, bias): dwact_bordered: dil == 1 and B (H + 2)(W + 2) <= 8192 -> the zero-bordered LDS layout
DWACT_CASES = [
    (3, 4, 4, 1, "gelu", True),      # bordered; 2 elements, wave 3 idle
    (3, 4, 4, 3, "relu", True),      # dilation 3 on 4x4: only the centre tap lands inside (bias NULL goes with GELU: without a bias
                                     # the zeroed pixels of the outlier regimes put relu's kink exactly on the pre-activation)
    (5, 7, 7, 1, "lrelu", True),     # bordered; ragged slot
    (13, 7, 7, 2, "gelu", False),    # 4 elements; dilation 2; bias NULL
    (30, 7, 7, 1, "gelu", True),     # bordered: 30 x 81 = 2430; 8 elements, 4 waves
    (35, 7, 7, 3, "gelu", True),     # 8 waves; dilation 3
    (70, 5, 5, 1, "relu", True),     # bordered: 70 x 49; 16 waves
    (128, 7, 7, 1, "gelu", True),    # dil = 1 where the bordered batch does NOT fit: 128 x 81 = 10368 > 8192; 16 waves, 8 elements
    (3, 14, 14, 1, "gelu", False),   # bordered; four rows per lane
    (2, 9, 13, 2, "lrelu", True),    # W odd: pix_ij on the unbordered layout
    (5, 16, 16, 1, "gelu", True),    # bordered: 5 x 324; HW a multiple of 64
]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", DWACT_CASES, ids=lambda c: _cid(c[:3]) + f"-d{c[3]}-{c[4]}" + ("" if c[5] else "-nobias"))
def test_dwact_bounds(dev, case, regime):
    for dt in (F32, BF):
        run_dwact(dev, regime, dt, *case)


# ---- pool_branch ---------------------------------------------------------------------------------------------------------------
def pool_ref(d, regime, dt, B, P, H, W, strided):
    g = _gen(5, B, P, H, W)
    x = _x((B, P, H, W), g, regime, (0, 0, 1))
    wc = _w((P, P), g, 0.5)
    if regime == "constant" and P > 1:  # channel 1 of t constant: it takes channel 1 of x alone
        wc[1] = 0.0
        wc[1, 1] = 1.0
    wc = wc.to(d)
    gamma, beta = _affine(P, g)
    gamma, beta = gamma.to(d), beta.to(d)
    rm, rv = _running(P, g, d)
    xs = _src(x, d, dt, strided)
    gs = _src(_cot((B, P, H, W), g, regime), d, dt, strided)
    of = R.pool_fwd(xs[3], wc, gamma, beta, EPS, SLOPE, rm, rv, MOM)
    mean, var = of["mean"].ref.float(), of["var"].ref.float()
    pooled, t = of["pooled"].ref.float(), of["t"].ref.float()  # operands of the backward: given
    ob = R.pool_bwd(gs[3], wc, gamma, beta, EPS, SLOPE, pooled, t, mean, var, H, W)
    _amb_ok(ob["amb"], f"pool {B, P, H, W} {regime}")
    return dict(g=g, xs=xs, gs=gs, wc=wc, gamma=gamma, beta=beta, rm=rm, rv=rv, of=of, ob=ob, mean=mean, var=var, pooled=pooled, t=t)


def run_pool(d, regime, dt, B, P, H, W, strided=False):
    r = pool_ref(d, regime, dt, B, P, H, W, strided)
    of, ob, g = r["of"], r["ob"], r["g"]
    xb, xo, sxb, _ = r["xs"]
    of.update(_prev_rmean=r["rm"].cpu(), _prev_rvar=r["rv"].cpu())
    RH, RW = DF._pool_matrices(H, W, d)  # as ops.pool_branch builds them: an error in the host-built maps fails too
    dims = ("image", "channel", "y", "x")
    yb, yo, syb = _dst((B, P, H, W), d, dt, strided)
    exps, sp = _stat_dests(of, d, P, g)
    exps.append((yb, R.as_exp(yb, yo, (B, P, H, W), _st4(syb, H, W), of["y"], dims=dims, kernel="y")))
    pb, tb = (torch.full((B * P * 49 + 8,), SENTINEL).to(d) for _ in range(2))
    for buf, k in ((pb, "pooled"), (tb, "t")):
        exps.append((buf, R.as_exp(buf, 4, (B, P, 49), (P * 49, 49, 1), of[k], dims=("image", "channel", "bin"), kernel=k)))
    nbt = torch.tensor([3, 5], dtype=torch.int64).to(d)
    kern.pool_branch_fwd(kern.Ptr(xb, xo), sxb, r["wc"], r["gamma"], r["beta"], EPS, SLOPE, RH, RW, kern.Ptr(yb, yo), syb, pb[4:], tb[4:],
                         sp["mean"], sp["var"], sp["rmean"], sp["rvar"], MOM, nbt, B, P, H, W)
    _sync(d)
    assert nbt.cpu().tolist() == [4, 5]
    _check(exps, f"pool_branch_fwd<{_tn(dt)}>", regime, d)
    gb, go, sgb, _ = r["gs"]
    dxb, do, sdb = _dst((B, P, H, W), d, dt, strided)
    exps, ap, prevs = _accs(ob, d, g, regime, ("dwc", "dgamma", "dbeta"))
    exps.append((dxb, R.as_exp(dxb, do, (B, P, H, W), _st4(sdb, H, W), ob["dx"], dims=dims, kernel="dx")))
    ws = torch.full((B * P * 49 + 8,), NAN).to(d)
    ws[B * P * 49:] = SENTINEL
    kern.pool_branch_bwd(kern.Ptr(gb, go), sgb, r["wc"], r["gamma"], r["beta"], EPS, SLOPE, RH, RW, r["pooled"].contiguous(),
                         r["t"].contiguous(), r["mean"], r["var"], ws, kern.Ptr(dxb, do), sdb, ap["dwc"], ap["dgamma"], ap["dbeta"],
                         B, P, H, W)
    _sync(d)
    assert bool((ws[B * P * 49:] == SENTINEL).all()), "the workspace was written beyond [B, P, 49]"
    _check(exps, f"pool_branch_bwd<{_tn(dt)}>", regime, d)


# (B, P, H, W, batch strides): windows repeated below 7, exact at 7, overlapping above, non-square, and the limits of pool_ok
POOL_CASES = [
    (1, 5, 4, 4, False),     # B = 1: 49 values per channel; every window a repeated pixel
    (3, 1, 10, 10, True),    # P = 1; overlapping windows; a channel slice
    (64, 2, 7, 7, False),    # B at its limit; windows of exactly one pixel; 49 == H: the second resampling is the identity
    (3, 32, 9, 20, True),    # P at its limit; non-square
    (2, 5, 64, 64, False),   # H, W at their limit
]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: _cid(c[:4]) + ("-slice" if c[4] else ""))
def test_pool_branch_bounds(dev, case, regime):
    for dt in (F32, BF):
        run_pool(dev, regime, dt, *case)


# ---- the ambiguity cap, on the reference alone ----------------------------------------------------------------------------------
def test_ambiguity_cap_on_the_reference():
    """every case and regime: at most 1 % of the elements ambiguous for relu / lrelu (the *_ref builders assert it); no kernel runs"""
    d = torch.device("cpu")
    for regime in REGIMES:
        for dt in (F32, BF):
            for c in EUCB_CASES:
                if c[0] * c[1] * c[2] <= 4000:  # (the large ones are asserted when their case runs; the seeds are the same)
                    eucb_ref(d, regime, dt, *c)
            for c in DWBN_CASES:
                dwbn_ref(d, regime, dt, *c)
            for c in DWACT_CASES:
                dwact_ref(d, regime, dt, *c)
            for c in POOL_CASES:
                if c[0] * c[1] * c[2] * c[3] <= 20000:
                    pool_ref(d, regime, dt, *c)
            for c in FRONT_CASES:  # (none of the 3 B C hidden units of the gate may be ambiguous)
                front_ref(d, regime, dt, *c)


# ---- the constants ---------------------------------------------------------------------------------------------------------------
def test_chanloc_constants_are_the_host_measurement():
    got = R.measure_constants()
    want = (R.MEASURED_GELU, R.MEASURED_DGELU, R.MEASURED_SIGM, R.MEASURED_MAP)
    for a, b in zip(got, want):
        assert abs(a - b) <= 2e-3 * b, (got, want)
    for c, m in zip((R.C_GELU, R.C_DGELU, R.C_SIGM, R.C_MAP), want):
        assert 4 * m <= c <= 4 * m * 1.02, (c, m)  # x 4, rounded up, not widened


# ---- self-test of the rule: wrong references must be rejected ------------------------------------------------------------------
def _rejected(got64, out, dt, what):
    """`got64`: a deliberately wrong evaluation standing in for the kernel's output, rounded to the storage type"""
    buf = torch.full((got64.numel() + 16,), SENTINEL).to(dt)
    exp = R.as_exp(buf, 8, got64.shape, _contig(got64.shape), out, kernel=what)
    buf[8:8 + got64.numel()] = got64.reshape(-1).float().to(dt)
    with pytest.raises(AssertionError):
        R.assert_bound(buf, exp, what)
    ok = buf.clone()
    ok[8:8 + got64.numel()] = out.ref.reshape(-1).float().to(dt)
    R.assert_bound(ok, exp, what)  # (and the reference itself, rounded once, passes)


@pytest.mark.parametrize("regime", ("normal", "offset"))
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_wrong_references_are_rejected(regime, dt):
    d = torch.device("cpu")
    g = _gen(9)
    B, C, H, W = 3, 2, 6, 7
    x = _x((B, C, H, W), g, regime, None)
    w, (gamma, beta) = _w((C, 9), g), _affine(C, g)
    rm, rv = _running(C, g, d)

    # a border tap dropped: the conv of eucb with the tap (0, 0) left out on output row 0
    o = R.eucb_fwd(x, w, gamma, beta, EPS, SLOPE, rm, rv, MOM)
    xu = R.up2(x.double())
    u = R.conv_dw(xu, w)[0]
    bad = u.clone()
    bad[:, :, 0, 1:] -= w[None, :, 3, None].double() * xu[:, :, 0, :-1]
    st = R.chan_stats(u, 0.0)
    y_of = lambda v: R._act64(R.bn_apply(v, 0.0, st, gamma, beta, EPS)[0], "lrelu", SLOPE)  # noqa: E731
    _rejected(y_of(bad), o["y"], dt, "border tap dropped")
    # the nearest-x2 quad shifted by one source pixel
    xs = torch.roll(x, 1, -1)
    _rejected(R.eucb_fwd(xs, w, gamma, beta, EPS, SLOPE)["y"].ref, o["y"], dt, "quad shifted")
    # a dilation off by one
    o2 = R.dwbn_fwd(x, [w[:1], w[1:]], (2, 1), 1, 0, gamma, beta, EPS, rm, rv, MOM, dt)
    _rejected(R.dwbn_fwd(x, [w[:1], w[1:]], (3, 1), 1, 0, gamma, beta, EPS, rm, rv, MOM, dt)["v"].ref, o2["v"], dt, "dilation off by one")
    # unbiased in place of biased batch variance
    n = B * 4 * H * W
    _rejected(o["var"].ref * n / (n - 1), o["var"], F32, "unbiased variance")
    # the last image left out of the statistics
    _rejected(R.chan_stats(u[:-1], 0.0).outs["mean"].ref, o["mean"], F32, "last image left out")
    _rejected(R.chan_stats(u[:-1], 0.0).outs["var"].ref, o["var"], F32, "last image left out (var)")
    # momentum applied the wrong way round
    _rejected(MOM * rm.double() + (1 - MOM) * o["mean"].ref, o["rmean"], F32, "momentum the wrong way round")
    # a pooling window one row short
    P, Hp, Wp = 2, 10, 9
    xp = _x((B, P, Hp, Wp), g, regime, None)
    wc = _w((P, P), g, 0.5)
    op = R.pool_fwd(xp, wc, gamma, beta, EPS, SLOPE, rm, rv, MOM)
    short = op["pooled"].ref.clone().reshape(B, P, 7, 7)
    for oy in range(7):
        ys, ye = (oy * Hp) // 7, -(-(oy + 1) * Hp // 7)
        if ye - ys > 1:
            for ox in range(7):
                xs_, xe = (ox * Wp) // 7, -(-(ox + 1) * Wp // 7)
                short[:, :, oy, ox] = xp[:, :, ys:ye - 1, xs_:xe].double().mean((2, 3))
    _rejected(short.reshape(B, P, 49), op["pooled"], F32, "pooling window one row short")
