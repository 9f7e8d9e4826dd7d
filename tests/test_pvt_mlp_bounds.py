"""The fused PVT MLP kernels (pvt_mlp.hip: one forward kernel, two backward kernels and a fold) held per element, stage by stage, to
the float64 reference of tests/pvt_mlp_ref.py, on every tile path the launch code can take.

* The reference is the header's meaning of cenet_pvt_mlp_fwd_bf16 / cenet_pvt_mlp_bwd_bf16 in float64 (pvt_mlp_ref), NOT the chain of
  the project's own launches (tests/test_pvt_mlp.py compares those two: both are code under test and share gelu_as, the fragment
  layouts, the bf16 pack and the LayerNorm arithmetic).  Each stage is checked against the reference applied to the kernel's own
  stored output of the stage before it, so a failure names the stage, the tensor and the element.
* CASES: the smallest shapes at which each path of the launch code exists; the path of every row is ASSERTED through
  cenet_pvt_mlp_bwd_plan (tile rows of the forward / second backward kernel, tile rows of the first backward kernel K1, tiles per K1
  run, K1 runs per image), so retuning the launch code cannot un-cover a path silently.  The two large rows reach K1's tile loop
  (prefetch of the next tile into the other LDS buffer, both buffers reused, accumulators carried across tiles, a short last run);
  they are fed to the backward entry point only, with random bf16 h and float64 LayerNorm statistics.
* input classes (each on the 2 x 2-tile row and on both 28 x 14 rows): plain (DropPath scale None / first and last sample 0, the rest
  1.25 / -- where that leaves no live sample, B <= 2 -- also (0, 1.25)); LayerNorm edges (constant rows: var = 0; rows with a common
  offset 50 x their spread; a zero in ln_g); GELU range (wd scaled so that the float64 pre-activation spans both tails, |u| <= U_RANGE
  asserted on the reference; hidden channels that are exactly 0, one of them with bd = 0); zero sample (a sample of g all zero, a
  sample with s_b = 0: its a_out and gu are exactly 0).
* contract: outputs pre-filled with NaN come back finite; guard rows around every output buffer are untouched (bitwise); dwd, dbd,
  dln_g, dln_b, db2 are ADDED onto non-zero previous values; db2 = None and no up_scale / dxs leave gu / dh / dx bit-equal; the
  inference form gives a bit-equal y; two runs give bit-equal results (the atomically accumulated sums: only their bound); dxs is
  exactly bf16(up_scale_b * float(dx as stored)); the entry points refuse what the header says they refuse.
* the bound must bite (no kernel): the reference's own values with 1 % of the elements moved by two bf16 ulps (fp32 sums: by 4 x
  their bound) are rejected.
`sim` = the kernel sources on the host SIMT checker (CPU); `hip` = the gfx950 library (marker gpu)."""
import math

import pytest
import torch

import pvt_mlp_ref as R
from backend import dev  # noqa: F401
from cenet_amd import kern

BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-6
NAN, SENTINEL = float("nan"), 12288.0  # (the sentinel is exact in bf16)

# (C, HD, H, W, B) -> (tile rows, K1 tile rows, K1 tiles per run, K1 runs per image), and what the row reaches
CASES = {
    "one_tile": ((64, 64, 7, 14, 1), (7, 7, 1, 1)),            # one tile, one slab: no weight prefetch, no halo neighbour
    "odd_slabs": ((128, 192, 8, 14, 2), (8, 8, 1, 1)),         # 8-row tile, 3 slabs (buffer parity), image border between batch entries
    "tiles2x2": ((64, 128, 16, 28, 2), (8, 8, 1, 4)),          # 2 x 2 tiles: every halo side comes from a neighbouring tile
    "rows7": ((128, 128, 14, 28, 2), (7, 7, 1, 4)),            # 7-row tiles in both backward kernels (H % 4 != 0)
    "k1rows4_c64": ((64, 128, 28, 14, 2), (7, 4, 1, 7)),       # K1 on the 4-row instance while K2 keeps 7 rows
    "k1rows4_c128": ((128, 128, 28, 14, 2), (7, 4, 1, 7)),
    "run4_short": ((128, 1024, 28, 14, 22), (7, 4, 4, 2)),     # backward only: 4-row instance, runs of 4 and 3 tiles
    "run2_short": ((64, 2048, 24, 14, 12), (8, 8, 2, 2)),      # backward only: 8-row tiles, runs of 2 and 1 tiles
}
SMALL = ("one_tile", "odd_slabs", "tiles2x2", "rows7", "k1rows4_c64", "k1rows4_c128")
LARGE = ("run4_short", "run2_short")
CLASS_ROWS = ("tiles2x2", "k1rows4_c64", "k1rows4_c128")
CLASSES = ("lnedge", "gelu", "zero")


def _sync(d):
    if d.type == "cuda":
        torch.cuda.synchronize()


def _gen(name, salt=0):
    s = 17 + salt
    for ch in name:
        s = (s * 1000003 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _scales(B, mode):
    """the DropPath scale of a run: None; "ends0": first and last sample 0, the rest 1.25; "mixed": (0, 1.25, 1.25, ...);
    "last0": (1.25, ..., 0)"""
    if mode is None:
        return None
    s = torch.full((B,), 1.25)
    if mode == "ends0":
        s[0] = s[-1] = 0.0
    elif mode == "mixed":
        s[0] = 0.0 if B > 1 else 1.25
    elif mode == "last0":
        s[-1] = 0.0
    return s


def _modes(B):
    """plain class: None, the rule of the case matrix, and where that rule leaves no live sample also a mixed one"""
    return (None, "ends0") + (("mixed",) if B <= 2 else ())


def plan_of(name):
    (C, HD, H, W, B), want = CASES[name]
    got = kern.pvt_mlp_bwd_plan(B, H, W, C, HD)
    assert got == want, f"{name}: cenet_pvt_mlp_bwd_plan gives (tile rows, K1 tile rows, K1 tiles per run, K1 runs) = {got}, the " \
                        f"case was chosen for {want}: the launch code changed, re-derive the case matrix"
    return got


# ---- data ----------------------------------------------------------------------------------------------------------------------
def make(name, cls, mode):
    """operands of a case on the host: bf16 x, g; fp32 parameters (w1 / w2 bf16-exact); the float64 chain's h, mean, rstd for the
    backward entry point"""
    (C, HD, H, W, B), _ = CASES[name]
    g = _gen(name + cls)
    N = H * W
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc  # noqa: E731
    x = (0.3 + 1.5 * r(B, N, C)).to(BF)
    p = dict(ln_g=1.0 + 0.2 * r(C), ln_b=0.1 * r(C), w1=r(HD, C, sc=C ** -0.5).to(BF), b1=0.1 * r(HD), wd=r(HD, 9, sc=0.4), bd=0.1 * r(HD),
             w2=r(C, HD, sc=HD ** -0.5).to(BF), b2=0.1 * r(C))
    gy = r(B, N, C).to(BF)
    if cls == "lnedge":
        x[:, 3::11] = 1.75                                                      # constant rows: var = 0, rstd = eps^-1/2
        x[:, 5::13] = (50.0 + r(B, len(range(5, N, 13)), C)).to(BF)               # a common offset 50 x the spread
        p["ln_g"][C // 2] = 0.0
    if cls == "gelu":
        p["w1"][5::16] = 0.0                                                    # hidden channels that are exactly 0: u = bd there
        p["b1"][5::16] = 0.0
        p["bd"][5] = 0.0
    if cls == "zero":
        gy[0] = 0.0
        mode = "last0"
    if name in LARGE:                                                           # random bf16 h, float64 statistics: no forward is paid for
        h = (0.8 * r(B, N, HD)).to(BF)
    else:
        xd = x.double()
        xn = torch.nn.functional.layer_norm(xd, (C,), p["ln_g"].double(), p["ln_b"].double(), EPS).float().to(BF)
        h = (xn.double() @ p["w1"].double().t() + p["b1"].double()).float().to(BF)
    if cls == "gelu":                                                           # both tails: max |DW3x3(h)| = 20, |bd| stays ~0.1
        u0 = R.preact(h, p["wd"], torch.zeros(HD), B, H, W)[0]
        p["wd"] = (p["wd"].double() * (20.0 / float(u0.abs().max()))).float()
    xd = x.double()
    mean = xd.mean(-1).reshape(-1)
    rstd = (xd.var(-1, unbiased=False).reshape(-1) + EPS) ** -0.5
    return dict(C=C, HD=HD, H=H, W=W, B=B, x=x, g=gy, p=p, h=h, mean=mean.float(), rstd=rstd.float(), bscale=_scales(B, mode),
                up=0.5 + torch.rand(B, generator=g))


def _range_ok(u, cls):
    assert float(u.abs().max()) <= R.U_RANGE, f"|u| reaches {float(u.abs().max())}: outside the range the GELU constants were measured over"
    if cls == "gelu":
        assert float(u.max()) > 12.0 and float(u.min()) < -12.0, (float(u.min()), float(u.max()))


# ---- destinations with guard rows ------------------------------------------------------------------------------------------------
def _lead(shape):
    return max(2 * shape[-1], 8)  # two rows, at least 16 bytes


def _dest(shape, dt, d, prev=None):
    """an output [.., width] between two guard rows of SENTINEL, NaN (or `prev`) inside -> (buffer, lead, the view the kernel gets)"""
    n, lead = math.prod(shape), _lead(shape)
    buf = torch.full((lead + n + lead,), SENTINEL, dtype=F32)
    buf[lead:lead + n] = NAN if prev is None else prev.reshape(-1)
    buf = buf.to(dt).to(d)
    return buf, lead, buf[lead:lead + n].view(shape)


def _contig(shape):
    st, s = [], 1
    for n in reversed(shape):
        st.append(s)
        s *= n
    return tuple(reversed(st))


class Dests:
    """the outputs of one launch: NaN-filled (accumulators: previous values) between guard rows, checked against Outs"""

    def __init__(self, d):
        self.d, self.items = d, {}

    def new(self, name, shape, dt, prev=None):
        buf, lead, v = _dest(tuple(shape), dt, self.d, prev)
        self.items[name] = (buf, buf.clone(), lead, tuple(shape), prev is not None)
        return v

    def view(self, name):
        buf, _, lead, shape, _ = self.items[name]
        return buf[lead:lead + math.prod(shape)].view(shape)

    def check(self, name, o, what, dims):
        """assert_bound of the buffer (guard rows bitwise unchanged, every own element finite and within its bound)"""
        buf, before, lead, shape, add = self.items[name]
        exp = R.as_exp(before, lead, shape, _contig(shape), o, add=add, dims=dims, kernel=name)
        worst = R.assert_bound(buf, exp, what)
        print(f"BOUND {what} {name}: worst |err| / bound = {worst:.3f}")
        return worst

    def untouched(self, name, what):
        buf, before, *_ = self.items[name]
        assert torch.equal(buf.view(torch.int16 if buf.element_size() == 2 else torch.int32),
                           before.view(torch.int16 if buf.element_size() == 2 else torch.int32)), f"{what}: {name} was written"


TOK = ("image", "token", "channel")


def _to(d, *ts):
    return [None if t is None else t.to(d) for t in ts]


# ---- forward -------------------------------------------------------------------------------------------------------------------
def launch_fwd(m, d, saved=True):
    C, HD, H, W, B, p = m["C"], m["HD"], m["H"], m["W"], m["B"], m["p"]
    N = H * W
    D = Dests(d)
    y = D.new("y", (B, N, C), BF)
    sv = None
    if saved:
        sv = (D.new("xn", (B, N, C), BF), D.new("mean", (B * N,), F32), D.new("rstd", (B * N,), F32), D.new("h", (B, N, HD), BF),
              D.new("a", (B, N, HD), BF))
    x, ln_g, ln_b, w1, b1, wd, bd, w2, b2, bs = _to(d, m["x"], p["ln_g"], p["ln_b"], p["w1"], p["b1"], p["wd"], p["bd"], p["w2"], p["b2"],
                                                    m["bscale"])
    kern.pvt_mlp_fwd(x, ln_g, ln_b, EPS, w1, b1, wd, bd, w2, b2, bs, y, B, H, W, C, HD, sv)
    _sync(d)
    return D


def check_fwd(m, D, cls, what):
    C, HD, H, W, B, p, d = m["C"], m["HD"], m["H"], m["W"], m["B"], m["p"], D.d
    got = {k: D.view(k) for k in ("xn", "h", "a")}
    ops = _to(d, m["x"], p["ln_g"], p["ln_b"])
    w1, b1, wd, bd, w2, b2, bs = _to(d, p["w1"], p["b1"], p["wd"], p["bd"], p["w2"], p["b2"], m["bscale"])
    o = R.fwd(ops[0], ops[1], ops[2], EPS, w1, b1, wd, bd, w2, b2, bs, got, B, H, W)
    _range_ok(o["u"], cls)
    N = H * W
    xn = o["xn"]
    D.check("xn", R.Out(xn.ref.reshape(B, N, C), xn.mag.reshape(B, N, C), xn.K, xn.extra.reshape(B, N, C)), what, TOK)
    D.check("mean", o["mean"], what, ("row",))
    D.check("rstd", o["rstd"], what, ("row",))
    for k in ("h", "a", "y"):
        D.check(k, o[k], what, TOK)
    ex = o["y_exact_rows"]
    if bool(ex.any()):  # s_b = 0: y is x bit for bit, the saved a exactly 0
        assert torch.equal(D.view("y")[ex], ops[0][ex]), f"{what}: y of a sample with s_b = 0 is not x bit for bit"
        assert bool((D.view("a")[ex] == 0).all()), f"{what}: a_out of a sample with s_b = 0 is not 0"


def run_fwd(d, name, cls, mode):
    m = make(name, cls, mode)
    what = f"pvt_mlp_fwd {name} [{cls}, bscale {mode}]"
    D = launch_fwd(m, d)
    check_fwd(m, D, cls, what)
    D2 = launch_fwd(m, d)                                                       # a second run: bit-equal
    for k in ("y", "xn", "mean", "rstd", "h", "a"):
        assert torch.equal(D.items[k][0].view(torch.uint8), D2.items[k][0].view(torch.uint8)), f"{what}: {k} differs between two runs"
    D3 = launch_fwd(m, d, saved=False)                                          # the inference form: nothing saved, the same y
    assert torch.equal(D.items["y"][0].view(torch.uint8), D3.items["y"][0].view(torch.uint8)), f"{what}: the inference form's y differs"


# ---- backward ------------------------------------------------------------------------------------------------------------------
SUMS = ("dwd", "dbd", "dln_g", "dln_b", "db2")


def launch_bwd(m, d, full=True):
    """full: with db2 and up_scale / dxs; else without either"""
    C, HD, H, W, B, p = m["C"], m["HD"], m["H"], m["W"], m["B"], m["p"]
    N = H * W
    D = Dests(d)
    gu, dh, dx = D.new("gu", (B, N, HD), BF), D.new("dh", (B, N, HD), BF), D.new("dx", (B, N, C), BF)
    gp = _gen("prev")
    prev = lambda *s: 0.75 + 0.5 * torch.rand(*s, generator=gp)  # noqa: E731
    dwd, dbd, dg, db = D.new("dwd", (HD, 9), F32, prev(HD, 9)), D.new("dbd", (HD,), F32, prev(HD)), D.new("dln_g", (C,), F32, prev(C)), \
        D.new("dln_b", (C,), F32, prev(C))
    db2 = D.new("db2", (C,), F32, prev(C))
    dxs = D.new("dxs", (B, N, C), BF)
    g, bs, w1, w2, wd, bd, h, x, ln_g, mean, rstd, up = _to(d, m["g"], m["bscale"], p["w1"], p["w2"], p["wd"], p["bd"], m["h"], m["x"], p["ln_g"],
                                                            m["mean"], m["rstd"], m["up"])
    kern.pvt_mlp_bwd(g, bs, w1, w2, wd, bd, h, x, ln_g, mean, rstd, gu, dh, dx, dwd, dbd, dg, db, db2 if full else None, B, H, W, C, HD,
                     up_scale=up if full else None, dxs=dxs if full else None)
    _sync(d)
    return D


def check_bwd(m, D, cls, what, full=True):
    H, W, B, p, d = m["H"], m["W"], m["B"], m["p"], D.d
    g, bs, w1, w2, wd, bd, h, x, ln_g, mean, rstd, up = _to(d, m["g"], m["bscale"], p["w1"], p["w2"], p["wd"], p["bd"], m["h"], m["x"], p["ln_g"],
                                                            m["mean"], m["rstd"], m["up"])
    o = R.bwd(g, bs, w1, w2, wd, bd, h, x, ln_g, mean, rstd, dict(gu=D.view("gu"), dh=D.view("dh")), B, H, W)
    _range_ok(o["u"], cls)
    for k in ("gu", "dh", "dx"):
        D.check(k, o[k], what, TOK)
    D.check("dwd", o["dwd"], what, ("channel", "tap"))
    for k in ("dbd", "dln_g", "dln_b") + (("db2",) if full else ()):
        D.check(k, o[k], what, ("channel",))
    if full:
        want = R.dxs_exact(D.view("dx"), up)
        D.check("dxs", R.Out(want.double(), torch.zeros_like(want, dtype=torch.float64), 1), what, TOK)  # (guard rows, finite)
        assert torch.equal(D.view("dxs").view(torch.int16), want.view(torch.int16)), f"{what}: dxs is not bf16(up_scale_b * float(dx))"
    else:
        D.untouched("db2", what)
        D.untouched("dxs", what)
    if bs is not None and bool((bs == 0).any()):
        assert bool((D.view("gu")[bs == 0] == 0).all()), f"{what}: gu of a sample with s_b = 0 is not 0"


def run_bwd(d, name, cls, mode, twice=True):
    m = make(name, cls, mode)
    what = f"pvt_mlp_bwd {name} [{cls}, bscale {mode}]"
    D = launch_bwd(m, d)
    check_bwd(m, D, cls, what)
    if twice:  # a second run without db2 / up_scale / dxs: gu, dh, dx bit-equal; the atomically accumulated sums only within their bound
        D2 = launch_bwd(m, d, full=False)
        for k in ("gu", "dh", "dx"):
            assert torch.equal(D.items[k][0].view(torch.int16), D2.items[k][0].view(torch.int16)), \
                f"{what}: {k} differs without db2 / dxs (or between two runs)"
        check_bwd(m, D2, cls, what + " (no db2, no dxs)", full=False)


# ---- the tests -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_takes_the_path_it_was_chosen_for(dev, name):
    plan_of(name)


@pytest.mark.parametrize("name", SMALL)
def test_forward_stages_plain(dev, name):
    plan_of(name)
    for mode in _modes(CASES[name][0][4]):
        run_fwd(dev, name, "plain", mode)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", CLASS_ROWS)
def test_forward_stages_input_classes(dev, name, cls):
    plan_of(name)
    run_fwd(dev, name, cls, "mixed")


@pytest.mark.parametrize("name", SMALL)
def test_backward_stages_plain(dev, name):
    plan_of(name)
    for mode in _modes(CASES[name][0][4]):
        run_bwd(dev, name, "plain", mode)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", CLASS_ROWS)
def test_backward_stages_input_classes(dev, name, cls):
    plan_of(name)
    run_bwd(dev, name, cls, "mixed")


@pytest.mark.parametrize("name", LARGE)
def test_backward_tile_runs(dev, name):
    """K1's tile loop: tiles per run > 1 with a short last run (asserted), one launch"""
    _, _, tpw, runs = plan_of(name)
    (C, HD, H, W, B), (_, k1th, _, _) = CASES[name]
    tiles = (H // k1th) * (W // 14)
    assert tpw >= 2 and runs >= 2 and 0 < tiles - (runs - 1) * tpw < tpw, (tpw, runs, tiles)
    run_bwd(dev, name, "plain", "ends0", twice=False)


def test_entry_points_refuse(dev):
    m = make("one_tile", "plain", None)
    C, HD, H, W, B = CASES["one_tile"][0]
    for (c, hd, h, w) in ((C, HD, H, 12), (C, HD, 9, W), (96, HD, H, W), (C, 96, H, W)):
        assert not kern.pvt_mlp_supported(m["x"].to(dev), c, hd, h, w)
        with pytest.raises(RuntimeError, match="cenet_pvt_mlp_bwd_plan failed with error code 2"):
            kern.pvt_mlp_bwd_plan(B, h, w, c, hd)
        big = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731 (large enough for any of the four: nothing may launch)
        n = B * max(h, H) * max(w, W)
        args = dict(x=big(n, 128), v=big(2048, dt=F32), w=big(128 * 128), hid=big(n, 128))
        with pytest.raises(RuntimeError, match="cenet_pvt_mlp_fwd_bf16 failed with error code 2"):
            kern.pvt_mlp_fwd(args["x"], args["v"], args["v"], EPS, args["w"], args["v"], args["v"], args["v"], args["w"], args["v"], None,
                             args["x"], B, h, w, c, hd)
        with pytest.raises(RuntimeError, match="cenet_pvt_mlp_bwd_bf16 failed with error code 2"):
            kern.pvt_mlp_bwd(args["x"], None, args["w"], args["w"], args["v"], args["v"], args["hid"], args["x"], args["v"], args["v"],
                             args["v"], args["hid"], args["hid"], args["x"], args["v"], args["v"], args["v"], args["v"], None, B, h, w, c, hd)
    # three of the five saved tensors; up_scale without dxs: CENET_EINVAL, nothing written
    p = m["p"]
    x, ln_g, ln_b, w1, b1, wd, bd, w2, b2 = _to(dev, m["x"], p["ln_g"], p["ln_b"], p["w1"], p["b1"], p["wd"], p["bd"], p["w2"], p["b2"])
    N = H * W
    D = Dests(dev)
    y, xn, mean, rstd = D.new("y", (B, N, C), BF), D.new("xn", (B, N, C), BF), D.new("mean", (B * N,), F32), D.new("rstd", (B * N,), F32)
    with pytest.raises(RuntimeError, match="cenet_pvt_mlp_fwd_bf16 failed with error code 1"):
        kern.pvt_mlp_fwd(x, ln_g, ln_b, EPS, w1, b1, wd, bd, w2, b2, None, y, B, H, W, C, HD, (xn, mean, rstd, None, None))
    _sync(dev)
    for k in D.items:
        D.untouched(k, "fwd with three saved tensors")
    D = Dests(dev)
    gu, dh, dx = D.new("gu", (B, N, HD), BF), D.new("dh", (B, N, HD), BF), D.new("dx", (B, N, C), BF)
    acc = [D.new(k, s, F32, torch.ones(s)) for k, s in (("dwd", (HD, 9)), ("dbd", (HD,)), ("dln_g", (C,)), ("dln_b", (C,)))]
    g, h, mu, rs, up = _to(dev, m["g"], m["h"], m["mean"], m["rstd"], m["up"])
    with pytest.raises(RuntimeError, match="cenet_pvt_mlp_bwd_bf16 failed with error code 1"):
        kern.pvt_mlp_bwd(g, None, w1, w2, wd, bd, h, x, ln_g, mu, rs, gu, dh, dx, *acc, None, B, H, W, C, HD, up_scale=up, dxs=None)
    _sync(dev)
    for k in D.items:
        D.untouched(k, "bwd with up_scale and no dxs")


# ---- the bound must bite (no kernel) ------------------------------------------------------------------------------------------------
def _bf(t):
    return t.float().to(BF)


def _ulp(v):
    """one bf16 ulp at the non-zero bf16 values v"""
    return 2.0 ** (torch.floor(torch.log2(v.float().abs().clamp_min(2.0 ** -100))) - 7)


@pytest.mark.parametrize("name", ["tiles2x2", "k1rows4_c128"])
def test_the_bound_rejects_a_wrong_result(name):
    """every output at the reference's own value (the stage inputs being the reference's own rounded outputs) passes; with 1 % of the
    elements two bf16 ulps off (fp32 sums: 4 x their bound) it is rejected"""
    m = make(name, "plain", "mixed")
    C, HD, H, W, B, p = m["C"], m["HD"], m["H"], m["W"], m["B"], m["p"]
    gsel = _gen(name, 3)
    # a self-consistent set of stage outputs: each stage's own reference, rounded, fed to the next
    xd = m["x"].double()
    xn = _bf(torch.nn.functional.layer_norm(xd, (C,), p["ln_g"].double(), p["ln_b"].double(), EPS))
    h = m["h"]
    s = R._scale(m["bscale"], B, xd)
    a = _bf(s * R.gelu_of(*R.preact(h, p["wd"], p["bd"], B, H, W))[0])
    of = R.fwd(m["x"], p["ln_g"], p["ln_b"], EPS, p["w1"], p["b1"], p["wd"], p["bd"], p["w2"], p["b2"], m["bscale"], dict(xn=xn, h=h, a=a), B, H, W)
    ob0 = R.bwd(m["g"], m["bscale"], p["w1"], p["w2"], p["wd"], p["bd"], h, m["x"], p["ln_g"], m["mean"], m["rstd"],
                dict(gu=torch.zeros_like(h), dh=torch.zeros_like(h)), B, H, W)
    gu = _bf(ob0["gu"].ref)
    dh0 = R.bwd(m["g"], m["bscale"], p["w1"], p["w2"], p["wd"], p["bd"], h, m["x"], p["ln_g"], m["mean"], m["rstd"],
                dict(gu=gu, dh=torch.zeros_like(h)), B, H, W)["dh"].ref
    ob = R.bwd(m["g"], m["bscale"], p["w1"], p["w2"], p["wd"], p["bd"], h, m["x"], p["ln_g"], m["mean"], m["rstd"], dict(gu=gu, dh=_bf(dh0)),
               B, H, W)
    outs = [("xn", R.Out(of["xn"].ref.reshape(B, -1, C), 0.0, 1, of["xn"].extra.reshape(B, -1, C)), BF)]
    outs += [(k, of[k], BF) for k in ("h", "a", "y")] + [(k, ob[k], BF) for k in ("gu", "dh", "dx")]
    outs += [(k, ob[k], F32) for k in SUMS] + [("mean", of["mean"], F32), ("rstd", of["rstd"], F32)]
    for k, o, dt in outs:
        shape = tuple(o.ref.shape)
        add = k in SUMS
        prev = torch.full(shape, 0.75) if add else None
        buf, lead, v = _dest(shape, dt, torch.device("cpu"), prev)
        exp = R.as_exp(buf.clone(), lead, shape, _contig(shape), o, add=add, dims=tuple(f"d{i}" for i in range(len(shape))), kernel=k)
        good = (o.ref + (0.75 if add else 0.0)).float().to(dt)
        v.copy_(good)
        R.assert_bound(buf, exp, f"{k} at the reference")
        pick = torch.rand(shape, generator=gsel) < 0.01
        pick.view(-1)[int((good.reshape(-1) != 0).nonzero()[0])] = True
        if dt == BF:
            pick &= good != 0  # (an exact zero -- a sample with s_b = 0 -- has no ulp to speak of)
            bad = torch.where(pick, (good.float() + 2.0 * _ulp(good)).to(BF), good)
        else:
            idx = exp.idx
            bound = R.bound_of(exp.C, exp.Mag, exp.u_out, exp.K_tot)[idx]
            bad = torch.where(pick, (good.double() + 4.0 * bound).float(), good)
        v.copy_(bad)
        with pytest.raises(AssertionError, match="outside"):
            R.assert_bound(buf, exp, f"{k} moved")
