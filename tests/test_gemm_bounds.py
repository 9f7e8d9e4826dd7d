"""Every GEMM kernel instance the dispatcher can name, held to the float64 interpreter of the ABI (tests/gemm_ref.py).

* INSTANCES: one case per kernel instance `kern.last_gemm_kernel()` can report (the dispatcher, gemm.hip, is host code: the name
  is asserted on the host checker as on the MI355X), at the smallest shapes that select it BY SHAPE, with ragged edges in M and N
  and a K tail.  Every case runs the exact regime (integer operands: the output must equal the reference, no tolerance);
  bf16-store and `act` cases also run the bound regime.  The set of covered names is held equal to the set the dispatcher's rules
  can produce (`_nameable`), and the step replay (tests/test_gemm_replay.py) holds what a training step launches to it.  Operands sit inside NaN-filled buffers, the destination inside a
  sentinel-filled one with an offset and padded strides: nothing outside the M x N x batch footprint may change.
* ABI features no other kernel-level test reaches: col2im scatter, the two-level batch, kinner / sk_outer, r_offset, bscale_rows
  across the edges of the 128-wide tiles, asum on every ring instance.
* grouped weight gradients: every class of cenet_wgrad_group_plan, exact regime.
* mutation self-test (no kernel): deliberately wrong REFERENCES must be rejected by the rules.  Claimed for the two regimes:
      mutation                                          exact   bound (normal + 1 operands)
      last K element dropped                            yes     yes (one of 144 same-sign terms against u_out = 0.4 %)
      one 8-element chunk taken from the next row       yes     no  (same distribution: the rows hit move by less than u_out)
      one split (K batch) omitted                       yes     yes
      bias skipped in the last ragged column            yes     yes
      bscale of the neighbouring sample                 yes     yes
      one col2im tap off by one                         yes     yes
      truncation instead of round-to-nearest (bf16)     yes     yes (up to 2 u_out: C_OUT may not reach 2)
  ("no" = not claimed, not asserted either way.)
`sim` = the kernel sources on the host SIMT checker (CPU); `hip` = the gfx950 library (marker gpu)."""
import math

import pytest
import torch

import gemm_ref as G
from backend import dev  # noqa: F401
from cenet_amd import kern

BF = torch.bfloat16
SENTINEL = 12288.0  # exact in bf16
GARBAGE = 7.5e8     # exact in fp32


def tf(b):
    return "true" if b else "false"


def _sync(dev_):
    if dev_.type == "cuda":
        torch.cuda.synchronize()


# ---- operands inside NaN-filled buffers --------------------------------------------------------------------------------------
def _embed(x, dtype, dev_, aligned, fill=float("nan")):
    """x [L, rows, cols] -> (buffer, element offset, row pitch, matrix stride): rows padded, the lot surrounded by `fill`.
    aligned: offset and pitch multiples of 8 elements (16 bytes in bf16); else odd."""
    L, rows, cols = x.shape
    lead, pitch = (16, (cols + 7) // 8 * 8 + 8) if aligned else (3, cols + 5)
    mat = rows * pitch + (8 if aligned else 7)
    buf = torch.full((lead + L * mat + 16,), fill, dtype=torch.float32)
    body = buf[lead:lead + L * mat].view(L, mat)[:, :rows * pitch].view(L, rows, pitch)
    body[:, :, :cols] = x
    return buf.to(dtype).to(dev_), lead, pitch, mat


def _mat(x, role, kfast, dtype, dev_, aligned, nbatch, nkb, share_batch=False):
    """logical A [L, M, K] / B [L, K, N] (L = nbatch x nkb, or nkb when the operand is shared by the batches) as a MatT"""
    k_last = (role == "A")
    stored = x if (k_last == bool(kfast)) else x.transpose(1, 2)
    buf, lead, pitch, mat = _embed(stored.contiguous(), dtype, dev_, aligned)
    sb = 0 if share_batch else nkb * mat
    if role == "A":
        sr, sc = (pitch, 1) if kfast else (1, pitch)
    else:
        sr, sc = (1, pitch) if kfast else (pitch, 1)
    m = kern.mat_plain(buf, sr, sc, sb=sb, skb=mat, kfast=int(bool(kfast)), offset=lead)
    return m, buf


def _dest(M, N, nbatch, store, dtype, dev_, aligned, fill):
    rows, cols = (M, N) if store == "row" else (N, M)
    lead, pitch = (24, (cols + 7) // 8 * 8 + 8) if aligned else (5, cols + 3)
    mat = rows * pitch + (16 if aligned else 9)
    if isinstance(fill, torch.Generator):
        buf = G.ints((lead + nbatch * mat + 16,), fill)
    else:
        buf = torch.full((lead + nbatch * mat + 16,), fill, dtype=torch.float32)
    kw = dict(scr=pitch, scc=1) if store == "row" else dict(scr=1, scc=pitch)
    kw.update(scb=mat, c_offset=lead)
    return buf.to(dtype).to(dev_), kw


def _vals(shape, g, regime):
    if regime == "exact":
        return G.ints(shape, g)
    return G.reals(shape, g, 1.0 if regime == "offset" else 0.0).to(BF).float()


def _pow2(n, g):
    return torch.tensor([0.5, 1.0, 2.0, -1.0, -2.0, 0.25])[torch.randint(0, 6, (n,), generator=g)]


def run_case(dev_, c, regime):
    """one launch of case `c` (a dict) in one regime; returns the worst bound ratio (0 in the exact regime)"""
    g = torch.Generator().manual_seed(c.get("seed", 1))
    M, N, K = c["M"], c["N"], c["K"]
    nbatch, nkb, atomic = c.get("nbatch", 1), c.get("nkb", 1), c.get("atomic", 0)
    dt = torch.float32 if c.get("f32") else BF
    out_dt = torch.float32 if (atomic or c.get("f32")) else BF
    aligned, store = c.get("aligned", True), c.get("store", "row")
    act = c.get("act", "none")
    if act != "none":  # the exact regime takes a piecewise-linear activation (slope 1/4), the bound regime the transcendental one
        act = ("lrelu" if c.get("lrelu") else "relu") if regime == "exact" else "gelu"
    with G.capture():
        a = _vals((nbatch * nkb if not c.get("share_a", True) else nkb, M, K), g, regime)
        A, ba = _mat(a, "A", c["akf"], dt, dev_, aligned, nbatch, nkb, share_batch=c.get("share_a", True))
        if "im2col" in c:
            Bm, bb = c["im2col"](g, regime, dt, dev_)
        else:
            b = _vals((nbatch * nkb, K, N), g, regime)
            Bm, bb = _mat(b, "B", c["bkf"], dt, dev_, aligned, nbatch, nkb)
    if atomic == 1:
        fill = g if regime == "exact" else 0.75
    else:
        fill = GARBAGE if atomic == 2 else SENTINEL
    Cbuf, kw = _dest(M, N, nbatch, store, out_dt, dev_, aligned, fill)
    kw.update(nbatch=nbatch, nkb=nkb, atomic=atomic, splits=c.get("splits", 1))
    kw["alpha"] = c.get("alpha", 0.5 if atomic else 2.0)
    if atomic == 1 and c.get("asum"):
        kw["asum"] = (G.ints((M,), g) if regime == "exact" else torch.zeros(M)).to(dev_)
    if not atomic:
        on_row = store == "col"
        kw.update(bias=_vals((M if on_row else N,), g, regime).to(dev_), bias_on_row=on_row, act=act, slope=0.25)
        if c.get("bscale_rows"):
            kw.update(bscale=_pow2(-(-M // c["bscale_rows"]), g).to(dev_), bscale_rows=c["bscale_rows"])
        elif nbatch > 1:
            kw["bscale"] = _pow2(nbatch, g).to(dev_)
        if c.get("resid", True):
            r = _vals((nbatch, M, N) if store == "row" else (nbatch, N, M), g, regime)
            Rbuf, lead, pitch, mat = _embed(r, out_dt, dev_, aligned)
            kw.update(R=Rbuf, r_offset=lead, srb=mat, **(dict(srr=pitch, src=1) if store == "row" else dict(srr=1, src=pitch)))
    exp = G.expected(A, Bm, Cbuf, M, N, K, **kw)
    kern.gemm(A, Bm, Cbuf, M, N, K, **kw)
    _sync(dev_)
    assert kern.last_gemm_kernel() == c["name"], (kern.last_gemm_kernel(), c["name"])
    what = f"{c['name']} [{regime}]"
    if regime == "exact":
        G.assert_exact(Cbuf, exp, what)
        if "asum" in kw:
            G.assert_vec_exact(kw["asum"], exp.asum, exp.asum_mag, what + " asum")
        return 0.0
    ratio = G.assert_bound(Cbuf, exp, what)
    if "asum" in kw:
        G.assert_vec_bound(kw["asum"], exp.asum, exp.asum_mag, exp.K_tot, what + " asum")
    print(f"BOUND {what} M={M} N={N} K={K} nbatch={nbatch} nkb={nkb}: worst |err| / bound = {ratio:.3f}")
    return ratio


# ---- the covered instances: the parametrisation below is generated from this list, the step replay's census is held to it -----
ORIENT = [(1, 1), (1, 0), (0, 1), (0, 0)]
COVERED = []


def _add(name, **c):
    c["name"] = name
    c["id"] = f"{name.replace(' ', '')}-{c['M']}x{c['N']}x{c['K']}" + ("" if c.get("aligned", True) else "-unal") + c.pop("tag", "")
    COVERED.append(c)


# ring (LDS-DMA) kernel: tile chosen by the number of workgroups (non-atomic) or by K nkb and M N (atomic)
RING_SHAPES = {  # (bm, bn, ns): (M, N, K, nbatch) -- M x N ragged against the tile, K = whole steps + a tail of 8
    (64, 64, 4): (104, 72, 136, 1),
    (128, 128, 2): (248, 248, 72, 64),   # 2 x 2 x 64 = 256 workgroups of 128 x 128
    (128, 64, 3): (240, 248, 72, 32),    # 128 of 128 x 128 is too few; M < N halves the column tile: 2 x 4 x 32
    (64, 128, 3): (248, 248, 72, 32),    # M >= N halves the row tile
}
RING_ATOMIC = {  # (M, N, K, nkb): the rectangular tiles need K nkb >= 4096 and M N >= 131072
    (64, 64, 4): (104, 72, 136, 2),
    (64, 128, 3): (368, 360, 1032, 4),
    (128, 64, 3): (1096, 120, 1032, 4),
}
for (bm, bn, ns), (M, N, K, nb) in RING_SHAPES.items():
    for akf, bkf in ORIENT:
        for store in ("row", "col"):
            _add(f"gemm_ring_kernel<{tf(akf)}, {tf(bkf)}, {bm}, {bn}, {ns}, {tf(store == 'row')}>", M=M, N=N, K=K, nbatch=nb,
                 akf=akf, bkf=bkf, store=store, bound=True, share_a=(nb > 1), slow=(nb > 1 and (akf, bkf) not in ((1, 1), (0, 0))))
for (bm, bn, ns), (M, N, K, nkb) in RING_ATOMIC.items():
    for akf, bkf in ORIENT:
        big = M * N > 100000
        _add(f"gemm_ring_kernel<{tf(akf)}, {tf(bkf)}, {bm}, {bn}, {ns}, false>", M=M, N=N, K=K, nkb=nkb, akf=akf, bkf=bkf,
             atomic=1, splits=3, asum=True, tag="-add", slow=big and (akf, bkf) != (1, 0))
        _add(f"gemm_ring_kernel<{tf(akf)}, {tf(bkf)}, {bm}, {bn}, {ns}, false>", M=M, N=N, K=K, nkb=nkb, akf=akf, bkf=bkf,
             atomic=2, store="col" if akf else "row", tag="-store", slow=big and (akf, bkf) != (0, 1))
# pitches / extents / K that are not multiples of 8 elements and an odd base offset (ring_unal): every tile, both stores
for (bm, bn, ns), (M, N, K, nb) in RING_SHAPES.items():
    for (akf, bkf), store in (((1, 1), "row"), ((0, 0), "col")):
        _add(f"gemm_ring_kernel<{tf(akf)}, {tf(bkf)}, {bm}, {bn}, {ns}, {tf(store == 'row')}>", M=M - 3, N=N - 5, K=K + 3, nbatch=nb,
             akf=akf, bkf=bkf, store=store, aligned=False, bound=True, share_a=(nb > 1), slow=(nb > 1 and store == "col"))
_add("gemm_ring_kernel<true, true, 64, 64, 4, false>", M=49, N=49, K=515, nkb=2, akf=1, bkf=1, atomic=1, splits=2, asum=True,
     aligned=False, tag="-add")
# persistent streaming variant: K = 64 / 128, at least 768 tiles of 64 x 64 (7 x 4 x 28), aligned operands only
for K in (64, 128):
    for akf, bkf in ORIENT:
        for store in ("row", "col"):
            _add(f"gemm_ring_stream_kernel<{tf(akf)}, {tf(bkf)}, {tf(store == 'row')}, {K // 64}>", M=440, N=248, K=K, nbatch=28,
                 akf=akf, bkf=bkf, store=store, bound=True, share_a=True, slow=(akf, bkf) not in ((1, 1), (0, 0)))
# plain kernel (what the ring does not take: an activation, M or N below 48), bf16 and fp32 (parity mode): pick_tile's six tiles x both
# stores; the 128-wide ones need 256 workgroups.  bf16 has a K-step-64 instance of the 32 x 64 and 64 x 64 tiles (K >= 128).
TILE_SHAPES = {  # (bm, bn): (M, N, nbatch)
    (32, 64): (40, 100, 1), (32, 256): (40, 300, 1), (64, 64): (104, 72, 1),
    (128, 64): (248, 72, 128), (64, 128): (72, 248, 128), (128, 128): (248, 248, 64),
}
for f32 in (False, True):
    ty = "float" if f32 else "unsigned short"
    for (bm, bn), (M, N, nb) in TILE_SHAPES.items():
        for store in ("row", "col"):
            for ks in (32, 64):
                if ks == 64 and (f32 or bn != 64 or bm > 64):
                    continue
                K = 200 if ks == 64 else (40 if (f32 and nb > 1) else 72)
                _add(f"gemm_kernel<{ty}, {bm}, {bn}, false, {tf(store == 'row')}, {ks}>", M=M, N=N, K=K, nbatch=nb, akf=1,
                     bkf=(store == "col"), store=store, act="relu", bound=True, share_a=(nb > 1), lrelu=(store == "col"), f32=f32,
                     slow=(nb > 1 and (store == "col" or f32)))
_add("gemm_kernel<unsigned short, 64, 64, false, true, 32>", M=101, N=67, K=75, akf=0, bkf=0, act="relu", aligned=False, bound=True)
_add("gemm_kernel<unsigned short, 32, 64, false, false, 32>", M=40, N=60, K=136, nkb=3, akf=0, bkf=1, atomic=1, splits=2,
     tag="-add")
_add("gemm_kernel<float, 64, 64, false, false, 32>", M=101, N=67, K=75, akf=0, bkf=0, f32=True, store="col", aligned=False,
     tag="-rr")
_add("gemm_kernel<float, 64, 64, false, false, 32>", M=104, N=72, K=136, nkb=2, akf=1, bkf=0, f32=True, atomic=1, splits=3,
     asum=True, tag="-add")


def _conv_b(Ci, H, W, k, stride, pad, form):
    """im2col B operand of a convolution: form 'fwd' (patch rows, pixels columns), 'dgrad' (the transposed gather) or 'wgrad'
    (pixels are the reduction: kfast, K batches).  Returns (factory for run_case, N or K)"""
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1

    def make(g, regime, dt, dev_, nb):
        if form == "dgrad":  # the image gathered from is dY [Ci, Ho, Wo]; output pixels are the input grid H x W
            x = _vals((nb, Ci * Ho, Wo), g, regime)
            buf, lead, pitch, mat = _embed(x, dt, dev_, True)
            return kern.mat_im2col(buf, sb=mat, skb=0, sci=Ho * pitch, sy=pitch, sx=1, KH=k, KW=k, Pw=W, Hs=Ho, Ws=Wo, stride=stride,
                                   pad=pad, dil=1, patch_is_row=1, transposed=1, kfast=0, offset=lead), buf
        x = _vals((nb, Ci * H, W), g, regime)
        buf, lead, pitch, mat = _embed(x, dt, dev_, True)
        if form == "fwd":
            return kern.mat_im2col(buf, sb=mat, skb=0, sci=H * pitch, sy=pitch, sx=1, KH=k, KW=k, Pw=Wo, Hs=H, Ws=W, stride=stride,
                                   pad=pad, dil=1, patch_is_row=1, transposed=0, kfast=0, offset=lead), buf
        return kern.mat_im2col(buf, sb=0, skb=mat, sci=H * pitch, sy=pitch, sx=1, KH=k, KW=k, Pw=Wo, Hs=H, Ws=W, stride=stride,
                               pad=pad, dil=1, patch_is_row=0, transposed=0, kfast=1, offset=lead), buf
    return make, Ho, Wo


def _add_conv(name, Co, Ci, H, W, k, stride, pad, form, nb, **c):
    make, Ho, Wo = _conv_b(Ci, H, W, k, stride, pad, form)
    if form == "fwd":
        M, N, K, extra = Co, Ho * Wo, Ci * k * k, dict(nbatch=nb)
    elif form == "dgrad":
        M, N, K, extra = Co, H * W, Ci * k * k, dict(nbatch=nb)   # (Co here = channels of dX, Ci = channels of dY)
    else:
        M, N, K, extra = Co, Ci * k * k, Ho * Wo, dict(nkb=nb, atomic=1, splits=2)
    _add(name, M=M, N=N, K=K, akf=1, share_a=(form != "wgrad"), tag=f"-{form}k{k}s{stride}",
         im2col=lambda g, regime, dt, dev_, make=make, nb=nb: make(g, regime, dt, dev_, nb), **extra, **c)


# im2col instances, bf16 and fp32: a forward convolution on each of the six tiles, stored row-major and transposed (the 128-wide
# tiles are what a convolution at training batch selects); the transposed (data-gradient) gather; the weight-gradient view (k-fast
# gather, atomic; with a 32-row tile it never takes the 256-column one)
CONV_SHAPES = {  # (bm, bn): (Co, Ci, H, W, k, stride, pad, nbatch)
    (32, 64): (6, 5, 13, 11, 3, 2, 1, 2), (32, 256): (6, 5, 17, 15, 3, 1, 1, 2), (64, 64): (56, 3, 29, 27, 7, 4, 3, 2),
    (128, 64): (136, 5, 9, 8, 3, 1, 1, 64), (64, 128): (56, 2, 15, 15, 3, 1, 1, 128), (128, 128): (136, 5, 15, 15, 3, 1, 1, 64),
}
for f32 in (False, True):
    ty = "float" if f32 else "unsigned short"
    for (bm, bn), (Co, Ci, H, W, k, st, pad, nb) in CONV_SHAPES.items():
        for store in ("row", "col"):
            _add_conv(f"gemm_kernel<{ty}, {bm}, {bn}, true, {tf(store == 'row')}, 32>", Co, Ci, H, W, k, st, pad, "fwd", nb,
                      store=store, f32=f32, bound=(not f32 or (bm, bn) == (64, 64)), act="relu" if (bm, bn) == (64, 64) else "none",
                      slow=(nb > 2 and (store == "col" or f32)))
    _add_conv(f"gemm_kernel<{ty}, 64, 64, true, true, 32>", 50, 6, 13, 11, 3, 1, 1, "dgrad", 2, f32=f32, bound=not f32)
    _add_conv(f"gemm_kernel<{ty}, 32, 64, true, false, 32>", 6, 5, 13, 11, 3, 2, 1, "wgrad", 3, f32=f32)
    _add_conv(f"gemm_kernel<{ty}, 64, 64, true, false, 32>", 56, 5, 13, 11, 3, 1, 1, "wgrad", 3, f32=f32)

COVERED_NAMES = sorted({c["name"] for c in COVERED})   # the step replay's census (tests/test_gemm_replay.py) is held to this list
GROUP_COVERED = [G.group_name(64, 64, 4), G.group_name(128, 128, 2)]  # plan classes of test_grouped_wgrad_plan_classes_exact


def _nameable():
    """every name gemm_dispatch (csrc/gemm.hip) can print, from its rules: the ring and its streaming variant over the four operand
    orientations and both stores, four ring tiles; the plain kernel over both element types, pick_tile's six tiles, plain / im2col,
    both stores, with a K-step-64 instance for bf16 plain operands on the 32 x 64 and 64 x 64 tiles.  Nothing is excluded."""
    names = set()
    for akf, bkf in ORIENT:
        for swap in (True, False):
            names |= {f"gemm_ring_kernel<{tf(akf)}, {tf(bkf)}, {bm}, {bn}, {ns}, {tf(swap)}>"
                      for bm, bn, ns in ((64, 64, 4), (128, 128, 2), (128, 64, 3), (64, 128, 3))}
            names |= {f"gemm_ring_stream_kernel<{tf(akf)}, {tf(bkf)}, {tf(swap)}, {ks}>" for ks in (1, 2)}
    for ty in ("unsigned short", "float"):
        for bm, bn in ((32, 64), (32, 256), (64, 64), (128, 64), (64, 128), (128, 128)):
            for im in (False, True):
                for swap in (True, False):
                    names.add(f"gemm_kernel<{ty}, {bm}, {bn}, {tf(im)}, {tf(swap)}, 32>")
                    if ty == "unsigned short" and not im and bm <= 64 and bn == 64:
                        names.add(f"gemm_kernel<{ty}, {bm}, {bn}, {tf(im)}, {tf(swap)}, 64>")
    return names


def test_every_nameable_instance_has_a_case():
    assert set(COVERED_NAMES) == _nameable(), (sorted(_nameable() - set(COVERED_NAMES)), sorted(set(COVERED_NAMES) - _nameable()))


def _slow(c):
    """on the host checker a case costs about a second per 20 M multiply-adds: the big-tile instances (256 workgroups and more) are
    marked slow there; with -m gpu every case runs"""
    return c.get("slow") or c["M"] * c["N"] * c["K"] * c.get("nbatch", 1) * c.get("nkb", 1) > 40e6


def _params(cases):
    return [pytest.param(c, id=c["id"], marks=[pytest.mark.slow] if _slow(c) else []) for c in cases]


@pytest.mark.parametrize("case", _params(COVERED))
def test_instance_exact(dev, case):
    """integer operands: the instance named, the output equal to the reference, nothing outside the footprint touched"""
    run_case(dev, case, "exact")


@pytest.mark.parametrize("regime", ["normal", "offset"])
@pytest.mark.parametrize("case", _params([c for c in COVERED if c.get("bound")]))
def test_instance_bound(dev, case, regime):
    """bf16-store and activation cases on real-valued operands: |err| <= C_OUT u_out |ref| + C_ACC 2^-24 sqrt(K) Mag"""
    run_case(dev, case, regime)


# ---- the asum reductions of the non-ring contractions -------------------------------------------------------------------------
def _asum_route(A, M, K, nkb):
    """which reduction launch_asum (csrc/gemm.hip) takes for an A descriptor: its predicates, in its order"""
    if A.sr == 1 and A.sc == M and nkb == 1:
        return "col_sum"            # token-major dY [K, M]: cenet_col_sum_acc
    if A.sc == 1 and A.sr == K and (nkb == 1 or A.skb >= M * K):
        return "chan_dot"           # channel planes [nkb][M][K]: cenet_chan_dot_acc
    if A.sr == 1 and A.sc != 1:
        return "rows_contiguous"    # gemm_asum_kernel, thread = row
    return "row_per_workgroup"      # gemm_asum_kernel, workgroup = row


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("route", ["col_sum", "chan_dot", "rows_contiguous", "row_per_workgroup"])
def test_asum_routes(dev, route, f32):
    """launch_asum (gemm.hip): the two tuned reductions (token-major dY [K, M]; channel planes [nkb][M][K]) and the two forms of
    gemm_asum_kernel (rows contiguous with K batches; a padded k-contiguous A), N < 48 so that the ring does not take them.
    The route is decided by A's strides alone: the descriptor of each case is held to launch_asum's predicate (_asum_route), so a
    layout change that sends a case down another route fails here instead of leaving a reduction untested."""
    g = torch.Generator().manual_seed(7)
    dt = torch.float32 if f32 else BF
    M, N, K = 72, 40, 203
    nkb = 1 if route == "col_sum" else 3
    with G.capture():
        a = G.ints((nkb, M, K), g)
        if route == "col_sum":
            ta = a[0].t().contiguous().to(dt).to(dev)
            A = kern.mat_plain(ta, 1, M, kfast=0)
        elif route == "chan_dot":
            ta = a.contiguous().to(dt).to(dev)
            A = kern.mat_plain(ta, K, 1, skb=M * K, kfast=1)
        else:
            A, ta = _mat(a, "A", route == "row_per_workgroup", dt, dev, False, 1, nkb)
        Bm, tb = _mat(G.ints((nkb, K, N), g), "B", 1, dt, dev, False, 1, nkb)
    assert _asum_route(A, M, K, nkb) == route
    Cbuf, kw = _dest(M, N, 1, "row", torch.float32, dev, False, g)
    asum = G.ints((M,), g).to(dev)
    kw.update(nkb=nkb, atomic=1, splits=2, asum=asum, alpha=0.5)
    exp = G.expected(A, Bm, Cbuf, M, N, K, **kw)
    kern.gemm(A, Bm, Cbuf, M, N, K, **kw)
    _sync(dev)
    assert kern.last_gemm_kernel().startswith(f"gemm_kernel<{'float' if f32 else 'unsigned short'}, 64, 64, false, false, ")
    G.assert_exact(Cbuf, exp, route)
    G.assert_vec_exact(asum, exp.asum, exp.asum_mag, route + " asum")


# ---- ABI features --------------------------------------------------------------------------------------------------------------
def _col2im_case(dev_, dt, k, stride, pad, regime, seed=3):
    """data gradient of a strided convolution as linear.py issues it: dXcol[(ci,ky,kx), p] = W^T dY[:, p] scattered into dX
    (atomic adds into fp32 when the patches overlap, k > stride)"""
    g = torch.Generator().manual_seed(seed)
    B, Ci, Co, H, W = 2, 5, 12, 18, 14
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    Kd, overlap = Ci * k * k, k > stride
    out_dt = torch.float32 if (overlap or dt == torch.float32) else BF
    with G.capture():
        w = _vals((1, Co, Kd), g, regime)       # A(m, c) = W[c, m]: rows contiguous
        A, wa = _mat(w.transpose(1, 2).contiguous(), "A", 0, dt, dev_, True, 1, 1, share_batch=True)
        dy = _vals((B, Co, Ho * Wo), g, regime)
        Bm, wb = _mat(dy, "B", 0, dt, dev_, True, B, 1)
    lead, sy = 11, W + 3
    plane = H * sy + 5
    if overlap:
        dx = (G.ints((lead + B * Ci * plane + 9,), g) if regime == "exact" else torch.full((lead + B * Ci * plane + 9,), 0.5))
    else:
        dx = torch.full((lead + B * Ci * plane + 9,), SENTINEL)
    dx = dx.to(out_dt).to(dev_)
    kw = dict(scr=0, scc=0, scb=Ci * plane, nbatch=B, atomic=int(overlap), c_offset=lead,
              col2im=dict(KH=k, KW=k, Pw=Wo, Hs=H, Ws=W, stride=stride, pad=pad, sci=plane, sy=sy, sx=1))
    return A, Bm, dx, (Kd, Ho * Wo, Co), kw, (wa, wb)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("k,stride,pad", [(2, 2, 0), (4, 4, 0), (3, 2, 1), (7, 4, 3)])
def test_col2im_scatter(dev, k, stride, pad, f32):
    """stride 2 / 4, non-overlapping patches (plain stores; the image pixels no patch covers keep their value) and overlapping
    ones (atomic adds onto a non-zero fp32 image)"""
    for regime in ("exact", "offset"):
        A, Bm, dx, (M, N, K), kw, keep = _col2im_case(dev, torch.float32 if f32 else BF, k, stride, pad, regime)
        exp = G.expected(A, Bm, dx, M, N, K, **kw)
        kern.gemm(A, Bm, dx, M, N, K, **kw)
        _sync(dev)
        if regime == "exact":
            G.assert_exact(dx, exp, f"col2im k{k}s{stride}")
        else:
            G.assert_bound(dx, exp, f"col2im k{k}s{stride}")


@pytest.mark.parametrize("M,N,K,ring", [(104, 72, 72, True), (40, 60, 45, False)])
def test_two_level_batch(dev, M, N, K, ring):
    """nb_inner > 1: batch z -> (z / nb_inner, z % nb_inner) with sb2 / scb2 / srb2, as the attention and grouped-conv call sites
    use it: [B, H] heads whose operands, outputs and residual have independent outer and inner strides (nbatch not a multiple of
    nb_inner is not used by the product)"""
    g = torch.Generator().manual_seed(11)
    Bo, Hh = 2, 3
    with G.capture():
        # A: [H, B, M, K] (inner stride larger than the outer), B: [B, H, K, N]
        a, b = G.ints((Hh * Bo, M, K), g), G.ints((Bo * Hh, K, N), g)
        A, ta = _mat(a, "A", 1, BF, dev, True, 1, 1)
        Bm, tb = _mat(b, "B", 0, BF, dev, True, 1, 1)
        A.sb, A.sb2 = A.skb, Bo * A.skb
        Bm.sb, Bm.sb2 = Hh * Bm.skb, Bm.skb
    Cbuf, kw = _dest(M, N, Bo * Hh, "row", BF, dev, True, SENTINEL)
    mat = kw.pop("scb")
    r = G.ints((Bo * Hh, M, N), g)
    Rbuf, lead, pitch, rmat = _embed(r, BF, dev, True)
    # C laid out [H, B] (scb = one matrix, scb2 = B matrices), R laid out [B, H]
    kw.update(scb=mat, scb2=Bo * mat, nbatch=Bo * Hh, nb_inner=Hh, R=Rbuf, r_offset=lead, srb=Hh * rmat, srb2=rmat, srr=pitch, src=1,
              bias=G.ints((N,), g).to(dev), alpha=2.0)
    exp = G.expected(A, Bm, Cbuf, M, N, K, **kw)
    kern.gemm(A, Bm, Cbuf, M, N, K, **kw)
    _sync(dev)
    assert kern.last_gemm_kernel().startswith("gemm_ring_kernel") == ring
    G.assert_exact(Cbuf, exp, "nb_inner")


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_kinner_split_reduction_index(dev, f32):
    """kinner / sk_outer: the data gradient of a stride-1 convolution reads W [Cout, Cin, k, k] as A(ci, (co, ky, kx)):
    k -> (k / (k k)) sk_outer + (k % (k k)) (linear.py), against the transposed im2col gather of dY"""
    g = torch.Generator().manual_seed(13)
    dt = torch.float32 if f32 else BF
    B, Ci, Co, H, W, k, pad = 2, 7, 6, 13, 11, 3, 1
    with G.capture():
        w = G.ints((Co, Ci, k, k), g)
        wbuf, lead, pitch, mat = _embed(w.reshape(1, Co * Ci, k * k), dt, dev, False)
        A = kern.mat_plain(wbuf, pitch, 1, kfast=1, kinner=k * k, sk_outer=Ci * pitch, offset=lead)
        make, Ho, Wo = _conv_b(Co, H, W, k, 1, pad, "dgrad")
        Bm, tb = make(g, "exact", dt, dev, B)
    M, N, K = Ci, H * W, Co * k * k
    Cbuf, kw = _dest(M, N, B, "row", dt, dev, False, SENTINEL)
    kw.update(nbatch=B, alpha=0.5)
    exp = G.expected(A, Bm, Cbuf, M, N, K, **kw)
    kern.gemm(A, Bm, Cbuf, M, N, K, **kw)
    _sync(dev)
    G.assert_exact(Cbuf, exp, "kinner")


@pytest.mark.parametrize("bm", [pytest.param(128, marks=pytest.mark.slow), 64])
def test_bscale_rows_straddles_tile_edges(dev, bm):
    """per-sample scale looked up by row (bscale_rows = n) with n = 50: samples straddle the 64- and 128-row tile edges; on the
    128 x 128 ring tile (256 workgroups) and the 64 x 64 one"""
    n = 50
    c = dict(M=4050 if bm == 128 else 250, N=1000 if bm == 128 else 72, K=72, akf=1, bkf=1, bscale_rows=n,
             name=f"gemm_ring_kernel<true, true, {bm}, {bm}, {2 if bm == 128 else 4}, true>")
    run_case(dev, c, "exact")
    run_case(dev, c, "offset")


# ---- grouped weight gradients --------------------------------------------------------------------------------------------------
def _group_problem(g, dev_, kind, M, N, K, nkb=1, aligned=True, share=None):
    """kind 'lin': dY [K, M], X [K, N] token-major (kfast 0); 'conv': dY [nkb, M, K], X [nkb, N, K] (kfast 1).  Integer operands,
    NaN-surrounded; the destination starts from non-zero integers."""
    kf = int(kind == "conv")
    a = G.ints((nkb, K, M) if not kf else (nkb, M, K), g)
    b = G.ints((nkb, K, N) if not kf else (nkb, N, K), g)
    ba, la, pa, ma = _embed(a, BF, dev_, aligned)
    bb, lb, pb, mb = _embed(b, BF, dev_, aligned)
    if share is None:
        dW, db = G.ints((M, N), g).to(dev_), G.ints((M,), g).to(dev_)
    else:
        dW, db = share
    av, bv = ba[la:], bb[lb:]
    item = (av.data_ptr(), bv.data_ptr(), dW.data_ptr(), db.data_ptr(), pa, pb, ma, mb, M, N, K, nkb, kf)
    return dict(item=item, a=av, b=bv, dW=dW, db=db, args=(pa, pb, ma, mb, M, N, K, nkb, kf), keep=(ba, bb))


@pytest.mark.parametrize("depth", [None, "8"], ids=["depth32", "depth8"])
def test_grouped_wgrad_plan_classes_exact(dev, monkeypatch, depth):
    """cenet_wgrad_group_plan's classes in one call: skinny (64 x 64 x 4 tiles) and both sides >= 128 (128 x 128 x 2), both
    orientations, ragged M / N / K, unaligned planes; long reductions cut into K slices and folded (a small depth target
    reaches that class at test sizes); two problems sharing one destination (the atomic path)"""
    if depth:
        monkeypatch.setenv("CENET_GROUP_DEPTH", depth)
    g = torch.Generator().manual_seed(19)
    probs = [_group_problem(g, dev, "lin", 72, 136, 203), _group_problem(g, dev, "lin", 136, 200, 150),
             _group_problem(g, dev, "conv", 64, 56, 49, nkb=3, aligned=False), _group_problem(g, dev, "conv", 136, 160, 100, nkb=2),
             _group_problem(g, dev, "lin", 64, 128, 6000), _group_problem(g, dev, "conv", 160, 136, 196, nkb=33, aligned=False)]
    shared = _group_problem(g, dev, "lin", 64, 64, 500)
    probs += [shared, _group_problem(g, dev, "lin", 64, 64, 260, share=(shared["dW"], shared["db"]))]
    plan = kern.wgrad_group_plan([p["item"] for p in probs])
    assert {(bm, bn, ns) for _, bm, bn, ns in plan} == {(64, 64, 4), (128, 128, 2)}
    assert len({li for li, *_ in plan}) == 4  # (orientation x tile class)
    exps = {}
    for p in probs:  # two problems with one destination: the second expectation starts from the first
        key = p["dW"].data_ptr()
        prev = exps.get(key)
        e = G.expected_wgrad(p["a"], p["b"], p["dW"] if prev is None else prev.C, p["db"] if prev is None else prev.asum, *p["args"])
        if prev is not None:
            e.Mag, e.asum_mag = e.Mag + prev.Mag, e.asum_mag + prev.asum_mag
        exps[key] = e
    need = kern.wgrad_group([p["item"] for p in probs], dev)
    _sync(dev)
    assert need > 0, "the K-sliced class (workspace + fold launch) is reached"
    for p in probs:
        e = exps[p["dW"].data_ptr()]
        what = f"grouped {p['args'][4:]}"
        G.assert_vec_exact(p["dW"], e.C, e.Mag, what + " C")
        G.assert_vec_exact(p["db"], e.asum, e.asum_mag, what + " asum")


# ---- mutation self-test: no kernel involved ------------------------------------------------------------------------------------
def _trunc_bf16(x64):
    return (x64.float().view(torch.int32) & -65536).view(torch.float32).to(BF)


def _mut_setup(regime, seed=23):
    """a [B n, K] x [N, K]^T flat Linear with bias, per-row sample scale and K batches on CPU tensors: (descriptors, kwargs)"""
    g = torch.Generator().manual_seed(seed)
    M, N, K, nkb, n = 150, 70, 72, 2, 50
    cpu = torch.device("cpu")
    with G.capture():
        a, b = _vals((nkb, M, K), g, regime), _vals((nkb, K, N), g, regime)
        A, ta = _mat(a, "A", 1, BF, cpu, True, 1, nkb)
        Bm, tb = _mat(b, "B", 1, BF, cpu, True, 1, nkb)
    Cbuf, kw = _dest(M, N, 1, "row", BF, cpu, True, SENTINEL)
    bs = torch.tensor([0.5, 2.0, -1.0])
    kw.update(nkb=nkb, bias=_vals((N,), g, regime) + (4.0 if regime != "exact" else 0.0), bscale=bs, bscale_rows=n, alpha=1.0)
    return (A, Bm, Cbuf, M, N, K), kw, (ta, tb)


def _as_output(exp_wrong, exp, truncate=False):
    """what a kernel computing the wrong reference would have left in the buffer"""
    conv = _trunc_bf16 if truncate else (lambda x: x.float().to(exp.out_dtype))
    return torch.where(exp.own, conv(exp_wrong.C), conv(exp.C))


MUTATIONS = ["drop_last_k", "chunk_next_row", "omit_split", "bias_last_col", "bscale_neighbour", "truncate"]
BOUND_CLAIMS = {"drop_last_k", "omit_split", "bias_last_col", "bscale_neighbour", "truncate", "col2im_tap"}


def _mutated(name, regime):
    (A, Bm, Cbuf, M, N, K), kw, keep = _mut_setup(regime)
    exp = G.expected(A, Bm, Cbuf, M, N, K, **kw)
    aflat, abase = G.storage(A._t, A._off)
    kw2, trunc = dict(kw), False
    if name == "drop_last_k":
        aflat[abase + torch.arange(M) * A.sr + (K - 1)] = 0.0  # (first K batch only)
    elif name == "chunk_next_row":
        r = 77
        aflat[abase + r * A.sr + 16: abase + r * A.sr + 24] = aflat[abase + (r + 1) * A.sr + 16: abase + (r + 1) * A.sr + 24].clone()
    elif name == "omit_split":
        kw2["nkb"] = 1
    elif name == "bias_last_col":
        kw2["bias"] = kw["bias"].clone()
        kw2["bias"][N - 1] = 0.0
    elif name == "bscale_neighbour":  # rows 100 .. 127 (sample 2's share of the 64-row tile that sample 1 starts) scaled as sample 1
        e2 = G.expected(A, Bm, Cbuf, M, N, K, **dict(kw, bscale=torch.tensor([0.5, 2.0, 2.0])))
        wrong = exp.C.clone()
        rows = exp.idx[0, 100:128].reshape(-1)
        wrong[rows] = e2.C[rows]
        return exp, _as_output(G.SimpleNamespace(C=wrong), exp)
    elif name == "truncate":
        trunc = True
    wrong = G.expected(A, Bm, Cbuf, M, N, K, **kw2)
    return exp, _as_output(wrong, exp, truncate=trunc)


@pytest.mark.parametrize("name", MUTATIONS)
def test_mutations_are_rejected(name):
    """the acceptance rules fed deliberately wrong references: the exact regime rejects every one, the bound regime those the
    module docstring claims for it; and both accept the unmutated reference"""
    exp, got = _mutated(name, "exact")
    G.assert_exact(G.round_once(exp.C, exp.out_dtype), exp, "unmutated")
    with pytest.raises(AssertionError):
        G.assert_exact(got, exp, name)
    if name in BOUND_CLAIMS:
        exp, got = _mutated(name, "offset")
        assert G.assert_bound(exp.C.float().to(BF), exp, "unmutated") <= 1.0
        with pytest.raises(AssertionError):
            G.assert_bound(got, exp, name)


def test_mutation_col2im_tap_off_by_one():
    cpu = torch.device("cpu")
    for regime, check in (("exact", G.assert_exact), ("offset", G.assert_bound)):
        A, Bm, dx, (M, N, K), kw, keep = _col2im_case(cpu, BF, 3, 2, 1, regime)
        exp = G.expected(A, Bm, dx, M, N, K, **kw)
        check(exp.C.float() if regime != "exact" else G.round_once(exp.C, exp.out_dtype), exp, "unmutated")
        # tap (ci 1, ky 1, kx 0) lands where (ci 1, ky 1, kx 1) belongs: its row of A moves one patch row down
        aflat, abase = G.storage(A._t, A._off)
        m0 = 1 * 9 + 1 * 3 + 0
        cols = abase + torch.arange(K) * A.sc
        aflat[cols + m0 + 1] += aflat[cols + m0]
        aflat[cols + m0] = 0.0
        wrong = G.expected(A, Bm, dx, M, N, K, **kw)
        with pytest.raises(AssertionError):
            check(wrong.C.float(), exp, "col2im tap")


def test_constants_are_the_host_measurement():
    """C_ACC / C_OUT in gemm_ref.py come from this measurement (fp32 on the host against float64), never from a kernel.  The
    shapes are those of the matrix above with M and N clipped to 128 and without the batch (batches are independent contractions
    of one shape; the ratio depends on K and the number of K batches).  The values gemm_ref records are pinned: the measurement
    must reproduce them, C_ACC is 4 x the accumulation ratio rounded up to a tenth, C_OUT covers the store ratio and stays
    below what truncation needs (2)."""
    shapes = sorted({(min(c["M"], 128), min(c["N"], 128), c["K"], c.get("nkb", 1)) for c in COVERED})
    r_acc, r_out = G.measure_constants(shapes)
    print(f"measured on the host: accumulation {r_acc:.3f}, store {r_out:.4f}")
    assert r_acc == pytest.approx(G.MEASURED_ACC, abs=0.01) and r_out == pytest.approx(G.MEASURED_OUT, abs=0.0005)
    assert G.C_ACC == math.ceil(4.0 * G.MEASURED_ACC * 10.0) / 10.0
    assert G.MEASURED_OUT <= G.C_OUT == 1.0
    assert math.isclose(G.U_BF16, 2.0 ** -8) and math.isclose(G.U_FP32, 2.0 ** -24)
