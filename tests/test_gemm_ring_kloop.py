"""The K loop of the LDS-DMA ring GEMM (csrc/gemm_ring.h, gemm_group.hip) at the smallest shapes that can still break a ring,
held to the float64 interpreter and the acceptance rules of tests/gemm_ref.py exactly as tests/test_gemm_bounds.py holds the
instances (run_case: exact regime on integer operands, bound regime on real ones, NaN-surrounded operands, sentinel-surrounded
destination, the instance name asserted through kern.last_gemm_kernel()).

Since round 8 the row-fast fragments of these loops are read by inline asm, so that the compiler no longer drains the ring's
tiles in flight in front of them; what orders a read behind its tile is then only the loop's own counted vmcnt + barrier, and the
first use of a fragment behind its read only ring_frag_landed().  A ring that is one wait short shows at: fewer K-steps than slots,
as many, one more (K = 64 .. 320 on the 4-slot 64 x 64 tile); K tails (a zero-filled chunk, a masked chunk); clamped rows; the
hand-fetched tail chunk of unaligned planes; every batch form; K batches; the split-K atomic epilogue (which reuses the ring as
its strip); all four orientations (k-fast = ds_read_b128, row-fast = the transposing read).
`sim` = the kernel sources on the host SIMT checker (CPU); `hip` = the gfx950 library (marker gpu)."""
import pytest
import torch

import gemm_ref as G
from backend import dev  # noqa: F401
from cenet_amd import kern
from test_gemm_bounds import BF, ORIENT, SENTINEL, _dest, _embed, _group_problem, _sync, run_case, tf


def name(akf, bkf, swap):
    return f"gemm_ring_kernel<{tf(akf)}, {tf(bkf)}, 64, 64, 4, {tf(swap)}>"


def _case(M, N, K, akf=1, bkf=0, store="row", **c):
    c.update(M=M, N=N, K=K, akf=akf, bkf=bkf, store=store, name=name(akf, bkf, store == "row" and not c.get("atomic")))
    return c


def _both(dev_, c):
    run_case(dev_, c, "exact")
    if not c.get("atomic"):
        run_case(dev_, c, "offset")


@pytest.mark.parametrize("K", [64, 128, 192, 320])
def test_ksteps_against_slots(dev, K):
    """1, 2, 3 and 5 K-steps on the 4-slot ring: the prologue fills fewer slots than it has, all it keeps in flight, and the loop
    refills a slot; swap epilogue with bias and residual; M and N ragged"""
    _both(dev, _case(65, 130, K))


@pytest.mark.parametrize("K", [72, 100])
def test_k_tail(dev, K):
    """K = 72: the tail K-step holds one chunk of data and seven zero-filled ones; K = 100: not a multiple of 8, the last chunk of a
    k-fast row runs into the next row and is masked in the fragment"""
    _both(dev, _case(65, 48, K))
    _both(dev, _case(65, 48, K, akf=0, bkf=1, store="col"))


@pytest.mark.parametrize("M,N", [(48, 65), (65, 130), (130, 48)])
def test_edges(dev, M, N):
    """partial tiles in M and N: rows beyond the operand are clamped, their products never stored"""
    _both(dev, _case(M, N, 136))


@pytest.mark.parametrize("akf,bkf", ORIENT)
@pytest.mark.parametrize("store", ["row", "col"])
def test_orientations(dev, akf, bkf, store):
    _both(dev, _case(65, 130, 200, akf=akf, bkf=bkf, store=store))


def test_k_blocked(dev):
    """nkb = 3: the loop runs over (K batch, K tile) pairs, each batch with its own tail"""
    _both(dev, _case(65, 48, 72, nkb=3))


def test_split_k_atomic(dev):
    """K = 4096 on one 64 x 64 tile: the split count is the dispatcher's; every split runs the ring over its chunk of K tiles and adds
    its tile through the strip that reuses the ring's memory; row sums of A ride along"""
    _both(dev, _case(64, 64, 4096, atomic=1, splits=8, asum=True))


@pytest.mark.parametrize("ld", [196, 49])
def test_unaligned_row_fast_planes(dev, ld):
    """per-image planes B [3][K][ld] with N = ld: pitch and plane stride are not multiples of 8 elements, so chunks start at
    2-byte aligned addresses and the last chunk of the last plane is fetched by hand (ring_unal, ring_fix_tail_chunk)"""
    g = torch.Generator().manual_seed(29)
    M, N, K, nb = 72, ld, 136, 3
    for regime in ("exact", "offset"):
        vals = (lambda s: G.ints(s, g)) if regime == "exact" else (lambda s: G.reals(s, g, 1.0).to(BF).float())
        with G.capture():
            a = vals((1, M, K))
            abuf, lead, pitch, mat = _embed(a, BF, dev, True)
            A = kern.mat_plain(abuf, pitch, 1, kfast=1, offset=lead)
            # planes packed with no padding at all; NaN in front, and nothing behind the last element but the buffer's end
            bbuf = torch.cat([torch.full((3,), float("nan")), vals((nb * K * N,))]).to(BF).to(dev)
            Bm = kern.mat_plain(bbuf, N, 1, sb=K * N, kfast=0, offset=3)
        Cbuf, kw = _dest(M, N, nb, "row", BF, dev, False, SENTINEL)
        kw.update(nbatch=nb, alpha=2.0, bias=vals((N,)).to(dev))
        exp = G.expected(A, Bm, Cbuf, M, N, K, **kw)
        kern.gemm(A, Bm, Cbuf, M, N, K, **kw)
        _sync(dev)
        assert kern.last_gemm_kernel() == name(1, 0, True)
        (G.assert_exact if regime == "exact" else G.assert_bound)(Cbuf, exp, f"ld {ld} [{regime}]")


def test_two_level_batch(dev):
    """nbatch 6 with nb_inner 2: batch z -> (z / 2, z % 2) with independent outer and inner strides on A, B, C and R"""
    g = torch.Generator().manual_seed(31)
    M, N, K, Bo, Hh = 65, 72, 200, 3, 2
    with G.capture():
        a, b = G.ints((Hh * Bo, M, K), g), G.ints((Bo * Hh, K, N), g)
        abuf, la, pa, ma = _embed(a, BF, dev, True)
        bbuf, lb, pb, mb = _embed(b, BF, dev, True)
        A = kern.mat_plain(abuf, pa, 1, sb=ma, sb2=Bo * ma, kfast=1, offset=la)        # laid out [H, B]
        Bm = kern.mat_plain(bbuf, pb, 1, sb=Hh * mb, sb2=mb, kfast=0, offset=lb)      # laid out [B, H]
    Cbuf, kw = _dest(M, N, Bo * Hh, "row", BF, dev, True, SENTINEL)
    mat = kw.pop("scb")
    Rbuf, lead, pitch, rmat = _embed(G.ints((Bo * Hh, M, N), g), BF, dev, True)
    kw.update(scb=mat, scb2=Bo * mat, nbatch=Bo * Hh, nb_inner=Hh, R=Rbuf, r_offset=lead, srb=Hh * rmat, srb2=rmat, srr=pitch, src=1,
              bias=G.ints((N,), g).to(dev), alpha=2.0)
    exp = G.expected(A, Bm, Cbuf, M, N, K, **kw)
    kern.gemm(A, Bm, Cbuf, M, N, K, **kw)
    _sync(dev)
    assert kern.last_gemm_kernel() == name(1, 0, True)
    G.assert_exact(Cbuf, exp, "nb_inner")


@pytest.mark.parametrize("kind", ["lin", "conv"])
def test_grouped_two_problems_one_launch(dev, kind):
    """gemm_group_kernel: two problems of different shape in ONE launch, one of them a single 64 x 64 tile of a single K-step, the
    other ragged in M, N and K; 'lin' = row-fast operands (the transposing read), 'conv' = k-fast"""
    g = torch.Generator().manual_seed(37)
    nkb = 2 if kind == "conv" else 1
    probs = [_group_problem(g, dev, kind, 64, 64, 64, nkb=nkb), _group_problem(g, dev, kind, 72, 100, 330, nkb=nkb)]
    plan = kern.wgrad_group_plan([p["item"] for p in probs])
    assert len({li for li, *_ in plan}) == 1 and {(bm, bn, ns) for _, bm, bn, ns in plan} == {(64, 64, 4)}, plan
    exps = [G.expected_wgrad(p["a"], p["b"], p["dW"], p["db"], *p["args"]) for p in probs]
    kern.wgrad_group([p["item"] for p in probs], dev)
    _sync(dev)
    for p, e in zip(probs, exps):
        what = f"grouped {kind} {p['args'][4:]}"
        G.assert_vec_exact(p["dW"], e.C, e.Mag, what + " C")
        G.assert_vec_exact(p["db"], e.asum, e.asum_mag, what + " asum")
