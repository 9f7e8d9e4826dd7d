"""GEMM reference for the bound tests (tests/test_gemm_bounds.py): a float64 interpreter of the GEMM ABI, the per-element
magnitude that goes with it, and the two acceptance rules.  Plain helper module: no fixtures.

`expected()` takes the MatT / EpiT arguments exactly as `kern.gemm` receives them and evaluates what include/cenet_hip.h says the
call means (cenet_mat_t / cenet_epi_t, the text above `cenet_gemm_f32`), in float64 on the tensors' device:

    A(z, kb, m, k), B(z, kb, k, n)     mode 0: ptr[(z / nb_inner) sb + (z % nb_inner) sb2 + kb skb + r sr + c sc], with the
                                       reduction index split k -> (k / kinner) sk_outer + (k % kinner) (sc | sr) when kinner > 0;
                                       mode 1: the im2col gather, both `transposed` forms, zero outside the image
    acc(z, m, n) = sum over kb < nkb, k < K of A B           v = alpha acc
    atomic 1: C += v      atomic 2: C = v (fp32)      else: C = bscale[z | m / bscale_rows] act(v + bias[m | n]) + R
    C / R address: offset + (z / nb_inner) s?b + (z % nb_inner) s?b2 + m s?r + n s?c, or the col2im scatter (cmode 1)
    asum[m] += sum over kb, k of A(0, kb, m, k)

and returns the WHOLE destination buffer (the elements the call does not own keep their previous value), plus the magnitude: the
same formula with every operand replaced by its absolute value.  `expected_wgrad()` does the same for one cenet_wgrad_prob_t.
The formulas are written from the header, not from the kernels.

A MatT holds a raw pointer; `capture()` wraps kern.mat_plain / kern.mat_im2col for its duration so that the descriptor keeps
its tensor and element offset (as tools/gemm_replay.py does).

Acceptance rules.

EXACT regime (`assert_exact`): operands, bias, R and the previous C are small integers (bf16-exact values in [-4, 4]), alpha and
bscale powers of two.  Every product and every partial sum is then an integer multiple of a power of two below 2^24 in
magnitude (checked: max Mag < 2^24), so fp32 arithmetic is exact in ANY summation order, splits and atomics included, and the
kernel's output must EQUAL the float64 result rounded once to the output type.  No tolerance.  (Equality of finite floats is
equality of bits up to the sign of a zero, which no consumer can see.)  This is the regime that catches a dropped, doubled or
mis-indexed term at any K; it covers every linear epilogue.

BOUND regime (`assert_bound`): real-valued operands (normal; normal with a common offset so that terms do not cancel), needed
for `act` and for what integers cannot show: operand rounding, accumulation that is not fp32.
    |y - ref| <= C_OUT u_out |ref| + C_ACC 2^-24 sqrt(K nkb) Mag
u_out = 2^-8 (bf16 store: 8 significant bits, round to nearest) or 2^-24 (fp32 store / add): derived.

The constants are measured on the HOST, never on the kernels (`measure_constants()` below re-runs the measurement): a plain fp32
evaluation of the same call (torch fp32 matmul on the CPU, the K batches / K slices as separate fp32 products added in a
shuffled order to stand in for splits and atomics, the epilogue in fp32) against the float64 one, over the shapes of the
instance matrix in test_gemm_bounds.py (M and N clipped to 128, one batch: batches are independent contractions of one shape, and
the ratios depend on K and the number of K batches), in both operand regimes:
    accumulation: largest |y32 - ref| / (2^-24 sqrt(K nkb) Mag)                               measured 0.563  -> C_ACC = 2.3
    store:        largest (|bf16(y32) - ref| - |y32 - ref|) / (2^-8 |ref|)                    measured 0.9960 -> C_OUT = 1.0
C_ACC is the measured ratio with a factor of 4 (rounded up) for the summation order the device is free to choose.  C_OUT takes
no such factor: one round-to-nearest of the fp32 value is at most u_out of it whatever the order it was summed in (the distance of
that fp32 value from the reference is the accumulation term's business), and 1.0 is what separates round-to-nearest from
truncation (up to 2 u_out), which the mutation self-test holds the bound regime to.
These constants are not to be widened to make a kernel pass: a kernel that needs more is a finding."""
from __future__ import annotations

import contextlib
import math
from types import SimpleNamespace

import torch

U_BF16 = 2.0 ** -8
U_FP32 = 2.0 ** -24
MEASURED_ACC, MEASURED_OUT = 0.563, 0.9960  # what measure_constants() gives over the matrix's shapes (pinned by the tests)
C_OUT = 1.0   # measured 0.9960 (host, bf16 round-to-nearest of the fp32 evaluation); see the module docstring
C_ACC = 2.3   # measured 0.563 (host, fp32 evaluation against float64) x 4, rounded up
EXACT_LIMIT = 2.0 ** 24
_CHUNK = 1 << 25  # float64 elements of one operand gathered at a time
TILE = 64     # the failure report names the 64 x 64 output tile of the worst element
BF = torch.bfloat16
ACT_LIPSCHITZ = {"none": 1.0, "relu": 1.0, "lrelu": 1.0, "gelu": 1.13, "silu": 1.1, "sigmoid": 0.25}


# ---- descriptors that keep their tensors -------------------------------------------------------------------------------------
@contextlib.contextmanager
def capture():
    """kern.mat_plain / kern.mat_im2col return descriptors that remember their tensor (`_t`) and element offset (`_off`)"""
    from cenet_amd import kern
    orig_plain, orig_im = kern.mat_plain, kern.mat_im2col

    def plain(t, *a, **k):
        m = orig_plain(t, *a, **k)
        off = k.get("offset", a[5] if len(a) > 5 else 0)
        m._t, m._off = t, off
        return m

    def im2col(t, *a, **k):
        m = orig_im(t, *a, **k)
        m._t, m._off = t, k.get("offset", 0)
        return m

    kern.mat_plain, kern.mat_im2col = plain, im2col
    try:
        yield
    finally:
        kern.mat_plain, kern.mat_im2col = orig_plain, orig_im


def storage(t, extra: int = 0):
    """(flat view of the whole storage behind a tensor-like, element index of its first element + extra).  Tensor-likes: tensors,
    kern.Ptr (.t / .off) and the offset views of cenet_amd.ops (._t / ._off)."""
    while not isinstance(t, torch.Tensor):
        if hasattr(t, "_t"):
            t, extra = t._t, extra + t._off
        else:
            t, extra = t.t, extra + t.off
    flat = torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())
    return flat, t.storage_offset() + extra


def _vec(t, n):
    """float64 copy of the first n elements of a tensor-like"""
    if isinstance(t, torch.Tensor):
        return t.reshape(-1)[:n].double()
    flat, base = storage(t)
    return flat[base:base + n].double()


def _ar(n, dev):
    return torch.arange(n, device=dev, dtype=torch.int64)


def _batch_off(z, nb_inner, sb, sb2):
    return (z // nb_inner) * sb + (z % nb_inner) * sb2


def _operand(m, z, kb0, kb1, rows, cols, k_is_col, nb_inner):
    """float64 [kb1 - kb0, rows, cols] of the logical operand for batch z (zeros where an im2col tap leaves the image)"""
    flat, base = storage(m._t, m._off)
    dev = flat.device
    r, c, kb = _ar(rows, dev)[None, :, None], _ar(cols, dev)[None, None, :], _ar(kb1 - kb0, dev)[:, None, None] + kb0
    off = base + _batch_off(z, nb_inner, m.sb, m.sb2) + kb * m.skb
    if m.mode == 0:
        if m.kinner > 0:
            k, ks = (c, m.sc) if k_is_col else (r, m.sr)
            kaddr = (k // m.kinner) * m.sk_outer + (k % m.kinner) * ks
            idx = off + (r * m.sr + kaddr if k_is_col else kaddr + c * m.sc)
        else:
            idx = off + r * m.sr + c * m.sc
        return flat[idx].double()
    e, p = (r, c) if m.patch_is_row else (c, r)
    ci, ky, kx = e // (m.KH * m.KW), (e // m.KW) % m.KH, e % m.KW
    py, px = p // m.Pw, p % m.Pw
    if not m.transposed:
        iy, ix = py * m.stride - m.pad + ky * m.dil, px * m.stride - m.pad + kx * m.dil
        ok = torch.ones_like(iy, dtype=torch.bool)
    else:
        ny, nx = py + m.pad - ky * m.dil, px + m.pad - kx * m.dil
        ok = (ny % m.stride == 0) & (nx % m.stride == 0) & (ny >= 0) & (nx >= 0)
        iy, ix = ny // m.stride, nx // m.stride
    ok = ok & (iy >= 0) & (iy < m.Hs) & (ix >= 0) & (ix < m.Ws)
    idx = off + ci * m.sci + iy.clamp(0, m.Hs - 1) * m.sy + ix.clamp(0, m.Ws - 1) * m.sx
    idx, ok = torch.broadcast_tensors(idx, ok)
    v = flat[idx].double()
    return torch.where(ok, v, torch.zeros_like(v))


def _act64(v, act, slope):
    if act == "none":
        return v
    if act == "relu":
        return v.clamp_min(0.0)
    if act == "lrelu":
        return torch.where(v > 0, v, v * slope)
    if act == "gelu":
        return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))
    if act == "silu":
        return v * torch.sigmoid(v)
    if act == "sigmoid":
        return torch.sigmoid(v)
    raise ValueError(act)


def expected(A, B, Cout, M, N, K, *, scr, scc, scb=0, nbatch=1, nkb=1, splits=1, bias=None, bias_on_row=False, act="none",
             slope=0.0, bscale=None, R=None, srb=0, srr=0, src=0, atomic=False, alpha=1.0, c_offset=0, r_offset=0, nb_inner=1,
             scb2=0, srb2=0, col2im=None, bscale_rows=0, asum=None):
    """What kern.gemm(A, B, Cout, M, N, K, **same keywords) must leave in Cout's storage, given its contents NOW (call this before
    the launch, or on a snapshot, when the epilogue is atomic or strided).  Returns a namespace:
      C, Mag    float64, flat over the whole storage of Cout: expected value / magnitude (0 where the call does not write)
      own       bool, flat: the elements the call writes
      prev_raw  the storage as it is now, in its own type (what the elements outside `own` must still hold, bit for bit)
      idx       int64 [nbatch, M, N]: flat address of output (z, m, n), -1 where a col2im tap falls outside the image
      asum, asum_mag   float64 [M] or None
      out_dtype, u_out, K_tot"""
    atomic = int(atomic)
    cflat, cbase = storage(Cout, c_offset)
    dev = cflat.device
    C64, Mag = cflat.double().clone(), torch.zeros(cflat.numel(), dtype=torch.float64, device=dev)
    prev = C64.clone()
    own = torch.zeros(cflat.numel(), dtype=torch.bool, device=dev)
    idx_all = torch.empty(nbatch, M, N, dtype=torch.int64, device=dev)
    m_i, n_i = _ar(M, dev)[:, None], _ar(N, dev)[None, :]
    if R is not None:
        rflat, rbase = storage(R, r_offset)
    b64 = _vec(bias, M if bias_on_row else N) if bias is not None else None
    s64 = _vec(bscale, -(-M // bscale_rows) if bscale_rows > 0 else nbatch) if bscale is not None else None
    a_sum = a_sum_mag = None
    lip = ACT_LIPSCHITZ[act]
    for z in range(nbatch):
        acc = torch.zeros(M, N, dtype=torch.float64, device=dev)
        mag = torch.zeros_like(acc)
        step = max(1, _CHUNK // max(1, K * max(M, N)))
        for kb0 in range(0, nkb, step):
            kb1 = min(nkb, kb0 + step)
            a = _operand(A, z, kb0, kb1, M, K, True, nb_inner)   # [kb, M, K]
            b = _operand(B, z, kb0, kb1, K, N, False, nb_inner)  # [kb, K, N]
            acc += torch.bmm(a, b).sum(0)
            mag += torch.bmm(a.abs(), b.abs()).sum(0)
            if asum is not None and z == 0:
                if a_sum is None:
                    a_sum = _vec(asum, M).clone()
                    a_sum_mag = a_sum.abs()
                a_sum += a.sum((0, 2))
                a_sum_mag += a.abs().sum((0, 2))
            del a, b
        v, vm = alpha * acc, abs(alpha) * mag
        zoff = _batch_off(z, nb_inner, scb, scb2)
        if col2im is None:
            idx = cbase + zoff + m_i * scr + n_i * scc
            ok = None
        else:
            q = SimpleNamespace(**col2im)
            ci, ky, kx = m_i // (q.KH * q.KW), (m_i // q.KW) % q.KH, m_i % q.KW
            py, px = n_i // q.Pw, n_i % q.Pw
            oy, ox = py * q.stride - q.pad + ky, px * q.stride - q.pad + kx
            ok = (oy >= 0) & (oy < q.Hs) & (ox >= 0) & (ox < q.Ws)
            idx = cbase + zoff + ci * q.sci + oy * q.sy + ox * q.sx
            idx = torch.where(ok, idx, torch.full_like(idx, -1))
        idx_all[z] = idx
        if not atomic:
            if b64 is not None:
                bb = b64[:M, None] if bias_on_row else b64[None, :N]
                v, vm = v + bb, vm + bb.abs()
            v, vm = _act64(v, act, slope), lip * vm
            if s64 is not None:
                sc = s64[m_i // bscale_rows] if bscale_rows > 0 else s64[z]
                v, vm = sc * v, sc.abs() * vm
            if R is not None:
                r = rflat[rbase + _batch_off(z, nb_inner, srb, srb2) + m_i * srr + n_i * src].double()
                v, vm = v + r, vm + r.abs()
        sel = slice(None) if ok is None else ok
        fi, fv, fm = idx[sel].reshape(-1), v[sel].reshape(-1), vm[sel].reshape(-1)
        if atomic == 1:
            C64.index_add_(0, fi, fv)
            Mag.index_add_(0, fi, fm)
        else:
            C64[fi], Mag[fi] = fv, fm
        own[fi] = True
    if atomic == 1:
        Mag = torch.where(own, Mag + prev.abs(), Mag)
    out_dtype = cflat.dtype
    if asum is not None:  # a bias gradient in the same storage as C (slots of one gradient arena) is the call's to write as well
        sflat, sbase = storage(asum)
        if sflat.data_ptr() == cflat.data_ptr() and sflat.dtype == cflat.dtype:
            other = torch.zeros_like(own)  # (checked on their own: assert_vec_bound / assert_vec_exact)
            other[sbase:sbase + M] = True
        else:
            other = None
    else:
        other = None
    return SimpleNamespace(C=C64, Mag=Mag, own=own, other=other, prev_raw=cflat.clone(), idx=idx_all, asum=a_sum, asum_mag=a_sum_mag, out_dtype=out_dtype,
                           u_out=U_BF16 if out_dtype == BF else U_FP32, K_tot=K * nkb, M=M, N=N, nbatch=nbatch)


def expected_wgrad(A, B, Cprev, asum_prev, lda, ldb, skbA, skbB, M, N, K, nkb, kfast):
    """One cenet_wgrad_prob_t (include/cenet_hip.h): C[m, n] += sum over kb, k of A(m, k) B(k, n), asum[m] += sum of A(m, k), with
    A(m, k) = kfast ? A[kb skbA + m lda + k] : A[kb skbA + k lda + m] and B likewise; A, B tensors (bf16), Cprev [M, N] fp32 and
    asum_prev [M] (or None) hold the destinations' contents before the call.  Returns C, Mag, asum, asum_mag in float64."""
    aflat, abase = storage(A)
    bflat, bbase = storage(B)
    dev = aflat.device
    kb, m, n = _ar(nkb, dev)[:, None, None], _ar(M, dev), _ar(N, dev)
    k = _ar(K, dev)
    if kfast:
        ia = abase + kb * skbA + m[None, :, None] * lda + k[None, None, :]
        ib = bbase + kb * skbB + n[None, None, :] * ldb + k[None, :, None]
    else:
        ia = abase + kb * skbA + k[None, None, :] * lda + m[None, :, None]
        ib = bbase + kb * skbB + k[None, :, None] * ldb + n[None, None, :]
    a, b = aflat[ia].double(), bflat[ib].double()
    r = SimpleNamespace(C=Cprev.double() + torch.bmm(a, b).sum(0), Mag=Cprev.double().abs() + torch.bmm(a.abs(), b.abs()).sum(0),
                        asum=None, asum_mag=None, K_tot=K * nkb)
    if asum_prev is not None:
        r.asum = asum_prev.double() + a.sum((0, 2))
        r.asum_mag = asum_prev.double().abs() + a.abs().sum((0, 2))
    return r


# ---- acceptance rules --------------------------------------------------------------------------------------------------------
def round_once(x64, dtype):
    """float64 -> output type with ONE rounding to nearest even.  torch converts float64 -> bf16 through fp32; that is a single
    rounding when the value is exact in fp32, which the exact regime guarantees and this asserts."""
    f = x64.float()
    if dtype != torch.float32:
        assert bool((f.double() == x64).all()), "value not exact in fp32: float64 -> bf16 would round twice"
    return f.to(dtype)


def _where(exp, flat):
    """(z, m, n) of a flat destination address, for the failure report"""
    hit = (exp.idx == flat).nonzero()
    return tuple(int(v) for v in hit[0]) if len(hit) else None


def _locate(exp, flat, what):
    pos = _where(exp, flat) if getattr(exp, "idx", None) is not None else None
    if pos is None:
        return f"{what}: buffer element {flat} (outside the call's footprint)"
    z, m, n = pos
    return (f"{what}: output (batch {z}, row {m}, column {n}), {TILE} x {TILE} tile ({m // TILE}, {n // TILE}) of "
            f"({-(-exp.M // TILE)}, {-(-exp.N // TILE)})")


def assert_exact(got, exp, what=""):
    """got: the destination buffer after the launch (any shape over the whole storage).  Every element must equal the float64
    expectation rounded once to the output type: the call's own elements AND everything around them."""
    got = storage(got)[0]
    assert float(exp.Mag.max()) < EXACT_LIMIT, f"{what}: magnitude {float(exp.Mag.max())} is outside the exact regime"
    want = round_once(exp.C, exp.out_dtype)
    bad = ~((got == want) & torch.isfinite(got))
    if bool(bad.any()):
        flat = int(bad.nonzero()[0])
        own_bad = int((bad & exp.own).sum())
        raise AssertionError(f"{_locate(exp, flat, what)}: got {float(got[flat])!r}, expected {float(want[flat])!r}; "
                             f"{own_bad} wrong outputs, {int(bad.sum()) - own_bad} elements changed outside the footprint")


def assert_vec_exact(got, want64, mag, what=""):
    assert float(mag.max()) < EXACT_LIMIT, what
    got = got.detach().double().reshape(-1)
    bad = ~((got == want64.reshape(-1)) & torch.isfinite(got))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: element {i}: got {float(got[i])!r}, expected {float(want64.reshape(-1)[i])!r} "
                             f"({int(bad.sum())} of {bad.numel()} wrong)")


def bound_of(ref, mag, u_out, K_tot, c_out=C_OUT, c_acc=C_ACC):
    return c_out * u_out * ref.abs() + c_acc * U_FP32 * math.sqrt(K_tot) * mag


def assert_bound(got, exp, what=""):
    """|got - ref| <= C_OUT u_out |ref| + C_ACC 2^-24 sqrt(K_tot) Mag on the call's own elements; everything else unchanged.
    Returns the worst |err| / bound."""
    got = storage(got)[0]
    g64 = got.double()
    bits = torch.int16 if got.element_size() == 2 else torch.int32  # (bits: a workspace may hold NaNs around the footprint)
    outside = ~exp.own & (got.view(bits) != exp.prev_raw.view(bits))
    if getattr(exp, "other", None) is not None:
        outside &= ~exp.other
    if bool(outside.any()):
        flat = int(outside.nonzero()[0])
        raise AssertionError(f"{what}: buffer element {flat} outside the footprint changed: {float(got[flat])!r} "
                             f"(was {float(exp.C[flat])!r}); {int(outside.sum())} such elements")
    err = (g64 - exp.C).abs()
    err = torch.where(torch.isfinite(g64), err, torch.full_like(err, math.inf))
    bound = bound_of(exp.C, exp.Mag, exp.u_out, exp.K_tot)
    ratio = torch.where(exp.own, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max())
    if worst > 1.0:
        flat = int(torch.argmax(ratio))
        raise AssertionError(f"{_locate(exp, flat, what)}: got {float(got[flat]):.9g}, reference {float(exp.C[flat]):.9g}, "
                             f"|err| = {float(err[flat]):.3g} = {worst:.3g} x bound (u_out = {exp.u_out:.3g}, K_tot = {exp.K_tot}, "
                             f"Mag = {float(exp.Mag[flat]):.3g}); {int((ratio > 1).sum())} of {int(exp.own.sum())} outputs outside")
    return worst


def assert_vec_bound(got, ref, mag, K_tot, what="", ncols=0):
    """fp32 accumulators outside the C buffer (asum, grouped C): |got - ref| <= C_OUT 2^-24 |ref| + C_ACC 2^-24 sqrt(K_tot) Mag.
    ncols: row length of a matrix destination, for the failure report."""
    g64 = got.detach().double().reshape(ref.shape)
    err = (g64 - ref).abs()
    err = torch.where(torch.isfinite(g64), err, torch.full_like(err, math.inf))
    ratio = err / bound_of(ref, mag, U_FP32, K_tot).clamp_min(1e-300)
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(torch.argmax(ratio))
        if ncols:
            what = f"{what}: output (row {i // ncols}, column {i % ncols}), {TILE} x {TILE} tile ({i // ncols // TILE}, {i % ncols // TILE})"
        raise AssertionError(f"{what}: element {i}: got {float(g64.reshape(-1)[i]):.9g}, reference {float(ref.reshape(-1)[i]):.9g}, "
                             f"{worst:.3g} x bound (K_tot = {K_tot})")
    return worst


# ---- replay: every GEMM launch of real code checked as it happens ----------------------------------------------------------
def ptr_view(ptr, n, dtype, device):
    """n elements of `dtype` (fp32 / bf16) at a raw address as a tensor that shares the memory (the grouped entry takes addresses)"""
    f32 = dtype == torch.float32
    if device.type == "cpu":
        import ctypes
        arr = ((ctypes.c_float if f32 else ctypes.c_int16) * n).from_address(ptr)
        t = torch.frombuffer(arr, dtype=torch.float32 if f32 else torch.int16)
    else:
        class _Mem:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4" if f32 else "<i2", "data": (ptr, False), "version": 2}
        t = torch.as_tensor(_Mem(), device=device)
    return t if f32 else t.view(BF)


def group_name(bm, bn, ns):
    """how the census names a tile class of the grouped weight-gradient plan (cenet_wgrad_group_plan)"""
    return f"wgrad_group<{bm}, {bn}, {ns}>"


class Replay:
    """Context manager: for its duration kern.gemm and kern.wgrad_group check EVERY call against the interpreter in the bound
    regime, with the operands as they occur (kern.mat_plain / kern.mat_im2col keep their tensors, `capture()`).  The destination is
    read before the launch (atomic and strided epilogues start from it), the device is idle around each launch, the float64
    references are dropped call by call.  Nothing raises inside the replayed code: failures are collected (`failures`: shape key,
    instance name, worst element and its 64 x 64 tile), `seen` maps instance name -> [calls, worst |err| / bound]."""

    def __init__(self):
        self.seen, self.failures, self.calls = {}, [], 0

    def _note(self, name, ratio):
        e = self.seen.setdefault(name, [0, 0.0])
        e[0] += 1
        e[1] = max(e[1], ratio)

    @staticmethod
    def _idle(dev):
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)

    def _check(self, name, key, fn):
        try:
            r = fn()
        except AssertionError as e:
            self.failures.append(f"[{key}] {name}: {e}")
            r = math.inf
        self._note(name, r)

    def __enter__(self):
        from cenet_amd import kern
        self._kern, self._gemm, self._group = kern, kern.gemm, kern.wgrad_group
        self._cap = capture()
        self._cap.__enter__()
        kern.gemm, kern.wgrad_group = self.gemm, self.wgrad_group
        return self

    def __exit__(self, *exc):
        self._kern.gemm, self._kern.wgrad_group = self._gemm, self._group
        self._cap.__exit__(*exc)
        return False

    def gemm(self, A, B, Cout, M, N, K, **kw):
        dev = storage(Cout)[0].device
        self._idle(dev)
        exp = expected(A, B, Cout, M, N, K, **kw)
        self._gemm(A, B, Cout, M, N, K, **kw)
        self._idle(dev)
        self.calls += 1
        name = self._kern.last_gemm_kernel()
        key = (f"M={M} N={N} K={K} nbatch={kw.get('nbatch', 1)} nb_inner={kw.get('nb_inner', 1)} nkb={kw.get('nkb', 1)} "
               f"{'im2col' if B.mode else 'plain'} a{A.kfast}b{B.kfast} atomic={int(kw.get('atomic', 0))}"
               f"{' col2im' if kw.get('col2im') else ''}{' act=' + kw['act'] if kw.get('act', 'none') != 'none' else ''}")

        def check():
            r = assert_bound(Cout, exp, "C")
            if exp.asum is not None:
                r = max(r, assert_vec_bound(_vec(kw["asum"], M), exp.asum, exp.asum_mag, exp.K_tot, "asum"))
            return r
        self._check(name, key, check)
        del exp

    def wgrad_group(self, probs, device, *a, **k):
        device = torch.device(device)
        self._idle(device)
        dests = {}
        for t, (_, bm, bn, ns) in zip(probs, self._kern.wgrad_group_plan(probs)):
            pa, pb, pc, ps, lda, ldb, skbA, skbB, M, N, K, nkb, kf = t[:13]

            def extent(ld, skb, rows):
                return (nkb - 1) * skb + ((rows - 1) * ld + K if kf else (K - 1) * ld + rows)
            d = dests.get(pc)
            if d is None:
                c = ptr_view(pc, M * N, torch.float32, device)
                v = ptr_view(ps, M, torch.float32, device) if ps else None
                d = dests[pc] = SimpleNamespace(c=c, v=v, c0=c.clone(), v0=v.clone() if v is not None else None, probs=[], M=M, N=N)
            d.probs.append((ptr_view(pa, extent(lda, skbA, M), BF, device), ptr_view(pb, extent(ldb, skbB, N), BF, device),
                            (lda, ldb, skbA, skbB, M, N, K, nkb, kf), group_name(bm, bn, ns)))
        need = self._group(probs, device, *a, **k)
        self._idle(device)
        self.calls += 1
        for d in dests.values():
            e = None
            for pa, pb, args, name in d.probs:  # problems that share a destination: each starts from the one before
                e1 = expected_wgrad(pa, pb, d.c0.view(d.M, d.N) if e is None else e.C, d.v0 if e is None else e.asum, *args)
                if e is not None:
                    e1.Mag, e1.K_tot = e1.Mag + e.Mag, e1.K_tot + e.K_tot
                    if e1.asum is not None:
                        e1.asum_mag = e1.asum_mag + e.asum_mag
                e = e1
            key = " + ".join("M={4} N={5} K={6} nkb={7} kfast={8}".format(*p[2]) for p in d.probs)

            def check(e=e, d=d):
                r = assert_vec_bound(d.c, e.C, e.Mag, e.K_tot, "C", ncols=d.N)
                if e.asum is not None:
                    r = max(r, assert_vec_bound(d.v, e.asum, e.asum_mag, e.K_tot, "asum"))
                return r
            for name in {p[3] for p in d.probs}:
                self._check(name, key, check)
            del e
        return need

    def table(self):
        return [f"{n}  x{c}  worst |err| / bound = {r:.3f}" for n, (c, r) in sorted(self.seen.items())]


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def ints(shape, g, lo=-4, hi=4):
    """small integers as fp32 (exact in bf16)"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def reals(shape, g, offset=0.0):
    return torch.randn(*shape, generator=g) + offset


# ---- host measurement of the constants ---------------------------------------------------------------------------------------
def measure_constants(shapes, seed=0):
    """The measurement the module docstring quotes: fp32 evaluation on the CPU against float64, over (M, N, K, nkb) shapes, in the
    two operand regimes (normal; normal + 1).  The K batches are separate fp32 products added in a shuffled order (splits /
    atomics).  Returns (accumulation ratio, store ratio)."""
    g = torch.Generator().manual_seed(seed)
    r_acc = r_out = 0.0
    for (M, N, K, nkb) in shapes:
        for off in (0.0, 1.0):
            a = reals((nkb, M, K), g, off).to(BF).float()
            b = reals((nkb, K, N), g, off).to(BF).float()
            bias = reals((N,), g)
            ref = torch.bmm(a.double(), b.double()).sum(0) + bias.double()
            mag = torch.bmm(a.double().abs(), b.double().abs()).sum(0) + bias.double().abs()
            parts = torch.bmm(a, b)
            y = torch.zeros(M, N)
            for i in torch.randperm(nkb, generator=g).tolist():
                y = y + parts[i]
            y = y + bias
            e32 = (y.double() - ref).abs()
            r_acc = max(r_acc, float((e32 / (U_FP32 * math.sqrt(K * nkb) * mag)).max()))
            e16 = (y.to(BF).double() - ref).abs()
            r_out = max(r_out, float(((e16 - e32) / (U_BF16 * ref.abs()).clamp_min(1e-300)).max()))
    return r_acc, r_out
