"""Thin, autograd-free Python bindings over the C ABI in include/cenet_hip.h.

Every function here launches hand-written HIP kernels on the current torch stream with raw data pointers.
Tensors must live on the GPU (the only exception is the tests' host-side SIMT checker, which swaps the library handle — see
cenet_amd/_lib.py) and have exactly the element type the header declares for the parameter they are passed as: `_launch` /
`_call` hold every tensor argument to the prototype of the entry point they call (a bf16 `gamma`, an fp32 residual beside bf16
activations, a float64 tensor where the header says `float*` raise a TypeError naming the parameter); `_chk` remains for the
tensors whose pointers travel inside argument structs and pointer arrays.
Activation tensors are fp32 (parity mode) or bf16 (throughput mode); a call whose tensor arguments include a bf16 tensor goes
to the `_bf16` twin of the entry point (include/cenet_hip.h), in which every ACTIVATION pointer is bf16 while parameters,
statistics and parameter gradients stay fp32.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from ._lib import AttnT, DiffAttnT, EpiT, MatT, WgradProbT  # noqa: F401 (the ABI structs, generated from the header)

ACT = {"none": 0, "relu": 1, "lrelu": 2, "gelu": 3, "silu": 4, "sigmoid": 5}


def _chk(*ts):
    """the check of tensors that reach the library inside an argument struct or an array of pointers, where the header's
    parameter types cannot speak for them (everything handed to _call / _launch directly is held to the header there)"""
    for t in ts:
        if t is None:
            continue
        if isinstance(t, Ptr):
            t = t.t
        if t.dtype not in (torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8):
            raise TypeError(f"cenet_amd kernels take fp32 / bf16 tensors (int32 / int64 / uint8 for indices and masks); "
                            f"got {t.dtype}")
        if not t.is_cuda and not _lib.is_hostsim():
            raise RuntimeError("cenet_amd kernels run on the MI355X only: tensor is not on a CUDA/HIP device "
                               "(there is no CPU fallback)")


def P(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """the current torch stream as a raw hipStream_t (this runs once per kernel launch: keep it cheap)"""
    if _lib.is_hostsim():
        return 0
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------
# GEMM / implicit GEMM
# ------------------------------------------------------------------------------------------------
BF16 = torch.bfloat16


def is_bf16(t) -> bool:
    return t is not None and t.dtype == BF16


def esz(t) -> int:
    """bytes per element of a tensor-like (tensors, ops._OffsetView)"""
    return 2 if t.dtype == BF16 else 4


def mat_plain(t: torch.Tensor, sr: int, sc: int, sb: int = 0, skb: int = 0, kfast: int = 0, offset: int = 0,
              sb2: int = 0, kinner: int = 0, sk_outer: int = 0) -> MatT:
    m = MatT()
    m.bf16 = t.dtype == BF16  # python-side attribute: picks cenet_gemm_bf16
    m.ptr = t.data_ptr() + esz(t) * offset
    m.sb, m.sb2, m.skb, m.sr, m.sc = sb, sb2, skb, sr, sc
    m.kinner, m.sk_outer = kinner, sk_outer
    m.mode, m.kfast = 0, kfast
    return m


def mat_im2col(t: torch.Tensor, *, sb: int, skb: int, sci: int, sy: int, sx: int, KH: int, KW: int, Pw: int,
               Hs: int, Ws: int, stride: int, pad: int, dil: int, patch_is_row: int, transposed: int,
               kfast: int, offset: int = 0) -> MatT:
    m = MatT()
    m.bf16 = t.dtype == BF16
    m.ptr = t.data_ptr() + esz(t) * offset
    m.sb, m.skb, m.sr, m.sc = sb, skb, 0, 0
    m.mode, m.kfast = 1, kfast
    m.patch_is_row, m.transposed = patch_is_row, transposed
    m.KH, m.KW, m.Pw, m.Hs, m.Ws = KH, KW, Pw, Hs, Ws
    m.stride, m.pad, m.dil = stride, pad, dil
    m.sci, m.sy, m.sx = sci, sy, sx
    return m


def pick_splits(M: int, N: int, nbatch: int, iters: int, target_blocks: int = 1024) -> int:
    blocks = ((M + 63) // 64) * ((N + 63) // 64) * nbatch
    if blocks >= target_blocks or iters <= 4:
        return 1
    return max(1, min(iters // 2, (target_blocks + blocks - 1) // blocks, 256))


def gemm(A: MatT, B: MatT, Cout: torch.Tensor, M: int, N: int, K: int, *, scr: int, scc: int, scb: int = 0,
         nbatch: int = 1, nkb: int = 1, splits: int = 1, bias: Optional[torch.Tensor] = None, bias_on_row: bool = False,
         act: str = "none", slope: float = 0.0, bscale: Optional[torch.Tensor] = None,
         R: Optional[torch.Tensor] = None, srb: int = 0, srr: int = 0, src: int = 0, atomic: bool = False,
         alpha: float = 1.0, c_offset: int = 0, r_offset: int = 0, nb_inner: int = 1, scb2: int = 0, srb2: int = 0,
         col2im: Optional[dict] = None, bscale_rows: int = 0, asum: Optional[torch.Tensor] = None):
    """asum (atomic contractions, nbatch == 1): fp32 vector that receives asum[m] += sum_k A[m, k] — the bias gradient riding
    in the weight-gradient pass"""
    _chk(Cout, bias, bscale, R, asum)
    if A.bf16 != B.bf16:
        raise TypeError("cenet_gemm: A and B must have the same element type (fp32 or bf16)")
    want = torch.float32 if (atomic or not A.bf16) else BF16  # atomic epilogues always add into fp32
    if Cout.dtype != want or (R is not None and R.dtype != want):
        raise TypeError(f"cenet_gemm: C / R must be {want} here (operands {'bf16' if A.bf16 else 'fp32'}, atomic={atomic}); "
                        f"got {Cout.dtype}" + (f" / {R.dtype}" if R is not None else ""))
    e = EpiT()
    e.C = Cout.data_ptr() + esz(Cout) * c_offset
    e.scb, e.scb2, e.scr, e.scc = scb, scb2, scr, scc
    e.bias = bias.data_ptr() if bias is not None else None
    e.bias_on_row = int(bias_on_row)
    e.act, e.slope = ACT[act], slope
    e.bscale = bscale.data_ptr() if bscale is not None else None
    e.bscale_rows = bscale_rows
    e.asum = asum.data_ptr() if asum is not None else None
    e.R = (R.data_ptr() + esz(R) * r_offset) if R is not None else None
    e.srb, e.srb2, e.srr, e.src = srb, srb2, srr, src
    e.atomic, e.alpha = int(atomic), alpha
    if col2im is not None:  # scatter epilogue (data-gradient of strided convolutions)
        e.cmode = 1
        e.cKH, e.cKW, e.cPw = col2im["KH"], col2im["KW"], col2im["Pw"]
        e.cHs, e.cWs, e.cstride, e.cpad = col2im["Hs"], col2im["Ws"], col2im["stride"], col2im["pad"]
        e.csci, e.csy, e.csx = col2im["sci"], col2im["sy"], col2im["sx"]
    _launch("cenet_gemm_bf16" if A.bf16 else "cenet_gemm_f32", C.byref(A), C.byref(B), C.byref(e), M, N, K, nbatch, nb_inner, nkb,
            splits)


def _wgrad_array(probs):
    n = len(probs)
    arr = (WgradProbT * n)()
    for d, t in zip(arr, probs):
        d.A, d.B, d.C, d.asum, d.lda, d.ldb, d.skbA, d.skbB, d.M, d.N, d.K, d.nkb = t[:12]
        d.akf = d.bkf = t[12]
    return arr


def wgrad_group(probs, device, phases=(0,), between=None):
    """probs: list of tuples (A_ptr, B_ptr, C_ptr, asum_ptr, lda, ldb, skbA, skbB, M, N, K, nkb, kfast) — all the recorded
    weight gradients of a backward segment in one call (gemm_group.hip): C_i += A_i^T-style contraction, asum_i += row sums.
    phases=(1, 2) issues the K-slice launches and the fold launches as two calls (`between()` runs in between): bench.py"""
    n = len(probs)
    arr = _wgrad_array(probs)
    need = _lib.lib().cenet_wgrad_group_ws_floats(arr, n)
    ws = torch.empty(max(need, 1), device=device, dtype=torch.float32)
    for i, ph in enumerate(phases):
        if i and between is not None:
            between()
        if ph == 0:
            _launch("cenet_wgrad_group_bf16", arr, n, ws, need)
        else:
            _launch("cenet_wgrad_group_phase_bf16", arr, n, ws, need, ph)
    return need


def wgrad_group_plan(probs):
    """[(launch index, bm, bn, ns)] per problem: the partition kern.wgrad_group makes (the library's own, gemm_group.hip)"""
    n = len(probs)
    arr = _wgrad_array(probs)
    out = [(C.c_int * n)() for _ in range(4)]
    _lib.check(_lib.lib().cenet_wgrad_group_plan(arr, n, *out), "cenet_wgrad_group_plan")
    return [tuple(o[i] for o in out) for i in range(n)]


def last_gemm_kernel() -> str:
    """name of the kernel instance the last gemm() on this thread launched (as rocprofv3 prints it); measurement aid"""
    return _lib.lib().cenet_gemm_last_kernel().decode()


def last_conv_kernel() -> str:
    """what the last call on this thread into conv_direct.hip / conv_c1.hip / dwconv.hip launched: the kernel with its template
    arguments and the run-time numbers that pick a code path inside it (cenet_conv_last_kernel); test and measurement aid"""
    return _lib.lib().cenet_conv_last_kernel().decode()


def last_norm_kernel() -> str:
    """what the last call on this thread into norm.hip launched: kernels with template arguments and the run-time numbers that pick a
    code path, joined by '+' when the call launches several (cenet_norm_last_kernel); test and measurement aid"""
    return _lib.lib().cenet_norm_last_kernel().decode()


# ------------------------------------------------------------------------------------------------
# generic call helper
# ------------------------------------------------------------------------------------------------
class Ptr:
    """a tensor seen from an element offset: Ptr(t, off) is passed to _call like a tensor"""

    def __init__(self, t, off: int = 0):
        self.t, self.off = t, off
        self.dtype, self.is_cuda = t.dtype, t.is_cuda

    def data_ptr(self):
        return self.t.data_ptr() + esz(self.t) * self.off


# What include/cenet_hip.h declares a data pointer to point at -> the element type a tensor passed there must have.
# `unsigned`: the four count tables of cenet_argmax_counts_* / cenet_argmax_resize_counts_* ([K + 1, 3] voxel counts, below 2^31);
# every caller allocates them as int32 (evaluate.py), the only 32-bit integer type torch computes with.
_ANY, _NO_TENSOR = object(), object()  # `void*`: any element type; scalars, pointer arrays, argument structs: not a tensor's place
_DTYPE_OF = {"float": torch.float32, "unsigned short": BF16, "double": torch.float64, "long": torch.int64, "int": torch.int32,
             "unsigned": torch.int32, "unsigned char": torch.uint8, "void": _ANY, None: _NO_TENSOR, _lib.PTR_PTR: _NO_TENSOR,
             _lib.STRUCT_PTR: _NO_TENSOR}


def _expect(name):
    """per argument of entry point `name` (without the trailing stream): a torch dtype, _ANY or _NO_TENSOR"""
    try:
        return tuple(_DTYPE_OF[kind] for _, kind in _lib.PARAMS[name][:-1])
    except KeyError as e:  # (as _lib.parse_header: an unknown spelling raises at import, nothing is guessed)
        raise ValueError(f"cenet_hip.h: no tensor type for `{e.args[0]}` in {name}") from None


# entry point -> (its expectations, the entry point a bf16 tensor selects, that one's expectations); entries that launch
# (last parameter: the stream) only.  Built once: a launch does two tuple lookups per argument and no parsing.
_LAUNCHES = {n for n, ps in _lib.PARAMS.items() if ps and ps[-1][0] == "stream"}
_EXPECT = {n: (_expect(n), *((n[:-4] + "_bf16", _expect(n[:-4] + "_bf16")) if n.endswith("_f32") and n[:-4] + "_bf16" in _LAUNCHES
                             else (n, _expect(n)))) for n in _LAUNCHES}


def _refuse(name, i, a):
    pname, kind = _lib.PARAMS[name][i]
    want = _DTYPE_OF[kind]
    if want is _NO_TENSOR:
        raise TypeError(f"{name}: `{pname}` takes no tensor (include/cenet_hip.h: "
                        f"{'a scalar' if kind is None else 'an array of pointers' if kind == _lib.PTR_PTR else 'an argument struct'})")
    raise TypeError(f"{name}: `{pname}` is `{kind}*` in include/cenet_hip.h and takes a {want} tensor, got {a.dtype}")


def _on_device(host):
    if host and not _lib.is_hostsim():
        raise RuntimeError("cenet_amd kernels run on the MI355X only: tensor is not on a CUDA/HIP device "
                           "(there is no CPU fallback)")


def _launch(name, *args):
    """call entry point `name` on the current stream: tensors and `Ptr` go as their data pointer (None: NULL), everything else
    as it is — include/cenet_hip.h types it (_lib.bind).  Every tensor must have exactly the element type the header declares
    for its parameter (TypeError naming both), then live on the GPU; both are settled before the library is touched."""
    want = _EXPECT[name][0]
    if len(args) != len(want):
        raise TypeError(f"{name} takes {len(want)} arguments and the stream, got {len(args)}")
    cargs, host, i = [], False, 0
    for a in args:
        if isinstance(a, (torch.Tensor, Ptr)):
            w = want[i]
            if a.dtype is not w and w is not _ANY:
                _refuse(name, i, a)
            host = host or not a.is_cuda
            a = a.data_ptr()
        cargs.append(a)
        i += 1
    _on_device(host)
    _lib.check(getattr(_lib.lib(), name)(*cargs, stream()), name)


def _call(name, *args):
    """_launch where `name` ends in `_f32` and a bf16 tensor among the arguments selects the `_bf16` twin (all activation
    arguments of one call share their element type); the tensors are held to the prototype of the entry point that is
    called, the twin's then.  One pass over the arguments, this is the hot path of an eager step"""
    want, twin, want16 = _EXPECT[name]
    if len(args) != len(want):
        raise TypeError(f"{name} takes {len(want)} arguments and the stream, got {len(args)}")
    cargs, host, bf, bad, bad16, i = [], False, False, -1, -1, 0
    for a in args:
        if isinstance(a, (torch.Tensor, Ptr)):
            d, w, w16 = a.dtype, want[i], want16[i]
            bf = bf or d is BF16
            if d is not w and w is not _ANY and bad < 0:
                bad = i
            if d is not w16 and w16 is not _ANY and bad16 < 0:
                bad16 = i
            host = host or not a.is_cuda
            a = a.data_ptr()
        cargs.append(a)
        i += 1
    if bf:  # (entries that exist for bf16 tensors only are named so by the caller: they are their own twin)
        name, bad = twin, bad16
    if bad >= 0:
        _refuse(name, bad, args[bad])
    _on_device(host)
    _lib.check(getattr(_lib.lib(), name)(*cargs, stream()), name)


def flash_supported(D: int, Dv: int) -> bool:
    return bool(_lib.lib().cenet_flash_attn_supported(D, Dv))


def flashb_supported(D: int, Dv: int) -> bool:
    """head dims the bf16 (throughput-mode) tiled attention kernels cover: D <= 64, Dv <= 128"""
    return D <= 64 and Dv <= 128


def flash_fwd(a: AttnT, bf16: bool = False):
    name = "cenet_flash_attn_fwd_bf16" if bf16 else "cenet_flash_attn_fwd_f32"
    _launch(name, C.byref(a))


def flash_bwd(a: AttnT, bf16: bool = False):
    name = "cenet_flash_attn_bwd_bf16" if bf16 else "cenet_flash_attn_bwd_f32"
    _launch(name, C.byref(a))


def diffattn_heads_supported(hd: int, N: int) -> bool:
    return bool(_lib.lib().cenet_diffattn_heads_supported(hd, N))


def diffattn_heads_ws_bytes(B: int, H: int, N: int) -> int:
    return _lib.lib().cenet_diffattn_heads_ws_bytes(B, H, N)


def diffattn_heads(a: DiffAttnT, backward: bool):
    name = "cenet_diffattn_heads_bwd_bf16" if backward else "cenet_diffattn_heads_fwd_bf16"
    _launch(name, C.byref(a))


def attn64_ws_bytes(B: int, H: int, N: int) -> int:
    return _lib.lib().cenet_attn64_ws_bytes(B, H, N)


def attn64(a: DiffAttnT, backward: bool):
    """plain self-attention, head dimension 64, bf16 token-major tensors (attn_diff.hip, single-softmax form)"""
    name = "cenet_attn64_bwd_bf16" if backward else "cenet_attn64_fwd_bf16"
    _launch(name, C.byref(a))


def sra_attn_bwd_supported(hd: int, Nk: int) -> bool:
    return bool(_lib.lib().cenet_sra_attn_bwd_supported(hd, Nk))


def sra_attn_bwd_blocks_supported(hd: int, Nk: int) -> bool:
    return bool(_lib.lib().cenet_sra_attn_bwd_blocks_supported(hd, Nk))


def sra_attn_fwd(q, kv, o, lse, B, H, Nq, Nk, scale):
    """spatial-reduction attention forward with resident keys (bf16, head dim 64, <= 64 keys): o and the natural-log lse"""
    _launch("cenet_sra_attn_fwd_bf16", q, kv, o, lse, B, H, Nq, Nk, scale)


def sra_attn_bwd(q, kv, o, dout, lse, dq, dkv, B, H, Nq, Nk, scale):
    """fused spatial-reduction attention backward (bf16, head dim 64, <= 64 keys); dkv: fp32, zero-filled"""
    _launch("cenet_sra_attn_bwd_bf16", q, kv, o, dout, lse, dq, dkv, B, H, Nq, Nk, scale)


def sra_attn_bwd_direct_supported(B, H, Nq, Nk) -> bool:
    return bool(_lib.lib().cenet_sra_attn_bwd_direct_supported(B, H, Nq, Nk))


def sra_attn_bwd_tiles(B, H, Nq) -> int:
    """32-query tiles per wave of the fused backward's launch for this problem (<= 64 keys)"""
    return int(_lib.lib().cenet_sra_attn_bwd_tiles(B, H, Nq))


def sra_attn_bwd_direct(q, kv, o, dout, lse, dq, dkv, B, H, Nq, Nk, scale):
    """as sra_attn_bwd where one workgroup owns a (batch, head): dkv bf16, written (not accumulated)"""
    _launch("cenet_sra_attn_bwd_direct_bf16", q, kv, o, dout, lse, dq, dkv, B, H, Nq, Nk, scale)


def softmax_rows_fwd(x, y, rows, n):
    _call("cenet_softmax_rows_fwd_f32", x, y, rows, n)


def softmax_rows_bwd(y, dy, dx, rows, n):
    _call("cenet_softmax_rows_bwd_f32", y, dy, dx, rows, n)


def softmax_rows_finite_fwd(x, y, rows, n):
    """fp32 parity mode: the scores x pass through torch.nan_to_num before the softmax (multihead_diffattn.py:106)"""
    _call("cenet_softmax_rows_finite_fwd_f32", x, y, rows, n)


def softmax_rows_finite_bwd(y, dy, x, dx, rows, n):
    """... and dx = 0 where the raw score x was not finite (nan_to_num's backward)"""
    _call("cenet_softmax_rows_finite_bwd_f32", y, dy, x, dx, rows, n)


# ---- norms -----------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, y, mean, rstd, rows, Cn, eps):
    _call("cenet_layernorm_fwd_f32", x, gamma, beta, y, mean, rstd, rows, Cn, eps)


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, rows, Cn, dx_add=None):
    _call("cenet_layernorm_bwd_add_acc_f32", dy, x, gamma, mean, rstd, dx_add, dx, dgamma, dbeta, rows, Cn)


def layernorm_bwd_part_supported(dy, x, Cn) -> bool:
    return bool(is_bf16(dy) and is_bf16(x) and Cn % 8 == 0 and Cn <= 512 and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0)


def layernorm_bwd_part(dy, x, gamma, mean, rstd, dx, rows, Cn, dx_add=None, bscale=None, dxs=None):
    """LayerNorm backward whose affine gradients go to a partial buffer [workgroups, 2 C] (returned) instead of float atomics;
    ln_fold_group adds the column sums of many such buffers into their gradients with one launch.
    bscale [B] + dxs (like dx): also write dxs = bscale[sample] * dx (what scale_batch(dx, bscale) would)."""
    nrows = _lib.lib().cenet_layernorm_bwd_part_rows(rows, Cn)
    part = torch.empty((nrows, 2 * Cn), device=dy.device, dtype=torch.float32)
    if bscale is None:
        _call("cenet_layernorm_bwd_add_part_bf16", dy, x, gamma, mean, rstd, dx_add, dx, part, rows, Cn)
    else:
        _call("cenet_layernorm_bwd_add_part_scaled_bf16", dy, x, gamma, mean, rstd, dx_add, dx, part, bscale,
              rows // bscale.numel(), dxs, rows, Cn)
    return part


def ln_fold_group(items):
    """items: [(part [nrows, 2 C], dgamma [C], dbeta [C])]: dgamma / dbeta += column sums, one launch per 48 items"""
    n = len(items)
    if n == 0:
        return
    _chk(*[t for item in items for t in item])
    parts = (C.c_void_p * n)(*[t[0].data_ptr() for t in items])
    dgs = (C.c_void_p * n)(*[t[1].data_ptr() for t in items])
    dbs = (C.c_void_p * n)(*[t[2].data_ptr() for t in items])
    nr = (C.c_int * n)(*[t[0].shape[0] for t in items])
    cs = (C.c_int * n)(*[t[0].shape[1] // 2 for t in items])
    _launch("cenet_ln_fold_group", parts, dgs, dbs, nr, cs, n)


def bn_stats(x, sb, B, Cn, HW, ws, mean, var, rmean, rvar, momentum, nbt):
    _call("cenet_bn_stats_f32", x, sb, B, Cn, HW, ws, mean, var, rmean, rvar, momentum, nbt)


def bn1d_supported(B: int) -> bool:
    return bool(_lib.lib().cenet_bn1d_supported(B))


def bn1d_train_fwd(z, zn, mean, var, rmean, rvar, momentum, nbt, eps, gamma, beta, B, Cn):
    """train-mode BatchNorm1d of a [B, C] fp32 matrix (2 <= B <= 64) in one launch: zn, mean / var, running statistics, counter"""
    _launch("cenet_bn1d_train_fwd_f32", z, zn, mean, var, rmean, rvar, momentum, nbt, eps, gamma, beta, B, Cn)


def bn1d_bwd(dy, z, dz, mean, var, eps, gamma, dgamma, dbeta, B, Cn):
    _launch("cenet_bn1d_bwd_acc_f32", dy, z, dz, mean, var, eps, gamma, dgamma, dbeta, B, Cn)


def bn_train_fwd(x, sxb, y, syb, ws, mean, var, rmean, rvar, momentum, nbt, eps, gamma, beta, act, slope, B, Cn, HW):
    """train-mode BatchNorm forward: statistics + normalisation (+ activation), mean / var / running statistics written"""
    _call("cenet_bn_train_fwd_f32", x, sxb, y, syb, ws, mean, var, rmean, rvar, momentum, nbt, eps, gamma,
          beta, ACT[act], slope, B, Cn, HW, nbt.numel() if nbt is not None else 1)


def bn_apply(x, sxb, y, syb, mean, var, eps, gamma, beta, act, slope, B, Cn, HW):
    _call("cenet_bn_apply_f32", x, sxb, y, syb, mean, var, eps, gamma, beta, ACT[act], slope, B, Cn, HW)


def bn_bwd(dy, sgb, x, sxb, dx, sdb, mean, var, eps, gamma, beta, act, slope, B, Cn, HW, ws, dgamma, dbeta, dx_add=None):
    """dx_add (contiguous [B, C, HW], optional): added to dx by the kernel that writes it (the gradient of a residual connection
    around the BatchNorm)"""
    if dx_add is None:
        _call("cenet_bn_bwd_acc_f32", dy, sgb, x, sxb, dx, sdb, mean, var, eps, gamma, beta, ACT[act],
              slope, B, Cn, HW, ws, dgamma, dbeta)
    else:
        _call("cenet_bn_bwd_add_acc_f32", dy, sgb, x, sxb, dx, sdb, dx_add, Cn * HW, mean, var, eps, gamma, beta,
              ACT[act], slope, B, Cn, HW, ws, dgamma, dbeta)


def res_tail_supported(x2, x3) -> bool:
    return bool(is_bf16(x2) and is_bf16(x3) and x2.dim() == 4 and x2.shape == x3.shape and x2.data_ptr() % 16 == 0
                and x3.data_ptr() % 16 == 0 and _lib.lib().cenet_res_tail_supported(x2.shape[2], x2.shape[3]))


def res_tail_fwd(x2, x3, mean2, var2, g2, b2, eps2, mean3, var3, g3, b3, eps3, w, slope, out, B, Cn, H, W):
    """out = w[c] * MaxPool2x2(LeakyReLU(BN2(x2) + BN3(x3))) from the batch statistics, one launch (csrc/res_tail.hip)"""
    _call("cenet_res_tail_fwd_bf16", x2, x3, mean2, var2, g2, b2, eps2, mean3, var3, g3, b3, eps3, w, slope, out,
          B, Cn, H, W)


def res_tail_bwd(g, x2, x3, mean2, var2, g2, b2, eps2, mean3, var3, g3, b3, eps3, w, slope, dx2, dx3, dg2, db2, dg3, db3, dw, B, Cn,
                 H, W):
    ws = torch.empty(_lib.lib().cenet_res_tail_bwd_ws_floats(Cn), device=g.device, dtype=torch.float32)
    _call("cenet_res_tail_bwd_bf16", g, x2, x3, mean2, var2, g2, b2, eps2, mean3, var3, g3, b3, eps3, w, slope,
          dx2, dx3, dg2, db2, dg3, db3, dw, ws, B, Cn, H, W)


def res_tail_img_fwd(x2, img, mean2, var2, g2, b2, eps2, imean, ivar, w3, g3, b3, eps3, rm3, rv3, nbt3, mom3, w, slope, out, B, Cn, H, W):
    """res_tail_fwd with the shortcut x3 = w3[c] * img not materialised (one-channel input); updates BatchNorm3's running statistics"""
    _call("cenet_res_tail_img_fwd_bf16", x2, img, mean2, var2, g2, b2, eps2, imean, ivar, w3, g3, b3, eps3, rm3, rv3, nbt3,
          mom3, w, slope, out, B, Cn, H, W)


def res_tail_img_bwd(g, x2, img, mean2, var2, g2, b2, eps2, imean, ivar, w3, g3, b3, eps3, w, slope, dx2, dg2, db2, dg3, db3, dw3, dw,
                     B, Cn, H, W):
    ws = torch.empty(_lib.lib().cenet_res_tail_bwd_ws_floats(Cn), device=g.device, dtype=torch.float32)
    _call("cenet_res_tail_img_bwd_bf16", g, x2, img, mean2, var2, g2, b2, eps2, imean, ivar, w3, g3, b3, eps3, w,
          slope, dx2, dg2, db2, dg3, db3, dw3, dw, ws, B, Cn, H, W)


# ---- depthwise conv ------------------------------------------------------------------------------------
# ---- channel-local fused chains (csrc/chanloc.hip) --------------------------------------------------------------------------
_NO_CHANLOC = False  # True: the unfused launch chains (the tests' reference for the fused kernels)


def eucb_supported(x) -> bool:
    B, _, H, W = x.shape
    return (not _NO_CHANLOC) and bool(_lib.lib().cenet_eucb_supported(B, H, W, esz(x)))


def eucb_fwd(x, w, gamma, beta, eps, slope, y, mean, var, rmean, rvar, momentum, nbt, B, Cn, H, W):
    _call("cenet_eucb_fwd_f32", x, Cn * H * W, w, gamma, beta, eps, slope, y, 4 * Cn * H * W, mean, var, rmean,
          rvar, momentum, nbt, B, Cn, H, W)


def eucb_bwd(g, x, w, gamma, beta, eps, slope, mean, var, dx, dw, dgamma, dbeta, B, Cn, H, W):
    _call("cenet_eucb_bwd_acc_f32", g, 4 * Cn * H * W, x, Cn * H * W, w, gamma, beta, eps, slope, mean, var, dx,
          Cn * H * W, dw, dgamma, dbeta, B, Cn, H, W)


def chanloc_supported(B: int, HW: int) -> bool:
    return (not _NO_CHANLOC) and bool(_lib.lib().cenet_chanloc_supported(B, HW))


def cfam_mid_fwd(p_raw, m, x0, x1, y2, gp, bp, epsp, meanp, varp, rmp, rvp, momp, nbtp, w, ls, g2, b2, eps2, mean2, var2, rm2, rv2,
                 mom2, nbt2, B, Cn, HW):
    _call("cenet_cfam_mid_fwd_f32", p_raw, m, x0, x1, y2, gp, bp, epsp, meanp, varp, rmp, rvp, momp, nbtp, w, ls, g2,
          b2, eps2, mean2, var2, rm2, rv2, mom2, nbt2, B, Cn, HW)


def cfam_mid_bwd(g_y2, g_x1, p_raw, m, x1, d_p, d_m, d_x0, gp, bp, epsp, meanp, varp, w, ls, g2, eps2, mean2, var2, dgp, dbp, dw, dls,
                 dg2, db2, B, Cn, HW):
    _call("cenet_cfam_mid_bwd_acc_f32", g_y2, g_x1, p_raw, m, x1, d_p, d_m, d_x0, gp, bp, epsp, meanp, varp, w, ls, g2,
          eps2, mean2, var2, dgp, dbp, dw, dls, dg2, db2, B, Cn, HW)


def dwbn_fwd(x, ws, dils, g, p, v, rest, gamma, beta, eps, mean, var, rmean, rvar, momentum, nbt, B, H, W):
    """MultiOrderDWConv's dilated depthwise branches + BatchNorm + ReLU and the pooled slice's copy in one launch (chanloc.hip)"""
    _chk(*ws)
    nb, Ct = len(ws), len(ws) * g + p
    _call("cenet_dwbn_fwd_f32", x, Ct * H * W, _ptr_arr([w.data_ptr() for w in ws]), (C.c_int * nb)(*dils), nb,
          g, p, v, nb * g * H * W, rest, p * H * W, gamma, beta, eps, mean, var, rmean, rvar, momentum, nbt, B, H, W)


def dwbn_bwd(g_v, g_rest, x, ws, dils, g, p, gamma, beta, eps, mean, var, dx, dws, dgamma, dbeta, B, H, W):
    _chk(*ws, *dws)
    nb, Ct = len(ws), len(ws) * g + p
    _call("cenet_dwbn_bwd_acc_f32", g_v, nb * g * H * W, g_rest, p * H * W, None, 0, x, Ct * H * W,
          _ptr_arr([w.data_ptr() for w in ws]), (C.c_int * nb)(*dils), nb, g, p, gamma, beta, eps, mean, var,
          dx, Ct * H * W, _ptr_arr([w.data_ptr() for w in dws]), dgamma, dbeta, B, H, W)


def cfam_front_fwd(x0, y1, xs, g1, b1, eps1, mean1, var1, rm1, rv1, mom1, nbt1, fc1, fc2, gd, bd, epsd, meand, vard, rmd, rvd, momd,
                   nbtd, u, amax, z, zn, B, Cn, HW):
    _call("cenet_cfam_front_fwd_f32", x0, y1, xs, g1, b1, eps1, mean1, var1, rm1, rv1, mom1, nbt1, fc1, fc2, gd, bd,
          epsd, meand, vard, rmd, rvd, momd, nbtd, u, amax, z, zn, B, Cn, HW)


def cfam_front_bwd(g_xs, g_y1, g_tap, x0, dx0, g1, b1, eps1, mean1, var1, fc1, fc2, gd, epsd, meand, vard, u, amax, z, zn, dg1, db1,
                   dfc1, dfc2, dgd, dbd, B, Cn, HW):
    _call("cenet_cfam_front_bwd_acc_f32", g_xs, g_y1, g_tap, x0, dx0, g1, b1, eps1, mean1, var1, fc1, fc2, gd, epsd,
          meand, vard, u, amax, z, zn, dg1, db1, dfc1, dfc2, dgd, dbd, B, Cn, HW)


def dwact_supported(x) -> bool:
    B, _, H, W = x.shape
    return B * H * W <= 8192 and chanloc_supported(B, H * W)


def dwact_fwd(x, w, bias, y, act, slope, dil, B, Cn, H, W):
    _call("cenet_dwact_fwd_f32", x, w, bias, y, ACT[act], slope, dil, B, Cn, H, W)


def dwact_bwd(g, x, w, bias, dx, dw, db, act, slope, dil, B, Cn, H, W):
    _call("cenet_dwact_bwd_acc_f32", g, x, w, bias, dx, dw, db, ACT[act], slope, dil, B, Cn, H, W)


def pool_branch_supported(B, P, H, W) -> bool:
    return (not _NO_CHANLOC) and 1 <= B <= 64 and 1 <= P <= 32 and 1 <= H <= 64 and 1 <= W <= 64 and H * W >= 16


def pool_branch_fwd(x, sxb, wc, gamma, beta, eps, slope, RH, RW, y, syb, pooled, t, mean, var, rmean, rvar, momentum, nbt, B, P, H, W):
    _call("cenet_pool_branch_fwd_f32", x, sxb, wc, gamma, beta, eps, slope, RH, RW, y, syb, pooled, t, mean, var,
          rmean, rvar, momentum, nbt, B, P, H, W)


def pool_branch_bwd(g, sgb, wc, gamma, beta, eps, slope, RH, RW, pooled, t, mean, var, dt_ws, dx, sdb, dwc, dgamma, dbeta, B, P, H, W):
    _call("cenet_pool_branch_bwd_acc_f32", g, sgb, wc, gamma, beta, eps, slope, RH, RW, pooled, t, mean, var, dt_ws,
          dx, sdb, dwc, dgamma, dbeta, B, P, H, W)


def dw_nchw(x, sxb, w, bias, y, syb, a, sab, B, Cn, H, W, dil, flip, act="none", slope=0.0, x_off=0, y_off=0):
    """x_off / y_off (elements): read / write a channel slice of a wider tensor in place (batch strides sxb / syb)"""
    _call("cenet_dwconv3x3_nchw_f32", Ptr(x, x_off), sxb, w, bias, Ptr(y, y_off) if y is not None else None, syb, a, sab,
          B, Cn, H, W, dil, flip, ACT[act], slope)


def _ptr_arr(vals):
    return (C.c_void_p * len(vals))(*vals)


def dw_nchw_multi(branches, B, H, W, flip):
    """branches: [(x, x_off, sxb, w, y, y_off, syb, C, dil)] — up to 4 bias-free depthwise 3x3 convs (or their data gradients, flip)
    of bf16 NCHW channel slices in ONE launch.  Returns False when the library has no single-launch form for them (the caller
    then launches them one by one)."""
    n = len(branches)
    if n < 1 or n > 4 or any(not is_bf16(b[0]) or not is_bf16(b[4]) for b in branches):
        return False
    _chk(*[b[0] for b in branches], *[b[3] for b in branches], *[b[4] for b in branches])
    xs = _ptr_arr([b[0].data_ptr() + 2 * b[1] for b in branches])
    ws = _ptr_arr([b[3].data_ptr() for b in branches])
    ys = _ptr_arr([b[4].data_ptr() + 2 * b[5] for b in branches])
    sx = (C.c_long * n)(*[b[2] for b in branches])
    sy = (C.c_long * n)(*[b[6] for b in branches])
    cs = (C.c_int * n)(*[b[7] for b in branches])
    ds = (C.c_int * n)(*[b[8] for b in branches])
    rc = _lib.lib().cenet_dwconv3x3_nchw_multi_bf16(xs, sx, ws, ys, sy, cs, ds, n, B, H, W, flip, stream())
    if rc == 2:  # CENET_EUNSUPPORTED
        return False
    _lib.check(rc, "cenet_dwconv3x3_nchw_multi_bf16")
    return True


def dw_wgrad_nchw_multi(branches, B, H, W):
    """branches: [(x, x_off, sxb, dy, g_off, sgb, dw, C, dil)]: dw[i] += dy[i] (*) x[i] for up to 4 branches in ONE launch; False
    when unsupported"""
    n = len(branches)
    if n < 1 or n > 4 or any(not is_bf16(b[0]) or not is_bf16(b[3]) for b in branches):
        return False
    _chk(*[b[0] for b in branches], *[b[3] for b in branches], *[b[6] for b in branches])
    xs = _ptr_arr([b[0].data_ptr() + 2 * b[1] for b in branches])
    gs = _ptr_arr([b[3].data_ptr() + 2 * b[4] for b in branches])
    dws = _ptr_arr([b[6].data_ptr() for b in branches])
    sx = (C.c_long * n)(*[b[2] for b in branches])
    sg = (C.c_long * n)(*[b[5] for b in branches])
    cs = (C.c_int * n)(*[b[7] for b in branches])
    ds = (C.c_int * n)(*[b[8] for b in branches])
    rc = _lib.lib().cenet_dwconv3x3_wgrad_nchw_multi_bf16(xs, sx, gs, sg, dws, cs, ds, n, B, H, W, stream())
    if rc == 2:
        return False
    _lib.check(rc, "cenet_dwconv3x3_wgrad_nchw_multi_bf16")
    return True

def dw_tok(x, w, bias, y, a, B, Cn, H, W, flip, act="none", slope=0.0):
    _call("cenet_dwconv3x3_tok_f32", x, w, bias, y, a, B, Cn, H, W, flip, ACT[act], slope)


def dw_tok_bwd_pre(x, g, w, bias, gu, dw, dbias, B, Cn, H, W, act, slope=0.0):
    """bf16 tokens: gu = g * act'(DW3x3(x) + bias), dw += gu (*) x, dbias += sum gu (pre-activation recomputed from x)."""
    _call("cenet_dwconv3x3_tok_bwd_pre_bf16", x, g, w, bias, gu, dw, dbias, B, Cn, H, W, ACT[act], slope)


def dw_tok_tiled(x):
    """the LDS-tiled bf16 token-layout depthwise kernels apply (16-byte channel groups)"""
    return is_bf16(x) and x.shape[-1] % 8 == 0 and x.data_ptr() % 16 == 0


def pvt_mlp_supported(x, Cn, HD, H, W) -> bool:
    """the fused PVT-MLP kernels (pvt_mlp.hip) have an instance for these bf16 tokens"""
    return bool(is_bf16(x) and x.data_ptr() % 16 == 0 and _lib.lib().cenet_pvt_mlp_supported(Cn, HD, H, W))


def pvt_mlp_fwd(x, ln_g, ln_b, eps, w1, b1, wd, bd, w2, b2, bscale, y, B, H, W, Cn, HD, saved=None):
    """y = x + s_b (fc2(GELU(DW3x3(fc1(LN(x))) + bd)) + b2), one launch (bf16 tokens; w1 / w2 are the bf16 shadows).
    saved = (xn, mean, rstd, h, a): also store the LayerNorm output and statistics, the fc1 output and s_b * the GELU output (what
    the backward kernels and the fc1 / fc2 weight gradients read)."""
    xn, mean, rstd, h, a = saved if saved is not None else (None,) * 5
    _call("cenet_pvt_mlp_fwd_bf16", x, ln_g, ln_b, eps, w1, b1, wd, bd, w2, b2, bscale, y, xn, mean, rstd, h, a, B, H, W,
          Cn, HD)


def pvt_mlp_bwd(g, bscale, w1, w2, wd, bd, h, x, ln_g, mean, rstd, gu, dh, dx, dwd, dbd, dln_g, dln_b, db2, B, H, W, Cn, HD,
                up_scale=None, dxs=None):
    """backward of pvt_mlp_fwd from its saved tensors in two launches (+ a fold): gu = (s_b g . W2) * GELU'(DW(h) + bd) with the
    depthwise weight / bias gradients ADDED into dwd / dbd; dh = DW^T(gu) (the operand of the fc1 weight gradient), dx = g +
    LayerNormBackward(dh . W1) with the affine gradients ADDED into dln_g / dln_b and the fc2 bias gradient (column sums of s_b g)
    into db2 (None: not wanted).  up_scale [B] + dxs: also dxs = up_scale_b * dx (see ops._prescaled_put)."""
    ws = torch.empty(_lib.lib().cenet_pvt_mlp_bwd_ws_floats(B, H, W, Cn), device=g.device, dtype=torch.float32)
    _call("cenet_pvt_mlp_bwd_bf16", g, bscale, w1, w2, wd, bd, h, x, ln_g, mean, rstd, gu, dh, dx, up_scale, dxs, dwd, dbd, dln_g,
          dln_b, db2, ws, B, H, W, Cn, HD)


def pvt_mlp_bwd_plan(B, H, W, Cn, HD):
    """the tiling pvt_mlp_fwd / pvt_mlp_bwd launch with -> (tile_rows, k1_tile_rows, k1_tiles_per_run, k1_runs), see
    cenet_pvt_mlp_bwd_plan in include/cenet_hip.h (host only; raises where there is no fused instance)"""
    out = [C.c_int(0) for _ in range(4)]
    _lib.check(_lib.lib().cenet_pvt_mlp_bwd_plan(B, H, W, Cn, HD, *(C.addressof(o) for o in out)), "cenet_pvt_mlp_bwd_plan")
    return tuple(o.value for o in out)


def dw_wgrad_nchw(x, sxb, dy, sgb, dw, dbias, B, Cn, H, W, dil, x_off=0, g_off=0):
    _call("cenet_dwconv3x3_wgrad_nchw_acc_f32", Ptr(x, x_off), sxb, Ptr(dy, g_off), sgb, dw, dbias, B, Cn, H, W, dil)


def dw_wgrad_tok(x, dy, dw, dbias, B, Cn, H, W):
    _call("cenet_dwconv3x3_wgrad_tok_acc_f32", x, dy, dw, dbias, B, Cn, H, W)


# ---- resampling ------------------------------------------------------------------------------------------
def bilinear_fwd(x, sxb, y, syb, B, Cn, Hi, Wi, Ho, Wo, sh, sw, align):
    _call("cenet_bilinear_fwd_f32", x, sxb, y, syb, B, Cn, Hi, Wi, Ho, Wo, sh, sw, align)


def bilinear_bwd(dy, sgb, dx, sdb, B, Cn, Hi, Wi, Ho, Wo, sh, sw, align, dx_add=None):
    """dx_add (laid out like dx, optional): added to dx by the kernel that writes it"""
    if dx_add is None:
        _call("cenet_bilinear_bwd_f32", dy, sgb, dx, sdb, B, Cn, Hi, Wi, Ho, Wo, sh, sw, align)
    else:
        _call("cenet_bilinear_bwd_add_f32", dy, sgb, dx, sdb, dx_add, B, Cn, Hi, Wi, Ho, Wo, sh, sw, align)


def nearest2x_fwd(x, sxb, y, syb, B, Cn, Hi, Wi):
    _call("cenet_nearest2x_fwd_f32", x, sxb, y, syb, B, Cn, Hi, Wi)


def nearest2x_bwd(dy, sgb, dx, sdb, B, Cn, Hi, Wi):
    _call("cenet_nearest2x_bwd_f32", dy, sgb, dx, sdb, B, Cn, Hi, Wi)


def avgpool_fwd(x, sxb, y, syb, B, Cn, Hi, Wi, Ho, Wo):
    _call("cenet_adaptive_avgpool_fwd_f32", x, sxb, y, syb, B, Cn, Hi, Wi, Ho, Wo)


def avgpool_bwd(dy, sgb, dx, sdb, B, Cn, Hi, Wi, Ho, Wo):
    _call("cenet_adaptive_avgpool_bwd_f32", dy, sgb, dx, sdb, B, Cn, Hi, Wi, Ho, Wo)


def maxpool2_fwd(x, y, syb, scale, B, Cn, Hi, Wi):
    _call("cenet_maxpool2_fwd_f32", x, y, syb, scale, B, Cn, Hi, Wi)


def maxpool2_bwd(x, dy, sgb, dx, scale, dscale, B, Cn, Hi, Wi):
    _call("cenet_maxpool2_bwd_acc_f32", x, dy, sgb, dx, scale, dscale, B, Cn, Hi, Wi)


# ---- CCU / SRM ---------------------------------------------------------------------------------------------
def ccu_stats_fwd(x, fc1, fc2, u, amax, z, B, Cn, HW):
    _call("cenet_ccu_stats_fwd_f32", x, fc1, fc2, u, amax, z, B, Cn, HW)


def gate_chan_fwd(x, g, y, BC, HW):
    _call("cenet_gate_chan_fwd_f32", x, g, y, BC, HW)


def gate_chan_bwd_reduce(x, dy, g, dg, BC, HW):
    _call("cenet_gate_chan_bwd_reduce_f32", x, dy, g, dg, BC, HW)


def ccu_bwd_apply(x, dy, g, dz, u, amax, fc1, fc2, dfc1, dfc2, dx, B, Cn, HW, dx_add=None):
    if dx_add is None:
        _call("cenet_ccu_bwd_apply_acc_f32", x, dy, g, dz, u, amax, fc1, fc2, dfc1, dfc2, dx, B, Cn, HW)
    else:
        _call("cenet_ccu_bwd_apply_add_acc_f32", x, dy, g, dz, u, amax, fc1, fc2, dfc1, dfc2, dx, dx_add, B, Cn, HW)


def srm_stats_fwd(x, u, amax, B, Cn, HW):
    _call("cenet_srm_stats_fwd_f32", x, u, amax, B, Cn, HW)


def srm_conv_fwd(u, pwc, dwc, f, B, H, W):
    _call("cenet_srm_conv_fwd_f32", u, pwc, dwc, f, B, H, W)


def srm_conv_bwd(u, df, pwc, dwc, du, dpwc, ddwc, B, H, W):
    _call("cenet_srm_conv_bwd_acc_f32", u, df, pwc, dwc, du, dpwc, ddwc, B, H, W)


def srm_fused_supported(B, H, W) -> bool:
    return (not _NO_CHANLOC) and bool(_lib.lib().cenet_srm_fused_supported(B, H, W))


def srm_parts(B, H, W) -> int:
    return _lib.lib().cenet_srm_parts(B, H, W)


def srm_conv_gelu_fwd(u, pwc, dwc, f, fa, part, B, H, W):
    _call("cenet_srm_conv_gelu_fwd_f32", u, pwc, dwc, f, fa, part, B, H, W)


def gate_pix_bn_fwd(x, fa, part, G, fb, y, gamma, beta, eps, mean, var, rmean, rvar, momentum, nbt, B, Cn, HW):
    _call("cenet_gate_pix_bn_fwd_f32", x, fa, part, G, fb, y, gamma, beta, eps, mean, var, rmean, rvar, momentum, nbt, B,
          Cn, HW)


def srm_conv_bn_bwd(u, dfb, fa, f, mean, var, eps, gamma, pwc, dwc, part2, du, dpwc, ddwc, dgamma, dbeta, B, H, W):
    _call("cenet_srm_conv_bn_bwd_acc_f32", u, dfb, fa, f, mean, var, eps, gamma, pwc, dwc, part2, du, dpwc, ddwc, dgamma,
          dbeta, B, H, W)


def gate_pix_fwd(x, f, y, B, Cn, HW):
    _call("cenet_gate_pix_fwd_f32", x, f, y, B, Cn, HW)


def gate_pix_bwd_reduce(x, dy, f, df, B, Cn, HW):
    _call("cenet_gate_pix_bwd_reduce_f32", x, dy, f, df, B, Cn, HW)


def srm_bwd_apply(x, dy, f, u, du, amax, dx, B, Cn, HW):
    _call("cenet_srm_bwd_apply_f32", x, dy, f, u, du, amax, dx, B, Cn, HW)


# ---- glue ---------------------------------------------------------------------------------------------------
def transpose(x, sxb, y, syb, B, R, Cc, x_off=0, y_off=0, add=None):
    """y[b] = x[b]^T (+ add[b], laid out like y with batch stride syb)"""
    if add is None:
        _call("cenet_transpose_f32", Ptr(x, x_off), sxb, Ptr(y, y_off), syb, B, R, Cc)
    else:
        _call("cenet_transpose_add_f32", Ptr(x, x_off), sxb, Ptr(y, y_off), syb, add, B, R, Cc)


def copy_batched(x, sxb, y, syb, B, n, accumulate=False, x_off=0, y_off=0):
    _call("cenet_copy_batched_f32", Ptr(x, x_off), sxb, Ptr(y, y_off), syb, B, n, accumulate)


def cat_channels(parts, joined, B, HW, split=False):
    """joined [B, sum c, HW] <- parts [B, c_j, HW] (or the reverse with split=True); at most four parts, one launch"""
    assert 1 <= len(parts) <= 4
    ps = list(parts) + [None] * (4 - len(parts))
    cs = [t.shape[1] for t in parts] + [0] * (4 - len(parts))
    _call("cenet_cat_channels_f32", *ps, *cs, joined, B, HW, split)


def split_channels_add(parts, adds, joined, B, HW):
    """parts[j] [B, c_j, HW] = channel slice j of joined + adds[j] (None: the slice alone); at most four parts, one launch"""
    assert 1 <= len(parts) <= 4 and len(adds) == len(parts)
    ps = list(parts) + [None] * (4 - len(parts))
    ads = list(adds) + [None] * (4 - len(adds))
    cs = [t.shape[1] for t in parts] + [0] * (4 - len(parts))
    _call("cenet_split_channels_add_f32", *ps, *ads, *cs, joined, B, HW)


def add2_fwd(a, b, y, n):
    """y = a + b over n elements (the add join of a DSEB in skip_mode='add'), one launch"""
    _call("cenet_add2_fwd_f32", a, b, y, n)


def add2_bwd(g, ga, gb, da, db, n):
    """da = g + ga, db = g + gb (ga / gb None: g alone) over n elements, one launch reading g once"""
    _call("cenet_add2_bwd_f32", g, ga, gb, da, db, n)


def im2col_tok(src, dst, B, H, W, C, K, stride, pad, inverse=False):
    _call("cenet_im2col_tok_f32", src, dst, B, H, W, C, K, stride, pad, inverse)


def patch_tok(src, dst, B, Ho, Wo, C, S, inverse=False):
    """Space-to-depth of a token map (inverse: patch rows back to tokens); pvtv2.py:93-95 kernel == stride conv."""
    _call("cenet_patch_tok_f32", src, dst, B, Ho, Wo, C, S, inverse)


def scale_batch(x, s, y, B, n):
    _call("cenet_scale_batch_f32", x, s, y, B, n)


def act_fwd(x, y, n, act, slope=0.0):
    _call("cenet_act_fwd_f32", x, y, n, ACT[act], slope)


def act_bwd(pre, dy, dx, n, act, slope=0.0):
    _call("cenet_act_bwd_f32", pre, dy, dx, n, ACT[act], slope)


def silu_mul_fwd(a, b, y, n):
    _call("cenet_silu_mul_fwd_f32", a, b, y, n)


def silu_mul_bwd(a, b, dy, da, db, n):
    _call("cenet_silu_mul_bwd_f32", a, b, dy, da, db, n)


def mix_fwd(x, p, w, z, n):
    _call("cenet_mix_fwd_f32", x, p, w, z, n)


def mix_bwd(x, p, w, dz, dx, dp, dw, n):
    _call("cenet_mix_bwd_acc_f32", x, p, w, dz, dx, dp, dw, n)


def scale_residual_fwd(x, y, ls, out, B, Cn, HW):
    _call("cenet_scale_residual_fwd_f32", x, y, ls, out, B, Cn, HW)


def scale_chan(g, ls, out, B, Cn, HW):
    _call("cenet_scale_chan_f32", g, ls, out, B, Cn, HW)


def chan_dot(a, sab, b, sbb, out, B, Cn, HW):
    _call("cenet_chan_dot_acc_f32", a, sab, b, sbb, out, B, Cn, HW)


def col_sum(a, out, R, Cn):
    _call("cenet_col_sum_acc_f32", a, out, R, Cn)


def add_act_fwd(a, b, out, n, act="none", slope=0.0):
    _call("cenet_add_act_fwd_f32", a, b, out, n, ACT[act], slope)


def lrelu_bwd_from_out(out, dy, dx, n, slope):
    _call("cenet_lrelu_bwd_from_out_f32", out, dy, dx, n, slope)


def dseb_combine_fwd(y, rs, n, w, diff, ycoef, z, B, Cn, HW):
    r = list(rs) + [None] * (3 - len(rs))
    _call("cenet_dseb_combine_fwd_f32", y, r[0], r[1], r[2], n, w, diff, ycoef, z, B, Cn, HW)


def dseb_combine_bwd(y, rs, n, w, diff, ycoef, dz, dy, drs, ddiff, dw, B, Cn, HW):
    r = list(rs) + [None] * (3 - len(rs))
    d = list(drs) + [None] * (3 - len(drs))
    _call("cenet_dseb_combine_bwd_acc_f32", y, r[0], r[1], r[2], n, w, diff, ycoef, dz, dy, d[0], d[1], d[2], ddiff, dw, B,
          Cn, HW)


def diffattn_lambda_fwd(q1, k1, q2, k2, lam0, lam3, hd):
    _call("cenet_diffattn_lambda_fwd_f32", q1, k1, q2, k2, lam0, lam3, hd)


def diffattn_lambda_bwd(q1, k1, q2, k2, lam3, dlam, dq1, dk1, dq2, dk2, hd):
    _call("cenet_diffattn_lambda_bwd_acc_f32", q1, k1, q2, k2, lam3, dlam, dq1, dk1, dq2, dk2, hd)


def diffattn_combine_fwd(U, lam3, out, B, H, N, dv, eps, post):
    _call("cenet_diffattn_combine_fwd_f32", U, lam3, out, B, H, N, dv, eps, post)


def diffattn_combine_bwd(U, lam3, dout, dU, dlam, B, H, N, dv, eps, post):
    _call("cenet_diffattn_combine_bwd_acc_f32", U, lam3, dout, dU, dlam, B, H, N, dv, eps, post)


# ---- loss / optimiser --------------------------------------------------------------------------------------
def dice_ce_fwd(logits, labels, acc, loss, B, K, HW, w_dice, w_ce):
    _call("cenet_dice_ce_fwd_f32", logits, labels, acc, loss, B, K, HW, w_dice, w_ce)


def dice_ce_bwd(logits, labels, acc, gout, dlogits, B, K, HW, w_dice, w_ce):
    _call("cenet_dice_ce_bwd_f32", logits, labels, acc, gout, dlogits, B, K, HW, w_dice, w_ce)


def seg_loss_fwd(logits, labels, acc, loss, B, K, H, W, w_dice, w_ce, w_bd):
    _call("cenet_seg_loss_fwd_f32", logits, labels, acc, loss, B, K, H, W, w_dice, w_ce, w_bd)


def seg_loss_bwd(logits, labels, acc, gout, dlogits, B, K, H, W, w_dice, w_ce, w_bd):
    _call("cenet_seg_loss_bwd_f32", logits, labels, acc, gout, dlogits, B, K, H, W, w_dice, w_ce, w_bd)


def seg_loss_ex_ws_floats(B, K, H, W) -> int:
    """floats of workspace cenet_seg_loss_ex_fwd needs: the compact sums plus one row of partials per forward workgroup"""
    n = _lib.lib().cenet_seg_loss_ex_ws_floats(B, K, H, W)
    if n <= 0:
        raise ValueError(f"seg_loss_ex: unsupported shape B={B} K={K} H={H} W={W} (K <= 16)")
    return n


def seg_loss_ex_fwd(logits, labels, cw, ws, loss, B, K, H, W, w_dice, w_ce, w_bd, w_jac, smooth, ignore_index, from_probs):
    """cw: [2K] fp32 class weights (Dice then CE) or None; ignore_index: int or None"""
    has_ignore, ign = (0, 0) if ignore_index is None else (1, int(ignore_index))
    _call("cenet_seg_loss_ex_fwd_f32", logits, labels, cw, ws, ws.numel(), loss, B, K, H, W, w_dice, w_ce, w_bd, w_jac, smooth,
          has_ignore, ign, int(from_probs))


def seg_loss_ex_bwd(logits, labels, cw, ws, gout, dlogits, B, K, H, W, w_dice, w_ce, w_bd, w_jac, smooth, ignore_index,
                    from_probs):
    has_ignore, ign = (0, 0) if ignore_index is None else (1, int(ignore_index))
    _call("cenet_seg_loss_ex_bwd_f32", logits, labels, cw, ws, gout, dlogits, B, K, H, W, w_dice, w_ce, w_bd, w_jac, smooth,
          has_ignore, ign, int(from_probs))


def argmax_counts(logits, labels, pred, counts, B, K, HW):
    _call("cenet_argmax_counts_f32", logits, labels, pred, counts, B, K, HW)


def surface_border(mask_u8, border_u8, D, H, W):
    _call("cenet_surface_border_u8", mask_u8, border_u8, D, H, W)


def min_sqdist(a_i32, b_i32, out_i32):
    _call("cenet_min_sqdist_i32", a_i32, a_i32.shape[0], b_i32, b_i32.shape[0], out_i32)


LB_COLS = 17  # CENET_LB_COLS
CP_CHUNK = 4096  # voxels per workgroup of the border compaction (csrc/edt.hip)


def edt_supported(D, H, W) -> bool:
    return D > 0 and H > 0 and W > 0 and D * D + H * H + W * W < 2 ** 31


def edt_sq_raw(feat_u8, match, tmp_i32, d2_i32, D, H, W):
    """cenet_edt_sq_u8 without the feature check: d2 = INT_MAX everywhere when no voxel of feat_u8 is a feature"""
    if not edt_supported(D, H, W):
        raise ValueError(f"the distance transform needs D^2 + H^2 + W^2 < 2^31, got {(D, H, W)}")
    _call("cenet_edt_sq_u8", feat_u8, match, tmp_i32, d2_i32, D, H, W)


def edt_sq(feat_u8: torch.Tensor) -> torch.Tensor:
    """exact squared Euclidean distance transform: feat_u8 [D,H,W] uint8 (non-zero = feature voxel) -> int32 [D,H,W],
    d2[v] = min over feature voxels f of |v - f|^2 (unit spacing).  A volume without a feature voxel is refused."""
    assert feat_u8.dim() == 3, "[D,H,W] expected"
    feat_u8 = feat_u8.contiguous()
    if not bool(feat_u8.any()):
        raise ValueError("edt_sq: the volume has no feature voxel")
    d2 = torch.empty(feat_u8.shape, dtype=torch.int32, device=feat_u8.device)
    edt_sq_raw(feat_u8, -1, torch.empty_like(d2), d2, *feat_u8.shape)
    return d2


def check_spacing3(spacing):
    """(sz, sy, sx) as floats; ValueError unless it holds three positive finite numbers"""
    try:
        sp = tuple(float(v) for v in spacing)
    except (TypeError, ValueError):
        raise ValueError(f"spacing: three positive finite numbers (z, y, x) expected, got {spacing!r}") from None
    if len(sp) != 3 or not all(0.0 < v < math.inf for v in sp):
        raise ValueError(f"spacing: three positive finite numbers (z, y, x) expected, got {spacing!r}")
    return sp


def edt_sq_spaced_raw(feat_u8, match, xd_i32, tmp_f64, d2_f64, D, H, W, spacing):
    """cenet_edt_sq_spaced_u8 without the feature check: d2 = +inf everywhere when no voxel of feat_u8 is a feature"""
    if not edt_supported(D, H, W):
        raise ValueError(f"the distance transform needs D^2 + H^2 + W^2 < 2^31, got {(D, H, W)}")
    _call("cenet_edt_sq_spaced_u8", feat_u8, match, xd_i32, tmp_f64, d2_f64, D, H, W, *check_spacing3(spacing))


def edt_sq_spaced(feat_u8: torch.Tensor, spacing) -> torch.Tensor:
    """exact squared Euclidean distance transform with a voxel spacing: feat_u8 [D,H,W] uint8 (non-zero = feature voxel),
    spacing (sz, sy, sx) -> float64 [D,H,W], d2[v] = min over feature voxels f of sz^2 (vz-fz)^2 + sy^2 (vy-fy)^2 + sx^2 (vx-fx)^2
    (scipy: distance_transform_edt(~feat, sampling=spacing)^2).  A volume without a feature voxel is refused."""
    assert feat_u8.dim() == 3, "[D,H,W] expected"
    spacing = check_spacing3(spacing)
    feat_u8 = feat_u8.contiguous()
    if not bool(feat_u8.any()):
        raise ValueError("edt_sq_spaced: the volume has no feature voxel")
    d2 = torch.empty(feat_u8.shape, dtype=torch.float64, device=feat_u8.device)
    xd = torch.empty(feat_u8.shape, dtype=torch.int32, device=feat_u8.device)
    edt_sq_spaced_raw(feat_u8, -1, xd, torch.empty_like(d2), d2, *feat_u8.shape, spacing)
    return d2


def min_sqdist_spaced(a_i32, b_i32, out_f64, spacing):
    """out[i] = min_j of the squared distance between the voxels a_i and b_j ([n,3] int32 (z, y, x) rows) under `spacing`; out is
    written, not merged into.  No atomics: a split of b goes through a scratch of partial minima allocated here."""
    sp = check_spacing3(spacing)
    na, nb = a_i32.shape[0], b_i32.shape[0]
    n = int(_lib.lib().cenet_min_sqdist_spaced_ws_doubles(na, nb))
    ws = torch.empty(n, dtype=torch.float64, device=out_f64.device) if n else None
    _call("cenet_min_sqdist_spaced_f64", a_i32, na, b_i32, nb, *sp, ws, n, out_f64)


def label_borders(pred_f32, gt_f32, border_pred_u8, border_gt_u8, table_i32, K, D, H, W, zfaces=True):
    _call("cenet_label_borders_f32", pred_f32, gt_f32, border_pred_u8, border_gt_u8, table_i32, K, D, H, W, bool(zfaces))


def border_count(bl_u8, match, n, counts_i32):
    _call("cenet_border_count_u8", bl_u8, match, n, counts_i32)


def border_gather(bl_u8, match, D, H, W, offs_i32, src, out):
    """src None: out (int32) gets the (z, y, x) rows of the matching voxels; else src at those voxels — both in C order.  src and
    out are int32, or float64 (the spaced transform's values)"""
    if src is not None and src.dtype == torch.float64:
        _call("cenet_border_gather_f64", bl_u8, match, D, H, W, offs_i32, src, out)
    else:
        _call("cenet_border_gather_i32", bl_u8, match, D, H, W, offs_i32, src, out)


def ccl_supported(D, H, W) -> bool:
    return D > 0 and H > 0 and W > 0 and D * H * W < 2 ** 31


def _ccl_check(K, D, H, W, connectivity=1, zlinks=True):
    if not ccl_supported(D, H, W):
        raise ValueError(f"connected components need positive sides and D*H*W < 2^31, got {(D, H, W)}")
    if not 2 <= K <= 64:
        raise ValueError(f"2 <= classes <= 64 expected, got {K}")
    if connectivity not in (1, 2, 3) or (connectivity == 3 and not zlinks):
        raise ValueError(f"connectivity 1, 2 or 3 expected (1 or 2 per slice), got {connectivity}")


def ccl_label(labels_f32, roots_i32, K, D, H, W, connectivity=1, zlinks=True):
    """roots [D*H*W] = the smallest linear index of each voxel's component (same class, 6 / 18 / 26 neighbours; zlinks False:
    in-plane neighbours only), -1 for background (csrc/ccl.hip)"""
    _ccl_check(K, D, H, W, connectivity, zlinks)
    _call("cenet_ccl_label_f32", labels_f32, roots_i32, K, D, H, W, connectivity, bool(zlinks))


def ccl_sizes(roots_i32, sizes_i32, n):
    """sizes[r] = voxels of the component with root r, 0 elsewhere (zeroed by the call)"""
    _call("cenet_ccl_sizes_i32", roots_i32, sizes_i32, n)


def ccl_ws_ints(K, D, zlinks=True) -> int:
    n = _lib.lib().cenet_ccl_ws_ints(K, D, bool(zlinks))
    if n <= 0:
        raise ValueError(f"connected components: unsupported K={K} D={D} (2 <= K <= 64)")
    return n


def _overlap(a, b) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def ccl_keep(labels_f32, roots_i32, sizes_i32, ws_i32, out_f32, table_i32, K, D, H, W, zlinks=True, min_size=0):
    """out = labels where the voxel's component is its class's largest (per slice with zlinks False; ties: the smaller root) or
    has >= min_size > 0 voxels, else 0; table [K, 3] = components, voxels kept, voxels removed per class.  out may not alias labels."""
    _ccl_check(K, D, H, W)
    if _overlap(out_f32, labels_f32):
        raise ValueError("ccl_keep: out may not alias the label volume")
    _call("cenet_ccl_keep_f32", labels_f32, roots_i32, sizes_i32, ws_i32, ws_i32.numel(), out_f32, table_i32, K, D, H, W,
          bool(zlinks), int(min_size))


def dist_maps_supported(B, K, H, W) -> bool:
    """what cenet_dist_maps_* takes: 2 B (K-1) planes (every mask and its complement) in one launch grid, int32 distances"""
    return B >= 1 and 2 <= K <= 16 and H >= 1 and W >= 1 and 2 * B * (K - 1) <= 65535 and H * H + W * W < 2 ** 31


def _dist_check(what, B, K, H, W):
    if not 2 <= K <= 16:
        raise ValueError(f"{what}: 2 <= classes <= 16 expected, got {K}")
    if not dist_maps_supported(B, K, H, W):
        raise ValueError(f"{what}: positive sides, 2 B (K-1) <= 65535 planes and H^2 + W^2 < 2^31 expected, got {(B, K, H, W)}")


def dist_maps_ws_ints(B, K, H, W) -> int:
    """ints of scratch cenet_dist_maps_* needs: two int32 planes and one byte per pixel of the 2 B (K-1) planes"""
    _dist_check("dist_maps", B, K, H, W)
    return _lib.lib().cenet_dist_maps_ws_ints(B, K, H, W)


def _dist_maps(name, src, n_src, ws_i32, d2_i32, B, K, H, W):
    _dist_check("dist_maps", B, K, H, W)
    if src.numel() != n_src or d2_i32.numel() != B * (K - 1) * H * W:
        raise ValueError(f"dist_maps: {n_src} input and {B * (K - 1) * H * W} output elements expected for {(B, K, H, W)}, got "
                         f"{src.numel()} and {d2_i32.numel()}")
    if _overlap(d2_i32, ws_i32) or _overlap(d2_i32, src) or _overlap(ws_i32, src):
        raise ValueError("dist_maps: input, workspace and output may not alias")
    _call(name, src, ws_i32, ws_i32.numel(), d2_i32, B, K, H, W)


def dist_maps_labels(labels_f32, ws_i32, d2_i32, B, K, H, W):
    """d2 [B,K-1,H,W] int32 = squared distance of every pixel to the nearest pixel of the other kind, for the masks
    {label == c}, c = 1 .. K-1; 0 on a plane whose mask is empty or full (csrc/edt.hip).  No sync, same bits on every run."""
    _dist_maps("cenet_dist_maps_labels_f32", labels_f32, B * H * W, ws_i32, d2_i32, B, K, H, W)


def dist_maps_logits(logits, ws_i32, d2_i32, B, K, H, W):
    """the same for the masks {softmax_c > 1/2} of fp32 or bf16 logits [B,K,H,W]"""
    _dist_maps("cenet_dist_maps_logits_f32", logits, B * K * H * W, ws_i32, d2_i32, B, K, H, W)


def dist_loss_ws_floats(B, K, H, W) -> int:
    """floats of workspace cenet_dist_loss_fwd needs: one row of two partial sums per forward workgroup"""
    n = _lib.lib().cenet_dist_loss_ws_floats(B, K, H, W)
    if n <= 0:
        raise ValueError(f"dist_loss: unsupported shape B={B} K={K} H={H} W={W} (2 <= K <= 16)")
    return n


def _dist_loss_check(logits, labels, d2g, d2p, w, B, K, H, W, surface, hausdorff):
    if not (surface or hausdorff):
        raise ValueError("dist_loss: neither the surface nor the Hausdorff term is present")
    if not 2 <= K <= 16 or B < 1 or H < 1 or W < 1:
        raise ValueError(f"dist_loss: unsupported shape B={B} K={K} H={H} W={W} (2 <= K <= 16)")
    n = B * (K - 1) * H * W
    if logits.numel() != B * K * H * W or labels.numel() != B * H * W or d2g.numel() != n or w.numel() != 2:
        raise ValueError(f"dist_loss: tensor sizes do not match {(B, K, H, W)}")
    if hausdorff and (d2p is None or d2p.numel() != n):
        raise ValueError("dist_loss: the Hausdorff term needs the prediction's distance maps [B,K-1,H,W]")


def dist_loss_fwd(logits, labels, d2g, d2p, w, ws, loss, B, K, H, W, surface, hausdorff):
    """loss[0] = w[0] L_surf + w[1] L_hd (include/cenet_hip.h spells them out); w: fp32 [2] on the device, read by the kernels;
    d2p is passed on only with the Hausdorff term"""
    _dist_loss_check(logits, labels, d2g, d2p, w, B, K, H, W, surface, hausdorff)
    _call("cenet_dist_loss_fwd_f32", logits, labels, d2g, d2p if hausdorff else None, w, ws, ws.numel(), loss, B, K, H, W,
          int(bool(surface)), int(bool(hausdorff)))


def dist_loss_bwd(logits, labels, d2g, d2p, w, gout, dlogits, B, K, H, W, surface, hausdorff):
    _dist_loss_check(logits, labels, d2g, d2p, w, B, K, H, W, surface, hausdorff)
    if dlogits.numel() != logits.numel() or _overlap(dlogits, logits):
        raise ValueError("dist_loss: dlogits has the logits' size and may not alias them")
    _call("cenet_dist_loss_bwd_f32", logits, labels, d2g, d2p if hausdorff else None, w, gout, dlogits, B, K, H, W,
          int(bool(surface)), int(bool(hausdorff)))


def lovasz_tile() -> int:
    """elements per tile of the radix sort of csrc/lovasz.hip"""
    return _lib.lib().cenet_lovasz_tile()


def _lovasz_shape(B, K, H, W, per_image):
    S, n = (B * K, H * W) if per_image else (K, B * H * W)
    if not 2 <= K <= 16 or B < 1 or H < 1 or W < 1 or S > 65535 or n >= 2 ** 31:
        raise ValueError(f"lovasz: unsupported shape B={B} K={K} H={H} W={W} per_image={bool(per_image)} "
                         f"(2 <= K <= 16, at most 65535 segments of fewer than 2^31 pixels)")


def lovasz_ws_bytes(B, K, H, W, per_image) -> int:
    """bytes of workspace cenet_lovasz_fwd needs: keys and payloads twice, the digit counts of a pass, the g counts, the loss rows"""
    _lovasz_shape(B, K, H, W, per_image)
    return _lib.lib().cenet_lovasz_ws_bytes(B, K, H, W, int(bool(per_image)))


def lovasz_order_ws_bytes(S, n) -> int:
    if not (1 <= S <= 65535 and 1 <= n < 2 ** 31):
        raise ValueError(f"lovasz_order: 1 <= S <= 65535 segments of 1 <= n < 2^31 elements expected, got S={S} n={n}")
    return _lib.lib().cenet_lovasz_order_ws_bytes(S, n)


def lovasz_order(errors_f32, ws, perm_i32, S, n):
    """perm [S,n] int32 = the stable descending order of errors [S,n] (fp32, non-negative): numpy's argsort(-e, kind="stable")"""
    lovasz_order_ws_bytes(S, n)
    if errors_f32.numel() != S * n or perm_i32.numel() != S * n:
        raise ValueError(f"lovasz_order: tensor sizes do not match {(S, n)}")
    _call("cenet_lovasz_order_f32", errors_f32, ws, ws.numel() * ws.element_size(), perm_i32, S, n)


def lovasz_fwd(inputs, labels, ws, coef, loss, B, K, H, W, per_image, classes_all, ignore_index, from_probs):
    """loss[0] = the Lovasz-Softmax loss, coef [B,K,H,W] fp32 = dloss / dp (include/cenet_hip.h spells both out);
    ignore_index: None or the label that is in no class"""
    _lovasz_shape(B, K, H, W, per_image)
    if inputs.numel() != B * K * H * W or labels.numel() != B * H * W or coef.numel() != inputs.numel():
        raise ValueError(f"lovasz: tensor sizes do not match {(B, K, H, W)}")
    _call("cenet_lovasz_fwd_f32", inputs, labels, ws, ws.numel() * ws.element_size(), coef, loss, B, K, H, W,
          int(bool(per_image)), int(bool(classes_all)), int(ignore_index is not None),
          0 if ignore_index is None else int(ignore_index), int(bool(from_probs)))


def lovasz_bwd(inputs, coef, gout, dinputs, B, K, H, W, from_probs):
    if not 2 <= K <= 16 or B < 1 or H < 1 or W < 1:
        raise ValueError(f"lovasz: unsupported shape B={B} K={K} H={H} W={W} (2 <= K <= 16)")
    if inputs.numel() != B * K * H * W or coef.numel() != inputs.numel():
        raise ValueError(f"lovasz: tensor sizes do not match {(B, K, H, W)}")
    if dinputs.numel() != inputs.numel() or _overlap(dinputs, inputs):
        raise ValueError("lovasz: dinputs has the inputs' size and may not alias them")
    _call("cenet_lovasz_bwd_f32", inputs, coef, gout, dinputs, B, K, H, W, int(bool(from_probs)))


def topk_tile() -> int:
    """elements per tile of the tie rank of csrc/topk_ce.hip"""
    return _lib.lib().cenet_topk_tile()


def _topk_shape(B, K, H, W, per_image):
    S, n = (B, H * W) if per_image else (1, B * H * W)
    if not 2 <= K <= 16 or B < 1 or H < 1 or W < 1 or S > 65535 or n >= 2 ** 31:
        raise ValueError(f"topk_ce: unsupported shape B={B} K={K} H={H} W={W} per_image={bool(per_image)} "
                         f"(2 <= K <= 16, at most 65535 segments of fewer than 2^31 pixels)")


def topk_ce_ws_bytes(B, H, W, per_image) -> int:
    """bytes of workspace cenet_topk_ce_fwd needs: the keys, the digit bins of the four rounds, the tie counts, the loss rows"""
    _topk_shape(B, 2, H, W, per_image)
    return _lib.lib().cenet_topk_ce_ws_bytes(B, H, W, int(bool(per_image)))


def topk_mask_ws_bytes(S, n) -> int:
    if not (1 <= S <= 65535 and 1 <= n < 2 ** 31):
        raise ValueError(f"topk_mask: 1 <= S <= 65535 segments of 1 <= n < 2^31 elements expected, got S={S} n={n}")
    return _lib.lib().cenet_topk_mask_ws_bytes(S, n)


def topk_mask(values_f32, m_i32, ws, mask_u8, S, n):
    """mask [S,n] uint8 = 1 on the m[s] largest of values [S,n] (fp32, non-negative), equal values by ascending index: numpy's
    argsort(-v, kind="stable")[:m]"""
    topk_mask_ws_bytes(S, n)
    if values_f32.numel() != S * n or mask_u8.numel() != S * n or m_i32.numel() != S:
        raise ValueError(f"topk_mask: tensor sizes do not match {(S, n)}")
    _call("cenet_topk_mask_f32", values_f32, m_i32, ws, ws.numel() * ws.element_size(), mask_u8, S, n)


def topk_ce_fwd(logits, labels, kpercent, ws, wgt, loss, B, K, H, W, per_image, ignore_index):
    """loss[0] = the top-k cross-entropy, wgt [B,H,W] fp32 = 1 / (m S_valid) on the kept pixels (include/cenet_hip.h spells both
    out); kpercent: one fp32 on the device, read there; ignore_index: None or the label that is in no count"""
    _topk_shape(B, K, H, W, per_image)
    if logits.numel() != B * K * H * W or labels.numel() != B * H * W or wgt.numel() != B * H * W or kpercent.numel() != 1:
        raise ValueError(f"topk_ce: tensor sizes do not match {(B, K, H, W)}")
    _call("cenet_topk_ce_fwd_f32", logits, labels, kpercent, ws, ws.numel() * ws.element_size(), wgt, loss, B, K, H, W,
          int(bool(per_image)), int(ignore_index is not None), 0 if ignore_index is None else int(ignore_index))


def topk_ce_bwd(logits, labels, wgt, gout, dlogits, B, K, H, W, ignore_index):
    if not 2 <= K <= 16 or B < 1 or H < 1 or W < 1:
        raise ValueError(f"topk_ce: unsupported shape B={B} K={K} H={H} W={W} (2 <= K <= 16)")
    if logits.numel() != B * K * H * W or labels.numel() != B * H * W or wgt.numel() != B * H * W:
        raise ValueError(f"topk_ce: tensor sizes do not match {(B, K, H, W)}")
    if dlogits.numel() != logits.numel() or _overlap(dlogits, logits):
        raise ValueError("topk_ce: dlogits has the logits' size and may not alias them")
    _call("cenet_topk_ce_bwd_f32", logits, labels, wgt, gout, dlogits, B, K, H, W, int(ignore_index is not None),
          0 if ignore_index is None else int(ignore_index))


def sgd_step(p, g, buf, hyper5, n, shadow=None):
    """shadow: bf16 copy of the parameters, rewritten by the same kernel (the GEMM operand of the throughput mode)"""
    if shadow is None:
        _call("cenet_sgd_step_f32", p, g, buf, hyper5, n)
    else:
        _launch("cenet_sgd_step_shadow_f32", p, g, buf, hyper5, n, shadow)


def adam_step(p, g, exp_avg, exp_avg_sq, hyper12, n, shadow=None):
    """fused Adam / AdamW update (hyper12: include/cenet_hip.h); shadow: bf16 copy of the parameters, rewritten in the same pass"""
    if shadow is None:
        _call("cenet_adam_step_f32", p, g, exp_avg, exp_avg_sq, hyper12, n)
    else:
        _launch("cenet_adam_step_shadow_f32", p, g, exp_avg, exp_avg_sq, hyper12, n, shadow)


def cast(x: torch.Tensor, dtype) -> torch.Tensor:
    """fp32 <-> bf16 copy of a contiguous tensor (cenet_cast_*); returns x itself when it already has `dtype`"""
    if x.dtype == dtype:
        return x
    x = x if x.is_contiguous() else x.contiguous()
    y = torch.empty(x.shape, device=x.device, dtype=dtype)
    name = "cenet_cast_f32_to_bf16" if dtype == BF16 else "cenet_cast_bf16_to_f32"
    _launch(name, x, y, x.numel())
    return y


def cast_clear(x: torch.Tensor, y: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """y (bf16) = x (fp32, contiguous) [+ bias over the last axis]; x = 0 afterwards (see ops._ZeroWs)"""
    assert x.numel() == y.numel()
    if bias is None:
        _launch("cenet_cast_clear_f32_to_bf16", x, y, x.numel())
    else:
        _launch("cenet_cast_clear_bias_f32_to_bf16", x, y, bias, bias.numel(), x.numel())


def cast_into(x: torch.Tensor, y: torch.Tensor):
    name = "cenet_cast_f32_to_bf16" if y.dtype == BF16 else "cenet_cast_bf16_to_f32"
    assert x.numel() == y.numel() and x.is_contiguous() and y.is_contiguous()
    _launch(name, x, y, x.numel())


def wq(W: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """The weight as the GEMM operand for activations of `like`'s type: W itself (fp32) or its bf16 shadow.
    A parameter that lives in a `ParamArena` has a slot in the arena's bf16 buffer, refreshed by the fused SGD kernel; any
    other tensor gets a private shadow.  A shadow is re-cast whenever the tensor was modified in place through torch since
    (`Tensor._version`), e.g. by load_state_dict or a torch optimizer."""
    if like.dtype != BF16 or W is None:
        return W
    sh = getattr(W, "_cenet_shadow", None)
    if sh is None:
        slot = getattr(W, "_cenet_arena_slot", None)
        if slot is not None and slot[0].params.device == W.device:
            slot[0].enable_shadow()
            sh = W._cenet_shadow
    if sh is None or sh.shape != W.shape or sh.device != W.device:
        sh = torch.empty(W.shape, device=W.device, dtype=BF16)
        W._cenet_shadow = sh
        W._cenet_shadow_ver = -1
    if W._cenet_shadow_ver != W._version:
        cast_into(W.detach() if W.is_contiguous() else W.detach().contiguous(), sh)
        W._cenet_shadow_ver = W._version
    return sh


def zero_(t: torch.Tensor):
    """zero-fill with the library's own kernel (a kernel node replays faithfully in a hipGraph; hipMemsetAsync did not)"""
    nbytes = t.numel() * t.element_size()
    assert t.is_contiguous(), "zero_: contiguous tensor"
    if nbytes == 0:
        return t
    if nbytes % 4 == 0 and t.data_ptr() % 4 == 0:  # whole 4-byte words: cenet_zero_f32 fills them, whatever they hold
        _launch("cenet_zero_f32", t if t.dtype is torch.float32 else t.view(-1).view(torch.float32), nbytes // 4)
    else:  # a bf16 tensor with an odd element count / an odd-element view: head and tail bytes handled by the kernel
        _launch("cenet_zero_bytes", t, nbytes)
    return t


def conv_direct_supported(Cin: int, Cout: int, k: int, stride: int, pad: int) -> bool:
    return bool(_lib.lib().cenet_conv_direct_supported(Cin, Cout, k, stride, pad))


def conv_direct(x, w, y, B, Cin, Cout, H, W, k, dgrad):
    """direct convolution on bf16 tensors (LDS halo tiles, weights resident in LDS; w = fp32 master weight);
    dgrad: x=dY, w=forward weight, y=dX."""
    _launch("cenet_conv_direct_bf16", x, w, y, B, Cin, Cout, H, W, k, dgrad)


def conv_c1_supported(Cin: int, Cout: int, k: int, stride: int, pad: int) -> bool:
    return bool(_lib.lib().cenet_conv_c1_supported(Cin, Cout, k, stride, pad))


def conv_c1_fwd(x, w, y, B, Cout, H, W, k):
    """one-channel bf16 image -> Cout <= 32 channels, stride 1, same padding (conv_c1.hip)"""
    _launch("cenet_conv_c1_fwd_bf16", x, w, y, B, Cout, H, W, k)


def conv_c1_wgrad(x, dy, dw, B, Cout, H, W, k):
    _launch("cenet_conv_c1_wgrad_bf16", x, dy, dw, B, Cout, H, W, k)


def pw_fewout_supported(Cin: int, Cout: int) -> bool:
    return bool(_lib.lib().cenet_pw_fewout_supported(Cin, Cout))


def pw_fewout_wgrad_supported(Cin: int, Cout: int) -> bool:
    return bool(_lib.lib().cenet_pw_fewout_wgrad_supported(Cin, Cout))


def pw_fewout_fwd(x, W, bias, y, B, Cin, Cout, HW):
    """64 -> few channels 1x1 conv with bias on bf16 tensors (conv_c1.hip); W: bf16 [Cout, 64]"""
    _launch("cenet_pw_fewout_fwd_bf16", x, W, bias, y, B, Cin, Cout, HW)


def pw_fewout_dgrad(dy, W, dx, B, Cin, Cout, HW):
    _launch("cenet_pw_fewout_dgrad_bf16", dy, W, dx, B, Cin, Cout, HW)


def pw_fewout_wgrad(x, dy, dW, dbias, B, Cin, Cout, HW):
    _launch("cenet_pw_fewout_wgrad_bf16", x, dy, dW, dbias, B, Cin, Cout, HW)


def pw_small_supported(G: int) -> bool:
    return bool(_lib.lib().cenet_pw_small_supported(G))


def pw_small(x, W, y, B, groups, G, HW, transpose=False):
    """groups x (G x G) bias-free 1x1 convs on bf16 NCHW tensors, G <= 40 (conv_c1.hip); W: bf16 [groups, G, G]"""
    _launch("cenet_pw_small_bf16", x, W, y, B, groups, G, HW, transpose)


def conv_wgrad_direct_supported(Cin: int, Cout: int, k: int, stride: int, pad: int) -> bool:
    return bool(_lib.lib().cenet_conv_wgrad_direct_supported(Cin, Cout, k, stride, pad))


def conv_wgrad_direct(x, dy, dw, B, Cin, Cout, H, W, k):
    """bf16-operand direct weight gradient (LDS tiles of dY and the X halo, funnel-shifted tap windows): dw += dY (*) x."""
    ws = torch.empty(_lib.lib().cenet_conv_wgrad_direct_ws_floats(Cin, Cout, k), device=x.device, dtype=torch.float32)
    _launch("cenet_conv_wgrad_direct_bf16", x, dy, dw, ws, B, Cin, Cout, H, W, k)


# ---- precision mode ------------------------------------------------------------------------------------------------
# The element type of the tensors decides which kernels run: fp32 tensors take the exact fp32 MFMA chain (parity mode),
# bf16 tensors the throughput path (bf16 in HBM and in the MFMA operands, fp32 accumulation / softmax / statistics).  This
# flag only tells `CENet.forward` to cast its input (and thereby the whole network) to bf16.
_COMPUTE_BF16 = False


def set_compute_bf16(on: bool) -> bool:
    """False (default): CENet runs in fp32, the mode every parity claim is made in.  True: CENet casts its input to bf16 and
    all activations, activation gradients and GEMM operands are bf16 (weights through a bf16 shadow of the fp32 master
    copy); logits come back as bf16.  Returns the previous setting."""
    global _COMPUTE_BF16
    old = _COMPUTE_BF16
    _COMPUTE_BF16 = bool(on)
    return old


def get_compute_bf16() -> bool:
    return _COMPUTE_BF16


def augment_acdc(pool_img, pool_lab, tab, dp, stage_img, stage_lab, stage_stride, max_h, max_w, out_img, out_lab, B, OH, OW):
    """cenet_augment_acdc (augment.hip): gather + augment one training batch from the device-resident slices"""
    for t in (pool_img, pool_lab, tab, dp, stage_img, stage_lab, out_img, out_lab):
        assert t.is_contiguous()
    _launch("cenet_augment_acdc", pool_img, pool_lab, tab, dp, stage_img, stage_lab, stage_stride, max_h, max_w, out_img, out_lab,
            B, OH, OW)


AUG_OPS = {"copy": 0, "flip_ud": 1, "flip_lr": 2, "affine": 3, "grid_warp": 4, "blur": 5, "noise": 6, "contrast": 7}
AUG_OPS_DP = 32  # doubles per (sample, stage) of cenet_augment_ops


def augment_ops(pool_img, pool_lab, tab_host, dp_host, tab, dp, work_img, work_lab, stride, max_h, max_w, B, S):
    """cenet_augment_ops (augment_ops.hip): S stages of flips / warps / blur / noise / contrast for one batch of device-resident
    slices.  tab_host [B, 3 + S] int64 and dp_host [B, S, 32] float64 are the plan as numpy arrays, tab / dp the same tables on
    the device; work_img / work_lab: two fp32 and two uint8 buffers of B * stride elements.  The result is in buffer S & 1."""
    import numpy as np
    assert tab_host.dtype == np.int64 and tab_host.shape == (B, 3 + S) and tab_host.flags.c_contiguous
    assert dp_host.dtype == np.float64 and dp_host.shape == (B, S, AUG_OPS_DP) and dp_host.flags.c_contiguous
    assert tab.numel() == tab_host.size and dp.numel() == dp_host.size
    for t in (pool_img, pool_lab, tab, dp, *work_img, *work_lab):
        assert t.is_contiguous()
    assert all(t.numel() >= B * stride for t in (*work_img, *work_lab))
    _launch("cenet_augment_ops", pool_img, pool_lab, tab_host.ctypes.data, dp_host.ctypes.data, tab, dp, work_img[0], work_lab[0],
            work_img[1], work_lab[1], stride, max_h, max_w, B, S)
    return S & 1


def philox4x32_10(ctr_key, out):
    """cenet_philox4x32_10: ctr_key [n, 6] int64 (4 counter + 2 key words) -> out [n, 4] int64, the generator of the noise op"""
    assert ctr_key.is_contiguous() and out.is_contiguous() and ctr_key.shape[1] == 6 and out.shape == (ctr_key.shape[0], 4)
    _launch("cenet_philox4x32_10", ctr_key, out, ctr_key.shape[0])


def augment_normalize(x, mean, std):
    """cenet_augment_normalize: x = (x - mean) / std in fp32, in place"""
    assert x.is_contiguous()
    _launch("cenet_augment_normalize", x, x.numel(), mean, std)


AUG_IMAGE_OPS = {"copy": 0, "flip_ud": 1, "flip_lr": 2, "affine": 3, "blur": 4, "brightness_contrast": 5, "elastic": 6}
AUG_IMAGE_MIRROR = 256  # bit 8 of an affine / elastic op word: mode='mirror' instead of 'constant'
AUG_MINMAX_PARTS = 128  # workgroups per sample of cenet_augment_minmax


def augment_image_ops(pool_img, pool_lab, tab_host, dp_host, tab, dp, fw_host, fw, field, work_img, work_lab, out_lab, N, C, H, W,
                      B, S):
    """cenet_augment_image_ops (augment_image_ops.hip): S stages of flips / affine / blur / brightness-contrast / elastic warp for
    one batch of device-resident C-channel images.  tab_host [B, 1 + S] int64 and dp_host [B, S, 32] float64 are the plan as numpy
    arrays, tab / dp the same tables on the device; fw_host (numpy float64 [radius + 1]) / fw: the elastic field's kernel, field:
    B * 2 * H * W float64 of scratch (all three None when no chain is elastic); work_img / work_lab: two fp32 buffers of
    B * C * H * W and two uint8 buffers of B * H * W elements; out_lab: None or [B, H, W] fp32.  The result is in buffer S & 1."""
    import numpy as np
    assert tab_host.dtype == np.int64 and tab_host.shape == (B, 1 + S) and tab_host.flags.c_contiguous
    assert dp_host.dtype == np.float64 and dp_host.shape == (B, S, AUG_OPS_DP) and dp_host.flags.c_contiguous
    assert tab.numel() == tab_host.size and dp.numel() == dp_host.size
    radius = 0
    if fw_host is not None:
        assert fw_host.dtype == np.float64 and fw_host.ndim == 1 and fw_host.flags.c_contiguous and fw.numel() == fw_host.size
        assert field.numel() >= B * 2 * H * W
        radius = fw_host.size - 1
    for t in (pool_img, pool_lab, tab, dp, fw, field, *work_img, *work_lab, out_lab):
        assert t is None or t.is_contiguous()
    assert pool_img.numel() >= N * C * H * W and pool_lab.numel() >= N * H * W
    assert all(t.numel() >= B * C * H * W for t in work_img) and all(t.numel() >= B * H * W for t in work_lab)
    assert out_lab is None or out_lab.numel() == B * H * W
    _launch("cenet_augment_image_ops", pool_img, pool_lab, tab_host.ctypes.data, dp_host.ctypes.data, tab, dp,
            None if fw_host is None else fw_host.ctypes.data, fw, radius, field, work_img[0], work_lab[0], work_img[1], work_lab[1],
            out_lab, N, C, H, W, B, S)
    return S & 1


def augment_minmax(x, y, part, B, n):
    """cenet_augment_minmax: y[b] = (x[b] - min) / ((max - min) + 1e-8f) per sample of x [B, n] fp32, in float32 (y may be x);
    part: B * 2 * AUG_MINMAX_PARTS floats of scratch"""
    assert x.is_contiguous() and y.is_contiguous() and part.is_contiguous()
    assert x.numel() >= B * n and y.numel() >= B * n and part.numel() >= B * 2 * AUG_MINMAX_PARTS
    _launch("cenet_augment_minmax", x, y, part, B, n)


_SPLINE_POLE = math.sqrt(3.0) - 2.0  # the cubic B-spline prefilter's pole (scipy ni_splines)


def vol_resize_supported(H: int, W: int, PH: int, PW: int) -> bool:
    """scipy special-cases length-1 axes; the kernels do not"""
    return min(H, W, PH, PW) >= 2


def vol_resize_cubic(src, stage, out, n, H, W, PH, PW, normalize=None):
    """cenet_vol_resize_cubic (volresize.hip): zoom(order=3) of n slices src [n, H, W] fp32 -> out [n, 1, PH, PW] fp32; stage: at
    least n * H * W float64 of scratch; normalize = (mean, std) or None"""
    assert src.is_contiguous() and out.is_contiguous() and stage.is_contiguous()
    assert src.numel() >= n * H * W and stage.numel() >= n * H * W and out.numel() == n * PH * PW
    mean, std = normalize if normalize is not None else (0.0, 1.0)
    _launch("cenet_vol_resize_cubic", src, stage, out, n, H, W, PH, PW, _SPLINE_POLE ** (H - 1), _SPLINE_POLE ** (W - 1),
            normalize is not None, mean, std)


def argmax_resize_counts(logits, labels, pred, counts, n, K, PH, PW, H, W):
    """cenet_argmax_resize_counts (volresize.hip): logits [n, K, PH, PW] fp32 / bf16 -> pred [n, H, W] class ids as float (argmax +
    zoom(order=0) in one pass); with labels [n, H, W] float, counts [K + 1, 3] int32 as argmax_counts fills them"""
    assert logits.is_contiguous() and pred.is_contiguous()
    assert logits.numel() == n * K * PH * PW and pred.numel() == n * H * W
    if labels is not None:
        assert labels.is_contiguous() and labels.numel() == n * H * W
        assert counts is not None and counts.numel() == (K + 1) * 3
    _call("cenet_argmax_resize_counts_f32", logits, labels, pred, counts, n, K, PH, PW, H, W)


# test-time augmentation (tta.hip): a view is an element of D4 coded 0..7 (bit 0 flip along W, bit 1 flip along H, bit 2 transpose), a
# view set a mask of those codes
TTA_SETS = {"flips": 0b0000_0111, "flips4": 0b0000_1111, "d4": 0xFF}


def tta_view_mask(tta):
    """(view mask, number of views T) of a named set of TTA_SETS or a tuple of view codes 0..7"""
    if isinstance(tta, str):
        if tta not in TTA_SETS:
            raise ValueError(f"tta: one of {sorted(TTA_SETS)} or a tuple of view codes 0..7 expected, got {tta!r}")
        mask = TTA_SETS[tta]
    else:
        codes = list(tta) if isinstance(tta, (tuple, list)) else None
        if not codes or any(not isinstance(g, int) or isinstance(g, bool) or not 0 <= g <= 7 for g in codes):
            raise ValueError(f"tta: one of {sorted(TTA_SETS)} or a non-empty tuple of view codes 0..7 expected, got {tta!r}")
        mask = 0
        for g in codes:
            mask |= 1 << g
    return mask, bin(mask).count("1")


def _tta_views_of(view_mask):
    """T of a valid mask; 1 for one the entry point refuses (so that the refusal is the library's, with its name)"""
    return bin(view_mask).count("1") if 1 <= view_mask <= 255 else 1


def tta_views(src, out, n, C, PH, PW, view_mask):
    """cenet_tta_views_f32 (tta.hip): src [n, C, PH, PW] fp32 -> out [T, n, C, PH, PW], the views of `view_mask` in ascending code
    order, one launch"""
    assert src.is_contiguous() and out.is_contiguous()
    assert src.numel() == n * C * PH * PW and out.numel() == _tta_views_of(view_mask) * n * C * PH * PW
    _launch("cenet_tta_views_f32", src, out, n, C, PH, PW, view_mask)


def tta_argmax_resize_counts(logits, labels, pred, conf, counts, n, K, PH, PW, H, W, view_mask):
    """cenet_tta_argmax_resize_counts (tta.hip): logits [T, n, K, PH, PW] fp32 / bf16, one stack per view -> pred [n, H, W] class ids
    as float (un-view + softmax + mean over the views + argmax + zoom(order=0) in one pass) and conf [n, H, W] (or None), the
    winner's mean probability; labels / counts as for argmax_resize_counts"""
    assert logits.is_contiguous() and pred.is_contiguous()
    assert logits.numel() == _tta_views_of(view_mask) * n * K * PH * PW and pred.numel() == n * H * W
    assert conf is None or (conf.is_contiguous() and conf.numel() == n * H * W)
    if labels is not None:
        assert labels.is_contiguous() and labels.numel() == n * H * W
        assert counts is None or counts.numel() == (K + 1) * 3
    _call("cenet_tta_argmax_resize_counts_f32", logits, labels, pred, conf, counts, n, K, PH, PW, H, W, view_mask)


# sliding-window inference (sliding_window.hip): the window grid is nnU-Net's, the Gaussian importance map MONAI's (sigma_scale 0.125)
SW_MAX_WINDOWS = 32  # per axis (SW_MAXW)
SW_IMPORTANCE = ("gaussian", "constant")


def sw_origins(L: int, P: int, overlap: float):
    """the window origins along an axis of length L for windows of side P: one centred window (origin -((P - L) // 2), the rest
    is padding) for L <= P, else N = ceil((L - P) / (P (1 - overlap))) + 1 windows at round(i (L - P) / (N - 1))"""
    import numpy as np
    L, P = int(L), int(P)
    if L < 1 or P < 1:
        raise ValueError(f"sliding window: sides >= 1 expected, got image side {L}, window side {P}")
    if isinstance(overlap, bool) or not isinstance(overlap, (int, float)) or not 0.0 <= overlap < 1.0:
        raise ValueError(f"window overlap: a number in [0, 1) expected, got {overlap!r}")
    if L <= P:
        return [-((P - L) // 2)]
    N = int(math.ceil((L - P) / (P * (1.0 - overlap)))) + 1
    if N > SW_MAX_WINDOWS:
        raise ValueError(f"sliding window: {N} windows of side {P} along an axis of {L} at overlap {overlap}, at most "
                         f"{SW_MAX_WINDOWS} are supported")
    o = [int(np.round(i * (L - P) / (N - 1))) for i in range(N)]
    if any(b <= a for a, b in zip(o, o[1:])):  # (a step below one pixel: P (1 - overlap) < 1)
        raise ValueError(f"sliding window: overlap {overlap} of a window of side {P} steps by less than a pixel")
    return o


def sw_weights(P: int, importance: str = "gaussian"):
    """one factor [P] of the separable importance map as a float32 numpy vector, computed in float64: "gaussian"
    exp(-0.5 ((i - (P - 1) / 2) / (0.125 P))^2), "constant" ones"""
    import numpy as np
    if importance not in SW_IMPORTANCE:
        raise ValueError(f"window importance: one of {SW_IMPORTANCE} expected, got {importance!r}")
    if importance == "constant":
        return np.ones(int(P), dtype=np.float32)
    i = np.arange(int(P), dtype=np.float64)
    return np.exp(-0.5 * ((i - (P - 1) / 2.0) / (0.125 * P)) ** 2).astype(np.float32)


def _sw_table(o):
    """an origin table as the C int array the entry points read on the host"""
    import numpy as np
    return np.ascontiguousarray(np.asarray(o, dtype=np.int64).astype(np.int32).reshape(-1))


def sw_windows(src, out, oy, ox, n, C, H, W, PH, PW, normalize=None, pad_value=0.0):
    """cenet_sw_windows_f32 (sliding_window.hip): src [n, C, H, W] fp32 -> out [n * len(oy) * len(ox), C, PH, PW], window
    (b, iy, ix) holding source pixel (oy[iy] + y, ox[ix] + x), `pad_value` outside the slice; normalize = (mean, std) or None.
    oy / ox: sequences of ints (host); the library checks them"""
    ty, tx = _sw_table(oy), _sw_table(ox)
    assert src.is_contiguous() and out.is_contiguous()
    assert src.numel() == n * C * H * W and out.numel() == n * ty.size * tx.size * C * PH * PW
    mean, std = normalize if normalize is not None else (0.0, 1.0)
    _launch("cenet_sw_windows_f32", src, out, ty.ctypes.data, tx.ctypes.data, n, C, H, W, PH, PW, ty.size, tx.size,
            normalize is not None, mean, std, pad_value)


def sw_merge_counts(logits, labels, wy, wx, oy, ox, pred, conf, counts, n, K, PH, PW, H, W, view_mask=1):
    """cenet_sw_merge_counts (sliding_window.hip): logits [T, n * len(oy) * len(ox), K, PH, PW] fp32 / bf16, one stack per view ->
    pred [n, H, W] class ids as float (softmax per window and view, blended with wy [PH] x wx [PW] fp32 on the device, argmax) and
    conf [n, H, W] (or None), the winner's blended probability; labels / counts as for argmax_resize_counts"""
    ty, tx = _sw_table(oy), _sw_table(ox)
    assert logits.is_contiguous() and pred.is_contiguous() and wy.is_contiguous() and wx.is_contiguous()
    assert logits.numel() == _tta_views_of(view_mask) * n * ty.size * tx.size * K * PH * PW and pred.numel() == n * H * W
    assert wy.numel() == PH and wx.numel() == PW
    assert conf is None or (conf.is_contiguous() and conf.numel() == n * H * W)
    if labels is not None:
        assert labels.is_contiguous() and labels.numel() == n * H * W
        assert counts is None or counts.numel() == (K + 1) * 3
    _call("cenet_sw_merge_counts_f32", logits, labels, wy, wx, ty.ctypes.data, tx.ctypes.data, pred, conf, counts, n, K, PH, PW, H,
          W, ty.size, tx.size, view_mask)


def layernorm_fwd_acc(acc, bias, xpre, gamma, beta, y, mean, rstd, rows, Cn, eps):
    """cenet_layernorm_fwd_acc_bf16: LayerNorm straight from a split-K fp32 accumulator (+ bias); acc is zero afterwards"""
    _launch("cenet_layernorm_fwd_acc_bf16", acc, bias, xpre, gamma, beta, y, mean, rstd, rows, Cn, eps)
