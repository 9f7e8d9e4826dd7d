"""The C-ABI library loads and exports every entry point that include/cenet_hip.h declares, and the ctypes layer types every one
of them from that header (cenet_amd/_lib.py): prototypes, struct layouts, refusals and conversions."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from backend import dev  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "cenet_hip.h")).read()
    return sorted(set(re.findall(r"\b(?:int|long|const char\*)\s+(cenet_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert len(syms) >= 55
    assert "cenet_gemm_f32" in syms and "cenet_flash_attn_fwd_f32" in syms and "cenet_sgd_step_f32" in syms


def test_hip_library_exports_every_declared_symbol():
    from cenet_amd import build
    lib_path = build.build_hip(verbose=False)  # hipcc cross-compiles for gfx950 without a GPU
    lib = ctypes.CDLL(lib_path)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"libcenet_hip.so does not export: {missing}"


def test_product_path_refuses_cpu_tensors():
    """No CPU fallback: the product ops raise on host tensors instead of silently computing elsewhere."""
    import torch
    from cenet_amd import _lib, ops
    assert not _lib.is_hostsim()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear(torch.randn(4, 8), torch.randn(3, 8))


def test_missing_library_fails_loudly(monkeypatch):
    from cenet_amd import _lib
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libcenet_hip.so")
    monkeypatch.setattr(_lib, "_LIB", None)
    with pytest.raises(RuntimeError, match="no CPU/PyTorch fallback"):
        _lib.lib()


# ---- typed prototypes (cenet_amd/_lib.py bind) -------------------------------------------------------------------------------------
def header_text():
    """include/cenet_hip.h without its comments"""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cenet_hip.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def hip_lib():
    """the gfx950 library, bound; nothing here launches a kernel"""
    from cenet_amd import _lib, build
    return _lib.bind(ctypes.CDLL(build.build_hip(verbose=False)))


def test_every_declared_prototype_is_bound(hip_lib):
    protos = re.findall(r"\b(cenet_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_text())
    assert sorted({n for n, _ in protos}) == declared_symbols()
    for name, params in protos:
        fn = getattr(hip_lib, name)
        want = 0 if params.strip() in ("", "void") else params.count(",") + 1
        assert fn.argtypes is not None and len(fn.argtypes) == want, name
        assert fn.restype in (ctypes.c_int, ctypes.c_long, ctypes.c_char_p), name
    assert hip_lib.cenet_gemm_last_kernel.restype is ctypes.c_char_p
    assert hip_lib.cenet_wgrad_group_ws_floats.restype is ctypes.c_long


STRUCTS = {"cenet_mat_t": "MatT", "cenet_epi_t": "EpiT", "cenet_wgrad_prob_t": "WgradProbT", "cenet_attn_t": "AttnT",
           "cenet_diffattn_t": "DiffAttnT"}


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof / offsetof of every field as the host C compiler lays the header's structs out, against the generated ctypes classes:
    the field names come from the header text, the numbers from the compiler"""
    from cenet_amd import _lib
    bodies = dict((n, b) for b, n in re.findall(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", header_text()))
    assert sorted(bodies) == sorted(STRUCTS)
    fields = {n: [re.findall(r"\w+", d)[-1] for decl in b.split(";") if decl.strip() for d in decl.split(",")]
              for n, b in bodies.items()}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cenet_hip.h"', 'int main(void) {']
    for n, fs in fields.items():
        lines.append(f'  printf("{n} %zu\\n", sizeof({n}));')
        lines += [f'  printf("{n}.{f} %zu %zu\\n", offsetof({n}, {f}), sizeof((({n}*)0)->{f}));' for f in fs]
    lines += ['  return 0;', '}']
    (tmp_path / "probe.c").write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-DCENET_HOSTSIM_BUILD", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o",
                           str(tmp_path / "probe")])
    out = dict((k, [int(x) for x in v]) for k, *v in map(str.split, subprocess.check_output([str(tmp_path / "probe")], text=True)
                                                        .splitlines()))
    for n, fs in fields.items():
        cls = getattr(_lib, STRUCTS[n])
        assert [f for f, _ in cls._fields_] == fs, n
        assert [ctypes.sizeof(cls)] == out[n], n
        for f in fs:
            d = getattr(cls, f)
            assert [d.offset, d.size] == out[f"{n}.{f}"], (n, f)


def test_lib_binds_a_handle_put_in_its_place(monkeypatch):
    """whatever CDLL stands in `_lib._LIB` (the host checker's, loaded by a test helper) is typed before the package uses it"""
    from cenet_amd import _lib, build
    raw = ctypes.CDLL(build.build_hip(verbose=False))
    raw.cenet_zero_bytes.argtypes = None
    monkeypatch.setattr(_lib, "_LIB", raw)
    assert _lib.lib() is raw and raw.cenet_zero_bytes.argtypes == [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]


def test_wrong_argument_count_is_refused(hip_lib):
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        hip_lib.cenet_conv_direct_supported(32, 32, 5, 1)
    assert hip_lib.cenet_conv_direct_supported(32, 32, 5, 1, 2) in (0, 1)


def test_float_for_int_is_refused(hip_lib):
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        hip_lib.cenet_conv_direct_supported(32, 32, 5.0, 1, 2)


def test_wrong_struct_is_refused(hip_lib):
    from cenet_amd import _lib
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        hip_lib.cenet_diffattn_heads_fwd_bf16(ctypes.byref(_lib.AttnT()), 0)
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        hip_lib.cenet_diffattn_heads_fwd_bf16(_lib.AttnT(), 0)


def test_long_argument_arrives_intact(hip_lib):
    """no entry point returns a function of a `long` argument, so: the batch stride of cenet_bn_stats_f32 is typed long and its
    converter keeps all the bits of 2^31 + 8"""
    sb = hip_lib.cenet_bn_stats_f32.argtypes[1]
    assert sb is ctypes.c_long and ctypes.sizeof(sb) == 8
    assert repr(sb.from_param(2 ** 31 + 8)) == f"<cparam 'l' ({2 ** 31 + 8})>"
    assert ctypes.c_long(2 ** 31 + 8).value == 2 ** 31 + 8


def test_parser_refuses_unknown_spellings():
    from cenet_amd import _lib
    ok = "int cenet_x(const float* const* p, long n, cenet_stream_t stream);"
    assert _lib.parse_header(ok)[1] == {"cenet_x": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p])}
    for bad in ("int cenet_x(size_t n, cenet_stream_t stream);", "int cenet_x(long long n);", "int cenet_x(float);",
                "short cenet_x(int n);", "int cenet_x(cenet_mat_t m);", "int cenet_x(int n); int cenet_x(long n);"):
        with pytest.raises(ValueError, match="cenet_x"):
            _lib.parse_header(bad)


def test_integer_hyperparameters_convert_to_float(dev):
    """a Python int where the header says float (slope=1, eps=1) computes what the float does, bit for bit"""
    from cenet_amd import kern
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 8, 7, 7, generator=g).to(dev)
    w, b = torch.randn(8, 9, generator=g).to(dev), torch.randn(8, generator=g).to(dev)
    ys = []
    for slope in (1, 1.0, 0.25):
        y = torch.full_like(x, float("nan"))
        kern.dwact_fwd(x, w, b, y, "lrelu", slope, 1, 1, 8, 7, 7)
        ys.append(y.cpu())
    assert torch.equal(ys[0], ys[1]) and bool(torch.isfinite(ys[0]).all()) and not torch.equal(ys[0], ys[2])
    r = torch.randn(4, 8, generator=g).to(dev)
    gamma, beta = torch.randn(8, generator=g).to(dev), torch.randn(8, generator=g).to(dev)
    outs = []
    for eps in (1, 1.0, 1e-6):
        y, mean, rstd = torch.full_like(r, float("nan")), torch.empty(4, device=dev), torch.empty(4, device=dev)
        kern.layernorm_fwd(r, gamma, beta, y, mean, rstd, 4, 8, eps)
        outs.append((y.cpu(), rstd.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool(torch.isfinite(outs[0][0]).all()) and not torch.equal(outs[0][0], outs[2][0])
