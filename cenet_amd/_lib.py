"""ctypes loader for libcenet_hip.so — the hand-written gfx950 kernel library.

There is NO fallback: if the library is missing (or a tensor is not on the GPU) the product path raises.
(`tests/hostsim` may point `_LIB` at a g++ build of the same kernel sources running on a SIMT interpreter to
check kernel logic without a GPU; nothing in the package does that.)

include/cenet_hip.h is the one declaration of the C ABI: `parse_header` reads the five argument structs and every prototype
from it, `bind` gives each entry point of a loaded library its `restype` / `argtypes`.  Callers pass plain Python values; a
missing argument or one of the wrong kind raises instead of launching.  ctypes sees every data pointer as `void*`; what a pointer
points AT is kept beside the prototypes (`PARAMS`), and cenet_amd/kern.py holds the tensors of every launch to it.  This module
stays free of torch.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcenet_hip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "cenet_hip.h")

_LIB = None
_HOSTSIM = False  # set only by tests/hostsim

_SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "unsigned": C.c_uint,
            "cenet_stream_t": C.c_void_p}
_POINTEES = {"void", "char", "unsigned char", "unsigned short", "unsigned", "int", "long", "float", "double"}
_TYPE_WORDS = {w for t in (*_SCALARS, *_POINTEES) for w in t.split()} | {"short", "signed"}
_RETURNS = {"int": C.c_int, "long": C.c_long, "const char *": C.c_char_p}
_STRUCTS = {"cenet_mat_t": "MatT", "cenet_epi_t": "EpiT", "cenet_wgrad_prob_t": "WgradProbT", "cenet_attn_t": "AttnT",
            "cenet_diffattn_t": "DiffAttnT"}


PTR_PTR, STRUCT_PTR = "**", "struct*"  # parameter kinds that take no tensor: an array of pointers, an argument struct


def _ctype(decl: str, structs, where: str):
    """(ctypes type, name, kind) of one declarator with its type, `const float* const* x` or `long sb`; kind: the pointee
    spelling of a single-level data pointer ("float", "unsigned short", ...), PTR_PTR, STRUCT_PTR, None for a scalar"""
    toks = decl.replace("*", " * ").split()
    words = [t for t in toks if t not in ("*", "const")]
    if len(words) < 2 or toks[-1] != words[-1] or words[-1] in _TYPE_WORDS:  # (every parameter and field is named)
        raise ValueError(f"cenet_hip.h: cannot read `{decl.strip()}` in {where}")
    base, stars = " ".join(words[:-1]), toks.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base], words[-1], None
    if stars == 1 and base in structs:
        return C.POINTER(structs[base]), words[-1], STRUCT_PTR
    if stars and base in _POINTEES:
        return C.c_void_p, words[-1], (base if stars == 1 else PTR_PTR)
    raise ValueError(f"cenet_hip.h: unknown type `{decl.strip()}` in {where}")


def parse_header(text: str):
    """(structs, protos, params) of a header text: {C struct name: ctypes.Structure subclass} for the `typedef struct { ... } name;`
    bodies, {symbol: (restype, [argtypes])} for the prototypes and {symbol: ((parameter name, kind), ...)} with the kinds of
    `_ctype`.  A spelling it does not know raises; it never guesses."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    structs = {}

    def struct(m):
        body, cname, fields = m.group(1), m.group(2), []
        for decl in filter(str.strip, body.split(";")):  # `type a, b, *c`
            first, *rest = decl.split(",")
            base = " ".join(first.replace("*", " * ").split()[:-1]).rstrip("* ")
            fields += [_ctype(d, {}, cname)[1::-1] for d in (first, *(f"{base} {d}" for d in rest))]
        structs[cname] = type(_STRUCTS.get(cname, cname), (C.Structure,),
                              {"_fields_": fields, "__doc__": f"{cname} (include/cenet_hip.h)."})
        return " "

    text = re.sub(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"typedef[^;]*;", " ", text)
    protos, params_of = {}, {}
    for ret, name, params in re.findall(r"([^;{}()]+?)\b(\w+)\s*\(([^()]*)\)\s*;", text):
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in _RETURNS:
            raise ValueError(f"cenet_hip.h: unknown return type `{ret}` of {name}")
        params = [] if params.strip() in ("", "void") else params.split(",")
        decls = [_ctype(p, structs, name) for p in params]
        proto = (_RETURNS[ret], [d[0] for d in decls])
        if protos.setdefault(name, proto) != proto:
            raise ValueError(f"cenet_hip.h: {name} is declared twice, differently")
        params_of[name] = tuple(d[1:] for d in decls)
    return structs, protos, params_of


with open(HEADER_PATH) as _f:
    _STRUCT_TYPES, PROTOS, PARAMS = parse_header(_f.read())
MatT, EpiT, WgradProbT, AttnT, DiffAttnT = (_STRUCT_TYPES[c] for c in _STRUCTS)


_BOUND = None  # the handle `lib()` last returned


def bind(lib):
    """type every entry point of include/cenet_hip.h that `lib` exports (a symbol it lacks is skipped: tests/test_abi.py holds the
    real library to the full list)"""
    for name, (restype, argtypes) in PROTOS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def lib():
    """Return the loaded kernel library, loading it on first use. Raises if it has not been built.
    A handle someone else put into `_LIB` (tests/hostsim) is bound here before its first use: callers pass plain Python values,
    and an untyped function would take a 64-bit pointer for an int."""
    global _LIB, _BOUND
    if _LIB is not _BOUND or _LIB is None:
        if _LIB is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"{LIB_PATH} not found: the HIP kernel library is required (no CPU/PyTorch fallback exists). "
                    "Build it with `python -m cenet_amd.build` (hipcc --offload-arch=gfx950).")
            _LIB = C.CDLL(LIB_PATH)
        _BOUND = bind(_LIB) if isinstance(_LIB, C.CDLL) else _LIB  # (flops._Recorder is no CDLL and takes anything)
    return _LIB


def is_hostsim() -> bool:
    return _HOSTSIM


def check(rc: int, name: str):
    if rc != 0:
        raise RuntimeError(f"libcenet_hip: {name} failed with error code {rc}")
