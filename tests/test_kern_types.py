"""include/cenet_hip.h types the tensors of every launch: `_lib.parse_header` keeps what each pointer parameter points at, and
`kern._launch` / `kern._call` hold every tensor argument to the prototype of the entry point they call — before the device
check and before the library is touched, so none of this needs a GPU or a built library."""
import pytest
import torch

from cenet_amd import _lib, kern

BF16 = torch.bfloat16


def test_every_pointer_parameter_has_a_tensor_type():
    assert len(_lib.PARAMS) == len(_lib.PROTOS) >= 200
    pointers = 0
    for name, (_, argtypes) in _lib.PROTOS.items():
        params = _lib.PARAMS[name]
        assert len(params) == len(argtypes), name
        for pname, kind in params:
            assert pname.isidentifier(), (name, pname)
            if kind not in (None, _lib.PTR_PTR, _lib.STRUCT_PTR):  # a single-level data pointer
                pointers += 1
                want = kern._DTYPE_OF[kind]
                assert want is kern._ANY if kind == "void" else isinstance(want, torch.dtype), (name, pname, kind)
    assert pointers >= 1000
    assert _lib.PARAMS["cenet_layernorm_fwd_bf16"][:3] == (("x", "unsigned short"), ("gamma", "float"), ("beta", "float"))
    assert _lib.PARAMS["cenet_dwbn_fwd_f32"][2] == ("w", _lib.PTR_PTR) and _lib.PARAMS["cenet_gemm_f32"][0] == ("A", _lib.STRUCT_PTR)
    assert _lib.PARAMS["cenet_vol_resize_cubic"][1] == ("stage", "double") and _lib.PARAMS["cenet_gemm_last_kernel"] == ()


def test_every_launch_has_its_expectations_precomputed():
    for name, params in _lib.PARAMS.items():
        if params and params[-1][0] == "stream":
            want, twin, want16 = kern._EXPECT[name]
            assert len(want) == len(want16) == len(params) - 1, name
            assert twin == name or (name.endswith("_f32") and twin == name[:-4] + "_bf16" and twin in _lib.PARAMS), name


def _ln(x, gamma, y):
    rows, Cn = x.shape
    kern.layernorm_fwd(x, gamma, torch.zeros(Cn), y, torch.zeros(rows), torch.zeros(rows), rows, Cn, 1e-5)


def test_bf16_parameter_beside_bf16_activations_is_refused():
    x, y = torch.zeros(4, 8, dtype=BF16), torch.zeros(4, 8, dtype=BF16)
    with pytest.raises(TypeError) as e:
        _ln(x, torch.ones(8, dtype=BF16), y)
    for word in ("cenet_layernorm_fwd_bf16", "gamma", "torch.float32", "torch.bfloat16"):
        assert word in str(e.value), str(e.value)


def test_mixed_activation_types_are_refused():
    with pytest.raises(TypeError, match="cenet_layernorm_fwd_bf16.*`x`"):
        _ln(torch.zeros(4, 8), torch.ones(8), torch.zeros(4, 8, dtype=BF16))


def test_fp64_activation_is_refused():
    x = torch.zeros(16, dtype=torch.float64)
    with pytest.raises(TypeError, match="cenet_act_fwd_f32.*torch.float64"):
        kern.act_fwd(x, torch.zeros(16), 16, "relu")


def test_fp64_stage_is_what_the_header_declares():
    """the float64 scratch of the cubic resize passes the type check (the old allow-list had to skip it); what stops the call
    here is the device"""
    n, H, W, PH, PW = 1, 4, 4, 8, 8
    src, out = torch.zeros(n, H, W), torch.zeros(n, 1, PH, PW)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kern.vol_resize_cubic(src, torch.zeros(n * H * W, dtype=torch.float64), out, n, H, W, PH, PW)
    with pytest.raises(TypeError, match="cenet_vol_resize_cubic.*`stage`.*torch.float64.*torch.float32"):
        kern.vol_resize_cubic(src, torch.zeros(n * H * W), out, n, H, W, PH, PW)


def test_well_typed_cpu_tensors_meet_the_device_check():
    assert not _lib.is_hostsim()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _ln(torch.zeros(4, 8), torch.ones(8), torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _ln(torch.zeros(4, 8, dtype=BF16), torch.ones(8), torch.zeros(4, 8, dtype=BF16))


def test_type_errors_come_before_the_device_check():
    """a wrongly typed call is wrong on any device: the fp64 `y` AFTER the well-typed host tensor `x` still decides"""
    with pytest.raises(TypeError, match="`y`"):
        kern.act_fwd(torch.zeros(16), torch.zeros(16, dtype=torch.float64), 16, "relu")


def test_tensor_where_the_header_has_an_array_of_pointers_is_refused():
    f = torch.zeros(8)
    args = [f, 8, f, None, 1, 1, 0, f, 8, None, 0, f, f, 1e-5, f, f, None, None, 0.1, None, 1, 1, 8]
    assert len(args) == len(_lib.PARAMS["cenet_dwbn_fwd_f32"]) - 1
    with pytest.raises(TypeError, match="cenet_dwbn_fwd_f32: `w` takes no tensor"):
        kern._call("cenet_dwbn_fwd_f32", *args)
    with pytest.raises(TypeError, match="cenet_gemm_f32: `A` takes no tensor"):
        kern._launch("cenet_gemm_f32", f, None, None, 1, 1, 1, 1, 1, 1, 1)


def test_unknown_pointee_spelling_raises():
    with pytest.raises(ValueError, match="cenet_x"):
        _lib.parse_header("int cenet_x(const short* p, cenet_stream_t stream);")
    _, _, params = _lib.parse_header("int cenet_x(const char* p, cenet_stream_t stream);")
    assert params == {"cenet_x": (("p", "char"), ("stream", None))}  # (the parser knows `char`; no tensor type stands for it)
    assert "char" not in kern._DTYPE_OF
