"""skip_mode='add' (reference dseb.py:89-118,153-165; --skip_mode of main_acdc.py / main_synapse.py / main_skin.py): every DSEB
joins `dec + skip` on C channels instead of concatenating to 2C.

  constructor / schema (CPU): the product draws the reference's weights bit for bit under the same torch seed, keeps its
      state-dict layout, round-trips through cenet_amd.checkpoint, refuses unknown modes
  kernels (host SIMT checker and MI355X): the add join (ops.add2) bit-exact against torch; the differential-attention pair
      kernels at the new head dims 4 and 40 against an fp32 softmax, with canary-filled outputs (nothing past the real columns)
  parity (MI355X, fp32): three DSEB module fixtures, the ACDC / Synapse add models (eval, loss, gradients, two SGD steps)
  bf16 mode, path census, graph replay (MI355X)
Fixtures: tools/gen_golden_skip_add.py (the unmodified reference, CPU)."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch

from backend import BACKENDS, use_hip, use_sim
from oracle import cenet_oracle as O
from oracle.gen_golden_keys import PROBE_BUFFERS, PROBE_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

MODEL_KW = {
    "acdc_add": dict(input_channels=1, num_classes=4, scale_factors=[1.0, 0.5], diffatt_num_heads=[4, 4, 4],
                     out_up_block="upcn", skip_mode="add"),
    "synapse_add": dict(input_channels=1, num_classes=9, scale_factors=[0.8, 0.4], diffatt_num_heads=[16, 8, 8],
                        out_up_block="upcn", skip_mode="add"),
}
DSEB_KW = {
    "dseb_add": dict(dim=80, scale_factors=[1.0, 0.5], num_heads=1, input_size=12, mode="add", depth=4),
    "dseb_add_hd10": dict(dim=80, scale_factors=[0.8, 0.4], num_heads=4, input_size=10, mode="add", depth=4),
    "dseb_add_hd4": dict(dim=64, scale_factors=[0.8, 0.4], num_heads=8, input_size=10, mode="add", depth=2),
}


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def _check_ctor(sd, z):
    """per-tensor float64 sum and absolute sum of the constructor's weights against the reference's (the tolerance
    tests/test_wellcond.py pins the cat-mode initialisation with)"""
    keys = [str(k) for k in z["ck_keys"]]
    assert list(sd.keys()) == keys
    for k, ref in zip(keys, z["ck_sum"]):
        v = sd[k].double()
        np.testing.assert_allclose([v.sum().item(), v.abs().sum().item()], ref, rtol=1e-11, atol=1e-13, err_msg=k)


def _product(name, ctor_seed):
    """CENet(skip_mode='add') of preset `name` built under the fixture's constructor seed"""
    from cenet_amd.networks import CENet
    torch.manual_seed(ctor_seed)
    net = CENet(**MODEL_KW[name])
    return net


# ---------------------------------------------------------------------------------------------------------------------------------
# constructor, schema, checkpoint (CPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_add_mode_builds_in_either_case_and_refuses_unknown_modes():
    from cenet_amd.networks import CENet
    from cenet_amd.networks.cenet.modules.dseb import DSEBlock
    for mode in ("add", "ADD"):
        net = CENet(**dict(MODEL_KW["acdc_add"], skip_mode=mode))
        assert net.decoder.skip_enhancer3.mode == "add"
        assert net.decoder.skip_enhancer3.mixer.weight.shape == (320, 320, 1, 1)
    with pytest.raises(ValueError, match="mode"):
        CENet(**dict(MODEL_KW["acdc_add"], skip_mode="foo"))
    with pytest.raises(ValueError, match="mode"):
        DSEBlock(dim=8, scale_factors=[1.0, 0.5], num_heads=2, input_size=8, mode="foo")
    with pytest.raises(NotImplementedError):
        DSEBlock(dim=8, scale_factors=[1.0, 0.5], num_heads=2, input_size=8, mode="add", use_command="dog")
    # the reference's own default: a bare DSEBlock / Decoder is in add mode
    assert DSEBlock(dim=8, scale_factors=[1.0, 0.5], num_heads=2, input_size=8).mode == "add"


def test_state_dict_matches_the_reference_schema():
    from cenet_amd.networks import CENet
    ref = json.load(open(os.path.join(GOLDEN, "schema_acdc_add.json")))
    mine = {k: list(v.shape) for k, v in CENet(**MODEL_KW["acdc_add"]).state_dict().items()}
    assert list(mine) == list(ref)
    assert mine == ref


@pytest.mark.parametrize("fixture,name", [("model_acdc_add.npz", "acdc_add"), ("model_synapse_add.npz", "synapse_add"),
                                          ("model_acdc_add_64.npz", "acdc_add")])
def test_constructor_draws_the_reference_weights(fixture, name):
    z = _load(fixture)
    net = _product(name, int(z["ctor_seed"]))
    _check_ctor(net.state_dict(), z)


@pytest.mark.parametrize("case", list(DSEB_KW))
def test_dseb_constructor_draws_the_reference_weights(case):
    from cenet_amd.networks.cenet.modules.dseb import DSEBlock
    z = _load(f"mod_{case}.npz")
    torch.manual_seed(int(z["ctor_seed"]))
    sd = DSEBlock(**DSEB_KW[case]).state_dict()
    _check_ctor(sd, z)
    for k, v in sd.items():
        assert torch.equal(v, torch.from_numpy(z["sd." + k])), k


def test_checkpoint_round_trip_is_strict(tmp_path):
    from cenet_amd import checkpoint
    from cenet_amd.networks import CENet
    a = CENet(**MODEL_KW["acdc_add"])
    O.fill_state_dict_(a.state_dict(), seed=11)
    p = str(tmp_path / "add.pth")
    checkpoint.save_weights(a, p)
    b = CENet(**MODEL_KW["acdc_add"])
    checkpoint.load_weights(b, p, strict=True)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    with pytest.raises(RuntimeError):  # a cat-mode model does not take an add-mode checkpoint
        checkpoint.load_weights(CENet(**dict(MODEL_KW["acdc_add"], skip_mode="cat")), p, strict=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# host checker: the whole add-mode model at 64 x 64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.slow
def test_small_add_model_forward_on_host_checker():
    from cenet_amd import _lib
    z = _load("model_acdc_add_64.npz")
    use_sim()
    try:
        net = _product("acdc_add", int(z["ctor_seed"]))
        _check_ctor(net.state_dict(), z)
        O.fill_state_dict_(net.state_dict(), seed=int(z["fill_seed"]), layer_scale=float(z["layer_scale"]))
        net.eval()
        x = torch.randn(1, 1, 64, 64, generator=torch.Generator().manual_seed(int(z["x_seed"])))
        with torch.no_grad():
            got = net(x)
        torch.testing.assert_close(got, torch.from_numpy(z["logits"]), rtol=1e-3, atol=1e-3)
    finally:
        _lib._LIB = None
        _lib._HOSTSIM = False


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels on both backends
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=BACKENDS)
def dev(request):
    from cenet_amd import _lib
    d = use_sim() if request.param == "sim" else use_hip()
    yield d
    _lib._LIB = None
    _lib._HOSTSIM = False


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,offset", [(2 * 64 * 56 * 56 + 0, 0), (4099, 0), (1003, 1)])
def test_add_join_is_bit_exact(dev, dtype, n, offset):
    from cenet_amd import kern
    g = torch.Generator().manual_seed(n)
    a, b, gy, ga, gb = (torch.randn(n + offset, generator=g).to(dtype).to(dev)[offset:] for _ in range(5))
    y = torch.empty_like(a)
    kern.add2_fwd(a, b, y, n)
    assert torch.equal(y.cpu(), (a.cpu() + b.cpu()))
    for ta, tb in ((None, None), (ga, None), (None, gb), (ga, gb)):
        da, db = torch.full_like(a, 7.0), torch.full_like(a, 7.0)
        kern.add2_bwd(gy, ta, tb, da, db, n)
        assert torch.equal(da.cpu(), gy.cpu() if ta is None else gy.cpu() + ta.cpu())
        assert torch.equal(db.cpu(), gy.cpu() if tb is None else gy.cpu() + tb.cpu())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_add2_autograd_routes_the_taps(dev, dtype):
    """y = a + b with a second consumer on each input (the decoder's residual on dec, the mixer's on skip): one backward launch"""
    from cenet_amd import kern, ops
    g = torch.Generator().manual_seed(5)
    a0, b0, gy, ga, gb = (torch.randn(2, 8, 5, 7, generator=g).to(dtype) for _ in range(5))
    a, b = a0.to(dev).requires_grad_(True), b0.to(dev).requires_grad_(True)
    calls = []
    orig = kern.add2_bwd
    kern.add2_bwd = lambda *x: (calls.append(1), orig(*x))[1]
    try:
        y, at, bt = ops.add2(a, b, tap=True)
        torch.autograd.backward([y, at, bt], [gy.to(dev), ga.to(dev), gb.to(dev)])
    finally:
        kern.add2_bwd = orig
    assert len(calls) == 1
    assert y.dtype == dtype and torch.equal(y.detach().cpu(), a0 + b0)
    assert torch.equal(a.grad.cpu(), gy + ga) and torch.equal(b.grad.cpu(), gy + gb)


def _pair_case(dev, B, N, H, hd, seed):
    """bf16 q, k, v with random values, canary-filled outputs: U, dq, dk, dv from the pair kernels and the fp32 reference"""
    from cenet_amd import kern
    E = 2 * H * hd
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, N, E, generator=g).bfloat16() for _ in range(3))
    dU = torch.randn(B, 2 * H, N, 2 * hd, generator=g).bfloat16()
    canary = -12352.0  # exact in bf16
    U = torch.full((B, 2 * H, N, 2 * hd), canary, dtype=torch.bfloat16, device=dev)
    lse = torch.empty((B, 2 * H, N), device=dev)
    qd, kd, vd, dUd = (t.to(dev) for t in (q, k, v, dU))
    a = kern.DiffAttnT()
    a.q, a.k, a.v, a.U, a.lse = qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), U.data_ptr(), lse.data_ptr()
    a.B, a.H, a.N, a.hd, a.scale = B, H, N, hd, hd ** -0.5
    kern.diffattn_heads(a, backward=False)
    # the gradients land inside canary-filled buffers one row longer on each side: nothing is written past the real rows
    pad = E
    bufs = [torch.full((B * N * E + 2 * pad,), canary, dtype=torch.bfloat16, device=dev) for _ in range(3)]
    dq, dk, dv = (t[pad:pad + B * N * E] for t in bufs)
    ws = torch.empty(kern.diffattn_heads_ws_bytes(B, H, N), dtype=torch.uint8, device=dev)
    a.dU, a.dq, a.dk, a.dv, a.ws = dUd.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr()
    kern.diffattn_heads(a, backward=True)
    for t in bufs:
        assert (t[:pad].float() == canary).all() and (t[pad + B * N * E:].float() == canary).all()
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    qh = qf.view(B, N, 2 * H, hd).transpose(1, 2)
    kh = kf.view(B, N, 2 * H, hd).transpose(1, 2)
    vh = vf.view(B, N, H, 2 * hd).transpose(1, 2).repeat_interleave(2, dim=1)
    ref = torch.softmax(qh @ kh.transpose(-1, -2) * hd ** -0.5, dim=-1) @ vh
    ref.backward(dU.float())
    return (U.cpu(), dq.cpu().view(B, N, E), dk.cpu().view(B, N, E), dv.cpu().view(B, N, E)), \
        (ref.detach(), qf.grad, kf.grad, vf.grad)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))


@pytest.mark.parametrize("hd,H,N_hip,N_sim", [(4, 8, 3136, 70), (40, 4, 196, 45)])
def test_pair_kernels_new_head_dims(dev, hd, H, N_hip, N_sim):
    """hd 4 (Synapse add, 56 x 56: two heads per 16-byte pair row) and hd 40 (ACDC add, 14 x 14: HDP = 48 tiles); tolerances of
    tests/test_attention_presets.py.  Every output element is written (no canary left) and none past the tensors."""
    from cenet_amd import kern
    assert kern.diffattn_heads_supported(hd, 1)
    N = N_hip if dev.type == "cuda" else N_sim
    B = 2 if dev.type == "cuda" else 1
    got, ref = _pair_case(dev, B, N, H, hd, seed=hd)
    for x in got:
        assert not (x.float() == -12352.0).any()
    assert _rel(got[0], ref[0]) < 2e-2
    for a, b in zip(got[1:], ref[1:]):
        assert _rel(a, b) < 3e-2


def test_pair_kernel_head_dims_gate():
    """hd 4 and 40 are new; hd 10 stays on the tiled flash path (its pair rows are 40 bytes, not 16-byte aligned); 20 and 80 keep
    their paths (tests/test_path_census.py)"""
    from cenet_amd import kern
    sup = [hd for hd in range(1, 161) if kern.diffattn_heads_supported(hd, 196)]
    assert sup == [4, 8, 16, 32, 40, 64]


# ---------------------------------------------------------------------------------------------------------------------------------
# parity (fp32 parity mode)
# ---------------------------------------------------------------------------------------------------------------------------------
def _close(a, b, rtol=1e-3, atol=None, what=""):
    a = a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else a
    scale = max(1.0, float(np.abs(b).max()))
    np.testing.assert_allclose(a, b, rtol=rtol, atol=(atol if atol is not None else 2e-4 * scale), err_msg=what)


@pytest.mark.parametrize("case", list(DSEB_KW))
def test_dseb_add_module_parity(dev, case):
    """the tolerances tests/test_modules_parity.py holds mod_dseb*.npz to"""
    from cenet_amd.networks.cenet.modules.dseb import DSEBlock
    z = _load(f"mod_{case}.npz")
    m = DSEBlock(**DSEB_KW[case]).to(dev)
    sd = {k[3:]: torch.from_numpy(z[k]).to(dev) for k in z.files if k.startswith("sd.")}
    m.load_state_dict(sd, strict=True)
    ins = [torch.from_numpy(z[f"in{i}"]).to(dev) for i in range(2)]
    m.eval()
    with torch.no_grad():
        _close(m(ins[0], ins[1]), z["out_eval"], what="eval output")
    m.train()
    ins_t = [t.clone().requires_grad_(True) for t in ins]
    out = m(ins_t[0], ins_t[1])
    _close(out, z["out"], what="train output")
    out.backward(torch.from_numpy(z["cot"]).to(dev))
    for i, t in enumerate(ins_t):
        _close(t.grad, z[f"gin{i}"], rtol=2e-3, what=f"grad input {i}")
    params = dict(m.named_parameters())
    for k in z.files:
        if k.startswith("gsd."):
            _close(params[k[4:]].grad, z[k], rtol=2e-3, what=k)


def _build_model(name, dev):
    z = _load(f"model_{name}.npz")
    net = _product(name, int(z["ctor_seed"]))  # (the fill overwrites every tensor: the constructor check is a CPU test)
    O.fill_state_dict_(net.state_dict(), seed=int(z["fill_seed"]), layer_scale=float(z["layer_scale"]))
    kw = MODEL_KW[name]
    x, lab = O.synthetic_batch(2, kw["input_channels"], kw["num_classes"], seed=int(z["x_seed"]))
    return net.to(dev), z, x.to(dev), lab.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODEL_KW))
def test_add_model_eval_parity(name):
    dev = use_hip()
    net, z, x, lab = _build_model(name, dev)
    K = MODEL_KW[name]["num_classes"]
    net.eval()
    with torch.no_grad():
        le = net(x).cpu()
    np.testing.assert_allclose(le[:, :, ::9, ::9].numpy(), z["logits_eval_sub"], rtol=1e-3, atol=1e-3)
    assert abs(le.double().sum().item() - float(z["logits_eval_sum"])) < 1e-4 * float(z["logits_eval_abs"])
    assert (O.predict(le)[:, ::5, ::5].numpy() != z["pred_eval_sub"]).mean() < 1e-3
    assert abs(O.mean_class_dice(le, lab.cpu(), K) - float(z["dice_eval"])) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODEL_KW))
def test_add_model_train_two_sgd_steps(name):
    """the budgets of test_model_parity.py::test_model_train_two_sgd_steps"""
    from cenet_amd import losses, optim
    dev = use_hip()
    net, z, x, lab = _build_model(name, dev)
    K = MODEL_KW[name]["num_classes"]
    net.train()
    net.backbone.reset_drop_path(0.0)
    arena = optim.ParamArena(net, optim.cenet_segments())
    opt = optim.FusedSGD(arena, lr=0.01, momentum=0.9, weight_decay=1e-4)
    crit = losses.Criterion(K, argparse.Namespace(loss_type="dice,ce", loss_weights="0.5,0.5"))
    params = dict(net.named_parameters())
    bufs = dict(net.named_buffers())
    for step, (lk, pk) in enumerate((("loss", "p1."), ("loss2", "p2."))):
        opt.zero_grad()
        lt = net(x)
        loss = crit(lt, lab)
        loss.backward()
        assert abs(loss.item() - float(z[lk])) < 2e-4, (loss.item(), float(z[lk]))
        if step == 0:
            np.testing.assert_allclose(lt.detach().cpu()[:, :, ::9, ::9].numpy(), z["logits_train_sub"], rtol=1e-3, atol=1e-3)
            for k in PROBE_KEYS:
                g = params[k].grad.reshape(-1).cpu()
                n32, n64, nmine = float(z["g." + k + ".norm"]), float(z["g64." + k + ".norm"]), g.double().norm().item()
                rel = 2e-2 if g.numel() == 1 else 3e-3
                assert abs(nmine - n64) <= 6.0 * abs(n32 - n64) + rel * n64 + 1e-7, (k, nmine, n32, n64)
                g64, g32 = z["g64." + k + ".head"], z["g." + k + ".head"].astype(np.float64)
                budget = 6.0 * np.abs(g32 - g64).max() + (rel / 3) * np.abs(g64).max() + 1e-9
                assert np.abs(g[:16].double().numpy() - g64).max() <= budget, k
            for k in PROBE_BUFFERS:
                np.testing.assert_allclose(bufs[k].reshape(-1)[:16].cpu().numpy(), z["b." + k], rtol=1e-3, atol=1e-5, err_msg=k)
        opt.step()
        for k in PROBE_KEYS:
            np.testing.assert_allclose(params[k].detach().reshape(-1)[:16].cpu().numpy(), z[pk + k + ".head"], rtol=1e-3,
                                       atol=3e-5, err_msg=pk + k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODEL_KW))
def test_add_model_bf16_mode_stays_close_to_fp32_goldens(name):
    """test_bf16_mode.py's bounds for cat mode: mean |dlogit| < 2 % of the logit range, < 1 % mask flips, Dice within 1e-3 —
    with two differences forced by the fixtures, not by the kernels.  The add-mode fixtures (layer scales 0.02, see
    tools/gen_golden_skip_add.py) have many near-tied pixels: the top two fp32 logits lie within 2 % of the range of each other
    at 2.6 % (ACDC) / 15.6 % (Synapse) of the sampled pixels, against 1.4 % / 0.9 % in model_{acdc,synapse}.npz.  A bf16 logit
    error of 0.5 % of the range (measured) flips some of those: flips are counted where the fp32 margin is >= 2 % of the range,
    and Dice (0.16 / 0.07 on these fixtures, every flip moves it) gets 2e-3 (measured on the MI355X: 1.2e-3 / 1.7e-6)."""
    from cenet_amd import kern
    dev = use_hip()
    net, z, x, lab = _build_model(name, dev)
    net.eval()
    old = kern.set_compute_bf16(True)
    try:
        with torch.no_grad():
            le = net(x)
        assert le.dtype == torch.bfloat16
        le = le.float().cpu()
    finally:
        kern.set_compute_bf16(old)
    ref = z["logits_eval_sub"]
    rng = np.abs(ref).max()
    diff = np.abs(le[:, :, ::9, ::9].numpy() - ref)
    flip = O.predict(le)[:, ::5, ::5].numpy() != z["pred_eval_sub"]
    # margins need the golden's logits: they are stored on the ::9 grid, so the margin-filtered flips are counted there
    top = np.sort(ref, axis=1)
    clear = (top[:, -1] - top[:, -2]) >= 0.02 * rng
    flip9 = O.predict(le)[:, ::9, ::9].numpy() != np.argmax(ref, axis=1)
    ddice = abs(O.mean_class_dice(le, lab.cpu(), MODEL_KW[name]["num_classes"]) - float(z["dice_eval"]))
    print(f"[bf16 eval {name}] mean|dlogit|/range {diff.mean() / rng:.4f}  mask flips {flip.mean():.4f} (all)  "
          f"{flip9[clear].mean():.4f} (margin >= 2 %)  dDice {ddice:.2e}")
    assert diff.mean() < 0.02 * rng
    assert flip9[clear].mean() < 1e-2
    assert ddice < 2e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# path census (bf16, baseline batches), as tests/test_path_census.py counts it
# ---------------------------------------------------------------------------------------------------------------------------------
class _AtenAdds(torch.utils._python_dispatch.TorchDispatchMode):
    """counts aten::add calls (forward and the autograd engine's gradient sums), and those inside a DSEB's forward"""

    def __init__(self, inside):
        super().__init__()
        self.inside, self.total, self.in_block = inside, 0, 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func.overloadpacket in (torch.ops.aten.add, torch.ops.aten.add_):
            self.total += 1
            self.in_block += bool(self.inside["n"])
        return func(*args, **(kwargs or {}))


def mode_census(preset, skip_mode):
    import bench
    import test_path_census as PC
    from cenet_amd import kern
    from cenet_amd.networks import CENet
    from cenet_amd.networks.cenet.modules import dseb

    def make_model(dev, cfg=None):
        cfg = cfg or bench.CONFIGS["acdc"]
        torch.manual_seed(1234)
        net = CENet(input_channels=cfg["in_ch"], num_classes=cfg["classes"], scale_factors=cfg["scales"],
                    diffatt_num_heads=cfg["heads"], skip_mode=skip_mode, out_up_block="upcn")
        return net.to(dev).train()

    inside = {"n": 0}
    cats = {"n": 0}
    orig_fwd, orig_cat, orig_make = dseb.DSEBlock.forward, kern.cat_channels, bench.make_model

    def fwd(self, skip, dec):
        inside["n"] += 1
        try:
            return orig_fwd(self, skip, dec)
        finally:
            inside["n"] -= 1

    def cat(*a, **k):
        cats["n"] += bool(inside["n"])
        return orig_cat(*a, **k)

    bench.make_model, dseb.DSEBlock.forward, kern.cat_channels = make_model, fwd, cat
    try:
        with _AtenAdds(inside) as adds:
            counts = PC.census(preset)
    finally:
        bench.make_model, dseb.DSEBlock.forward, kern.cat_channels = orig_make, orig_fwd, orig_cat
    return counts, cats["n"], adds


ADD_EXPECT = {
    "acdc": {"dattn_pairs_fwd_hd40": 1, "dattn_pairs_bwd_hd40": 1, "dattn_pairs_fwd_hd16": 1, "dattn_pairs_bwd_hd16": 1,
             "dattn_pairs_fwd_hd8": 1, "dattn_pairs_bwd_hd8": 1, "add2_fwd_f32": 3, "add2_bwd_f32": 3,
             "flash_fwd": 0, "flash_bwd": 0},
    "synapse": {"dattn_pairs_fwd_hd8": 1, "dattn_pairs_bwd_hd8": 1, "dattn_pairs_fwd_hd4": 1, "dattn_pairs_bwd_hd4": 1,
                "add2_fwd_f32": 3, "add2_bwd_f32": 3,
                "flash_fwd": 1, "flash_bwd": 1},  # DSEB3: hd 10 on the tiled flash kernels
}


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["acdc", "synapse"])
def test_add_mode_fast_paths_taken_at_the_baseline_batch(preset):
    got, cats, adds = mode_census(preset, "add")
    bad = {k: (got.get(k, 0), v) for k, v in ADD_EXPECT[preset].items() if got.get(k, 0) != v}
    assert not bad, f"{preset} add: (taken, expected) per entry point: {bad}"
    assert cats == 0 and adds.in_block == 0, (cats, adds.in_block)
    # the join's gradients meet in add2_bwd: the step runs no more aten::add than the cat-mode step does
    _, _, adds_cat = mode_census(preset, "cat")
    assert adds.total <= adds_cat.total, (adds.total, adds_cat.total)


# ---------------------------------------------------------------------------------------------------------------------------------
# graph replay
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_add_mode_graph_replay_trains_like_eager():
    """a captured add-mode step (graph.GraphedStep) over four steps on changing batches matches eager launches, up to the order of
    fp32 atomics (the bounds tests/test_graph_replay.py holds cat mode to)"""
    import copy
    from cenet_amd import kern, losses, ops, optim
    from cenet_amd.graph import GraphedStep
    from cenet_amd.networks import CENet
    dev = torch.device("cuda:0")
    old_bf, old_ov = kern.set_compute_bf16(True), ops.set_wgrad_overlap(True)
    try:
        torch.manual_seed(3)
        base = CENet(**MODEL_KW["acdc_add"]).to(dev).train()
        for m in base.modules():
            if hasattr(m, "drop_prob"):
                m.drop_prob = 0.0
        B = 4
        g = torch.Generator().manual_seed(7)
        batches = [(torch.randn(B, 1, 224, 224, generator=g), torch.randint(0, 4, (B, 224, 224), generator=g).float())
                   for _ in range(3)]

        def run(net, graphed):
            arena = optim.ParamArena(net, optim.cenet_segments())
            opt = optim.FusedSGD(arena, lr=0.01, momentum=0.9, weight_decay=1e-4)
            crit = losses.Criterion(4, argparse.Namespace(loss_type="dice,ce", loss_weights="0.5,0.5"))
            x, lab = batches[0][0].to(dev), batches[0][1].to(dev)  # static inputs, refilled per step

            def body():
                opt.zero_grad()
                loss = crit(net(x), lab)
                loss.backward()
                opt.step(sync_hyper=False)
                return loss

            out = []
            step = GraphedStep(body, optimizer=opt, warmup=1) if graphed else None
            # (GraphedStep's warm-up + capture train two steps on batch 0; the eager run does the same)
            if not graphed:
                for _ in range(2):
                    opt.prepare()
                    body()
            for xb, lb in batches[1:3]:
                x.copy_(xb.to(dev))
                lab.copy_(lb.to(dev))
                if graphed:
                    out.append(float(step().detach()))
                else:
                    opt.prepare()
                    out.append(float(body().detach()))
            torch.cuda.synchronize()
            return out, arena.params.clone()

        le, pe = run(base, False)
        lg, pg = run(copy.deepcopy(base), True)
        assert all(np.isfinite(lg))
        for a, b in zip(le, lg):
            assert abs(a - b) <= 2e-2 * max(1.0, abs(a)), (le, lg)
        cos = torch.nn.functional.cosine_similarity((pe - pe.mean()).flatten(), (pg - pg.mean()).flatten(), dim=0).item()
        rel = ((pe - pg).norm() / pe.norm()).item()
        assert cos > 0.9999 and rel < 2e-3, (cos, rel)
    finally:
        kern.set_compute_bf16(old_bf)
        ops.set_wgrad_overlap(old_ov)
