"""Test-time augmentation inside the device inference loop on the real ACDC network (evaluate.predict_volume(tta=...), MI355X only):
the fused path (views in one launch, ONE forward over T * n slices, merge kernel) against the recipe of tests/test_tta.py applied
to logits from three separate forwards of torch.flip-ed inputs; the same bounds as there (conf within 1e-6, predictions equal
except where the reference's own top-2 gap is below 1e-5, at most 0.1 % of the voxels)."""
import numpy as np
import pytest
import torch

from backend import use_hip
from cenet_amd import evaluate, kern, ops
from tta_ref import hold_to_reference, reference, smooth_volume

pytestmark = pytest.mark.gpu


def _acdc_net(d):
    from cenet_amd.networks import CENet
    from oracle import cenet_oracle as O
    from oracle.golden_cases import MODEL_CONFIGS, config_from_kwargs
    kw = MODEL_CONFIGS["acdc"]["kw"]
    net = CENet(**kw)
    net.load_state_dict(O.make_state_dict(config_from_kwargs(kw), seed=42), strict=True)
    return net.to(d).eval()


def test_real_cenet_volume_with_flips():
    """Observed on the MI355X: conf within 1.67e-7 of the recipe, no voxel under the gap bound, none differing (the forward over
    the six views in one batch gives each slice the logits its own forward gives, to well below the bounds)."""
    d = use_hip()
    net = _acdc_net(d)
    D, H, W, P = 2, 40, 36, 224
    vol = torch.from_numpy(smooth_volume((D, H, W), 31)).to(d)
    inp = torch.empty(D, 1, P, P, device=d)
    kern.vol_resize_cubic(vol, torch.empty(D * H * W, dtype=torch.float64, device=d), inp, D, H, W, P, P)
    stacks = []
    with torch.no_grad(), ops.batch1_semantics():
        for dims in ((), (-1,), (-2,)):  # views 0, 1, 2: identity, flip along W, flip along H
            stacks.append(net(torch.flip(inp, dims).contiguous() if dims else inp).float().cpu().numpy())
    want_pred, want_conf, gap = reference(np.stack(stacks), 0x07, (H, W))
    assert len(np.unique(want_pred)) > 1
    out = []
    for _ in range(2):
        conf = torch.full((D, H, W), -1.0, device=d)
        pred, counts = evaluate.predict_volume(net, vol, (P, P), tta="flips", conf_out=conf)
        assert counts is None and pred.is_cuda
        out.append((pred.cpu(), conf.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])  # a second call: bit-identical
    hold_to_reference(f"CENet acdc {(D, H, W)} flips", out[0][0].numpy(), out[0][1].numpy(), want_pred, want_conf, gap)


def test_predict_volume_with_tta_makes_no_host_round_trip(monkeypatch):
    """as test_predict_volume_makes_no_host_round_trip (tests/test_volume_inference.py): sync-debug mode raises on every
    synchronising call, and Tensor.cpu / .numpy / .tolist / .item are patched to raise as well"""
    d = use_hip()
    K = 4
    vol = torch.from_numpy(smooth_volume((10, 64, 56), 11)).to(d)
    lab = torch.clamp((vol * K).floor(), 0, K - 2)

    class Proj(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.linspace(-3, 3, K).view(1, K, 1, 1))

        def forward(self, x):
            return x * self.w + self.w * self.w

    net = Proj().to(d)
    conf = torch.empty(10, 64, 56, device=d)
    evaluate.predict_volume(net, vol[:2], (48, 48), labels=lab[:2], tta="d4", conf_out=conf[:2])  # (loads the library, warms up)
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("host round trip inside predict_volume")

    for name in ("cpu", "numpy", "tolist", "item"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pred, counts = evaluate.predict_volume(net, vol, (48, 48), batch_slices=32, normalize=(0.5, 0.5), labels=lab, tta="d4",
                                               conf_out=conf)
    finally:
        torch.cuda.set_sync_debug_mode(old)
        monkeypatch.undo()
    torch.cuda.synchronize()
    assert pred.is_cuda and counts.is_cuda and tuple(pred.shape) == (10, 64, 56)
    assert int(counts[:K, 1].sum()) == pred.numel() and float(conf.min()) >= 1.0 / K - 1e-6 and float(conf.max()) <= 1.0 + 1e-6


def test_train_acdc_hands_test_tta_to_inference(monkeypatch):
    from cenet_amd import train
    from cenet_amd.networks import CENet
    from oracle import cenet_oracle as O
    d = use_hip()
    torch.manual_seed(77)
    net = CENet(input_channels=1, num_classes=4, scale_factors=[1.0, 0.5], diffatt_num_heads=[4, 4, 4], out_up_block="upcn")
    net.backbone.reset_drop_path(0.0)
    x, lab = O.synthetic_batch(2, 1, 4, seed=21)
    seen = []
    monkeypatch.setattr(evaluate, "validate", lambda net, batches: 0.5)
    monkeypatch.setattr(evaluate, "inference", lambda net, volumes, classes, **kw: (seen.append(kw), (0.4, 9.0))[1])
    for tta in ("flips", None):
        train.train_acdc(net, [{"image": x, "label": lab.long()}], max_epochs=1, base_lr=0.01, device=d, graph=False,
                         val_batches=lambda: [], log=lambda s: None, test_volumes=lambda: ["vol"], test_tta=tta)
    assert seen[0]["tta"] == "flips" and seen[0]["resize"] == "device" and "tta" not in seen[1]
