"""Sliding-window inference inside the device inference loop on the real ACDC network (evaluate.predict_volume(window_overlap=...),
MI355X only): the fused path (windows in one launch, forwards of the window batch, merge kernel) against the float64 restatement of
tests/sw_ref.py fed by separate forwards of torch-cropped and padded inputs; the same bounds as tests/test_sliding_window.py (conf
within 2e-6, predictions equal except where the reference's own top-2 gap is below 2e-5, at most 0.5 % of the voxels)."""
import numpy as np
import pytest
import torch

import sw_ref
from backend import use_hip
from cenet_amd import evaluate, kern, ops
from tta_ref import smooth_volume

pytestmark = pytest.mark.gpu


def _acdc_net(d):
    from cenet_amd.networks import CENet
    from oracle import cenet_oracle as O
    from oracle.golden_cases import MODEL_CONFIGS, config_from_kwargs
    kw = MODEL_CONFIGS["acdc"]["kw"]
    net = CENet(**kw)
    net.load_state_dict(O.make_state_dict(config_from_kwargs(kw), seed=42), strict=True)
    return net.to(d).eval()


@pytest.fixture(scope="module")
def acdc():
    """the network, a (2, 200, 240) volume and, computed once, the logits of every window from its own forward of a torch-made crop:
    the volume pads along y (one window, origin -12) and takes two windows along x (origins 0 and 16)"""
    d = use_hip()
    net = _acdc_net(d)
    D, H, W, P = 2, 200, 240, 224
    vol = torch.from_numpy(smooth_volume((D, H, W), 31)).to(d)
    oy, ox = kern.sw_origins(H, P, 0.5), kern.sw_origins(W, P, 0.5)
    assert (oy, ox) == ([-12], [0, 16])
    padded = torch.nn.functional.pad(vol[:, None], (0, 0, 12, 12))  # [D, 1, 224, 240], zeros above and below
    logits = {}
    with torch.no_grad(), ops.batch1_semantics():
        for dims in ((), (-1,), (-2,)):  # views 0, 1, 2: identity, flip along W, flip along H
            rows = []
            for b in range(D):
                for x0 in ox:
                    crop = padded[b:b + 1, :, :, x0:x0 + P].contiguous()
                    rows.append(net(torch.flip(crop, dims).contiguous() if dims else crop).float().cpu().numpy())
            logits[dims] = np.concatenate(rows)
    return d, net, vol, (D, H, W, P), oy, ox, logits


@pytest.mark.parametrize("tta", [None, "flips"])
def test_real_cenet_volume_with_windows(acdc, tta):
    """Observed on the MI355X: conf within 2.69e-7 (no augmentation) and 2.75e-7 (flips) of the recipe, 2 and 0 of 96 000 voxels
    under the gap bound, none differing."""
    d, net, vol, (D, H, W, P), oy, ox, logits = acdc
    mask = 0x01 if tta is None else 0x07
    stacks = np.stack([logits[dims] for dims in ((), (-1,), (-2,))[:1 if tta is None else 3]])
    wy = wx = kern.sw_weights(P)
    want_pred, want_conf, gap = sw_ref.reference(stacks, mask, D, oy, ox, wy, wx, (H, W))
    assert len(np.unique(want_pred)) > 1
    out = []
    for _ in range(2):
        conf = torch.full((D, H, W), -1.0, device=d)
        pred, counts = evaluate.predict_volume(net, vol, (P, P), tta=tta, conf_out=conf, window_overlap=0.5)
        assert counts is None and pred.is_cuda
        out.append((pred.cpu(), conf.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])  # a second call: bit-identical
    sw_ref.hold_to_reference(f"CENet acdc {(D, H, W)} windows {P} tta {tta}", out[0][0].numpy(), out[0][1].numpy(), want_pred,
                             want_conf, gap)


def test_predict_volume_with_windows_makes_no_host_round_trip(monkeypatch):
    """as test_predict_volume_with_tta_makes_no_host_round_trip (tests/test_tta_gpu.py): sync-debug mode raises on every
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
    kw = dict(tta="d4", window_overlap=0.5)
    evaluate.predict_volume(net, vol[:2], (48, 48), labels=lab[:2], conf_out=conf[:2], **kw)  # (loads the library, warms up)
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("host round trip inside predict_volume")

    for name in ("cpu", "numpy", "tolist", "item"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pred, counts = evaluate.predict_volume(net, vol, (48, 48), batch_slices=32, normalize=(0.5, 0.5), labels=lab, conf_out=conf,
                                               **kw)
    finally:
        torch.cuda.set_sync_debug_mode(old)
        monkeypatch.undo()
    torch.cuda.synchronize()
    assert pred.is_cuda and counts.is_cuda and tuple(pred.shape) == (10, 64, 56)
    assert int(counts[:K, 1].sum()) == pred.numel() and float(conf.min()) >= 1.0 / K - 1e-6 and float(conf.max()) <= 1.0 + 1e-6


def test_train_acdc_hands_test_window_overlap_to_inference(monkeypatch):
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
    for ov in (0.5, None):
        train.train_acdc(net, [{"image": x, "label": lab.long()}], max_epochs=1, base_lr=0.01, device=d, graph=False,
                         val_batches=lambda: [], log=lambda s: None, test_volumes=lambda: ["vol"], test_window_overlap=ov)
    assert seen[0]["window_overlap"] == 0.5 and seen[0]["resize"] == "device" and "window_overlap" not in seen[1]
