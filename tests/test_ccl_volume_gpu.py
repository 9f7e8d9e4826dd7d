"""postprocess="lcc" through the volume entry points on the MI355X: test_single_volume / synapse_test_single_volume with both
resizes, the saved prediction, inference, and the epoch tail of train.train_acdc — each against keep_largest_component applied by
hand to the unfiltered prediction of the same network.  The network is a small randomly initialised CENet, whose predictions are
full of islands, on a few slices whose sides differ from the patch side."""
import copy
import os

import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

from backend import use_hip
from cenet_amd import _lib, evaluate
from oracle import cenet_oracle as O

K = 4
PATCH = (224, 224)


@pytest.fixture
def hip():
    d = use_hip()
    yield d
    _lib._LIB = None
    _lib._HOSTSIM = False


def _net(d):
    from cenet_amd.networks import CENet
    torch.manual_seed(77)
    net = CENet(input_channels=1, num_classes=K, scale_factors=[1.0, 0.5], diffatt_num_heads=[4, 4, 4], out_up_block="upcn")
    net.backbone.reset_drop_path(0.0)
    return net.to(d).eval()


def _volume(shape, seed):
    """smooth random intensities and a label volume cut from them, [1, D, H, W] each"""
    rng = np.random.default_rng(seed)
    low = rng.standard_normal((shape[0], 7, 7))
    image = np.stack([zoom(s, (shape[1] / 7, shape[2] / 7), order=1) for s in low]).astype(np.float32)
    label = np.clip(((image - image.min()) / (image.max() - image.min()) * K).astype(np.int64), 0, K - 1).astype(np.float32)
    return torch.from_numpy(image)[None], torch.from_numpy(label)[None]


def _pred(path, case):
    return np.load(os.path.join(path, f"{case}_pred.npy"))


@pytest.mark.gpu
@pytest.mark.parametrize("resize", ["device", "host"])
def test_single_volume_scores_and_saves_the_filtered_prediction(hip, tmp_path, resize):
    net = _net(hip)
    image, label = _volume((3, 200, 180), 1)
    lab_d = label[0].to(hip)
    for fn, kind, kw in ((evaluate.test_single_volume, "acdc", {}),
                         (evaluate.synapse_test_single_volume, "synapse", {"normalize": (0.5, 0.5)})):
        args = dict(patch_size=PATCH, device=hip, resize=resize, batch_slices=2)
        plain = fn(image, label, net, K, test_save_path=str(tmp_path / kind / "plain"), case="c", **args)
        assert plain == fn(image, label, net, K, postprocess=None, **args)  # the keyword's default is the call without it
        got = fn(image, label, net, K, postprocess="lcc", test_save_path=str(tmp_path / kind / "lcc"), case="c", **args)
        own = torch.from_numpy(_pred(tmp_path / kind / "plain", "c")).to(hip)  # this path's own unfiltered prediction
        filt, table = evaluate.keep_largest_component(own, K)
        assert table[1:, 0].max() > 1 and table[:, 2].sum() > 0  # islands: there was something to remove
        assert got == evaluate.label_metrics(filt, lab_d, K, kind) and got != plain
        assert np.array_equal(_pred(tmp_path / kind / "lcc", "c"), filt.cpu().numpy())
        # ... which is predict_volume's (the host resize may differ from it in a few voxels, tests/test_volume_inference.py)
        pred, _ = evaluate.predict_volume(net, image[0].to(hip), PATCH, batch_slices=2, **kw)
        if resize == "device" or torch.equal(pred, own):
            assert got == evaluate.label_metrics(evaluate.keep_largest_component(pred, K)[0], lab_d, K, kind)
        assert resize == "host" or torch.equal(pred, own)
        # the other options reach the filter
        got2 = fn(image, label, net, K, postprocess="lcc", lcc_connectivity=2, lcc_per_slice=True, **args)
        assert got2 == evaluate.label_metrics(evaluate.keep_largest_component(own, K, 2, True)[0], lab_d, K, kind)


@pytest.mark.gpu
def test_inference_averages_the_filtered_cases(hip, tmp_path):
    net = _net(hip)
    cases = []
    for i, shape in enumerate([(3, 200, 180), (2, 190, 210)]):
        image, label = _volume(shape, 10 + i)
        cases.append({"image": image, "label": label, "case_name": f"case{i}"})
    dice, hd = evaluate.inference(net, cases, K, patch_size=PATCH, log=lambda s: None, postprocess="lcc", batch_slices=2)
    per_case = []
    for c in cases:
        pred, _ = evaluate.predict_volume(net, c["image"][0].to(hip), PATCH, batch_slices=2)
        per_case.append(np.array(evaluate.label_metrics(evaluate.keep_largest_component(pred, K)[0], c["label"][0].to(hip), K)))
    table = sum(per_case) / len(per_case)
    assert dice == float(np.mean(table, axis=0)[0]) and hd == float(np.mean(table, axis=0)[1])
    assert (dice, hd) != evaluate.inference(net, cases, K, patch_size=PATCH, log=lambda s: None, batch_slices=2)


@pytest.mark.gpu
def test_train_loop_forwards_test_postprocess(hip):
    from cenet_amd import train
    net = _net(hip)
    x, lab = O.synthetic_batch(4, 1, K, seed=21)
    loader = [{"image": x[:2], "label": lab[:2].long()}, {"image": x[2:], "label": lab[2:].long()}]
    xv, lv = O.synthetic_batch(1, 1, K, seed=5)
    image, label = _volume((3, 200, 180), 3)
    vols = lambda: [{"image": image, "label": label, "case_name": "case0"}]  # noqa: E731
    val = lambda: [(xv.to(hip), lv.to(hip))]  # noqa: E731
    runs = {}
    for post in (None, "lcc"):
        n = copy.deepcopy(net)
        h = train.train_acdc(n, loader, max_epochs=1, base_lr=0.01, device=hip, graph=False, val_batches=val, log_every=1,
                             log=lambda s: None, test_volumes=vols, test_postprocess=post)
        assert len(h["test_hd95"]) == 1
        direct = evaluate.inference(n, vols(), K, patch_size=PATCH, log=lambda s: None, postprocess=post)
        assert (h["test_dice"][0], h["test_hd95"][0]) == direct
        runs[post] = h["test_hd95"][0]
    assert runs[None] != runs["lcc"]  # (fixed seeds: the islands of a barely trained network move the 95th percentile)
    with pytest.raises(ValueError, match="postprocess"):
        train.train_acdc(copy.deepcopy(net), loader, max_epochs=1, device=hip, graph=False, val_batches=val, test_volumes=vols,
                         test_postprocess="largest")
