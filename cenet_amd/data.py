"""Input pipeline of the ACDC preset: the reference's dataset classes and training-time augmentation
with the same names, arguments and random-number consumption, plus what the reference lacks to keep an MI355X fed — worker
processes with per-worker seeds, pinned staging buffers and a copy stream that uploads batch i+1 while batch i trains.

Mirrors src/datasets/dataset_acdc.py:
  * `random_rot_flip` (:15-22), `random_rotate` (:25-29), `RandomGenerator` (:32-48) — numpy / scipy on the host exactly
    as the reference does (`np.rot90`, `np.flip`, `ndimage.rotate(order=0, reshape=False)`, `zoom(order=3)` for the image and
    `zoom(order=0)` for the label); with the same seeds of `random` and `np.random` the samples are bit-identical
    (tests/test_data.py against vectors produced by the reference's own classes, oracle/gen_golden_data.py);
  * `ACDCdataset` (:51-78) and `ACDCdatasetFast` (:81-114) — same constructor and `__getitem__` contract
    (`{'image', 'label', 'case_name'}`; the transform only on split 'train').
The reference builds `DataLoader(db_train, batch_size, shuffle=True)` with `num_workers=0` (src/main_acdc.py:140): one host
process does all the resampling, 30 samples/s measured (tools/data_bench.py), against ~750 images/s per GPU for the step.
`make_train_loader` + `DevicePrefetcher` are the replacement; with `num_workers=0` the loader is the reference's.

Round 5, the MI355X-native form of the same pipeline: `DeviceSlices` keeps the whole training set in HBM (ACDC: 1 312 slices,
0.35 GB of 288), `DeviceAugmenter` draws the reference's random numbers on the host IN THE REFERENCE'S ORDER and runs the
resampling of a whole batch as three kernel launches (csrc/augment.hip, cenet_augment_acdc), `DeviceTrainLoader` is the
`DataLoader(db_train, batch_size, shuffle=True)` of main_acdc.py:140 over them — same permutation from the same torch seed, same
augmentation decisions from the same `random` / `np.random` seeds, no worker processes, no host copies of pixels.

The Synapse training pipeline (src/datasets/dataset_synapse.py:86-112: imgaug SomeOf over ten augmenters, zoom, Normalize) on the
same device-resident slices: `SegAugmenter` + `SYNAPSE_OPS` (csrc/augment_ops.hip, cenet_augment_ops), handed to
`DeviceTrainLoader(augmenter=...)`.  The operator family and its distribution, each operator specified by scipy — not imgaug's numbers.
"""
from __future__ import annotations

import os
import random
from typing import Iterable, Iterator, Optional, Sequence

import numpy as np
import torch
from scipy import ndimage
from scipy.ndimage import zoom
from torch.utils.data import DataLoader, Dataset


def _apply_pair(fn, image, label):
    return fn(image), fn(label)


def random_rot_flip(image, label):
    """dataset_acdc.py:15-22 — k quarter turns, then a flip along a random axis.  Draw order (np.random): k, then axis."""
    k = np.random.randint(0, 4)
    image, label = _apply_pair(lambda a: np.rot90(a, k), image, label)
    axis = np.random.randint(0, 2)
    return _apply_pair(lambda a: np.flip(a, axis=axis).copy(), image, label)


def random_rotate(image, label):
    """dataset_acdc.py:25-29 — whole-degree rotation in [-20, 20) (one np.random draw), nearest sampling for image and
    label alike, output shape kept."""
    angle = np.random.randint(-20, 20)
    return _apply_pair(lambda a: ndimage.rotate(a, angle, order=0, reshape=False), image, label)


def _resize_pair(image, label, size):
    """Cubic spline for the image, nearest for the label, scipy's default (non-grid) coordinate mapping (dataset_acdc.py:43-44)."""
    h, w = image.shape
    if h == size[0] and w == size[1]:
        return image, label
    factors = (size[0] / h, size[1] / w)
    return zoom(image, factors, order=3), zoom(label, factors, order=0)


class RandomGenerator(object):
    """dataset_acdc.py:32-48.  sample {'image' [H,W], 'label' [H,W]} -> {'image' float32 [1,h,w], 'label' int64 [h,w]}.
    `random` draws: one to choose the quarter-turn branch; only if that fails a second one to choose the rotation branch."""

    def __init__(self, output_size: Sequence[int]):
        self.output_size = output_size

    def __call__(self, sample):
        image, label = sample['image'], sample['label']
        if random.random() > 0.5:
            image, label = random_rot_flip(image, label)
        elif random.random() > 0.5:
            image, label = random_rotate(image, label)
        image, label = _resize_pair(image, label, self.output_size)
        image_t = torch.from_numpy(image.astype(np.float32)).unsqueeze(0)
        label_t = torch.from_numpy(label.astype(np.float32)).long()
        return {'image': image_t, 'label': label_t}


class ACDCdataset(Dataset):
    """dataset_acdc.py:51-78: `<list_dir>/<split>.txt` names .npz files holding 'img' and 'label'; train / valid entries
    are slices under `<base_dir>/<split>/`, test entries whole volumes under `<base_dir>/`."""

    def __init__(self, base_dir, list_dir, split, transform=None):
        self.transform = transform
        self.split = split
        with open(os.path.join(list_dir, self.split + '.txt')) as f:
            self.sample_list = f.readlines()
        self.data_dir = base_dir

    def __len__(self):
        return len(self.sample_list)

    def _path(self, idx):
        name = self.sample_list[idx].strip('\n')
        if self.split == "train" or self.split == "valid":
            return os.path.join(self.data_dir, self.split, name)
        return self.data_dir + "/{}".format(name)

    def _load(self, idx):
        with np.load(self._path(idx)) as data:
            return data['img'], data['label']

    def __getitem__(self, idx):
        image, label = self._load(idx)
        sample = {'image': image, 'label': label}
        if self.transform and self.split == "train":
            sample = self.transform(sample)
        sample['case_name'] = self.sample_list[idx].strip('\n')
        return sample


class ACDCdatasetFast(ACDCdataset):
    """dataset_acdc.py:81-114: everything decoded into memory once."""

    def __init__(self, base_dir, list_dir, split, transform=None):
        super().__init__(base_dir, list_dir, split, transform)
        self.all_data = [super(ACDCdatasetFast, self)._load(i) for i in range(len(self.sample_list))]

    def _load(self, idx):
        return self.all_data[idx]


def _seed_worker(worker_id: int):
    """Each worker process draws its augmentations from its own stream: torch hands every worker base_seed + id, which is
    folded into `random` and `np.random` (a forked worker would otherwise repeat the parent's numpy stream)."""
    s = torch.initial_seed() % (2 ** 32)
    random.seed(s)
    np.random.seed(s)


def make_train_loader(dataset: Dataset, batch_size: int, num_workers: int = 0, seed: Optional[int] = None,
                      drop_last: bool = False, sampler=None) -> DataLoader:
    """`DataLoader(db_train, batch_size=..., shuffle=True)` of src/main_acdc.py:140 when num_workers == 0; otherwise the same
    batches produced by worker processes into pinned memory (persistent workers, two batches ahead each).  Pass a
    `DistributedSampler` for one process per GPU."""
    g = None
    if seed is not None:
        g = torch.Generator()
        g.manual_seed(seed)
    kw = {}
    if num_workers > 0:
        kw = dict(worker_init_fn=_seed_worker, persistent_workers=True, prefetch_factor=2)
    return DataLoader(dataset, batch_size=batch_size, shuffle=sampler is None, sampler=sampler, num_workers=num_workers,
                      pin_memory=torch.cuda.is_available(), drop_last=drop_last, generator=g, **kw)


class DevicePrefetcher:
    """Iterates a loader of dict batches and returns them with their tensors already on `device`: batch i+1 is copied on a
    separate stream (from the loader's pinned buffers, non-blocking) while the caller trains on batch i; the consumer's
    stream waits on the copy's event only when it takes the batch.  Non-tensor fields (case names) pass through."""

    def __init__(self, loader: Iterable, device, float_labels: bool = True):
        self.loader, self.device = loader, torch.device(device)
        self.float_labels = float_labels  # the loss kernels take class ids as float (core.py:179-188 casts per call)
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None

    def __len__(self):
        return len(self.loader)

    def _upload(self, batch):
        out = {}
        for k, v in batch.items():
            if torch.is_tensor(v):
                v = v.to(self.device, non_blocking=True)
                if k == "label" and self.float_labels:
                    v = v.float()
            out[k] = v
        return out

    def __iter__(self) -> Iterator[dict]:
        it = iter(self.loader)
        if self.stream is None:
            for batch in it:
                yield self._upload(batch)
            return
        nxt, ev = None, None

        def fetch():
            nonlocal nxt, ev
            try:
                b = next(it)
            except StopIteration:
                nxt, ev = None, None
                return
            with torch.cuda.stream(self.stream):
                nxt = self._upload(b)
                ev = torch.cuda.Event()
                ev.record(self.stream)

        fetch()
        while nxt is not None:
            cur, cur_ev = nxt, ev
            torch.cuda.current_stream(self.device).wait_event(cur_ev)
            for v in cur.values():
                if torch.is_tensor(v):
                    v.record_stream(torch.cuda.current_stream(self.device))
            fetch()  # the next upload overlaps the caller's work on `cur`
            yield cur


# ---------------------------------------------------------------------------------------------------------------------------
# Device-resident training set + device-side augmentation (csrc/augment.hip)
# ---------------------------------------------------------------------------------------------------------------------------
_SPLINE_POLE = np.sqrt(3.0) - 2.0  # the cubic B-spline prefilter's pole (scipy ni_splines)


class DeviceSlices:
    """All (image [H, W] float32, label [H, W] uint8 class ids) training slices, sizes may differ, packed into two device pools."""

    def __init__(self, samples: Sequence, device, names: Optional[Sequence[str]] = None):
        imgs, labs, shapes = [], [], []
        for img, lab in samples:
            img, lab = np.asarray(img), np.asarray(lab)
            assert img.ndim == 2 and img.shape == lab.shape, (img.shape, lab.shape)
            assert lab.min() >= 0 and lab.max() < 256, "labels are class ids"
            imgs.append(np.ascontiguousarray(img, dtype=np.float32).reshape(-1))
            labs.append(np.ascontiguousarray(lab).astype(np.uint8).reshape(-1))
            shapes.append(img.shape)
        self.shapes = np.asarray(shapes, dtype=np.int64).reshape(-1, 2)
        self.offsets = np.concatenate([[0], np.cumsum(self.shapes[:, 0] * self.shapes[:, 1])]).astype(np.int64)
        self.device = torch.device(device)
        self.pool_img = torch.from_numpy(np.concatenate(imgs)).to(self.device)
        self.pool_lab = torch.from_numpy(np.concatenate(labs)).to(self.device)
        self.max_h, self.max_w = int(self.shapes[:, 0].max()), int(self.shapes[:, 1].max())
        self.max_side = max(self.max_h, self.max_w)  # (a quarter turn swaps the sides)
        self.names = list(names) if names is not None else None

    @classmethod
    def from_dataset(cls, ds: "ACDCdataset", device):
        """every slice of an ACDCdataset / ACDCdatasetFast (train split; its host transform, if any, is not used)"""
        return cls([ds._load(i) for i in range(len(ds))], device, names=[n.strip('\n') for n in ds.sample_list])

    def __len__(self):
        return len(self.shapes)


class DeviceAugmenter:
    """RandomGenerator (dataset_acdc.py:32-48) for a batch of DeviceSlices indices -> {'image' [B, 1, h, w] float32, 'label'
    [B, h, w] float32 class ids} on the device.  `draw` consumes `random` and `np.random` exactly as the reference's
    __getitem__ calls would for the same samples in the same order (one `random.random()`; then k and axis from np.random, or a
    second `random.random()` and the angle), so a seeded run makes the reference's augmentation decisions."""

    def __init__(self, slices: DeviceSlices, output_size: Sequence[int]):
        self.slices, self.output_size = slices, (int(output_size[0]), int(output_size[1]))
        self.stride = slices.max_side * slices.max_side
        self._stage = {}

    def draw(self, indices: Sequence[int]):
        OH, OW = self.output_size
        tab = np.zeros((len(indices), 8), dtype=np.int64)
        dp = np.zeros((len(indices), 10), dtype=np.float64)
        for n, idx in enumerate(indices):
            H, W = (int(v) for v in self.slices.shapes[idx])
            mode = k = axis = 0
            if random.random() > 0.5:  # dataset_acdc.py:38-39 -> :15-22
                mode, k, axis = 1, int(np.random.randint(0, 4)), int(np.random.randint(0, 2))
            elif random.random() > 0.5:  # :40-41 -> :25-29; the matrix and offset scipy.ndimage.rotate(reshape=False) builds
                mode = 2
                ang = np.deg2rad(np.random.randint(-20, 20))
                c, s_ = np.cos(ang), np.sin(ang)
                m = np.array([[c, s_], [-s_, c]], dtype=np.float64)
                ctr = (np.array([H, W], dtype=np.float64) - 1) / 2
                off = ctr - m @ ctr
                dp[n, 0:4] = m.reshape(-1)
                dp[n, 4:6] = off
            Ha, Wa = (W, H) if (mode == 1 and k & 1) else (H, W)
            resize = int(Ha != OH or Wa != OW)  # :42-45
            tab[n] = (self.slices.offsets[idx], H, W, mode, k, axis, resize, 0)
            dp[n, 6], dp[n, 7] = _SPLINE_POLE ** (Ha - 1), _SPLINE_POLE ** (Wa - 1)
            dp[n, 8] = (Ha - 1) / (OH - 1)  # scipy zoom, grid_mode=False: input coordinate = output index * (in - 1) / (out - 1)
            dp[n, 9] = (Wa - 1) / (OW - 1)
        return tab, dp

    def apply(self, tab: np.ndarray, dp: np.ndarray) -> dict:
        from . import kern
        sl, dev = self.slices, self.slices.device
        B = tab.shape[0]
        OH, OW = self.output_size
        if self._stage.get("B", 0) < B:
            self._stage = {"B": B, "img": torch.empty(B * self.stride, dtype=torch.float64, device=dev),
                           "lab": torch.empty(B * self.stride, dtype=torch.uint8, device=dev)}
        pin = dev.type == "cuda"
        tab_t, dp_t = torch.from_numpy(tab), torch.from_numpy(dp)
        if pin:
            tab_t, dp_t = tab_t.pin_memory(), dp_t.pin_memory()
        tab_d, dp_d = tab_t.to(dev, non_blocking=True), dp_t.to(dev, non_blocking=True)
        image = torch.empty(B, 1, OH, OW, dtype=torch.float32, device=dev)
        label = torch.empty(B, OH, OW, dtype=torch.float32, device=dev)
        kern.augment_acdc(sl.pool_img, sl.pool_lab, tab_d, dp_d, self._stage["img"], self._stage["lab"], self.stride,
                          sl.max_side, sl.max_side, image, label, B, OH, OW)
        return {"image": image, "label": label}

    def __call__(self, indices: Sequence[int]) -> dict:
        return self.apply(*self.draw(indices))


# The Synapse training pipeline's operators (dataset_synapse.py:86-97), in the reference's order, with its ranges.  (name, params):
#   flips: `p`, the probability that a picked flip flips; noise: `scale` as the reference writes it (0.005 * 255); blur: `sigma`;
#   contrast: alpha range and centre; scale: per-axis factor range; rotate / shear: degree ranges; grid_warp: control grid and the
#   range of s in displacements ~ N(0, s) * side; translate: range of the fraction of each side.
SYNAPSE_OPS = (
    ("flip_ud", {"p": 0.5}),
    ("flip_lr", {"p": 0.5}),
    ("noise", {"scale": 0.005 * 255}),
    ("blur", {"sigma": 1.0}),
    ("contrast", {"alpha": (0.5, 1.5), "center": 0.0}),
    ("scale", {"factor": (0.5, 2.0)}),
    ("rotate", {"degrees": (-40.0, 40.0)}),
    ("shear", {"degrees": (-16.0, 16.0)}),
    ("grid_warp", {"grid": (4, 4), "scale": (0.008, 0.03)}),
    ("translate", {"fraction": (-0.2, 0.2)}),
)
AUG_MAX_STAGES, AUG_MAX_RADIUS, AUG_MAX_GRID = 8, 16, 16  # cenet_augment_ops' limits (csrc/augment_ops.hip)


def gaussian_weights(sigma: float, truncate: float = 4.0):
    """(radius, the normalised weights at distance 0 .. radius) of scipy.ndimage.gaussian_filter1d's kernel, computed as scipy does"""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    phi = phi / phi.sum()
    return radius, phi[radius:]


def centred_affine(m, shape, shift=(0.0, 0.0)):
    """(matrix, offset) of scipy.ndimage.affine_transform for the output -> input map o -> m (o - ctr) + ctr - shift about
    ctr = ((H - 1) / 2, (W - 1) / 2), as ndimage.rotate(reshape=False) builds its own"""
    m = np.asarray(m, dtype=np.float64).reshape(2, 2)
    ctr = (np.asarray(shape, dtype=np.float64) - 1) / 2
    return m, ctr - m @ ctr - np.asarray(shift, dtype=np.float64)


class SegAugmenter:
    """The Synapse training augmentation (dataset_synapse.py:86-112: imgaug `SomeOf((0, 4), [...ten augmenters...],
    random_order=True)`, then zoom(order=3) / zoom(order=0) to the patch size, then Normalize) for a batch of DeviceSlices indices
    -> {'image' [B, 1, h, w] float32, 'label' [B, h, w] float32 class ids} on the device (csrc/augment_ops.hip, then the resize of
    csrc/augment.hip).

    What this reproduces is the pipeline's operator family and its distribution — which operators, in what ranges, how many per
    sample and in what order — with every operator specified by scipy (include/cenet_hip.h, cenet_augment_ops).  It does not
    reproduce imgaug's numbers: imgaug's random stream and its cv2 interpolation are not pinned here.  The contrast centre 0.0 for
    float images is imgaug's behaviour as remembered from its source: unverified.

    The augmenter owns a numpy Generator (`seed`) and never touches the global `random` / `np.random` streams.  `draw` picks per
    sample n uniformly in `some_of`, n distinct entries of `ops`, their order (random_order) and each one's parameters; the names
    picked by the last draw are kept in `picked` (a picked flip that does not fire runs as a copy)."""

    def __init__(self, slices: DeviceSlices, output_size: Sequence[int], ops=SYNAPSE_OPS, some_of=(0, 4), random_order: bool = True,
                 normalize=None, seed=None):
        self.slices, self.output_size = slices, (int(output_size[0]), int(output_size[1]))
        self.ops, self.some_of, self.random_order = tuple(ops), (int(some_of[0]), int(some_of[1])), bool(random_order)
        if not 0 <= self.some_of[0] <= self.some_of[1] <= min(len(self.ops), AUG_MAX_STAGES):
            raise ValueError(f"some_of {some_of}: between 0 and min(len(ops), {AUG_MAX_STAGES}) ops per sample")
        self.normalize = None if normalize is None else (float(normalize[0]), float(normalize[1]))
        self.rng = np.random.default_rng(seed)
        self.stride = slices.max_h * slices.max_w
        self.picked = []
        self._buf = {}

    # ---- one drawn operator -> the kernel's ops: (kind, *parameters) ---------------------------------------------------------------
    def _draw_op(self, name, prm, H, W):
        rng = self.rng
        if name in ("flip_ud", "flip_lr"):
            return (name,) if rng.random() < prm["p"] else ("copy",)
        if name == "noise":
            k0, k1 = (int(v) for v in rng.integers(0, 2 ** 32, 2, dtype=np.uint64))
            return ("noise", float(prm["scale"]), k0, k1)
        if name == "blur":
            return ("blur", float(prm["sigma"]))
        if name == "contrast":
            return ("contrast", float(rng.uniform(*prm["alpha"])), float(prm["center"]))
        if name == "scale":  # the output is the input magnified by (sy, sx) about the centre
            sy, sx = rng.uniform(*prm["factor"], 2)
            return ("affine", *centred_affine([[1 / sy, 0], [0, 1 / sx]], (H, W)))
        if name == "rotate":
            a = np.deg2rad(rng.uniform(*prm["degrees"]))
            return ("affine", *centred_affine([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], (H, W)))
        if name == "shear":  # along x: the input column moves with the row
            return ("affine", *centred_affine([[1, 0], [np.tan(np.deg2rad(rng.uniform(*prm["degrees"]))), 1]], (H, W)))
        if name == "translate":
            ty, tx = rng.uniform(*prm["fraction"], 2)
            return ("affine", *centred_affine(np.eye(2), (H, W), shift=(ty * H, tx * W)))
        if name == "grid_warp":
            R, C = prm["grid"]
            s = rng.uniform(*prm["scale"])
            return ("grid_warp", rng.normal(0.0, s, (R, C)) * H, rng.normal(0.0, s, (R, C)) * W)
        raise ValueError(f"SegAugmenter: unknown op {name!r}")

    def plan(self, indices: Sequence[int], chains: Sequence[Sequence[tuple]]):
        """the (tab, dp) tables of cenet_augment_ops for explicit per-sample chains of kernel ops: ('copy',), ('flip_ud',),
        ('flip_lr',), ('affine', M [2, 2], offset [2]), ('grid_warp', dY [R, C], dX [R, C]), ('blur', sigma),
        ('noise', scale, key0, key1), ('contrast', alpha, centre); shorter chains end in copies"""
        from .kern import AUG_OPS, AUG_OPS_DP
        S = max(1, max((len(c) for c in chains), default=0))
        tab = np.zeros((len(indices), 3 + S), dtype=np.int64)
        dp = np.zeros((len(indices), S, AUG_OPS_DP), dtype=np.float64)
        for n, (idx, chain) in enumerate(zip(indices, chains)):
            tab[n, :3] = (self.slices.offsets[idx], *self.slices.shapes[idx])
            for s, (kind, *a) in enumerate(chain):
                word, row = AUG_OPS[kind], dp[n, s]
                if kind == "affine":
                    row[0:4], row[4:6] = np.asarray(a[0], dtype=np.float64).reshape(-1), a[1]
                elif kind == "grid_warp":
                    dy, dx = (np.asarray(v, dtype=np.float64) for v in a)
                    R, C = dy.shape
                    assert dx.shape == (R, C) and R < 256 and C < 256
                    word += 256 * R + 65536 * C
                    if R * C <= AUG_MAX_GRID:  # (a larger grid is left for the library to refuse)
                        row[:R * C], row[AUG_MAX_GRID:AUG_MAX_GRID + R * C] = dy.reshape(-1), dx.reshape(-1)
                elif kind == "blur":
                    radius, w = gaussian_weights(a[0])
                    row[0] = radius
                    if radius <= AUG_MAX_RADIUS:
                        row[1:2 + radius] = w
                elif kind == "noise":
                    row[0:3] = a
                elif kind == "contrast":
                    row[0:2] = a
                tab[n, 3 + s] = word
        return tab, dp

    def draw(self, indices: Sequence[int]):
        chains, self.picked = [], []
        for idx in indices:
            H, W = (int(v) for v in self.slices.shapes[idx])
            n = int(self.rng.integers(self.some_of[0], self.some_of[1] + 1))
            pick = self.rng.choice(len(self.ops), size=n, replace=False)  # (a uniformly random n-subset in uniformly random order)
            if not self.random_order:
                pick = np.sort(pick)
            self.picked.append(tuple(self.ops[i][0] for i in pick))
            chains.append([self._draw_op(*self.ops[i], H, W) for i in pick])
        return self.plan(indices, chains)

    def apply(self, plan) -> dict:
        from . import kern
        tab, dp = plan
        sl, dev = self.slices, self.slices.device
        B, S = tab.shape[0], tab.shape[1] - 3
        OH, OW = self.output_size
        if self._buf.get("B", 0) < B:
            n = B * self.stride
            self._buf = {"B": B, "img": [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)],
                         "lab": [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2)],
                         "stage_img": torch.empty(n, dtype=torch.float64, device=dev),
                         "stage_lab": torch.empty(n, dtype=torch.uint8, device=dev)}
        # the resize of RandomGenerator (cenet_augment_acdc, mode 0: no quarter turn, no rotation) with the work buffer as its pool
        tab2 = np.zeros((B, 8), dtype=np.int64)
        dp2 = np.zeros((B, 10), dtype=np.float64)
        H, W = tab[:, 1], tab[:, 2]
        tab2[:, 0], tab2[:, 1], tab2[:, 2] = np.arange(B) * self.stride, H, W
        tab2[:, 6] = (H != OH) | (W != OW)
        dp2[:, 6], dp2[:, 7] = _SPLINE_POLE ** (H - 1), _SPLINE_POLE ** (W - 1)
        dp2[:, 8], dp2[:, 9] = (H - 1) / (OH - 1), (W - 1) / (OW - 1)
        pin = dev.type == "cuda"
        up = []
        for a in (tab, dp, tab2, dp2):
            t = torch.from_numpy(a)
            up.append((t.pin_memory() if pin else t).to(dev, non_blocking=True))
        buf = self._buf
        r = kern.augment_ops(sl.pool_img, sl.pool_lab, tab, dp, up[0], up[1], buf["img"], buf["lab"], self.stride, sl.max_h, sl.max_w,
                             B, S)
        image = torch.empty(B, 1, OH, OW, dtype=torch.float32, device=dev)
        label = torch.empty(B, OH, OW, dtype=torch.float32, device=dev)
        kern.augment_acdc(buf["img"][r], buf["lab"][r], up[2], up[3], buf["stage_img"], buf["stage_lab"], self.stride, sl.max_h,
                          sl.max_w, image, label, B, OH, OW)
        if self.normalize is not None:
            kern.augment_normalize(image, *self.normalize)
        return {"image": image, "label": label}

    def __call__(self, indices: Sequence[int]) -> dict:
        return self.apply(self.draw(indices))


class DeviceImages:
    """All (image [C, H, W] float32 — channels first, planar; 1 <= C <= 4 —, label [H, W] class ids) training samples of ONE
    shape, packed into two device pools: sample n's channels at pool_img[n * C * H * W], its label at pool_lab[n * H * W].
    (A channels-last [H, W, C] image is NOT accepted: with H or W <= 4 the two layouts cannot be told apart; `from_arrays` takes
    the reference's files.)"""

    def __init__(self, samples: Sequence, device, names: Optional[Sequence[str]] = None):
        imgs, labs = [], []
        for img, lab in samples:
            img, lab = np.asarray(img), np.asarray(lab)
            assert img.ndim == 3 and img.shape[1:] == lab.shape, (img.shape, lab.shape)
            assert lab.min() >= 0 and lab.max() < 256, "labels are class ids"
            imgs.append(np.ascontiguousarray(img, dtype=np.float32))
            labs.append(np.ascontiguousarray(lab).astype(np.uint8))
        assert imgs and all(a.shape == imgs[0].shape for a in imgs), "all samples share one shape"
        self.channels, self.height, self.width = (int(v) for v in imgs[0].shape)
        assert 1 <= self.channels <= 4, self.channels
        self.device = torch.device(device)
        self.pool_img = torch.from_numpy(np.stack(imgs).reshape(-1)).to(self.device)
        self.pool_lab = torch.from_numpy(np.stack(labs).reshape(-1)).to(self.device)
        self.count = len(imgs)
        self.names = list(names) if names is not None else None

    @classmethod
    def from_arrays(cls, X, Y, device, names: Optional[Sequence[str]] = None):
        """the reference's X_tr_*.npy [N, C, H, W] in [0, 1] and Y_tr_*.npy [N, 1, H, W] (or [N, H, W]) in [0, 1]
        (dataset_ham.py:78-79): images become uint8(x * 255) held as float32 in [0, 255], masks class id 1 where uint8(y * 255) >=
        128 and 0 elsewhere (what the reference's per-sample min-max makes of a 0 / 255 mask)"""
        X, Y = np.asarray(X), np.asarray(Y)
        Y = Y[:, 0] if Y.ndim == 4 else Y
        assert X.ndim == 4 and Y.shape == (X.shape[0], *X.shape[2:]), (X.shape, Y.shape)
        return cls([(np.uint8(x * 255).astype(np.float32), (np.uint8(y * 255) >= 128).astype(np.uint8)) for x, y in zip(X, Y)],
                   device, names=names)

    def __len__(self):
        return self.count


# The skin training pipeline's transforms (dataset_ham.py:273-281, dataset_ph2.py:250-257: albumentations Compose), in the
# reference's order, each with its own probability `p` and its ranges.  (name, params):
#   rotate: degree range, border 'mirror' (albumentations' default BORDER_REFLECT_101 is scipy's 'mirror'); flips: `p` only;
#   brightness_contrast: alpha = 1 + U(contrast), beta = max_value * U(brightness), clipped to [0, max_value] — contrast_limit =
#   brightness_limit = 0.2 and brightness_by_max on uint8 are albumentations' defaults as remembered from its source: unverified;
#   blur: odd kernel sizes k, sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8 (cv2.getGaussianKernel's rule for sigma = 0), radius
#   (k - 1) / 2, weights normalised; elastic: displacement = alpha * gaussian_filter(uniform(-1, 1), sigma, truncate), border 'mirror'.
SKIN_OPS = (
    ("rotate", {"p": 0.5, "degrees": (-30.0, 30.0), "mode": "mirror"}),
    ("flip_lr", {"p": 0.5}),
    ("flip_ud", {"p": 0.5}),
    ("brightness_contrast", {"p": 0.2, "contrast": (-0.2, 0.2), "brightness": (-0.2, 0.2), "max_value": 255.0}),
    ("blur", {"p": 0.3, "kernel": (3, 5, 7)}),
    ("elastic", {"p": 0.3, "alpha": 1.0, "sigma": 50.0, "truncate": 4.0, "mode": "mirror"}),
)
AUG_MAX_FIELD_RADIUS = 256  # cenet_augment_image_ops' limit (csrc/augment_image_ops.hip)


def blur_weights(k: int):
    """(radius, the normalised weights at distance 0 .. radius) of a k-tap Gaussian with cv2's sigma for a kernel size"""
    radius = (int(k) - 1) // 2
    sigma = 0.3 * ((int(k) - 1) * 0.5 - 1) + 0.8
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return radius, phi[radius:]


class ComposeAugmenter:
    """The skin training augmentation (dataset_ham.py:273-281 / dataset_ph2.py:250-257: albumentations `Compose([Rotate(limit=30,
    p=0.5), HorizontalFlip(p=0.5), VerticalFlip(p=0.5), RandomBrightnessContrast(p=0.2), GaussianBlur(blur_limit=(3, 7), p=0.3),
    ElasticTransform(alpha=1, sigma=50, p=0.3)])`, then the per-sample min-max of :113) for a batch of DeviceImages indices ->
    {'image' [B, C, H, W] float32, 'label' [B, H, W] float32 class ids} on the device (csrc/augment_image_ops.hip).

    What this reproduces is the pipeline's operator family and its distribution — which operators, in what ranges, each with its
    own probability, in the reference's order — with every operator specified by scipy (include/cenet_hip.h,
    cenet_augment_image_ops).  It does not reproduce albumentations' numbers: albumentations' random stream, its cv2 interpolation
    and its uint8 LUT rounding are not pinned here.  The brightness / contrast limits 0.2 and the scaling of the brightness term
    by 255 for uint8 images are albumentations' defaults as remembered from its source: unverified.

    The augmenter owns a numpy Generator (`seed`) and never touches the global `random` / `np.random` streams.  `draw` walks
    `ops` in order for every sample, each op fires with its own `p` and draws its parameters; the names that fired in the last draw
    are kept in `picked`.  All elastic ops of `ops` share one (sigma, truncate): the field kernel is one per call."""

    def __init__(self, images: DeviceImages, ops=SKIN_OPS, minmax: bool = True, seed=None):
        self.images, self.ops, self.minmax = images, tuple(ops), bool(minmax)
        if len(self.ops) > AUG_MAX_STAGES:
            raise ValueError(f"ComposeAugmenter: at most {AUG_MAX_STAGES} ops per sample")
        fields = {(float(p["sigma"]), float(p.get("truncate", 4.0))) for n, p in self.ops if n == "elastic"}
        if len(fields) > 1:
            raise ValueError("ComposeAugmenter: one (sigma, truncate) for all elastic ops")
        self.field = fields.pop() if fields else None
        self.rng = np.random.default_rng(seed)
        self.picked = []
        self._buf = {}

    # ---- one fired transform -> the kernel's op: (kind, *parameters) -----------------------------------------------------------------
    def _draw_op(self, name, prm):
        rng, H, W = self.rng, self.images.height, self.images.width
        if name in ("flip_ud", "flip_lr"):
            return (name,)
        if name == "rotate":
            a = np.deg2rad(rng.uniform(*prm["degrees"]))
            return ("affine", *centred_affine([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], (H, W)), prm.get("mode", "constant"))
        if name == "brightness_contrast":
            alpha, beta = 1.0 + rng.uniform(*prm["contrast"]), prm["max_value"] * rng.uniform(*prm["brightness"])
            return ("brightness_contrast", float(alpha), float(beta), 0.0, float(prm["max_value"]))
        if name == "blur":
            return ("blur", int(rng.choice(prm["kernel"])))
        if name == "elastic":
            k0, k1 = (int(v) for v in rng.integers(0, 2 ** 32, 2, dtype=np.uint64))
            return ("elastic", float(prm["alpha"]), k0, k1, prm.get("mode", "constant"))
        raise ValueError(f"ComposeAugmenter: unknown op {name!r}")

    def plan(self, indices: Sequence[int], chains: Sequence[Sequence[tuple]], field=None):
        """the (tab, dp, fw) tables of cenet_augment_image_ops for explicit per-sample chains of kernel ops: ('copy',),
        ('flip_ud',), ('flip_lr',), ('affine', M [2, 2], offset [2], mode), ('blur', k) or ('blur', weights [radius + 1]),
        ('brightness_contrast', alpha, beta, lo, hi), ('elastic', alpha, key0, key1, mode); mode 'constant' / 'mirror'; shorter
        chains end in copies.  field: (sigma, truncate) of the elastic kernel (default: the augmenter's own); fw is its
        gaussian_weights [radius + 1], or None when no chain is elastic"""
        from .kern import AUG_IMAGE_MIRROR, AUG_IMAGE_OPS, AUG_OPS_DP
        S = max(1, max((len(c) for c in chains), default=0))
        tab = np.zeros((len(indices), 1 + S), dtype=np.int64)
        dp = np.zeros((len(indices), S, AUG_OPS_DP), dtype=np.float64)
        elastic = False
        for n, (idx, chain) in enumerate(zip(indices, chains)):
            tab[n, 0] = idx
            for s, (kind, *a) in enumerate(chain):
                word, row = AUG_IMAGE_OPS[kind], dp[n, s]
                if kind == "affine":
                    row[0:4], row[4:6] = np.asarray(a[0], dtype=np.float64).reshape(-1), a[1]
                elif kind == "blur":
                    radius, w = blur_weights(a[0]) if np.ndim(a[0]) == 0 else (len(a[0]) - 1, np.asarray(a[0], dtype=np.float64))
                    row[0] = radius
                    if radius <= AUG_MAX_RADIUS:  # (a larger one is left for the library to refuse)
                        row[1:2 + radius] = w
                elif kind == "brightness_contrast":
                    row[0:4] = a
                elif kind == "elastic":
                    row[0:3] = a[0:3]
                    elastic = True
                if kind in ("affine", "elastic"):
                    mode = a[-1]
                    assert mode in ("constant", "mirror"), mode
                    word += AUG_IMAGE_MIRROR * (mode == "mirror")
                tab[n, 1 + s] = word
        fw = None
        if elastic:
            field = self.field if field is None else field
            assert field is not None, "an elastic op needs the field's (sigma, truncate)"
            fw = np.ascontiguousarray(gaussian_weights(*field)[1])
        return tab, dp, fw

    def draw(self, indices: Sequence[int]):
        chains, self.picked = [], []
        for _ in indices:
            fired = [(n, p) for n, p in self.ops if self.rng.random() < p["p"]]
            self.picked.append(tuple(n for n, _ in fired))
            chains.append([self._draw_op(n, p) for n, p in fired])
        return self.plan(indices, chains)

    def apply(self, plan) -> dict:
        from . import kern
        tab, dp, fw = plan
        im, dev = self.images, self.images.device
        B, S = tab.shape[0], tab.shape[1] - 1
        C, H, W = im.channels, im.height, im.width
        n = C * H * W
        if self._buf.get("B", 0) < B:
            self._buf = {"B": B, "img": [torch.empty(B * n, dtype=torch.float32, device=dev) for _ in range(2)],
                         "lab": [torch.empty(B * H * W, dtype=torch.uint8, device=dev) for _ in range(2)],
                         "part": torch.empty(B * 2 * kern.AUG_MINMAX_PARTS, dtype=torch.float32, device=dev), "field": None}
        buf = self._buf
        if fw is not None and buf["field"] is None:
            buf["field"] = torch.empty(buf["B"] * 2 * H * W, dtype=torch.float64, device=dev)
        pin = dev.type == "cuda"
        up = []
        for a in (tab, dp, fw):
            t = None if a is None else torch.from_numpy(a)
            up.append(None if t is None else (t.pin_memory() if pin else t).to(dev, non_blocking=True))
        label = torch.empty(B, H, W, dtype=torch.float32, device=dev)
        r = kern.augment_image_ops(im.pool_img, im.pool_lab, tab, dp, up[0], up[1], fw, up[2], buf["field"] if fw is not None else None,
                                   buf["img"], buf["lab"], label, len(im), C, H, W, B, S)
        if self.minmax:
            image = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
            kern.augment_minmax(buf["img"][r], image, buf["part"], B, n)
        else:
            image = buf["img"][r][:B * n].view(B, C, H, W).clone()
        return {"image": image, "label": label}

    def __call__(self, indices: Sequence[int]) -> dict:
        return self.apply(self.draw(indices))


class DeviceTrainLoader:
    """`DataLoader(db_train, batch_size=B, shuffle=True)` (main_acdc.py:140) over DeviceSlices: the index order is torch's own
    RandomSampler / BatchSampler (and one draw for the iterator's base seed, as DataLoader makes), so the same torch seed gives
    the reference's batches; every batch is {'image', 'label', 'case_name'} with the tensors already on the device."""

    def __init__(self, slices: DeviceSlices, output_size: Sequence[int], batch_size: int, shuffle: bool = True,
                 drop_last: bool = False, generator: Optional[torch.Generator] = None, sampler=None, augmenter=None):
        """sampler: an index sampler over range(len(slices)) instead of the shuffle — one process per GPU passes
        `DistributedSampler(range(len(slices)), num_replicas=world, rank=rank)` (and calls its set_epoch), exactly as with a DataLoader;
        every rank keeps the whole set resident (0.35 GB) and augments its own shard.
        augmenter: called with a batch's indices in place of the built-in DeviceAugmenter (a SegAugmenter over the same slices for
        the Synapse pipeline; a ComposeAugmenter over DeviceImages, passed as `slices`, for the skin pipeline); output_size is the
        built-in augmenter's and unused then."""
        from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
        self.slices, self.aug = slices, augmenter if augmenter is not None else DeviceAugmenter(slices, output_size)
        self.generator = generator
        src = range(len(slices))
        if sampler is None:
            sampler = RandomSampler(src, generator=generator) if shuffle else SequentialSampler(src)
        self.sampler = sampler
        self.batch_sampler = BatchSampler(sampler, batch_size, drop_last)

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self) -> Iterator[dict]:
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)  # _BaseDataLoaderIter's base-seed draw
        for idx in self.batch_sampler:
            batch = self.aug(idx)
            if self.slices.names is not None:
                batch["case_name"] = [self.slices.names[i] for i in idx]
            yield batch
