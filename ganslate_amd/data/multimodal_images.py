"""Multi-modal 2-D image datasets: several float and 8-bit modalities per sample, stacked along channels — the training
set and the val / test set of the reference's ClearGrasp project (projects/cleargrasp_depth_estimation/datasets/
train_dataset.py:75-146, val_test_dataset.py:80-167), the data its cyclegan_balanced.yaml, cyclegan_naive.yaml and
pix2pix_new.yaml experiments are trained on: A = [rgb | normal], B = [rgb | depth] or [depth].

Layout: `<root>/<modality>/<file>`, e.g. `rgb/`, `normal/`, `depth/`. The files of a modality are sorted by name and matched
across modalities by position, like the reference's; unequal counts are an error. A file is a `.npy` of shape (H, W) or
(H, W, C), uint8 or float32, or — for 8-bit modalities — anything Pillow decodes (read as RGB or L). The reference reads
EXR through cv2; EXR is not read here: convert it to `.npy` once. The reference hard-codes its three modalities, their
ranges and which of them gets noise; here those are config fields.

Per modality, in the reference's order: the image as fp32 CHW -> `transforms.Resize((load_size[1], load_size[0]), BICUBIC)`
on the TENSOR, which is `F.interpolate(x, size, mode="bicubic", align_corners=False)` without antialiasing (`bicubic_taps`
states it per axis) -> clamp to `clip_range` -> with `rescale` min-max to [-1, 1] (the normal map is clamped only) -> in
training, with `noise_std`, `+ torch.normal(0, std, size=(H, W))` and clamp(-1, 1): ONE plane broadcast over the
modality's channels -> concat along channels. A stored size equal to `load_size` gives weights (0, 1, 0, 0): the resize is
then a bit-exact copy (the case of the reference's own pre-resized data). The reference's `apply_transforms` is the identity.

Training (train_dataset.py:80-81): index_A = index % n, index_B = index_A when paired, else random.randint(0, n - 1). The
line `index_A, index_B = 9, 1` that follows there (train_dataset.py:82) is a debugging leftover that pins every sample to
the same two files; it is NOT reproduced.

Val / test is paired. `dummy_channels_B: [front, back]` puts zero channels around B ([3, 0] is the reference's
`model_is_cyclegan_balanced`), `metadata = {"sample_id": ...}` is the stem of the first A modality's file without its last
`-`-separated field (val_test_dataset.py:59), `denormalize` maps [-1, 1] back to the range of `denormalize_modality`, and
`save` writes that modality's generated channels as `<save_dir>/<sample_id>.npy` (the reference writes EXR).

With `device_transforms: true` a training sample is two indices plus the key words of its noise planes, a val / test /
infer sample an index plus metadata; the decoded images stay resident in HBM as stored and DeviceMultiModalImagePipeline
(data/device_images.py) builds each domain's batch tensor with one gs_img_stack launch (csrc/imgstack.hip)."""
import math
import random
from dataclasses import dataclass, field
from functools import lru_cache
from pathlib import Path
from typing import Any, Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import Dataset

from .. import configs
from .device_transforms import collate_raw
from .multimodal_volumes import _field
from .utils.normalization import min_max_denormalize, min_max_normalize

PIL_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".tif", ".tiff")
CUBIC_A = -0.75


@dataclass
class MultiModalImageDatasetConfig(configs.base.BaseDatasetConfig):
    paired: bool = True
    # folder names per domain, in channel order: {A: [rgb, normal], B: [rgb, depth]}; a folder may appear in both
    modalities: Dict[str, Any] = field(default_factory=dict)
    clip_range: Dict[str, Any] = field(default_factory=dict)        # {name: [min, max]}, required for every name
    rescale: Dict[str, Any] = field(default_factory=dict)           # {name: bool}, default true; false: clamp only
    noise_std: Dict[str, Any] = field(default_factory=dict)         # {A: {name: std}, B: {name: std}}; reference: B rgb 0.05
    load_size: Tuple[int, int] = (512, 256)                         # (W, H), the reference's order
    # not in the reference: images resident in HBM, resize + normalisation + noise + concat on the GPU (data/device_images.py)
    device_transforms: bool = False


@dataclass
class MultiModalImageValTestDatasetConfig(configs.base.BaseDatasetConfig):
    modalities: Dict[str, Any] = field(default_factory=dict)        # {A: [rgb, normal], B: [depth]}
    clip_range: Dict[str, Any] = field(default_factory=dict)
    rescale: Dict[str, Any] = field(default_factory=dict)
    load_size: Tuple[int, int] = (512, 256)
    dummy_channels_B: Tuple[int, int] = (0, 0)                      # zero channels [front, back] around B's
    denormalize_modality: Optional[str] = None                      # B modality whose range `denormalize` and `save` undo
    device_transforms: bool = False


class TapTable(NamedTuple):
    """the four taps of every output index of one axis: idx int32 [n_out, 4], w fp32 [n_out, 4]"""
    idx: Any
    w: Any
    n_in: int
    n_out: int


def cubic_weights(t):
    """c2(t + 1), c1(t), c1(1 - t), c2(2 - t) of the cubic convolution with A = -0.75"""
    A = CUBIC_A
    c1 = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    c2 = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)


@lru_cache(maxsize=256)
def bicubic_taps(n_in: int, n_out: int):
    """One axis of torch's bicubic interpolation (align_corners=False, no antialiasing), n_in -> n_out, in float64 and
    rounded once to fp32: s = (o + 0.5) * n_in / n_out - 0.5, f = floor(s), t = s - f, taps f-1 .. f+2 clamped to
    [0, n_in - 1]. n_out == n_in gives t = 0 and the weights (0, 1, 0, 0) exactly."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"bicubic_taps: sizes must be positive; got {n_in} -> {n_out}")
    idx = np.empty((n_out, 4), np.int32)
    w = np.empty((n_out, 4), np.float64)
    for o in range(n_out):
        s = (o + 0.5) * n_in / n_out - 0.5
        f = math.floor(s)
        w[o] = cubic_weights(s - f)
        idx[o] = [min(max(f + j, 0), n_in - 1) for j in (-1, 0, 1, 2)]
    return TapTable(idx, w.astype(np.float32), n_in, n_out)


def read_image(path):
    """(H, W) or (H, W, C) array, uint8 or float32, as stored"""
    path = Path(path)
    if path.suffix.lower() == ".npy":
        v = np.load(path)
        if v.ndim not in (2, 3) or v.dtype not in (np.uint8, np.float32):
            raise ValueError(f"{path}: expected a (H, W) or (H, W, C) array of uint8 or float32, got {v.shape} {v.dtype}")
        return v
    from PIL import Image
    with Image.open(path) as img:
        return np.asarray(img.convert("L" if img.mode in ("1", "L", "LA") else "RGB"))


def list_files(folder):
    folder = Path(folder)
    if not folder.is_dir():
        raise ValueError(f"no modality folder {folder}")
    names = sorted(p.name for p in folder.iterdir() if p.is_file())
    exr = [n for n in names if n.lower().endswith(".exr")]
    if exr:
        raise ValueError(f"{folder} holds EXR files ({exr[0]}, ...): EXR is not read here, convert them to .npy once")
    return [n for n in names if n.lower().endswith((".npy",) + PIL_EXTENSIONS)]


class RawImageSample:
    """what a worker hands over with device_transforms on: which sample of a domain, and per modality with noise the two
    32-bit key words of its plane"""
    __slots__ = ("domain", "index", "keys")

    def __init__(self, domain, index, keys=None):
        self.domain, self.index, self.keys = domain, int(index), dict(keys or {})


class _MultiModalImages(Dataset):
    """files, ranges and the host chain shared by the training and the val / test set"""

    def _init_common(self, conf):
        self.mode = str(conf.mode)
        d = conf[conf.mode].dataset
        self.root = Path(d.root)
        mods = _field(d, "modalities", {})
        self.modalities = {k: [str(n) for n in (mods[k] if k in mods else [])] for k in ("A", "B")}
        if not self.modalities["A"] or not self.modalities["B"]:
            raise ValueError(f"modalities needs at least one folder name for A and for B; got {self.modalities}")
        names = list(dict.fromkeys(self.modalities["A"] + self.modalities["B"]))
        clip = _field(d, "clip_range", {})
        missing = [n for n in names if n not in clip]
        if missing:
            raise ValueError(f"clip_range has no entry for {missing}")
        self.clip_range = {n: (float(clip[n][0]), float(clip[n][1])) for n in names}
        if any(hi <= lo for lo, hi in self.clip_range.values()):
            raise ValueError(f"clip_range entries need min < max: {self.clip_range}")
        rescale = _field(d, "rescale", {})
        self.rescale = {n: bool(rescale[n]) if n in rescale else True for n in names}
        load = [int(v) for v in d.load_size]
        if len(load) != 2 or min(load) < 1:
            raise ValueError(f"load_size must be two positive sizes (W, H); got {load}")
        self.size = (load[1], load[0])                               # (H, W)
        self.files = {n: list_files(self.root / n) for n in names}
        counts = {str(self.root / n): len(f) for n, f in self.files.items()}
        if len(set(counts.values())) != 1:
            raise ValueError(f"the modality folders hold different numbers of files: {counts}")
        if not next(iter(counts.values())):
            raise ValueError(f"no image files under {list(counts)}")
        first = {n: read_image(self.root / n / self.files[n][0]) for n in names}
        self.channels = {n: 1 if v.ndim == 2 else int(v.shape[2]) for n, v in first.items()}
        self.stored_ndim = {n: v.ndim for n, v in first.items()}
        self.raw = bool(_field(d, "device_transforms", False))

    def __len__(self):
        return len(self.files[self.modalities["A"][0]])

    def domain_channels(self, domain):
        return sum(self.channels[n] for n in self.modalities[domain])

    def load(self, name, index):
        """(H, W) or (H, W, C) array of one file, in the dtype it is stored in"""
        path = self.root / name / self.files[name][index]
        v = read_image(path)
        if (1 if v.ndim == 2 else v.shape[2]) != self.channels[name]:
            raise ValueError(f"{path}: {v.shape} does not have the {self.channels[name]} channel(s) of "
                             f"{self.files[name][0]}")
        return v

    # ---- host path ------------------------------------------------------------------------------------------------------
    def prepare(self, name, array, noise_std=0.0):
        """fp32 [C, H, W] of one modality: tensor resize -> clamp -> min-max -> noise plane (module docstring)"""
        lo, hi = self.clip_range[name]
        x = torch.from_numpy(np.array(array)).float()                 # a copy: Pillow hands out read-only arrays
        x = x.unsqueeze(0) if x.dim() == 2 else x.permute(2, 0, 1)
        x = F.interpolate(x.unsqueeze(0).contiguous(), size=self.size, mode="bicubic", align_corners=False)[0]
        x = torch.clamp(x, lo, hi)
        if self.rescale[name]:
            x = min_max_normalize(x, lo, hi)
        if noise_std:
            x = torch.clamp(x + torch.normal(mean=0.0, std=float(noise_std), size=self.size), -1, 1)
        return x

    def stack(self, domain, index, noise=None):
        return torch.cat([self.prepare(n, self.load(n, index), (noise or {}).get(n, 0.0)) for n in self.modalities[domain]])

    # ---- picked up by build_loader and the engines ----------------------------------------------------------------------
    @property
    def collate_fn(self):
        return collate_raw if self.raw else None

    def device_pipeline(self, conf, device):
        if not self.raw:
            return None
        from .device_images import DeviceMultiModalImagePipeline
        return DeviceMultiModalImagePipeline(self, device)


class MultiModalImageDataset(_MultiModalImages):

    def __init__(self, conf):
        self._init_common(conf)
        self.paired = bool(_field(conf[conf.mode].dataset, "paired", True))
        noise = _field(conf[conf.mode].dataset, "noise_std", {})
        self.noise_std = {}
        for k in ("A", "B"):
            node = noise[k] if k in noise and noise[k] is not None else {}
            self.noise_std[k] = {str(n): float(node[n]) for n in node if node[n] is not None and float(node[n]) != 0.0}
            unknown = [n for n in self.noise_std[k] if n not in self.modalities[k]]
            if unknown or any(v < 0 for v in self.noise_std[k].values()):
                raise ValueError(f"noise_std.{k} must give a std >= 0 for modalities of {self.modalities[k]}; got "
                                 f"{self.noise_std[k]}")

    def domains(self):
        return ("A", "B")

    def dummy_channels(self, domain):
        return (0, 0)

    def __getitem__(self, index):
        n = len(self)
        index_A = index % n
        index_B = index_A if self.paired else random.randint(0, n - 1)
        if self.raw:
            # two 32-bit words per noise plane from np.random, in the order A's modalities, then B's
            keys = {k: {m: tuple(int(v) for v in np.random.randint(0, 1 << 32, size=2, dtype=np.uint64))
                        for m in self.modalities[k] if m in self.noise_std[k]} for k in ("A", "B")}
            return {"A": RawImageSample("A", index_A, keys["A"]), "B": RawImageSample("B", index_B, keys["B"])}
        return {"A": self.stack("A", index_A, self.noise_std["A"]), "B": self.stack("B", index_B, self.noise_std["B"])}


class MultiModalImageValTestDataset(_MultiModalImages):

    def __init__(self, conf):
        self._init_common(conf)
        d = conf[conf.mode].dataset
        self.noise_std = {"A": {}, "B": {}}
        self.dummy_channels_B = tuple(int(v) for v in _field(d, "dummy_channels_B", (0, 0)))
        if len(self.dummy_channels_B) != 2 or min(self.dummy_channels_B) < 0:
            raise ValueError(f"dummy_channels_B must be two counts [front, back]; got {self.dummy_channels_B}")
        self.denormalize_modality = str(_field(d, "denormalize_modality", self.modalities["B"][0]))
        if self.denormalize_modality not in self.modalities["B"]:
            raise ValueError(f"denormalize_modality must name one of B's modalities {self.modalities['B']}; got "
                             f"{self.denormalize_modality!r}")
        self.sample_ids = [self.sample_id(name) for name in self.files[self.modalities["A"][0]]]

    @staticmethod
    def sample_id(file_name):
        """`000000012-rgb.jpg` -> `000000012`: the stem without its last `-`-separated field (val_test_dataset.py:59); a stem
        without a `-` stays whole (the reference's expression would leave nothing of it)"""
        stem = Path(file_name).stem
        return stem.rsplit("-", 1)[0] if "-" in stem else stem

    def domains(self):
        return ("A",) if self.mode == "infer" else ("A", "B")

    def dummy_channels(self, domain):
        return self.dummy_channels_B if domain == "B" else (0, 0)

    def add_dummies(self, B):
        front, back = self.dummy_channels_B
        zeros = lambda n: B.new_zeros((n, *B.shape[1:]))
        return torch.cat([zeros(front), B, zeros(back)]) if front or back else B

    def __getitem__(self, index):
        index = index % len(self)
        meta = {"sample_id": self.sample_ids[index]}
        if self.raw:
            sample = {k: RawImageSample(k, index) for k in self.domains()}
        else:
            sample = {k: self.stack(k, index) for k in self.domains()}
            if "B" in sample:
                sample["B"] = self.add_dummies(sample["B"])
        sample["metadata"] = meta
        return sample

    # ---- picked up by the engines -----------------------------------------------------------------------------------------
    def denormalize(self, tensor):
        """[-1, 1] back to the clip range of `denormalize_modality`, IN PLACE like the reference's; a modality that is only
        clamped is left as it is"""
        if not self.rescale[self.denormalize_modality]:
            return tensor
        return min_max_denormalize(tensor, *self.clip_range[self.denormalize_modality])

    def save(self, tensor, save_dir, metadata):
        """the channels of `denormalize_modality` of one generated sample, denormalised, without the dummy channels, as
        `<save_dir>/<sample_id>.npy` (fp32): (H, W) for a modality stored as (H, W), else (H, W, C). `tensor` is the whole
        domain tensor with or without the dummy channels, or that modality's channels alone; any other channel count is
        refused"""
        names = self.modalities["B"]
        m = self.denormalize_modality
        j = sum(self.channels[n] for n in names[:names.index(m)])
        total = self.domain_channels("B")
        if tensor.shape[0] == total + sum(self.dummy_channels_B):
            j += self.dummy_channels_B[0]
        elif tensor.shape[0] == self.channels[m] and tensor.shape[0] != total:
            j = 0                                             # a generator that emits the translated channels only
        elif tensor.shape[0] != total:
            raise ValueError(f"save: a tensor of {tensor.shape[0]} channels is neither B's {total} channels, nor those with the "
                             f"dummy channels {list(self.dummy_channels_B)} around them, nor the {self.channels[m]} of `{m}`")
        out = self.denormalize(tensor[j:j + self.channels[m]].detach().float().cpu().clone())
        out = out[0] if self.stored_ndim[m] == 2 else out.permute(1, 2, 0)
        path = Path(save_dir) / f"{metadata['sample_id']}.npy"
        path.parent.mkdir(parents=True, exist_ok=True)
        np.save(path, np.ascontiguousarray(out.numpy().astype(np.float32)))
        return path
