"""Unpaired 3-D volume dataset with the reference's training-patch path (second half).

The reference keeps its 3-D datasets in the projects (e.g. projects/brats_mri_sequence_translation/datasets/
train_dataset.py:47-96): load two volumes (A by index, B at random — `random.randint`), draw a pair of spatially
corresponding patches with `StochasticFocalPatchSampler`, `z_score_normalize(patch, scale_to_range=(-1, 1))` each, add
the channel axis. Their file readers are SimpleITK, which this image does not have; `UnpairedVolumeDataset` is the same
`__getitem__` over `.npy` volumes in `<root>/A` and `<root>/B` (fp32 or int16, (D, H, W)), and
`BratsDatasetConfig`'s fields (`patch_size`, `focal_region_proportion`) keep their names.

With `device_transforms: true` the volumes live in HBM (uploaded on first use and kept — a few hundred 36-MB volumes are
nothing against 288 GB) and a sample is only ("A", index, start) coordinates: `DeviceVolumePipeline` crops and
normalises on the GPU (csrc/volproc.hip) in front of `set_input`, through the same Trainer hook as the image pipeline.

`augmentation` (not in the reference; data/utils/patch_affine.py, 3-D patch sizes only) replaces the crop by one trilinear
gather through a random 3 x 3 matrix per domain — flips, rotation, zoom, `fill` outside the volume — in front of the same
z-score; the patch starts still come from `random`, the matrices from `np.random` (A's eight uniforms, then B's). With
its `elastic` key a free-form deformation (control-point lattice, cubic B-splines) precedes the matrix inside the same
gather, and each set takes 1 + 3 G_0 G_1 G_2 further uniforms after its eight. Its `intensity` key
(data/utils/patch_intensity.py) runs bias field, contrast, brightness, gamma and noise on the z-score's normalised value in
front of its last step; each domain's block of 7 (+ 1 + G_0 G_1 G_2) uniforms follows its geometric set, and `modalities`
names the domains ("A" / "B")."""
import random
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import configs
from .device_transforms import collate_raw
from .utils.normalization import z_score_normalize
from .utils.patch_affine import check_elastic, draw_set, matrix_tuple, parse_augmentation, sample_patch
from .utils.patch_intensity import active, bias_field, check_intensity, draw_block, z_score_intensity
from .utils.stochastic_focal_patching import StochasticFocalPatchSampler

EXTENSIONS = [".npy"]


@dataclass
class UnpairedVolumeDatasetConfig(configs.base.BaseDatasetConfig):
    patch_size: Tuple[int, ...] = field(default_factory=lambda: [32, 32, 32])
    # proportion of the focal region's size to the volume's (stochastic_focal_patching.py:18-19)
    focal_region_proportion: float = 0
    # not in the reference: volumes resident in HBM, crop + normalisation on the GPU (data/device_volumes.py)
    device_transforms: bool = False
    # not in the reference: random flips / rotation / zoom of every patch as one trilinear gather (data/utils/
    # patch_affine.py): {prob, flip: [D, H, W], rotate_deg: [D, H, W], scale: [lo, hi], spacing: [D, H, W], fill,
    # elastic: {prob, control_points: [D, H, W], max_displacement: [D, H, W] in the units of spacing},
    # intensity: {prob, modalities, gamma, contrast, brightness, noise_std: [lo, hi] each, bias_field: {prob,
    # control_points, max}} (data/utils/patch_intensity.py)}
    augmentation: Optional[Dict[str, Any]] = None


class RawPatch:
    """what a worker hands over with device_transforms on: which volume, where the patch starts, its augmentation
    matrix (9 floats, row-major) or None, and next to it the elastic field (float64 [3, G0, G1, G2], already in voxels)
    or None, and last the intensity block of its domain — (rows, bias lattice): one row (gamma, contrast, brightness,
    noise_std, bias, key0, key1) and float64 [G0, G1, G2] or None — or None"""
    __slots__ = ("domain", "index", "start", "matrix", "field", "intensity")

    def __init__(self, domain, index, start, matrix=None, field=None, intensity=None):
        self.domain, self.index, self.start = domain, int(index), tuple(int(v) for v in start)
        self.matrix = None if matrix is None else matrix_tuple(matrix)
        self.field = field
        self.intensity = intensity


class UnpairedVolumeDataset(Dataset):

    def __init__(self, conf):
        d = conf[conf.mode].dataset
        root = Path(d.root)
        self.paths = {k: sorted(p for p in (root / k).rglob("*") if p.suffix.lower() in EXTENSIONS) for k in ("A", "B")}
        assert self.paths["A"] and self.paths["B"], f"no .npy volumes under {root}/A or {root}/B"
        self.patch_size = np.array([int(v) for v in d.patch_size])
        self.patch_sampler = StochasticFocalPatchSampler(self.patch_size, d.focal_region_proportion)
        try:
            self.raw = bool(d["device_transforms"])
        except (KeyError, AttributeError):
            self.raw = False
        try:
            node = d["augmentation"]
        except (KeyError, AttributeError):
            node = None
        self.augmentation = parse_augmentation(node, fill_allowed=True)
        if self.augmentation is not None and self.patch_sampler.dims != 3:
            raise ValueError(f"augmentation needs a 3-D patch_size (D, H, W); got {[int(v) for v in self.patch_size]}")
        check_elastic(self.augmentation, self.patch_size)
        check_intensity(self.augmentation and self.augmentation.intensity, self.patch_size, ("A", "B"))
        self._shapes = {}

    def load(self, domain, index):
        """(D, H, W) tensor of one volume, in the dtype it is stored in (fp32 / int16 stay as they are)"""
        v = np.load(self.paths[domain][index], mmap_mode="r")
        assert v.ndim == 3, f"{self.paths[domain][index]}: expected a (D, H, W) array, got {v.shape}"
        return torch.from_numpy(np.ascontiguousarray(v))

    def shape(self, domain, index):
        key = (domain, index)
        if key not in self._shapes:
            self._shapes[key] = tuple(np.load(self.paths[domain][index], mmap_mode="r").shape)
        return self._shapes[key]

    def __getitem__(self, index):
        index_A = index % len(self.paths["A"])
        index_B = random.randint(0, len(self.paths["B"]) - 1)
        aug = self.augmentation
        if self.raw:
            start_A, start_B = self.patch_sampler.get_start_pair(self.shape("A", index_A), self.shape("B", index_B))
            set_A, set_B = self.draw_sets()
            return {"A": RawPatch("A", index_A, start_A, *set_A), "B": RawPatch("B", index_B, start_B, *set_B)}
        A, B = self.load("A", index_A).float(), self.load("B", index_B).float()
        if aug:
            start_A, start_B = self.patch_sampler.get_start_pair(A.shape, B.shape)
            size = [int(v) for v in self.patch_size]
            (M_A, field_A, int_A), (M_B, field_B, int_B) = self.draw_sets()
            A = torch.from_numpy(sample_patch(A.numpy(), None, start_A, size, M_A, aug.fill, field_A))
            B = torch.from_numpy(sample_patch(B.numpy(), None, start_B, size, M_B, aug.fill, field_B))
        else:
            A, B = self.patch_sampler.get_patch_pair(A, B)
            int_A = int_B = None
        return {"A": self.normalize(A, int_A).unsqueeze(0), "B": self.normalize(B, int_B).unsqueeze(0)}

    def draw_sets(self):
        """((M_A, field_A, intensity_A), (M_B, field_B, intensity_B)): A's geometric set, A's intensity block
        (patch_intensity.draw_block, only with `intensity`), then B's set and B's block; all None without `augmentation`"""
        aug = self.augmentation
        if not aug:
            return (None, None, None), (None, None, None)
        block = lambda k: None if aug.intensity is None else draw_block(aug.intensity, (k,))
        set_A = draw_set(aug)
        int_A = block("A")
        set_B = draw_set(aug)
        return (*set_A, int_A), (*set_B, block("B"))

    def normalize(self, patch, intensity):
        """the z-score to [-1, 1]; a patch whose intensity row came out neutral (or that carries none) takes the plain one"""
        intensity = active(intensity)
        if intensity is None:
            return z_score_normalize(patch, scale_to_range=(-1, 1))
        (row,), lattice = intensity
        beta = None if lattice is None else bias_field([int(v) for v in self.patch_size], lattice)
        return z_score_intensity(patch, row, beta, (-1.0, 1.0))

    def __len__(self):
        return max(len(self.paths["A"]), len(self.paths["B"]))

    # ---- picked up by build_loader / Trainer ----------------------------------------------------------------------
    @property
    def collate_fn(self):
        return collate_raw if self.raw else None

    def device_pipeline(self, conf, device):
        if not self.raw:
            return None
        from .device_volumes import DeviceVolumePipeline
        return DeviceVolumePipeline(self, device)
