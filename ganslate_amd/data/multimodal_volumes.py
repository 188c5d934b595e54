"""Multi-modal volume dataset with body-mask patch sampling: the training set of the reference's HX4-PET project
(projects/maastro_hx4_pet_translation/datasets/train_dataset.py, datasets/utils/patch_samplers.py, datasets/utils/basic.py)
— the data the Pix2Pix (Unet3D + PatchGAN3D) and CycleGANBalanced recipes are trained on there.

Layout: `<root>/<case>/<name>.npy`, dense (D, H, W) arrays; images fp32 or int16, masks uint8 or bool; cases sorted by
name. The reference reads NRRD through SimpleITK and hard-codes its four modalities; here the modalities, their clip ranges,
the value outside the body and the optional per-case divisor (the reference's aorta-SUV normalisation) are config fields.

Per sample (train_dataset.py:106-188): index_A = index % n, index_B = index_A when paired, else random.randint(0, n - 1);
the patch centre ("focal point") is drawn inside the body mask and the valid zone, uniformly or weighted by one of A's
modalities; paired training uses the same point (and A's mask and case) for B, unpaired training the stochastic-focal
variant: B's point is drawn uniformly inside the body within a box around the corresponding point. Every draw consumes one
`np.random` uniform, like the reference's `np.random.choice(p=...)`.

The selection rule — shared by this host path, the device kernel (csrc/volsample.hip, gs_voxel_draw) and the test oracle —
is stated at `draw_focal_point`. With `device_transforms: true` a sample is only case indices and uniforms; the volumes
stay resident in HBM and `DeviceMultiModalPipeline` (data/device_volumes.py) draws, crops and normalises on the GPU.

`augmentation` (not in the reference; data/utils/patch_affine.py) turns the crop into one trilinear gather through a random
3 x 3 matrix — flips, rotation, zoom — round the same patch centre: mask, then interpolate, then the same normalisation.
Its eight `np.random` uniforms per matrix follow the sample's draws above (one matrix for a paired sample, A's then B's
otherwise); without the field nothing changes, the random streams included. Its `elastic` key adds a free-form
deformation in front of the matrix — a lattice of control-point displacements, cubic B-splines — inside the same gather;
each set then takes 1 + 3 G_0 G_1 G_2 further uniforms after its eight, and a paired sample shares one field."""
import json
import math
import random
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import configs
from .device_transforms import collate_raw
from .utils.normalization import min_max_normalize
from .utils.patch_affine import check_elastic, draw_set, matrix_tuple, parse_augmentation, sample_patch
from .utils.patch_intensity import active, apply, bias_field, check_intensity, draw_block, is_neutral

PAIRED_SAMPLING_SCHEMES = ("uniform-random-within-body", "fdg-pet-weighted")
UNPAIRED_SAMPLING_SCHEMES = ("uniform-random-within-body-sf", "fdg-pet-weighted-sf")


@dataclass
class MultiModalVolumeDatasetConfig(configs.base.BaseDatasetConfig):
    paired: bool = True
    # file stems per domain, in channel order: {A: [fdg_pet, pct], B: [hx4_pet]}
    modalities: Dict[str, Any] = field(default_factory=dict)
    # mask file stem per domain; paired training uses A's mask (and A's case) for B, as the reference does
    body_mask: Dict[str, Any] = field(default_factory=dict)
    clip_range: Dict[str, Any] = field(default_factory=dict)        # {name: [min, max]}
    outside_value: Dict[str, Any] = field(default_factory=dict)     # {name: value outside the body}; reference: CT -1024, PET 0
    divisors: Optional[str] = None                                  # JSON file {name: {case: value}}; default divisor 1
    patch_size: Tuple[int, int, int] = (32, 128, 128)               # DHW
    patch_sampling: str = "uniform-random-within-body"
    weight_modality: Optional[str] = None                           # the A modality behind the weighted schemes
    focal_region_proportion: Tuple[float, float, float] = (0.6, 0.3, 0.3)   # DHW, unpaired only
    # not in the reference: volumes resident in HBM, draw + crop + normalisation on the GPU (data/device_volumes.py)
    device_transforms: bool = False
    # not in the reference: random flips / rotation / zoom of every patch as one trilinear gather (data/utils/
    # patch_affine.py): {prob, flip: [D, H, W], rotate_deg: [D, H, W], scale: [lo, hi], spacing: [D, H, W],
    # elastic: {prob, control_points: [D, H, W], max_displacement: [D, H, W] in the units of spacing},
    # intensity: {prob, modalities, gamma, contrast, brightness, noise_std: [lo, hi] each, bias_field: {prob,
    # control_points, max}} (data/utils/patch_intensity.py)}
    augmentation: Optional[Dict[str, Any]] = None


def valid_zone(size, patch):
    """per axis [floor(p / 2), size - ceil(p / 2)), upper bound exclusive (get_valid_region_corner_points)"""
    return [int(p) // 2 for p in patch], [int(s) - (int(p) + 1) // 2 for s, p in zip(size, patch)]


def focal_box(focal_A, size_A, size_B, proportion):
    """the stochastic-focal box in B around A's point (_sample_focal_point_B, _apply_stochastic_focal_method), float64"""
    lo, hi = [], []
    for a in range(3):
        rel = float(focal_A[a]) / float(size_A[a])
        f = rel * float(size_B[a])
        region = int(float(proportion[a]) * float(size_B[a]))
        lo.append(max(int(f - region / 2), 0))
        hi.append(min(int(f + region / 2), int(size_B[a])))
    return lo, hi


def draw_focal_point(mask, weight, patch, u, box=None):
    """One focal point of a (D, H, W) case from the uniform u in [0, 1): ((z, y, x), fallback_used), or (None, flag) when
    the set is empty or its total weight is 0.

    The weight of a voxel of the valid zone is `mask != 0`, times `max(w, 0)` with a weight volume. Over the zone in C
    order: mask-only, the k-th non-zero voxel with k = min(int(floor(u * count)), count - 1); weighted, the first voxel
    whose float64 inclusive prefix sum exceeds u * total, else the last voxel of positive weight. This is the voxel
    `np.random.choice(len(idxs), p=map[map > 0] / map.sum())` picks from the same uniform. With `box` = (lo, hi) the draw
    is over zone ∩ body ∩ box, and over zone ∩ body (fallback_used = 1) when that is empty."""
    lo, hi = valid_zone(mask.shape, patch)
    if any(h <= l for l, h in zip(lo, hi)):
        return None, 0
    zone = tuple(slice(l, h) for l, h in zip(lo, hi))
    body = np.asarray(mask[zone]) != 0
    flag = 0
    if box is not None:
        cut = np.zeros_like(body)
        cut[tuple(slice(max(bl - l, 0), max(bh - l, 0)) for bl, bh, l in zip(box[0], box[1], lo))] = True
        cut &= body
        flag = 0 if cut.any() else 1
        body = cut if flag == 0 else body
    if weight is None:
        nz = np.flatnonzero(body.ravel())
        if nz.size == 0:
            return None, flag
        flat = int(nz[min(int(math.floor(u * float(nz.size))), nz.size - 1)])
    else:
        w = np.where(body, np.maximum(np.asarray(weight[zone]).astype(np.float64), 0.0), 0.0).ravel()
        w[np.isnan(w)] = 0.0
        prefix = np.cumsum(w)
        total = float(prefix[-1])
        if not total > 0.0:
            return None, flag
        flat = int(np.searchsorted(prefix, u * total, side="right"))
        if flat >= w.size:
            flat = int(np.flatnonzero(w > 0)[-1])
    point = np.unravel_index(flat, body.shape)
    return tuple(int(p) + l for p, l in zip(point, lo)), flag


class RawCase:
    """what a worker hands over with device_transforms on: which case, the uniform its focal point is drawn from, the
    augmentation matrix of its patch (9 floats, row-major) or None, and next to it the elastic field (float64
    [3, G0, G1, G2], already in voxels) or None, and last the intensity block of its domain — (rows, bias lattice): one
    (gamma, contrast, brightness, noise_std, bias, key0, key1) per modality and float64 [G0, G1, G2] or None — or None"""
    __slots__ = ("domain", "index", "u", "matrix", "field", "intensity")

    def __init__(self, domain, index, u, matrix=None, field=None, intensity=None):
        self.domain, self.index, self.u = domain, int(index), (None if u is None else float(u))
        self.matrix = None if matrix is None else matrix_tuple(matrix)
        self.field = field
        self.intensity = intensity


def _field(node, name, default=None):
    try:
        v = node[name]
    except (KeyError, AttributeError):
        return default
    return default if v is None else v


class MultiModalVolumeDataset(Dataset):

    def __init__(self, conf):
        d = conf[conf.mode].dataset
        self.root = Path(d.root)
        self.paired = bool(_field(d, "paired", True))
        self.patch_sampling = str(_field(d, "patch_sampling", "uniform-random-within-body"))
        schemes = PAIRED_SAMPLING_SCHEMES if self.paired else UNPAIRED_SAMPLING_SCHEMES
        if self.patch_sampling not in schemes:
            raise ValueError(f"`{self.patch_sampling}` not a valid {'paired' if self.paired else 'unpaired'} patch sampling "
                             f"scheme. Available schemes: {schemes}")
        self.modalities = {k: [str(n) for n in _field(d, "modalities", {})[k]] for k in ("A", "B")}
        masks = _field(d, "body_mask", {})
        self.body_mask = {"A": str(masks["A"]), "B": str(masks["A"] if self.paired else masks["B"])}
        names = self.modalities["A"] + self.modalities["B"]
        clip = _field(d, "clip_range", {})
        missing = [n for n in names if n not in clip]
        if missing:
            raise ValueError(f"clip_range has no entry for {missing}")
        self.clip_range = {n: (float(clip[n][0]), float(clip[n][1])) for n in names}
        if any(hi <= lo for lo, hi in self.clip_range.values()):
            raise ValueError(f"clip_range entries need min < max: {self.clip_range}")
        outside = _field(d, "outside_value", {})
        self.outside_value = {n: float(outside[n]) if n in outside else 0.0 for n in names}
        self.weight_modality = None
        if self.patch_sampling.startswith("fdg-pet-weighted"):
            self.weight_modality = _field(d, "weight_modality")
            if self.weight_modality not in self.modalities["A"]:
                raise ValueError(f"`{self.patch_sampling}` needs `weight_modality` to name one of A's modalities "
                                 f"{self.modalities['A']}; got {self.weight_modality!r}")
        self.patch_size = tuple(int(v) for v in d.patch_size)
        if len(self.patch_size) != 3 or min(self.patch_size) < 1:
            raise ValueError(f"patch_size must be three positive sizes (D, H, W); got {self.patch_size}")
        self.focal_region_proportion = tuple(float(v) for v in _field(d, "focal_region_proportion", (0.6, 0.3, 0.3)))
        self.cases = sorted(p.name for p in self.root.iterdir() if p.is_dir()) if self.root.is_dir() else []
        if not self.cases:
            raise ValueError(f"no case folders under {self.root}")
        path = _field(d, "divisors")
        self.divisors = json.loads(Path(path).read_text()) if path else {}
        self.raw = bool(_field(d, "device_transforms", False))
        self.augmentation = parse_augmentation(_field(d, "augmentation"), fill_allowed=False)
        check_elastic(self.augmentation, self.patch_size)
        check_intensity(self.augmentation and self.augmentation.intensity, self.patch_size, names)

    def __len__(self):
        return len(self.cases)

    # ---- files ------------------------------------------------------------------------------------------------------
    def load(self, name, index):
        """(D, H, W) array of one file, in the dtype it is stored in"""
        path = self.root / self.cases[index] / f"{name}.npy"
        v = np.load(path, mmap_mode="r")
        if v.ndim != 3:
            raise ValueError(f"{path}: expected a (D, H, W) array, got {v.shape}")
        return v

    def divisor(self, name, index):
        return float(self.divisors.get(name, {}).get(self.cases[index], 1.0))

    def empty_zone_error(self, domain, index):
        return ValueError(f"case {self.cases[index]!r} (domain {domain}): no voxel of the body mask with positive weight "
                          f"lies in the valid zone of patch size {self.patch_size}")

    # ---- host path --------------------------------------------------------------------------------------------------
    def normalize(self, name, index, patch, mask, intensity=None):
        """where(mask, v, outside) -> / divisor -> clamp -> min_max_normalize (basic.py:17-41, train_dataset.py:164-172).
        intensity: None or (row, beta, channel) — the chain of data/utils/patch_intensity.py on the min-max value, in front
        of its 2 n - 1"""
        lo, hi = self.clip_range[name]
        v = torch.from_numpy(np.array(patch)).float()
        m = torch.from_numpy(np.array(mask) != 0)
        v = torch.where(m, v, torch.tensor(self.outside_value[name], dtype=torch.float32))
        v = v / self.divisor(name, index)
        if intensity is None or is_neutral(intensity[0]):
            return min_max_normalize(torch.clamp(v, lo, hi), lo, hi)
        unit = (torch.clamp(v, lo, hi) - lo) / (hi - lo)                       # min_max_normalize's first half
        unit = torch.from_numpy(apply(unit.numpy(), *intensity))
        return 2 * unit - 1

    def crop(self, domain, index, mask, focal, matrix=None, field=None, intensity=None):
        start = [f - p // 2 for f, p in zip(focal, self.patch_size)]
        names = self.modalities[domain]
        intensity = active(intensity)
        chains = [None] * len(names)
        if intensity is not None:
            rows, lattice = intensity
            beta = None if lattice is None else bias_field(self.patch_size, lattice)
            chains = [(rows[c], beta, c) for c in range(len(names))]
        if matrix is not None:              # mask, then interpolate (sample_patch), then the same chain
            full = np.ones(self.patch_size, bool)
            return torch.stack([self.normalize(n, index, sample_patch(self.load(n, index), mask, start, self.patch_size,
                                                                      matrix, self.outside_value[n], field), full, chains[c])
                                for c, n in enumerate(names)])
        win = tuple(slice(s, s + p) for s, p in zip(start, self.patch_size))
        m = mask[win]
        return torch.stack([self.normalize(n, index, self.load(n, index)[win], m, chains[c]) for c, n in enumerate(names)])

    def sample_points(self, index_A, index_B):
        """((focal_A, focal_B), fallback_used) with the reference's consumption of np.random: one uniform per draw"""
        mask_A = self.load(self.body_mask["A"], index_A)
        weight = self.load(self.weight_modality, index_A) if self.weight_modality else None
        focal_A, _ = draw_focal_point(mask_A, weight, self.patch_size, np.random.random_sample())
        if focal_A is None:
            raise self.empty_zone_error("A", index_A)
        if self.paired:
            return (focal_A, focal_A), 0
        mask_B = self.load(self.body_mask["B"], index_B)
        box = focal_box(focal_A, mask_A.shape, mask_B.shape, self.focal_region_proportion)
        focal_B, flag = draw_focal_point(mask_B, None, self.patch_size, np.random.random_sample(), box)
        if focal_B is None:
            raise self.empty_zone_error("B", index_B)
        return (focal_A, focal_B), flag

    def draw_matrices(self):
        """((M_A, field_A, intensity_A), (M_B, field_B, intensity_B)) after the sample's other draws: none without
        `augmentation`, one geometric set (eight uniforms, and the field's with `elastic`) shared by A and B when paired,
        A's set then B's set when unpaired. With `intensity` every domain's block (patch_intensity.draw_block) follows its
        geometric set: shared set, A's block, B's block when paired — intensity is never shared — and A's set, A's block,
        B's set, B's block when unpaired."""
        aug = self.augmentation
        if aug is None:
            return (None, None, None), (None, None, None)
        block = lambda k: None if aug.intensity is None else draw_block(aug.intensity, self.modalities[k])
        set_A = draw_set(aug)
        int_A = block("A")
        set_B = set_A if self.paired else draw_set(aug)
        return (*set_A, int_A), (*set_B, block("B"))

    def __getitem__(self, index):
        index_A = index % len(self.cases)
        index_B = index_A if self.paired else random.randint(0, len(self.cases) - 1)
        if self.raw:
            u_A = np.random.random_sample()
            u_B = None if self.paired else np.random.random_sample()
            set_A, set_B = self.draw_matrices()
            return {"A": RawCase("A", index_A, u_A, *set_A), "B": RawCase("B", index_B, u_B, *set_B)}
        (focal_A, focal_B), _ = self.sample_points(index_A, index_B)
        set_A, set_B = self.draw_matrices()
        mask_A = self.load(self.body_mask["A"], index_A)
        mask_B = mask_A if self.paired else self.load(self.body_mask["B"], index_B)
        return {"A": self.crop("A", index_A, mask_A, focal_A, *set_A), "B": self.crop("B", index_B, mask_B, focal_B, *set_B)}

    # ---- picked up by build_loader / Trainer ----------------------------------------------------------------------
    @property
    def collate_fn(self):
        return collate_raw if self.raw else None

    def device_pipeline(self, conf, device):
        if not self.raw:
            return None
        from .device_volumes import DeviceMultiModalPipeline
        return DeviceMultiModalPipeline(self, device)
