"""Whole multi-modal cases with their region masks for the Validator, the Tester and the Inferer: the evaluation side of
the reference's HX4-PET project (projects/maastro_hx4_pet_translation/datasets/val_test_dataset.py with
datasets/utils/basic.py), next to the training set of data/multimodal_volumes.py.

Layout: `<root>/<case>/<name>.npy`, dense (D, H, W) arrays; images fp32 or int16, masks uint8 or bool; cases sorted by name;
the set is paired (A and B of a sample are the same case). The reference reads NRRD through SimpleITK and hard-codes its
modalities, mask names, the (64, 512, 512) padding and the one patient without a body mask; here those are config fields.

Per case, in the reference's order (val_test_dataset.py:136-161):
  1. the body mask: its file, or — `generate_body_mask` — made from the CT `body_mask_from` by
     data/utils/body_mask.get_body_mask (threshold `body_mask_threshold`, largest component, per-slice fill);
  2. x = where(body, v, outside_value) per modality;
  3. with `pad_to`, centred padding up to that shape by data/utils/ops.pad: images with min(x), every mask with its own
     minimum; `pad_to: null` leaves the case as it is (the reference's `use_patch_based_inference`);
  4. x / divisor, clamp to the clip range, min-max to [-1, 1] (MultiModalVolumeDataset.normalize's torch chain).
A sample is {"A": [C_A, D, H, W], "B": [before + C_B + after, D, H, W] with `dummy_channels_B` zero channels around B (the
reference's `model_is_hx4_cyclegan_balanced` stacks [HX4, 0]), "masks": {label: uint8 [1, D, H, W]} with `supply_masks`,
"metadata": {"case", "size", "pad_before"}}; under `infer` it is {"A", "metadata"}.

`save` differs from the reference in one point: it crops the padding off again, so `<save_dir>/<case>.npy` has the shape
of the case's files (the reference writes the padded volume under the unpadded volume's geometry).

With `device_transforms: true` a sample is the case index; volumes and masks stay resident in HBM and
DeviceWholeVolumePipeline (data/device_volumes.py) generates missing body masks with gs_body_mask and prepares every case
with one gs_volume_prepare call."""
import json
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import configs
from .device_transforms import collate_raw
from .multimodal_volumes import _field
from .utils.body_mask import get_body_mask
from .utils.normalization import min_max_denormalize, min_max_normalize
from .utils.ops import pad, pad_widths

GENERATE_MODES = ("never", "missing", "always")


@dataclass
class MultiModalVolumeValTestDatasetConfig(configs.base.BaseDatasetConfig):
    modalities: Dict[str, Any] = field(default_factory=dict)        # {A: [fdg_pet, pct], B: [hx4_pet]}
    body_mask: str = "body"                                         # one stem: the set is paired
    clip_range: Dict[str, Any] = field(default_factory=dict)        # {name: [min, max]}
    outside_value: Dict[str, Any] = field(default_factory=dict)     # {name: value outside the body}
    divisors: Optional[str] = None                                  # JSON file {name: {case: value}}; default divisor 1
    masks: Dict[str, Any] = field(default_factory=dict)             # {label: stem}, e.g. {BODY: pct_body, GTV: pct_gtv}
    supply_masks: bool = False
    pad_to: Optional[Tuple[int, int, int]] = None                   # DHW; the reference pads to (64, 512, 512)
    generate_body_mask: str = "missing"                             # never | missing | always
    body_mask_from: Optional[str] = None                            # the A modality (a CT) the mask is generated from
    body_mask_threshold: float = -300.0                             # the reference's HU_THRESHOLD
    dummy_channels_B: Tuple[int, int] = (0, 0)                      # zero channels [before, after] B's
    denormalize_modality: Optional[str] = None                      # B modality whose clip range `denormalize` uses
    device_transforms: bool = False


class RawWholeCase:
    """what a worker hands over with device_transforms on: which case"""
    __slots__ = ("index",)

    def __init__(self, index):
        self.index = int(index)


class MultiModalVolumeValTestDataset(Dataset):

    def __init__(self, conf):
        self.mode = str(conf.mode)
        d = conf[conf.mode].dataset
        self.root = Path(d.root)
        self.modalities = {k: [str(n) for n in _field(d, "modalities", {})[k]] for k in ("A", "B")}
        self.body_mask = str(_field(d, "body_mask", "body"))
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
        self.supply_masks = bool(_field(d, "supply_masks", False))
        self.masks = {str(k): str(v) for k, v in _field(d, "masks", {}).items()}
        pad_to = _field(d, "pad_to")
        self.pad_to = None if pad_to is None else tuple(int(v) for v in pad_to)
        if self.pad_to is not None and (len(self.pad_to) != 3 or min(self.pad_to) < 1):
            raise ValueError(f"pad_to must be three positive sizes (D, H, W) or null; got {self.pad_to}")
        self.generate_body_mask = str(_field(d, "generate_body_mask", "missing"))
        if self.generate_body_mask not in GENERATE_MODES:
            raise ValueError(f"generate_body_mask must be one of {GENERATE_MODES}; got {self.generate_body_mask!r}")
        self.body_mask_from = _field(d, "body_mask_from")
        if self.generate_body_mask != "never" and self.body_mask_from not in self.modalities["A"]:
            raise ValueError(f"generate_body_mask: {self.generate_body_mask} needs `body_mask_from` to name one of A's "
                             f"modalities {self.modalities['A']}; got {self.body_mask_from!r}")
        self.body_mask_threshold = float(_field(d, "body_mask_threshold", -300.0))
        self.dummy_channels_B = tuple(int(v) for v in _field(d, "dummy_channels_B", (0, 0)))
        if len(self.dummy_channels_B) != 2 or min(self.dummy_channels_B) < 0:
            raise ValueError(f"dummy_channels_B must be two counts [before, after]; got {self.dummy_channels_B}")
        self.denormalize_modality = str(_field(d, "denormalize_modality", self.modalities["B"][0]))
        if self.denormalize_modality not in self.modalities["B"]:
            raise ValueError(f"denormalize_modality must name one of B's modalities {self.modalities['B']}; got "
                             f"{self.denormalize_modality!r}")
        self.cases = sorted(p.name for p in self.root.iterdir() if p.is_dir()) if self.root.is_dir() else []
        if not self.cases:
            raise ValueError(f"no case folders under {self.root}")
        path = _field(d, "divisors")
        self.divisors = json.loads(Path(path).read_text()) if path else {}
        self.raw = bool(_field(d, "device_transforms", False))
        self._generated = {}

    def __len__(self):
        return len(self.cases)

    # ---- files ------------------------------------------------------------------------------------------------------
    def path(self, name, index):
        return self.root / self.cases[index] / f"{name}.npy"

    def load(self, name, index):
        """(D, H, W) array of one file, in the dtype it is stored in"""
        path = self.path(name, index)
        v = np.load(path, mmap_mode="r")
        if v.ndim != 3:
            raise ValueError(f"{path}: expected a (D, H, W) array, got {v.shape}")
        return v

    def divisor(self, name, index):
        return float(self.divisors.get(name, {}).get(self.cases[index], 1.0))

    def generates(self, index):
        """whether this case's body mask is generated: by the mode, and whether its file is there"""
        if self.generate_body_mask == "always":
            return True
        if self.path(self.body_mask, index).is_file():
            return False
        if self.generate_body_mask == "never":
            raise FileNotFoundError(f"case {self.cases[index]!r} has no body mask `{self.body_mask}.npy` and "
                                    "generate_body_mask is `never`")
        return True

    def empty_body_error(self, index):
        return ValueError(f"case {self.cases[index]!r}: no voxel of `{self.body_mask_from}` reaches the threshold "
                          f"{self.body_mask_threshold}; no body mask can be generated")

    def mask_labels(self):
        return list(self.masks) if self.supply_masks and self.mode != "infer" else []

    def domains(self):
        return ("A",) if self.mode == "infer" else ("A", "B")

    def metadata(self, index):
        size = tuple(int(v) for v in self.load(self.modalities["A"][0], index).shape)
        widths = pad_widths(size, self.pad_to) if self.pad_to else [(0, 0)] * 3
        return {"case": self.cases[index], "size": list(size), "pad_before": [w[0] for w in widths]}

    # ---- host path --------------------------------------------------------------------------------------------------
    def host_body_mask(self, index):
        """uint8 0 / 1 (D, H, W): the file, or the mask generated from the CT (kept per case)"""
        if not self.generates(index):
            return (np.asarray(self.load(self.body_mask, index)) != 0).astype(np.uint8)
        if index not in self._generated:
            try:
                self._generated[index] = get_body_mask(np.asarray(self.load(self.body_mask_from, index)),
                                                       self.body_mask_threshold)
            except ValueError:
                raise self.empty_body_error(index) from None
        return self._generated[index]

    def normalize(self, name, index, volume, mask):
        lo, hi = self.clip_range[name]
        v = torch.from_numpy(np.array(volume)).float()
        v = torch.where(torch.from_numpy(mask != 0), v, torch.tensor(self.outside_value[name], dtype=torch.float32))
        if self.pad_to:
            v = torch.from_numpy(pad(v.numpy(), self.pad_to))
        v = v / self.divisor(name, index)
        return min_max_normalize(torch.clamp(v, lo, hi), lo, hi)

    def host_mask(self, stem, index, body):
        m = body if stem == self.body_mask else (np.asarray(self.load(stem, index)) != 0).astype(np.uint8)
        return torch.from_numpy(pad(m, self.pad_to) if self.pad_to else np.array(m))

    def add_dummies(self, B):
        before, after = self.dummy_channels_B
        zeros = lambda n: B.new_zeros((n, *B.shape[1:]))
        return torch.cat([zeros(before), B, zeros(after)]) if before or after else B

    def __getitem__(self, index):
        index = index % len(self.cases)
        meta = self.metadata(index)
        if self.raw:
            sample = {k: RawWholeCase(index) for k in self.domains()}
            sample["metadata"] = meta
            return sample
        body = self.host_body_mask(index)
        sample = {}
        for k in self.domains():
            sample[k] = torch.stack([self.normalize(n, index, self.load(n, index), body) for n in self.modalities[k]])
        if "B" in sample:
            sample["B"] = self.add_dummies(sample["B"])
        labels = self.mask_labels()
        if labels:
            sample["masks"] = {label: self.host_mask(self.masks[label], index, body).unsqueeze(0) for label in labels}
        sample["metadata"] = meta
        return sample

    # ---- picked up by the engines -------------------------------------------------------------------------------------
    def denormalize(self, tensor):
        """[-1, 1] back to the clip range of `denormalize_modality`, IN PLACE like the reference's"""
        return min_max_denormalize(tensor, *self.clip_range[self.denormalize_modality])

    def save(self, tensor, save_dir, metadata):
        """the real B channel of one generated sample, without the padding, in the units of the case's file
        (denormalised, times the case's divisor), as `<save_dir>/<case>.npy` (fp32)"""
        names = self.modalities["B"]
        j = names.index(self.denormalize_modality)
        if tensor.shape[0] == len(names) + sum(self.dummy_channels_B):
            j += self.dummy_channels_B[0]
        elif tensor.shape[0] != len(names):
            j = 0                                             # a generator that emits the translated channel only
        case = str(metadata["case"])
        start = [int(v) for v in metadata["pad_before"]]
        size = [int(v) for v in metadata["size"]]
        crop = tensor[j][tuple(slice(s, s + n) for s, n in zip(start, size))]
        out = self.denormalize(crop.detach().float().cpu().clone()) * self.divisor(self.denormalize_modality,
                                                                                   self.cases.index(case))
        path = Path(save_dir) / f"{case}.npy"
        path.parent.mkdir(parents=True, exist_ok=True)
        np.save(path, out.numpy().astype(np.float32))
        return path

    @property
    def collate_fn(self):
        return collate_raw if self.raw else None

    def device_pipeline(self, conf, device):
        if not self.raw:
            return None
        from .device_volumes import DeviceWholeVolumePipeline
        return DeviceWholeVolumePipeline(self, device)
