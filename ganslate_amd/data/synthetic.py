"""Synthetic unpaired/paired image dataset: U(-1,1) tensors of the configured shape (the value range
`Normalize(0.5, 0.5)` gives real images, data/utils/transforms.py:54-57). Used by bench.py and the tests —
no dataset can be downloaded on the target machines.

`SyntheticMaskedImageDataset` yields the same samples plus `masks = {label: bool tensor of the sample's shape}`, the
form in which the medical val / test datasets hand region masks (BODY, GTV, ...) to the validator
(validator_tester.py:78-98): seeded boxes and balls, never empty.

`SyntheticSavingImageDataset` yields the same samples plus a `metadata` entry and has a `save()`: the path by which the
val / test / infer engines hand every generated tensor back to the dataset (engines/base.py save_generated_tensor)."""
from dataclasses import dataclass, field
from pathlib import Path
from typing import Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import configs


@dataclass
class SyntheticImageDatasetConfig(configs.base.BaseDatasetConfig):
    root: str = ""
    num_workers: int = 0
    image_channels: int = 3
    final_size: Tuple[int, ...] = field(default_factory=lambda: [256, 256])
    length: int = 1024
    seed: int = 1234


@dataclass
class SyntheticMaskedImageDatasetConfig(SyntheticImageDatasetConfig):
    mask_labels: Tuple[str, ...] = field(default_factory=lambda: ["BODY", "GTV"])


@dataclass
class SyntheticSavingImageDatasetConfig(SyntheticImageDatasetConfig):
    pass


class SyntheticImageDataset(Dataset):

    def __init__(self, conf):
        d = conf[conf.mode].dataset
        self.shape = (d.image_channels, *(int(v) for v in d.final_size))   # (H, W) images or (D, H, W) volumes
        self.length, self.seed = d.length, d.seed

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self.seed + int(index))
        return {"A": torch.rand(self.shape, generator=g) * 2 - 1, "B": torch.rand(self.shape, generator=g) * 2 - 1}

    def __len__(self):
        return self.length


class SyntheticMaskedImageDataset(SyntheticImageDataset):
    """The samples of SyntheticImageDataset for the same seed, plus one region mask per label of `mask_labels`: labels
    at even positions get an axis-aligned box, those at odd positions a ball, each covering every channel, drawn from
    a generator of its own (seeded by seed, index and label position) so that A and B do not move."""

    def __init__(self, conf):
        super().__init__(conf)
        self.labels = [str(k) for k in conf[conf.mode].dataset.mask_labels]

    def _mask(self, index, position):
        g = torch.Generator().manual_seed((self.seed + int(index)) * 1000003 + 7919 * (position + 1))
        spatial = self.shape[1:]
        # a centre anywhere in the grid and a half-extent of 1/8 .. 3/8 of each axis: at least the centre is inside
        centre = [int(torch.randint(0, s, (1,), generator=g)) for s in spatial]
        frac = [float(torch.rand(1, generator=g)) * 0.25 + 0.125 for _ in spatial]
        grids = torch.meshgrid(*[torch.arange(s) for s in spatial], indexing="ij")
        if position % 2 == 0:
            inside = torch.ones(spatial, dtype=torch.bool)
            for x, c, f, s in zip(grids, centre, frac, spatial):
                inside &= (x - c).abs() <= max(1, int(f * s))
        else:
            r2 = torch.zeros(spatial)
            for x, c, f, s in zip(grids, centre, frac, spatial):
                r2 += ((x - c).float() / max(1.0, f * s)) ** 2
            inside = r2 <= 1.0
        return inside.unsqueeze(0).expand(self.shape).clone()

    def __getitem__(self, index):
        sample = super().__getitem__(index)
        sample["masks"] = {k: self._mask(index, i) for i, k in enumerate(self.labels)}
        return sample


class SyntheticSavingImageDataset(SyntheticImageDataset):
    """The samples of SyntheticImageDataset for the same seed, each with `metadata = {"id": "sample_<index>", "index":
    index}`; `save(tensor, save_dir, metadata)` writes the generated tensor as `<save_dir>/<metadata id>.npy` (fp32)."""

    def __getitem__(self, index):
        sample = super().__getitem__(index)
        sample["metadata"] = {"id": f"sample_{int(index):04d}", "index": int(index)}
        return sample

    def save(self, tensor, save_dir, metadata):
        path = Path(save_dir) / f"{metadata['id']}.npy"
        path.parent.mkdir(parents=True, exist_ok=True)
        np.save(path, tensor.detach().float().cpu().numpy())
        return path
