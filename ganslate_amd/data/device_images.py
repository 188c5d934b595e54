"""Device-side input pipeline of the multi-modal 2-D image datasets (data/multimodal_images.py): decoded images resident in
HBM as stored (uint8 / fp32), per iteration only sample indices and noise keys arrive from the loader, and each domain's
fp32 [N, C, H, W] batch is built by one gs_img_stack launch (csrc/imgstack.hip): bicubic tensor resize, clamp, min-max,
noise plane and channel concat of every (sample, modality), the dummy channels of a val / test sample included. Reference
path being replaced: projects/cleargrasp_depth_estimation/datasets/train_dataset.py:75-146, val_test_dataset.py:80-167."""
from typing import Any, NamedTuple

import numpy as np
import torch

from .multimodal_images import RawImageSample, TapTable, bicubic_taps
from .resident_cache import ResidentCache


class StackItem(NamedTuple):
    """host side of one GsImgStackItem (include/ganslate_hip.h): one modality of one sample, or `c` zero channels"""
    src: Any
    taps_y: Any
    taps_x: Any
    c: int
    item: int
    c0: int
    lo: float = 0.0
    hi: float = 1.0
    rescale: bool = True
    noise_std: float = 0.0
    key: Any = (0, 0)
    hwc: bool = True                 # False: src is (c, in_h, in_w), planes apart; the datasets store (H, W[, C])


class DeviceMultiModalImagePipeline(ResidentCache):
    """callable(raw batch) -> {"A": fp32 [N, C_A, H, W] on the device, "B": fp32 [N, front + C_B + back, H, W],
    "metadata": as it came} for MultiModalImageDataset and MultiModalImageValTestDataset. Images are uploaded on first use
    and stay resident under `max_resident_bytes` (beyond it: uploaded per use); the tap tables of every (stored size,
    load size) pair met are built once on the host in float64 (bicubic_taps) and stay on the device. One launch per domain
    tensor per batch; nothing synchronises."""

    def __init__(self, dataset, device, ops=None, max_resident_bytes=200 << 30):
        super().__init__(device, ops, max_resident_bytes)
        self.dataset = dataset
        self.size = tuple(int(v) for v in dataset.size)               # (H, W)
        self.tables = {}
        self.uploads = 0

    def image(self, name, index):
        def upload():
            self.uploads += 1
            return torch.from_numpy(np.array(self.dataset.load(name, index))).to(self.device)

        return self._get((name, index), upload)

    def taps(self, n_in, n_out):
        key = (int(n_in), int(n_out))
        t = self.tables.get(key)
        if t is None:
            host = bicubic_taps(*key)
            t = TapTable(torch.from_numpy(host.idx).to(self.device), torch.from_numpy(host.w).to(self.device), *key)
            self.tables[key] = t
        return t

    def items(self, domain, samples):
        """the descriptors of one domain's batch tensor, and its channel count"""
        ds = self.dataset
        front, back = ds.dummy_channels(domain)
        total = front + ds.domain_channels(domain) + back
        H, W = self.size
        out = []
        for i, s in enumerate(samples):
            if front:
                out.append(StackItem(None, None, None, front, i, 0))
            c0 = front
            for name in ds.modalities[domain]:
                src = self.image(name, s.index)
                lo, hi = ds.clip_range[name]
                std = ds.noise_std[domain].get(name, 0.0)
                out.append(StackItem(src, self.taps(src.shape[0], H), self.taps(src.shape[1], W), ds.channels[name], i, c0,
                                     lo, hi, ds.rescale[name], std, s.keys[name] if std else (0, 0)))
                c0 += ds.channels[name]
            if back:
                out.append(StackItem(None, None, None, back, i, c0))
        return out, total

    def __call__(self, batch):
        first = batch.get("A")
        if not first or not isinstance(first[0], RawImageSample):
            return batch
        out = {k: v for k, v in batch.items() if k not in ("A", "B")}
        for domain in ("A", "B"):
            samples = batch.get(domain)
            if not samples:
                continue
            items, channels = self.items(domain, samples)
            dst = torch.empty((len(samples), channels, *self.size), dtype=torch.float32, device=self.device)
            self.ops.img_stack(items, dst)
            out[domain] = dst
        return out
