"""What the device pipelines that keep their inputs in HBM share (data/device_volumes.py, data/device_images.py): the
device, the lazily resolved kernel backend, and the residency rule — a tensor is uploaded (or generated) on first use and
kept while `resident_bytes + nbytes <= max_resident_bytes`; beyond the budget it is made again per use."""
import torch


class ResidentCache:

    def __init__(self, device, ops=None, max_resident_bytes=200 << 30):
        self.device = torch.device(device)
        self._ops = ops
        self.resident = {}
        self.resident_bytes, self.max_resident_bytes = 0, max_resident_bytes

    @property
    def ops(self):
        if self._ops is None:
            from ..nn.native.backend import get_ops
            self._ops = get_ops()
        return self._ops

    def _keep(self, key, v):
        nbytes = v.numel() * v.element_size()
        if self.resident_bytes + nbytes <= self.max_resident_bytes:          # beyond the budget: upload / generate per use
            self.resident[key] = v
            self.resident_bytes += nbytes
        return v

    def _get(self, key, make):
        """the resident tensor of `key`, or make() -> device tensor, kept under the budget rule"""
        v = self.resident.get(key)
        return self._keep(key, make()) if v is None else v
