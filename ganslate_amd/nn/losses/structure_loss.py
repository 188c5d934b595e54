"""Structure-consistency loss (Yang et al. 2018) between an image and its translation — interface of StructureLoss /
MINDDescriptor in the reference's projects/cleargrasp_depth_estimation/modules/old/cyclegan_losses_with_structure.py:41-182
and of its tutorial docs/tutorials_basic/2_new_project.md, on the fused kernels of csrc/mind.hip.

The descriptor is fixed to MIND_DESCRIPTOR_CONFIG (non-local region 9x9, patch 7x7, neighbourhood 3x3, sigma 2). Images
with several channels are reduced to one plane by the mean over their channels; the project-specific channel slicing of the
reference's v1 / v2 variants is left to the caller (slice before calling).

Volumes take MINDDescriptor3D / StructureLoss3D on the kernels of csrc/mind3d.hip: MIND3D_DESCRIPTOR_CONFIG (non-local region
3x3x3, patch 5x5x5, neighbourhood 3x3x3, sigma 2), a definition of this project's own (include/ganslate_hip.h) — the
reference has none. The 2-D classes refuse volumes and the 3-D classes refuse images."""
import torch

from ..native.backend import get_ops
from .functional import mind3d_structure_autograd, mind_structure_autograd, scalar_affine

MIND_DESCRIPTOR_CONFIG = {"non_local_region_size": 9, "patch_size": 7, "neighbor_size": 3, "gaussian_patch_sigma": 2.0}
MIND3D_DESCRIPTOR_CONFIG = {"non_local_region_size": 3, "patch_size": 5, "neighbor_size": 3, "gaussian_patch_sigma": 2.0}


def _need(ops, method):
    if not hasattr(ops, method):
        raise NotImplementedError(f"the '{getattr(ops, 'name', type(ops).__name__)}' backend has no MIND kernels "
                                  f"(missing ops.{method})")


class _Descriptor:
    """One rank's descriptor: the subclass names its config, its tensor rank, its refusal and its backend method."""
    _CONFIG = _DIM = _TAKES = _METHOD = None

    def __init__(self, **config):
        unknown = set(config) - set(self._CONFIG)
        if unknown:
            raise TypeError(f"unknown MIND descriptor setting(s): {sorted(unknown)}")
        self.config = dict(self._CONFIG, **config)

    def __call__(self, sample):
        if sample.dim() != self._DIM:
            raise ValueError(f"{self._TAKES}; got {tuple(sample.shape)}")
        ops = get_ops()
        _need(ops, self._METHOD)
        with torch.no_grad():
            return getattr(ops, self._METHOD)(sample.detach().contiguous().float(), cfg=self.config)


class _Structure:
    """One rank's loss: the subclass names its backend methods and its autograd function."""
    _PREFIX = None
    _autograd = None

    def __init__(self, lambda_structure):
        self.lambda_structure = lambda_structure

    def terms(self, input_, fake):
        """[(weight, 0-d loss)] whose weighted sum is the loss"""
        _need(get_ops(), f"{self._PREFIX}_l1")
        _need(get_ops(), f"{self._PREFIX}_l1_backward")
        return [(self.lambda_structure, self._autograd(input_, fake))]

    def __call__(self, input_, fake):
        (w, x), = self.terms(input_, fake)
        return scalar_affine([x], [[w]])[0]


class MINDDescriptor(_Descriptor):
    """image [N, C, H, W] -> features [N, 81, H, W]; channel i is the shift with row offset i % 9 - 4 and column offset
    i // 9 - 4. No gradient flows through it: the differentiable path is StructureLoss."""
    _CONFIG, _DIM, _METHOD = MIND_DESCRIPTOR_CONFIG, 4, "mind_descriptor"
    _TAKES = "the MIND descriptor takes [N, C, H, W] images (volumes are not supported)"


class StructureLoss(_Structure):
    """lambda_structure * sum_{n,a,p} |f_a(input) - f_a(fake)| / (H W 81). As in the reference this is a SUM over the
    batch, not a mean: the loss grows with the batch size."""
    _PREFIX, _autograd = "mind", staticmethod(mind_structure_autograd)


class MINDDescriptor3D(_Descriptor):
    """volume [N, C, D, H, W] -> features [N, 27, D, H, W]; channel i is the shift with depth offset i % 3 - 1, row offset
    (i // 3) % 3 - 1 and column offset i // 9 - 1. No gradient flows through it: the differentiable path is
    StructureLoss3D."""
    _CONFIG, _DIM, _METHOD = MIND3D_DESCRIPTOR_CONFIG, 5, "mind3d_descriptor"
    _TAKES = "the volumetric MIND descriptor takes [N, C, D, H, W] volumes"


class StructureLoss3D(_Structure):
    """lambda_structure * sum_{n,a,p} |f_a(input) - f_a(fake)| / (D H W 27): StructureLoss for volumes, a SUM over the batch
    as well."""
    _PREFIX, _autograd = "mind3d", staticmethod(mind3d_structure_autograd)

    def terms(self, input_, fake):
        for t in (input_, fake):           # refused before the backend is asked for its kernels
            if t.dim() != 5:
                raise ValueError(f"the volumetric structure loss takes [N, C, D, H, W] volumes; got {tuple(t.shape)}")
        return super().terms(input_, fake)
