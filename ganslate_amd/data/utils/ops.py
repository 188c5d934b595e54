"""Array helpers of the datasets, host side (ganslate/data/utils/ops.py)."""
import numpy as np


def pad_widths(shape, target_shape):
    """per axis (front, back): an axis below its target gets `total // 2` in front and `total // 2 + total % 2` behind,
    an axis at or above its target nothing"""
    if len(target_shape) != len(shape):
        raise ValueError(f"target shape {tuple(target_shape)} and array shape {tuple(shape)} differ in rank")
    widths = []
    for size, target in zip(shape, target_shape):
        total = max(int(target) - int(size), 0)
        widths.append((total // 2, total // 2 + total % 2))
    return widths


def pad(volume, target_shape):
    """`volume` padded centred up to `target_shape` with its own minimum (ops.py:4-15)"""
    volume = np.asarray(volume)
    return np.pad(volume, pad_widths(volume.shape, target_shape), "constant", constant_values=volume.min())
