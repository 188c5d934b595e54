"""Patient body mask from a CT (ganslate/data/utils/body_mask.py): threshold, largest connected component, per-slice
hole filling. The definition below is shared by this host utility, the device kernels (csrc/bodymask.hip, gs_body_mask)
and the test reference (tests/bodymask_ref.py).

For a dense (D, H, W) volume `v` (fp32 or int16; anything else is converted to fp32) and a threshold `t` (rounded to fp32;
the comparison runs in fp32, in which every int16 is exact):

1. `b = v >= t`. A NaN voxel is outside.
2. Components of `b` use 6-connectivity (`scipy.ndimage.label`'s default structure, as the reference uses it).
3. The component with the most voxels is taken; ties go to the component whose first voxel in C order comes first (the
   reference's `np.argmax` over labels in scan order).
4. Per depth slice the holes of that component's slice are filled: the result is every pixel that is NOT a non-component
   pixel 4-connected to the slice's border through non-component pixels (`scipy.ndimage.binary_fill_holes` per slice). A
   cavity that opens to the border in one slice stays open in that slice; a hole that touches the outside only diagonally
   is filled.
5. If no voxel reaches the threshold the reference fails in `np.argmax([])`; `get_body_mask` raises ValueError, the kernel
   writes an all-zero mask and reports a count of 0.

Deliberate deviation: the reference then keeps only the largest OpenCV contour of each slice and redraws it smoothed
(body_mask.py:82-102). OpenCV is not a dependency here and its polygon rasterisation cannot be restated exactly, so steps
1-4 ARE the definition: a slice may keep several pieces (arms next to the trunk), and outlines are not smoothed.

numpy only. Components are found by the scheme the kernels use — every voxel holds a parent index inside its component,
roots of adjacent voxels are hooked to the smaller one, parents are replaced by roots, until nothing changes — so a label is
the smallest flat index of its component and the number of passes does not grow with the length of a thin path."""
import numpy as np


def _min_index_labels(fg, axes):
    """flat array: the smallest flat index of every voxel's component of `fg` under adjacency along `axes`; -1 outside"""
    n = fg.size
    dtype = np.int32 if n < 2 ** 31 else np.int64
    idx = np.arange(n, dtype=dtype).reshape(fg.shape)
    parent = np.where(fg, idx, dtype(-1)).ravel()
    first, second = [], []
    for axis in axes:
        lo = tuple(slice(None, -1) if a == axis else slice(None) for a in range(fg.ndim))
        hi = tuple(slice(1, None) if a == axis else slice(None) for a in range(fg.ndim))
        both = fg[lo] & fg[hi]
        first.append(idx[lo][both])
        second.append(idx[hi][both])
    first, second = np.concatenate(first), np.concatenate(second)
    members = np.flatnonzero(fg.ravel())
    while True:
        a, b = parent[first], parent[second]
        differ = a != b
        if not differ.any():
            return parent
        a, b = a[differ], b[differ]
        np.minimum.at(parent, np.maximum(a, b), np.minimum(a, b))          # hook the larger root to the smaller one
        while True:                                                        # parents -> roots
            up = parent[parent[members]]
            if np.array_equal(up, parent[members]):
                break
            parent[members] = up


def get_body_mask(image, hu_threshold):
    """uint8 (D, H, W) body mask of `image` by the definition in this module's docstring"""
    image = np.asarray(image)
    if image.ndim != 3:
        raise ValueError(f"expected a (D, H, W) array, got {image.shape}")
    with np.errstate(invalid="ignore"):
        b = image.astype(np.float32) >= np.float32(hu_threshold)
    labels = _min_index_labels(b, (0, 1, 2))
    roots, counts = np.unique(labels[labels >= 0], return_counts=True)     # ascending roots: argmax takes the first of a tie
    if roots.size == 0:
        raise ValueError(f"no voxel reaches the threshold {hu_threshold}: there is no body to mask")
    component = (labels == roots[np.argmax(counts)]).reshape(image.shape)
    rest = ~component
    labels = _min_index_labels(rest, (1, 2))
    border = np.zeros(image.shape, bool)
    border[:, [0, -1], :] = True
    border[:, :, [0, -1]] = True
    outside_root = np.zeros(image.size + 1, bool)                          # slot -1 takes the component's voxels
    outside_root[labels[(border & rest).ravel()]] = True
    outside_root[-1] = False
    return (~outside_root[labels]).reshape(image.shape).astype(np.uint8)


def apply_body_mask(array, apply_mask=True, masking_value=-1024, hu_threshold=-300):
    """`array` with `masking_value` outside the body mask generated from it (body_mask.py:107-132)"""
    if apply_mask:
        body_mask = get_body_mask(array, hu_threshold)
        array = np.where(body_mask, array, masking_value)
    return array
