"""CPU reference of the multi-modal patch-sampling ops (csrc/volsample.hip), restated from the rule in
include/ganslate_hip.h in plain numpy for tests/test_mmvol_cpu.py and tests/test_mmvol_gpu.py. Nothing here calls the
package's sampling code or the kernels: the draw is written the slow, obvious way (a full-volume weight map, a python
prefix rule), the patch chain as five float32 numpy operations. `RefMMOps` carries the same method signatures as HipOps, so
DeviceMultiModalPipeline(ops=RefMMOps()) runs the device pipeline's control flow on CPU tensors."""
import math

import numpy as np
import torch

NR = 256          # workgroup ranges of gs_voxel_draw's first pass


def synthetic_case(shape, seed, body="ellipsoid"):
    """seeded volumes of one case (numpy Generator streams are version-stable); tools/gen_golden_mmvol.py builds the same.
    pet: fp32 multiples of 1/8, some negative; ct: int16; hx4: fp32 multiples of 1/8; index: every voxel's own flat index
    (exact in fp32 below 2^24), so a patch of it reveals where it starts. body: an ellipsoid with holes, or a box in the
    low / high corner of the volume (for draws whose focal box misses the body)."""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    if body == "ellipsoid":
        g = np.meshgrid(*[(np.arange(s) - (s - 1) / 2) / (0.46 * s) for s in shape], indexing="ij")
        mask = (g[0] ** 2 + g[1] ** 2 + g[2] ** 2 <= 1.0) & (rng.random(shape) > 0.08)
    else:
        mask = np.zeros(shape, bool)
        cut = [slice(0, max(2, int(0.45 * s))) if body == "low" else slice(s - max(2, int(0.45 * s)), s) for s in shape]
        mask[tuple(cut)] = True
        mask &= rng.random(shape) > 0.08
    return {"body": mask.astype(np.uint8),
            "pet": (rng.integers(-8, 64, size=shape) / 8.0).astype(np.float32),
            "ct": rng.integers(-1100, 2200, size=shape).astype(np.int16),
            "hx4": (rng.integers(0, 40, size=shape) / 8.0).astype(np.float32),
            "index": np.arange(D * H * W, dtype=np.float32).reshape(shape)}


def zone_of(size, patch):
    return [p // 2 for p in patch], [s - (p + 1) // 2 for s, p in zip(size, patch)]


def focal_box(focal_A, dims_A, dims_B, proportion):
    lo, hi = [], []
    for a in range(3):
        rel = np.float64(focal_A[a]) / np.float64(dims_A[a])
        f = rel * np.float64(dims_B[a])
        region = int(np.float64(proportion[a]) * np.float64(dims_B[a]))
        lo.append(max(int(f - np.float64(region) / 2), 0))
        hi.append(min(int(f + np.float64(region) / 2), dims_B[a]))
    return lo, hi


def weight_map(mask, weight, patch, box=None):
    """float64 map of the whole volume: the weight of every voxel inside zone [∩ box], 0 elsewhere"""
    mask = np.asarray(mask)
    lo, hi = zone_of(mask.shape, patch)
    m = np.zeros(mask.shape, np.float64)
    if all(h > l for l, h in zip(lo, hi)):
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1.0
    m *= (mask != 0)
    if weight is not None:
        m *= np.maximum(np.asarray(weight).astype(np.float64), 0.0)
    if box is not None:
        b = np.zeros(mask.shape, np.float64)
        b[box[0][0]:box[1][0], box[0][1]:box[1][1], box[0][2]:box[1][2]] = 1.0
        m *= b
    return m


def select(m, u, weighted):
    """the rule on a weight map: (z, y, x) or None"""
    w = m.ravel()
    pos = np.flatnonzero(w > 0)
    if pos.size == 0:
        return None
    if not weighted:                                # mask-only: the k-th non-zero voxel
        k = min(int(math.floor(np.float64(u) * np.float64(pos.size))), pos.size - 1)
        flat = pos[k]
    else:
        prefix = np.cumsum(w)
        hit = np.flatnonzero(prefix > np.float64(u) * prefix[-1])
        flat = hit[0] if hit.size else pos[-1]
    return tuple(int(v) for v in np.unravel_index(int(flat), m.shape))


def voxel_draw(mask, weight, patch, u, focal_A=None, dims_A=None, proportion=None):
    """(z, y, x, fallback_used); (-1, -1, -1, flag) for an empty set"""
    mask = np.asarray(mask)
    flag = 0
    m = None
    if focal_A is not None:
        box = focal_box(focal_A, dims_A, mask.shape, proportion)
        m = weight_map(mask, weight, patch, box)
        if not (m > 0).any():
            flag, m = 1, None
    if m is None:
        m = weight_map(mask, weight, patch)
    p = select(m, u, weight is not None)
    return (-1, -1, -1, flag) if p is None else (*p, flag)


def patch_clip_minmax(volumes, mask, point, patch, outside, divisor, lo, hi):
    """[C, d, h, w] float32: the five fp32 operations of gs_patch_clip_minmax, one numpy operation each"""
    mask = np.asarray(mask)
    start = [min(max(int(point[a]) - patch[a] // 2, 0), mask.shape[a] - patch[a]) for a in range(3)]
    win = tuple(slice(s, s + p) for s, p in zip(start, patch))
    out = []
    f = np.float32
    for c, vol in enumerate(volumes):
        v = np.where(mask[win] != 0, np.asarray(vol)[win].astype(np.float32), f(outside[c])).astype(np.float32)
        v = v / f(divisor[c])
        v = np.minimum(np.maximum(v, f(lo[c])), f(hi[c]))
        v = (v - f(lo[c])) / (f(hi[c]) - f(lo[c]))
        v = f(2) * v - f(1)
        assert v.dtype == np.float32
        out.append(v)
    return np.stack(out)


class RefMMOps:
    """the two ops on CPU tensors, with HipOps' signatures"""

    def voxel_draw_range_len(self, dims, patch):
        lo, hi = zone_of([int(v) for v in dims], [int(v) for v in patch])
        if any(h <= l for l, h in zip(lo, hi)):
            return 0
        n = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
        return -(-n // NR)

    def voxel_draw(self, mask, weight, patch, u, out, focal_A=None, dims_A=None, proportion=None):
        got = voxel_draw(mask.numpy(), None if weight is None else weight.numpy(), [int(v) for v in patch], u,
                         None if focal_A is None else [int(v) for v in focal_A[:3]], dims_A, proportion)
        out.copy_(torch.tensor(got, dtype=torch.int32))

    def patch_clip_minmax(self, volumes, mask, point, patch, outside, divisor, lo, hi, out):
        out.copy_(torch.from_numpy(patch_clip_minmax([v.numpy() for v in volumes], mask.numpy(), [int(v) for v in point[:3]],
                                                     [int(v) for v in patch], outside, divisor, lo, hi)))
