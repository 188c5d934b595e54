"""CPU reference of the elastic patch gather (gs_patch_elastic_clip_minmax / gs_patch_elastic, csrc/volsample.hip; host path
ganslate_amd/data/utils/patch_affine.py), restated from the definition in include/ganslate_hip.h as a plain per-voxel loop:
Python ints for the lattice interval, Python floats (IEEE doubles, one rounding per operation, no fused multiply-add) for
the B-spline weights, the displacement and r' = r + u. Everything after r' — the matrix, floor, t, the reach test, the
masked corners, the float32 lerps, the clip / min-max chain — is the loop of tests/patch_affine_ref.py, called with the
per-voxel displacements (its `coords` adds them to r and carries the elastic definition's t = 0 outside the reach test).
Nothing here calls the package's sampling code or the kernels.

The displacement is a function of (patch, field) alone, about 500 float operations per voxel: `displacements` keeps the last
few, so the tests of one case pay for it once. `RefElasticOps` carries HipOps' signatures for the pipelines' control flow."""
import functools

import numpy as np
import torch

from tests import patch_affine_ref as A


def axis_weights(o, p, G):
    """(j, (B0, B1, B2, B3)) of output index o on an axis of p voxels over G control points"""
    num, den = o * (G - 3), p - 1
    j = min(num // den, G - 4)
    f = float(num - j * den) / float(den)
    f2 = f * f
    f3 = f2 * f
    g = 1.0 - f
    B0 = ((g * g) * g) / 6.0
    B1 = ((3.0 * f3 - 6.0 * f2) + 4.0) / 6.0
    B2 = (((3.0 * f2 - 3.0 * f3) + 3.0 * f) + 1.0) / 6.0
    B3 = f3 / 6.0
    return j, (B0, B1, B2, B3)


def dot4(B, v):
    return ((B[0] * v[0] + B[1] * v[1]) + B[2] * v[2]) + B[3] * v[3]


@functools.lru_cache(maxsize=8)
def _displacements(patch, grid, raw):
    phi = np.frombuffer(raw, dtype=np.float64).reshape(3, *grid).tolist()          # Python floats
    rows = []
    for oz in range(patch[0]):
        j0, Bz = axis_weights(oz, patch[0], grid[0])
        for oy in range(patch[1]):
            j1, By = axis_weights(oy, patch[1], grid[1])
            for ox in range(patch[2]):
                j2, Bx = axis_weights(ox, patch[2], grid[2])
                u = []
                for a in range(3):
                    R = []
                    for n in range(4):
                        q = [dot4(Bz, [phi[a][j0 + l][j1 + m][j2 + n] for l in range(4)]) for m in range(4)]
                        R.append(dot4(By, q))
                    u.append(dot4(Bx, R))
                rows.append(tuple(u))
    return rows


def displacements(patch, field):
    """per output voxel in C order: (u_0, u_1, u_2) — the naive per-voxel evaluation, D innermost, W outermost"""
    field = np.ascontiguousarray(field, dtype=np.float64)
    assert field.ndim == 4 and field.shape[0] == 3 and min(field.shape[1:]) >= 4 and min(patch) >= 2
    return _displacements(tuple(int(p) for p in patch), tuple(field.shape[1:]), field.tobytes())


def gather(volumes, mask, start, patch, M, field, outside):
    """[C, d, h, w] float32: the affine reference's gather loop on the displaced coordinates"""
    patch = [int(p) for p in patch]
    return A.gather(volumes, mask, start, patch, M, outside, displacements(patch, field))


def patch_elastic_clip_minmax(volumes, mask, point, patch, M, field, outside, divisor, lo, hi):
    patch = [int(p) for p in patch]
    g = gather(volumes, mask, A.start_of(point, patch, mask.shape), patch, M, field, outside)
    return np.stack([A.clip_minmax(g[c], divisor[c], lo[c], hi[c]) for c in range(len(volumes))])


def patch_elastic(volume, start, size, M, field, fill):
    return gather([volume], None, [int(v) for v in start], size, M, field, [fill])[0]


def random_field(grid, patch, seed, fraction=0.35):
    """uniform control-point displacements within `fraction` (< 0.4, the fold guard) of the control spacing, voxels"""
    rng = np.random.default_rng(seed)
    bound = np.array([fraction * (patch[a] - 1) / (grid[a] - 3) for a in range(3)]).reshape(3, 1, 1, 1)
    return np.ascontiguousarray((2.0 * rng.random((3, *grid)) - 1.0) * bound)


def far_field(grid, patch, seed):
    """displacements of ten patch sizes (0.9 to 1.1 of that), one sign, behind two zero control planes at the low W end:
    the first voxels of a row stay near the patch, all others land far outside any of the test volumes"""
    rng = np.random.default_rng(seed)
    field = (0.9 + 0.2 * rng.random((3, *grid))) * (10.0 * np.array(patch, dtype=np.float64)).reshape(3, 1, 1, 1)
    field[..., :2] = 0.0
    return np.ascontiguousarray(field)


class RefElasticOps(A.RefAffineOps):
    """the two elastic ops on CPU tensors, with HipOps' signatures"""

    def patch_elastic_clip_minmax(self, volumes, mask, point, patch, matrix, field, outside, divisor, lo, hi, out):
        M = np.asarray(matrix, dtype=np.float64).reshape(3, 3)
        out.copy_(torch.from_numpy(patch_elastic_clip_minmax([v.numpy() for v in volumes], mask.numpy(),
                                                             [int(v) for v in point[:3]], patch, M, field.numpy(), outside,
                                                             divisor, lo, hi)))

    def patch_elastic(self, volume, start, size, matrix, field, fill, out):
        M = np.asarray(matrix, dtype=np.float64).reshape(3, 3)
        out.copy_(torch.from_numpy(patch_elastic(volume.numpy(), start, size, M, field.numpy(), fill)))
