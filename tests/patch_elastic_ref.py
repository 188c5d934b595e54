"""CPU reference of the elastic patch gather (gs_patch_elastic_clip_minmax / gs_patch_elastic, csrc/volsample.hip; host path
ganslate_amd/data/utils/patch_affine.py), restated from the definition in include/ganslate_hip.h as a plain per-voxel loop:
Python ints for the lattice interval, Python floats (IEEE doubles, one rounding per operation, no fused multiply-add) for
the B-spline weights, the displacement and r' = r + u. Everything after r' — the matrix, floor, t, the reach test, the
masked corners, the float32 lerps, the clip / min-max chain — is the loop of tests/patch_affine_ref.py, called with its
per-voxel coordinates replaced by the displaced ones. Nothing here calls the package's sampling code or the kernels.

The displacement is a function of (patch, field) alone, about 500 float operations per voxel: `displacements` keeps the last
few, so the tests of one case pay for it once. `RefElasticOps` carries HipOps' signatures for the pipelines' control flow."""
import functools
import math
from unittest import mock

import numpy as np
import torch

from tests import patch_affine_ref as A

F = np.float32


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


def coords(size, patch, start, M, u):
    """tests/patch_affine_ref.py coords with r' = r + u, and t_a = 0 where s_a fails the reach test (s - floor(s) is no
    number for a NaN or infinite s): (reach, (i_0, i_1, i_2), (t_0, t_1, t_2)) per voxel"""
    M = [[float(M[a][b]) for b in range(3)] for a in range(3)]
    c = [(patch[a] - 1) / 2.0 for a in range(3)]
    base = [float(start[a]) + c[a] for a in range(3)]
    rows, n = [], 0
    for oz in range(patch[0]):
        for oy in range(patch[1]):
            for ox in range(patch[2]):
                r = (oz - c[0] + u[n][0], oy - c[1] + u[n][1], ox - c[2] + u[n][2])     # o - c is exact: one rounded add
                n += 1
                reach, idx, t = True, [], []
                for a in range(3):
                    p0 = M[a][0] * r[0]
                    p1 = M[a][1] * r[1]
                    p2 = M[a][2] * r[2]
                    s = ((p0 + p1) + p2) + base[a]
                    if not (s >= -1.0 and s < float(size[a])):         # NaN included
                        reach = False
                        idx.append(0)
                        t.append(F(0.0))                                   # the elastic definition's addition
                        continue
                    fl = math.floor(s)
                    idx.append(int(fl))
                    t.append(F(s - fl))
                rows.append((reach, idx, t))
    return rows


def gather(volumes, mask, start, patch, M, field, outside):
    """[C, d, h, w] float32: the affine reference's gather loop on the displaced coordinates"""
    patch = [int(p) for p in patch]
    u = displacements(patch, field)
    with mock.patch.object(A, "coords", lambda size, p, s, m: coords(size, p, s, m, u)):
        return A.gather(volumes, mask, start, patch, M, outside)


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
