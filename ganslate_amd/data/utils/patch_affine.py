"""Random affine augmentation of 3-D training patches: flips, small rotations and zoom as ONE trilinear gather through a
3 x 3 matrix. Not in the reference (its HX4 train_dataset.py:3 asks "What's a good way to use data augmentation ?"); the
definition is stated once in include/ganslate_hip.h (gs_patch_affine_clip_minmax) and restated here in numpy — this module
is the datasets' host path, csrc/volsample.hip the device path, tests/patch_affine_ref.py the per-voxel loop both are
tested against.

For a volume of size (D, H, W), a patch p = (d, h, w) starting at `start` and a matrix M (patch offsets -> source offsets):
    c_a = (p_a - 1) / 2,  r = o - c                                              float64, exact
    s_a = ((M[a][0] r_0 + M[a][1] r_1) + M[a][2] r_2) + (start_a + c_a)          float64, one rounding per operation
    i_a = floor(s_a),  t_a = float32(s_a - i_a)
    any s_a < -1 or s_a >= size_a (or NaN): all eight corners are outside
    corner value: float32(volume[corner]) when inside the volume and (with a mask) mask[corner] != 0, else `outside`
    lerp(a, b, t) = a + t * (b - a) in float32, along W, then H, then D
M = I is the plain crop, diag(+-1) the flipped crop, a signed permutation np.rot90 of it (as equal numbers).

`augmentation` in a dataset config: {prob: 1.0, flip: [false, false, false], rotate_deg: [0, 0, 0], scale: [1, 1],
spacing: [1, 1, 1], fill: 0.0 (UnpairedVolumeDataset only)}. Per sample and matrix `draw_params` takes eight np.random
uniforms — always all eight, after the sample's other draws."""
import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np

KEYS = ("prob", "flip", "rotate_deg", "scale", "spacing", "fill")
UNIFORMS = 8          # np.random uniforms per drawn matrix


@dataclass(frozen=True)
class AffineAugmentation:
    prob: float = 1.0
    flip: Tuple[bool, bool, bool] = (False, False, False)
    rotate_deg: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    scale: Tuple[float, float] = (1.0, 1.0)
    spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    fill: float = 0.0


def _numbers(name, value, n):
    try:
        vals = [float(v) for v in value]
    except TypeError:
        raise ValueError(f"augmentation.{name}: expected {n} numbers; got {value!r}") from None
    if len(vals) != n or not all(math.isfinite(v) for v in vals):
        raise ValueError(f"augmentation.{name}: expected {n} finite numbers; got {vals}")
    return tuple(vals)


def parse_augmentation(node, fill_allowed):
    """the `augmentation` field of a dataset config -> AffineAugmentation, or None when the field is absent / null"""
    if node is None:
        return None
    unknown = sorted(set(node.keys()) - set(KEYS))
    if unknown:
        raise ValueError(f"augmentation: unknown keys {unknown}; known: {list(KEYS)}")
    get = lambda k, default: default if k not in node or node[k] is None else node[k]
    prob = float(get("prob", 1.0))
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"augmentation.prob must lie in [0, 1]; got {prob}")
    flip = list(get("flip", (False, False, False)))
    if len(flip) != 3:
        raise ValueError(f"augmentation.flip: expected three booleans (D, H, W); got {flip}")
    rotate = _numbers("rotate_deg", get("rotate_deg", (0.0, 0.0, 0.0)), 3)
    scale = _numbers("scale", get("scale", (1.0, 1.0)), 2)
    if not 0.0 < scale[0] <= scale[1]:
        raise ValueError(f"augmentation.scale needs 0 < lo <= hi; got {list(scale)}")
    spacing = _numbers("spacing", get("spacing", (1.0, 1.0, 1.0)), 3)
    if min(spacing) <= 0.0:
        raise ValueError(f"augmentation.spacing must be positive; got {list(spacing)}")
    if "fill" in node and node["fill"] is not None and not fill_allowed:
        raise ValueError("augmentation.fill is UnpairedVolumeDataset's; here a voxel outside the volume or the body mask "
                         "takes the modality's `outside_value`")
    return AffineAugmentation(prob, tuple(bool(v) for v in flip), rotate, scale, spacing, float(get("fill", 0.0)))


def _cos_sin(deg):
    """(cos, sin) of an angle in degrees, exact at multiples of 90"""
    q = math.fmod(float(deg), 360.0)
    exact = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0),
             -90.0: (0.0, -1.0), -180.0: (-1.0, 0.0), -270.0: (0.0, 1.0)}
    if q in exact:
        return exact[q]
    th = math.radians(q)
    return math.cos(th), math.sin(th)


def rotation(axis, deg):
    """R_axis: the rotation by `deg` degrees in the plane of the other two axes"""
    c, s = _cos_sin(deg)
    i, j = [a for a in range(3) if a != axis]
    R = [[1.0 if a == b else 0.0 for b in range(3)] for a in range(3)]
    R[i][i], R[i][j], R[j][i], R[j][j] = c, -s, s, c
    return R


def _matmul(A, B):
    return [[(A[a][0] * B[0][b] + A[a][1] * B[1][b]) + A[a][2] * B[2][b] for b in range(3)] for a in range(3)]


def affine_matrix(flips, angles_deg, zoom, spacing):
    """M = diag(1 / sp) . R_0(th_0) . R_1(th_1) . R_2(th_2) . diag(f) . (1 / zoom) . diag(sp), float64 [3, 3]: patch offsets
    (voxels) -> source offsets (voxels). f_a = -1 for a flipped axis; sp = voxel spacing (D, H, W), so that the rotation is
    rigid in millimetres on anisotropic volumes; zoom > 1 magnifies (the source step shrinks). Built as
    M[a][b] = (R[a][b] * f_b / zoom) * (sp_b / sp_a): neutral parameters give eye(3), flips diag(+-1), zoom 2 I / 2 and
    equal spacings no trace of the spacing — all exactly."""
    zoom = float(zoom)
    sp = [float(v) for v in spacing]
    if not (zoom > 0.0 and math.isfinite(zoom)) or len(sp) != 3 or not all(v > 0.0 and math.isfinite(v) for v in sp):
        raise ValueError(f"affine_matrix: zoom {zoom} and spacing {sp} must be positive and finite")
    R = _matmul(_matmul(rotation(0, angles_deg[0]), rotation(1, angles_deg[1])), rotation(2, angles_deg[2]))
    f = [-1.0 if v else 1.0 for v in flips]
    inv = 1.0 / zoom
    return np.array([[(R[a][b] * f[b] * inv) * (sp[b] / sp[a]) for b in range(3)] for a in range(3)], dtype=np.float64)


def draw_params(cfg):
    """One matrix from eight np.random uniforms, always all eight: u0 < prob applies rotation + zoom, u1..u3 < 0.5 flips an
    enabled axis, th_a = (2 u_{4+a} - 1) rotate_deg[a], zoom = lo + u7 (hi - lo); without the affine part M = diag(f)."""
    u = [float(np.random.random_sample()) for _ in range(UNIFORMS)]
    flips = [bool(cfg.flip[a]) and u[1 + a] < 0.5 for a in range(3)]
    if not u[0] < cfg.prob:
        return np.diag([-1.0 if v else 1.0 for v in flips])
    angles = [(2.0 * u[4 + a] - 1.0) * cfg.rotate_deg[a] for a in range(3)]
    zoom = cfg.scale[0] + u[7] * (cfg.scale[1] - cfg.scale[0])
    return affine_matrix(flips, angles, zoom, cfg.spacing)


def matrix_tuple(M):
    """the 9-tuple of floats (row-major) a worker hands over"""
    return tuple(float(v) for v in np.asarray(M, dtype=np.float64).reshape(9))


def sample_patch(volume, mask, start, patch, M, outside):
    """float32 [d, h, w]: the definition above, vectorised — every numpy operation is one IEEE operation per element.
    volume: (D, H, W) array of any real dtype (read as float32); mask: (D, H, W) or None."""
    vol = np.asarray(volume)
    size = vol.shape
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    f32 = np.float32
    c = [(int(p) - 1) / 2.0 for p in patch]
    o = np.meshgrid(*[np.arange(int(p), dtype=np.float64) for p in patch], indexing="ij")
    r = [o[a] - c[a] for a in range(3)]
    s = [((M[a, 0] * r[0] + M[a, 1] * r[1]) + M[a, 2] * r[2]) + (float(int(start[a])) + c[a]) for a in range(3)]
    fl = [np.floor(x) for x in s]
    with np.errstate(invalid="ignore"):
        t = [(x - y).astype(f32) for x, y in zip(s, fl)]
        reach = np.ones(s[0].shape, bool)
        for a in range(3):
            reach &= (s[a] >= -1.0) & (s[a] < float(size[a]))
    i = [np.where(reach, x, 0.0).astype(np.int64) for x in fl]
    fill = f32(outside)

    def corner(dz, dy, dx):
        z, y, x = i[0] + dz, i[1] + dy, i[2] + dx
        ok = reach & (z >= 0) & (z < size[0]) & (y >= 0) & (y < size[1]) & (x >= 0) & (x < size[2])
        zc, yc, xc = np.clip(z, 0, size[0] - 1), np.clip(y, 0, size[1] - 1), np.clip(x, 0, size[2] - 1)
        if mask is not None:
            ok &= np.asarray(mask)[zc, yc, xc] != 0
        return np.where(ok, vol[zc, yc, xc].astype(f32), fill)

    def lerp(a, b, w):
        d = b - a
        p = w * d
        return a + p

    with np.errstate(invalid="ignore", over="ignore"):
        c00, c01 = lerp(corner(0, 0, 0), corner(0, 0, 1), t[2]), lerp(corner(0, 1, 0), corner(0, 1, 1), t[2])
        c10, c11 = lerp(corner(1, 0, 0), corner(1, 0, 1), t[2]), lerp(corner(1, 1, 0), corner(1, 1, 1), t[2])
        out = lerp(lerp(c00, c01, t[1]), lerp(c10, c11, t[1]), t[0])
    assert out.dtype == f32
    return out
