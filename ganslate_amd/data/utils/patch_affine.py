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

Elastic deformation (`elastic`, also stated in include/ganslate_hip.h) is a free-form deformation in front of the matrix:
a lattice of G = (G_0, G_1, G_2) >= 4 control-point displacements PHI[a][i][j][k] (float64, voxels of axis a), aligned
with the patch so that [0, p_a - 1] spans its G_a - 3 inner intervals, interpolated by uniform cubic B-splines:
    num = o_a (G_a - 3), den = p_a - 1, j_a = min(num // den, G_a - 4), f = float(num - j_a den) / float(den)
    f2 = f f, f3 = f2 f, g = 1 - f
    B0 = ((g g) g) / 6, B1 = ((3 f3 - 6 f2) + 4) / 6, B2 = (((3 f2 - 3 f3) + 3 f) + 1) / 6, B3 = f3 / 6
    q[m][n] = ((Bz0 PHI[a][j_0][j_1+m][j_2+n] + Bz1 PHI[a][j_0+1][..]) + Bz2 PHI[a][j_0+2][..]) + Bz3 PHI[a][j_0+3][..]
    R[n] = ((By0 q[0][n] + By1 q[1][n]) + By2 q[2][n]) + By3 q[3][n]
    u_a = ((Bx0 R[0] + Bx1 R[1]) + Bx2 R[2]) + Bx3 R[3];    r'_a = r_a + u_a
and s is computed from r' instead of r; the rest is unchanged, except that t_a = 0 where s_a fails the reach test (no bit
changes for a finite s_a; a NaN or infinite displacement then gives the outside value instead of NaN).

`augmentation` in a dataset config: {prob: 1.0, flip: [false, false, false], rotate_deg: [0, 0, 0], scale: [1, 1],
spacing: [1, 1, 1], fill: 0.0 (UnpairedVolumeDataset only), elastic: null or {prob: 1.0, control_points: [7, 7, 7],
max_displacement: [0, 4, 4]} (D, H, W; in the units of `spacing`)}. Per sample and matrix `draw_params` takes eight
np.random uniforms — always all eight, after the sample's other draws; with `elastic` set `draw_field` takes
1 + 3 G_0 G_1 G_2 more after them, always all of them. The `intensity` key (data/utils/patch_intensity.py: bias field,
contrast, brightness, gamma, noise on the normalised value) needs nothing else here: with everything else neutral the
matrix drawn is the identity."""
import math
from dataclasses import dataclass
from typing import Any, Optional, Tuple

import numpy as np

KEYS = ("prob", "flip", "rotate_deg", "scale", "spacing", "fill", "elastic", "intensity")
ELASTIC_KEYS = ("prob", "control_points", "max_displacement")
UNIFORMS = 8          # np.random uniforms per drawn matrix
MAX_CONTROL_POINTS = 1024      # GS_ELASTIC_MAX_POINTS: the lattice travels as 3 * 1024 doubles at the most
FOLD_BOUND = 0.4      # of the control spacing: Choi and Lee's sufficient bound for a 3-D cubic B-spline map without folds


@dataclass(frozen=True)
class ElasticAugmentation:
    prob: float = 1.0
    control_points: Tuple[int, int, int] = (7, 7, 7)
    max_displacement: Tuple[float, float, float] = (0.0, 0.0, 0.0)      # D, H, W, in the units of `spacing`

    @property
    def uniforms(self):
        """np.random uniforms per drawn field: the switch, then one per component and control point"""
        g = self.control_points
        return 1 + 3 * g[0] * g[1] * g[2]


@dataclass(frozen=True)
class AffineAugmentation:
    prob: float = 1.0
    flip: Tuple[bool, bool, bool] = (False, False, False)
    rotate_deg: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    scale: Tuple[float, float] = (1.0, 1.0)
    spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    fill: float = 0.0
    elastic: Optional[ElasticAugmentation] = None
    intensity: Optional[Any] = None          # patch_intensity.IntensityAugmentation


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
    from .patch_intensity import parse_intensity          # that module builds on this one
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
    return AffineAugmentation(prob, tuple(bool(v) for v in flip), rotate, scale, spacing, float(get("fill", 0.0)),
                              parse_elastic(get("elastic", None)), parse_intensity(get("intensity", None)))


def parse_elastic(node):
    """the `elastic` sub-field -> ElasticAugmentation, or None when it is absent / null"""
    if node is None:
        return None
    unknown = sorted(set(node.keys()) - set(ELASTIC_KEYS))
    if unknown:
        raise ValueError(f"augmentation.elastic: unknown keys {unknown}; known: {list(ELASTIC_KEYS)}")
    get = lambda k, default: default if k not in node or node[k] is None else node[k]
    prob = float(get("prob", 1.0))
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"augmentation.elastic.prob must lie in [0, 1]; got {prob}")
    raw = list(get("control_points", (7, 7, 7)))
    if len(raw) != 3 or not all(float(v) == int(v) for v in raw):
        raise ValueError(f"augmentation.elastic.control_points: expected three integers (D, H, W); got {raw}")
    grid = tuple(int(v) for v in raw)
    if min(grid) < 4:
        raise ValueError(f"augmentation.elastic.control_points: a cubic B-spline lattice needs at least 4 per axis; got "
                         f"{list(grid)}")
    if grid[0] * grid[1] * grid[2] > MAX_CONTROL_POINTS:
        raise ValueError(f"augmentation.elastic.control_points: {list(grid)} are {grid[0] * grid[1] * grid[2]} control points; "
                         f"at most {MAX_CONTROL_POINTS}")
    disp = _numbers("elastic.max_displacement", get("max_displacement", (0.0, 0.0, 0.0)), 3)
    if min(disp) < 0.0:
        raise ValueError(f"augmentation.elastic.max_displacement must not be negative; got {list(disp)}")
    return ElasticAugmentation(prob, grid, disp)


def check_elastic(cfg, patch):
    """Where the patch size is known: refuses a patch axis under 2 voxels and any axis a with
    max_displacement[a] / spacing[a] >= 0.4 (p_a - 1) / (G_a - 3), i.e. control-point displacements of 0.4 control
    spacings or more. Below that bound a 3-D cubic B-spline map is free of folds (Choi and Lee); it is applied per axis
    here, which is a guard and not a proof for lattices whose control spacing differs between the axes."""
    if cfg is None or cfg.elastic is None:
        return
    patch = [int(p) for p in patch]
    if len(patch) != 3 or min(patch) < 2:
        raise ValueError(f"augmentation.elastic needs a 3-D patch_size of at least 2 voxels per axis; got {patch}")
    for a in range(3):
        bound = FOLD_BOUND * (patch[a] - 1) / (cfg.elastic.control_points[a] - 3)        # voxels
        if cfg.elastic.max_displacement[a] / cfg.spacing[a] >= bound:
            raise ValueError(f"augmentation.elastic.max_displacement[{a}] = {cfg.elastic.max_displacement[a]} (axis {'DHW'[a]}) "
                             f"may fold the patch: with {cfg.elastic.control_points[a]} control points over {patch[a]} voxels "
                             f"of spacing {cfg.spacing[a]} it must stay below {bound * cfg.spacing[a]:.6g}")


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


def draw_field(cfg):
    """One lattice of control-point displacements from 1 + 3 G_0 G_1 G_2 np.random uniforms, always all of them (one
    vectorised draw, which consumes the stream as that many single draws would): the first < elastic.prob switches the
    field on, the others give PHI_mm[a][i][j][k] = (2 u - 1) max_displacement[a], component-major, lattice in C order.
    Returns float64 [3, G_0, G_1, G_2] in voxels (PHI_mm[a] / spacing[a]), or None when switched off."""
    e = cfg.elastic
    u = np.random.random_sample(e.uniforms)
    if not float(u[0]) < e.prob:
        return None
    mm = (2.0 * u[1:].reshape(3, *e.control_points) - 1.0) * np.asarray(e.max_displacement, np.float64).reshape(3, 1, 1, 1)
    return np.ascontiguousarray(mm / np.asarray(cfg.spacing, np.float64).reshape(3, 1, 1, 1))


def draw_set(cfg):
    """(M, field) of one patch: the matrix's eight uniforms, then — only with `elastic` set — the field's"""
    M = draw_params(cfg)
    return M, (None if cfg.elastic is None else draw_field(cfg))


def bspline_axis(p, G):
    """per output index of an axis of p voxels over G control points: (j [p] int64, (B0, B1, B2, B3) float64 [p] each)"""
    o = np.arange(int(p), dtype=np.int64)
    num, den = o * (int(G) - 3), int(p) - 1
    j = np.minimum(num // den, int(G) - 4)
    f = (num - j * den).astype(np.float64) / np.float64(den)
    f2 = f * f
    f3 = f2 * f
    g = 1.0 - f
    return j, (((g * g) * g) / 6.0, ((3.0 * f3 - 6.0 * f2) + 4.0) / 6.0, (((3.0 * f2 - 3.0 * f3) + 3.0 * f) + 1.0) / 6.0,
               f3 / 6.0)


def displacement(patch, field):
    """[u_0, u_1, u_2], float64 [d, h, w] each: the free-form deformation of the definition above, vectorised — D
    innermost, then H, W outermost, every numpy operation one IEEE operation per element"""
    field = np.asarray(field, dtype=np.float64)
    if field.ndim != 4 or field.shape[0] != 3 or min(field.shape[1:]) < 4 or min(int(p) for p in patch) < 2:
        raise ValueError(f"elastic field {field.shape} on patch {list(patch)}: expected [3, G0, G1, G2] with every G >= 4 and "
                         f"a patch of at least 2 voxels per axis")
    (j0, Bz), (j1, By), (j2, Bx) = [bspline_axis(patch[a], field.shape[1 + a]) for a in range(3)]
    j0, j1, j2 = j0[:, None, None], j1[None, :, None], j2[None, None, :]
    Bz = [b[:, None, None] for b in Bz]
    By = [b[None, :, None] for b in By]
    Bx = [b[None, None, :] for b in Bx]
    dot = lambda B, v: ((B[0] * v[0] + B[1] * v[1]) + B[2] * v[2]) + B[3] * v[3]
    with np.errstate(invalid="ignore", over="ignore"):
        return [dot(Bx, [dot(By, [dot(Bz, [field[a][j0 + l, j1 + m, j2 + n] for l in range(4)]) for m in range(4)])
                         for n in range(4)]) for a in range(3)]


def matrix_tuple(M):
    """the 9-tuple of floats (row-major) a worker hands over"""
    return tuple(float(v) for v in np.asarray(M, dtype=np.float64).reshape(9))


def sample_patch(volume, mask, start, patch, M, outside, field=None):
    """float32 [d, h, w]: the definition above, vectorised — every numpy operation is one IEEE operation per element.
    volume: (D, H, W) array of any real dtype (read as float32); mask: (D, H, W) or None; field: None or the elastic
    lattice, float64 [3, G0, G1, G2] in voxels."""
    vol = np.asarray(volume)
    size = vol.shape
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    f32 = np.float32
    c = [(int(p) - 1) / 2.0 for p in patch]
    o = np.meshgrid(*[np.arange(int(p), dtype=np.float64) for p in patch], indexing="ij")
    r = [o[a] - c[a] for a in range(3)]
    if field is not None:
        u = displacement(patch, field)
        with np.errstate(invalid="ignore", over="ignore"):
            r = [r[a] + u[a] for a in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        s = [((M[a, 0] * r[0] + M[a, 1] * r[1]) + M[a, 2] * r[2]) + (float(int(start[a])) + c[a]) for a in range(3)]
    fl = [np.floor(x) for x in s]
    with np.errstate(invalid="ignore"):
        t = [(x - y).astype(f32) for x, y in zip(s, fl)]
        reach = np.ones(s[0].shape, bool)
        for a in range(3):
            inside = (s[a] >= -1.0) & (s[a] < float(size[a]))
            reach &= inside
            if field is not None:
                t[a] = np.where(inside, t[a], f32(0))
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
