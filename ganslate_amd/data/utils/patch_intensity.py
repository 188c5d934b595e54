"""Intensity augmentation of 3-D training patches: a smooth multiplicative bias field, contrast and brightness, gamma and
additive Gaussian noise on the normalised value the patch chains already form. The definition is stated once in
include/ganslate_hip.h (gs_patch_augment_clip_minmax / gs_patch_zscore_intensity) and restated here in numpy — this module
is the datasets' host path, csrc/intensity.hpp the device path, tests/patch_intensity_ref.py the per-voxel loop both are
tested against.

The chain acts on n in [0, 1]: n = (v - lo) / (hi - lo) of the clip / min-max chain (before 2 n - 1), n = (t - min t) /
(max t - min t) of the z-score with rescale (before span n + lo). Per modality a row (gamma, contrast, brightness,
noise_std, bias, key0, key1); float32, one IEEE operation per step:
    1. bias != 0:    m = float32(1.0 + float64(bias) * beta), n = n * m; beta the cubic B-spline interpolation of ONE
                     scalar lattice BETA[G_0][G_1][G_2] (float64 in [-1, 1]) exactly as one component of the elastic field
                     (data/utils/patch_affine.py), shared by the modalities of the domain
    2. contrast != 1 or brightness != 0:    n = (((n - 0.5) * contrast) + 0.5) + brightness
    3. n = min(max(n, 0), 1), NaN stays NaN
    4. gamma != 1:   n = n ** gamma (the one step whose bits host and device need not share)
    5. noise_std > 0:    n = n + noise_std * z, z = sqrt(-2 ln u1) cos(2 pi u2) from the first two words of Philox4x32-10
                     on the counter (i & 0xffffffff, i >> 32, c, 0) — i the voxel's linear index in the patch, c its channel
                     — and the key (key0, key1); u1 = ((r0 >> 9) + 0.5) 2^-23, u2 = (r1 >> 8) 2^-24
    6. step 3 again
A step with neutral parameters is skipped, not evaluated, so a neutral row changes no bit.

`augmentation.intensity` in a dataset config: {prob: 1.0 (per modality and sample), modalities: null (all) or a list of
names, gamma: [1, 1], contrast: [1, 1], brightness: [0, 0], noise_std: [0, 0], bias_field: null or {prob: 1.0,
control_points: [4, 4, 4], max: 0.3}}. `draw_block` takes, per domain and after the domain's geometric set, seven
np.random uniforms per modality in channel order — always all of them — and with `bias_field` set 1 + G_0 G_1 G_2 more."""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .patch_affine import MAX_CONTROL_POINTS, bspline_axis

KEYS = ("prob", "modalities", "gamma", "contrast", "brightness", "noise_std", "bias_field")
BIAS_KEYS = ("prob", "control_points", "max")
UNIFORMS = 7          # np.random uniforms per modality of a block
F = np.float32
NEUTRAL = (1.0, 1.0, 0.0, 0.0, 0.0, 0, 0)       # gamma, contrast, brightness, noise_std, bias, key0, key1


@dataclass(frozen=True)
class BiasField:
    prob: float = 1.0
    control_points: Tuple[int, int, int] = (4, 4, 4)
    max: float = 0.3

    @property
    def uniforms(self):
        """np.random uniforms per drawn lattice: the switch, then one per control point"""
        g = self.control_points
        return 1 + g[0] * g[1] * g[2]


@dataclass(frozen=True)
class IntensityAugmentation:
    prob: float = 1.0
    modalities: Optional[Tuple[str, ...]] = None
    gamma: Tuple[float, float] = (1.0, 1.0)
    contrast: Tuple[float, float] = (1.0, 1.0)
    brightness: Tuple[float, float] = (0.0, 0.0)
    noise_std: Tuple[float, float] = (0.0, 0.0)
    bias_field: Optional[BiasField] = None

    def uniforms(self, channels):
        """np.random uniforms of one block of a domain with `channels` modalities"""
        return UNIFORMS * channels + (0 if self.bias_field is None else self.bias_field.uniforms)


def _range(name, value):
    try:
        vals = [float(v) for v in value]
    except TypeError:
        raise ValueError(f"augmentation.intensity.{name}: expected [lo, hi]; got {value!r}") from None
    if len(vals) != 2 or not all(math.isfinite(v) for v in vals):
        raise ValueError(f"augmentation.intensity.{name}: expected two finite numbers [lo, hi]; got {vals}")
    if vals[0] > vals[1]:
        raise ValueError(f"augmentation.intensity.{name} needs lo <= hi; got {vals}")
    return tuple(vals)


def _prob(name, value):
    prob = float(value)
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"augmentation.intensity.{name} must lie in [0, 1]; got {prob}")
    return prob


def parse_intensity(node):
    """the `intensity` sub-field of `augmentation` -> IntensityAugmentation, or None when it is absent / null"""
    if node is None:
        return None
    unknown = sorted(set(node.keys()) - set(KEYS))
    if unknown:
        raise ValueError(f"augmentation.intensity: unknown keys {unknown}; known: {list(KEYS)}")
    get = lambda k, default: default if k not in node or node[k] is None else node[k]
    names = get("modalities", None)
    if names is not None:
        if isinstance(names, str) or len(names) == 0:
            raise ValueError(f"augmentation.intensity.modalities: expected null or a non-empty list of names; got {names!r}")
        names = tuple(str(n) for n in names)
    gamma = _range("gamma", get("gamma", (1.0, 1.0)))
    if not gamma[0] > 0.0:
        raise ValueError(f"augmentation.intensity.gamma needs 0 < lo <= hi; got {list(gamma)}")
    contrast = _range("contrast", get("contrast", (1.0, 1.0)))
    if contrast[0] < 0.0:
        raise ValueError(f"augmentation.intensity.contrast needs 0 <= lo <= hi; got {list(contrast)}")
    noise = _range("noise_std", get("noise_std", (0.0, 0.0)))
    if noise[0] < 0.0:
        raise ValueError(f"augmentation.intensity.noise_std needs 0 <= lo <= hi; got {list(noise)}")
    return IntensityAugmentation(_prob("prob", get("prob", 1.0)), names, gamma, contrast,
                                 _range("brightness", get("brightness", (0.0, 0.0))), noise,
                                 parse_bias_field(get("bias_field", None)))


def parse_bias_field(node):
    """the `bias_field` sub-field -> BiasField, or None when it is absent / null"""
    if node is None:
        return None
    unknown = sorted(set(node.keys()) - set(BIAS_KEYS))
    if unknown:
        raise ValueError(f"augmentation.intensity.bias_field: unknown keys {unknown}; known: {list(BIAS_KEYS)}")
    get = lambda k, default: default if k not in node or node[k] is None else node[k]
    raw = list(get("control_points", (4, 4, 4)))
    if len(raw) != 3 or not all(float(v) == int(v) for v in raw):
        raise ValueError(f"augmentation.intensity.bias_field.control_points: expected three integers (D, H, W); got {raw}")
    grid = tuple(int(v) for v in raw)
    if min(grid) < 4:
        raise ValueError(f"augmentation.intensity.bias_field.control_points: a cubic B-spline lattice needs at least 4 per "
                         f"axis; got {list(grid)}")
    if grid[0] * grid[1] * grid[2] > MAX_CONTROL_POINTS:
        raise ValueError(f"augmentation.intensity.bias_field.control_points: {list(grid)} are {grid[0] * grid[1] * grid[2]} "
                         f"control points; at most {MAX_CONTROL_POINTS}")
    top = float(get("max", 0.3))
    if not 0.0 <= top < 1.0:
        raise ValueError(f"augmentation.intensity.bias_field.max must lie in [0, 1); got {top}")
    return BiasField(_prob("bias_field.prob", get("prob", 1.0)), grid, top)


def check_intensity(cfg, patch, names):
    """Where the patch size and the dataset's modality names are known: refuses a name in `modalities` that the dataset
    does not have and, with `bias_field`, a patch axis under 2 voxels. cfg: IntensityAugmentation or None."""
    if cfg is None:
        return
    if cfg.modalities is not None:
        missing = [n for n in cfg.modalities if n not in names]
        if missing:
            raise ValueError(f"augmentation.intensity.modalities: {missing} not among the dataset's {list(names)}")
    if cfg.bias_field is not None:
        patch = [int(p) for p in patch]
        if len(patch) != 3 or min(patch) < 2:
            raise ValueError(f"augmentation.intensity.bias_field needs a 3-D patch_size of at least 2 voxels per axis; got "
                             f"{patch}")


def row(gamma=1.0, contrast=1.0, brightness=0.0, noise_std=0.0, bias=0.0, key0=0, key1=0):
    """one modality's parameters as they travel: the five numbers rounded to float32, the key as two uint32"""
    return (float(F(gamma)), float(F(contrast)), float(F(brightness)), float(F(noise_std)), float(F(bias)),
            int(key0) & 0xffffffff, int(key1) & 0xffffffff)


def is_neutral(r):
    """True when no step of the chain runs for this row"""
    return r[0] == 1.0 and r[1] == 1.0 and r[2] == 0.0 and not r[3] > 0.0 and r[4] == 0.0


def draw_block(cfg, names):
    """(rows, lattice) of one domain: per modality of `names` in channel order seven np.random uniforms, always all of them
    — u0 < prob switches a listed modality on, u1..u4 give gamma, contrast, brightness and noise_std as lo + u (hi - lo)
    (float64, then rounded to float32), u5 and u6 the key floor(u 2^32); a modality switched off or not listed gets the
    neutral row. With `bias_field` 1 + G_0 G_1 G_2 more in one vectorised draw: the first < bias_field.prob switches the
    lattice on, the others are BETA = 2 u - 1 (float64 [G_0, G_1, G_2]); a modality that is on then has bias =
    bias_field.max. lattice is None without `bias_field` or when switched off."""
    draws = []
    for name in names:
        u = [float(np.random.random_sample()) for _ in range(UNIFORMS)]
        draws.append((u, u[0] < cfg.prob and (cfg.modalities is None or name in cfg.modalities)))
    lattice = None
    if cfg.bias_field is not None:
        b = cfg.bias_field
        u = np.random.random_sample(b.uniforms)
        if float(u[0]) < b.prob:
            lattice = np.ascontiguousarray(2.0 * u[1:].reshape(b.control_points) - 1.0)
    bias = cfg.bias_field.max if lattice is not None else 0.0
    rows = []
    for u, on in draws:
        if not on:
            rows.append(row())
            continue
        pick = lambda r, v: r[0] + v * (r[1] - r[0])
        rows.append(row(pick(cfg.gamma, u[1]), pick(cfg.contrast, u[2]), pick(cfg.brightness, u[3]), pick(cfg.noise_std, u[4]),
                        bias, int(math.floor(u[5] * 4294967296.0)), int(math.floor(u[6] * 4294967296.0))))
    if lattice is not None and all(r[4] == 0.0 for r in rows):
        lattice = None                       # nobody reads it
    return tuple(rows), lattice


def active(intensity):
    """the (rows, lattice) a sample carries, or None when it carries none or every row is neutral"""
    if intensity is None or all(is_neutral(r) for r in intensity[0]):
        return None
    return intensity


def bias_field(patch, lattice):
    """beta, float64 [d, h, w]: the cubic B-spline interpolation of the scalar lattice over the patch — D innermost, then H,
    W outermost, every numpy operation one IEEE operation per element (patch_affine.displacement for one component)"""
    lattice = np.asarray(lattice, dtype=np.float64)
    if lattice.ndim != 3 or min(lattice.shape) < 4 or min(int(p) for p in patch) < 2:
        raise ValueError(f"bias lattice {lattice.shape} on patch {list(patch)}: expected [G0, G1, G2] with every G >= 4 and a "
                         f"patch of at least 2 voxels per axis")
    (j0, Bz), (j1, By), (j2, Bx) = [bspline_axis(patch[a], lattice.shape[a]) for a in range(3)]
    j0, j1, j2 = j0[:, None, None], j1[None, :, None], j2[None, None, :]
    Bz = [b[:, None, None] for b in Bz]
    By = [b[None, :, None] for b in By]
    Bx = [b[None, None, :] for b in Bx]
    dot = lambda B, v: ((B[0] * v[0] + B[1] * v[1]) + B[2] * v[2]) + B[3] * v[3]
    with np.errstate(invalid="ignore", over="ignore"):
        return dot(Bx, [dot(By, [dot(Bz, [lattice[j0 + l, j1 + m, j2 + n] for l in range(4)]) for m in range(4)])
                        for n in range(4)])


M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


def philox_r01(c0, c1, c2, c3, key0, key1):
    """first two output words of Philox4x32-10 (Salmon et al., Random123), vectorised: counters as uint64 arrays holding
    32-bit values (broadcast against each other), the key two Python ints -> (r0, r1) uint64 arrays of 32-bit values"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3)])
    k0, k1 = int(key0) & 0xffffffff, int(key1) & 0xffffffff
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                    # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c0, c1


def noise_plane(count, channel, key0, key1):
    """z, float32 [count]: the Box-Muller value of voxels 0 .. count - 1 of one channel, in float32 as the kernels form it"""
    i = np.arange(int(count), dtype=np.uint64)
    r0, r1 = philox_r01(i, i >> np.uint64(32), np.uint64(int(channel)), np.uint64(0), key0, key1)
    u1 = ((r0 >> np.uint64(9)).astype(F) + F(0.5)) * F(2.0 ** -23)
    u2 = (r1 >> np.uint64(8)).astype(F) * F(2.0 ** -24)
    z = np.sqrt(F(-2.0) * np.log(u1)) * np.cos(F(6.283185307179586) * u2)
    assert z.dtype == F
    return z


def apply(n, r, beta=None, channel=0):
    """the chain on n (float32, the patch's [d, h, w]) for the row r; beta: bias_field(...) of the domain's lattice (needed
    when r's bias is not 0). Every numpy operation is one IEEE operation per element."""
    n = np.asarray(n)
    assert n.dtype == F
    gamma, contrast, brightness, noise_std, bias = [F(v) for v in r[:5]]
    with np.errstate(invalid="ignore", over="ignore"):
        if bias != 0:
            m = (1.0 + np.float64(bias) * np.asarray(beta, dtype=np.float64)).astype(F)
            n = n * m
        if contrast != 1 or brightness != 0:
            n = (((n - F(0.5)) * contrast) + F(0.5)) + brightness
        n = np.where(n < 0, F(0), n)
        n = np.where(n > 1, F(1), n)
        if gamma != 1:
            n = np.power(n, gamma)
        if noise_std > 0:
            n = n + noise_std * noise_plane(n.size, channel, r[5], r[6]).reshape(n.shape)
        n = np.where(n < 0, F(0), n)
        n = np.where(n > 1, F(1), n)
    assert n.dtype == F
    return n


def z_score_intensity(patch, r, beta=None, scale_to_range=(-1.0, 1.0)):
    """z_score_normalize(patch, scale_to_range) of data/utils/normalization.py with the chain on n = (t - min t) /
    (max t - min t): torch tensor in, torch tensor out"""
    import torch
    t = (patch - patch.mean()) / patch.std()
    n = (t - t.min()) / (t.max() - t.min())
    n = torch.from_numpy(apply(n.numpy(), r, beta))
    lo, hi = F(scale_to_range[0]), F(scale_to_range[1])
    return torch.from_numpy((hi - lo) * n.numpy() + lo)
