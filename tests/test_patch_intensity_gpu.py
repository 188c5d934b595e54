"""Intensity augmentation in the patch launches on the GPU (csrc/volsample.hip gs_patch_augment_clip_minmax, csrc/volproc.hip
gs_patch_zscore_intensity, csrc/intensity.hpp) against the per-voxel loop of tests/patch_intensity_ref.py.

Cases (volume / patch): (9, 17, 13) / (3, 5, 7), 105 voxels, one partial workgroup; (12, 20, 40) / (4, 9, 31), 1116 voxels,
rows straddle workgroups and the width divides nothing; (16, 40, 40) / (8, 16, 16), 2048 voxels, several full workgroups
and, for the z-score entry, two workgroups of four voxels per thread (its grid-stride loop). Bias lattices (4, 4, 4) and
(5, 7, 9); every case with and without an elastic field of another grid, (4, 5, 6); every launch in both LDS forms (the
option elastic_rows = 0 forces the per-voxel form); every output in the middle of a NaN-filled buffer.

With gamma = 1 and noise_std = 0 the definition fixes every IEEE operation: equal bits are demanded. Else:
- gamma: against float64 pow of the float32 value in front of the step (tests/patch_intensity_ref.py chain64), counted in
  float32 ulps of the result, on the z-score entry with the range (0, 1), whose last step 1 * n + 0 changes no bit of n.
  The worst case seen on the MI355X is GAMMA_SEEN = 1.128 ulps (gammas 0.5 / 0.7 / 1.5 / 2.2: 1.008 / 1.104 / 1.065 / 1.128;
  the test prints them); the assertion is GAMMA_ULPS = twice that, 2.256, below the cap of 16 ulps beyond which it would be
  a wrong formula and not rounding.
- noise: 8e-6 * noise_std on n (the bound tests/test_mmimg_gpu.py derives for the same Philox / Box-Muller code: 6.3e-6 per
  unit std for the angle, logf, sqrtf and cosf, asserted at 8e-6). With noise_std >= 0.05, as here, the remaining 1.7e-6 *
  noise_std also covers the roundings of the product and the sum (2^-24 * (5.77 noise_std + 1)). Doubled after 2 n - 1.
- pipelines against the host path with gamma and noise on: host np.power (HOST_POW_ULPS) and device powf (GAMMA_ULPS)
  against the same float64 value, both noise planes against the same float64 plane, one ulp for each of the noise step's
  roundings on either side, doubled by 2 n - 1: PIPE_BOUND. The z-score pipeline is not bitwise to begin with (the
  statistics are summed in another order: tests/test_patch_elastic_gpu.py allows 2e-6 on the output); the exact steps
  stretch that by at most contrast * (1 + max) = 1.25 * 1.3 here.
The counter's second word (i >> 32) only differs from 0 beyond 2^32 voxels, a 16 GiB patch: not run here."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests import patch_affine_ref as A
from tests import patch_elastic_ref as E
from tests import patch_intensity_ref as R
from tests.test_mmvol_cpu import dataset_conf, toy_folder
from tests.test_patch_affine_gpu import PARAMS, ROT, _case, _dev, _i3, _poisoned, _untouched, _with_aug
from tests.test_patch_intensity_cpu import EXACT, HOST_POW_ULPS, INTENSITY
from tests.test_volume_patches_cpu import _conf as vol_conf
from tests.test_volume_patches_cpu import _volume_folder

pytestmark = pytest.mark.gpu

F = np.float32
GAMMA_SEEN = 1.128         # gammas 0.5 / 0.7 / 1.5 / 2.2: 1.008 / 1.104 / 1.065 / 1.128 ulps
GAMMA_ULPS = 2.0 * GAMMA_SEEN
assert GAMMA_ULPS <= 16.0
PIPE_BOUND = 2.0 * ((HOST_POW_ULPS + GAMMA_ULPS) * 2.0 ** -24 + 2.0 * 8e-6 * 0.05 + 4.0 * 2.0 ** -24)

CASES = [((9, 17, 13), (3, 5, 7)), ((12, 20, 40), (4, 9, 31)), ((16, 40, 40), (8, 16, 16))]
GRIDS = [(4, 4, 4), (5, 7, 9)]
ELASTIC_GRID = (4, 5, 6)
NAMES = [("ct",), ("pet",), ("pet", "ct", "hx4")]          # int16, fp32, C = 3 with mixed dtypes
# exact rows per modality; the middle one of C = 3 is neutral
EXACT_ROWS = [(1.0, 1.2, -0.05, 0.0, 0.3, 0, 0), R.NEUTRAL, (1.0, 0.8, 0.1, 0.0, -0.6, 0, 0)]


def _rows(names):
    return [EXACT_ROWS[0]] if len(names) == 1 else list(EXACT_ROWS)


def _point(shape):
    return tuple(s // 2 - 1 for s in shape)


def _aug(ops, dev_vols, dev_mask, names, point, patch, M, field, rows, lattice, finite=True):
    cols = list(zip(*[PARAMS[n] for n in names]))
    n = len(names) * int(np.prod(patch))
    buf, out = _poisoned(n, (len(names), *patch), ops.device)
    pt = torch.tensor([*point, 0], dtype=torch.int32, device=ops.device)
    ops.patch_augment_clip_minmax(dev_vols, dev_mask, pt, patch, M, None if field is None else _dev(field, ops.device), rows,
                                  None if lattice is None else _dev(lattice, ops.device), *cols, out)
    got = out.cpu().numpy()
    assert _untouched(buf, n) and (not finite or np.isfinite(got).all())
    return got, cols


def _geo(ops, dev_vols, dev_mask, names, point, patch, M, field):
    """today's entry points for the same geometry"""
    cols = list(zip(*[PARAMS[n] for n in names]))
    out = torch.empty((len(names), *patch), device=ops.device)
    pt = torch.tensor([*point, 0], dtype=torch.int32, device=ops.device)
    if field is None:
        ops.patch_affine_clip_minmax(dev_vols, dev_mask, pt, patch, M, *cols, out)
    else:
        ops.patch_elastic_clip_minmax(dev_vols, dev_mask, pt, patch, M, _dev(field, ops.device), *cols, out)
    return out.cpu().numpy()


def _zs(ops, dev_vol, start, patch, row, lattice, scale=(-1.0, 1.0), finite=True):
    n = int(np.prod(patch))
    buf, out = _poisoned(n, patch, ops.device)
    ops.patch_zscore_intensity(dev_vol, start, patch, out, row, None if lattice is None else _dev(lattice, ops.device), scale)
    got = out.cpu().numpy()
    assert _untouched(buf, n) and (not finite or np.isfinite(got).all())
    return got


def _t(ops, dev_vol, start, patch):
    """the plain z-score of the window, from today's entry point"""
    t = torch.empty(patch, device=ops.device)
    ops.patch_zscore(dev_vol, start, patch, t, None)
    return t.cpu().numpy()


# ---- the exact steps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", NAMES)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("shape,patch", CASES)
def test_clip_entry_equals_the_loop_reference(hip_ops, shape, patch, grid, names):
    """bits against the loop, both LDS forms, with and without an elastic field; the neutral modality of the mixed launch
    and an all-neutral launch give today's entry points"""
    v = _case(shape)
    dev_vols, dev_mask = [_dev(v[n], hip_ops.device) for n in names], _dev(v["holes"], hip_ops.device)
    lattice, rows, point = R.random_lattice(grid, 41), _rows(names), _point(shape)
    for field in (None, E.random_field(ELASTIC_GRID, patch, 17)):
        got = {}
        for option in (0, 32768):
            with hip_ops.options(elastic_rows=option):
                got[option], cols = _aug(hip_ops, dev_vols, dev_mask, names, point, patch, ROT, field, rows, lattice)
        assert np.array_equal(got[0], got[32768])
        want = R.patch_augment_clip_minmax([v[n] for n in names], v["holes"], point, patch, ROT, field, rows, lattice, *cols)
        assert got[0].dtype == want.dtype == F and np.array_equal(got[0], want), (float(np.abs(got[0] - want).max()),
                                                                                    int((got[0] != want).sum()))
        assert got[0].min() >= -1.0 and got[0].max() <= 1.0
        today = _geo(hip_ops, dev_vols, dev_mask, names, point, patch, ROT, field)
        assert not np.array_equal(got[0][0], today[0])
        if len(names) == 3:
            assert np.array_equal(got[0][1], today[1])
        for lat in (None, lattice):                              # all rows neutral, with and without a lattice nobody reads
            neutral, _ = _aug(hip_ops, dev_vols, dev_mask, names, point, patch, ROT, field, [R.NEUTRAL] * len(names), lat)
            assert np.array_equal(neutral, today)


@pytest.mark.parametrize("name", ["ct", "pet"])                  # int16, fp32
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("shape,patch", CASES)
def test_zscore_entry_equals_the_loop_reference(hip_ops, shape, patch, grid, name):
    v = _case(shape, 11)
    vol = _dev(v[name], hip_ops.device)
    lattice = R.random_lattice(grid, 42)
    start = A.start_of(_point(shape), list(patch), shape)
    t = _t(hip_ops, vol, start, patch)
    for row, lat in ((EXACT_ROWS[0], lattice), (EXACT_ROWS[2], lattice), ((1.0, 1.1, 0.02, 0.0, 0.0, 0, 0), None)):
        for scale in ((-1.0, 1.0), (0.0, 1.0)):
            got = _zs(hip_ops, vol, start, patch, row, lat, scale)
            want = R.patch_zscore_intensity(t, row, lat, *scale)
            assert np.array_equal(got, want), (row, scale, float(np.abs(got - want).max()), int((got != want).sum()))
    unit = _zs(hip_ops, vol, start, patch, R.NEUTRAL, None, (0.0, 1.0))          # the entry's own n, bit for bit
    assert np.array_equal(unit, R.zscore_units(t))


# ---- gamma and noise --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [0.5, 0.7, 1.5, 2.2])
def test_gamma_in_ulps_of_float64_pow(hip_ops, gamma):
    """worst case seen on the MI355X over the four gammas: 1.128 ulps (GAMMA_SEEN); asserted at twice that, 2.256, under
    the cap of 16"""
    shape, patch = CASES[2]
    v = _case(shape, 12)
    vol = _dev(v["pet"], hip_ops.device)
    lattice = R.random_lattice(GRIDS[1], 43)
    start = A.start_of(_point(shape), list(patch), shape)
    n = R.zscore_units(_t(hip_ops, vol, start, patch))
    row = (gamma, 1.2, -0.05, 0.0, 0.3, 0, 0)
    got = _zs(hip_ops, vol, start, patch, row, lattice, (0.0, 1.0)).astype(np.float64)
    want, powed = R.chain64(n, row, R.beta(patch, lattice), 0)
    ulps = np.abs(got - want) / np.spacing(np.abs(want).astype(F)).astype(np.float64)
    print(f"gamma {gamma}: worst {float(ulps.max()):.3f} ulps over {ulps.size} voxels, values in [{want.min():.3g}, {want.max():.3g}]")
    assert (want > 0).sum() > 1000 and (want < 1).sum() > 1000
    assert float(ulps.max()) <= GAMMA_ULPS
    # the clip entry: the same step in front of 2 n - 1
    names = ("pet", "ct")
    dev_vols, dev_mask = [_dev(v[k], hip_ops.device) for k in names], _dev(v["holes"], hip_ops.device)
    rows = [row, (gamma, 1.0, 0.0, 0.0, 0.0, 0, 0)]
    out, cols = _aug(hip_ops, dev_vols, dev_mask, names, _point(shape), patch, ROT, None, rows, lattice)
    units = R.units([v[k] for k in names], v["holes"], _point(shape), patch, ROT, None, *cols)
    for c in range(2):
        want, powed = R.chain64(units[c], rows[c], R.beta(patch, lattice), c)
        bound = 2.0 * R.gamma_noise_bound(powed, rows[c], GAMMA_ULPS) + 2.0 ** -24
        assert (np.abs(out[c].astype(np.float64) - (2.0 * want - 1.0)) <= bound).all(), c


@pytest.mark.parametrize("noise_std", [0.05, 0.1])
def test_noise_against_the_reference_plane(hip_ops, noise_std):
    shape, patch = CASES[1]
    v = _case(shape, 13)
    vol = _dev(v["pet"], hip_ops.device)
    start = A.start_of(_point(shape), list(patch), shape)
    n = R.zscore_units(_t(hip_ops, vol, start, patch))
    row = (1.0, 0.6, 0.0, noise_std, 0.0, 123456789, 987654321)              # contrast 0.6: few voxels reach the clamps
    got = _zs(hip_ops, vol, start, patch, row, None, (0.0, 1.0)).astype(np.float64)
    want, _ = R.chain64(n, row, None, 0)
    err = float(np.abs(got - want).max())
    print(f"noise_std {noise_std}: worst {err:.3g} on n, bound {8e-6 * noise_std:.3g}")
    assert err <= 8e-6 * noise_std
    quiet = _zs(hip_ops, vol, start, patch, (1.0, 0.6, 0.0, 0.0, 0.0, 0, 0), None, (0.0, 1.0)).astype(np.float64)
    free = (got > 0) & (got < 1)
    z = (got - quiet)[free] / noise_std
    assert free.mean() > 0.9 and abs(z.mean()) <= 4.0 / np.sqrt(z.size) + 0.05 and abs(z.std() - 1.0) <= 0.1
    # the clip entry: channel c enters the counter, the same key gives another plane per channel; doubled by 2 n - 1
    names = ("pet", "ct", "hx4")
    dev_vols, dev_mask = [_dev(v[k], hip_ops.device) for k in names], _dev(v["holes"], hip_ops.device)
    rows = [row, R.NEUTRAL, row]
    out, cols = _aug(hip_ops, dev_vols, dev_mask, names, _point(shape), patch, ROT, None, rows, None)
    units = R.units([v[k] for k in names], v["holes"], _point(shape), patch, ROT, None, *cols)
    for c in (0, 2):
        want, _ = R.chain64(units[c], rows[c], None, c)
        assert float(np.abs(out[c].astype(np.float64) - (2.0 * want - 1.0)).max()) <= 2.0 * 8e-6 * noise_std, c
    again, _ = _aug(hip_ops, dev_vols, dev_mask, names, _point(shape), patch, ROT, None, rows, None)
    assert np.array_equal(out, again)                                          # the same key: the same bits
    other, _ = _aug(hip_ops, dev_vols, dev_mask, names, _point(shape), patch, ROT, None, [row[:5] + (5, 6), R.NEUTRAL, row], None)
    assert not np.array_equal(out[0], other[0]) and np.array_equal(out[1:], other[1:])


# ---- NaN ------------------------------------------------------------------------------------------------------------------
def test_nan_handling(hip_ops):
    shape, patch = CASES[2]
    grid = GRIDS[1]
    v = _case(shape, 14)
    dev = hip_ops.device
    clean = R.random_lattice(grid, 44)
    js = [[E.axis_weights(o, patch[a], grid[a])[0] for o in range(patch[a])] for a in range(3)]
    at = tuple(js[a][patch[a] // 2] for a in range(3))           # the first control point the middle voxel reads
    bad = clean.copy()
    bad[at] = np.nan
    reads = [np.array([j <= at[a] <= j + 3 for j in js[a]]) for a in range(3)]
    support = reads[0][:, None, None] & reads[1][None, :, None] & reads[2][None, None, :]
    assert support.any() and not support.all()
    names = ("pet", "ct")
    dev_vols, dev_mask = [_dev(v[n], dev) for n in names], _dev(v["holes"], dev)
    rows = [EXACT_ROWS[0], R.NEUTRAL]
    for option in (0, 32768):
        with hip_ops.options(elastic_rows=option):
            one, _ = _aug(hip_ops, dev_vols, dev_mask, names, _point(shape), patch, ROT, None, rows, bad, finite=False)
            two, _ = _aug(hip_ops, dev_vols, dev_mask, names, _point(shape), patch, ROT, None, rows, clean)
        assert np.array_equal(np.isnan(one[0]), support) and np.isfinite(one[1]).all()
        assert np.array_equal(one[0][~support], two[0][~support]) and np.array_equal(one[1], two[1])
    vol = _dev(v["pet"], dev)
    start = A.start_of(_point(shape), list(patch), shape)
    z = _zs(hip_ops, vol, start, patch, EXACT_ROWS[0], bad, finite=False)
    assert np.array_equal(np.isnan(z), support)
    assert np.array_equal(z[~support], _zs(hip_ops, vol, start, patch, EXACT_ROWS[0], clean)[~support])
    const = torch.full(shape, 3.0, device=dev)                   # a constant patch: NaN, as in gs_patch_zscore
    assert np.isnan(_zs(hip_ops, const, start, patch, EXACT_ROWS[0], clean, finite=False)).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(hip_ops):
    from ganslate_amd.hip import lib as L
    dev = hip_ops.device
    v = _case((9, 17, 13))
    mask, pet, ct = _dev(v["holes"], dev), _dev(v["pet"], dev), _dev(v["ct"], dev)
    pt = torch.tensor([4, 8, 6, 0], dtype=torch.int32, device=dev)
    buf, out = _poisoned(105, (1, 3, 5, 7), dev)
    lat = lambda *g: torch.zeros(g, dtype=torch.float64, device=dev)
    field = lambda *g: torch.zeros((3, *g), dtype=torch.float64, device=dev)
    ok = (1.0, 1.0, 0.0, 0.0, 0.5, 0, 0)
    one = lambda **k: hip_ops.patch_augment_clip_minmax([pet], mask, pt, k.get("patch", (3, 5, 7)), k.get("M", np.eye(3)),
                                                        k.get("field", None), [k.get("row", ok)], k.get("lat", lat(4, 4, 4)),
                                                        [0.0], [k.get("div", 1.0)], [k.get("lo", 0.0)], [6.0], k.get("out", out))
    zs = lambda **k: hip_ops.patch_zscore_intensity(ct, k.get("start", (1, 2, 3)), k.get("patch", (3, 5, 7)), k.get("out", out[0]),
                                                    k.get("row", ok), k.get("lat", lat(4, 4, 4)))
    nan, inf = float("nan"), float("inf")
    for fn in (one, zs):
        for row, match in [((0.0,) + ok[1:], "gamma"), ((-1.0,) + ok[1:], "gamma"), ((inf,) + ok[1:], "gamma"),
                           ((nan,) + ok[1:], "gamma"), ((1.0, -0.5) + ok[2:], "contrast"), ((1.0, inf) + ok[2:], "contrast"),
                           ((1.0, nan) + ok[2:], "contrast"), ((1.0, 1.0, inf) + ok[3:], "brightness"),
                           ((1.0, 1.0, nan) + ok[3:], "brightness"), ((1.0, 1.0, 0.0, -0.1) + ok[4:], "noise_std"),
                           ((1.0, 1.0, 0.0, inf) + ok[4:], "noise_std"), ((1.0, 1.0, 0.0, nan) + ok[4:], "noise_std"),
                           ((1.0, 1.0, 0.0, 0.0, 1.0, 0, 0), "bias"), ((1.0, 1.0, 0.0, 0.0, -1.0, 0, 0), "bias"),
                           ((1.0, 1.0, 0.0, 0.0, nan, 0, 0), "bias")]:
            with pytest.raises(L.HipError, match=match + ".*of intensity 0"):
                fn(row=row)
        with pytest.raises(L.HipError, match="a non-zero bias needs bias_grid and bias_field"):
            fn(lat=None)
        for g in ((3, 4, 4), (4, 3, 4), (4, 4, 3)):
            with pytest.raises(L.HipError, match="bias_grid lattice needs at least 4 control points per axis"):
                fn(lat=lat(*g))
        for g in ((11, 10, 10), (4, 4, 65)):
            with pytest.raises(L.HipError, match="bias_grid lattice of .* exceeds 1024"):
                fn(lat=lat(*g))
        for patch in ((1, 5, 7), (3, 1, 7), (3, 5, 1)):
            small = torch.full((1, *patch) if fn is one else patch, 5.0, device=dev)
            with pytest.raises(L.HipError, match="bias_grid lattice needs at least 2 voxels per axis"):
                fn(patch=patch, out=small)
            torch.cuda.synchronize()
            assert bool((small == 5.0).all())
        for wrong in (lat(4, 4, 4).float(), lat(4, 4, 4).cpu(), lat(4, 4, 8)[..., ::2], field(4, 4, 4), np.zeros((4, 4, 4))):
            with pytest.raises(ValueError, match="bias_lattice"):
                fn(lat=wrong)
        with pytest.raises(ValueError, match="intensity"):
            fn(row=ok[:6])
    # what the base entries refuse
    bad = np.eye(3)
    bad[1, 2] = nan
    with pytest.raises(L.HipError, match="non-finite"):
        one(M=bad)
    with pytest.raises(L.HipError, match="does not fit"):
        one(patch=(3, 18, 7), out=torch.full((1, 3, 18, 7), 5.0, device=dev))
    with pytest.raises(L.HipError, match="clip range"):
        one(lo=6.0)
    with pytest.raises(L.HipError, match="divisor"):
        one(div=0.0)
    with pytest.raises(L.HipError, match="at least 4 control points per axis"):
        one(field=field(3, 4, 4))
    with pytest.raises(L.HipError, match="outside the 9 x 17 x 13 volume"):
        zs(start=(7, 2, 3))
    # straight at the C entry points: null arguments
    lib = hip_ops.lib
    fl = lambda x: (C.c_float * 1)(x)
    eye = (C.c_double * 9)(*np.eye(3).reshape(9))
    table = (L.PatchIntensity * 1)()
    table[0].gamma, table[0].contrast, table[0].bias = 1.0, 1.0, 0.5
    bz, fz = lat(4, 4, 4), field(4, 4, 4)
    base = dict(vols=(C.c_void_p * 1)(pet.data_ptr()), dtypes=(C.c_int32 * 1)(0), C=1, mask=mask.data_ptr(), D=9, H=17, W=13,
                point=pt.data_ptr(), patch=_i3((3, 5, 7)), M=eye, grid=None, field=None, intensity=table, bias_grid=_i3((4, 4, 4)),
                bias_field=bz.data_ptr(), outside=fl(0.0), divisor=fl(1.0), lo=fl(0.0), hi=fl(6.0), out=out.data_ptr(),
                stream=None)
    call = lambda **k: L.check(lib.gs_patch_augment_clip_minmax(*{**base, **k}.values()), "gs_patch_augment_clip_minmax")
    ws = torch.empty(int(lib.gs_patch_zscore_ws_floats()), device=dev)
    zbase = dict(vol=ct.data_ptr(), dtype=1, D=9, H=17, W=13, start=_i3((1, 2, 3)), size=_i3((3, 5, 7)), lo=C.c_float(-1.0),
                 hi=C.c_float(1.0), intensity=table, bias_grid=_i3((4, 4, 4)), bias_field=bz.data_ptr(), out=out.data_ptr(),
                 scratch=ws.data_ptr(), stream=None)
    zcall = lambda **k: L.check(lib.gs_patch_zscore_intensity(*{**zbase, **k}.values()), "gs_patch_zscore_intensity")
    for fn in (call, zcall):
        with pytest.raises(L.HipError, match="null intensity"):
            fn(intensity=None)
        for k in (dict(bias_grid=None), dict(bias_field=None), dict(bias_grid=None, bias_field=None)):
            with pytest.raises(L.HipError, match="a non-zero bias needs bias_grid and bias_field"):
                fn(**k)
    for k in (dict(grid=_i3((4, 4, 4))), dict(field=fz.data_ptr())):
        with pytest.raises(L.HipError, match="grid and field come together"):
            call(**k)
    for name in ("vols", "dtypes", "mask", "point", "patch", "M", "outside", "divisor", "lo", "hi", "out"):
        with pytest.raises(L.HipError, match="null argument"):
            call(**{name: None})
    for name in ("vol", "start", "size", "out", "scratch"):
        with pytest.raises(L.HipError, match="null argument"):
            zcall(**{name: None})
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())                          # nothing was launched on the shared output
    call()                                                       # the unmodified argument sets are valid ones
    call(grid=_i3((4, 4, 4)), field=fz.data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and _untouched(buf, 105)
    out.fill_(nan)
    zcall()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and _untouched(buf, 105)


# ---- pipelines, Trainer ---------------------------------------------------------------------------------------------------
GEO = dict(prob=1.0, flip=[True, True, True], rotate_deg=[12.0, 6.0, 6.0], scale=[0.9, 1.15], spacing=[3.0, 1.0, 1.0])
ELASTIC = dict(prob=0.6, control_points=[4, 5, 4], max_displacement=[2.0, 1.5, 2.0])


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("paired,scheme", [(True, "fdg-pet-weighted"), (False, "uniform-random-within-body-sf")])
def test_multimodal_pipeline_equals_the_host_dataset_path(hip_ops, tmp_path, paired, scheme, exact):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.device_volumes import DeviceMultiModalPipeline
    from ganslate_amd.data.utils.patch_intensity import active
    div = toy_folder(tmp_path / "data")
    aug = dict(GEO, elastic=ELASTIC, intensity=dict(EXACT if exact else INTENSITY, prob=0.7))
    mk = lambda dt: _with_aug(dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16), divisors=div, device_transforms=dt),
                              aug)
    host, raw = MultiModalVolumeDataset(mk(False)), MultiModalVolumeDataset(mk(True))
    pipe = DeviceMultiModalPipeline(raw, hip_ops.device, ops=hip_ops)
    random.seed(21)
    np.random.seed(21)
    want = [host[i] for i in range(4)]
    runs = []
    for _ in range(2):
        random.seed(21)
        np.random.seed(21)
        samples = [raw[i] for i in range(4)]
        on = [active(s[k].intensity) is not None for s in samples for k in "AB"]
        assert any(on) and any(s[k].field is not None for s in samples for k in "AB")
        runs.append({k: t.cpu() for k, t in pipe(raw.collate_fn(samples)).items()})
    for key in "AB":
        ref = torch.stack([w[key] for w in want])
        assert runs[0][key].shape == ref.shape and runs[0][key].dtype == torch.float32
        worst = float((runs[0][key] - ref).abs().max())
        if exact:
            assert np.array_equal(runs[0][key].numpy(), ref.numpy()), (key, worst)
        else:
            assert worst <= PIPE_BOUND, (key, worst)
        assert np.array_equal(runs[0][key].numpy(), runs[1][key].numpy())          # one seed, identical batches


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_volume_pipeline_equals_the_host_dataset_path(hip_ops, tmp_path, dtype, exact):
    from ganslate_amd.data.device_volumes import DeviceVolumePipeline
    from ganslate_amd.data.utils.patch_intensity import active
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset, collate_raw
    root = _volume_folder(tmp_path, dtype)
    aug = dict(GEO, fill=-5.0, elastic=ELASTIC, intensity=dict(EXACT if exact else INTENSITY, prob=0.7))
    host = UnpairedVolumeDataset(_with_aug(vol_conf(root, False), aug))
    raw = UnpairedVolumeDataset(_with_aug(vol_conf(root, True), aug))
    pipe = DeviceVolumePipeline(raw, hip_ops.device, ops=hip_ops)
    random.seed(21)
    np.random.seed(21)
    want = [host[i] for i in range(4)]
    runs = []
    for _ in range(2):
        random.seed(21)
        np.random.seed(21)
        samples = [raw[i] for i in range(4)]
        on = [active(s[k].intensity) is not None for s in samples for k in "AB"]
        assert any(on) and not all(on)                            # both apply kernels run in this batch
        runs.append({k: t.cpu() for k, t in pipe(collate_raw(samples)).items()})
    # 2e-6 is what the plain z-score pipeline is given; the chain stretches n's share of it by contrast * (1 + max) at most
    bound = 2e-6 * 1.25 * 1.3 + (0.0 if exact else PIPE_BOUND)
    for key in "AB":
        ref = torch.stack([w[key] for w in want])
        assert runs[0][key].shape == ref.shape == (4, 1, 8, 16, 16)
        worst = float((runs[0][key] - ref).abs().max())
        assert worst <= bound, (key, worst, bound)
        assert torch.equal(runs[0][key], runs[1][key])


def test_trainer_runs_on_intensity_device_batches(hip_ops, tmp_path):
    """two iterations of the paired 3-D Pix2Pix recipe on tests/configs/pix2pix3d_mmvol_intensity.yaml (intensity on A's
    modalities only) against the same seed on tests/configs/pix2pix3d_mmvol.yaml: finite losses, batches in [-1, 1], A's
    batches differ, B's — the target — are the plain crop of the same points bit for bit"""
    from ganslate_amd.engines import init_engine
    div = toy_folder(tmp_path / "data", shape=(36, 40, 38), shape_B=(34, 44, 40))
    args = [f"train.output_dir={tmp_path / 'out'}", f"train.dataset.root={tmp_path / 'data'}", f"train.dataset.divisors={div}",
            "train.seed=5", "train.n_iters=2", "train.dataset.device_transforms=True"]
    runs = {}
    for key, conf in (("intensity", "pix2pix3d_mmvol_intensity"), ("plain", "pix2pix3d_mmvol")):
        extra = [] if key == "intensity" else ["train.dataset.augmentation={flip: [false, false, false]}"]
        trainer = init_engine("train", [f"config=tests/configs/{conf}.yaml"] + args + extra)
        seen = []
        orig = trainer.model.set_input
        trainer.model.set_input = lambda data, _o=orig, _s=seen: (_s.append({k: v.detach().float().cpu().clone()
                                                                           for k, v in data.items()}), _o(data))[1]
        trainer.run()
        assert trainer.input_pipeline is not None
        assert all(bool(torch.isfinite(v.detach()).all()) for v in trainer.model.losses.values() if v is not None)
        runs[key] = seen
    assert len(runs["intensity"]) == len(runs["plain"]) == 2
    a, b = runs["intensity"][0], runs["plain"][0]                 # the first batch: the streams part after it
    for k, ch in (("A", 2), ("B", 1)):
        assert a[k].shape == b[k].shape == (2, ch, 32, 32, 32)
        for run in runs["intensity"]:
            assert bool(torch.isfinite(run[k]).all()) and float(run[k].min()) >= -1.0 and float(run[k].max()) <= 1.0
    assert not torch.equal(a["A"], b["A"])
    assert torch.equal(a["B"][0], b["B"][0])                      # sample 0 of batch 0: the same focal point and matrix
