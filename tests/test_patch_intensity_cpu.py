"""Intensity augmentation of 3-D training patches on the host (ganslate_amd/data/utils/patch_intensity.py and the two volume
datasets): the vectorised numpy chain against the per-voxel loop of tests/patch_intensity_ref.py — equal bits for the bias,
contrast / brightness and clamp steps, and against the float64 restatement within a stated bound once gamma and noise are
on —, neutral rows against today's paths, the skip rules, the parser, the consumption of np.random (7 C uniforms per
domain, + 1 + G_0 G_1 G_2 with a bias field), the noise plane's moments, and the descriptor's layout.

Bounds with gamma and noise on (tests/patch_intensity_ref.py gamma_noise_bound): the float64 restatement takes the float32
value in front of the gamma step, so what is left is pow's own error — np.power on float32 is glibc's powf, documented
within 1 ulp; with the rounding of the float64 result to float32 that is HOST_POW_ULPS = 2 — and, with noise, 8e-6 *
noise_std for the float32 Box-Muller value plus one ulp of a value below 2 for the multiply and for the add."""
import ctypes
import random
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import patch_affine_ref as A
from tests import patch_intensity_ref as R
from tests.mmvol_ref import synthetic_case
from tests.test_mmvol_cpu import _D, dataset_conf, toy_folder
from tests.test_patch_elastic_cpu import _np_state, _uniform_after, with_aug
from tests.test_volume_patches_cpu import _conf as vol_conf
from tests.test_volume_patches_cpu import _volume_folder

F = np.float32
HOST_POW_ULPS = 2
INTENSITY = dict(prob=1.0, gamma=[0.7, 1.5], contrast=[0.75, 1.25], brightness=[-0.1, 0.1], noise_std=[0.0, 0.05],
                 bias_field=dict(prob=1.0, control_points=[4, 5, 4], max=0.3))
EXACT = dict(prob=1.0, contrast=[0.75, 1.25], brightness=[-0.1, 0.1],
             bias_field=dict(prob=1.0, control_points=[4, 5, 4], max=0.3))       # gamma 1, no noise: every step exact
N_LATTICE = 1 + 4 * 5 * 4
ROWS = [(1.0, 1.2, -0.05, 0.0, 0.3, 0, 0), (1.0, 0.8, 0.3, 0.0, 0.0, 0, 0), (1.0, 1.0, 0.0, 0.0, -0.95, 0, 0),
        (1.0, 0.0, 0.0, 0.0, 0.2, 0, 0), (1.0, 2.5, -0.4, 0.0, 0.999, 0, 0)]


def _vol_root(tmp_path):
    (tmp_path / "vol").mkdir()
    return _volume_folder(tmp_path / "vol")


def _units(patch, seed):
    """n of a patch: uniform values with exact 0s and 1s, tiny values and a NaN"""
    n = np.random.default_rng(seed).random(patch).astype(F)
    flat = n.reshape(-1)
    flat[:6] = [0.0, 1.0, 1e-9, 0.5, 1.0 - 2.0 ** -24, np.nan]
    return n


# ---- the chain ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(4, 4, 4), (5, 7, 9)])
@pytest.mark.parametrize("patch", [(3, 5, 7), (8, 16, 16)])
def test_host_chain_equals_the_loop_reference(patch, grid):
    from ganslate_amd.data.utils.patch_intensity import apply, bias_field
    lattice = R.random_lattice(grid, 31)
    beta = bias_field(patch, lattice)
    want_beta = np.array(R.beta(patch, lattice)).reshape(patch)
    assert beta.dtype == np.float64 and np.array_equal(beta, want_beta) and np.abs(beta).max() <= 1.0
    n = _units(patch, 32)
    for row in ROWS:
        got = apply(n, row, beta, 1)
        want = R.chain(n, row, want_beta.reshape(-1), 1)
        assert got.dtype == want.dtype == F and np.array_equal(got, want, equal_nan=True), row
        assert np.isnan(got.reshape(-1)[5]) and np.isnan(got).sum() == 1
        assert np.nanmin(got) >= 0.0 and np.nanmax(got) <= 1.0
    # gamma and noise on: against the float64 restatement
    clean = np.nan_to_num(n, nan=0.25)
    for row in [(0.7, 1.2, -0.05, 0.05, 0.3, 5, 6), (1.5, 1.0, 0.0, 0.0, 0.0, 0, 0), (2.0, 0.9, 0.02, 0.02, -0.2, 1, 2),
                (1.0, 1.0, 0.0, 0.03, 0.0, 123456789, 987654321)]:
        got = apply(clean, row, beta, 2).astype(np.float64)
        want, powed = R.chain64(clean, row, want_beta.reshape(-1), 2)
        err = np.abs(got - want)
        assert (err <= R.gamma_noise_bound(powed, row, HOST_POW_ULPS)).all(), (row, float(err.max()))


def test_neutral_rows_give_todays_bits(tmp_path):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.utils.normalization import z_score_normalize
    from ganslate_amd.data.utils.patch_intensity import NEUTRAL, active, apply, is_neutral
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset
    n = _units((3, 5, 7), 33)
    assert is_neutral(NEUTRAL) and active(((NEUTRAL, NEUTRAL), None)) is None
    assert np.array_equal(apply(n, NEUTRAL), n, equal_nan=True)                     # the clamps change no bit in [0, 1]
    # multi-modal: prob 0 switches every modality off; the host path is then today's sample_patch + normalize
    div = toy_folder(tmp_path / "data")
    mk = lambda aug: MultiModalVolumeDataset(with_aug(dataset_conf(tmp_path / "data", True, "fdg-pet-weighted", (8, 16, 16),
                                                                   divisors=div), aug))
    out = []
    for ds in (mk(dict(flip=[False] * 3)), mk(dict(flip=[False] * 3, intensity=dict(INTENSITY, prob=0.0,
                                                                                      bias_field=None)))):
        random.seed(5)
        np.random.seed(5)
        out.append(ds[1])
    assert all(torch.equal(out[0][k], out[1][k]) for k in "AB")
    plain = mk(None)
    random.seed(5)
    np.random.seed(5)
    crop = plain[1]
    assert all(torch.equal(out[0][k], crop[k]) for k in "AB")                       # M = I: the plain crop, bit for bit
    # z-score: a neutral row takes z_score_normalize itself
    root = _vol_root(tmp_path)
    ds = UnpairedVolumeDataset(with_aug(vol_conf(root, False), dict(intensity=dict(INTENSITY, prob=0.0))))
    patch = torch.from_numpy(np.random.default_rng(3).random((8, 16, 16)).astype(F))
    assert torch.equal(ds.normalize(patch, ((NEUTRAL,), None)), z_score_normalize(patch, scale_to_range=(-1, 1)))
    assert torch.equal(ds.normalize(patch, None), z_score_normalize(patch, scale_to_range=(-1, 1)))


def test_skip_rules():
    from ganslate_amd.data.utils.patch_intensity import apply
    tiny = np.array([1e-9, 3e-8, 0.0, 1.0], F)
    assert F(F(tiny[0] - F(0.5)) + F(0.5)) != tiny[0]                               # evaluated, the step would change it
    for row in [(1.0, 1.0, 0.0, 0.0, 0.0, 7, 8), (1.0, 1.0, 0.0, 0.0, 0.0, 0, 0)]:
        assert np.array_equal(apply(tiny, row), tiny)
        assert np.array_equal(R.chain(tiny, row), tiny)
    moved = apply(tiny, (1.0, 1.0, 0.25, 0.0, 0.0, 0, 0))
    assert np.array_equal(moved, R.chain(tiny, (1.0, 1.0, 0.25, 0.0, 0.0, 0, 0))) and moved[0] == F(0.25) and moved[3] == 1
    assert np.array_equal(apply(tiny, (1.0, 1.0, 0.0, 0.0, 0.5, 0, 0), np.zeros(4)), tiny)      # beta = 0: m = 1
    # a NaN lattice entry: NaN inside its support, nothing outside
    from ganslate_amd.data.utils.patch_intensity import bias_field
    lattice = R.random_lattice((5, 7, 9), 4)
    bad = lattice.copy()
    bad[0, 0, 0] = np.nan
    b0, b1 = bias_field((8, 16, 16), lattice), bias_field((8, 16, 16), bad)
    assert np.isnan(b1).any() and not np.isnan(b1).all() and np.array_equal(b0[~np.isnan(b1)], b1[~np.isnan(b1)])
    n = np.full((8, 16, 16), 0.5, F)
    out = apply(n, (1.0, 1.0, 0.0, 0.0, 0.3, 0, 0), b1)
    assert np.array_equal(np.isnan(out), np.isnan(b1))


# ---- the parser -----------------------------------------------------------------------------------------------------------
def test_parser_defaults_null_and_refusals(tmp_path):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.utils.patch_affine import parse_augmentation
    from ganslate_amd.data.utils.patch_intensity import BiasField, IntensityAugmentation, parse_intensity
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset
    assert parse_intensity(None) is None
    assert parse_augmentation(dict(intensity=None), True).intensity is None
    assert parse_augmentation(dict(flip=[True, False, False]), True).intensity is None
    d = parse_augmentation(dict(intensity={}), False)
    assert d.intensity == IntensityAugmentation() and d.intensity.uniforms(3) == 21
    assert (d.prob, d.flip, d.rotate_deg, d.scale) == (1.0, (False, False, False), (0.0, 0.0, 0.0), (1.0, 1.0))
    full = parse_intensity(dict(INTENSITY, modalities=["pet"]))
    assert full.bias_field == BiasField(1.0, (4, 5, 4), 0.3) and full.modalities == ("pet",)
    assert full.uniforms(2) == 14 + N_LATTICE and full.gamma == (0.7, 1.5)
    assert parse_intensity(dict(bias_field={})).bias_field == BiasField(1.0, (4, 4, 4), 0.3)
    bad = [(dict(gama=[1, 1]), "unknown keys"), (dict(gamma=[0.0, 1.0]), "gamma needs 0 < lo"),
           (dict(gamma=[-1.0, 1.0]), "gamma needs 0 < lo"), (dict(gamma=[1.5, 1.0]), "gamma needs lo <= hi"),
           (dict(gamma=[]), "gamma"), (dict(gamma=[1.0]), "gamma"), (dict(gamma=2.0), "gamma"),
           (dict(contrast=[-0.1, 1.0]), "contrast needs 0 <= lo"), (dict(contrast=[2.0, 1.0]), "contrast needs lo <= hi"),
           (dict(brightness=[0.1, -0.1]), "brightness needs lo <= hi"), (dict(brightness=[0.0, float("inf")]), "finite"),
           (dict(noise_std=[-0.01, 0.1]), "noise_std needs 0 <= lo"), (dict(noise_std=[0.2, 0.1]), "noise_std needs lo <= hi"),
           (dict(prob=1.5), r"prob must lie in \[0, 1\]"), (dict(modalities=[]), "modalities"),
           (dict(bias_field=dict(maximum=0.3)), "bias_field: unknown keys"), (dict(bias_field=dict(max=1.0)), r"\[0, 1\)"),
           (dict(bias_field=dict(max=-0.1)), r"\[0, 1\)"), (dict(bias_field=dict(prob=-0.5)), "bias_field.prob"),
           (dict(bias_field=dict(control_points=[3, 4, 4])), "at least 4 per axis"),
           (dict(bias_field=dict(control_points=[4, 4])), "three integers"),
           (dict(bias_field=dict(control_points=[11, 10, 10])), "at most 1024")]
    for node, match in bad:
        with pytest.raises(ValueError, match=match):
            parse_intensity(node)
    # at construction: names and the patch
    div = toy_folder(tmp_path / "data")
    mm = lambda patch, node: MultiModalVolumeDataset(with_aug(dataset_conf(tmp_path / "data", True, "fdg-pet-weighted", patch,
                                                                           divisors=div), dict(intensity=node)))
    assert mm((8, 16, 16), dict(modalities=["pet", "hx4"])).augmentation.intensity.modalities == ("pet", "hx4")
    with pytest.raises(ValueError, match=r"modalities: \['mri'\] not among"):
        mm((8, 16, 16), dict(modalities=["pet", "mri"]))
    with pytest.raises(ValueError, match="at least 2 voxels per axis"):
        mm((1, 16, 16), dict(bias_field={}))
    mm((1, 16, 16), dict(gamma=[0.5, 2.0]))                                         # without a lattice any patch will do
    root = _vol_root(tmp_path)
    vol = lambda node: UnpairedVolumeDataset(with_aug(vol_conf(root, False), dict(intensity=node)))
    assert vol(dict(modalities=["B"])).augmentation.intensity.modalities == ("B",)
    with pytest.raises(ValueError, match="not among"):
        vol(dict(modalities=["pet"]))


# ---- the draws ------------------------------------------------------------------------------------------------------------
def test_draw_block_follows_the_definition():
    from ganslate_amd.data.utils.patch_intensity import NEUTRAL, draw_block, parse_intensity
    cfg = parse_intensity(dict(INTENSITY, modalities=["pet", "hx4"]))
    names = ("pet", "ct", "hx4")
    np.random.seed(3)
    us = [float(np.random.random_sample()) for _ in range(21 + N_LATTICE)]
    np.random.seed(3)
    rows, lattice = draw_block(cfg, names)
    assert float(np.random.random_sample()) == _uniform_after(3, 21 + N_LATTICE)
    assert lattice.dtype == np.float64 and lattice.shape == (4, 5, 4)
    assert np.array_equal(lattice, np.array([2.0 * u - 1.0 for u in us[22:]]).reshape(4, 5, 4))
    assert rows[1] == NEUTRAL                                                        # not listed: neutral, its draws taken
    for c in (0, 2):
        u = us[7 * c:7 * c + 7]
        want = [F(lo + v * (hi - lo)) for (lo, hi), v in zip((cfg.gamma, cfg.contrast, cfg.brightness, cfg.noise_std), u[1:5])]
        assert rows[c][:4] == tuple(float(w) for w in want) and rows[c][4] == float(F(0.3))
        assert rows[c][5:] == (int(u[5] * 2 ** 32), int(u[6] * 2 ** 32))
    # switched off: all draws still taken, neutral rows, and a lattice nobody reads does not travel
    for node in (dict(INTENSITY, prob=0.0), dict(INTENSITY, bias_field=dict(INTENSITY["bias_field"], prob=0.0))):
        np.random.seed(3)
        rows, lattice = draw_block(parse_intensity(node), names)
        assert lattice is None and all(r[4] == 0.0 for r in rows)
        assert float(np.random.random_sample()) == _uniform_after(3, 21 + N_LATTICE)
    assert all(r == NEUTRAL for r in rows) is False and rows[0][0] != 1.0            # lattice off: the rest stays on
    np.random.seed(3)
    rows, _ = draw_block(parse_intensity(dict(INTENSITY, prob=us[0])), names)        # u < prob is strict
    assert rows[0] == NEUTRAL
    np.random.seed(3)
    draw_block(parse_intensity(dict(INTENSITY, bias_field=None)), names)
    assert float(np.random.random_sample()) == _uniform_after(3, 21)


@pytest.mark.parametrize("paired,scheme", [(True, "fdg-pet-weighted"), (False, "uniform-random-within-body-sf")])
@pytest.mark.parametrize("device_transforms", [False, True])
def test_multimodal_streams(tmp_path, paired, scheme, device_transforms):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.utils.patch_affine import draw_set, matrix_tuple
    from ganslate_amd.data.utils.patch_intensity import draw_block
    div = toy_folder(tmp_path / "data")
    mk = lambda aug: MultiModalVolumeDataset(with_aug(dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16), divisors=div,
                                                                   device_transforms=device_transforms), aug))
    geo = dict(prob=1.0, flip=[True, True, True], rotate_deg=[12.0, 6.0, 6.0], scale=[0.9, 1.15], spacing=[3.0, 1.0, 1.0])
    affine, null, both = mk(geo), mk(dict(geo, intensity=None)), mk(dict(geo, intensity=INTENSITY))
    states = []
    for ds in (affine, null):
        random.seed(4)
        np.random.seed(4)
        out = ds[0]
        states.append((random.getstate(), _np_state()))
        assert device_transforms is False or (out["A"].intensity is None and out["B"].intensity is None)
    assert states[0] == states[1]                          # `intensity: null` draws nothing extra
    draws = 1 if paired else 2
    random.seed(4)
    np.random.seed(4)
    s = both[0]
    assert random.getstate() == states[0][0]               # `random` is not touched
    n_B = len(both.modalities["B"])
    blocks = (7 * 2 + N_LATTICE) + (7 * n_B + N_LATTICE)   # A has two modalities, B one (paired) or two
    assert float(np.random.random_sample()) == _uniform_after(4, draws + 8 * draws + blocks)
    if device_transforms:
        np.random.seed(4)
        for _ in range(draws):
            np.random.random_sample()
        cfg = both.augmentation
        M, _ = draw_set(cfg)                               # paired: the shared set, A's block, B's block
        assert s["A"].matrix == matrix_tuple(M)
        rows, lattice = draw_block(cfg.intensity, both.modalities["A"])
        assert s["A"].intensity[0] == rows and np.array_equal(s["A"].intensity[1], lattice) and len(rows) == 2
        if not paired:                                     # unpaired: A's set, A's block, B's set, B's block
            M, _ = draw_set(cfg)
        assert s["B"].matrix == matrix_tuple(M)
        rows, lattice = draw_block(cfg.intensity, both.modalities["B"])
        assert s["B"].intensity[0] == rows and np.array_equal(s["B"].intensity[1], lattice) and len(rows) == n_B
        assert s["A"].intensity[1] is not s["B"].intensity[1]          # never shared between the domains


@pytest.mark.parametrize("device_transforms", [False, True])
def test_unpaired_volume_streams(tmp_path, device_transforms):
    from ganslate_amd.data.utils.patch_affine import draw_set, matrix_tuple
    from ganslate_amd.data.utils.patch_intensity import draw_block
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset
    root = _volume_folder(tmp_path)
    mk = lambda aug: UnpairedVolumeDataset(with_aug(vol_conf(root, device_transforms), aug))
    geo = dict(flip=[True, True, True], rotate_deg=[12.0, 6.0, 6.0])
    affine, null, both = mk(geo), mk(dict(geo, intensity=None)), mk(dict(geo, intensity=dict(INTENSITY, modalities=["A"])))
    states = []
    for ds in (affine, null, both):
        random.seed(8)
        np.random.seed(8)
        out = [ds[i] for i in range(2)]
        states.append((random.getstate(), _np_state()))
    assert states[0] == states[1] and states[0][0] == states[2][0]
    np.random.set_state(("MT19937", np.array(states[2][1][0], dtype=np.uint32), states[2][1][1], 0, 0.0))
    assert float(np.random.random_sample()) == _uniform_after(8, 2 * 2 * (8 + 7 + N_LATTICE))    # per sample: A's, then B's
    if device_transforms:
        from ganslate_amd.data.utils.patch_intensity import NEUTRAL
        np.random.seed(8)
        for o in out:
            for k in "AB":
                M, _ = draw_set(both.augmentation)
                rows, lattice = draw_block(both.augmentation.intensity, (k,))
                assert o[k].matrix == matrix_tuple(M) and o[k].intensity[0] == rows
                assert (lattice is None) == (k == "B") and (rows[0] == NEUTRAL) == (k == "B")


# ---- the noise plane ------------------------------------------------------------------------------------------------------
def test_noise_plane_moments_and_keys():
    from ganslate_amd.data.utils.patch_intensity import noise_plane, philox_r01
    from tests.mmimg_ref import philox4x32_10
    n = 16384
    planes = {}
    for key in ((5, 6), (1, 2), (123456789, 987654321)):
        z = noise_plane(n, 0, *key)
        planes[key] = z
        mean, std = float(z.astype(np.float64).mean()), float(z.astype(np.float64).std())
        assert abs(mean) <= 4.0 / np.sqrt(n) and abs(std - 1.0) <= 4.0 / np.sqrt(2 * n), (key, mean, std)
        assert np.array_equal(z, noise_plane(n, 0, *key))                           # the same key: the same bits
    assert not np.array_equal(planes[(5, 6)], planes[(1, 2)])
    assert not np.array_equal(planes[(5, 6)], noise_plane(n, 1, 5, 6))              # another channel: another plane
    # the words themselves, and the float64 value, against the scalar Philox of tests/mmimg_ref.py
    for i, c, key in ((0, 0, (5, 6)), (16383, 2, (1, 2)), ((1 << 32) + 7, 1, (123456789, 987654321))):
        r0, r1 = philox_r01(np.uint64(i & 0xffffffff), np.uint64(i >> 32), np.uint64(c), np.uint64(0), *key)
        assert (int(r0), int(r1)) == philox4x32_10((i & 0xffffffff, i >> 32, c, 0), key)[:2]
    want = R.noise_plane64(256, 0, (5, 6))
    assert float(np.abs(planes[(5, 6)][:256].astype(np.float64) - want).max()) <= 8e-6


# ---- the descriptor -------------------------------------------------------------------------------------------------------
def test_descriptor_layout_matches_the_header():
    from ganslate_amd.hip import lib as L
    header = (Path(__file__).resolve().parent.parent / "include" / "ganslate_hip.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} GsPatchIntensity;", header).group(1)
    fields = []
    for ctype, names in re.findall(r"(float|uint32_t|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    mirror = {ctypes.c_float: "float", ctypes.c_uint32: "uint32_t", ctypes.c_int32: "int32_t"}
    assert fields == [(n, mirror[t]) for n, t in L.PatchIntensity._fields_]
    assert ctypes.sizeof(L.PatchIntensity) == 32 and [getattr(L.PatchIntensity, n).offset for n, _ in fields] == list(range(0, 32, 4))
    for sym in ("gs_patch_augment_clip_minmax", "gs_patch_zscore_intensity"):
        assert sym in L.EXPORTS and re.search(r"\bint " + sym + r"\(", header)


# ---- datasets and pipelines (reference ops) -------------------------------------------------------------------------------
def test_host_dataset_paths_apply_the_chain(tmp_path):
    """the host paths of both datasets against the loop reference applied to their own intermediate values: bits with the
    exact steps (gamma 1, no noise)"""
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.utils.patch_affine import sample_patch
    div = toy_folder(tmp_path / "data")
    ds = MultiModalVolumeDataset(with_aug(dataset_conf(tmp_path / "data", True, "fdg-pet-weighted", (8, 16, 16), divisors=div),
                                          dict(flip=[True, False, True], intensity=dict(EXACT, modalities=["pet", "hx4"]))))
    random.seed(6)
    np.random.seed(6)
    got = ds[1]
    random.seed(6)
    np.random.seed(6)
    (focal, _), _ = ds.sample_points(1, 1)
    (M, field, int_A), (_, _, int_B) = ds.draw_matrices()
    mask = ds.load(ds.body_mask["A"], 1)
    start = [f - p // 2 for f, p in zip(focal, ds.patch_size)]
    for k, block in (("A", int_A), ("B", int_B)):
        rows, lattice = block
        betas = R.beta(ds.patch_size, lattice)
        for c, name in enumerate(ds.modalities[k]):
            g = sample_patch(ds.load(name, 1), mask, start, ds.patch_size, M, ds.outside_value[name], field)
            lo, hi = ds.clip_range[name]
            n = R.clip_unit(g, ds.divisor(name, 1), lo, hi)
            want = F(2) * R.chain(n, rows[c], betas, c) - F(1)
            assert np.array_equal(got[k][c].numpy(), want), (k, name)
            plain = A.clip_minmax(g, ds.divisor(name, 1), lo, hi)
            assert np.array_equal(got[k][c].numpy(), plain) == (name == "ct")       # ct is not listed: today's bits


@pytest.mark.parametrize("paired,scheme", [(True, "fdg-pet-weighted"), (False, "uniform-random-within-body-sf")])
def test_multimodal_pipeline_on_reference_ops(tmp_path, paired, scheme):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.device_volumes import DeviceMultiModalPipeline
    div = toy_folder(tmp_path / "data")
    aug = dict(flip=[True, False, True], intensity=dict(EXACT, prob=0.6))           # active, partly and fully neutral blocks mix
    mk = lambda dt: MultiModalVolumeDataset(with_aug(dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16), divisors=div,
                                                                  device_transforms=dt), aug))
    host, raw = mk(False), mk(True)
    random.seed(9)
    np.random.seed(9)
    want = [host[i] for i in range(3)]
    random.seed(9)
    np.random.seed(9)
    samples = [raw[i] for i in range(3)]
    got = DeviceMultiModalPipeline(raw, "cpu", ops=R.RefIntensityOps())(raw.collate_fn(samples))
    for k in "AB":
        assert np.array_equal(got[k].numpy(), torch.stack([w[k] for w in want]).numpy()), k


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_volume_pipeline_on_reference_ops(tmp_path, dtype):
    from ganslate_amd.data.device_volumes import DeviceVolumePipeline
    from ganslate_amd.data.utils.patch_intensity import active
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset, collate_raw
    (tmp_path / "vol").mkdir()
    root = _volume_folder(tmp_path / "vol", dtype)
    aug = dict(flip=[True, True, False], fill=-5.0, intensity=dict(EXACT, modalities=["A"]))
    mk = lambda dt: UnpairedVolumeDataset(with_aug(vol_conf(root, dt), aug))
    host, raw = mk(False), mk(True)
    random.seed(12)
    np.random.seed(12)
    want = host[0]
    random.seed(12)
    np.random.seed(12)
    sample = raw[0]
    assert active(sample["A"].intensity) is not None and active(sample["B"].intensity) is None
    got = DeviceVolumePipeline(raw, "cpu", ops=R.RefIntensityOps())(collate_raw([sample]))
    for k in "AB":
        assert torch.allclose(got[k][0], want[k], atol=1e-6, rtol=0), k
