"""Elastic deformation of 3-D training patches on the host (ganslate_amd/data/utils/patch_affine.py and the two volume
datasets): the vectorised host gather against the per-voxel loop of tests/patch_elastic_ref.py (equal numbers: both
evaluate the same IEEE operations in the same order), the zero field against the affine gather, the parser and the fold
guard, the consumption of np.random (8 + 1 + 3 G_0 G_1 G_2 uniforms per set), and both datasets and device pipelines
(on injected reference ops) with the `elastic` key."""
import random

import numpy as np
import pytest
import torch

from tests import patch_affine_ref as A
from tests import patch_elastic_ref as E
from tests.mmvol_ref import synthetic_case
from tests.test_mmvol_cpu import _D, dataset_conf, toy_folder
from tests.test_volume_patches_cpu import _conf as vol_conf
from tests.test_volume_patches_cpu import _volume_folder

AUG = dict(prob=1.0, flip=[True, True, True], rotate_deg=[12.0, 6.0, 6.0], scale=[0.9, 1.15], spacing=[3.0, 1.0, 1.0])
ELASTIC = dict(prob=1.0, control_points=[4, 5, 4], max_displacement=[2.0, 1.5, 2.0])     # patch (8, 16, 16): bounds 8.4, 3, 6
N_FIELD = 1 + 3 * 4 * 5 * 4


def with_aug(conf, aug):
    conf.train.dataset["augmentation"] = None if aug is None else _D(aug)
    return conf


def _holes(shape, seed):
    return (np.random.default_rng(seed).random(shape) > 0.15).astype(np.uint8)


# ---- sample_patch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(4, 4, 4), (5, 7, 9)])
def test_host_gather_equals_the_loop_reference(grid):
    from ganslate_amd.data.utils.patch_affine import sample_patch
    shape, patch = (9, 17, 13), [3, 5, 7]
    v = synthetic_case(shape, 5)
    holes = _holes(shape, 6)
    fields = [E.random_field(grid, patch, 17), E.far_field(grid, patch, 18)]
    bad = fields[0].copy()
    bad[1, 1, 2, 1], bad[2, 0, 0, 0] = np.nan, np.inf
    for k, field in enumerate(fields + [bad]):
        for M in (A.rot_zoom_matrix(30.0, 1.1), np.eye(3), A.SHEAR):
            for name in ("ct", "pet"):                           # int16, float32
                for mask in (holes, None):
                    for start in ([2, 4, 3], [0, 0, 0], [6, 12, 6]):
                        got = sample_patch(v[name], mask, start, patch, M, -1024.0, field)
                        want = E.gather([v[name]], mask, start, patch, M, field, [-1024.0])[0]
                        assert got.dtype == want.dtype == np.float32 and np.isfinite(got).all()
                        assert np.array_equal(got, want), (grid, k, name, start)
    far = E.gather([v["pet"]], None, [2, 4, 3], patch, np.eye(3), fields[1], [-7.0])[0]
    assert (far == -7.0).mean() > 0.5                            # ten patch sizes of displacement: mostly outside
    plain = A.gather([v["pet"]], None, [2, 4, 3], patch, np.eye(3), [-7.0])[0]
    assert not np.array_equal(E.gather([v["pet"]], None, [2, 4, 3], patch, np.eye(3), fields[0], [-7.0])[0], plain)


def test_weights_of_the_definition():
    """f = 0 on every knot with (1/6, 4/6, 1/6, 0); the last voxel takes j = G - 4 and f = 1; the weights sum to 1"""
    from ganslate_amd.data.utils.patch_affine import bspline_axis
    j, B = bspline_axis(7, 9)                                    # 6 intervals over 6 steps: every voxel on a knot
    assert j.tolist() == [0, 1, 2, 3, 4, 5, 5]
    assert np.array_equal(np.stack(B)[:, :6], np.tile([[1 / 6], [4 / 6], [1 / 6], [0.0]], (1, 6)))
    assert [b[6] for b in B] == [0.0, 1 / 6, 4 / 6, 1 / 6]
    for p, G in ((3, 4), (16, 7), (10, 6), (2, 64)):
        j, B = bspline_axis(p, G)
        assert j.min() == 0 and j.max() == G - 4 and np.abs(sum(B) - 1.0).max() <= 4e-16
        for o in range(p):
            jr, Br = E.axis_weights(o, p, G)
            assert jr == j[o] and Br == tuple(float(b[o]) for b in B)


def test_a_zero_field_is_the_affine_gather():
    from ganslate_amd.data.utils.patch_affine import sample_patch
    v = synthetic_case((9, 17, 13), 7)
    holes = _holes((9, 17, 13), 8)
    for grid in ((4, 4, 4), (5, 7, 9)):
        for M in (A.rot_zoom_matrix(30.0, 1.1), np.eye(3)):
            for name, mask in (("ct", holes), ("pet", None)):
                got = sample_patch(v[name], mask, [2, 4, 3], [3, 5, 7], M, -3.0, np.zeros((3, *grid)))
                assert np.array_equal(got, sample_patch(v[name], mask, [2, 4, 3], [3, 5, 7], M, -3.0))
                assert np.array_equal(got, sample_patch(v[name], mask, [2, 4, 3], [3, 5, 7], M, -3.0, None))


# ---- parser and fold guard --------------------------------------------------------------------------------------------
BAD = [(dict(strength=1.0), r"elastic: unknown keys \['strength'\]"), (dict(prob=1.5), r"elastic\.prob must lie in \[0, 1\]"),
       (dict(prob=-0.1), r"elastic\.prob must lie"), (dict(prob=float("nan")), r"elastic\.prob must lie"),
       (dict(control_points=[3, 7, 7]), "at least 4 per axis"), (dict(control_points=[7, 7]), "expected three integers"),
       (dict(control_points=[7, 7.5, 7]), "expected three integers"),
       (dict(control_points=[11, 10, 10]), "1100 control points; at most 1024"),
       (dict(max_displacement=[0.0, -1.0, 0.0]), "must not be negative"),
       (dict(max_displacement=[0.0, float("inf"), 0.0]), "expected 3 finite numbers"),
       (dict(max_displacement=[0.0, float("nan"), 0.0]), "expected 3 finite numbers"),
       (dict(max_displacement=[1.0, 1.0]), "expected 3 finite numbers")]


@pytest.mark.parametrize("bad,match", BAD)
def test_parser_refusals(bad, match):
    from ganslate_amd.data.utils.patch_affine import parse_augmentation
    with pytest.raises(ValueError, match=match):
        parse_augmentation(dict(elastic=bad), fill_allowed=True)


def test_parser_defaults_and_null():
    from ganslate_amd.data.utils.patch_affine import parse_augmentation
    assert parse_augmentation(dict(AUG), True).elastic is None
    assert parse_augmentation(dict(AUG, elastic=None), True).elastic is None
    e = parse_augmentation(dict(elastic={}), True).elastic
    assert (e.prob, e.control_points, e.max_displacement, e.uniforms) == (1.0, (7, 7, 7), (0.0, 0.0, 0.0), 1 + 3 * 343)
    e = parse_augmentation(dict(elastic=dict(prob=0.25, control_points=[4, 16, 16], max_displacement=[0, 4, 4.5])), True).elastic
    assert (e.prob, e.control_points, e.max_displacement) == (0.25, (4, 16, 16), (0.0, 4.0, 4.5))      # 1024: at the cap


def test_fold_guard_at_the_bound_and_just_under_it(tmp_path):
    """refused: max_displacement[a] / spacing[a] >= 0.4 (p_a - 1) / (G_a - 3); patch (8, 16, 16), spacing (3, 1, 1)"""
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset
    div = toy_folder(tmp_path / "data")
    root = _volume_folder(tmp_path)
    grid, patch, spacing = (5, 7, 4), (8, 16, 16), (3.0, 1.0, 1.0)
    bound = [0.4 * (patch[a] - 1) / (grid[a] - 3) * spacing[a] for a in range(3)]          # in the units of spacing
    assert bound == pytest.approx([4.2, 1.5, 6.0])
    mm = lambda e: MultiModalVolumeDataset(with_aug(dataset_conf(tmp_path / "data", True, "uniform-random-within-body", patch,
                                                                 divisors=div), dict(AUG, elastic=e)))
    vol = lambda e: UnpairedVolumeDataset(with_aug(vol_conf(root, False), dict(AUG, elastic=e)))
    for make in (mm, vol):
        for a in range(3):
            under = [0.0, 0.0, 0.0]
            under[a] = float(np.nextafter(bound[a], 0.0))
            while under[a] / spacing[a] >= 0.4 * (patch[a] - 1) / (grid[a] - 3):           # the guard's own comparison
                under[a] = float(np.nextafter(under[a], 0.0))
            assert make(dict(control_points=list(grid), max_displacement=under)).augmentation.elastic.max_displacement[a] > 0
            at = list(under)
            at[a] = 0.4 * (patch[a] - 1) / (grid[a] - 3) * spacing[a]
            if at[a] / spacing[a] < 0.4 * (patch[a] - 1) / (grid[a] - 3):
                at[a] = float(np.nextafter(at[a], np.inf))
            with pytest.raises(ValueError, match=rf"max_displacement\[{a}\].*axis {'DHW'[a]}.*must stay below {bound[a]:.6g}"):
                make(dict(control_points=list(grid), max_displacement=at))
    with pytest.raises(ValueError, match="at least 2 voxels per axis"):
        UnpairedVolumeDataset(with_aug(vol_conf(root, False, patch=(1, 16, 16)), dict(elastic=dict(control_points=[4, 4, 4]))))
    with pytest.raises(ValueError, match="3-D patch_size"):
        UnpairedVolumeDataset(with_aug(vol_conf(root, False, patch=(24, 24)), dict(elastic=dict(control_points=[4, 4, 4]))))


# ---- random streams ---------------------------------------------------------------------------------------------------
def _np_state():
    s = np.random.get_state()
    return s[1].tolist(), s[2]


def _uniform_after(seed, n):
    np.random.seed(seed)
    for _ in range(n):
        np.random.random_sample()
    return float(np.random.random_sample())


def test_draw_field_consumes_single_draws_and_follows_the_definition():
    from ganslate_amd.data.utils.patch_affine import draw_field, draw_set, parse_augmentation
    cfg = parse_augmentation(dict(AUG, elastic=ELASTIC), True)
    assert cfg.elastic.uniforms == N_FIELD
    np.random.seed(3)
    us = [float(np.random.random_sample()) for _ in range(N_FIELD)]
    np.random.seed(3)
    field = draw_field(cfg)
    assert float(np.random.random_sample()) == _uniform_after(3, N_FIELD)
    want = np.array([(2.0 * u - 1.0) for u in us[1:]]).reshape(3, 4, 5, 4)
    want = want * np.array(ELASTIC["max_displacement"]).reshape(3, 1, 1, 1) / np.array(AUG["spacing"]).reshape(3, 1, 1, 1)
    assert field.dtype == np.float64 and field.flags["C_CONTIGUOUS"] and np.array_equal(field, want)
    off = parse_augmentation(dict(AUG, elastic=dict(ELASTIC, prob=0.0)), True)
    np.random.seed(3)
    M, none = draw_set(off)
    assert none is None and M.shape == (3, 3)
    assert float(np.random.random_sample()) == _uniform_after(3, 8 + N_FIELD)       # switched off: still all of them
    np.random.seed(3)
    M2, nothing = draw_set(parse_augmentation(dict(AUG), True))
    assert nothing is None and np.array_equal(M, M2) and float(np.random.random_sample()) == _uniform_after(3, 8)
    switch = parse_augmentation(dict(AUG, elastic=dict(ELASTIC, prob=us[0])), True)     # u < prob is strict
    np.random.seed(3)
    assert draw_field(switch) is None


@pytest.mark.parametrize("paired,scheme", [(True, "fdg-pet-weighted"), (False, "uniform-random-within-body-sf")])
@pytest.mark.parametrize("device_transforms", [False, True])
def test_multimodal_streams(tmp_path, paired, scheme, device_transforms):
    from ganslate_amd.data import MultiModalVolumeDataset
    div = toy_folder(tmp_path / "data")
    mk = lambda aug: MultiModalVolumeDataset(with_aug(dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16), divisors=div,
                                                                   device_transforms=device_transforms), aug))
    affine, null, elastic = mk(AUG), mk(dict(AUG, elastic=None)), mk(dict(AUG, elastic=ELASTIC))
    assert affine.augmentation.elastic is None and null.augmentation.elastic is None
    states = []
    for ds in (affine, null):
        random.seed(4)
        np.random.seed(4)
        out = ds[0]
        states.append((random.getstate(), _np_state()))
        assert device_transforms is False or (out["A"].field is None and out["B"].field is None)
    assert states[0] == states[1]                          # `elastic: null` draws nothing extra
    draws = 1 if paired else 2
    random.seed(4)
    np.random.seed(4)
    s = elastic[0]
    assert random.getstate() == states[0][0]               # `random` is not touched
    assert float(np.random.random_sample()) == _uniform_after(4, draws + (8 + N_FIELD) * draws)
    if device_transforms:
        from ganslate_amd.data.utils.patch_affine import draw_set, matrix_tuple
        assert s["A"].field.shape == (3, 4, 5, 4) and s["A"].field.dtype == np.float64
        assert (s["A"].field is s["B"].field) == paired and (s["A"].matrix == s["B"].matrix) == paired
        np.random.seed(4)
        for _ in range(draws):
            np.random.random_sample()
        for k in ("A",) if paired else ("A", "B"):         # the sets follow the sample's own draws: A's, then B's
            M, field = draw_set(elastic.augmentation)
            assert s[k].matrix == matrix_tuple(M) and np.array_equal(s[k].field, field)


@pytest.mark.parametrize("device_transforms", [False, True])
def test_unpaired_volume_streams(tmp_path, device_transforms):
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset
    root = _volume_folder(tmp_path)
    mk = lambda aug: UnpairedVolumeDataset(with_aug(vol_conf(root, device_transforms), aug))
    affine, null, elastic = mk(AUG), mk(dict(AUG, elastic=None)), mk(dict(AUG, elastic=ELASTIC))
    states = []
    for ds in (affine, null, elastic):
        random.seed(8)
        np.random.seed(8)
        out = [ds[i] for i in range(2)]
        states.append((random.getstate(), _np_state()))
    assert states[0] == states[1] and states[0][0] == states[2][0]
    np.random.set_state(("MT19937", np.array(states[2][1][0], dtype=np.uint32), states[2][1][1], 0, 0.0))
    assert float(np.random.random_sample()) == _uniform_after(8, 2 * 2 * (8 + N_FIELD))    # A's set, then B's, per sample
    if device_transforms:
        assert all(o[k].field.shape == (3, 4, 5, 4) for o in out for k in "AB")
        assert not np.array_equal(out[0]["A"].field, out[0]["B"].field)


# ---- datasets and pipelines -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired,scheme", [(True, "fdg-pet-weighted"), (False, "uniform-random-within-body-sf")])
def test_multimodal_dataset_and_pipeline(tmp_path, paired, scheme):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.device_volumes import DeviceMultiModalPipeline
    div = toy_folder(tmp_path / "data")
    mk = lambda aug, dt=False: MultiModalVolumeDataset(with_aug(dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16),
                                                                             divisors=div, device_transforms=dt), aug))
    both = dict(AUG, elastic=ELASTIC)
    out = {}
    for name, ds in (("affine", mk(AUG)), ("elastic", mk(both))):
        random.seed(9)
        np.random.seed(9)
        out[name] = ds[1]
    for k in "AB":
        got = out["elastic"][k]
        assert got.dtype == torch.float32 and got.shape == out["affine"][k].shape and bool(torch.isfinite(got).all())
        assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0
        assert not torch.equal(got, out["affine"][k]), k       # same seed, same matrix: the field does something
    raw = mk(both, True)
    random.seed(9)
    np.random.seed(9)
    sample = raw[1]
    got = DeviceMultiModalPipeline(raw, "cpu", ops=E.RefElasticOps())(raw.collate_fn([sample]))
    for k in "AB":
        assert np.array_equal(got[k][0].numpy(), out["elastic"][k].numpy()), k


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_volume_dataset_and_pipeline(tmp_path, dtype):
    from ganslate_amd.data.device_volumes import DeviceVolumePipeline
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset, collate_raw
    root = _volume_folder(tmp_path, dtype)
    aug = dict(AUG, fill=-5.0)
    mk = lambda a, dt=False: UnpairedVolumeDataset(with_aug(vol_conf(root, dt), a))
    both = dict(aug, elastic=dict(ELASTIC, prob=0.5))            # seed 12: A's field on, B's off (checked below)
    out = {}
    for name, ds in (("affine", mk(aug)), ("elastic", mk(both))):
        random.seed(12)
        np.random.seed(12)
        out[name] = ds[0]
    raw = mk(both, True)
    random.seed(12)
    np.random.seed(12)
    sample = raw[0]
    on = {k: sample[k].field is not None for k in "AB"}
    assert sorted(on.values()) == [False, True], on              # one launch of each kind in this batch
    for k in "AB":
        got = out["elastic"][k]
        assert got.shape == (1, 8, 16, 16) and bool(torch.isfinite(got).all())
        assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0
    got = DeviceVolumePipeline(raw, "cpu", ops=E.RefElasticOps())(collate_raw([sample]))
    for k in "AB":
        assert torch.allclose(got[k][0], out["elastic"][k], atol=1e-6, rtol=0), k
    k_on = "A" if on["A"] else "B"
    np.random.seed(12)                                          # the affine-only run of the same seed draws other matrices
    assert not torch.equal(out["elastic"][k_on], out["affine"][k_on])


def test_elastic_through_the_builders(tmp_path):
    from ganslate_amd.utils.builders import build_conf, build_loader
    div = toy_folder(tmp_path / "data", shape=(36, 40, 38), shape_B=(34, 44, 40))
    field = "{flip: [true, false, true], elastic: {prob: 0.5, control_points: [5, 5, 5], max_displacement: [1, 3, 3]}}"
    conf = build_conf(["config=tests/configs/pix2pix3d_mmvol.yaml", f"train.dataset.root={tmp_path / 'data'}",
                       f"train.dataset.divisors={div}", f"train.dataset.augmentation={field}"])
    conf.mode = "train"
    loader = build_loader(conf)
    e = loader.dataset.augmentation.elastic
    assert (e.prob, e.control_points, e.max_displacement) == (0.5, (5, 5, 5), (1.0, 3.0, 3.0))
    batch = next(iter(loader))
    assert batch["A"].shape == (2, 2, 32, 32, 32) and bool(torch.isfinite(batch["A"]).all())
