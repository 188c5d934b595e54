"""Random affine augmentation of 3-D training patches on the host (ganslate_amd/data/utils/patch_affine.py and the two
volume datasets): the matrix builder's exact cases, the vectorised host gather against the per-voxel loop of
tests/patch_affine_ref.py (equal numbers: both evaluate the same IEEE operations in the same order), the consumption of
the random streams, the config surface and its validation, and both device pipelines' control flow on injected reference
ops against the host dataset path. The multi-modal chain behind the gather is the same fp32 operations on both sides, so
equality is demanded; the z-score behind the raw gather keeps the 1e-6 of tests/test_volume_patches_cpu.py (double sums on
the op side, torch's fp32 cascade on the host side)."""
import random

import numpy as np
import pytest
import torch

from tests import patch_affine_ref as A
from tests.mmvol_ref import synthetic_case
from tests.test_mmvol_cpu import _D, dataset_conf, toy_folder
from tests.test_volume_patches_cpu import _conf as vol_conf
from tests.test_volume_patches_cpu import _volume_folder

AUG = dict(prob=1.0, flip=[True, True, True], rotate_deg=[12.0, 6.0, 6.0], scale=[0.9, 1.15], spacing=[3.0, 1.0, 1.0])


def with_aug(conf, aug):
    conf.train.dataset["augmentation"] = None if aug is None else _D(aug)
    return conf


# ---- affine_matrix ------------------------------------------------------------------------------------------------------
def test_matrix_exact_cases():
    from ganslate_amd.data.utils.patch_affine import affine_matrix
    none = (False, False, False)
    for sp in ((1, 1, 1), (3, 1, 1), (2.5, 0.9, 0.9), (0.7, 0.7, 0.7)):
        assert np.array_equal(affine_matrix(none, (0, 0, 0), 1.0, sp), np.eye(3))
        assert np.array_equal(affine_matrix(none, (0, 0, 0), 2.0, sp), np.eye(3) / 2)
        for flips in ((True, False, False), (False, True, True), (True, True, True)):
            assert np.array_equal(affine_matrix(flips, (0, 0, 0), 1.0, sp), np.diag([-1.0 if f else 1.0 for f in flips]))
    M = affine_matrix(none, (0, 0, 0), 1.0, (1, 1, 1))
    assert M.dtype == np.float64 and M.shape == (3, 3)
    for axis in range(3):                                  # quarter turns are signed permutations, exactly
        ang = [0.0, 0.0, 0.0]
        ang[axis] = 90.0
        assert np.array_equal(affine_matrix(none, ang, 1.0, (1, 1, 1)), A.rot90_matrix(axis))
        ang[axis] = -90.0
        assert np.array_equal(affine_matrix(none, ang, 1.0, (1, 1, 1)), A.rot90_matrix(axis, 3))


def test_matrix_rotations_are_orthogonal_and_rigid_in_millimetres():
    from ganslate_amd.data.utils.patch_affine import affine_matrix
    none = (False, False, False)
    for ang in ((30.0, 0.0, 0.0), (0.0, -17.5, 0.0), (0.0, 0.0, 44.0), (12.0, -7.0, 29.0)):
        R = affine_matrix(none, ang, 1.0, (1, 1, 1))
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15
        assert np.linalg.det(R) == pytest.approx(1.0, abs=1e-15)
    # a rotation about axis 0 turns in the (H, W) plane only: the spacing along D does not enter
    assert np.array_equal(affine_matrix(none, (30.0, 0, 0), 1.0, (3, 1, 1)), affine_matrix(none, (30.0, 0, 0), 1.0, (1, 1, 1)))
    # anisotropic in the rotated plane: rigid in millimetres, i.e. diag(sp) M diag(1 / sp) is the rotation
    sp = np.array([3.0, 1.0, 1.0])
    M = affine_matrix(none, (0, 25.0, 0), 1.0, sp)
    R = affine_matrix(none, (0, 25.0, 0), 1.0, (1, 1, 1))
    assert np.allclose(np.diag(sp) @ M @ np.diag(1 / sp), R, atol=1e-15, rtol=0) and not np.allclose(M, R, atol=1e-3)
    th = np.deg2rad(30.0)
    want = np.array([[1, 0, 0], [0, np.cos(th), -np.sin(th)], [0, np.sin(th), np.cos(th)]]) / 1.1
    assert np.allclose(affine_matrix((False, True, False), (30.0, 0, 0), 1.1, (1, 1, 1)), want @ np.diag([1, -1, 1]),
                       atol=1e-15, rtol=0)
    with pytest.raises(ValueError, match="zoom"):
        affine_matrix(none, (0, 0, 0), 0.0, (1, 1, 1))


# ---- sample_patch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ct", "pet"])                  # int16, fp32
@pytest.mark.parametrize("masked", [True, False])
def test_host_gather_equals_the_loop_reference(name, masked):
    from ganslate_amd.data.utils.patch_affine import sample_patch
    v = synthetic_case((9, 17, 13), 5)
    mask = v["body"] if masked else None
    patch = [3, 5, 7]
    for M in (A.rot_zoom_matrix(30.0, 1.1), A.SHEAR, np.eye(3) * 2.0):
        for start in ([2, 4, 3], [0, 0, 0], [6, 12, 6]):
            got = sample_patch(v[name], mask, start, patch, M, -1024.0)
            want = A.gather([v[name]], mask, start, patch, M, [-1024.0])[0]
            assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want), (start, M)
    assert (A.gather([v[name]], mask, [6, 12, 6], patch, np.eye(3) * 2.0, [-1024.0]) == -1024.0).any()   # reaches outside


def test_identity_flips_and_quarter_turns_reproduce_the_crop():
    from ganslate_amd.data.utils.patch_affine import sample_patch
    v = synthetic_case((10, 12, 12), 6)
    for patch, start in (([6, 6, 6], [4, 6, 6]), ([6, 6, 6], [0, 3, 2]), ([3, 5, 4], [7, 7, 8]), ([10, 12, 12], [0, 0, 0])):
        win = tuple(slice(s, s + p) for s, p in zip(start, patch))
        plain = np.where(v["body"][win] != 0, v["ct"][win].astype(np.float32), np.float32(-1024.0))
        for fn in (lambda M: sample_patch(v["ct"], v["body"], start, patch, M, -1024.0),
                   lambda M: A.gather([v["ct"]], v["body"], start, patch, M, [-1024.0])[0]):
            assert np.array_equal(fn(np.eye(3)), plain)          # the far faces too: an upper corner of weight 0
            for F in A.FLIPS:
                flipped = plain[::int(F[0, 0]), ::int(F[1, 1]), ::int(F[2, 2])]
                assert np.array_equal(fn(F), flipped)
            if patch == [6, 6, 6]:
                for axis in range(3):
                    plane = tuple(a for a in range(3) if a != axis)
                    assert np.array_equal(fn(A.rot90_matrix(axis)), np.rot90(plain, -1, plane))
                    assert np.array_equal(fn(A.rot90_matrix(axis, 3)), np.rot90(plain, 1, plane))
                    assert np.array_equal(fn(A.rot90_matrix(axis, 2)), np.rot90(plain, 2, plane))


# ---- random streams ---------------------------------------------------------------------------------------------------
def _states():
    return random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2]


def _uniform_after(seed, n):
    np.random.seed(seed)
    for _ in range(n):
        np.random.random_sample()
    return float(np.random.random_sample())


@pytest.mark.parametrize("paired,scheme", [(True, "fdg-pet-weighted"), (False, "uniform-random-within-body-sf")])
@pytest.mark.parametrize("device_transforms", [False, True])
def test_multimodal_streams(tmp_path, paired, scheme, device_transforms):
    from ganslate_amd.data import MultiModalVolumeDataset
    div = toy_folder(tmp_path / "data")
    mk = lambda: dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16), divisors=div, device_transforms=device_transforms)
    absent, none, aug = MultiModalVolumeDataset(mk()), MultiModalVolumeDataset(with_aug(mk(), None)), \
        MultiModalVolumeDataset(with_aug(mk(), AUG))
    assert absent.augmentation is None and none.augmentation is None and aug.augmentation.prob == 1.0
    runs = []
    for ds in (absent, none):
        random.seed(4)
        np.random.seed(4)
        runs.append(([ds[i] for i in range(3)], _states()))
    assert runs[0][1] == runs[1][1]                        # `augmentation: null` draws nothing
    for a, b in zip(runs[0][0], runs[1][0]):
        for k in "AB":
            if device_transforms:
                assert (a[k].index, a[k].u, a[k].matrix) == (b[k].index, b[k].u, None)
            else:
                assert torch.equal(a[k], b[k])
    draws = 1 if paired else 2
    random.seed(4)
    np.random.seed(4)
    s = aug[0]
    py_state = random.getstate()
    assert float(np.random.random_sample()) == _uniform_after(4, draws + 8 * draws)       # eight more per set, exactly
    random.seed(4)
    absent[0]
    assert random.getstate() == py_state                   # `random` is not touched
    if device_transforms:
        assert len(s["A"].matrix) == 9 and all(isinstance(x, float) for x in s["A"].matrix)
        assert (s["A"].matrix == s["B"].matrix) == paired  # one M for a paired sample, independent sets otherwise
        # the sets follow the sample's own draws: u_A [, u_B], then A's eight [, then B's eight]
        from ganslate_amd.data.utils.patch_affine import draw_params, matrix_tuple
        np.random.seed(4)
        us = [np.random.random_sample() for _ in range(draws)]
        assert s["A"].u == us[0] and (paired or s["B"].u == us[1])
        assert s["A"].matrix == matrix_tuple(draw_params(aug.augmentation))
        assert paired or s["B"].matrix == matrix_tuple(draw_params(aug.augmentation))


@pytest.mark.parametrize("device_transforms", [False, True])
def test_unpaired_volume_streams(tmp_path, device_transforms):
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset
    root = _volume_folder(tmp_path)
    absent = UnpairedVolumeDataset(vol_conf(root, device_transforms))
    none = UnpairedVolumeDataset(with_aug(vol_conf(root, device_transforms), None))
    aug = UnpairedVolumeDataset(with_aug(vol_conf(root, device_transforms), dict(AUG, fill=-3.0)))
    assert absent.augmentation is None and none.augmentation is None and aug.augmentation.fill == -3.0
    runs = []
    for ds in (absent, none, aug):
        random.seed(8)
        np.random.seed(8)
        runs.append(([ds[i] for i in range(3)], _states()))
    assert runs[0][1] == runs[1][1]
    assert runs[0][1][0] == runs[2][1][0]                  # augmentation leaves `random` (the patch starts) alone
    np.random.seed(8)
    assert float(np.random.random_sample()) == _uniform_after(8, 0)
    np.random.set_state(("MT19937", np.array(runs[2][1][1], dtype=np.uint32), runs[2][1][2], 0, 0.0))
    assert float(np.random.random_sample()) == _uniform_after(8, 3 * 16)                  # A's set, then B's set, per sample
    for a, b, c in zip(*[r[0] for r in runs]):
        for k in "AB":
            if device_transforms:
                assert (a[k].index, a[k].start, a[k].matrix) == (b[k].index, b[k].start, None)
                assert (c[k].index, c[k].start) == (a[k].index, a[k].start) and len(c[k].matrix) == 9
            else:
                assert torch.equal(a[k], b[k]) and c[k].shape == a[k].shape and not torch.equal(a[k], c[k])
        if device_transforms:
            assert c["A"].matrix != c["B"].matrix


def test_prob_zero_without_flips_gives_the_plain_tensors(tmp_path):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset
    off = dict(AUG, prob=0.0, flip=[False, False, False])
    div = toy_folder(tmp_path / "data")
    for paired, scheme in ((True, "uniform-random-within-body"), (False, "fdg-pet-weighted-sf")):
        mk = lambda: dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16), divisors=div)
        plain, ds = MultiModalVolumeDataset(mk()), MultiModalVolumeDataset(with_aug(mk(), off))
        for i in range(3):                                 # reseeded per sample: the eight uniforms come last
            out = []
            for d in (plain, ds):
                random.seed(30 + i)
                np.random.seed(30 + i)
                out.append(d[i])
            assert all(torch.equal(out[0][k], out[1][k]) for k in "AB")
    (tmp_path / "vol").mkdir()
    root = _volume_folder(tmp_path / "vol", np.int16)
    plain, ds = UnpairedVolumeDataset(vol_conf(root, False)), UnpairedVolumeDataset(with_aug(vol_conf(root, False), off))
    random.seed(3)
    want = [plain[i] for i in range(3)]
    random.seed(3)
    got = [ds[i] for i in range(3)]
    assert all(torch.equal(w[k], g[k]) for w, g in zip(want, got) for k in "AB")


# ---- device pipelines on reference ops --------------------------------------------------------------------------------
@pytest.mark.parametrize("paired,scheme", [(True, "fdg-pet-weighted"), (False, "uniform-random-within-body-sf")])
def test_multimodal_pipeline_on_reference_ops_equals_the_host_path(tmp_path, paired, scheme):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.device_volumes import DeviceMultiModalPipeline
    div = toy_folder(tmp_path / "data")
    mk = lambda dt: with_aug(dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16), divisors=div, device_transforms=dt), AUG)
    host, raw = MultiModalVolumeDataset(mk(False)), MultiModalVolumeDataset(mk(True))
    random.seed(9)
    np.random.seed(9)
    want = [host[i] for i in range(2)]
    after = _states()
    random.seed(9)
    np.random.seed(9)
    samples = [raw[i] for i in range(2)]
    assert _states() == after                              # both paths consume the same draws
    got = DeviceMultiModalPipeline(raw, "cpu", ops=A.RefAffineOps())(raw.collate_fn(samples))
    for key in "AB":
        ref = torch.stack([w[key] for w in want])
        assert got[key].shape == ref.shape == (2, 2 if key == "A" or not paired else 1, 8, 16, 16)
        assert got[key].dtype == torch.float32 and np.array_equal(got[key].numpy(), ref.numpy()), key
        assert float(ref.min()) >= -1.0 and float(ref.max()) <= 1.0
    plain = MultiModalVolumeDataset(dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16), divisors=div))
    random.seed(9)
    np.random.seed(9)
    assert not torch.equal(plain[0]["A"], want[0]["A"])    # the augmentation does something


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_volume_pipeline_on_reference_ops_equals_the_host_path(tmp_path, dtype):
    from ganslate_amd.data.device_volumes import DeviceVolumePipeline
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset, collate_raw
    root = _volume_folder(tmp_path, dtype)
    aug = dict(AUG, fill=-5.0)
    host = UnpairedVolumeDataset(with_aug(vol_conf(root, False), aug))
    raw = UnpairedVolumeDataset(with_aug(vol_conf(root, True), aug))
    random.seed(12)
    np.random.seed(12)
    want = [host[i] for i in range(2)]
    after = _states()
    random.seed(12)
    np.random.seed(12)
    samples = [raw[i] for i in range(2)]
    assert _states() == after
    got = DeviceVolumePipeline(raw, "cpu", ops=A.RefAffineOps())(collate_raw(samples))
    for key in "AB":
        ref = torch.stack([w[key] for w in want])
        assert got[key].shape == ref.shape == (2, 1, 8, 16, 16) and got[key].dtype == torch.float32
        assert torch.allclose(got[key], ref, atol=1e-6, rtol=0)


# ---- config surface ---------------------------------------------------------------------------------------------------
def test_augmentation_through_the_builders(tmp_path):
    from ganslate_amd.utils.builders import build_conf, build_loader
    div = toy_folder(tmp_path / "data", shape=(36, 40, 38), shape_B=(34, 44, 40))
    field = "{prob: 0.5, flip: [true, false, true], rotate_deg: [10, 0, 0], scale: [0.9, 1.1], spacing: [3, 1, 1]}"
    conf = build_conf(["config=tests/configs/pix2pix3d_mmvol.yaml", f"train.dataset.root={tmp_path / 'data'}",
                       f"train.dataset.divisors={div}", f"train.dataset.augmentation={field}"])
    conf.mode = "train"
    loader = build_loader(conf)
    a = loader.dataset.augmentation
    assert (a.prob, a.flip, a.rotate_deg, a.scale, a.spacing) == (0.5, (True, False, True), (10.0, 0.0, 0.0), (0.9, 1.1),
                                                                  (3.0, 1.0, 1.0))
    batch = next(iter(loader))
    assert batch["A"].shape == (2, 2, 32, 32, 32) and bool(torch.isfinite(batch["A"]).all())
    (tmp_path / "vol").mkdir()
    root = _volume_folder(tmp_path / "vol")
    conf = build_conf(["config=tests/configs/cyclegan3d_volumefolder.yaml", f"train.dataset.root={root}",
                       "train.dataset.augmentation={flip: [true, true, true], fill: -1.0}"])
    conf.mode = "train"
    loader = build_loader(conf)
    assert loader.dataset.augmentation.fill == -1.0 and loader.dataset.augmentation.prob == 1.0
    assert next(iter(loader))["A"].shape == (2, 1, 8, 16, 16)
    conf = build_conf(["config=tests/configs/cyclegan3d_volumefolder.yaml", f"train.dataset.root={root}"])
    assert conf.train.dataset.augmentation is None


BAD = [(dict(prob=1.5), "prob"), (dict(prob=-0.1), "prob"), (dict(prob=float("nan")), "prob"),
       (dict(scale=[0.0, 1.0]), "scale"), (dict(scale=[1.2, 1.1]), "scale"), (dict(scale=[1.0]), "scale"),
       (dict(spacing=[1.0, 0.0, 1.0]), "spacing"), (dict(spacing=[1.0, -2.0, 1.0]), "spacing"),
       (dict(spacing=[1.0, 1.0]), "spacing"), (dict(flip=[True, False]), "flip"), (dict(rotate_deg=[10.0, 10.0]), "rotate_deg"),
       (dict(rotate_deg=[10.0, float("inf"), 0.0]), "rotate_deg"), (dict(rotation=[1, 2, 3]), "unknown keys")]


@pytest.mark.parametrize("bad,match", BAD)
def test_validation_errors_are_raised_at_construction(tmp_path, bad, match):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset
    case = synthetic_case((12, 20, 20), 1)
    (tmp_path / "mm" / "case0").mkdir(parents=True)
    for k, v in case.items():
        np.save(tmp_path / "mm" / "case0" / f"{k}.npy", v)
    with pytest.raises(ValueError, match=match):
        MultiModalVolumeDataset(with_aug(dataset_conf(tmp_path / "mm", True, "uniform-random-within-body", (4, 8, 8)), bad))
    (tmp_path / "vol").mkdir()
    root = _volume_folder(tmp_path / "vol")
    with pytest.raises(ValueError, match=match):
        UnpairedVolumeDataset(with_aug(vol_conf(root, False), bad))


def test_fill_and_two_dimensional_patches(tmp_path):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset
    case = synthetic_case((12, 20, 20), 1)
    (tmp_path / "mm" / "case0").mkdir(parents=True)
    for k, v in case.items():
        np.save(tmp_path / "mm" / "case0" / f"{k}.npy", v)
    with pytest.raises(ValueError, match="fill"):          # the multi-modal dataset fills with outside_value
        MultiModalVolumeDataset(with_aug(dataset_conf(tmp_path / "mm", True, "uniform-random-within-body", (4, 8, 8)),
                                         dict(fill=1.0)))
    (tmp_path / "vol").mkdir()
    root = _volume_folder(tmp_path / "vol")
    with pytest.raises(ValueError, match="3-D patch_size"):
        UnpairedVolumeDataset(with_aug(vol_conf(root, False, patch=(24, 24)), dict(prob=1.0)))
    assert UnpairedVolumeDataset(with_aug(vol_conf(root, False, patch=(24, 24)), None)).augmentation is None
    assert UnpairedVolumeDataset(with_aug(vol_conf(root, False), {})).augmentation.flip == (False, False, False)
