"""Affine patch gather on the GPU (csrc/volsample.hip: gs_patch_affine_clip_minmax, gs_patch_affine) against the per-voxel
loop of tests/patch_affine_ref.py. The definition (include/ganslate_hip.h) fixes every IEEE operation and its order —
float64 coordinates without fused multiply-add, float32 lerps of three rounded steps, then the unchanged clip / min-max
chain — so equal numbers are demanded (np.array_equal; a zero may carry the other sign) on NaN-free inputs.

Shapes (volume / patch): (9, 17, 13) / (3, 5, 7) odd sizes; (16, 40, 40) / (8, 16, 16) eight workgroups; (10, 12, 12) /
(6, 6, 6) cubic, for the quarter turns; (24, 100, 90) / (4, 8, 10) rows of 10 voxels that wrap inside a wave and a second,
partly filled workgroup. Every matrix runs at an interior point, the 30 degrees x 1.1 and the sheared matrix at the eight
volume corners as well (the start clamped on every face, the gather reaching outside on three of them). The mask has
holes everywhere (15 % zeros), so corners of both kinds meet in most voxels. Every launch writes into the middle of a
NaN-filled buffer: the result must be finite and the margins untouched.
Raw gather + gs_patch_zscore against the host path: 2e-6 absolute on [-1, 1], the tolerance of
tests/test_volume_patches_gpu.py — the z-score stage is unchanged (double sums against torch's fp32 cascade)."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests import patch_affine_ref as A
from tests.mmvol_ref import synthetic_case
from tests.test_mmvol_cpu import _D, dataset_conf, toy_folder
from tests.test_volume_patches_cpu import _conf as vol_conf
from tests.test_volume_patches_cpu import _volume_folder

pytestmark = pytest.mark.gpu

SHAPES = [((9, 17, 13), (3, 5, 7)), ((16, 40, 40), (8, 16, 16)), ((10, 12, 12), (6, 6, 6)), ((24, 100, 90), (4, 8, 10))]
PARAMS = {"pet": (0.0, 1.0, 0.0, 6.0), "ct": (-1024.0, 1.0, -1000.0, 2000.0), "hx4": (0.0, 1.75, 0.0, 3.0)}   # fill, div, lo, hi
ROT = A.rot_zoom_matrix(30.0, 1.1)
MATRICES = ([("identity", np.eye(3))] + [(f"flip{k}", F) for k, F in enumerate(A.FLIPS) if k] +
            [(f"quarter{a}", A.rot90_matrix(a)) for a in range(3)] +
            [("rot30x1.1", ROT), ("zoom0.5", np.eye(3) * 2.0), ("shear", A.SHEAR)])
AUG = dict(prob=1.0, flip=[True, True, True], rotate_deg=[12.0, 6.0, 6.0], scale=[0.9, 1.15], spacing=[3.0, 1.0, 1.0])


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _case(shape, seed=9):
    v = synthetic_case(shape, seed)
    v["holes"] = (np.random.default_rng(seed + 1).random(shape) > 0.15).astype(np.uint8)
    return v


def _plan(shape, patch):
    """(name, M, point): every matrix at an interior point, two of them at the eight volume corners"""
    inner = tuple(s // 2 - 1 for s in shape)
    plan = [(n, M, inner) for n, M in MATRICES]
    for k, corner in enumerate((z, y, x) for z in (0, shape[0] - 1) for y in (0, shape[1] - 1) for x in (0, shape[2] - 1)):
        plan += [(f"rot30x1.1@corner{k}", ROT, corner), (f"shear@corner{k}", A.SHEAR, corner)]
    return plan


def _poisoned(n, shape, device):
    buf = torch.full((n + 128,), float("nan"), dtype=torch.float32, device=device)         # 64 guard floats on either side
    return buf, buf[64:64 + n].view(*shape)


def _untouched(buf, n):
    return bool(torch.isnan(torch.cat([buf[:64], buf[64 + n:]])).all())


def _clip(ops, dev_vols, dev_mask, names, point, patch, M):
    cols = list(zip(*[PARAMS[n] for n in names]))
    n = len(names) * int(np.prod(patch))
    buf, out = _poisoned(n, (len(names), *patch), ops.device)
    pt = torch.tensor([*point, 0], dtype=torch.int32, device=ops.device)
    ops.patch_affine_clip_minmax(dev_vols, dev_mask, pt, patch, M, *cols, out)
    got = out.cpu().numpy()
    assert _untouched(buf, n) and np.isfinite(got).all()
    return got, cols


@pytest.mark.parametrize("names", [("ct",), ("pet",), ("pet", "ct", "hx4")])
@pytest.mark.parametrize("shape,patch", SHAPES)
def test_clip_minmax_form_equals_the_loop_reference(hip_ops, shape, patch, names):
    v = _case(shape)
    dev_vols, dev_mask = [_dev(v[n], hip_ops.device) for n in names], _dev(v["holes"], hip_ops.device)
    for label, M, point in _plan(shape, patch):
        got, cols = _clip(hip_ops, dev_vols, dev_mask, names, point, patch, M)
        want = A.patch_affine_clip_minmax([v[n] for n in names], v["holes"], point, patch, M, *cols)
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (len(names), *patch)
        assert np.array_equal(got, want), (label, float(np.abs(got - want).max()), int((got != want).sum()))
        assert got.min() >= -1.0 and got.max() <= 1.0


@pytest.mark.parametrize("name", ["ct", "pet"])                  # int16, fp32
@pytest.mark.parametrize("shape,patch", SHAPES)
def test_raw_form_equals_the_loop_reference(hip_ops, shape, patch, name):
    v = _case(shape, 11)
    vol = _dev(v[name], hip_ops.device)
    n = int(np.prod(patch))
    for label, M, point in _plan(shape, patch):
        start = A.start_of(point, list(patch), shape)
        buf, out = _poisoned(n, patch, hip_ops.device)
        hip_ops.patch_affine(vol, start, patch, M, -7.5, out)
        got = out.cpu().numpy()
        assert _untouched(buf, n) and np.isfinite(got).all()
        want = A.patch_affine(v[name], start, patch, M, -7.5)
        assert np.array_equal(got, want), (label, float(np.abs(got - want).max()))
    assert (want == -7.5).any()                                  # the last one, at a volume corner, reaches outside


@pytest.mark.parametrize("shape,patch", SHAPES)
def test_identity_equals_the_plain_crop(hip_ops, shape, patch):
    """at the start `size - patch` the upper corners lie outside with weight 0: the voxel, not `outside`"""
    v = _case(shape, 13)
    names = ("pet", "ct", "hx4")
    dev = hip_ops.device
    dev_vols, dev_mask = [_dev(v[n], dev) for n in names], _dev(v["holes"], dev)
    top = tuple(s - p + p // 2 for s, p in zip(shape, patch))     # the point whose start is size - patch
    for point in (top, shape, (0, 0, 0), tuple(s // 2 for s in shape)):
        got, cols = _clip(hip_ops, dev_vols, dev_mask, names, point, patch, np.eye(3))
        plain = torch.empty((3, *patch), device=dev)
        hip_ops.patch_clip_minmax(dev_vols, dev_mask, torch.tensor([*point, 0], dtype=torch.int32, device=dev), patch, *cols,
                                  plain)
        assert np.array_equal(got, plain.cpu().numpy()), point
    assert A.start_of(top, list(patch), shape) == [s - p for s, p in zip(shape, patch)]
    for name in ("ct", "pet"):
        for start in ([s - p for s, p in zip(shape, patch)], [0, 0, 0]):
            out = torch.full(patch, float("nan"), device=dev)
            hip_ops.patch_affine(_dev(v[name], dev), start, patch, np.eye(3), 1e30, out)
            win = tuple(slice(s, s + p) for s, p in zip(start, patch))
            assert np.array_equal(out.cpu().numpy(), v[name][win].astype(np.float32)), (name, start)


def test_flips_and_quarter_turns_equal_the_transformed_crop(hip_ops):
    shape, patch = (10, 12, 12), (6, 6, 6)
    v = _case(shape, 14)
    dev = hip_ops.device
    dev_vols, dev_mask = [_dev(v["ct"], dev), _dev(v["pet"], dev)], _dev(v["holes"], dev)
    for point in ((5, 6, 6), (9, 11, 11), (0, 0, 0)):
        one = lambda M: _clip(hip_ops, dev_vols, dev_mask, ("ct", "pet"), point, patch, M)[0]
        plain = one(np.eye(3))
        for F in A.FLIPS:
            assert np.array_equal(one(F), plain[:, ::int(F[0, 0]), ::int(F[1, 1]), ::int(F[2, 2])])
        for axis in range(3):
            plane = tuple(1 + a for a in range(3) if a != axis)
            for k in (1, 2, 3):
                assert np.array_equal(one(A.rot90_matrix(axis, k)), np.rot90(plain, -k, plane)), (axis, k)


def test_far_outside_fills_and_stays_inside_its_output(hip_ops):
    """source steps of 40 voxels: all but the centre of the patch lies far outside the volume on every side"""
    shape, patch = (16, 40, 40), (8, 16, 16)
    v = _case(shape, 15)
    dev = hip_ops.device
    n = int(np.prod(patch))
    for M in (np.eye(3) * 40.0, np.eye(3) * -1e300, np.diag([1e18, -3.0, 1e-300])):
        buf, out = _poisoned(n, patch, dev)
        hip_ops.patch_affine(_dev(v["pet"], dev), (4, 12, 12), patch, M, 2.5, out)
        got = out.cpu().numpy()
        assert _untouched(buf, n) and np.isfinite(got).all()
        assert np.array_equal(got, A.patch_affine(v["pet"], (4, 12, 12), patch, M, 2.5))
        assert (got == 2.5).mean() > 0.8
        got, _ = _clip(hip_ops, [_dev(v["ct"], dev)], _dev(v["holes"], dev), ("ct",), (8, 20, 20), patch, M)
        assert (got == -1.0).mean() > 0.8                        # -1024 clamps to the range's low end


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _i3(vals):
    return (C.c_int32 * 3)(*vals)


def test_refusals_come_before_any_launch(hip_ops):
    from ganslate_amd.hip import lib as L
    dev = hip_ops.device
    v = _case((9, 17, 13))
    mask, pet, ct = _dev(v["holes"], dev), _dev(v["pet"], dev), _dev(v["ct"], dev)
    pt = torch.tensor([4, 8, 6, 0], dtype=torch.int32, device=dev)
    out = torch.full((1, 3, 5, 7), 5.0, device=dev)
    big = torch.full((9, 3, 5, 7), 5.0, device=dev)
    nan, inf = float("nan"), float("inf")
    one = lambda **k: hip_ops.patch_affine_clip_minmax(k.get("vols", [pet]), mask, pt, k.get("patch", (3, 5, 7)),
                                                       k.get("M", np.eye(3)), [0.0], [k.get("div", 1.0)], [k.get("lo", 0.0)],
                                                       [k.get("hi", 6.0)], k.get("out", out))
    for bad in (nan, inf, -inf):
        for at in (0, 4, 8):
            M = np.eye(3).reshape(9).copy()
            M[at] = bad
            with pytest.raises(L.HipError, match="non-finite"):
                one(M=M)
            with pytest.raises(L.HipError, match="non-finite"):
                hip_ops.patch_affine(ct, (1, 2, 3), (3, 5, 7), M, 0.0, out[0])
    with pytest.raises(L.HipError, match="clip range"):
        one(lo=6.0)
    with pytest.raises(L.HipError, match="clip range"):
        one(lo=7.0)
    with pytest.raises(L.HipError, match="clip range"):
        one(hi=nan)
    with pytest.raises(L.HipError, match="divisor"):
        one(div=0.0)
    with pytest.raises(L.HipError, match="divisor"):
        one(div=nan)
    for patch in ((3, 5, 14), (3, 18, 7), (10, 5, 7)):           # larger than the volume on one axis
        with pytest.raises(L.HipError, match="does not fit"):
            one(patch=patch, out=torch.full((1, *patch), 5.0, device=dev))
        with pytest.raises(L.HipError, match="does not fit"):
            hip_ops.patch_affine(ct, (0, 0, 0), patch, np.eye(3), 0.0, torch.full(patch, 5.0, device=dev))
    with pytest.raises(L.HipError, match="between 1 and 8 modalities"):
        hip_ops.patch_affine_clip_minmax([pet] * 9, mask, pt, (3, 5, 7), np.eye(3), [0.0] * 9, [1.0] * 9, [0.0] * 9, [6.0] * 9,
                                         big)
    for start in ((7, 2, 3), (1, 13, 3), (1, 2, -1)):            # the window leaves the volume
        with pytest.raises(L.HipError, match="outside the 9 x 17 x 13 volume"):
            hip_ops.patch_affine(ct, start, (3, 5, 7), np.eye(3), 0.0, out[0])
    # what HipOps itself would catch: straight at the C entry points
    lib = hip_ops.lib
    fl = lambda x: (C.c_float * 1)(x)
    eye = (C.c_double * 9)(*np.eye(3).reshape(9))
    base = dict(vols=(C.c_void_p * 1)(pet.data_ptr()), dtypes=(C.c_int32 * 1)(0), C=1, mask=mask.data_ptr(), D=9, H=17, W=13,
                point=pt.data_ptr(), patch=_i3((3, 5, 7)), M=eye, outside=fl(0.0), divisor=fl(1.0), lo=fl(0.0), hi=fl(6.0),
                out=out.data_ptr(), stream=None)
    call = lambda **k: L.check(lib.gs_patch_affine_clip_minmax(*{**base, **k}.values()), "gs_patch_affine_clip_minmax")
    for name in ("vols", "dtypes", "mask", "point", "patch", "M", "outside", "divisor", "lo", "hi", "out"):
        with pytest.raises(L.HipError, match="null argument"):
            call(**{name: None})
    with pytest.raises(L.HipError, match="null volume"):
        call(vols=(C.c_void_p * 1)(None))
    for bad_c in (0, -1, 9):
        with pytest.raises(L.HipError, match="between 1 and 8 modalities"):
            call(C=bad_c)
    for k in (dict(D=0), dict(H=-3), dict(W=0), dict(patch=_i3((0, 5, 7))), dict(patch=_i3((3, 5, -7)))):
        with pytest.raises(L.HipError, match="does not fit"):
            call(**k)
    for dt in (2, -1):
        with pytest.raises(L.HipError, match="dtype"):
            call(dtypes=(C.c_int32 * 1)(dt))
    raw = dict(vol=ct.data_ptr(), dtype=1, D=9, H=17, W=13, start=_i3((1, 2, 3)), size=_i3((3, 5, 7)), M=eye,
               fill=C.c_float(0.0), out=out.data_ptr(), stream=None)
    rcall = lambda **k: L.check(lib.gs_patch_affine(*{**raw, **k}.values()), "gs_patch_affine")
    for name in ("vol", "start", "size", "M", "out"):
        with pytest.raises(L.HipError, match="null argument"):
            rcall(**{name: None})
    for dt in (2, -1):
        with pytest.raises(L.HipError, match="dtype"):
            rcall(dtype=dt)
    for k in (dict(D=0), dict(W=-1), dict(size=_i3((3, 0, 7)))):
        with pytest.raises(L.HipError, match="does not fit"):
            rcall(**k)
    call()                                                       # the unmodified argument sets are valid ones
    torch.cuda.synchronize()
    assert not bool((out == 5.0).all())
    out.fill_(5.0)
    rcall()
    torch.cuda.synchronize()
    assert not bool((out == 5.0).all()) and bool((big == 5.0).all())


def test_refused_calls_leave_the_output_alone(hip_ops):
    from ganslate_amd.hip import lib as L
    dev = hip_ops.device
    v = _case((9, 17, 13))
    mask, pet = _dev(v["holes"], dev), _dev(v["pet"], dev)
    pt = torch.tensor([4, 8, 6, 0], dtype=torch.int32, device=dev)
    buf, out = _poisoned(105, (1, 3, 5, 7), dev)
    bad = np.eye(3)
    bad[1, 2] = float("nan")
    for k in (dict(M=bad), dict(lo=6.0), dict(div=0.0), dict(div=float("nan"))):
        with pytest.raises(L.HipError):
            hip_ops.patch_affine_clip_minmax([pet], mask, pt, (3, 5, 7), k.get("M", np.eye(3)), [0.0], [k.get("div", 1.0)],
                                             [k.get("lo", 0.0)], [6.0], out)
    with pytest.raises(L.HipError):
        hip_ops.patch_affine(pet, (7, 0, 0), (3, 5, 7), np.eye(3), 0.0, out[0])
    with pytest.raises(L.HipError):
        hip_ops.patch_affine(pet, (0, 0, 0), (3, 5, 7), bad, 0.0, out[0])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    with pytest.raises(ValueError, match="out"):
        hip_ops.patch_affine(pet, (0, 0, 0), (3, 5, 7), np.eye(3), 0.0, torch.empty((3, 5, 8), device=dev))
    with pytest.raises(ValueError, match="matrix"):
        hip_ops.patch_affine(pet, (0, 0, 0), (3, 5, 7), np.eye(4), 0.0, out[0])
    with pytest.raises(ValueError, match="point"):
        hip_ops.patch_affine_clip_minmax([pet], mask, pt.long(), (3, 5, 7), np.eye(3), [0.0], [1.0], [0.0], [6.0], out)


# ---- raw gather + z-score, pipelines, Trainer ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_raw_gather_then_zscore_equals_the_host_path(hip_ops, dtype):
    from ganslate_amd.data.utils.normalization import z_score_normalize
    from ganslate_amd.data.utils.patch_affine import sample_patch
    from tests.test_volume_patches_cpu import seeded_volume
    vol = seeded_volume((20, 36, 30), 41).numpy().astype(dtype)
    dev = hip_ops.device
    size = (8, 16, 16)
    for M, start in ((ROT, (6, 10, 7)), (A.SHEAR, (12, 20, 14)), (np.diag([-1.0, 1.0, -1.0]), (0, 0, 0))):
        raw, out = torch.empty(size, device=dev), torch.empty(size, device=dev)
        hip_ops.patch_affine(_dev(vol, dev), start, size, M, -2.0, raw)
        hip_ops.patch_zscore(raw, (0, 0, 0), size, out, (-1.0, 1.0))
        host = sample_patch(vol, None, start, size, M, -2.0)
        assert np.array_equal(raw.cpu().numpy(), host)
        want = z_score_normalize(torch.from_numpy(host), scale_to_range=(-1, 1))
        assert torch.allclose(out.cpu(), want, atol=2e-6, rtol=0)


def _with_aug(conf, aug):
    conf.train.dataset["augmentation"] = _D(aug)
    return conf


@pytest.mark.parametrize("paired,scheme", [(True, "fdg-pet-weighted"), (False, "uniform-random-within-body-sf")])
def test_multimodal_pipeline_equals_the_host_dataset_path(hip_ops, tmp_path, paired, scheme):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.device_volumes import DeviceMultiModalPipeline
    div = toy_folder(tmp_path / "data")
    mk = lambda dt: _with_aug(dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16), divisors=div, device_transforms=dt),
                              AUG)
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
        assert all(s["A"].matrix is not None and (s["A"].matrix == s["B"].matrix) == paired for s in samples)
        runs.append({k: t.cpu() for k, t in pipe(raw.collate_fn(samples)).items()})
    for key in "AB":
        ref = torch.stack([w[key] for w in want])
        assert runs[0][key].shape == ref.shape and runs[0][key].dtype == torch.float32
        assert np.array_equal(runs[0][key].numpy(), ref.numpy()), (key, float((runs[0][key] - ref).abs().max()))
        assert np.array_equal(runs[0][key].numpy(), runs[1][key].numpy())          # one seed, identical batches


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_volume_pipeline_equals_the_host_dataset_path(hip_ops, tmp_path, dtype):
    from ganslate_amd.data.device_volumes import DeviceVolumePipeline
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset, collate_raw
    root = _volume_folder(tmp_path, dtype)
    aug = dict(AUG, fill=-5.0)
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
        runs.append({k: t.cpu() for k, t in pipe(collate_raw([raw[i] for i in range(4)])).items()})
    for key in "AB":
        ref = torch.stack([w[key] for w in want])
        assert runs[0][key].shape == ref.shape == (4, 1, 8, 16, 16)
        assert torch.allclose(runs[0][key], ref, atol=2e-6, rtol=0), key
        assert torch.equal(runs[0][key], runs[1][key])


def test_trainer_runs_on_augmented_device_batches(hip_ops, tmp_path):
    """two iterations of the paired 3-D Pix2Pix recipe fed by the device pipeline, with and without `augmentation`: finite
    losses, batches in [-1, 1], and the augmented batches differ from the plain ones of the same seed"""
    from ganslate_amd.engines import init_engine
    div = toy_folder(tmp_path / "data", shape=(36, 40, 38), shape_B=(34, 44, 40))
    args = ["config=tests/configs/pix2pix3d_mmvol.yaml", f"train.output_dir={tmp_path / 'out'}",
            f"train.dataset.root={tmp_path / 'data'}", f"train.dataset.divisors={div}", "train.seed=5", "train.n_iters=2",
            "train.dataset.device_transforms=True"]
    field = "{prob: 1.0, flip: [true, true, true], rotate_deg: [12, 6, 6], scale: [0.9, 1.15], spacing: [3, 1, 1]}"
    runs = {}
    for aug in (True, False):
        trainer = init_engine("train", args + ([f"train.dataset.augmentation={field}"] if aug else []))
        seen = []
        orig = trainer.model.set_input
        trainer.model.set_input = lambda data, _o=orig, _s=seen: (_s.append({k: v.detach().float().cpu().clone()
                                                                           for k, v in data.items()}), _o(data))[1]
        trainer.run()
        assert trainer.input_pipeline is not None
        assert all(bool(torch.isfinite(v.detach()).all()) for v in trainer.model.losses.values() if v is not None)
        runs[aug] = seen
    assert len(runs[True]) == len(runs[False]) == 2
    for a, b in zip(runs[True], runs[False]):
        for k, ch in (("A", 2), ("B", 1)):
            assert a[k].shape == b[k].shape == (2, ch, 32, 32, 32)
            assert bool(torch.isfinite(a[k]).all()) and float(a[k].min()) >= -1.0 and float(a[k].max()) <= 1.0
            assert not torch.equal(a[k], b[k]), k
