"""Elastic patch gather on the GPU (csrc/volsample.hip: gs_patch_elastic_clip_minmax, gs_patch_elastic) against the
per-voxel loop of tests/patch_elastic_ref.py. The definition (include/ganslate_hip.h) fixes every IEEE operation and its
order — integer interval, one float64 division, the B-spline weights and the D / H / W sums without fused multiply-add,
then the affine definition — so equal numbers are demanded (np.array_equal) on finite output.

Cases (volume / patch / lattice): (9, 17, 13) / (3, 5, 7) / (4, 4, 4) one interval, the j clamp with f = 1 on the last
voxel; the same with (5, 7, 9): every voxel on a knot, f = 0; (16, 40, 40) / (8, 16, 16) / (7, 7, 7) fractional f, eight
workgroups; (24, 100, 90) / (4, 8, 10) / (4, 5, 6) rows of 10 that wrap inside a wave and a partly filled last workgroup
(27 rows of R per workgroup, the second one starting inside a row); and the same volume and patch under (4, 4, 64), whose
row table (27 x 3 x 64 doubles) passes the 32 KB up to which the row-shared kernel is launched: the per-voxel kernel.
Every launch writes into the middle of a NaN-filled buffer: the result must be finite and the margins untouched.
The displacement of a (patch, field) pair is computed once by the reference and shared by the tests of its case."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests import patch_affine_ref as A
from tests import patch_elastic_ref as E
from tests.test_mmvol_cpu import dataset_conf, toy_folder
from tests.test_patch_affine_gpu import AUG, PARAMS, ROT, _case, _dev, _i3, _poisoned, _untouched, _with_aug
from tests.test_volume_patches_cpu import _conf as vol_conf
from tests.test_volume_patches_cpu import _volume_folder

pytestmark = pytest.mark.gpu

CASES = [((9, 17, 13), (3, 5, 7), (4, 4, 4)), ((9, 17, 13), (3, 5, 7), (5, 7, 9)), ((16, 40, 40), (8, 16, 16), (7, 7, 7)),
         ((24, 100, 90), (4, 8, 10), (4, 5, 6)), ((24, 100, 90), (4, 8, 10), (4, 4, 64))]
LARGER = [CASES[2], CASES[3]]
MATRICES = [("rot30x1.1", ROT), ("identity", np.eye(3))]
ELASTIC = dict(prob=1.0, control_points=[4, 5, 4], max_displacement=[2.0, 1.5, 2.0])     # patch (8, 16, 16), spacing (3, 1, 1)


def _fields(patch, grid):
    """(name, field): random inside the fold guard, and ten patch sizes of displacement"""
    return [("guarded", E.random_field(grid, patch, 17)),
            ("far", E.far_field(grid, patch, 18))]


def _points(shape):
    return [tuple(s // 2 - 1 for s in shape), (0, 0, 0), tuple(s - 1 for s in shape)]


def _clip(ops, dev_vols, dev_mask, names, point, patch, M, field):
    cols = list(zip(*[PARAMS[n] for n in names]))
    n = len(names) * int(np.prod(patch))
    buf, out = _poisoned(n, (len(names), *patch), ops.device)
    pt = torch.tensor([*point, 0], dtype=torch.int32, device=ops.device)
    ops.patch_elastic_clip_minmax(dev_vols, dev_mask, pt, patch, M, _dev(field, ops.device), *cols, out)
    got = out.cpu().numpy()
    assert _untouched(buf, n) and np.isfinite(got).all()
    return got, cols


def _raw(ops, dev_vol, start, patch, M, field, fill):
    n = int(np.prod(patch))
    buf, out = _poisoned(n, patch, ops.device)
    ops.patch_elastic(dev_vol, start, patch, M, _dev(field, ops.device), fill, out)
    got = out.cpu().numpy()
    assert _untouched(buf, n) and np.isfinite(got).all()
    return got


@pytest.mark.parametrize("names", [("ct",), ("pet",), ("pet", "ct", "hx4")])          # int16, fp32, C = 3
@pytest.mark.parametrize("shape,patch,grid", CASES)
def test_clip_minmax_form_equals_the_loop_reference(hip_ops, shape, patch, grid, names):
    v = _case(shape)
    dev_vols, dev_mask = [_dev(v[n], hip_ops.device) for n in names], _dev(v["holes"], hip_ops.device)
    for fname, field in _fields(patch, grid):
        outside = 0
        for mname, M in MATRICES:
            for point in _points(shape):
                got, cols = _clip(hip_ops, dev_vols, dev_mask, names, point, patch, M, field)
                want = E.patch_elastic_clip_minmax([v[n] for n in names], v["holes"], point, patch, M, field, *cols)
                assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (len(names), *patch)
                assert np.array_equal(got, want), (fname, mname, point, float(np.abs(got - want).max()), int((got != want).sum()))
                assert got.min() >= -1.0 and got.max() <= 1.0
                lo_end = A.clip_minmax(np.float32([cols[0][0]]), cols[1][0], cols[2][0], cols[3][0])[0]
                outside += float((got[0] == lo_end).mean()) / 6
        assert fname != "far" or outside > 0.5               # most voxels take the outside value


@pytest.mark.parametrize("name", ["ct", "pet"])                  # int16, fp32
@pytest.mark.parametrize("shape,patch,grid", CASES)
def test_raw_form_equals_the_loop_reference(hip_ops, shape, patch, grid, name):
    v = _case(shape, 11)
    vol = _dev(v[name], hip_ops.device)
    for fname, field in _fields(patch, grid):
        outside = 0
        for mname, M in MATRICES:
            for point in _points(shape):
                start = A.start_of(point, list(patch), shape)
                got = _raw(hip_ops, vol, start, patch, M, field, -7.5)
                want = E.patch_elastic(v[name], start, patch, M, field, -7.5)
                assert np.array_equal(got, want), (fname, mname, point, float(np.abs(got - want).max()))
                outside += float((got == -7.5).mean()) / 6
        assert fname != "far" or outside > 0.5


@pytest.mark.parametrize("shape,patch,grid", CASES)
def test_a_zero_field_equals_the_affine_entry_points(hip_ops, shape, patch, grid):
    v = _case(shape, 13)
    names = ("pet", "ct", "hx4")
    dev = hip_ops.device
    dev_vols, dev_mask = [_dev(v[n], dev) for n in names], _dev(v["holes"], dev)
    zero = np.zeros((3, *grid))
    for _, M in MATRICES + [("shear", A.SHEAR)]:
        for point in _points(shape):
            got, cols = _clip(hip_ops, dev_vols, dev_mask, names, point, patch, M, zero)
            affine = torch.empty((3, *patch), device=dev)
            hip_ops.patch_affine_clip_minmax(dev_vols, dev_mask, torch.tensor([*point, 0], dtype=torch.int32, device=dev), patch,
                                             M, *cols, affine)
            assert np.array_equal(got, affine.cpu().numpy()), point
            start = A.start_of(point, list(patch), shape)
            for name in ("ct", "pet"):
                affine = torch.empty(patch, device=dev)
                hip_ops.patch_affine(_dev(v[name], dev), start, patch, M, -7.5, affine)
                assert np.array_equal(_raw(hip_ops, _dev(v[name], dev), start, patch, M, zero, -7.5), affine.cpu().numpy())


@pytest.mark.parametrize("shape,patch,grid", CASES)
def test_a_nan_entry_stays_inside_its_support(hip_ops, shape, patch, grid):
    v = _case(shape, 14)
    dev = hip_ops.device
    clean = E.random_field(grid, patch, 21)
    js = [[E.axis_weights(o, patch[a], grid[a])[0] for o in range(patch[a])] for a in range(3)]
    at = (1, *[js[a][patch[a] // 2] for a in range(3)])         # component H, the first control point the middle voxel reads
    bad = clean.copy()
    bad[at] = np.nan
    reads = [np.array([j <= at[1 + a] <= j + 3 for j in js[a]]) for a in range(3)]
    support = reads[0][:, None, None] & reads[1][None, :, None] & reads[2][None, None, :]
    assert support.any()
    start = A.start_of(_points(shape)[0], list(patch), shape)
    got = {k: _raw(hip_ops, _dev(v["pet"], dev), start, patch, ROT, f, -7.5) for k, f in (("clean", clean), ("bad", bad))}
    assert np.array_equal(got["bad"], E.patch_elastic(v["pet"], start, patch, ROT, bad, -7.5))
    assert np.array_equal(got["bad"][~support], got["clean"][~support])
    assert (got["bad"][support] == -7.5).all() and not np.array_equal(got["bad"], got["clean"])
    names = ("ct", "pet")
    dev_vols, dev_mask = [_dev(v[n], dev) for n in names], _dev(v["holes"], dev)
    one, cols = _clip(hip_ops, dev_vols, dev_mask, names, _points(shape)[0], patch, ROT, bad)
    assert np.array_equal(one, E.patch_elastic_clip_minmax([v[n] for n in names], v["holes"], _points(shape)[0], patch, ROT, bad,
                                                           *cols))
    two, _ = _clip(hip_ops, dev_vols, dev_mask, names, _points(shape)[0], patch, ROT, clean)
    assert np.array_equal(one[:, ~support], two[:, ~support])


@pytest.mark.parametrize("shape,patch,grid", CASES)
def test_the_per_voxel_kernel_gives_the_row_shared_kernels_bits(hip_ops, shape, patch, grid):
    """option elastic_rows = 0 forces the per-voxel form, 65536 the row-shared one (every case's table fits 64 KB)"""
    v = _case(shape, 16)
    dev = hip_ops.device
    names = ("pet", "ct", "hx4")
    dev_vols, dev_mask = [_dev(v[n], dev) for n in names], _dev(v["holes"], dev)
    assert hip_ops.get_option("elastic_rows") == 32768
    for _, field in _fields(patch, grid):
        for point in _points(shape):
            got = {}
            for rows in (0, 65536):
                with hip_ops.options(elastic_rows=rows):
                    got[rows] = (_clip(hip_ops, dev_vols, dev_mask, names, point, patch, ROT, field)[0],
                                 _raw(hip_ops, dev_vols[1], A.start_of(point, list(patch), shape), patch, ROT, field, -7.5))
            assert np.array_equal(got[0][0], got[65536][0]) and np.array_equal(got[0][1], got[65536][1]), point
    assert hip_ops.get_option("elastic_rows") == 32768


@pytest.mark.parametrize("shape,patch,grid", LARGER)
def test_both_forms_equal_the_host_path(hip_ops, shape, patch, grid):
    from ganslate_amd.data.utils.patch_affine import sample_patch
    v = _case(shape, 15)
    dev = hip_ops.device
    names = ("pet", "ct", "hx4")
    dev_vols, dev_mask = [_dev(v[n], dev) for n in names], _dev(v["holes"], dev)
    for _, field in _fields(patch, grid):
        for _, M in MATRICES + [("shear", A.SHEAR)]:
            for point in _points(shape):
                start = A.start_of(point, list(patch), shape)
                got, cols = _clip(hip_ops, dev_vols, dev_mask, names, point, patch, M, field)
                for c, n in enumerate(names):
                    host = sample_patch(v[n], v["holes"], start, patch, M, cols[0][c], field)
                    assert np.array_equal(got[c], A.clip_minmax(host, cols[1][c], cols[2][c], cols[3][c])), (n, point)
                for n in ("ct", "pet"):
                    assert np.array_equal(_raw(hip_ops, _dev(v[n], dev), start, patch, M, field, -7.5),
                                          sample_patch(v[n], None, start, patch, M, -7.5, field)), (n, point)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(hip_ops):
    from ganslate_amd.hip import lib as L
    dev = hip_ops.device
    v = _case((9, 17, 13))
    mask, pet, ct = _dev(v["holes"], dev), _dev(v["pet"], dev), _dev(v["ct"], dev)
    pt = torch.tensor([4, 8, 6, 0], dtype=torch.int32, device=dev)
    buf, out = _poisoned(105, (1, 3, 5, 7), dev)
    field = lambda *g: torch.zeros((3, *g), dtype=torch.float64, device=dev)
    one = lambda **k: hip_ops.patch_elastic_clip_minmax([pet], mask, pt, k.get("patch", (3, 5, 7)), k.get("M", np.eye(3)),
                                                        k.get("field", field(4, 4, 4)), [0.0], [k.get("div", 1.0)],
                                                        [k.get("lo", 0.0)], [6.0], k.get("out", out))
    raw = lambda **k: hip_ops.patch_elastic(ct, k.get("start", (1, 2, 3)), k.get("patch", (3, 5, 7)), k.get("M", np.eye(3)),
                                            k.get("field", field(4, 4, 4)), 0.0, k.get("out", out[0]))
    for fn in (one, raw):
        for g in ((3, 4, 4), (4, 3, 4), (4, 4, 3), (1, 8, 8)):
            with pytest.raises(L.HipError, match="at least 4 control points per axis"):
                fn(field=field(*g))
        for g in ((11, 10, 10), (4, 4, 65), (5, 5, 41)):
            with pytest.raises(L.HipError, match="exceeds 1024"):
                fn(field=field(*g))
        fn(field=field(4, 4, 64), out=torch.empty_like(out if fn is one else out[0]))       # 1024: at the cap
        for patch in ((1, 5, 7), (3, 1, 7), (3, 5, 1)):
            small = torch.full((1, *patch) if fn is one else patch, 5.0, device=dev)
            with pytest.raises(L.HipError, match="at least 2 voxels per axis"):
                fn(patch=patch, out=small)
            torch.cuda.synchronize()
            assert bool((small == 5.0).all())
        # what the affine entries refuse
        bad = np.eye(3)
        bad[1, 2] = float("nan")
        with pytest.raises(L.HipError, match="non-finite"):
            fn(M=bad)
        with pytest.raises(L.HipError, match="does not fit"):
            fn(patch=(3, 18, 7), out=torch.full((1, 3, 18, 7) if fn is one else (3, 18, 7), 5.0, device=dev))
        # a field that is not a contiguous float64 device tensor of shape [3, G0, G1, G2]
        for wrong in (field(4, 4, 4).float(), field(4, 4, 4).cpu(), field(4, 4, 8)[..., ::2], field(4, 4, 4)[:2],
                      field(4, 4, 4)[0], np.zeros((3, 4, 4, 4)), None):
            with pytest.raises(ValueError, match="field"):
                fn(field=wrong)
    with pytest.raises(L.HipError, match="clip range"):
        one(lo=6.0)
    with pytest.raises(L.HipError, match="divisor"):
        one(div=0.0)
    with pytest.raises(L.HipError, match="outside the 9 x 17 x 13 volume"):
        raw(start=(7, 2, 3))
    # straight at the C entry points: a null grid or field, and every other null argument
    lib = hip_ops.lib
    fl = lambda x: (C.c_float * 1)(x)
    eye = (C.c_double * 9)(*np.eye(3).reshape(9))
    fz = field(4, 4, 4)
    base = dict(vols=(C.c_void_p * 1)(pet.data_ptr()), dtypes=(C.c_int32 * 1)(0), C=1, mask=mask.data_ptr(), D=9, H=17, W=13,
                point=pt.data_ptr(), patch=_i3((3, 5, 7)), M=eye, grid=_i3((4, 4, 4)), field=fz.data_ptr(), outside=fl(0.0),
                divisor=fl(1.0), lo=fl(0.0), hi=fl(6.0), out=out.data_ptr(), stream=None)
    call = lambda **k: L.check(lib.gs_patch_elastic_clip_minmax(*{**base, **k}.values()), "gs_patch_elastic_clip_minmax")
    rbase = dict(vol=ct.data_ptr(), dtype=1, D=9, H=17, W=13, start=_i3((1, 2, 3)), size=_i3((3, 5, 7)), M=eye,
                 grid=_i3((4, 4, 4)), field=fz.data_ptr(), fill=C.c_float(0.0), out=out.data_ptr(), stream=None)
    rcall = lambda **k: L.check(lib.gs_patch_elastic(*{**rbase, **k}.values()), "gs_patch_elastic")
    for fn in (call, rcall):
        for k in (dict(grid=None), dict(field=None), dict(grid=None, field=None)):
            with pytest.raises(L.HipError, match="null grid or field"):
                fn(**k)
        with pytest.raises(L.HipError, match="at least 4 control points"):
            fn(grid=_i3((4, 4, -4)))
    for name in ("vols", "dtypes", "mask", "point", "patch", "M", "outside", "divisor", "lo", "hi", "out"):
        with pytest.raises(L.HipError, match="null argument"):
            call(**{name: None})
    for name in ("vol", "start", "size", "M", "out"):
        with pytest.raises(L.HipError, match="null argument"):
            rcall(**{name: None})
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())                          # nothing was launched on the shared output
    call()                                                       # the unmodified argument sets are valid ones
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and _untouched(buf, 105)
    out.fill_(float("nan"))
    rcall()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and _untouched(buf, 105)


# ---- pipelines, Trainer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired,scheme", [(True, "fdg-pet-weighted"), (False, "uniform-random-within-body-sf")])
def test_multimodal_pipeline_equals_the_host_dataset_path(hip_ops, tmp_path, paired, scheme):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.device_volumes import DeviceMultiModalPipeline
    div = toy_folder(tmp_path / "data")
    aug = dict(AUG, elastic=dict(ELASTIC, prob=0.6))             # elastic, affine-only and (never here) plain launches mix
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
        on = [s[k].field is not None for s in samples for k in "AB"]
        assert any(on) and not all(on)
        assert all((s["A"].field is s["B"].field) == paired or s["A"].field is None for s in samples)
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
    aug = dict(AUG, fill=-5.0, elastic=ELASTIC)
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
        assert all(s[k].field is not None for s in samples for k in "AB")
        runs.append({k: t.cpu() for k, t in pipe(collate_raw(samples)).items()})
    for key in "AB":
        ref = torch.stack([w[key] for w in want])
        assert runs[0][key].shape == ref.shape == (4, 1, 8, 16, 16)
        assert torch.allclose(runs[0][key], ref, atol=2e-6, rtol=0), key
        assert torch.equal(runs[0][key], runs[1][key])


def test_trainer_runs_on_elastic_device_batches(hip_ops, tmp_path):
    """two iterations of the paired 3-D Pix2Pix recipe fed by the device pipeline, with and without the `elastic` key:
    finite losses, batches in [-1, 1], and the elastic batches differ from the affine-only ones of the same seed"""
    from ganslate_amd.engines import init_engine
    div = toy_folder(tmp_path / "data", shape=(36, 40, 38), shape_B=(34, 44, 40))
    args = ["config=tests/configs/pix2pix3d_mmvol.yaml", f"train.output_dir={tmp_path / 'out'}",
            f"train.dataset.root={tmp_path / 'data'}", f"train.dataset.divisors={div}", "train.seed=5", "train.n_iters=2",
            "train.dataset.device_transforms=True"]
    affine = "prob: 1.0, flip: [true, true, true], rotate_deg: [12, 6, 6], scale: [0.9, 1.15], spacing: [3, 1, 1]"
    elastic = "elastic: {prob: 1.0, control_points: [5, 5, 5], max_displacement: [1, 3, 3]}"
    runs = {}
    for key, field in (("elastic", f"{{{affine}, {elastic}}}"), ("affine", f"{{{affine}}}")):
        trainer = init_engine("train", args + [f"train.dataset.augmentation={field}"])
        seen = []
        orig = trainer.model.set_input
        trainer.model.set_input = lambda data, _o=orig, _s=seen: (_s.append({k: v.detach().float().cpu().clone()
                                                                           for k, v in data.items()}), _o(data))[1]
        trainer.run()
        assert trainer.input_pipeline is not None
        assert all(bool(torch.isfinite(v.detach()).all()) for v in trainer.model.losses.values() if v is not None)
        runs[key] = seen
    assert len(runs["elastic"]) == len(runs["affine"]) == 2
    for a, b in zip(runs["elastic"], runs["affine"]):
        for k, ch in (("A", 2), ("B", 1)):
            assert a[k].shape == b[k].shape == (2, ch, 32, 32, 32)
            assert bool(torch.isfinite(a[k]).all()) and float(a[k].min()) >= -1.0 and float(a[k].max()) <= 1.0
            assert not torch.equal(a[k], b[k]), k
