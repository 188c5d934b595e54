"""Multi-modal patch sampling on the GPU (csrc/volsample.hip): gs_voxel_draw against the rule of tests/mmvol_ref.py with
exact equality of (z, y, x, flag), gs_patch_clip_minmax bit for bit against five numpy float32 operations, the device
pipeline against the host dataset path, and two Trainer runs fed through it.

Draw tests hold weights that are integers or small multiples of 1/8: every float64 sum is then exact in any order, so the
kernel's fixed summation order (per run, per range, over ranges) and numpy's cumsum give the same numbers and equality is
demanded outright. Shapes: (9, 17, 13) / (3, 5, 7) — odd sizes, floor vs ceil of p / 2, every rank; (16, 40, 40) / (8, 16,
16) — 4608 zone voxels over 256 ranges of 18, one voxel per run; (24, 100, 90) / (4, 8, 10) — 147200 zone voxels, ranges of
575, runs of 3 voxels that wrap rows. Values against the torch host path: op for op in fp32, 2e-6 absolute on [-1, 1] as in
tests/test_volume_patches_gpu.py."""
import random
import time

import numpy as np
import pytest
import torch

from tests import mmvol_ref as R
from tests.test_mmvol_cpu import dataset_conf, toy_folder

pytestmark = pytest.mark.gpu

LAST_U = float(np.nextafter(1.0, 0.0))
SHAPES = [((9, 17, 13), (3, 5, 7)), ((16, 40, 40), (8, 16, 16)), ((24, 100, 90), (4, 8, 10))]


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _draws(ops, mask, weight, patch, us, **focal):
    """one launch per u into one table, one copy back"""
    out = torch.full((len(us), 4), -7, dtype=torch.int32, device=mask.device)
    for i, u in enumerate(us):
        ops.voxel_draw(mask, weight, patch, u, out[i], **focal)
    return [tuple(r) for r in out.cpu().tolist()]


def _targets(m, patch, range_len, stride):
    """uniforms that land on chosen voxels of the weight map m: strided ranks, plus the first and last positive voxel of
    every workgroup range of the zone's box (box C order), u = 0 and the last double below 1"""
    lo, hi = R.zone_of(m.shape, patch)
    box = m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].ravel()
    pos = np.flatnonzero(box > 0)
    prefix = np.cumsum(box)
    total = prefix[-1]
    picks = set(pos[::stride].tolist())
    for start in range(0, box.size, range_len):
        inside = pos[(pos >= start) & (pos < start + range_len)]
        if inside.size:
            picks.update((int(inside[0]), int(inside[-1])))
    us = [float((prefix[j] - box[j] / 2) / total) for j in sorted(picks)]     # the middle of voxel j's share
    return [0.0, LAST_U] + us, len(picks)


@pytest.mark.parametrize("shape,patch", SHAPES)
@pytest.mark.parametrize("weight", [None, "pet", "ct"])
def test_draw_equals_the_reference_rule(hip_ops, shape, patch, weight):
    v = R.synthetic_case(shape, 5)
    w = None if weight is None else v[weight]                      # fp32 multiples of 1/8 / int16; both hold negatives
    m = R.weight_map(v["body"], w, patch)
    lo, hi = R.zone_of(shape, patch)
    zone_n = int(np.prod([h - l for l, h in zip(lo, hi)]))
    range_len = hip_ops.voxel_draw_range_len(shape, patch)
    assert range_len == -(-zone_n // 256) == R.RefMMOps().voxel_draw_range_len(shape, patch)
    count = int((m > 0).sum())
    if w is not None:
        body_zone = R.weight_map(v["body"], None, patch) > 0
        assert (np.asarray(w)[body_zone] < 0).any() and count < int(body_zone.sum())      # clipped weights are in play
    us, n = _targets(m, patch, range_len, 1 if count < 1000 else max(1, count // 150))
    assert n == count or count >= 1000                             # the small shape: every rank
    got = _draws(hip_ops, _dev(v["body"], hip_ops.device), None if w is None else _dev(w, hip_ops.device), patch, us)
    want = [(*R.select(m, u, w is not None), 0) for u in us]
    assert got == want
    assert len(set(want)) >= n                                     # the targets are distinct voxels, all of them hit


def test_draw_in_a_zone_holding_one_body_voxel(hip_ops):
    shape, patch = (9, 17, 13), (3, 5, 7)
    v = R.synthetic_case(shape, 6)
    mask = np.zeros(shape, np.uint8)
    mask[0, :, :] = 1                                              # body outside the zone does not count
    mask[:, :, 12] = 1
    mask[5, 9, 6] = 1
    for w in (None, v["ct"].astype(np.float32) * 0 + 0.125, np.full(shape, 3, np.int16)):
        got = _draws(hip_ops, _dev(mask, hip_ops.device), None if w is None else _dev(w, hip_ops.device), patch,
                     [0.0, 0.3, 0.999, LAST_U])
        assert got == [(5, 9, 6, 0)] * 4
        assert R.voxel_draw(mask, w, patch, 0.3) == (5, 9, 6, 0)


def test_empty_sets_give_minus_one(hip_ops):
    v = R.synthetic_case((8, 16, 16), 1)
    dev = hip_ops.device
    assert _draws(hip_ops, _dev(v["body"], dev), None, (8, 16, 16), [0.5]) == [(-1, -1, -1, 0)]       # patch == volume
    assert _draws(hip_ops, _dev(v["body"], dev), _dev(v["pet"], dev), (8, 16, 15), [0.5]) == [(-1, -1, -1, 0)]
    hollow = np.zeros((12, 20, 20), np.uint8)
    hollow[0] = 1
    assert _draws(hip_ops, _dev(hollow, dev), None, (4, 8, 8), [0.0, LAST_U]) == [(-1, -1, -1, 0)] * 2
    dark = R.synthetic_case((12, 20, 20), 3)
    dark["pet"][:] = -1.0
    assert _draws(hip_ops, _dev(dark["body"], dev), _dev(dark["pet"], dev), (4, 8, 8), [0.4]) == [(-1, -1, -1, 0)]
    assert R.voxel_draw(dark["body"], dark["pet"], (4, 8, 8), 0.4) == (-1, -1, -1, 0)
    focal = torch.tensor([6, 10, 10, 0], dtype=torch.int32, device=dev)
    got = _draws(hip_ops, _dev(hollow, dev), None, (4, 8, 8), [0.4], focal_A=focal, dims_A=(12, 20, 20),
                 proportion=(0.5, 0.5, 0.5))
    assert got == [(-1, -1, -1, 1)] == [R.voxel_draw(hollow, None, (4, 8, 8), 0.4, (6, 10, 10), (12, 20, 20), (0.5, 0.5, 0.5))]


@pytest.mark.parametrize("shape_A,shape_B,patch,prop", [((16, 40, 40), (18, 36, 44), (8, 16, 16), (0.6, 0.3, 0.3)),
                                                         ((9, 17, 13), (11, 15, 14), (3, 5, 7), (0.5, 0.4, 0.6)),
                                                         ((24, 100, 90), (30, 84, 97), (4, 8, 10), (0.35, 0.3, 0.25))])
def test_stochastic_focal_draw_with_boxes_cut_by_the_volume_edge(hip_ops, shape_A, shape_B, patch, prop):
    B = R.synthetic_case(shape_B, 17)
    mask = _dev(B["body"], hip_ops.device)
    lo, hi = R.zone_of(shape_A, patch)
    corners = [(z, y, x) for z in (lo[0], hi[0] - 1) for y in (lo[1], hi[1] - 1) for x in (lo[2], hi[2] - 1)]
    centre = tuple(s // 2 for s in shape_A)
    cut_low = cut_high = 0
    for fa in corners + [centre, (0, 0, 0), tuple(s - 1 for s in shape_A)]:
        blo, bhi = R.focal_box(fa, shape_A, shape_B, prop)
        cut_low += any(l == 0 for l in blo)
        cut_high += any(h == s for h, s in zip(bhi, shape_B))
        focal = torch.tensor([*fa, 0], dtype=torch.int32, device=hip_ops.device)
        us = [0.0, 0.123, 0.5, 0.877, LAST_U]
        got = _draws(hip_ops, mask, None, patch, us, focal_A=focal, dims_A=shape_A, proportion=prop)
        want = [R.voxel_draw(B["body"], None, patch, u, fa, shape_A, prop) for u in us]
        assert got == want, fa
        for z, y, x, flag in got:
            assert flag == 1 or all(l <= p < h for p, l, h in zip((z, y, x), blo, bhi))
    assert cut_low >= 1 and cut_high >= 1                          # boxes cut at 0 and at the volume's size were drawn from


def test_focal_box_that_misses_the_body_falls_back_to_the_unrestricted_draw(hip_ops):
    shape_A, shape_B, patch, prop = (16, 40, 40), (18, 36, 44), (8, 16, 16), (0.3, 0.2, 0.2)
    B = R.synthetic_case(shape_B, 4, "low")
    mask = _dev(B["body"], hip_ops.device)
    fa = (11, 30, 31)
    focal = torch.tensor([*fa, 0], dtype=torch.int32, device=hip_ops.device)
    us = [0.0, 0.25, 0.731, LAST_U] + [(k + 0.5) / 97 for k in range(97)]
    got = _draws(hip_ops, mask, None, patch, us, focal_A=focal, dims_A=shape_A, proportion=prop)
    free = _draws(hip_ops, mask, None, patch, us)
    assert all(g[3] == 1 for g in got) and all(f[3] == 0 for f in free)
    assert [g[:3] for g in got] == [f[:3] for f in free]
    assert got == [R.voxel_draw(B["body"], None, patch, u, fa, shape_A, prop) for u in us]


def test_draw_refusals_come_before_any_launch(hip_ops):
    from ganslate_amd.hip.lib import HipError
    v = R.synthetic_case((9, 17, 13), 5)
    mask, out = _dev(v["body"], hip_ops.device), torch.zeros(4, dtype=torch.int32, device=hip_ops.device)
    with pytest.raises(HipError, match="not in \\[0, 1\\)"):
        hip_ops.voxel_draw(mask, None, (3, 5, 7), 1.0, out)
    with pytest.raises(HipError, match="does not fit"):
        hip_ops.voxel_draw(mask, None, (3, 18, 7), 0.5, out)
    with pytest.raises(ValueError, match="differs from the mask"):
        hip_ops.voxel_draw(mask, _dev(v["pet"][:8], hip_ops.device), (3, 5, 7), 0.5, out)
    with pytest.raises(ValueError, match="weight"):
        hip_ops.voxel_draw(mask, _dev(v["pet"].astype(np.float64), hip_ops.device), (3, 5, 7), 0.5, out)
    with pytest.raises(ValueError, match="out"):
        hip_ops.voxel_draw(mask, None, (3, 5, 7), 0.5, out[:3])
    with pytest.raises(ValueError, match="dims_A"):
        hip_ops.voxel_draw(mask, None, (3, 5, 7), 0.5, out, focal_A=out)
    assert out.cpu().tolist() == [0, 0, 0, 0]


# ---- gs_patch_clip_minmax ---------------------------------------------------------------------------------------------
PARAMS = {"pet": (0.0, 1.0, 0.0, 6.0), "ct": (-1024.0, 1.0, -1000.0, 2000.0), "hx4": (0.0, 1.75, 0.0, 3.0)}   # fill, div, lo, hi


def _patch_both(ops, v, names, point, patch, poison=float("nan")):
    cols = list(zip(*[PARAMS[n] for n in names]))
    want = R.patch_clip_minmax([v[n] for n in names], v["body"], point, list(patch), *cols)
    dev = ops.device
    n = len(names) * int(np.prod(patch))
    buf = torch.full((n + 128,), poison, dtype=torch.float32, device=dev)            # 64 guard floats on either side
    out = buf[64:64 + n].view(len(names), *patch)
    pt = torch.tensor([*point, 0], dtype=torch.int32, device=dev)
    ops.patch_clip_minmax([_dev(v[n], dev) for n in names], _dev(v["body"], dev), pt, patch, *cols, out)
    guard = torch.cat([buf[:64], buf[64 + n:]]).cpu()
    assert torch.isnan(guard).all() if poison != poison else bool((guard == poison).all())
    return out.cpu().numpy(), want


@pytest.mark.parametrize("names", [("pet",), ("ct",), ("pet", "ct", "hx4")])
@pytest.mark.parametrize("shape,patch", [((9, 17, 13), (3, 5, 7)), ((16, 40, 40), (8, 16, 16)), ((20, 70, 75), (6, 33, 64))])
def test_patch_is_bit_equal_to_the_five_fp32_operations(hip_ops, names, shape, patch):
    v = R.synthetic_case(shape, 9)
    lo, hi = R.zone_of(shape, patch)
    # the zone's upper bound is exclusive, so a drawn point leaves one voxel to the far faces: `hi` itself (one past the zone)
    # is the point whose patch touches them; the kernel takes any point
    faces = [(z, y, x) for z in (lo[0], hi[0]) for y in (lo[1], hi[1]) for x in (lo[2], hi[2])]
    faces += [tuple(h - 1 for h in hi)]
    outside = [(0, 0, 0), (-1, -1, -1), shape, (lo[0], hi[1] + 3, lo[2] - 2)]       # clamped into the volume, never read outside
    for k, point in enumerate(faces + [tuple((l + h) // 2 for l, h in zip(lo, hi))] + outside):
        got, want = _patch_both(hip_ops, v, names, point, patch, poison=float("nan") if k % 2 else 1e30)
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (len(names), *patch)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (point, np.abs(got - want).max())
        assert got.min() >= -1.0 and got.max() <= 1.0
    start = [f - p // 2 for f, p in zip(faces[0], patch)]
    assert start == [0, 0, 0] and [f - p // 2 + p for f, p in zip(faces[7], patch)] == list(shape)


def test_patch_equals_the_torch_host_chain(hip_ops):
    from ganslate_amd.data.utils.normalization import min_max_normalize
    v = R.synthetic_case((16, 40, 40), 10)
    point, patch = (7, 19, 22), (8, 16, 16)
    got, _ = _patch_both(hip_ops, v, ("pet", "ct", "hx4"), point, patch)
    win = tuple(slice(f - p // 2, f - p // 2 + p) for f, p in zip(point, patch))
    m = torch.from_numpy(v["body"][win] != 0)
    for c, n in enumerate(("pet", "ct", "hx4")):
        fill, div, lo, hi = PARAMS[n]
        t = torch.where(m, torch.from_numpy(v[n][win].copy()).float(), torch.tensor(fill)) / div
        assert torch.allclose(torch.from_numpy(got[c]), min_max_normalize(torch.clamp(t, lo, hi), lo, hi), atol=2e-6, rtol=0)


def test_patch_refusals_come_before_any_launch(hip_ops):
    from ganslate_amd.hip.lib import HipError
    dev = hip_ops.device
    v = R.synthetic_case((9, 17, 13), 9)
    mask, pet, pt = _dev(v["body"], dev), _dev(v["pet"], dev), torch.tensor([4, 8, 6, 0], dtype=torch.int32, device=dev)
    out = torch.full((1, 3, 5, 7), 5.0, device=dev)
    one = lambda **k: hip_ops.patch_clip_minmax(k.get("vols", [pet]), mask, k.get("pt", pt), k.get("patch", (3, 5, 7)), [0.0],
                                                [k.get("div", 1.0)], [k.get("lo", 0.0)], [k.get("hi", 6.0)], k.get("out", out))
    with pytest.raises(HipError, match="clip range"):
        one(lo=6.0)
    with pytest.raises(HipError, match="divisor"):
        one(div=0.0)
    with pytest.raises(HipError, match="does not fit"):
        one(patch=(3, 5, 14), out=torch.empty((1, 3, 5, 14), device=dev))
    with pytest.raises(ValueError, match="out"):
        one(out=torch.empty((1, 3, 5, 8), device=dev))
    with pytest.raises(ValueError, match="volume 0"):
        one(vols=[pet.double()])
    with pytest.raises(ValueError, match="point"):
        one(pt=pt.long())
    with pytest.raises(HipError, match="between 1 and 8 modalities"):
        hip_ops.patch_clip_minmax([pet] * 9, mask, pt, (3, 5, 7), [0.0] * 9, [1.0] * 9, [0.0] * 9, [6.0] * 9,
                                  torch.empty((9, 3, 5, 7), device=dev))
    with pytest.raises(ValueError, match="at least one volume"):
        hip_ops.patch_clip_minmax([], mask, pt, (3, 5, 7), [], [], [], [], torch.empty((0, 3, 5, 7), device=dev))
    assert bool((out == 5.0).all())


# ---- pipeline and Trainer ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired,scheme", [(True, "uniform-random-within-body"), (True, "fdg-pet-weighted"),
                                           (False, "uniform-random-within-body-sf"), (False, "fdg-pet-weighted-sf")])
@pytest.mark.parametrize("dtype_ct", [np.int16, np.float32])
def test_pipeline_equals_the_host_dataset_path(hip_ops, tmp_path, paired, scheme, dtype_ct):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.device_volumes import DeviceMultiModalPipeline
    div = toy_folder(tmp_path / "data", dtype_ct=dtype_ct)
    host = MultiModalVolumeDataset(dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16), divisors=div))
    raw = MultiModalVolumeDataset(dataset_conf(tmp_path / "data", paired, scheme, (8, 16, 16), divisors=div,
                                               device_transforms=True))
    pipe = DeviceMultiModalPipeline(raw, hip_ops.device, ops=hip_ops)
    random.seed(21)
    np.random.seed(21)
    idx, points = [], []
    for i in range(5):                                             # the host path's draws, as __getitem__ makes them
        ia = i % len(host)
        ib = ia if paired else random.randint(0, len(host) - 1)
        (fa, fb), flag = host.sample_points(ia, ib)
        idx.append((ia, ib))
        points.append([[*fa, 0], [*fb, flag]])
    random.seed(21)
    np.random.seed(21)
    want = [host[i] for i in range(5)]
    random.seed(21)
    np.random.seed(21)
    samples = [raw[i] for i in range(5)]
    assert [(s["A"].index, s["B"].index) for s in samples] == idx
    got = pipe(raw.collate_fn(samples))
    assert pipe.points.cpu().tolist() == points                    # identical focal points, hence identical starts
    for key in "AB":
        ref = torch.stack([w[key] for w in want])
        assert got[key].is_cuda and got[key].shape == ref.shape and got[key].dtype == torch.float32
        assert torch.allclose(got[key].cpu(), ref, atol=2e-6, rtol=0), key
    assert pipe.resident and all(t.is_cuda for t in pipe.resident.values())


def test_pipeline_raises_for_a_case_that_cannot_be_sampled(hip_ops, tmp_path):
    from ganslate_amd.data import MultiModalVolumeDataset
    from tests.test_mmvol_cpu import write_case
    dark = R.synthetic_case((12, 20, 20), 3)
    dark["pet"][:] = -1.0
    write_case(tmp_path / "patient_dark", dark)
    raw = MultiModalVolumeDataset(dataset_conf(tmp_path, True, "fdg-pet-weighted", (4, 8, 8), device_transforms=True))
    pipe = raw.device_pipeline(None, hip_ops.device)
    with pytest.raises(ValueError, match="patient_dark"):
        pipe(raw.collate_fn([raw[0]]))


@pytest.mark.parametrize("yaml,channels_B,patch", [("pix2pix3d_mmvol.yaml", 1, (32, 32, 32)),
                                                   ("cyclegan_balanced_mmvol.yaml", 2, (32, 32, 32))])
def test_trainer_runs_on_the_multimodal_pipeline(hip_ops, tmp_path, yaml, channels_B, patch):
    """case folder -> index-and-uniform samples -> DeviceMultiModalPipeline -> set_input: three iterations, finite losses,
    and the batches the model saw equal the host path's for the same draws"""
    from ganslate_amd.engines import init_engine
    div = toy_folder(tmp_path / "data", shape=(36, 40, 38), shape_B=(34, 44, 40))
    args = [f"config=tests/configs/{yaml}", f"train.output_dir={tmp_path / 'out'}", f"train.dataset.root={tmp_path / 'data'}",
            f"train.dataset.divisors={div}", "train.seed=5"]
    runs = {}
    for dev_tf in (True, False):
        trainer = init_engine("train", args + [f"train.dataset.device_transforms={dev_tf}"])
        seen = []
        orig = trainer.model.set_input
        trainer.model.set_input = lambda data, _o=orig, _s=seen: (_s.append({k: v.detach().float().cpu().clone()
                                                                           for k, v in data.items()}), _o(data))[1]
        trainer.run()
        assert (trainer.input_pipeline is not None) == dev_tf
        assert all(bool(torch.isfinite(v.detach()).all()) for v in trainer.model.losses.values() if v is not None)
        runs[dev_tf] = seen
    assert len(runs[True]) == len(runs[False]) == 3
    for a, b in zip(runs[True], runs[False]):
        assert a["A"].shape == (2, 2, *patch) and a["B"].shape == (2, channels_B, *patch)
        for k in ("A", "B"):
            assert torch.allclose(a[k], b[k], atol=2e-6, rtol=0), k


def test_draw_and_patch_rate_at_the_hx4_shape(hip_ops):
    """No threshold: there is no earlier device path to compare against. Prints samples per second of the paired (one
    weighted draw, 2 + 1 modalities) and the unpaired (two draws, 2 + 2 modalities) launch sequences on a resident
    90 x 300 x 300 case with patch (32, 128, 128), 50 iterations after warm-up."""
    shape, patch = (90, 300, 300), (32, 128, 128)
    v = R.synthetic_case(shape, 2)
    dev = hip_ops.device
    mask, pet, ct, hx4 = (_dev(v[k], dev) for k in ("body", "pet", "ct", "hx4"))
    pts = torch.zeros((2, 4), dtype=torch.int32, device=dev)
    out_A, out_B = torch.empty((2, *patch), device=dev), torch.empty((2, *patch), device=dev)
    rng = np.random.default_rng(0)

    def sample(paired):
        hip_ops.voxel_draw(mask, pet, patch, float(rng.random()), pts[0])
        hip_ops.patch_clip_minmax([pet, ct], mask, pts[0], patch, [0.0, -1024.0], [1.0, 1.0], [0.0, -1000.0], [6.0, 2000.0], out_A)
        if paired:
            hip_ops.patch_clip_minmax([hx4], mask, pts[0], patch, [0.0], [1.75], [0.0], [3.0], out_B[:1])
        else:
            hip_ops.voxel_draw(mask, None, patch, float(rng.random()), pts[1], focal_A=pts[0], dims_A=shape,
                               proportion=(0.6, 0.3, 0.3))
            hip_ops.patch_clip_minmax([hx4, ct], mask, pts[1], patch, [0.0, -1024.0], [1.75, 1.0], [0.0, -1000.0], [3.0, 2000.0],
                                      out_B)
    for paired in (True, False):
        for _ in range(5):
            sample(paired)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            sample(paired)
        torch.cuda.synchronize()
        rate = 50 / (time.perf_counter() - t0)
        print(f"\ndevice draw + patch path, {'paired' if paired else 'unpaired'}: {rate:.0f} samples/s "
              f"({shape[0]} x {shape[1]} x {shape[2]}, patch {patch})")
        assert int(pts[0, 0]) >= 0 and torch.isfinite(out_A).all() and torch.isfinite(out_B[:1]).all()
