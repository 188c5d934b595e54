"""gs_img_stack on the GPU (csrc/imgstack.hip) against the float64 oracle (tests/mmimg_ref.py), the noise plane's behaviour,
DeviceMultiModalImagePipeline against the host datasets, and the Trainer, Validator and Tester on the two new configs with
`device_transforms: true` in every mode.

Bounds. E = sum |w_y w_x x| and the expected value are both taken with the float64 weights, s = 2 / (hi - lo) for a rescaled
modality and 1 otherwise, eps32 = 2^-23.
- kernel against the oracle: 12 * eps32 * E * s + 2e-6 + 8e-6 * noise_std. The kernel reads its weights from tables that
  hold the float64 weights rounded once, and computes no coordinate; what is left are two weight roundings, two products
  and 15 additions per term chain — at most 19 roundings of eps32 / 2, 9.5 eps32, asserted at 12. 2e-6 is the tolerance
  tests/test_mmvol_gpu.py gives the same clamp / min-max chain. Noise: |z| <= 5.77, the angle 2 pi u2 is rounded once
  (2 pi * 2^-24 absolute) and logf, sqrtf, cosf are each a few ulp: 6.3e-6 per unit std, asserted at 8e-6.
- same size in and out: the weights are (0, 1, 0, 0) and the output is the fp32 clamp / min-max chain of the stored values,
  bit for bit (numpy fp32, one IEEE operation per step like the kernel).
- pipeline against the host dataset: (12 + K_t) * eps32 * E * s + 2e-6, the sum of the kernel's bound and torch's own fp32
  error on the same size pairs (tests/test_mmimg_cpu.py measure_kt; K_t = 54.1 on SIZES -> 8 x 9); 2e-6 where the stored
  size is the load size."""
import csv

import numpy as np
import pytest
import torch

from tests import mmimg_ref as R
from tests.test_mmimg_cpu import CLIP, RESCALE, SIZES, dataset_conf, engine_folder, measure_kt, stored, toy_folder

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
CLIP = dict(CLIP, grey=(0.0, 255.0))                            # an 8-bit (H, W) modality next to the three of the folders
RESCALE = dict(RESCALE, grey=True)


def _taps(n_in, n_out, dev):
    from ganslate_amd.data.multimodal_images import TapTable, bicubic_taps
    host = bicubic_taps(n_in, n_out)
    return TapTable(torch.from_numpy(host.idx).to(dev), torch.from_numpy(host.w).to(dev), n_in, n_out)


def _item(src, H, W, item, c0, name, dev, noise_std=0.0, key=(0, 0)):
    from ganslate_amd.data.device_images import StackItem
    t = torch.from_numpy(src).to(dev)
    return StackItem(t, _taps(src.shape[0], H, dev), _taps(src.shape[1], W, dev), 1 if src.ndim == 2 else src.shape[2], item, c0,
                     *CLIP[name], RESCALE[name], noise_std, key)


def _source(rng, name, h, w):
    if name == "rgb":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if name == "normal":
        return rng.uniform(-1.2, 1.2, size=(h, w, 3)).astype(np.float32)
    if name == "grey":                                          # an 8-bit (H, W) modality, rgb's range
        return rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    return rng.uniform(-0.5, 9.0, size=(h, w)).astype(np.float32)


def _check(out, item, c0, src, name, H, W, noise_std=0.0, key=(0, 0), label=""):
    """out[item, c0 : c0 + c] against the oracle for one descriptor; prints the worst figure in units of the bound"""
    x = R.to_chw(src)
    r, E = R.resize(x, H, W)                                    # float64 weights: the table's two roundings count in the 12
    lo, hi = CLIP[name]
    z = R.noise_plane(H, W, key) if noise_std else None
    want = R.chain(r, lo, hi, RESCALE[name], noise_std, z)
    bound = 12.0 * R.EPS32 * E * R.scale(lo, hi, RESCALE[name]) + 2e-6 + 8e-6 * noise_std
    got = out[item, c0:c0 + x.shape[0]].double().cpu().numpy()
    worst = float(np.max(np.abs(got - want) / bound))
    print(f"{label} {name} {src.shape} -> {(H, W)} std {noise_std}: worst error {worst:.3f} of the bound")
    assert np.all(np.abs(got - want) <= bound), (label, name, worst)
    return got


@pytest.mark.parametrize("src,dst", [((1, 1), (3, 3)), ((2, 3), (8, 9)), ((13, 17), (4, 5)), ((5, 7), (5, 7)), ((3, 20), (2, 257)),
                                     ((6, 300), (4, 257))])
def test_kernel_equals_the_oracle(hip_ops, src, dst):
    """one sample [rgb | normal | grey | depth] (8 channels) behind one dummy channel: uint8 and fp32 sources, (H, W) and
    (H, W, 3) arrays, non-zero channel offsets, a sentinel in every element beforehand"""
    dev = hip_ops.device
    rng = np.random.default_rng(21)
    H, W = dst
    names = ("rgb", "normal", "grey", "depth")
    srcs = {n: _source(rng, n, *src) for n in names}
    out = torch.full((1, 9, H, W), SENTINEL, dtype=torch.float32, device=dev)
    from ganslate_amd.data.device_images import StackItem
    items, c0 = [StackItem(None, None, None, 1, 0, 0)], 1
    offsets = {}
    for n in names:
        items.append(_item(srcs[n], H, W, 0, c0, n, dev))
        offsets[n] = c0
        c0 += items[-1].c
    hip_ops.img_stack(items[::-1], out)                         # the order of the descriptors does not matter
    torch.cuda.synchronize()
    assert not (out == SENTINEL).any() and torch.isfinite(out).all()
    assert not out[0, 0].any()
    for n in names:
        got = _check(out, 0, offsets[n], srcs[n], n, H, W, label=f"{src}")
        if src == dst:                                          # bit for bit the fp32 chain of the stored values
            lo, hi = np.float32(CLIP[n][0]), np.float32(CLIP[n][1])
            v = np.clip(R.to_chw(srcs[n]).astype(np.float32), lo, hi)
            if RESCALE[n]:
                v = np.float32(2.0) * ((v - lo) / (hi - lo)) - np.float32(1.0)
            assert v.dtype == np.float32 and np.array_equal(got.astype(np.float32), v), n


def test_two_samples_of_different_sizes_a_dummy_and_noise_in_one_launch(hip_ops):
    """a val-shaped B batch [3 dummies | depth] next to a train-shaped one: two samples stored at different sizes, noise on
    the rgb of both with different keys"""
    dev = hip_ops.device
    rng = np.random.default_rng(22)
    H, W = 6, 257
    from ganslate_amd.data.device_images import StackItem
    sizes = [(13, 17), (4, 300)]
    keys = [(0x243F6A88, 0x85A308D3), (7, 0xFFFFFFFF)]
    rgb = [_source(rng, "rgb", *s) for s in sizes]
    depth = [_source(rng, "depth", *s) for s in sizes[::-1]]
    out = torch.full((2, 6, H, W), SENTINEL, dtype=torch.float32, device=dev)
    items = []
    for i in range(2):
        items += [_item(rgb[i], H, W, i, 0, "rgb", dev, 0.05, keys[i]), StackItem(None, None, None, 2, i, 3),
                  _item(depth[i], H, W, i, 5, "depth", dev)]
    hip_ops.img_stack(items, out)
    torch.cuda.synchronize()
    assert not (out == SENTINEL).any() and not out[:, 3:5].any()
    for i in range(2):
        _check(out, i, 0, rgb[i], "rgb", H, W, 0.05, keys[i], label=f"sample {i}")
        _check(out, i, 5, depth[i], "depth", H, W, label=f"sample {i}")


def test_noise_plane_is_shared_by_the_channels_and_follows_the_key(hip_ops):
    dev = hip_ops.device
    rng = np.random.default_rng(23)
    H, W = 8, 70
    rgb = rng.integers(40, 216, size=(5, 9, 3), dtype=np.uint8)              # mid-range: few pixels reach the clamp

    def run(std, key):
        out = torch.full((1, 3, H, W), SENTINEL, dtype=torch.float32, device=dev)
        hip_ops.img_stack([_item(rgb, H, W, 0, 0, "rgb", dev, std, key)], out)
        return out[0]

    quiet, a, again, other = run(0.0, (0, 0)), run(0.25, (5, 6)), run(0.25, (5, 6)), run(0.25, (6, 5))
    torch.cuda.synchronize()
    _check(a[None], 0, 0, rgb, "rgb", H, W, 0.25, (5, 6), label="noise")
    assert torch.equal(a, again)                                # the same key: the same bits
    assert not torch.equal(a, other) and (a - other).abs().mean() > 0.05
    d = a.double() - quiet.double()
    free = ((a.abs() < 1.0) & (quiet.abs() < 1.0)).all(0)
    assert free.float().mean() > 0.8
    # v + std * z with one z per pixel: the channels' differences agree up to the rounding of the sum (values below 2)
    assert (d[0] - d[1])[free].abs().max() <= 4 * R.EPS32 and (d[0] - d[2])[free].abs().max() <= 4 * R.EPS32
    z = R.noise_plane(H, W, (5, 6))
    assert np.abs(d[0].cpu().numpy() - 0.25 * z)[free.cpu().numpy()].max() <= 8e-6 * 0.25 + 4 * R.EPS32
    assert a.abs().max() <= 1.0


def test_planar_sources_give_the_bits_of_their_interleaved_form(hip_ops):
    """GsImgStackItem.hwc = 0: the same pixels stored (C, H, W), uint8 and fp32, noise on"""
    dev = hip_ops.device
    rng = np.random.default_rng(25)
    H, W = 7, 66
    for name in ("rgb", "normal"):
        src = _source(rng, name, 9, 11)
        outs = []
        for hwc in (True, False):
            item = _item(src, H, W, 0, 0, name, dev, 0.1, (11, 12))
            if not hwc:
                item = item._replace(src=torch.from_numpy(np.ascontiguousarray(np.moveaxis(src, 2, 0))).to(dev), hwc=False)
            out = torch.full((1, 3, H, W), SENTINEL, dtype=torch.float32, device=dev)
            hip_ops.img_stack([item], out)
            outs.append(out)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and not (outs[0] == SENTINEL).any()
        _check(outs[1], 0, 0, src, name, H, W, 0.1, (11, 12), label="planar")


def test_bad_tables_are_refused_before_the_launch(hip_ops):
    from ganslate_amd.data.device_images import StackItem
    from ganslate_amd.hip import lib as L
    dev = hip_ops.device
    rng = np.random.default_rng(24)
    rgb = _source(rng, "rgb", 5, 7)
    out = torch.full((1, 4, 8, 9), SENTINEL, dtype=torch.float32, device=dev)
    with pytest.raises(L.HipError, match="channel 3 of batch item 0 is written by no descriptor"):
        hip_ops.img_stack([_item(rgb, 8, 9, 0, 0, "rgb", dev)], out)
    with pytest.raises(L.HipError, match="written twice"):
        hip_ops.img_stack([_item(rgb, 8, 9, 0, 0, "rgb", dev), StackItem(None, None, None, 2, 0, 2)], out)
    with pytest.raises(AssertionError):
        hip_ops.img_stack([_item(rgb, 8, 10, 0, 0, "rgb", dev), StackItem(None, None, None, 1, 0, 3)], out)       # tables of another W
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                              # nothing was launched


# ---- the pipeline ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,load", [("train", (8, 9)), ("val", (8, 9)), ("infer", (8, 9)), ("val", (5, 7))])
def test_pipeline_batches_equal_the_host_datasets(hip_ops, tmp_path, mode, load):
    from torch.utils.data import DataLoader
    from ganslate_amd.data import MultiModalImageDataset, MultiModalImageValTestDataset
    from ganslate_amd.data.device_images import DeviceMultiModalImagePipeline
    identity = load == (5, 7)
    sizes = [(5, 7)] * 3 if identity else SIZES
    root = toy_folder(tmp_path / "data", sizes=sizes)
    cls = MultiModalImageDataset if mode == "train" else MultiModalImageValTestDataset
    kw = {} if mode == "train" else dict(dummy_channels_B=[3, 0])
    host = cls(dataset_conf(root, mode, load=load, **kw))
    raw = cls(dataset_conf(root, mode, load=load, device_transforms=True, **kw))
    pipe = raw.device_pipeline(None, hip_ops.device)
    assert isinstance(pipe, DeviceMultiModalImagePipeline)
    pipe._ops = hip_ops
    kt = 0.0 if identity else measure_kt([(s, load) for s in sizes])
    print(f"{mode} {load}: K_t = {kt:.2f}")
    n = len(sizes)
    want = next(iter(DataLoader(host, batch_size=n)))
    domains = {"A": ("rgb", "normal")} if mode == "infer" else {"A": ("rgb", "normal"), "B": ("rgb", "depth") if mode == "train" else ("depth",)}
    for _ in range(2):
        got = pipe(next(iter(DataLoader(raw, batch_size=n, collate_fn=raw.collate_fn))))
        assert set(got) == set(want)
        for key, names in domains.items():
            g = got[key]
            assert g.is_cuda and g.is_contiguous() and g.dtype == torch.float32 and g.shape == want[key].shape
            c = 3 if (key == "B" and mode != "train") else 0
            assert not g[:, :c].any()
            for name in names:
                lo, hi = CLIP[name]
                for k in range(n):
                    x = R.to_chw(stored(root, name, k))
                    _, E = R.resize(x, *load)
                    bound = (12.0 + kt) * R.EPS32 * E * R.scale(lo, hi, RESCALE[name]) + 2e-6 if not identity else 2e-6
                    diff = np.abs(g[k, c:c + x.shape[0]].double().cpu().numpy() - want[key][k, c:c + x.shape[0]].double().numpy())
                    assert np.all(diff <= bound), (key, name, k, float(np.max(diff / bound)))
                c += 3 if name != "depth" else 1
        if mode != "train":
            assert got["metadata"] == want["metadata"]
    files = n * (2 if mode == "infer" else 3)
    assert pipe.uploads == files == len(pipe.resident) and all(t.is_cuda for t in pipe.resident.values())


# ---- the engines -------------------------------------------------------------------------------------------------------------
def _engine_args(tmp_path, yaml, *modes):
    if not (tmp_path / "data").is_dir():
        engine_folder(tmp_path / "data")
    args = [f"config=tests/configs/{yaml}", f"train.output_dir={tmp_path / 'out'}", "train.seed=5", "train.checkpointing.freq=2"]
    for mode in ("train",) + modes:
        args += [f"{mode}.dataset.root={tmp_path / 'data'}", f"{mode}.dataset.device_transforms=true"]
    for mode in modes:
        args.append(f"{mode}.output_dir={tmp_path / 'out'}")
    return args


@pytest.mark.parametrize("yaml,channels_B", [("cyclegan_balanced_mmimg_val.yaml", 4), ("pix2pix_mmimg_val.yaml", 1)])
def test_engines_on_the_device_pipeline(hip_ops, tmp_path, yaml, channels_B):
    """three training iterations with a validation at iteration 2, then the Tester on the checkpoint of iteration 2: metric
    rows, one saved depth map per sample id in the stored (H, W) form, one image grid per sample"""
    from ganslate_amd.data.device_images import DeviceMultiModalImagePipeline
    from ganslate_amd.engines import init_engine
    args = _engine_args(tmp_path, yaml, "val", "test")
    tr = init_engine("train", args)
    assert isinstance(tr.input_pipeline, DeviceMultiModalImagePipeline)
    tr.run()
    v = tr.validator
    loader = next(iter(v.data_loaders.values()))
    assert isinstance(v.input_pipeline(loader), DeviceMultiModalImagePipeline)
    assert [h[0] for h in v.history] == [2]
    rows = v.samples[None]
    assert len(rows) == 4 and all({"ssim", "mse", "nmse", "psnr", "mae"} <= set(r) for r in rows)
    assert all(np.isfinite(x) for r in rows for x in r.values())
    ids = [f"{k:09d}" for k in range(4)]
    for sample_id in ids:
        saved = np.load(tmp_path / "out" / "val" / "saved" / "2" / f"{sample_id}.npy")
        assert saved.shape == (64, 96) and saved.dtype == np.float32 and np.isfinite(saved).all()
        assert saved.min() >= 0.0 and saved.max() <= 8.0
    pngs = sorted((tmp_path / "out" / "val" / "images" / "2").glob("*.png"))
    assert len(pngs) == 4, sorted(str(p) for p in (tmp_path / "out").rglob("*.png"))
    assert tr.input_pipeline.uploads == len(tr.input_pipeline.resident) <= 12       # every file at most once in three iterations
    te = init_engine("test", args + [f"train.output_dir={tmp_path / 'elsewhere'}", "test.checkpointing.load_iter=2"])
    assert te.on_device
    te.run()
    with open(tmp_path / "out" / "test" / "metrics.csv", newline="") as f:
        got = list(csv.DictReader(f))
    assert len(got) == 4 and [r["sample"] for r in got] == ["0", "1", "2", "3"]
    assert {"mae", "ssim", "psnr"} <= set(got[0]) and all(np.isfinite(float(r[k])) for r in got for k in r)
    assert sorted(p.name for p in (tmp_path / "out" / "test" / "saved").iterdir()) == [f"{i}.npy" for i in ids]
    assert len(list((tmp_path / "out" / "test" / "images").glob("*.png"))) == 4
