"""MultiModalVolumeValTestDataset on the host (data/multimodal_valtest.py): samples against the expressions of the module's
docstring written out in numpy / torch, the three `generate_body_mask` modes, dummy channels, `supply_masks`, `infer`
mode, `denormalize`, the `save` round trip, the YAML surface of both new configs, the raw (device_transforms) samples, the
device pipeline's control flow on reference ops, and a Validator run on the host path. Values: the sample is built with the
same torch calls on the same fp32 inputs as the expressions here, so images are compared with 2e-6 absolute on [-1, 1]
(a last-ulp difference of one division, as in tests/test_mmvol_cpu.py); masks, shapes and metadata are exact."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import bodymask_ref as B
from tests.test_mmvol_cpu import _D, toy_folder

ROOT = Path(__file__).resolve().parent.parent
CLIP = {"pet": (0.0, 6.0), "ct": (-1000.0, 2000.0), "hx4": (0.0, 3.0)}
OUTSIDE = {"pet": 0.0, "ct": -1024.0, "hx4": 0.0}
MISSING = "case1"                       # the case without a body mask file


def valtest_folder(root, n=3, shape=(12, 20, 24)):
    """toy_folder's cases (A and B of one shape) plus a GTV mask each; case1 loses its body mask and gets a CT with air
    around an ellipsoid body and an air cavity inside it, so that the generated mask has a hole to fill"""
    div = toy_folder(root, n=n, shape=shape, shape_B=shape)
    rng = np.random.default_rng(17)
    for k in range(n):
        gtv = np.zeros(shape, np.uint8)
        c = [s // 2 + k - 1 for s in shape]
        gtv[c[0] - 2:c[0] + 2, c[1] - 3:c[1] + 3, c[2] - 4:c[2] + 4] = 1
        np.save(root / f"case{k}" / "gtv.npy", gtv)
    g = np.meshgrid(*[(np.arange(s) - (s - 1) / 2) / (0.42 * s) for s in shape], indexing="ij")
    r2 = g[0] ** 2 + g[1] ** 2 + g[2] ** 2
    ct = np.where(r2 <= 1.0, rng.integers(-250, 300, size=shape), rng.integers(-1100, -700, size=shape))
    ct = np.where(r2 <= 0.05, -950, ct).astype(np.int16)
    np.save(root / MISSING / "ct.npy", ct)
    (root / MISSING / "body.npy").unlink()
    return div


def dataset_conf(root, mode="val", **kw):
    ds = _D(root=str(root), modalities=_D(A=["pet", "ct"], B=["hx4"]), body_mask="body", masks=_D(BODY="body", GTV="gtv"),
            supply_masks=True, clip_range=_D({k: list(v) for k, v in CLIP.items()}), outside_value=_D(OUTSIDE), divisors=None,
            pad_to=None, generate_body_mask="missing", body_mask_from="ct", body_mask_threshold=-300.0, dummy_channels_B=[0, 0],
            denormalize_modality=None, device_transforms=False)
    ds.update(kw)
    return _D({"mode": mode, mode: _D(dataset=ds)})


def expected_sample(root, case, divisors, pad_to, generate="missing"):
    """the module docstring's steps 1-4 for one case"""
    from ganslate_amd.data.utils.normalization import min_max_normalize
    folder = Path(root) / case
    have = (folder / "body.npy").is_file() and generate != "always"
    body = (np.load(folder / "body.npy") != 0).astype(np.uint8) if have else B.body_mask(np.load(folder / "ct.npy"), -300)[0]
    target = pad_to or body.shape
    widths = B.pad_widths(body.shape, target)
    out = {}
    for name in ("pet", "ct", "hx4"):
        x = np.where(body != 0, np.load(folder / f"{name}.npy").astype(np.float32), np.float32(OUTSIDE[name])).astype(np.float32)
        x = torch.from_numpy(np.pad(x, widths, "constant", constant_values=x.min()))
        x = x / float(divisors.get(name, {}).get(case, 1.0))
        out[name] = min_max_normalize(torch.clamp(x, *CLIP[name]), *CLIP[name])
    gtv = (np.load(folder / "gtv.npy") != 0).astype(np.uint8)
    masks = {"BODY": np.pad(body, widths, "constant", constant_values=body.min()),
             "GTV": np.pad(gtv, widths, "constant", constant_values=gtv.min())}
    return out, masks, body, [w[0] for w in widths]


@pytest.mark.parametrize("pad_to", [None, (16, 20, 29), (8, 16, 16)])
def test_host_samples_equal_the_stated_expressions(tmp_path, pad_to):
    from ganslate_amd.data import MultiModalVolumeValTestDataset
    div = valtest_folder(tmp_path / "data")
    ds = MultiModalVolumeValTestDataset(dataset_conf(tmp_path / "data", divisors=div, pad_to=pad_to))
    assert len(ds) == 3 and ds.collate_fn is None and ds.device_pipeline(None, "cpu") is None
    divisors = json.loads(Path(div).read_text())
    assert divisors["hx4"] == {"case1": 1.5}
    for i, case in enumerate(("case0", "case1", "case2")):
        want, masks, body, before = expected_sample(tmp_path / "data", case, divisors, pad_to)
        s = ds[i]
        assert list(s) == ["A", "B", "masks", "metadata"]
        shape = tuple(max(a, b) for a, b in zip((12, 20, 24), pad_to or (0, 0, 0)))
        assert s["A"].shape == (2, *shape) and s["B"].shape == (1, *shape) and s["A"].dtype == s["B"].dtype == torch.float32
        for c, name in enumerate(("pet", "ct")):
            assert torch.allclose(s["A"][c], want[name], atol=2e-6, rtol=0), (case, name)
        assert torch.allclose(s["B"][0], want["hx4"], atol=2e-6, rtol=0)
        assert float(s["A"].min()) >= -1.0 and float(s["A"].max()) <= 1.0
        assert list(s["masks"]) == ["BODY", "GTV"]
        for label in ("BODY", "GTV"):
            m = s["masks"][label]
            assert m.dtype == torch.uint8 and m.shape == (1, *shape) and np.array_equal(m[0].numpy(), masks[label])
        assert s["metadata"] == {"case": case, "size": [12, 20, 24], "pad_before": before}
        if case == MISSING:                                    # generated: filled cavity, nothing of the air around
            assert body[6, 10, 12] == 1 and np.load(tmp_path / "data" / case / "ct.npy")[6, 10, 12] == -950
            assert body[0, 0, 0] == 0 and 0.2 < body.mean() < 0.5


def test_generate_body_mask_modes(tmp_path):
    from ganslate_amd.data import MultiModalVolumeValTestDataset
    from ganslate_amd.data.utils.body_mask import get_body_mask
    div = valtest_folder(tmp_path / "data")
    root = tmp_path / "data"
    never = MultiModalVolumeValTestDataset(dataset_conf(root, divisors=div, generate_body_mask="never", body_mask_from=None))
    assert never[0]["A"].shape == (2, 12, 20, 24)
    with pytest.raises(FileNotFoundError, match="case1"):
        never[1]
    always = MultiModalVolumeValTestDataset(dataset_conf(root, divisors=div, generate_body_mask="always"))
    for i in range(3):
        ct = np.load(root / f"case{i}" / "ct.npy")
        assert np.array_equal(always[i]["masks"]["BODY"][0].numpy(), get_body_mask(ct, -300))
        assert np.array_equal(always[i]["masks"]["BODY"][0].numpy(), B.body_mask(ct, -300)[0])
    missing = MultiModalVolumeValTestDataset(dataset_conf(root, divisors=div))
    assert np.array_equal(missing[0]["masks"]["BODY"][0].numpy(), np.load(root / "case0" / "body.npy"))
    assert not np.array_equal(always[0]["masks"]["BODY"][0].numpy(), np.load(root / "case0" / "body.npy"))
    assert torch.equal(missing[1]["masks"]["BODY"], always[1]["masks"]["BODY"])
    np.save(root / "case1" / "ct.npy", np.full((12, 20, 24), -900, np.int16))               # no body at all
    with pytest.raises(ValueError, match="case1"):
        MultiModalVolumeValTestDataset(dataset_conf(root, divisors=div))[1]
    for bad in (dict(generate_body_mask="sometimes"), dict(body_mask_from="hx4"), dict(body_mask_from=None),
                dict(pad_to=[8, 8]), dict(dummy_channels_B=[1]), dict(denormalize_modality="pet"),
                dict(clip_range=_D(pet=[0.0, 6.0]))):
        with pytest.raises(ValueError):
            MultiModalVolumeValTestDataset(dataset_conf(root, divisors=div, **bad))


def test_dummy_channels_masks_switch_and_infer_mode(tmp_path):
    from ganslate_amd.data import MultiModalVolumeValTestDataset
    div = valtest_folder(tmp_path / "data")
    root = tmp_path / "data"
    plain = MultiModalVolumeValTestDataset(dataset_conf(root, divisors=div))[2]
    for before, after in ((0, 1), (3, 0), (1, 2)):
        s = MultiModalVolumeValTestDataset(dataset_conf(root, divisors=div, dummy_channels_B=[before, after]))[2]
        assert s["B"].shape == (before + 1 + after, 12, 20, 24)
        assert torch.equal(s["B"][before], plain["B"][0]) and torch.equal(s["A"], plain["A"])
        assert not s["B"][:before].any() and not s["B"][before + 1:].any()
    s = MultiModalVolumeValTestDataset(dataset_conf(root, divisors=div, supply_masks=False))[2]
    assert list(s) == ["A", "B", "metadata"]
    s = MultiModalVolumeValTestDataset(dataset_conf(root, mode="infer", divisors=div))[1]
    assert list(s) == ["A", "metadata"] and torch.equal(s["A"], MultiModalVolumeValTestDataset(
        dataset_conf(root, divisors=div))[1]["A"])
    s = MultiModalVolumeValTestDataset(dataset_conf(root, mode="test", divisors=div))[0]
    assert list(s) == ["A", "B", "masks", "metadata"]


def test_denormalize_is_in_place_and_save_round_trips(tmp_path):
    from ganslate_amd.data import MultiModalVolumeValTestDataset
    from ganslate_amd.utils.io import decollate
    from torch.utils.data import DataLoader
    div = valtest_folder(tmp_path / "data")
    root = tmp_path / "data"
    ds = MultiModalVolumeValTestDataset(dataset_conf(root, divisors=div, pad_to=(16, 20, 29), dummy_channels_B=[1, 1]))
    t = torch.tensor([-1.0, 0.0, 1.0])
    assert ds.denormalize(t) is t and t.tolist() == [0.0, 1.5, 3.0]                          # hx4's range, B's first
    batch = next(iter(DataLoader(ds, batch_size=3)))
    assert batch["B"].shape == (3, 3, 16, 20, 29) and batch["masks"]["GTV"].shape == (3, 1, 16, 20, 29)
    metas = decollate(batch["metadata"], batch_size=3)
    assert metas[1] == {"case": "case1", "size": [12, 20, 24], "pad_before": [2, 0, 2]}
    for i, case in enumerate(("case0", "case1", "case2")):
        keep = batch["B"][i].clone()
        for tensor in (batch["B"][i], batch["B"][i][1:2]):       # with the dummies, and the translated channel alone
            path = ds.save(tensor=tensor, save_dir=tmp_path / "saved", metadata=metas[i])
            assert path == tmp_path / "saved" / f"{case}.npy"
            got = np.load(path)
            body = ds.host_body_mask(i)
            orig = np.where(body != 0, np.clip(np.load(root / case / "hx4.npy") / ds.divisor("hx4", i), 0.0, 3.0), 0.0)
            orig = orig * ds.divisor("hx4", i)
            assert got.dtype == np.float32 and got.shape == (12, 20, 24)
            assert np.allclose(got, orig, atol=1e-5, rtol=0)
        assert torch.equal(batch["B"][i], keep)                  # save denormalises a copy
    assert ds.divisor("hx4", 1) == 1.5


@pytest.mark.parametrize("yaml,channels_B", [("pix2pix3d_mmvol_val.yaml", 1), ("cyclegan_balanced_mmvol_val.yaml", 2)])
def test_dataset_through_the_builders(tmp_path, yaml, channels_B):
    from ganslate_amd.data import MultiModalVolumeDataset, MultiModalVolumeValTestDataset
    from ganslate_amd.utils.builders import build_conf, build_loader
    div = valtest_folder(tmp_path / "data", shape=(12, 36, 40))
    args = [f"config=tests/configs/{yaml}"]
    for mode in ("train", "val", "test"):
        args += [f"{mode}.dataset.root={tmp_path / 'data'}", f"{mode}.dataset.divisors={div}"]
    conf = build_conf(args)
    for mode in ("val", "test"):
        conf.mode = mode
        loader = build_loader(conf)
        ds = loader.dataset
        assert isinstance(ds, MultiModalVolumeValTestDataset) and not isinstance(ds, MultiModalVolumeDataset)
        assert ds.raw is False and ds.pad_to == (32, 32, 32) and ds.dummy_channels_B == (0, channels_B - 1)
        assert list(conf[mode].sliding_window.window_size) == list(conf.train.dataset.patch_size)
        batch = next(iter(loader))
        assert batch["A"].shape == (1, 2, 32, 36, 40) and batch["B"].shape == (1, channels_B, 32, 36, 40)
        assert ("masks" in batch) == (channels_B == 1) == ds.supply_masks and batch["metadata"]["case"] == ["case0"]
        assert list(ds.masks) == ["BODY", "GTV"]


def test_the_new_dataset_passes_the_engines_device_path_check(tmp_path):
    """engines/base.py refuses the two TRAINING volume datasets outside training; this one has `raw` and `device_pipeline`
    and is no subclass of either, so it gets its pipeline"""
    from ganslate_amd.data import MultiModalVolumeValTestDataset
    from ganslate_amd.data.device_volumes import DeviceWholeVolumePipeline
    from ganslate_amd.engines.base import BaseEngineWithInference
    div = valtest_folder(tmp_path / "data")
    engine = type("Engine", (BaseEngineWithInference,), {"_set_mode": lambda self: None})
    for flag in (True, False):
        ds = MultiModalVolumeValTestDataset(dataset_conf(tmp_path / "data", divisors=div, device_transforms=flag))
        eng = engine.__new__(engine)
        eng.conf = type("C", (), {"mode": "val"})()
        eng._input_pipelines = {}
        eng.model = type("M", (), {"device": torch.device("cpu")})()
        pipe = eng.input_pipeline(type("L", (), {"dataset": ds})())
        assert isinstance(pipe, DeviceWholeVolumePipeline) if flag else pipe is None


class RefWholeOps:
    """HipOps.body_mask / volume_prepare on CPU tensors through tests/bodymask_ref.py"""

    def __init__(self):
        self.body_mask_calls = 0

    def body_mask(self, volume, threshold, out=None):
        self.body_mask_calls += 1
        mask, info = B.body_mask(volume.numpy(), threshold)
        return torch.from_numpy(mask), torch.tensor(info, dtype=torch.int32)

    def volume_prepare(self, volumes, mask, extra_masks, target, outside, divisor, lo, hi, out=None, masks_out=None):
        got, masks = B.volume_prepare([v.numpy() for v in volumes], mask.numpy(), [m.numpy() for m in extra_masks], target,
                                      outside, divisor, lo, hi)
        out.copy_(torch.from_numpy(got))
        for dst, m in zip(masks_out, masks):
            dst.copy_(torch.from_numpy(m))
        return out, masks_out


@pytest.mark.parametrize("mode", ["val", "infer"])
def test_raw_samples_and_pipeline_on_reference_ops_equal_the_host_path(tmp_path, mode):
    from ganslate_amd.data import MultiModalVolumeValTestDataset
    from ganslate_amd.data.device_volumes import DeviceWholeVolumePipeline
    from ganslate_amd.data.multimodal_valtest import RawWholeCase, collate_raw
    from torch.utils.data import DataLoader
    div = valtest_folder(tmp_path / "data")
    kw = dict(divisors=div, pad_to=(16, 20, 29), dummy_channels_B=[0, 1])
    host = MultiModalVolumeValTestDataset(dataset_conf(tmp_path / "data", mode=mode, **kw))
    raw = MultiModalVolumeValTestDataset(dataset_conf(tmp_path / "data", mode=mode, device_transforms=True, **kw))
    assert raw.collate_fn is collate_raw and isinstance(raw.device_pipeline(None, "cpu"), DeviceWholeVolumePipeline)
    s = raw[1]
    assert isinstance(s["A"], RawWholeCase) and s["A"].index == 1 and s["metadata"] == host[1]["metadata"]
    ops = RefWholeOps()
    pipe = DeviceWholeVolumePipeline(raw, "cpu", ops=ops)
    want = next(iter(DataLoader(host, batch_size=3)))
    for _ in range(2):
        got = pipe(next(iter(DataLoader(raw, batch_size=3, collate_fn=raw.collate_fn))))
        assert list(got) == list(want) or set(got) == set(want)
        for key in ("A", "B") if mode == "val" else ("A",):
            assert got[key].shape == want[key].shape and got[key].is_contiguous()
            assert torch.allclose(got[key], want[key], atol=2e-6, rtol=0), key
        if mode == "val":
            assert list(got["masks"]) == ["BODY", "GTV"]
            for label in got["masks"]:
                assert got["masks"][label].dtype == torch.uint8 and torch.equal(got["masks"][label], want["masks"][label])
        else:
            assert "B" not in got and "masks" not in got
        assert got["metadata"]["case"] == want["metadata"]["case"]
        assert all(torch.equal(a, b) for a, b in zip(got["metadata"]["size"], want["metadata"]["size"]))
    assert ops.body_mask_calls == 1                               # the generated mask stays resident
    mixed = MultiModalVolumeValTestDataset(dataset_conf(tmp_path / "data", mode=mode, device_transforms=True, divisors=div))
    np.save(tmp_path / "data" / "case2" / "pet.npy", np.zeros((12, 20, 26), np.float32))
    for name in ("ct", "hx4", "body", "gtv"):
        np.save(tmp_path / "data" / "case2" / f"{name}.npy", np.zeros((12, 20, 26), np.int16 if name == "ct" else np.uint8))
    pipe = DeviceWholeVolumePipeline(mixed, "cpu", ops=RefWholeOps())
    with pytest.raises(ValueError, match="pad_to.*batch_size: 1"):
        pipe(collate_raw([mixed[1], mixed[2]]))


@pytest.fixture()
def fp32_oracle_backend():
    from ganslate_amd.nn.native import backend
    from oracle.ops_ref import RefOps
    backend.set_ops(RefOps(act_dtype=torch.float32))
    yield
    backend.set_ops(None)


def test_validator_runs_on_the_host_path(fp32_oracle_backend, tmp_path):
    from ganslate_amd.data import MultiModalVolumeValTestDataset
    from ganslate_amd.engines import init_engine
    div = valtest_folder(tmp_path / "data", shape=(12, 36, 40))
    args = ["config=tests/configs/pix2pix3d_mmvol_val.yaml", "train.cuda=false", f"train.output_dir={tmp_path / 'out'}",
            f"val.output_dir={tmp_path / 'out'}", "train.seed=3"]
    for mode in ("train", "val"):
        args += [f"{mode}.dataset.root={tmp_path / 'data'}", f"{mode}.dataset.divisors={div}"]
    tr = init_engine("train", args)
    v = tr.validator
    loader = next(iter(v.data_loaders.values()))
    assert isinstance(loader.dataset, MultiModalVolumeValTestDataset) and v.input_pipeline(loader) is None
    shapes = []
    infer = tr.model.infer
    tr.model.infer = lambda x, *a, **k: (shapes.append(tuple(x.shape)), infer(x, *a, **k))[1]
    v.run(current_idx=0)
    assert shapes and all(s[1:] == (2, 32, 32, 32) for s in shapes)
    assert len(v.samples[None]) == 3
    for row in v.samples[None]:
        assert set(row) == {"mae", "mse", "nmse", "psnr"} and all(np.isfinite(x) for x in row.values())
    saved = sorted(p.name for p in (tmp_path / "out" / "val" / "saved" / "0").iterdir())
    assert saved == ["case0.npy", "case1.npy", "case2.npy"]
    assert np.load(tmp_path / "out" / "val" / "saved" / "0" / "case1.npy").shape == (12, 36, 40)
