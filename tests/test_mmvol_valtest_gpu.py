"""MultiModalVolumeValTestDataset on the GPU: DeviceWholeVolumePipeline's batches (gs_body_mask + gs_volume_prepare on
resident volumes) against the host dataset's for the same folder — images within 2e-6 absolute on [-1, 1] (the tolerance
tests/test_mmvol_gpu.py sets for the same chain: a last-ulp difference of one division), masks exactly, the generated body
mask included — then the Validator and the Tester on the two new configs with sliding windows."""
import csv

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from tests.test_mmvol_valtest_cpu import MISSING, dataset_conf, valtest_folder

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode,pad_to,dummies", [("val", (16, 20, 29), (0, 1)), ("test", None, (0, 0)), ("infer", (8, 33, 24), (2, 0))])
def test_pipeline_batches_equal_the_host_datasets(hip_ops, tmp_path, mode, pad_to, dummies):
    from ganslate_amd.data import MultiModalVolumeValTestDataset
    from ganslate_amd.data.device_volumes import DeviceWholeVolumePipeline
    div = valtest_folder(tmp_path / "data")
    kw = dict(mode=mode, divisors=div, pad_to=pad_to, dummy_channels_B=list(dummies))
    host = MultiModalVolumeValTestDataset(dataset_conf(tmp_path / "data", **kw))
    raw = MultiModalVolumeValTestDataset(dataset_conf(tmp_path / "data", device_transforms=True, **kw))
    pipe = DeviceWholeVolumePipeline(raw, hip_ops.device, ops=hip_ops)
    calls = []
    body_mask = hip_ops.body_mask
    pipe._ops = type("Counting", (), {"body_mask": lambda self, *a, **k: (calls.append(1), body_mask(*a, **k))[1],
                                      "volume_prepare": staticmethod(hip_ops.volume_prepare)})()
    want = next(iter(DataLoader(host, batch_size=3)))
    for _ in range(2):
        got = pipe(next(iter(DataLoader(raw, batch_size=3, collate_fn=raw.collate_fn))))
        assert set(got) == set(want)
        for key in ("A", "B") if mode != "infer" else ("A",):
            assert got[key].is_cuda and got[key].is_contiguous() and got[key].dtype == torch.float32
            assert got[key].shape == want[key].shape
            assert torch.allclose(got[key].cpu(), want[key], atol=2e-6, rtol=0), key
        if mode != "infer":
            assert list(got["masks"]) == ["BODY", "GTV"]
            for label, m in got["masks"].items():
                assert m.is_cuda and m.dtype == torch.uint8 and torch.equal(m.cpu(), want["masks"][label]), label
        assert got["metadata"]["case"] == ["case0", "case1", "case2"]
    assert len(calls) == 1                                        # the generated mask of case1 stays resident
    assert (None, 1) in pipe.resident and all(t.is_cuda for t in pipe.resident.values())


def test_pipeline_errors_name_the_case_and_the_remedy(hip_ops, tmp_path):
    from ganslate_amd.data import MultiModalVolumeValTestDataset
    from ganslate_amd.data.multimodal_valtest import collate_raw
    div = valtest_folder(tmp_path / "data")
    root = tmp_path / "data"
    for name in ("pet", "ct", "hx4", "body", "gtv"):
        np.save(root / "case2" / f"{name}.npy", np.zeros((12, 20, 26), {"ct": np.int16, "body": np.uint8, "gtv": np.uint8}.get(
            name, np.float32)))
    raw = MultiModalVolumeValTestDataset(dataset_conf(root, device_transforms=True, divisors=div))
    pipe = raw.device_pipeline(None, hip_ops.device)
    with pytest.raises(ValueError, match="pad_to.*batch_size: 1"):
        pipe(collate_raw([raw[0], raw[2]]))
    assert pipe(collate_raw([raw[2]]))["A"].shape == (1, 2, 12, 20, 26)
    np.save(root / MISSING / "ct.npy", np.full((12, 20, 24), -900, np.int16))                # no body at all
    with pytest.raises(ValueError, match=MISSING):
        pipe(collate_raw([raw[1]]))


def _engine_args(tmp_path, yaml, div, *modes):
    """training patches of 32^3 come from a folder of larger cases; validation and test read the (12, 40, 48) folder"""
    from tests.test_mmvol_cpu import toy_folder
    if not (tmp_path / "train").is_dir():
        toy_folder(tmp_path / "train", shape=(36, 40, 38), shape_B=(34, 44, 40))
    args = [f"config=tests/configs/{yaml}", f"train.output_dir={tmp_path / 'out'}", "train.seed=5", "train.checkpointing.freq=2",
            f"train.dataset.root={tmp_path / 'train'}", f"train.dataset.divisors={tmp_path / 'train_divisors.json'}"]
    for mode in modes:
        args += [f"{mode}.dataset.root={tmp_path / 'data'}", f"{mode}.dataset.divisors={div}"]
    for mode in modes:
        args += [f"{mode}.output_dir={tmp_path / 'out'}", f"{mode}.dataset.device_transforms=true"]
    return args


def test_validator_on_the_device_pipeline_with_sliding_windows(hip_ops, tmp_path):
    """pix2pix3d_mmvol_val.yaml on three cases of (12, 40, 48), case1 without a body mask: D is padded to the 32^3 window,
    every case is translated window by window, scored as a whole and inside BODY and GTV, saved without its padding and
    logged as a PNG"""
    from ganslate_amd.data.device_volumes import DeviceWholeVolumePipeline
    from ganslate_amd.engines import init_engine
    div = valtest_folder(tmp_path / "data", shape=(12, 40, 48))
    tr = init_engine("train", _engine_args(tmp_path, "pix2pix3d_mmvol_val.yaml", div, "val"))
    tr.run()
    v = tr.validator
    loader = next(iter(v.data_loaders.values()))
    assert isinstance(v.input_pipeline(loader), DeviceWholeVolumePipeline)
    assert [h[0] for h in v.history] == [2]
    rows = v.samples[None]
    names = ["ssim", "mse", "nmse", "psnr", "mae"]
    assert len(rows) == 3
    for row in rows:
        assert set(row) == set(names + [f"{k}_{label}" for label in ("BODY", "GTV") for k in names])
        assert all(np.isfinite(x) for x in row.values())
        assert row["mae_GTV"] != row["mae"]
    for case in ("case0", "case1", "case2"):
        saved = np.load(tmp_path / "out" / "val" / "saved" / "2" / f"{case}.npy")
        assert saved.shape == (12, 40, 48) and saved.dtype == np.float32 and np.isfinite(saved).all()
    pngs = sorted((tmp_path / "out" / "val" / "images" / "2").glob("*.png"))
    assert len(pngs) == 3, sorted(str(p) for p in (tmp_path / "out").rglob("*.png"))


def test_tester_on_the_balanced_config_writes_one_row_per_case(hip_ops, tmp_path):
    from ganslate_amd.engines import init_engine
    div = valtest_folder(tmp_path / "data", shape=(12, 40, 48))
    args = _engine_args(tmp_path, "cyclegan_balanced_mmvol_val.yaml", div, "val", "test")
    tr = init_engine("train", args + ["val.freq=1000"])
    tr.run()
    te = init_engine("test", args + [f"train.output_dir={tmp_path / 'elsewhere'}", "test.checkpointing.load_iter=2"])
    assert te.on_device
    te.run()
    with open(tmp_path / "out" / "test" / "metrics.csv", newline="") as f:
        got = list(csv.DictReader(f))
    assert len(got) == 3 and [r["sample"] for r in got] == ["0", "1", "2"]
    assert {"mae", "ssim", "psnr"} <= set(got[0]) and "mae_BODY" not in got[0]     # the config leaves supply_masks off
    assert all(np.isfinite(float(r[k])) for r in got for k in r)
    assert sorted(p.name for p in (tmp_path / "out" / "test" / "saved").iterdir()) == ["case0.npy", "case1.npy", "case2.npy"]
