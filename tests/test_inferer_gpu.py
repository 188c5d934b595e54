"""The output side of the engines on the GPU, end to end: a 2-iteration training run writes `train/images/{iter}_*.png`
and a checkpoint; the Inferer loads it and writes one `images/{idx}_input-output.png` and one `saved/*.npy` per sample; the
Tester writes one mid-slice PNG per sample next to its metrics.csv. Decoded pixels are compared bit for bit with the oracle
of tests/visgrid_ref.py applied to the tensors the engines held. Two configs: 2-D (Resnet2D, 32x32, batch 2) and 3-D (the
networks of cyclegan3d_test_synthetic.yaml, sliding window)."""
import csv
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from tests import visgrid_ref as R

pytestmark = pytest.mark.gpu

CONFIGS = Path(__file__).resolve().parent / "configs"
TRAIN_NAMES = "real_A-fake_B-rec_A-real_B-fake_A-rec_B"


def _png(path):
    return torch.from_numpy(np.asarray(Image.open(path)).copy())


_RUNS = {}


def _trained(config, tmp_path_factory):
    """a training run of 2 iterations with a checkpoint at 2 (once per config); the visuals the model held at each
    logging time"""
    if config in _RUNS:
        return _RUNS[config]
    from ganslate_amd.engines import init_engine
    out = tmp_path_factory.mktemp(config.split("_")[0])
    args = [f"config={CONFIGS / config}", f"train.output_dir={out}", f"infer.output_dir={out}", "train.seed=7"]
    if "3d" in config:
        args.append(f"test.output_dir={out}")
    tr = init_engine("train", args)
    held = {}
    log_visuals = tr._log_visuals

    def recording(visuals):
        torch.cuda.synchronize()
        held[tr.iter_idx] = {k: v.detach().float().cpu().clone() for k, v in visuals.items() if v is not None}
        log_visuals(visuals)

    tr._log_visuals = recording
    tr.run()
    assert (out / "checkpoints" / "2.pth").is_file()
    _RUNS[config] = (out, args, held, "3d" in config)
    return _RUNS[config]


@pytest.fixture(scope="module", params=["infer2d_synthetic.yaml", "infer3d_synthetic.yaml"])
def run(request, hip_ops, tmp_path_factory):
    return _trained(request.param, tmp_path_factory)


@pytest.fixture(scope="module")
def run3d(hip_ops, tmp_path_factory):
    return _trained("infer3d_synthetic.yaml", tmp_path_factory)


def test_training_writes_the_first_example_at_every_logging_iteration(run):
    out, _, held, three_d = run
    images = out / "train" / "images"
    assert sorted(p.name for p in images.iterdir()) == [f"1_{TRAIN_NAMES}.png", f"2_{TRAIN_NAMES}.png"]
    assert (out / "train" / "train_config.yaml").is_file()
    for it in (1, 2):
        name, want = R.grid_ref(held[it], single_example=True)
        assert name == TRAIN_NAMES
        got = _png(images / f"{it}_{name}.png")
        assert got.shape == ((16 * 16, 6 * 16, 3) if three_d else (32, 6 * 32, 3))
        assert torch.equal(got, want[0]), f"iteration {it}: {int((got != want[0]).sum())} bytes differ"
    assert not torch.equal(_png(images / f"1_{TRAIN_NAMES}.png"), _png(images / f"2_{TRAIN_NAMES}.png"))


def test_inferer_writes_one_image_and_one_saved_tensor_per_sample(run):
    from ganslate_amd.engines import init_engine
    out, args, _, three_d = run
    eng = init_engine("infer", args)
    assert eng.conf.mode == "infer" and list(eng.model.networks) == ["G_AB"]
    assert (eng.sliding_window_inferer is not None) == three_d
    # the checkpoint's generator was loaded
    w = torch.load(out / "checkpoints" / "2.pth", map_location="cpu")["G_AB"]
    for k, v in eng.model.networks["G_AB"].state_dict().items():
        assert torch.equal(v.cpu(), w[k]), k
    eng.run()
    images, saved = out / "infer" / "images", out / "infer" / "saved"
    assert sorted(p.name for p in images.iterdir()) == [f"{i}_input-output.png" for i in (1, 2, 3)]
    assert sorted(p.name for p in saved.iterdir()) == [f"sample_000{i}.npy" for i in range(3)]
    assert (out / "infer" / "infer_config.yaml").is_file()
    seen = 0
    for b, data in enumerate(eng.data_loader):                     # batches of 2 + 1; iter_idx = b * 1 * 2 + 1
        with torch.no_grad():
            fake = eng.infer(data["A"]).float().cpu()
        name, want = R.grid_ref({"input": data["A"], "output": fake})
        assert name == "input-output"
        for i in range(fake.shape[0]):
            got = _png(images / f"{b * 2 + 1 + i}_input-output.png")
            assert got.shape == ((16 * 24, 2 * 20, 3) if three_d else (32, 2 * 32, 3))
            assert torch.equal(got, want[i])
            kept = np.load(saved / f"{data['metadata']['id'][i]}.npy")
            assert kept.dtype == np.float32 and np.array_equal(kept, fake[i].numpy())
            seen += 1
    assert seen == 3


def test_tester_writes_a_mid_slice_image_per_sample_and_the_same_metrics_csv(run3d):
    from ganslate_amd.engines import init_engine
    out, args, _, _ = run3d
    te = init_engine("test", args)
    te.run()
    images = out / "test" / "images"
    assert sorted(p.name for p in images.iterdir()) == [f"{i}_real_A-fake_B-real_B.png" for i in range(3)]
    assert sorted(p.name for p in (out / "test" / "saved").iterdir()) == [f"sample_000{i}.npy" for i in range(3)]
    with open(out / "test" / "metrics.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert [int(r["sample"]) for r in rows] == [0, 1, 2]
    assert set(rows[0]) == {"sample", "ssim", "mse", "nmse", "psnr", "mae"}       # TestMetricsConfig defaults
    idx = 0
    for data in te.data_loaders[None]:
        with torch.no_grad():
            fake = te.infer(data["A"].cuda())
        # metrics.csv holds what the metric kernels give for (fake_B, real_B), as before the images were added
        table = te.metricizer.to_lists(te.metricizer.table(fake.float(), data["B"].cuda().float()))
        _, want = R.grid_ref({"real_A": data["A"], "fake_B": fake.float().cpu(), "real_B": data["B"]}, mid_slice_only=True)
        for i in range(fake.shape[0]):
            got = _png(images / f"{idx}_real_A-fake_B-real_B.png")
            assert got.shape == (24, 3 * 20, 3) and torch.equal(got, want[i])
            assert np.array_equal(np.load(out / "test" / "saved" / f"sample_000{idx}.npy"), fake[i].float().cpu().numpy())
            for k, column in table.items():
                assert float(rows[idx][k]) == column[i], (idx, k)
            idx += 1
    assert idx == 3
