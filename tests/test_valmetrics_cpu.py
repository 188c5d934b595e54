"""The float64 restatement of val_test_metrics.py (tests/valmetrics_ref.py) against scipy's building blocks, and the
Tester engine (init_engine("test", ...)) on the oracle backend: checkpoint of a training run in, metrics.csv out."""
import csv
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

from ganslate_amd.nn.native import backend
from oracle.ops_ref import RefOps
from tests import valmetrics_ref as ref

CONF = Path(__file__).parent / "configs" / "cyclegan3d_test_synthetic.yaml"


def _pair(shape, seed, lo=-1.0, hi=1.0):
    rng = np.random.default_rng(seed)
    t = rng.uniform(lo, hi, shape).astype(np.float32)
    p = (t + rng.normal(0, 0.1 * (hi - lo), shape)).astype(np.float32)
    return t, p


@pytest.mark.parametrize("shape,lo,hi", [((3, 16, 20), -1, 1), ((1, 4, 9, 12), -1000, 3000)])
def test_ssim_restatement_matches_uniform_filter_and_crop(shape, lo, hi):
    """skimage structural_similarity (defaults): scipy.ndimage.uniform_filter (reflect padding) then crop(S, 3)"""
    ndimage = pytest.importorskip("scipy.ndimage")
    t, p = _pair(shape, 1, lo, hi)
    R = float(t.max())
    vals = []
    for a, b in zip(t.reshape(-1, *shape[-2:]).astype(np.float64), p.reshape(-1, *shape[-2:]).astype(np.float64)):
        f = lambda x: ndimage.uniform_filter(x, size=7)
        ux, uy, uxx, uyy, uxy = f(a), f(b), f(a * a), f(b * b), f(a * b)
        cov = 49 / 48
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        vals.append(S[3:-3, 3:-3].mean())
    assert ref.ssim(t, p) == pytest.approx(float(np.mean(vals)), abs=1e-9)
    assert ref.ssim(t, t) == pytest.approx(1.0, abs=1e-12)


def test_ssim_restatement_rejects_planes_below_the_window():
    t, p = _pair((1, 6, 9), 2)
    with pytest.raises(ValueError):
        ref.ssim(t, p)


@pytest.mark.parametrize("seed", [3, 4])
def test_nmi_and_chi2_restatement_match_scipy_entropy(seed):
    stats = pytest.importorskip("scipy.stats")
    t, p = _pair((2, 11, 13), seed)
    hist, _ = np.histogramdd([t.ravel(), p.ravel()], bins=100, density=True)
    want = (stats.entropy(hist.sum(axis=0)) + stats.entropy(hist.sum(axis=1))) / stats.entropy(hist.ravel())
    assert ref.nmi(t, p) == pytest.approx(want, rel=1e-12)
    # val_test_metrics.py:110-131 verbatim (NaN bins dropped)
    g, _ = np.histogram(t, bins=100)
    q, _ = np.histogram(p, bins=100)
    g, q = g / g.sum(), q / q.sum()
    with np.errstate(invalid="ignore"):
        d = (q - g) ** 2 / (q + g)
    assert ref.histogram_chi2(t, p) == pytest.approx(float(np.sum(d[~np.isnan(d)])), rel=1e-12)


def test_scalar_restatement_matches_val_test_metrics():
    t, p = _pair((1, 8, 8, 8), 5)
    t64, p64 = t.astype(np.float64), p.astype(np.float64)
    assert ref.mae(t, p) == pytest.approx(np.mean(np.abs(t64 - p64)), rel=1e-12)
    assert ref.nmse(t, p) == pytest.approx(np.linalg.norm(t64 - p64) ** 2 / np.linalg.norm(t64) ** 2, rel=1e-12)
    assert ref.psnr(t, p) == pytest.approx(10 * np.log10(float(t.max()) ** 2 / np.mean((t64 - p64) ** 2)), rel=1e-12)
    assert ref.psnr(t, t) == float("inf")


@pytest.fixture
def fp32_oracle_backend():
    backend.set_ops(RefOps(act_dtype=torch.float32))
    yield
    backend.set_ops(None)


def _train_checkpoint(run_dir):
    """a 2-iteration CPU training run of CONF that leaves <run_dir>/checkpoints/2.pth"""
    from ganslate_amd.engines import init_engine
    tr = init_engine("train", [f"config={CONF}", "train.cuda=false", f"train.output_dir={run_dir}", "train.seed=7",
                               "train.n_iters=2", "train.n_iters_decay=0", "train.checkpointing.freq=2"])
    tr.run()
    path = run_dir / "checkpoints" / "2.pth"
    assert path.is_file()
    return path


def test_tester_scores_a_training_checkpoint_into_metrics_csv(fp32_oracle_backend, tmp_path):
    """init_engine("test", ...) (validator_tester.py:127-135): builds the generator, loads test.checkpointing.load_iter
    from <test.output_dir>/checkpoints through BaseGAN.setup, scores every test sample and writes
    <test.output_dir>/test/metrics.csv, one row per sample. train.output_dir names another directory: nothing goes there."""
    from ganslate_amd.engines import init_engine
    ckpt = _train_checkpoint(tmp_path / "run")
    test_dir, other = tmp_path / "scored", tmp_path / "elsewhere"
    (test_dir / "checkpoints").mkdir(parents=True)
    shutil.copy(ckpt, test_dir / "checkpoints" / "2.pth")
    te = init_engine("test", [f"config={CONF}", "train.cuda=false", f"train.output_dir={other}",
                              f"test.output_dir={test_dir}", "test.checkpointing.load_iter=2"])
    assert list(te.model.networks) == ["G_AB"]
    # the checkpoint's generator weights were loaded
    w = torch.load(ckpt, map_location="cpu")["G_AB"]
    for k, v in te.model.networks["G_AB"].state_dict().items():
        assert torch.equal(v.cpu(), w[k]), k
    te.run()
    path = test_dir / "test" / "metrics.csv"
    assert path.is_file() and not other.exists()
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 3                                   # test.dataset.length, batches of 2 + 1
    assert set(rows[0]) == {"sample", "mae", "mse", "nmse", "psnr"}
    assert [int(r["sample"]) for r in rows] == [0, 1, 2]
    for r, s in zip(rows, te.samples[None]):
        assert all(float(r[k]) == pytest.approx(s[k], rel=1e-12) and np.isfinite(s[k]) for k in s)
    _, _, mean = te.history[-1]
    assert mean["mae"] == pytest.approx(np.mean([float(r["mae"]) for r in rows]), rel=1e-12)


def test_tester_csv_names_the_dataset_of_every_row_with_multi_dataset(fp32_oracle_backend, tmp_path):
    """test.multi_dataset: one loader per named dataset (builders.build_loader), all rows in one metrics.csv with a
    `dataset` column, and one history entry per dataset"""
    from ganslate_amd.engines import init_engine
    _train_checkpoint(tmp_path)
    text = CONF.read_text()
    single = """  dataset:
    _target_: ganslate.data.SyntheticImageDataset
    image_channels: 1
    final_size: [16, 24, 20]
    length: 3
  sliding_window:"""
    multi = """  multi_dataset:
    first:
      _target_: ganslate.data.SyntheticImageDataset
      image_channels: 1
      final_size: [16, 24, 20]
      length: 3
    second:
      _target_: ganslate.data.SyntheticImageDataset
      image_channels: 1
      final_size: [16, 24, 20]
      length: 1
      seed: 11
  sliding_window:"""
    assert text.count(single) == 1
    conf = tmp_path / "multi.yaml"
    conf.write_text(text.replace(single, multi))
    te = init_engine("test", [f"config={conf}", "train.cuda=false", f"train.output_dir={tmp_path}",
                              f"test.output_dir={tmp_path}", "test.checkpointing.load_iter=2"])
    assert set(te.data_loaders) == {"first", "second"}
    te.run()
    with open(tmp_path / "test" / "metrics.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == ["dataset", "sample", "mae", "mse", "nmse", "psnr"]
    assert [(r["dataset"], int(r["sample"])) for r in rows] == [("first", 0), ("first", 1), ("first", 2), ("second", 0)]
    assert [h[1] for h in te.history] == ["first", "second"]
    for name, rows_of in (("first", rows[:3]), ("second", rows[3:])):
        for r, s in zip(rows_of, te.samples[name]):
            assert all(float(r[k]) == pytest.approx(s[k], rel=1e-12) for k in s)


def test_infer_engine_is_still_out_of_scope():
    from ganslate_amd.engines import init_engine
    with pytest.raises(NotImplementedError):
        init_engine("infer", [f"config={CONF}"])
