"""The masked restatement (tests/valmetrics_masked_ref.py) against numpy's own masked arrays: build what the reference's
create_masked_array builds (val_test_metrics.py:19-29) and evaluate its one-line metric formulas (:37-53, the .max() of
:56-59, np.histogram / np.histogramdd of :90-131) on it. Plus the seeded synthetic dataset that yields masks."""
import numpy as np
import pytest
import torch

from tests import valmetrics_masked_ref as mref
from tests import valmetrics_ref as ref


def create_masked_array(x, mask):
    m = mask.astype(bool)
    return np.ma.masked_array(x * m, mask=~m)


def _case(seed, shape=(2, 12, 14)):
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1000, 3000, shape).astype(np.float64)
    p = t + rng.normal(0, 60, shape)
    return t, p, (rng.random(shape) < 0.4).astype(np.uint8)


@pytest.mark.parametrize("seed", range(4))
def test_scalars_match_numpy_masked_arrays(seed):
    t, p, mask = _case(seed)
    gt, pred = create_masked_array(t, mask), create_masked_array(p, mask)
    want = {"mae": np.mean(np.abs(gt - pred)), "mse": np.mean((gt - pred) ** 2),
            "nmse": np.linalg.norm(gt - pred) ** 2 / np.linalg.norm(gt) ** 2}
    for k, v in want.items():
        assert mref.FNS[k](t, p, mask) == pytest.approx(float(v), rel=1e-12, abs=0), k
    assert mref.masked_max(t, mask) == pytest.approx(float(gt.max()), rel=1e-12, abs=0)
    # psnr as skimage states it: np.asarray of both, mean over every element, data_range = the masked maximum
    err = np.mean((np.asarray(gt, dtype=np.float64) - np.asarray(pred, dtype=np.float64)) ** 2)
    assert mref.psnr(t, p, mask) == pytest.approx(float(10 * np.log10(float(gt.max()) ** 2 / err)), rel=1e-12, abs=0)


@pytest.mark.parametrize("seed", range(4))
def test_histograms_match_numpy_on_masked_arrays(seed):
    t, p, mask = _case(seed)
    t, p = t.astype(np.float32), p.astype(np.float32)
    gt, pred = create_masked_array(t, mask), create_masked_array(p, mask)
    ht, hp, hj = mref.bin_counts(t, p, mask)
    np.testing.assert_array_equal(ht, np.histogram(gt, bins=100)[0])
    np.testing.assert_array_equal(hp, np.histogram(pred, bins=100)[0])
    np.testing.assert_array_equal(hj, np.histogramdd([np.reshape(gt, -1), np.reshape(pred, -1)], bins=100)[0])
    assert ht.sum() == t.size          # masked-out elements are counted (as zeros), not dropped
    dens, _ = np.histogramdd([np.reshape(gt, -1), np.reshape(pred, -1)], bins=100, density=True)
    want = (ref._entropy(dens.sum(axis=0)) + ref._entropy(dens.sum(axis=1))) / ref._entropy(dens)
    assert mref.nmi(t, p, mask) == pytest.approx(want, rel=1e-12, abs=0)


def test_an_all_ones_mask_is_the_unmasked_restatement():
    t, p, _ = _case(9, (1, 9, 30))
    t, p = t.astype(np.float32), p.astype(np.float32)
    assert mref.metrics(t, p, np.ones_like(t)) == ref.metrics(t, p)
    for a, b in zip(mref.bin_counts(t, p, np.ones_like(t)), ref.bin_counts(t, p)):
        np.testing.assert_array_equal(a, b)


def test_the_data_range_is_the_masked_maximum_not_the_maximum_of_the_product():
    t, p, _ = _case(5)
    mask = np.zeros(t.shape, dtype=bool)
    mask[:, 2:8, 3:11] = True
    t[mask] = -np.abs(t[mask]) - 1.0                 # only negative targets inside
    gt = create_masked_array(t, mask)
    assert mref.masked_max(t, mask) < 0 and float((t * mask).max()) == 0.0
    assert mref.masked_max(t, mask) == float(gt.max())
    assert np.isfinite(mref.psnr(t, p, mask))        # Rm^2 > 0; max(t * m) = 0 would give -inf


def test_an_empty_mask_gives_nan():
    t, p, _ = _case(1)
    assert all(np.isnan(v) for v in mref.metrics(t, p, np.zeros(t.shape)).values())


def _dataset(name, shape, seed=11, labels=("BODY", "GTV", "OAR")):
    from ganslate_amd.configs.omegalite import OmegaConf
    from ganslate_amd import data
    conf = OmegaConf.create({"mode": "val", "val": {"dataset": {
        "image_channels": shape[0], "final_size": list(shape[1:]), "length": 6, "seed": seed,
        "mask_labels": list(labels)}}})
    return getattr(data, name)(conf)


@pytest.mark.parametrize("shape", [(1, 16, 24, 20), (1, 16, 16, 16), (3, 32, 32)], ids=str)
def test_the_masked_synthetic_dataset_is_seeded_and_never_empty(shape):
    a, b, plain = (_dataset("SyntheticMaskedImageDataset", shape), _dataset("SyntheticMaskedImageDataset", shape),
                   _dataset("SyntheticImageDataset", shape))
    other = _dataset("SyntheticMaskedImageDataset", shape, seed=12)
    assert len(a) == 6
    differs = False
    for i in range(len(a)):
        x, y, z = a[i], b[i], plain[i]
        assert torch.equal(x["A"], z["A"]) and torch.equal(x["B"], z["B"])        # the plain dataset's samples
        assert list(x["masks"]) == ["BODY", "GTV", "OAR"]
        for k, m in x["masks"].items():
            assert m.dtype == torch.bool and m.shape == x["A"].shape
            assert torch.equal(m, y["masks"][k])
            assert 0 < int(m.sum()) < m.numel()
            differs |= not torch.equal(m, other[i]["masks"][k])
    assert differs
