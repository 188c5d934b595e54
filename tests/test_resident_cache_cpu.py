"""The residency rule of the device pipelines (data/resident_cache.py: keep a tensor while resident_bytes + nbytes <=
max_resident_bytes, otherwise make it again per use) at and beyond its budget, on CPU tensors with the reference ops the
pipelines' own tests inject: a budget of 0 keeps nothing and changes no bit of a batch; a budget of exactly the first
tensor's bytes keeps that one and nothing else; the image pipeline counts an upload per use."""
import random

import numpy as np
import pytest
import torch

from tests import mmvol_ref as R
from tests import test_mmimg_cpu as IMG
from tests import test_mmvol_cpu as MM
from tests import test_mmvol_valtest_cpu as VT

SHAPE, PATCH = (6, 7, 8), (2, 3, 4)


class _D(dict):
    __getattr__ = dict.__getitem__


def volume_case(tmp_path):
    """(dataset, ops, pipeline class, two raw batches) of UnpairedVolumeDataset over two volumes per domain"""
    from ganslate_amd.data.device_volumes import DeviceVolumePipeline
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset, collate_raw
    from oracle.ops_ref import RefOps
    rng = np.random.default_rng(5)
    for dom in "AB":
        (tmp_path / dom).mkdir()
        for k in range(2):
            np.save(tmp_path / dom / f"vol{k}.npy", np.round(rng.gamma(2.0, 180.0, size=SHAPE)).astype(np.float32))
    raw = UnpairedVolumeDataset(_D(mode="train", train=_D(dataset=_D(root=str(tmp_path), patch_size=list(PATCH),
                                                                      focal_region_proportion=0.3, device_transforms=True))))
    random.seed(3)
    return raw, RefOps(), DeviceVolumePipeline, [collate_raw([raw[i] for i in range(3)]) for _ in range(2)]


def multimodal_case(tmp_path):
    from ganslate_amd.data import MultiModalVolumeDataset
    from ganslate_amd.data.device_volumes import DeviceMultiModalPipeline
    from ganslate_amd.data.multimodal_volumes import collate_raw
    div = MM.toy_folder(tmp_path / "data", n=2, shape=SHAPE, shape_B=SHAPE)
    raw = MultiModalVolumeDataset(MM.dataset_conf(tmp_path / "data", False, "uniform-random-within-body-sf", PATCH, divisors=div,
                                                  device_transforms=True))
    random.seed(3)
    np.random.seed(3)
    return raw, R.RefMMOps(), DeviceMultiModalPipeline, [collate_raw([raw[i] for i in range(3)]) for _ in range(2)]


def whole_case(tmp_path):
    from ganslate_amd.data import MultiModalVolumeValTestDataset
    from ganslate_amd.data.device_volumes import DeviceWholeVolumePipeline
    div = VT.valtest_folder(tmp_path / "data", n=2)
    raw = MultiModalVolumeValTestDataset(VT.dataset_conf(tmp_path / "data", device_transforms=True, divisors=div))
    return raw, VT.RefWholeOps(), DeviceWholeVolumePipeline, [raw.collate_fn([raw[i]]) for i in (1, 1)]


def tensors(batch):
    """the tensors of a pipeline's batch, flat and by name, as raw bits (a NaN equals itself)"""
    out = {}
    for k, v in batch.items():
        for name, t in (v.items() if isinstance(v, dict) else [("", v)]):
            if isinstance(t, torch.Tensor):
                out[k + name] = t.contiguous().view(torch.uint8 if t.dtype == torch.uint8 else torch.int32)
    return out


def nbytes(t):
    return t.numel() * t.element_size()


@pytest.mark.parametrize("case", [volume_case, multimodal_case, whole_case])
def test_a_budget_of_zero_keeps_nothing_and_changes_no_bit(tmp_path, case):
    raw, ops, cls, batches = case(tmp_path)
    unlimited, none = cls(raw, "cpu", ops=ops), cls(raw, "cpu", ops=ops, max_resident_bytes=0)
    for batch in batches:
        want, got = tensors(unlimited(batch)), tensors(none(batch))
        assert want and set(got) == set(want)
        for k in want:
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
        assert none.resident == {} and none.resident_bytes == 0
    assert unlimited.resident and unlimited.resident_bytes == sum(nbytes(t) for t in unlimited.resident.values())


@pytest.mark.parametrize("case", [volume_case, multimodal_case])
def test_a_budget_of_one_tensor_keeps_exactly_that_one(tmp_path, case):
    raw, ops, cls, batches = case(tmp_path)
    unlimited = cls(raw, "cpu", ops=ops)
    want = [tensors(unlimited(batch)) for batch in batches]
    first = next(iter(unlimited.resident))                         # dicts keep insertion order: the first upload
    budget = nbytes(unlimited.resident[first])
    one = cls(raw, "cpu", ops=ops, max_resident_bytes=budget)
    kept = None
    for batch, ref in zip(batches, want):
        got = tensors(one(batch))
        assert all(torch.equal(got[k], ref[k]) for k in ref)
        assert list(one.resident) == [first] and one.resident_bytes == nbytes(one.resident[first]) == budget
        assert kept is None or one.resident[first] is kept         # the same object on the next call
        kept = one.resident[first]
    assert torch.equal(kept, unlimited.resident[first])


def test_the_image_pipeline_uploads_per_use_beyond_its_budget(tmp_path):
    from ganslate_amd.data import MultiModalImageDataset
    from ganslate_amd.data.device_images import DeviceMultiModalImagePipeline
    root = IMG.toy_folder(tmp_path / "data", sizes=[(5, 7)] * 2)
    raw = MultiModalImageDataset(IMG.dataset_conf(root, load=(5, 7), device_transforms=True))
    batch = raw.collate_fn([raw[0], raw[1]])
    unlimited = DeviceMultiModalImagePipeline(raw, "cpu", ops=IMG.OracleOps())
    none = DeviceMultiModalImagePipeline(raw, "cpu", ops=IMG.OracleOps(), max_resident_bytes=0)
    want = tensors(unlimited(batch))
    per_use = none.uploads
    assert per_use == 0
    for use in (1, 2, 3):
        got = tensors(none(batch))
        assert all(torch.equal(got[k], want[k]) for k in want)
        per_use = per_use or none.uploads
        assert per_use > 0 and none.uploads == use * per_use and len(none.resident) == 0 and none.resident_bytes == 0
    unlimited(batch)
    assert unlimited.uploads == len(unlimited.resident) <= per_use         # resident: once per file, however often used
