"""gs_volume_prepare (csrc/volsample.hip) through HipOps.volume_prepare: bit-equal to the numpy float32 chain of
tests/bodymask_ref.volume_prepare (where, np.pad with the minimum, divide, clip, subtract / divide, 2 x - 1 — the standard
tests/test_mmvol_gpu.py sets for the patch kernel), and within 2e-6 absolute of the torch host chain of
MultiModalVolumeValTestDataset.normalize (the tolerance of tests/test_mmvol_gpu.py for the same chain: a last-ulp
difference of one division on [-1, 1])."""
import numpy as np
import pytest
import torch

from tests import bodymask_ref as B
from tests import mmvol_ref as R

pytestmark = pytest.mark.gpu

PARAMS = {"pet": (0.0, 1.0, 0.0, 6.0), "ct": (-1024.0, 1.0, -1000.0, 2000.0), "hx4": (0.0, 1.75, 0.0, 3.0)}   # fill, div, lo, hi
SHAPES = [((5, 9, 11), (8, 9, 16)),          # odd and even pad totals, one axis unpadded
          ((12, 20, 24), (12, 20, 24)),      # nothing padded: the minimum pass is skipped
          ((12, 20, 24), (8, 16, 24)),       # a target below the volume
          ((6, 10, 7), (5, 13, 8))]          # mixed: one axis above its target, odd totals of 3 and 1


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _case(shape, seed):
    v = R.synthetic_case(shape, seed)
    rng = np.random.default_rng(seed + 1)
    v["gtv"] = (rng.random(shape) < 0.2).astype(np.uint8)
    v["ones"] = np.ones(shape, np.uint8)
    return v


def _both(ops, v, names, mask, extra, target):
    cols = list(zip(*[PARAMS[n] for n in names]))
    want, want_masks = B.volume_prepare([v[n] for n in names], v[mask], [v[m] for m in extra], target, *cols)
    dev = ops.device
    got, got_masks = ops.volume_prepare([_dev(v[n], dev) for n in names], _dev(v[mask], dev), [_dev(v[m], dev) for m in extra],
                                        target, *cols)
    return got.cpu().numpy(), [m.cpu().numpy() for m in got_masks], want, want_masks


def _same_bits(got, want):
    return np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("names", [("pet",), ("ct",), ("pet", "ct", "hx4")])            # fp32, int16, mixed with a divisor
@pytest.mark.parametrize("shape,target", SHAPES)
def test_prepare_is_bit_equal_to_the_numpy_chain(hip_ops, shape, target, names):
    v = _case(shape, 11)
    got, got_masks, want, want_masks = _both(hip_ops, v, names, "body", ["gtv", "ones"], target)
    out_shape = tuple(max(s, t) for s, t in zip(shape, target))
    assert got.dtype == np.float32 and got.shape == want.shape == (len(names), *out_shape)
    assert _same_bits(got, want), np.abs(got - want).max()
    assert got.min() >= -1.0 and got.max() <= 1.0
    assert len(got_masks) == 3
    for g, w in zip(got_masks, want_masks):
        assert g.dtype == np.uint8 and g.shape == out_shape and np.array_equal(g, w)
    if out_shape != shape:
        assert got_masks[2].all() and not got_masks[0][0, 0, 0]                            # all-ones pads with 1, the body with 0


def test_an_all_ones_body_pads_with_the_volume_minimum(hip_ops):
    v = _case((5, 9, 11), 12)
    got, got_masks, want, _ = _both(hip_ops, v, ("pet", "ct"), "ones", [], (8, 9, 16))
    assert _same_bits(got, want) and got_masks[0].all()
    hx4 = np.maximum(v["hx4"], np.float32(0.5))               # a minimum inside the clip range: the pad value shows it
    v["hx4"] = hx4
    got, _, want, _ = _both(hip_ops, v, ("hx4",), "ones", [], (8, 9, 16))
    assert _same_bits(got, want)
    assert got[0, 0, 0, 0] == np.float32(2) * ((np.float32(0.5) / np.float32(1.75)) / np.float32(3.0)) - np.float32(1)


def test_a_nan_voxel_makes_the_pad_value_nan(hip_ops):
    v = _case((5, 9, 11), 13)
    v["pet"][2, 4, 5] = np.nan
    v["body"][2, 4, 5] = 1
    got, _, want, _ = _both(hip_ops, v, ("pet", "ct"), "body", [], (8, 9, 16))
    assert np.isnan(want[0, 0, 0, 0]) and np.isnan(got[0]).sum() == np.isnan(want[0]).sum() == 8 * 9 * 16 - 5 * 9 * 11 + 1
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(got[1]).any()
    keep = ~np.isnan(want)
    assert np.array_equal(got[keep].view(np.int32), want[keep].view(np.int32))
    v["body"][2, 4, 5] = 0                                     # outside the body the NaN is replaced before the minimum
    got, _, want, _ = _both(hip_ops, v, ("pet",), "body", [], (8, 9, 16))
    assert not np.isnan(got).any() and _same_bits(got, want)


def test_prepare_equals_the_torch_host_chain(hip_ops):
    from ganslate_amd.data.utils.normalization import min_max_normalize
    from ganslate_amd.data.utils.ops import pad
    v = _case((5, 9, 11), 14)
    names = ("pet", "ct", "hx4")
    got, got_masks, _, _ = _both(hip_ops, v, names, "body", ["gtv"], (8, 9, 16))
    m = torch.from_numpy(v["body"] != 0)
    for c, n in enumerate(names):
        fill, div, lo, hi = PARAMS[n]
        t = torch.where(m, torch.from_numpy(v[n].copy()).float(), torch.tensor(fill))
        t = torch.from_numpy(pad(t.numpy(), (8, 9, 16))) / div
        assert torch.allclose(torch.from_numpy(got[c]), min_max_normalize(torch.clamp(t, lo, hi), lo, hi), atol=2e-6, rtol=0)
    assert np.array_equal(got_masks[1], pad(v["gtv"], (8, 9, 16)))


def test_refusals_come_before_any_launch(hip_ops):
    from ganslate_amd.hip.lib import HipError
    dev = hip_ops.device
    v = _case((5, 9, 11), 15)
    mask, pet = _dev(v["body"], dev), _dev(v["pet"], dev)
    out = torch.full((1, 8, 9, 16), 5.0, device=dev)
    mo = [torch.full((8, 9, 16), 5, dtype=torch.uint8, device=dev)]
    one = lambda **k: hip_ops.volume_prepare(k.get("vols", [pet]), k.get("mask", mask), k.get("extra", []),
                                             k.get("target", (8, 9, 16)), [0.0], [k.get("div", 1.0)], [k.get("lo", 0.0)],
                                             [k.get("hi", 6.0)], out=k.get("out", out), masks_out=k.get("mo", mo))
    with pytest.raises(HipError, match="clip range"):
        one(lo=6.0)
    with pytest.raises(HipError, match="divisor"):
        one(div=0.0)
    with pytest.raises(HipError, match="divisor"):
        one(div=float("nan"))
    with pytest.raises(ValueError, match="out"):
        one(out=torch.empty((1, 8, 9, 15), device=dev))
    with pytest.raises(ValueError, match="volume 0"):
        one(vols=[pet.double()])
    with pytest.raises(ValueError, match="volume 0"):
        one(vols=[pet[:4]])
    with pytest.raises(ValueError, match="mask"):
        one(mask=mask.float())
    with pytest.raises(ValueError, match="extra mask 0"):
        one(extra=[mask[:4]], mo=mo * 2)
    with pytest.raises(ValueError, match="masks_out"):
        one(mo=mo * 2)
    with pytest.raises(ValueError, match="target"):
        one(target=(8, 9))
    with pytest.raises(ValueError, match="between 1 and 8 volumes"):
        hip_ops.volume_prepare([pet] * 9, mask, [], (8, 9, 16), [0.0] * 9, [1.0] * 9, [0.0] * 9, [6.0] * 9)
    with pytest.raises(ValueError, match="at most 8 extra masks"):
        one(extra=[mask] * 9)
    with pytest.raises(ValueError, match="one entry per volume"):
        hip_ops.volume_prepare([pet], mask, [], (8, 9, 16), [0.0, 1.0], [1.0], [0.0], [6.0])
    # the library's own refusals behind the wrapper's
    import ctypes as C
    lib = hip_ops.lib
    ws = torch.zeros(int(lib.gs_volume_prepare_ws_bytes()) // 4, dtype=torch.float32, device=dev)
    f1 = lambda x: (C.c_float * 1)(x)
    vp, mp, op = (C.c_void_p * 1)(pet.data_ptr()), (C.c_void_p * 1)(mask.data_ptr()), (C.c_void_p * 1)(mo[0].data_ptr())
    call = lambda **k: lib.gs_volume_prepare(k.get("vp", vp), (C.c_int32 * 1)(k.get("dtype", 0)), k.get("C", 1), k.get("mp", mp),
                                             k.get("M", 1), 5, 9, 11, (C.c_int32 * 3)(*k.get("target", (8, 9, 16))), f1(0.0),
                                             f1(1.0), f1(0.0), f1(6.0), C.c_void_p(out.data_ptr()), op,
                                             k.get("ws", C.c_void_p(ws.data_ptr())), None)
    assert call(dtype=2) == 2 and call(C=0) == 2 and call(C=9) == 2 and call(M=0) == 2 and call(M=10) == 2
    assert call(target=(0, 9, 16)) == 2 and call(ws=None) == 2
    assert call(vp=(C.c_void_p * 1)(None)) == 2 and call(mp=(C.c_void_p * 1)(None)) == 2
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((mo[0] == 5).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == 5.0).any())
