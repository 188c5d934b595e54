"""gs_body_mask (csrc/bodymask.hip) through HipOps.body_mask against the plain-numpy restatement of the definition in
tests/bodymask_ref.py: mask bytes and info = (voxels of the chosen component, its first voxel's flat index) must be EQUAL
on every case of that module, in both dtypes — everything is an integer. The serpentine case is the longest possible
geodesic through its volume; it has to finish in the seconds a test gets, which an implementation whose launches grow with
the path length does not."""
import time

import numpy as np
import pytest
import torch

from tests import bodymask_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()


def _run(ops, v, t, **kw):
    dev = torch.from_numpy(np.ascontiguousarray(v)).to(ops.device)
    n = v.size
    buf = torch.full((n + 256,), 7, dtype=torch.uint8, device=ops.device)         # 128 guard bytes on either side
    out = buf[128:128 + n].view(*v.shape)
    res = ops.body_mask(dev, t, out=out, **kw)
    guard = torch.cat([buf[:128], buf[128 + n:]])
    assert bool((guard == 7).all())
    return res


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("name", list(CASES))
def test_body_mask_equals_the_definition_exactly(hip_ops, name, dtype):
    v, t = CASES[name]
    v = R.as_dtype(v, dtype)
    if v is None:
        v = CASES[name][0]                                     # an fp32-only case runs as fp32 under both ids
    want, info_want = R.expected(name)
    t0 = time.perf_counter()
    mask, info, rounds = _run(hip_ops, v, t, return_rounds=True)
    got = mask.cpu().numpy()
    dt = time.perf_counter() - t0
    print(f"\n{name} [{v.dtype}]: rounds {rounds}, {dt * 1e3:.1f} ms wall")
    assert got.dtype == np.uint8 and got.shape == v.shape
    assert tuple(info.cpu().tolist()) == info_want
    assert np.array_equal(got, want), int((got != want).sum())
    again, info2 = _run(hip_ops, v, t)
    assert torch.equal(again, mask) and torch.equal(info2, info)                  # two runs, identical bytes


def test_nothing_at_the_threshold_gives_a_zero_mask(hip_ops):
    v, t = CASES["none_inside"]
    mask, info = _run(hip_ops, v, t)
    assert not bool(mask.any()) and info.cpu().tolist() == [0, -1]
    mask, info = _run(hip_ops, np.full((2, 3, 4), np.nan, np.float32), -1e30)
    assert not bool(mask.any()) and info.cpu().tolist() == [0, -1]


def test_serpentine_rounds_do_not_follow_the_path_length(hip_ops):
    v, t = CASES["serpentine"]
    _, (count, _) = R.expected("serpentine")
    _, info, rounds = _run(hip_ops, v, t, return_rounds=True)
    assert int(info[0]) == count > 7000
    assert rounds[0] < 64, rounds                             # a voxel-to-voxel spread would need thousands


def test_refusals_come_before_any_launch(hip_ops):
    import ctypes as C
    from ganslate_amd.hip import lib as L
    dev = hip_ops.device
    v = torch.zeros((3, 4, 5), dtype=torch.int16, device=dev)
    out = torch.full((3, 4, 5), 9, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="volume"):
        hip_ops.body_mask(v.double(), 0.0)
    with pytest.raises(ValueError, match="volume"):
        hip_ops.body_mask(v.cpu(), 0.0)
    with pytest.raises(ValueError, match="volume"):
        hip_ops.body_mask(v[:, :, ::2], 0.0)
    with pytest.raises(ValueError, match="NaN"):
        hip_ops.body_mask(v, float("nan"), out=out)
    with pytest.raises(ValueError, match="out"):
        hip_ops.body_mask(v, 0.0, out=out[:2])
    lib = hip_ops.lib
    info = torch.full((2,), 9, dtype=torch.int32, device=dev)
    ws = torch.zeros(int(lib.gs_body_mask_ws_bytes(3, 4, 5)) // 8 + 1, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda **k: lib.gs_body_mask(k.get("vol", p(v)), k.get("dtype", 1), *k.get("dims", (3, 4, 5)), k.get("t", 0.0),
                                        k.get("out", p(out)), p(info), k.get("ws", p(ws)), None)
    assert call(vol=None) == 2 and call(out=None) == 2 and call(ws=None) == 2
    assert call(dtype=2) == 2 and call(dims=(0, 4, 5)) == 2 and call(t=float("nan")) == 2
    assert call(dims=(2048, 1024, 1024)) == 2                                     # 2^31 voxels
    assert call(ws=C.c_void_p(ws.data_ptr() + 4)) == 2
    assert lib.gs_body_mask_ws_bytes(0, 4, 5) == 0 and lib.gs_body_mask_ws_bytes(3, 4, 5) >= 3 * 4 * 5 * 9
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and info.cpu().tolist() == [9, 9]
    assert call() == 0
    assert info.cpu().tolist() == [60, 0] and bool((out == 1).all())
