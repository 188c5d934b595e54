"""HipOps.visuals_grid (csrc/visgrid.hip) against the torch-CPU restatement of the reference's op sequence
(tests/visgrid_ref.py), bit for bit. The inputs walk through the fp32 neighbours of every byte threshold. Every case writes
into an output placed inside a larger 0xA5-filled byte buffer and checks that the bytes in front of and behind it stay
untouched; the refused calls must leave the whole buffer untouched."""
import pytest
import torch

from tests import visgrid_ref as R

pytestmark = pytest.mark.gpu

GUARD = 512          # bytes of guard on each side; an odd front offset is used where the case asks for it


def _dev(t):
    return t.to("cuda").contiguous()


def _run(ops, visuals, front=GUARD, **kw):
    """(name, grid bytes on the CPU) of visuals_grid written inside a poisoned buffer; asserts on the guards"""
    _, want = R.grid_ref({k: v for k, v in visuals.items()}, **kw)
    size = want.numel()
    buf = torch.full((front + size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[front:front + size].view(want.shape)
    name, got = ops.visuals_grid(visuals, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:front] == 0xA5).all()) and bool((host[front + size:] == 0xA5).all()), "guard bytes were written"
    return name, host[front:front + size].view(want.shape), want


def _check(ops, visuals, **kw):
    name, got, want = _run(ops, visuals, **kw)
    assert got.shape == want.shape and torch.equal(got, want), \
        f"{int((got != want).sum())} of {want.numel()} bytes differ from the oracle"
    return name, got


def _three(N, H, W, D=None, channels=(3, 1, 3)):
    sp = (H, W) if D is None else (D, H, W)
    names = ("real_A", "fake_B", "real_B")
    return {n: _dev(R.tiled((N, c, *sp), offset=1500 * i)) for i, (n, c) in enumerate(zip(names, channels))}


def test_every_byte_threshold_and_its_neighbours(hip_ops):
    """4599 values, 4608 elements: each of the 255 thresholds with 8 ulp on both sides, -0.0, +-1, +-1.5, +-inf, randn"""
    v = R.threshold_values()
    assert v.numel() <= 72 * 64
    name, got = _check(hip_ops, {"x": _dev(R.tiled((1, 1, 72, 64)))})
    assert name == "x" and got.shape == (1, 72, 64, 3)
    assert len(torch.unique(got)) == 256


def test_nan_and_infinities_have_the_documented_bytes(hip_ops):
    """include/ganslate_hip.h: NaN -> 0, +inf -> 255, -inf -> 0 (the oracle defines NaN the same way); both paths"""
    row = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -1.0, 1.0, 3.0, -3.0])
    want = torch.tensor([0, 255, 0, 128, 0, 255, 255, 0], dtype=torch.uint8)
    for w in (8, 7):
        _, got = _check(hip_ops, {"x": _dev(row[:w].repeat(2).reshape(1, 1, 2, w))})
        assert torch.equal(got[0, :, :, 0], want[:w].repeat(2).reshape(2, w))


def test_2d_vector_path(hip_ops):
    name, got = _check(hip_ops, _three(2, 5, 8))
    assert name == "real_A-fake_B-real_B" and got.shape == (2, 5, 24, 3)


def test_2d_scalar_path(hip_ops):
    _, got = _check(hip_ops, _three(2, 5, 7))
    assert got.shape == (2, 5, 21, 3)


def test_vector_path_with_a_source_that_is_not_16_byte_aligned(hip_ops):
    vis = _three(2, 5, 8)
    t = vis["real_A"]
    store = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
    shifted = store[1:].view(t.shape)
    shifted.copy_(t)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    vis["real_A"] = shifted
    _check(hip_ops, vis)


def test_output_that_is_not_4_byte_aligned(hip_ops):
    _check(hip_ops, _three(2, 5, 8), front=GUARD + 1)
    _check(hip_ops, _three(2, 5, 7), front=GUARD + 3)


def test_single_example_writes_sample_0_only(hip_ops):
    vis = _three(3, 5, 8)
    _, got = _check(hip_ops, vis, single_example=True)
    assert got.shape == (1, 5, 24, 3)
    _, want0 = R.grid_ref({k: v[:1] for k, v in vis.items()})
    assert torch.equal(got, want0)


def test_3d_all_slices_stacked(hip_ops):
    _, got = _check(hip_ops, _three(2, 4, 6, D=3, channels=(1, 1, 1)))
    assert got.shape == (2, 12, 18, 3)


@pytest.mark.parametrize("D, mid", [(3, 1), (4, 2)])
def test_3d_mid_slice_only(hip_ops, D, mid):
    vis = _three(2, 4, 6, D=D, channels=(1, 1, 1))
    _, got = _check(hip_ops, vis, mid_slice_only=True)
    assert got.shape == (2, 4, 18, 3)
    _, want = R.grid_ref({k: v[:, :, mid] for k, v in vis.items()})          # the 2-D grid of that slice
    assert torch.equal(got, want)


def test_3d_vector_path_more_than_one_block(hip_ops):
    vis = {"a": _dev(R.tiled((1, 3, 2, 40, 36))), "b": _dev(R.tiled((1, 1, 2, 40, 36), offset=999))}
    _, got = _check(hip_ops, vis)
    assert got.shape == (1, 80, 72, 3)


def test_modality_split_takes_channel_ranges_of_the_same_tensor(hip_ops):
    vis = {"real_A": _dev(R.tiled((2, 4, 5, 8))), "fake_B": _dev(R.tiled((2, 1, 5, 8), offset=2000))}
    split = {"A": [1, 3], "B": None}
    name, got = _check(hip_ops, vis, multi_modality_split=split)
    assert name == "real_A1-real_A2-fake_B" and got.shape == (2, 5, 24, 3)
    # real_A1 is gray (channel 0 three times), real_A2 the RGB of channels 1..3
    _, a1 = R.grid_ref({"x": vis["real_A"][:, :1]})
    _, a2 = R.grid_ref({"x": vis["real_A"][:, 1:]})
    assert torch.equal(got[:, :, :8], a1) and torch.equal(got[:, :, 8:16], a2)


def test_sixteen_visuals(hip_ops):
    vis = {f"v{i}": _dev(R.tiled((1, 1, 2, 2), offset=37 * i)) for i in range(16)}
    name, got = _check(hip_ops, vis)
    assert got.shape == (1, 2, 32, 3) and name.count("-") == 15


def test_none_entries_are_dropped(hip_ops):
    vis = _three(2, 5, 8)
    name, got = _check(hip_ops, {"real_A": vis["real_A"], "idt_B": None, "fake_B": vis["fake_B"]})
    assert name == "real_A-fake_B" and got.shape == (2, 5, 16, 3)


def _refused(ops, visuals, match, **kw):
    buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    first = next(v for v in visuals.values() if v is not None)
    sp = first.shape[2:]
    rows = sp[-2] * (sp[0] if len(sp) == 3 else 1)
    shape = (first.shape[0], rows, len(visuals) * sp[-1], 3)
    n = shape[0] * shape[1] * shape[2] * 3
    assert n + 2 * GUARD <= buf.numel()
    out = buf[GUARD:GUARD + n].view(shape)
    with pytest.raises(ValueError, match=match):
        ops.visuals_grid(visuals, out=out, **kw)
    torch.cuda.synchronize()
    assert bool((buf.cpu() == 0xA5).all()), "a refused call wrote"


def test_seventeen_visuals_are_refused(hip_ops):
    _refused(hip_ops, {f"v{i}": _dev(R.tiled((1, 1, 2, 2))) for i in range(17)}, "at most 16")


def test_a_two_channel_visual_is_refused(hip_ops):
    _refused(hip_ops, {"a": _dev(R.tiled((1, 1, 4, 4))), "b": _dev(R.tiled((1, 2, 4, 4)))}, "1 or 3 channels")


def test_a_shape_mismatch_is_refused(hip_ops):
    _refused(hip_ops, {"a": _dev(R.tiled((2, 1, 4, 4))), "b": _dev(R.tiled((2, 1, 4, 5)))}, "differ")
    _refused(hip_ops, {"a": _dev(R.tiled((2, 1, 4, 4))), "b": _dev(R.tiled((1, 1, 4, 4)))}, "differ")


def test_a_bf16_tensor_is_refused(hip_ops):
    _refused(hip_ops, {"a": _dev(R.tiled((1, 1, 4, 4))), "b": _dev(R.tiled((1, 1, 4, 4))).bfloat16()}, "float32")


def test_a_split_that_does_not_sum_to_the_channels_is_refused(hip_ops):
    _refused(hip_ops, {"real_A": _dev(R.tiled((1, 4, 4, 4)))}, "channel-split", multi_modality_split={"A": [1, 2], "B": None})
