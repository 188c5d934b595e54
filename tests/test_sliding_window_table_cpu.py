"""Host side of the sliding-window kernels (csrc/slidewin.hip): the window table they walk, and which path a call takes."""
import pytest
import torch

from ganslate_amd.utils.sliding_window_inferer import SlidingWindowInferer, window_starts, window_table


@pytest.mark.parametrize("size,roi,overlap,batch", [
    ((20, 24, 28), (8, 16, 16), 0.25, 1),
    ((17, 19, 23), (8, 8, 8), 0.5, 2),
    ((16, 12, 12), (16, 8, 8), 0.25, 3),          # the padded size of a 12^3 volume under a 16 x 8 x 8 window
    ((9, 13, 11), (4, 7, 5), 0.4, 1),
    ((40, 56), (16, 32), 0.25, 2),                # images: z = 0
    ((5, 24, 24), (1, 16, 16), 0.25, 1),          # a 2-D model over a volume
])
def test_window_table_is_window_starts_times_batch_in_order(size, roi, overlap, batch):
    table = window_table(list(size), list(roi), overlap, batch)
    starts = window_starts(list(size), list(roi), overlap)
    want = [[b] + [0] * (3 - len(st)) + list(st) for st in starts for b in range(batch)]      # start-major, batch item inner
    assert table.dtype == torch.int32 and table.shape == (len(starts) * batch, 4) and table.is_contiguous()
    assert table.tolist() == want
    # every window lies inside the (padded) size
    r3, s3 = [1] * (3 - len(roi)) + list(roi), [1] * (3 - len(size)) + list(size)
    for k in range(3):
        assert int(table[:, 1 + k].min()) == 0 and int(table[:, 1 + k].max()) == s3[k] - r3[k]


def test_padded_size_case_has_one_start_on_the_padded_axis():
    size0, roi = (12, 12, 12), (16, 8, 8)
    size = [max(s, r) for s, r in zip(size0, roi)]
    table = window_table(size, list(roi), 0.25, 1)
    assert size == [16, 12, 12] and set(table[:, 1].tolist()) == {0}
    assert table.shape[0] == len(window_starts([12], [8], 0.25)) ** 2


def test_cpu_tensors_take_the_torch_path_by_default(monkeypatch):
    inf = SlidingWindowInferer((8, 8, 8), 2, 0.25, "gaussian", cval=-1)
    assert inf.device_kernels is None
    monkeypatch.setattr(inf, "_infer_device", lambda *a: pytest.fail("a CPU tensor went to the device path"))
    x = torch.rand(1, 1, 12, 10, 9)
    out = inf(x, lambda w: w)
    assert torch.equal(out, SlidingWindowInferer((8, 8, 8), 2, 0.25, "gaussian", cval=-1, device_kernels=False)(x, lambda w: w))


def test_device_kernels_true_on_a_cpu_tensor_raises():
    inf = SlidingWindowInferer((8, 8, 8), 2, 0.25, "gaussian", cval=-1, device_kernels=True)
    with pytest.raises(RuntimeError, match="no CPU form"):
        inf(torch.rand(1, 1, 12, 10, 9), lambda w: w)
