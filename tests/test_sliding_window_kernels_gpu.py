"""Sliding-window inference as HIP kernels (csrc/slidewin.hip: gs_sw_gather / gs_sw_accumulate / gs_sw_finalize) against
the sequential host algorithm: the inferer's torch code on the CPU, bit for bit, and the loop-level MONAI restatement
(oracle/monai_ref.py) at the tolerance of tests/test_sliding_window_cpu.py. The predictor is arithmetic that is exact or
singly rounded on both sides, so every bit of a difference would be the stitching's."""
import functools

import pytest
import torch
import torch.nn.functional as F

from ganslate_amd.utils.sliding_window_inferer import SlidingWindowInferer, importance_map, window_table
from oracle import monai_ref

pytestmark = pytest.mark.gpu

CVAL = -1.0


def predictor(w):
    return torch.cat([w * 0.5 + 0.25, w * -0.25], 1)          # C_out = 2 C_in


CASES = [
    # the six of test_sliding_window_cpu.py::test_matches_loop_restatement
    ((1, 1, 20, 24, 28), (8, 16, 16), 0.25, "gaussian", 1),
    ((2, 2, 17, 19, 23), (8, 8, 8), 0.5, "gaussian", 3),
    ((1, 1, 12, 12, 12), (16, 8, 8), 0.25, "constant", 2),
    ((2, 3, 40, 56), (16, 32), 0.25, "gaussian", 4),
    ((1, 1, 16, 16, 16), (16, 16, 16), 0.25, "gaussian", 1),
    ((1, 1, 30, 33, 35), (16, 16, 16), 0.0, "constant", 5),
    ((1, 2, 9, 13, 11), (4, 7, 5), 0.4, "gaussian", 3),          # odd widths and odd starts: the scalar tail
    ((2, 1, 8, 16, 32), (8, 8, 16), 0.5, "constant", 4),         # aligned: the vector path
    ((1, 2, 5, 24, 24), (16, 16), 0.25, "gaussian", 2),          # a 2-D roi over a volume
]
IDS = [f"{'x'.join(map(str, c[0]))}-roi{'x'.join(map(str, c[1]))}" for c in CASES]


@functools.lru_cache(maxsize=None)
def reference(k):
    """(input, the torch path on the CPU, the MONAI restatement on the CPU) of case k — computed once, never modified"""
    shape, roi, overlap, mode, sw = CASES[k]
    x = torch.rand(shape, generator=torch.Generator().manual_seed(3)) * 2 - 1
    host = SlidingWindowInferer(roi, sw, overlap, mode, cval=CVAL, device_kernels=False)(x, predictor)
    if len(roi) == len(shape) - 2:
        monai = monai_ref.sliding_window_inference(x, list(roi), sw, predictor, overlap, mode, CVAL)
    else:                                                      # slice-wise: what network_wrapper does around the network
        monai = monai_ref.sliding_window_inference(x, [1, *roi], sw, lambda w: predictor(w.squeeze(2)).unsqueeze(2),
                                                   overlap, mode, CVAL)
    return x, host, monai


@functools.lru_cache(maxsize=None)
def device_result(k):
    shape, roi, overlap, mode, sw = CASES[k]
    x = reference(k)[0]
    return SlidingWindowInferer(roi, sw, overlap, mode, cval=CVAL, device_kernels=True)(x.cuda(), predictor).cpu()


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_device_path_equals_the_host_algorithm_bit_for_bit(hip_ops, k):
    _, host, _ = reference(k)
    got = device_result(k)
    assert got.shape == host.shape == (CASES[k][0][0], 2 * CASES[k][0][1], *CASES[k][0][2:])
    assert not torch.isnan(got).any()
    assert torch.equal(got, host), f"max |diff| {(got - host).abs().max().item():.3e}"


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_device_path_matches_the_monai_restatement(hip_ops, k):
    _, host, monai = reference(k)
    assert torch.allclose(host, monai, atol=1e-6, rtol=1e-5)           # the shape is a fair one for the reference
    assert torch.allclose(device_result(k), monai, atol=1e-6, rtol=1e-5)


def _padding(size0, roi):
    size = [max(s, r) for s, r in zip(size0, roi)]
    before = [(p - s) // 2 for p, s in zip(size, size0)]
    fpad = []
    for k in (2, 1, 0):                                        # F.pad order: last axis first
        fpad += [before[k], size[k] - size0[k] - before[k]]
    return size, before, fpad


@pytest.mark.parametrize("shape,roi,overlap,rows", [
    ((1, 2, 5, 9, 5), (8, 4, 8), 0.25, slice(None)),           # z and x shorter than the roi, both by 3: 1 in front, 2 behind
    ((2, 1, 6, 7, 9), (3, 4, 5), 0.5, slice(None)),            # two interleaved batch items, odd widths: the scalar form
    ((2, 2, 8, 8, 16), (4, 4, 8), 0.5, slice(3, 8)),           # a table slice that starts mid-table; aligned quads
    ((2, 1, 4, 6, 10), (4, 4, 8), 0.75, slice(1, None)),       # x starts 0, 2: quads that are not 16-byte aligned
], ids=["short-axes", "batch2-odd", "mid-table", "unaligned-quads"])
def test_gather_reads_the_padded_windows(hip_ops, shape, roi, overlap, rows):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(5)) * 2 - 1
    size, before, fpad = _padding(shape[2:], roi)
    table = window_table(size, list(roi), overlap, shape[0])
    assert table.shape[0] > 3 or rows == slice(None)
    sel = table[rows].contiguous()
    padded = F.pad(x, fpad, value=CVAL)
    want = torch.stack([padded[b, :, z:z + roi[0], y:y + roi[1], w:w + roi[2]] for b, z, y, w in sel.tolist()])
    out = torch.full(want.shape, float("nan"), device=hip_ops.device)
    got = hip_ops.sw_gather(x.to(hip_ops.device), table.to(hip_ops.device)[rows], roi, before, CVAL, out=out)
    assert got is out
    got = got.cpu()
    assert not torch.isnan(got).any()
    assert torch.equal(got, want)


@pytest.mark.parametrize("size0,roi,starts,chunk", [
    # every window covers voxels (·, 2..3, 3..4); odd width: the scalar form; z shorter than the roi: 1 plane cropped in front
    ((2, 6, 8), (4, 4, 5), [(0, 0, 0), (0, 2, 3), (0, 2, 0), (0, 0, 3)], 3),
    # every window covers voxels (2..3, 2..3, 4..7); x starts and widths multiples of 4: the vector form
    ((6, 6, 12), (4, 4, 8), [(2, 2, 4), (0, 0, 0), (2, 0, 4), (0, 2, 0), (2, 2, 0), (0, 0, 4), (0, 2, 4), (2, 0, 0)], 5),
], ids=["scalar-cropped", "vector"])
def test_accumulate_and_finalize_follow_the_sequential_loop(hip_ops, size0, roi, starts, chunk):
    B, Cc = 2, 3
    size, before, _ = _padding(size0, roi)
    rows = [(b, *st) for st in starts for b in range(B)]
    rows = rows[1:] + rows[:1]                                 # not sorted by batch item or start: the order is the table's
    table = torch.tensor(rows, dtype=torch.int32)
    g = torch.Generator().manual_seed(7)
    pred = torch.rand((len(rows), Cc, *roi), generator=g) * 2 - 1
    imap = importance_map(roi, "gaussian", "cpu")
    # the host loop, in fp32: one rounded product and one rounded sum per window, windows in table order
    acc = torch.zeros((B, Cc, *size))
    count = torch.zeros((B, 1, *size))
    for i, (b, z, y, w) in enumerate(rows):
        acc[b, :, z:z + roi[0], y:y + roi[1], w:w + roi[2]] += imap * pred[i]
        count[b, :, z:z + roi[0], y:y + roi[1], w:w + roi[2]] += imap
    z0, y0, w0 = before
    want = (acc / count)[:, :, z0:z0 + size0[0], y0:y0 + size0[1], w0:w0 + size0[2]]
    cover = torch.zeros(size, dtype=torch.int32)
    for st in starts:
        cover[st[0]:st[0] + roi[0], st[1]:st[1] + roi[1], st[2]:st[2] + roi[2]] += 1
    assert int(cover.min()) >= 1 and int(cover.max()) == len(starts)      # covered everywhere; all windows share a voxel

    dev = hip_ops.device
    table_d, pred_d, imap_d = table.to(dev), pred.to(dev), imap.to(dev)

    def run():
        a = torch.zeros((B, Cc, *size), device=dev)
        for g0 in range(0, len(rows), chunk):
            hip_ops.sw_accumulate(a, pred_d[g0:g0 + chunk], imap_d, table_d[g0:g0 + chunk], table[g0:g0 + chunk])
        out = torch.full((B, Cc, *size0), float("nan"), device=dev)
        assert hip_ops.sw_finalize(a, imap_d, table_d, size0, before, out=out) is out
        return a.cpu(), out.cpu()

    acc1, got1 = run()
    acc2, got2 = run()
    assert torch.equal(acc1, acc)
    assert not torch.isnan(got1).any()
    assert torch.equal(got1, want)
    assert torch.equal(got1.view(torch.int32), got2.view(torch.int32)) and torch.equal(acc1.view(torch.int32), acc2.view(torch.int32))


def test_shape_errors_raise_before_any_launch(hip_ops):
    dev = hip_ops.device
    x = torch.zeros(1, 1, 4, 4, 4, device=dev)
    table = torch.zeros(1, 4, dtype=torch.int32, device=dev)
    imap = torch.ones(2, 2, 2, device=dev)
    with pytest.raises(ValueError):
        hip_ops.sw_gather(x, table, (0, 2, 2), (0, 0, 0), 0.0)                         # roi[k] >= 1
    with pytest.raises(ValueError):
        hip_ops.sw_gather(x, table, (2, 2, 2), (1, 0, 0), 0.0)                         # no padding on an axis >= the roi
    with pytest.raises(ValueError):
        hip_ops.sw_gather(x.cpu(), table, (2, 2, 2), (0, 0, 0), 0.0)
    with pytest.raises(ValueError):
        hip_ops.sw_accumulate(x, torch.zeros(1, 2, 2, 2, 2, device=dev), imap, table, table.cpu())     # channels differ
    with pytest.raises(ValueError):
        hip_ops.sw_accumulate(x, torch.zeros(1, 1, 2, 2, 2, device=dev), imap, table,
                              torch.tensor([[0, 3, 0, 0]], dtype=torch.int32))         # the window leaves the accumulator
    with pytest.raises(ValueError):
        hip_ops.sw_finalize(x, imap, table, (4, 4, 5), (0, 0, 0))                      # acc is not at max(size, roi)
    # the library's own checks answer with its error code (nothing is launched): n >= 1, roi[k] >= 1
    import ctypes as C
    from ganslate_amd.hip.ops import _ptr, _stream
    roi, bad, pad = (C.c_int32 * 3)(2, 2, 2), (C.c_int32 * 3)(2, 0, 2), (C.c_int32 * 3)(0, 0, 0)
    out = torch.zeros(1, 1, 2, 2, 2, device=dev)
    assert hip_ops.lib.gs_sw_gather(_ptr(x), 1, 1, 4, 4, 4, _ptr(table), 0, roi, pad, 0.0, _ptr(out), _stream()) == 2
    assert hip_ops.lib.gs_sw_gather(_ptr(x), 1, 1, 4, 4, 4, _ptr(table), 1, bad, pad, 0.0, _ptr(out), _stream()) == 2
    assert hip_ops.lib.gs_sw_finalize(_ptr(x), 1, 1, 4, 4, 4, _ptr(table), 0, roi, pad, _ptr(imap), _ptr(x), _stream()) == 2
    assert b"gs_sw_finalize" in hip_ops.lib.gs_last_error()


def test_device_path_holds_no_count_volume(hip_ops):
    """peak device memory: the torch path holds the accumulator, `count` and the quotient; the kernels hold the accumulator
    and the result — at least one output volume less"""
    x = (torch.rand((1, 1, 48, 64, 64), generator=torch.Generator().manual_seed(11)) * 2 - 1).to(hip_ops.device)
    volume_bytes = x.numel() * 4
    peaks = {}
    for kernels in (False, True):
        inf = SlidingWindowInferer((32, 32, 32), 4, 0.5, "gaussian", cval=CVAL, device_kernels=kernels)
        out = inf(x, lambda w: w)                              # warm: the importance map is cached, code objects are loaded
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = inf(x, lambda w: w)
        torch.cuda.synchronize()
        peaks[kernels] = torch.cuda.max_memory_allocated() - base
        assert torch.allclose(out, x, atol=1e-6)
        del out
    print(f"peak bytes above the input: torch path {peaks[False]}, kernels {peaks[True]}, one volume {volume_bytes}")
    assert peaks[False] - peaks[True] >= volume_bytes, peaks


def test_predictor_sees_the_same_batches_in_the_same_order(hip_ops):
    shape, roi, overlap, mode, sw = (2, 2, 9, 13, 11), (4, 7, 5), 0.4, "gaussian", 3
    x = (torch.rand(shape, generator=torch.Generator().manual_seed(13)) * 2 - 1).to(hip_ops.device)
    seen = {}
    for kernels in (False, True):
        calls = seen.setdefault(kernels, [])

        def net(w, calls=calls):
            calls.append(w.detach().cpu().clone())
            return predictor(w)
        SlidingWindowInferer(roi, sw, overlap, mode, cval=CVAL, device_kernels=kernels)(x, net)
    assert [tuple(w.shape) for w in seen[True]] == [tuple(w.shape) for w in seen[False]]
    assert len(seen[True]) > 1 and max(w.shape[0] for w in seen[True]) == sw and seen[True][0].shape[1:] == (2, *roi)
    assert all(torch.equal(a, b) for a, b in zip(seen[True], seen[False]))
