"""Integer domain, bit for bit: every conv / dgrad / wgrad path of libganslate_hip.so against the oracle on the data of
tests/exact.py, with `torch.equal` (tests/test_exact_cpu.py pins the oracle to a float64 statement of each layer on the same
cases, so equality with the oracle is equality with float64). Products of small integers are exact in fp32 and integer sums
below 2^24 are exact in any order, so no summation order, split of K or accumulation tree may change a bit: a mismatch is a
wrong element, tap, border index, slot or rounding. Every case passes exact.assert_exact_domain (computed from the float64
reference alone) before it is used; a W-folded spec is the folded conv itself, on the folded layer's own domains.

Paths are forced the way tests/test_ops_gpu.py forces them (option set in try / finally and restored, planning queries
assert that the path under test took the layer); the case lists are that module's. Output buffers are zeros, statistics
partials NaN, as there. Statistics are compared as PARTIALS summed over slots in float64, never as mean / rstd.

Not here (they divide, take roots or exponentials): norm, Adam, loss, attention, PatchNCE kernels; `tanh`; lrelu with a
slope that is not a power of two.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ganslate_amd.hip import lib as L
from ganslate_amd.nn.native.spec import ConvSpec
from ganslate_amd.nn.native.twin import Twin
from oracle.ops_ref import RefOps
from tests import exact
from tests.test_exact_cpu import (ROUNDING_CASES, WALK_CASES, WALK_SEED, WALK_STRIP_CASE, oracle_dgrad, oracle_forward, oracle_wgrad,
                                  run_slice as _run_slice, slice_case as _slice_case, walk_id, walk_slice)
from tests.test_ops_gpu import (CONV_CASES, HWGRAD_FT_CASES, MULTI_CASES, PERSIST_CASES, PERSIST_PARITY_CASES, RING_CASES,
                                SPLITK_MULTI_CASES, STRIP_CASES, WGRAD_PAIR_CASES, WGRAD_ROWS_CASES, WIDE_HALO_CASES, _ids,
                                stats_slots)

pytestmark = pytest.mark.gpu

_ORACLE = {}


def cached(kind, c, fn, *args):
    """oracle results are computed once per (case, kind, arguments): the forced-path tests reuse them"""
    key = (id(c), kind) + args
    if key not in _ORACLE:
        _ORACLE[key] = fn(c, *args)
    return _ORACLE[key]


def hip_forward(ops, c, act="none", slope=0.2):
    """HIP forward of a case -> (bf16 output, float64 statistics partials summed over slots [N, 2, C]); every slot written"""
    low, N, dev = c.low, c.N, ops.device
    Co = low.fwd[0].Co
    y = torch.zeros(N, *low.out_dims, Co, dtype=torch.bfloat16, device=dev)
    slots, offs = stats_slots(ops, low, low.fwd, N)
    part = torch.full((N * slots * 2 * Co,), float("nan"), dtype=torch.float32, device=dev)
    ops.gconv_classes(low.fwd, c.xa.to(dev), c.fpack.to(dev), c.bias.to(dev), y, act=act, slope=slope, stats=part,
                      stats_slots=slots, stats_slot0s=offs)
    torch.cuda.synchronize()
    part = part.cpu()
    assert not torch.isnan(part).any(), "a statistics slot was not written"
    return y.cpu(), part.view(N, slots, 2, Co).double().sum(1)


def hip_dgrad(ops, c):
    dev = ops.device
    gx = torch.zeros(c.N, *c.low.dgrad_dims, c.low.dgrad[0].Co, dtype=torch.bfloat16, device=dev)
    ops.gconv_classes(c.low.dgrad, c.gy.to(dev), c.dpack.to(dev), None, gx)
    torch.cuda.synchronize()
    return gx.cpu()


def hip_wgrad(ops, c, prefill_w=0.0, prefill_b=0.0, **kw):
    spec, dev = c.spec, ops.device
    a, gt = (c.gy, c.xa) if spec.kind == "conv" else (c.xa, c.gy)
    dw = torch.full((spec.P * spec.T * spec.Q,), prefill_w, dtype=torch.float32, device=dev)
    ops.wgrad(c.low.wgrad, a.to(dev), gt.to(dev), dw, **kw)
    db = torch.full((spec.cout_p,), prefill_b, dtype=torch.float32, device=dev)
    ops.bias_grad(c.gy.to(dev), spec.cout_p, db)
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu()


def check_forward(ops, c, what, act="none", slope=0.2, stats=True):
    y_ref, s_ref = cached("fwd", c, oracle_forward, act, slope)
    y, s = hip_forward(ops, c, act, slope)
    dec = None if c.spec.wfold else (c.spec, c.xa, c.w, c.b)
    exact.assert_identical(y, y_ref, f"{what}: forward", decompose=dec if act == "none" else None)
    if stats:
        exact.assert_identical(s, s_ref, f"{what}: statistics partials (sum, sum of squares) summed over slots")
    return y, s


def check_dgrad(ops, c, what):
    exact.assert_identical(hip_dgrad(ops, c), cached("dgrad", c, oracle_dgrad), f"{what}: data gradient")


def check_wgrad(ops, c, what, **kw):
    dw_ref, db_ref = cached("wgrad", c, oracle_wgrad, 7.0, -5.0)
    dw, db = hip_wgrad(ops, c, 7.0, -5.0, **kw)
    sp = c.spec
    exact.assert_identical(dw.view(sp.P, sp.T, sp.Q), dw_ref.view(sp.P, sp.T, sp.Q), f"{what}: weight gradient [P][T][Q]")
    exact.assert_identical(db, db_ref, f"{what}: bias gradient")


def case_of(case, **kw):
    return exact.make_case(case[0], case[1], case[2:], **kw)


# ---- every layer on the paths the library picks by itself -------------------------------------------------------------------
@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_forward_and_statistics(hip_ops, case):
    check_forward(hip_ops, case_of(case, check=("fwd",)), "default path")


@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_data_gradient(hip_ops, case):
    check_dgrad(hip_ops, case_of(case, check=("dgrad",)), "default path")


@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_weight_and_bias_gradient(hip_ops, case):
    """accumulate semantics onto an integer prefill (7 in dw, -5 in db)"""
    check_wgrad(hip_ops, case_of(case, prefill=7.0, check=("wgrad",)), "default path")


@pytest.mark.parametrize("case", ROUNDING_CASES, ids=_ids)
def test_epilogue_rounds_to_nearest_even(hip_ops, case):
    """|y| in the thousands: the stored bf16 must be the RNE rounding of the exactly known integer (common.hpp:
    v_cvt_pk_bf16_f32); outputs only — statistics of values this large leave the exact domain"""
    check_forward(hip_ops, case_of(case, rounding=True, check=("fwd",)), "rounding variant", stats=False)


@pytest.mark.parametrize("act,slope", [("relu", 0.2), ("lrelu", 0.25), ("lrelu", 0.5)])
@pytest.mark.parametrize("case", [CONV_CASES[0], CONV_CASES[7], CONV_CASES[4], CONV_CASES[18]], ids=_ids)
def test_epilogue_activation(hip_ops, case, act, slope):
    """relu and power-of-two leaky slopes are exact; the statistics are those of the pre-activation values"""
    check_forward(hip_ops, case_of(case, check=("fwd",)), f"{act}({slope})", act, slope)


# ---- forced forward / data-gradient paths -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[0].k == 5 and c[0].dims == 3] +
                         [(ConvSpec("conv", 16, 16, 5, 1, 2, dims=3), 1, 20, 8, 40)], ids=_ids)
def test_narrow_halo_kernel_box_forms(hip_ops, case):
    c = case_of(case, check=("fwd", "dgrad"))
    slots = {}
    for box8 in (0, 1):
        with hip_ops.options(hconv_box8=box8):
            slots[box8] = hip_ops.stat_slots(c.low.fwd[0], c.N)
            check_forward(hip_ops, c, f"hconv_box8={box8}", "relu")
            check_dgrad(hip_ops, c, f"hconv_box8={box8}")
    if c.sizes[0] >= 8 and c.spec.cout <= 16:
        assert slots[1] < slots[0], slots          # the 8-deep boxes were really taken


@pytest.mark.parametrize("persist", [1, 0], ids=["persistent", "one-tile-per-workgroup"])
@pytest.mark.parametrize("case", WIDE_HALO_CASES, ids=_ids)
def test_wide_halo_kernel(hip_ops, case, persist):
    c = case_of(case, check=("fwd",))
    with hip_ops.options(hconvw_persist=persist):
        assert hip_ops.stat_slots(c.low.fwd[0], c.N) == (c.sizes[0] // 16) * (c.sizes[1] // 16), \
            "the wide halo kernel must take this layer"
        check_forward(hip_ops, c, f"hconvw (persist={persist})")


@pytest.mark.parametrize("case", STRIP_CASES, ids=_ids)
def test_boundary_convs_on_the_strip_kernels(hip_ops, case):
    c = case_of(case)
    g0 = c.low.fwd[0]
    for form, (on, regs) in (("regs", (1, 2)), ("lds", (1, 0)), ("im2col", (0, 0))):
        with hip_ops.options(hstrip=on, hstrip_regs=regs):
            if on and g0.Ci in (32, 64):
                rows = 16 if (regs and g0.Ci == 64 and g0.Co <= 32) else 32
                assert hip_ops.stat_slots(g0, c.N) == ((g0.Ho + rows - 1) // rows) * ((g0.Wo + 7) // 8)
            check_forward(hip_ops, c, f"hstrip {form}")
            check_dgrad(hip_ops, c, f"hstrip {form}")


# (the slice / accumulate form — _slice_case, _run_slice — lives in tests/test_exact_cpu.py, which pins it to float64)
def _check_slice(res, ref, base, cin, what):
    exact.assert_identical(res[0], ref[0], f"{what}: forward out of a channel slice")
    exact.assert_identical(res[1], ref[1], f"{what}: statistics partials")
    assert torch.equal(res[2][..., :cin], base[..., :cin]), f"{what}: the other half must be untouched"
    exact.assert_identical(res[2], ref[2], f"{what}: data gradient accumulated into a slice")


@pytest.mark.parametrize("seg", [0, 2], ids=["auto-segments", "two-segments"])
@pytest.mark.parametrize("sizes", [(8, 16, 16), (36, 32, 48)], ids=lambda s: "x".join(map(str, s)))
def test_register_resident_k5_kernel(hip_ops, sizes, seg):
    spec, N = ConvSpec("conv", 16, 16, 5, 1, 2, dims=3), 2
    c, x2, base = _slice_case(spec, N, sizes, 31)
    ref = cached("slice", c, lambda cc: _run_slice(RefOps(), "cpu", cc, x2, base))
    with hip_ops.options(hconv5_seg=seg, hconv5=1):
        on = _run_slice(hip_ops, hip_ops.device, c, x2, base)
    with hip_ops.options(hconv5_seg=seg, hconv5=0):
        off = _run_slice(hip_ops, hip_ops.device, c, x2, base)
    assert on[3] == (sizes[0] // 4) * (sizes[1] // 16) * (sizes[2] // 16) and off[3] != on[3], (on[3], off[3])
    _check_slice(on, ref, base, 16, "hconv5")
    _check_slice(off, ref, base, 16, "hconv5 = 0")


@pytest.mark.parametrize("case", [((32, 32), (32, 32, 32)), ((64, 64), (32, 32, 32)), ((16, 32), (33, 32, 40))],
                         ids=lambda c: "%dto%d-%s" % (c[0] + ("x".join(map(str, c[1])),)))
def test_persistent_narrow_volume_kernel(hip_ops, case):
    (cin, cout), sizes = case
    c, x2, base = _slice_case(ConvSpec("conv", cin, cout, 5, 1, 2, dims=3), 1, sizes, 61)
    ref = _run_slice(RefOps(), "cpu", c, x2, base)
    for v in (4, 0):
        with hip_ops.options(hconv2=v):
            _check_slice(_run_slice(hip_ops, hip_ops.device, c, x2, base), ref, base, cin, f"hconv2 = {v}")


# ---- persistent kernels walking several units per workgroup -----------------------------------------------------------------------
# WALK_CASES give every workgroup of hconv2_kernel / hconv5_kernel / hstripr_kernel a share of more than one box / segment /
# tile on the 256 CUs of the target: the hand-off from one unit to the next (the next unit's staging under the current tap
# loop, the epilogue between them, buffer parities and statistics scratch reused) is then held bit for bit. Each test restates
# its kernel's launch rule from the CU count and the slot query and asserts the depth the case claims BEFORE it compares: a
# case that does not walk must not pass on that footing. On another CU count the volume cases skip with the numbers.
TARGET_CUS = 256


def _assert_walk(what, units, grid, depth, uneven, cus=None):
    """workgroup i takes units i, i + grid, i + 2 * grid, ...: the deepest walk is ceil(units / grid), the shallowest
    floor(units / grid). cus: the CU count the grid was derived from, where it was"""
    got = -(-units // grid)
    line = f"{what}: {units} units on {grid} workgroups, walk depth {got}, shallowest {units // grid}"
    if cus is not None and cus != TARGET_CUS:
        pytest.skip(f"{line} on {cus} CUs; the case is sized for {TARGET_CUS} CUs (depth {depth})")
    print(line)
    assert got == depth and (units % grid != 0) == uneven and (uneven or units // grid == depth), line


def _hconv2_grid(ops, g, N, cus):
    """csrc/hconv.hip restated -> (boxes, workgroups per channel group, boxes per workgroup). plan(), `h.TI = ...` to
    `h.cog = ...`: TI tiles of 16 output channels per workgroup (two; one for <= 16 channels and for the small volumes of
    option values 3 / 4), cog channel groups over blockIdx.y. gs_hconv_try, `gmax`, `per`, `groups`: one workgroup per CU with
    the channel groups side by side, equal shares. hconv2_kernel: `for (; box < nboxes; box += gridDim.x)`."""
    boxes = N * ops.stat_slots(g, N)
    v = ops.get_option("hconv2")
    small = (v >= 3 and g.Co == 32 and boxes * 2 <= 256) or (v >= 4 and g.Co == 64 and boxes * 4 <= 256)
    TI = 1 if g.Co <= 16 or small else 2
    cog = -(-g.Co // (TI * 16))
    gmax = max(cus // cog, 1)
    per = -(-boxes // gmax)
    return boxes, -(-boxes // per), per


@pytest.mark.parametrize("case", [c for c in WALK_CASES if c[0] == "hconv2"], ids=walk_id)
def test_persistent_volume_kernel_walks_several_boxes(hip_ops, case):
    """hconv2_kernel with 2 - 3 boxes per workgroup and uneven shares (last_unit differs between workgroups): box -> box with
    two / four channel chunks per box and with one (the halo buffer parity flips per box), forward with statistics out of a
    slice and the accumulate epilogue between two boxes' staging; hconv2 = 0, the one-box-per-workgroup kernels, alongside"""
    _, cin, cout, N, sizes, launches, depth, uneven = case
    cus = torch.cuda.get_device_properties(hip_ops.device).multi_processor_count
    c, x2, base, ref = walk_slice(case)
    under = {"fwd": c.low.fwd[0], "dgrad": c.low.dgrad[0]}
    grid8 = int(np.prod([(s + 7) // 8 for s in sizes]))
    with hip_ops.options(hconv2=0):
        slots0 = {k: hip_ops.stat_slots(under[k], N) for k in launches}
    with hip_ops.options(hconv2=4):
        for k in launches:
            g = under[k]
            # more than 16 output channels on 8-deep boxes is hconv2_kernel alone (plan(), `h.NW = ...`: hconv_kernel's are 4 deep)
            assert g.Co > 16 and hip_ops.stat_slots(g, N) == grid8 != slots0[k], "hconv2_kernel must take this launch"
            boxes, grid, per = _hconv2_grid(hip_ops, g, N, cus)
            _assert_walk(f"hconv2 {k} {g.Ci} -> {g.Co}", boxes, grid, depth, uneven, cus)
            assert per == depth
        on = _run_slice(hip_ops, hip_ops.device, c, x2, base)
    with hip_ops.options(hconv2=0):
        off = _run_slice(hip_ops, hip_ops.device, c, x2, base)
    if "fwd" in launches:
        assert on[3] == grid8 != off[3], (on[3], off[3])
    _check_slice(on, ref, base, cin, "hconv2 = 4")
    _check_slice(off, ref, base, cin, "hconv2 = 0")


def test_register_resident_k5_kernel_walks_several_segments(hip_ops):
    """hconv5_kernel with two work items per workgroup: every workgroup restages all planes for a second segment, of another
    column, while the first one's stores drain; three segments per column, the middle one with its z halo from real planes on
    both sides, the last one ragged"""
    case, = [c for c in WALK_CASES if c[0] == "hconv5"]
    _, cin, cout, N, (D, H, W), launches, depth, uneven = case
    cus = torch.cuda.get_device_properties(hip_ops.device).multi_processor_count
    c, x2, base, ref = walk_slice(case)
    with hip_ops.options(hconv5_seg=0, hconv5=1):
        for g in (c.low.fwd[0], c.low.dgrad[0]):
            assert hip_ops.stat_slots(g, N) == (D // 4) * (H // 16) * (W // 16), "hconv5_kernel must take this launch"
        # csrc/hconv5.hip gs_hconv5_try, `columns` to `grid`, restated: columns of 16 x 16 voxels walked in steps of 4 planes are
        # cut into z segments until every CU has a workgroup; equal shares of whole segments. hconv5_kernel: `for (int work =
        # blockIdx.x; work < p.nwork; work += gridDim.x)`, `seg = b % p.nseg`, `nsteps = min(p.seg_steps, ...)` for the last one
        columns, steps = N * (H // 16) * (W // 16), D // 4
        nseg = min(max(-(-cus // columns), 1), steps)
        seg_steps = -(-steps // nseg)
        nseg = -(-steps // seg_steps)
        nwork = columns * nseg
        per = -(-nwork // cus)
        grid = -(-nwork // per)
        _assert_walk(f"hconv5 {columns} columns x {nseg} segments of <= {seg_steps} steps", nwork, grid, depth, uneven, cus)
        assert per == depth and [min(seg_steps, steps - s * seg_steps) for s in range(nseg)] == [3, 3, 1]
        assert grid % nseg == 0 and grid // nseg < columns, "a workgroup's second unit is a segment of ANOTHER column"
        on = _run_slice(hip_ops, hip_ops.device, c, x2, base)
    with hip_ops.options(hconv5_seg=0, hconv5=0):
        off = _run_slice(hip_ops, hip_ops.device, c, x2, base)
    assert on[3] == (D // 4) * (H // 16) * (W // 16) and off[3] != on[3], (on[3], off[3])
    _check_slice(on, ref, base, cin, "hconv5")
    _check_slice(off, ref, base, cin, "hconv5 = 0")


def test_strip_register_kernel_walks_several_tiles(hip_ops):
    """hstripr_kernel<32,64,32>'s forward WITH statistics on more tiles than workgroups (160 of the 512 walk two; ragged tile
    rows), and the <64,32,16> data gradient of the same layer (2 - 3 tiles per workgroup)"""
    spec, N, sizes = WALK_STRIP_CASE[0], WALK_STRIP_CASE[1], WALK_STRIP_CASE[2:]
    c = exact.make_case(spec, N, sizes, seed=WALK_SEED, check=("fwd", "dgrad"))
    with hip_ops.options(hstrip=1, hstrip_regs=2):
        # csrc/hstrip.hip restated. plan(), `tr = h.ci == 32 ? 32 : 16`: the register form takes 32 -> 64 channels on tiles of
        # 32 rows x 8 columns and 64 -> 32 on 16 x 8. gs_hstrip_try, `groups = blocks < 512 ? blocks : 512`. hstripr_kernel:
        # `for (int tile = tile0 + gx; tile < ntiles; tile += gnum)`, gnum = gridDim.x for one network
        for g, chans, rows, tiles_want, depth, what in ((c.low.fwd[0], (32, 64), 32, 672, 2, "forward with statistics"),
                                                        (c.low.dgrad[0], (64, 32), 16, 1248, 3, "data gradient")):
            per_img = ((g.Ho + rows - 1) // rows) * ((g.Wo + 7) // 8)
            assert (g.Ci, g.Co) == chans and hip_ops.stat_slots(g, N) == per_img, "the register strip kernel must take this launch"
            tiles = N * per_img
            assert tiles == tiles_want and tiles > 512 and g.Ho % rows, (tiles, g.Ho)
            _assert_walk(f"hstripr {what}", tiles, min(tiles, 512), depth, True)
        check_forward(hip_ops, c, "hstripr walk")
        check_dgrad(hip_ops, c, "hstripr walk")


def test_accumulate_through_split_k(hip_ops):
    spec, N, sizes = ConvSpec("conv", 64, 64, 5, 1, 2, dims=3), 1, (16, 16, 16)
    c, x2, base = _slice_case(spec, N, sizes, 23)
    d = hip_ops._gdesc(c.low.dgrad[0], N, 64, 0, 128, 64, "none", 0.2, 0, 0, True)
    assert hip_ops._splitk_floats(d) > 0, "the case must run split-K"
    ref = _run_slice(RefOps(), "cpu", c, x2, base)
    _check_slice(_run_slice(hip_ops, hip_ops.device, c, x2, base), ref, base, 64, "split-K accumulate")


@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[0].kind == "conv" and c[0].cin == 512 and c[0].stride == 2], ids=_ids)
@pytest.mark.parametrize("on", [1, 0])
def test_split_k_on_the_bottleneck_layers(hip_ops, case, on):
    """the single-class forward of the U-Net bottleneck convs with and without split-K (the transposed sibling's classes go
    through the merged split-K launch: test_split_k_over_merged_parity_classes); statistics come out of the finalize pass"""
    c = case_of(case, check=("fwd", "dgrad"))
    with hip_ops.options(splitk=on):
        g0 = c.low.fwd[0]
        slots = hip_ops.stat_slots(g0, c.N)
        d = hip_ops._gdesc(g0, c.N, c.xa.shape[-1], 0, g0.Co, 0, "none", 0.2, slots, 0)      # the launch check_forward makes
        assert (hip_ops._splitk_floats(d) > 0) == bool(on), "split-K must follow the option on this layer"
        check_forward(hip_ops, c, f"splitk={on}")
        check_dgrad(hip_ops, c, f"splitk={on}")


@pytest.mark.parametrize("sizes", [(16, 32, 48), (17, 33, 35)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("chans", [(32, 1), (1, 32), (64, 3), (16, 12)], ids=lambda c: "%dto%d" % c)
def test_pointwise_kernels(hip_ops, chans, sizes):
    c = exact.make_case(ConvSpec("conv", chans[0], chans[1], 1, 1, 0, dims=3), 2, sizes, seed=41, prefill=7.0)
    for on in (1, 0):
        with hip_ops.options(pwise=on):
            check_forward(hip_ops, c, f"pwise={on}", "lrelu", 0.25)
            check_dgrad(hip_ops, c, f"pwise={on}")
            check_wgrad(hip_ops, c, f"pwise={on}")


@pytest.mark.parametrize("cout1", ["1", "0"])
@pytest.mark.parametrize("case", [(512, 16, 31, 31), (256, 3, 17, 20), (64, 2, 9, 33)], ids=lambda c: "x".join(map(str, c)))
def test_one_output_channel_layer(hip_ops, case, cout1, monkeypatch):
    """cout1.hip (vector ALUs) and the matrix-core kernels (GS_COUT1=0): forward and weight gradient; padding channels zero"""
    Ci, N, H, W = case
    monkeypatch.setenv("GS_COUT1", cout1)
    c = exact.make_case(ConvSpec("conv", Ci, 1, 4, 1, 1), N, (H, W), seed=61, prefill=7.0, check=("fwd", "wgrad"))
    assert c.low.fwd[0].co_real == 1 and c.low.wgrad.p_real == 1
    y, _ = check_forward(hip_ops, c, f"GS_COUT1={cout1}")
    assert not y[..., 1:].any(), "padding channels stay zero"
    check_wgrad(hip_ops, c, f"GS_COUT1={cout1}")


@pytest.mark.parametrize("case", PERSIST_CASES[3:], ids=_ids)
@pytest.mark.parametrize("persist", [1000, 0])
def test_persistent_im2col_kernel(hip_ops, case, persist):
    """(the three smaller launches of PERSIST_CASES: the oracle of the 16 x 256 x 256 ones costs more than the rest of the file)"""
    c = case_of(case, check=("fwd",))
    g0 = c.low.fwd[0]
    with hip_ops.options(gconv_persist=persist):
        # pconv.hip takes a 256 x 128 tile launch with more tiles than CUs and at most `gconv_persist` K-steps: this one is
        tiles = c.N * hip_ops.stat_slots(g0, c.N) * ((g0.Co + 127) // 128)
        assert hip_ops.tile_m(g0, c.N) == 256 and tiles > torch.cuda.get_device_properties(hip_ops.device).multi_processor_count
        assert 4 <= g0.Kp // 64 <= 1000
        check_forward(hip_ops, c, f"gconv_persist={persist}", "relu")


@pytest.mark.parametrize("case", MULTI_CASES, ids=_ids)
@pytest.mark.parametrize("path", ["hconvt", "merged", "per-class"])
def test_parity_classes(hip_ops, case, path):
    """the output-parity classes of a stride-2 layer — forward (bias, lrelu 0.25, statistics) and data gradient — on the
    halo-resident class kernel (hconvt = 1, persistent and one tile per workgroup), as one merged im2col launch, and class by class"""
    c = case_of(case, check=("fwd", "dgrad"))
    assert len(c.low.fwd) > 1 or len(c.low.dgrad) > 1
    opts = {"hconvt": dict(hconvt=1, gconv_multi=1), "merged": dict(hconvt=0, gconv_multi=1),
            "per-class": dict(hconvt=0, gconv_multi=0)}[path]
    for persist in ((1, 0) if path == "hconvt" else (1,)):
        with hip_ops.options(hconvt_persist=persist, **opts):
            for classes in (c.low.fwd, c.low.dgrad):       # the class kernel takes exactly the layers its restatement names
                if len(classes) > 1:
                    taken = hip_ops.fused_multi_plan(classes, c.N, classes[0].Co) is not None
                    assert taken == (path == "hconvt" and RefOps().fused_multi_plan(classes, c.N, classes[0].Co) is not None)
            check_forward(hip_ops, c, f"{path} (hconvt_persist={persist})", "lrelu", 0.25)
            check_dgrad(hip_ops, c, f"{path} (hconvt_persist={persist})")


@pytest.mark.parametrize("case", [PERSIST_PARITY_CASES[1], PERSIST_PARITY_CASES[4]], ids=_ids)
@pytest.mark.parametrize("persist", [1, 0])
def test_persistent_parity_class_kernel(hip_ops, case, persist):
    """hconvt.hip with more tiles than CUs (persistent workgroups: K-step stream, weight ring and halo buffers run on across
    tiles) and the same launch as one tile per workgroup: u128's forward (two channel tiles, uneven tile counts) and the
    PatchGAN k4 data gradient. (PERSIST_PARITY_CASES[0], [2], [3] are the same two patterns at 2 - 4 times the oracle cost.)"""
    c = case_of(case, check=("fwd", "dgrad"))
    cus = torch.cuda.get_device_properties(hip_ops.device).multi_processor_count
    with hip_ops.options(hconvt=1, hconvt_persist=persist):
        ran = 0
        for classes, check in ((c.low.fwd, check_forward), (c.low.dgrad, check_dgrad)):
            if len(classes) != 4:
                continue
            g0 = classes[0]
            assert hip_ops.fused_multi_plan(classes, c.N, g0.Co) is not None, "the class kernel must take this layer"
            tiles = c.N * (g0.Hc // 16) * (g0.Wc // 16) * (g0.Co // 64)          # hconvt.hip: persistent when tiles > CUs
            assert tiles > cus and g0.Co // 64 <= cus, (tiles, cus)
            check(hip_ops, c, f"hconvt_persist={persist}", *(("relu",) if check is check_forward else ()))
            ran += 1
        assert ran


@pytest.mark.parametrize("case", SPLITK_MULTI_CASES, ids=_ids)
@pytest.mark.parametrize("on", [1, 0])
def test_split_k_over_merged_parity_classes(hip_ops, case, on):
    c = case_of(case, check=("fwd", "dgrad"))
    fwd_multi, dg_multi = len(c.low.fwd) == 4, len(c.low.dgrad) == 4
    assert fwd_multi or dg_multi
    with hip_ops.options(splitk_multi=on):
        classes = c.low.fwd if fwd_multi else c.low.dgrad
        descs = [hip_ops._gdesc(g, c.N, (c.xa if fwd_multi else c.gy).shape[-1], 0,
                                (c.spec.cout_p if fwd_multi else c.spec.cin_p), 0, "none", 0.2, 0, 0) for g in classes]
        arr = (C.POINTER(L.GConvDesc) * 4)(*[C.pointer(d) for d in descs])
        assert (int(hip_ops.lib.gs_gconv_multi_splitk_ws_floats(arr, 4)) > 0) == bool(on)
        if fwd_multi:
            check_forward(hip_ops, c, f"splitk_multi={on}", "lrelu", 0.25)
        if dg_multi:
            check_dgrad(hip_ops, c, f"splitk_multi={on}")


# ---- data gradient with the fused norm-backward sums ----------------------------------------------------------------------------
def _fused_operands(c, with_g2, act, seed):
    """the consumer's norm on the exact domain: integer raw output y, integer mean, rstd 1 or 2 per channel -> yh, gh integer"""
    spec, N, sizes = c.spec, c.N, c.sizes
    Cc = spec.cin_p
    g = torch.Generator().manual_seed(seed)
    y = exact.int_act(N, sizes, Cc, Cc, g, 0.5, 3)
    g2 = exact.int_act(N, sizes, Cc, Cc, g, 0.25, 3) if with_g2 else None
    mr = torch.empty(N, 2, Cc)
    mr[:, 0] = torch.randint(-2, 3, (N, Cc), generator=g).float()
    mr[:, 1] = 2.0 ** torch.randint(0, 2, (N, Cc), generator=g).float()
    return y, g2, mr.reshape(-1).contiguous()


def _fused_domain(c, y, g2, mr, act, gx_folded64):
    N, Cc = c.N, c.spec.cin_p
    bc = (N,) + (1,) * c.spec.dims + (Cc,)
    m = mr.view(N, 2, Cc).double()
    yh = (y.double() - m[:, 0].reshape(bc)) * m[:, 1].reshape(bc)
    gf = torch.zeros_like(yh)
    gf[..., :gx_folded64.shape[-1]] = gx_folded64
    if g2 is not None:
        gf = gf + g2.double()
    gh = gf * ((yh > 0).double() if act == "relu" else 1.0)
    exact.assert_exact_domain(c.spec, fused=(gh, yh))


FUSED_CASES = [
    (ConvSpec("conv", 256, 256, 3, 1, 1, pad_mode="reflect"), 2, 16, 16),
    (ConvSpec("conv", 256, 256, 3, 1, 1, pad_mode="reflect"), 8, 64, 64),                       # 320-pixel tiles
    (ConvSpec("conv", 128, 256, 3, 1, 1, pad_mode="replicate", dims=3), 1, 6, 10, 12),
    (ConvSpec("conv", 128, 128, 4, 1, 1), 2, 19, 23),                                          # zero padding: no fold
]          # (the cases of test_ops_gpu.test_dgrad_with_fused_norm_reduction)


def _run_fused(ops, dev, c, g, out_dims, plan, fold, y, g2, mr, act):
    """one fused data-gradient launch of class g -> (bf16 gradient, float64 sums of gh, gh * yh, yh over slots [N, 3, C])"""
    spec, N, Cc = c.spec, c.N, c.spec.cin_p
    plan[1].fill_(float("nan"))
    gx = torch.zeros(N, *out_dims, Cc, dtype=torch.bfloat16, device=dev)
    ops.gconv(g, c.gy.to(dev), c.dpack.to(dev), None, gx,
              fuse={"y": y.to(dev), "mean_rstd": mr.to(dev), "g2": None if g2 is None else g2.to(dev), "partial": plan[1],
                    "fold": fold, "fold_mode": spec.pad_mode if c.low.dgrad_fold else "reflect", "act": act, "slope": 0.2})
    if dev != "cpu":
        torch.cuda.synchronize()
    sums = plan[1][:N * plan[0] * 3 * Cc].cpu()
    assert not torch.isnan(sums).any(), "a slot of the fused sums was not written"
    return gx.cpu(), sums.view(N, plan[0], 3, Cc).double().sum(1)


def _fused_case(case, with_g2, act):
    c = case_of(case, check=("dgrad",))
    y, g2, mr = _fused_operands(c, with_g2, act, 26)
    folded = exact.dgrad_ref64(c.spec, c.sizes, c.gy, c.w, folded=True)
    exact.assert_exact_domain(c.spec, gy=c.gy, w=c.w, sizes=c.sizes, folded=True)     # the folded gradient is a bf16 integer too
    _fused_domain(c, y, g2, mr, act, folded)
    return c, y, g2, mr


@pytest.mark.parametrize("case", FUSED_CASES, ids=_ids)
@pytest.mark.parametrize("with_g2,act", [(False, "relu"), (True, "none")])
def test_data_gradient_with_fused_norm_sums(hip_ops, case, with_g2, act):
    """gs_gconv_forward_fused on the padded domain: the gradient and the three sums (gh, gh * yh, yh) summed over slots"""
    c, y, g2, mr = _fused_case(case, with_g2, act)
    N, Cc, low = c.N, c.spec.cin_p, c.low
    res = []
    for ops, dev in ((RefOps(), "cpu"), (hip_ops, hip_ops.device)):
        plan = ops.fused_norm_plan(low.dgrad[0], N, Cc, force=True)
        assert plan is not None
        res.append(_run_fused(ops, dev, c, low.dgrad[0], low.dgrad_dims, plan, low.dgrad_fold, y, g2, mr, act))
    exact.assert_identical(res[1][0], res[0][0], "fused launch: data gradient")
    exact.assert_identical(res[1][1], res[0][1], "fused launch: sums of gh, gh * yh, yh over slots")


@pytest.mark.parametrize("case", RING_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("with_g2,act", [(False, "relu"), (True, "none")])
def test_data_gradient_ring_form(hip_ops, case, with_g2, act):
    """gs_gconv_ring_slots (hconvw.hip RING): the fused data gradient of a reflect-padded 3x3 conv on the UNPADDED domain — the
    launch folds the ring itself, in fp32 before the storage rounding — and its sums: square and rectangular box grids, one
    and two channel tiles, 2 to 48 images"""
    Cc, N, H, W = case
    c, y, g2, mr = _fused_case((ConvSpec("conv", Cc, Cc, 3, 1, 1, pad_mode="reflect"), N, H, W), with_g2, act)
    low = c.low
    assert low.dgrad_ring is not None
    ref_ops = RefOps()
    ref_ops.ring_min_blocks = 0
    res = []
    for ops, dev in ((ref_ops, "cpu"), (hip_ops, hip_ops.device)):
        ring = ops.fused_ring_plan(low.dgrad_ring, N, Cc)
        assert ring is not None, "case must be eligible for the ring form"
        res.append(_run_fused(ops, dev, c, low.dgrad_ring, (H, W), ring, 1, y, g2, mr, act))
    want = exact.dgrad_ref64(c.spec, c.sizes, c.gy, c.w, folded=True)
    exact.assert_identical(res[0][0], exact.rne_bf16(want), "oracle ring form vs float64 through the pad layer")
    exact.assert_identical(res[1][0], res[0][0], "ring form: data gradient on the unpadded domain")
    exact.assert_identical(res[1][1], res[0][1], "ring form: sums of gh, gh * yh, yh over slots")


# ---- forced weight-gradient paths -------------------------------------------------------------------------------------------------
# (GS_HWGRAD_PLANES only changes the 3-D lowering: the 2-D cases run once. Of the two BASELINE-size launches the 32^3 one stays,
# on the depth planes; the 8 x 64 x 64 one runs in test_weight_and_bias_gradient and test_twin_batch, the im2col form of a
# 3 x 3 x 3 layer on the small volume)
_BIG = lambda c: c[1] * int(np.prod(c[2:])) >= 32768
@pytest.mark.parametrize("case,planes", [(c, p) for c in WGRAD_PAIR_CASES for p in ("1", "0")
                                         if (p == "1" or c[0].dims == 3) and not (_BIG(c) and (p == "0" or c[0].dims == 2))],
                         ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_weight_gradient_pair(hip_ops, case, planes, monkeypatch):
    """gs_wgrad_pair on the wide halo kernel / three depth planes / the im2col kernel: two accumulations in one launch"""
    monkeypatch.setenv("GS_HWGRAD_PLANES", planes)
    hip_ops.sync_options()
    c1 = case_of(case, seed=27, prefill=7.0, check=("wgrad",))
    c2 = case_of(case, seed=28, prefill=7.0, check=("wgrad",))
    spec, dev = c1.spec, hip_ops.device
    # one merged launch for the stride-1 layers, two launches for the strided one (the rule the library shares with the oracle;
    # the library has no query for it)
    assert RefOps.can_merge_wgrad(c1.low.wgrad) == (spec.stride == 1)
    res = []
    for ops, d in ((RefOps(), "cpu"), (hip_ops, dev)):
        dw = torch.full((spec.P * spec.T * spec.Q,), 7.0, dtype=torch.float32, device=d)
        ops.wgrad(c1.low.wgrad, c1.gy.to(d), c1.xa.to(d), dw, pair=(c2.gy.to(d), c2.xa.to(d)))
        res.append(dw.cpu())
    exact.assert_identical(res[1].view(spec.P, spec.T, spec.Q), res[0].view(spec.P, spec.T, spec.Q), "weight gradient pair")


# (the slab reduction of a launch with several pixel splits needs a 16-byte aligned dw: those cases run aligned only)
@pytest.mark.parametrize("case,misalign", [(c, m) for c in WGRAD_ROWS_CASES for m in (0, 1)
                                           if not (m and c[1] * int(np.prod(c[2:])) > 256)],
                         ids=lambda v: f"offset{v}" if isinstance(v, int) else _ids(v))
@pytest.mark.parametrize("rows", [1, 0])
def test_weight_gradient_epilogues(hip_ops, case, misalign, rows):
    """wgrad_kernel's two epilogues (option wgrad_rows), dw on and off a 16-byte boundary, and — aligned only — into a
    fresh buffer (dw_fresh): onto an integer prefill, the floats around dw untouched"""
    c = case_of(case, seed=41, prefill=8.0, check=("wgrad",))
    spec, dev = c.spec, hip_ops.device
    n = spec.P * spec.T * spec.Q
    a, gt = (c.gy, c.xa) if spec.kind == "conv" else (c.xa, c.gy)
    pre = torch.randint(-8, 9, (n + 4,), generator=torch.Generator().manual_seed(5)).float()
    ref = pre.clone()
    RefOps().wgrad(c.low.wgrad, a, gt, ref[misalign:misalign + n])
    with hip_ops.options(wgrad_rows=rows):
        buf = pre.clone().to(dev)
        hip_ops.wgrad(c.low.wgrad, a.to(dev), gt.to(dev), buf[misalign:misalign + n])
        torch.cuda.synchronize()
        exact.assert_identical(buf.cpu(), ref, f"wgrad_rows={rows}, offset {misalign}")
        if not misalign:
            fresh = torch.zeros(n, dtype=torch.float32, device=dev)
            hip_ops.wgrad(c.low.wgrad, a.to(dev), gt.to(dev), fresh, fresh=True)
            torch.cuda.synchronize()
            exact.assert_identical(fresh.cpu(), ref[:n] - pre[:n], f"wgrad_rows={rows}, fresh buffer")


@pytest.mark.parametrize("v", [2, 1])
def test_one_channel_volume_weight_gradient(hip_ops, v):
    c = exact.make_case(ConvSpec("conv", 256, 1, 4, 1, 1, dims=3), 2, (11, 15, 19), seed=51, prefill=7.0, check=("wgrad",))
    with hip_ops.options(hwgrad2=v):
        check_wgrad(hip_ops, c, f"hwgrad2={v}")


@pytest.mark.parametrize("flag", ["1", "0"])
@pytest.mark.parametrize("case", HWGRAD_FT_CASES[1:3], ids=_ids)      # the output conv at 256 x 256, the stem on ragged boxes
def test_few_tap_halo_resident_weight_gradient(hip_ops, case, flag, monkeypatch):
    """hwgrad_ft_kernel and the im2col kernel (GS_HWGRAD_FT=0) on the W-folded boundary convs: operands of the folded layer,
    all padded channels live"""
    monkeypatch.setenv("GS_HWGRAD_FT", flag)
    hip_ops.sync_options()
    spec, N, sizes = case[0], case[1], case[2:]
    c = exact.make_case(spec, N, sizes, seed=17, prefill=7.0, check=("wgrad",))
    dev = hip_ops.device
    res = []
    for ops, d in ((RefOps(), "cpu"), (hip_ops, dev)):
        dw = torch.full((spec.P * spec.T * spec.Q,), 7.0, dtype=torch.float32, device=d)
        ops.wgrad(c.low.wgrad, c.gy.to(d), c.xa.to(d), dw)
        res.append(dw.cpu())
    exact.assert_identical(res[1].view(spec.P, spec.T, spec.Q), res[0].view(spec.P, spec.T, spec.Q), f"GS_HWGRAD_FT={flag}")


# ---- twin batches: one launch over the images of two networks ---------------------------------------------------------------------
def test_twin_batch(hip_ops):
    """forward with statistics, data gradient and weight gradient of the trunk conv as twin launches (a weight set per half of
    the batch) against the oracle's two halves"""
    spec, N, sizes = ConvSpec("conv", 256, 256, 3, 1, 1, pad_mode="reflect"), 6, (64, 64)       # 192 tiles: the smallest twin batch
    ca = exact.make_case(spec, N, sizes, seed=101, prefill=7.0)
    cb = exact.make_case(spec, N, sizes, seed=202, prefill=7.0)
    dev, low, Cp = hip_ops.device, ca.low, spec.cout_p
    assert hip_ops.twin_native(low.fwd[0], 2 * N), "the twin launch is what this test is about"
    x, gy = torch.cat([ca.xa, cb.xa]).to(dev), torch.cat([ca.gy, cb.gy]).to(dev)
    fp, dp = torch.stack([ca.fpack, cb.fpack]).to(dev), torch.stack([ca.dpack, cb.dpack]).to(dev)
    bs = torch.stack([ca.bias, cb.bias]).to(dev)
    slots, offs = stats_slots(hip_ops, low, low.fwd, 2 * N)
    y = torch.zeros(2 * N, *sizes, Cp, dtype=torch.bfloat16, device=dev)
    part = torch.full((2 * N * slots * 2 * Cp,), float("nan"), dtype=torch.float32, device=dev)
    hip_ops.gconv_classes(low.fwd, x, Twin(fp[0], fp[1]), Twin(bs[0], bs[1]), y, stats=part, stats_slots=slots, stats_slot0s=offs)
    gx = torch.zeros(2 * N, *low.dgrad_dims, spec.cin_p, dtype=torch.bfloat16, device=dev)
    hip_ops.gconv_classes(low.dgrad, gy, Twin(dp[0], dp[1]), None, gx)
    dw = torch.full((2, spec.master_numel), 7.0, device=dev)
    hip_ops.wgrad(low.wgrad, gy, x, Twin(dw[0], dw[1]))
    torch.cuda.synchronize()
    s = part.cpu().view(2 * N, slots, 2, Cp).double().sum(1)
    for h, c in enumerate((ca, cb)):
        y_ref, s_ref = cached("fwd", c, oracle_forward, "none", 0.2)
        exact.assert_identical(y[h * N:(h + 1) * N].cpu(), y_ref, f"twin forward, network {h}")
        exact.assert_identical(s[h * N:(h + 1) * N], s_ref, f"twin statistics partials, network {h}")
        exact.assert_identical(gx[h * N:(h + 1) * N].cpu(), cached("dgrad", c, oracle_dgrad), f"twin data gradient, network {h}")
        exact.assert_identical(dw[h].cpu(), cached("wgrad", c, oracle_wgrad, 7.0, -5.0)[0], f"twin weight gradient, network {h}")
