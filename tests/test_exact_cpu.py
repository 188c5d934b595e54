"""The oracle (oracle/ops_ref.py behind the lowering and the packs) is EXACT on the integer domain of tests/exact.py: forward
with statistics partials, data gradient, weight and bias gradient of every entry of CONV_CASES are `torch.equal` to a plain
float64 statement of the layer (exact.conv_ref64 & co: F.pad / F.conv / F.conv_transpose / autograd) after the one documented
storage rounding. That licenses the oracle as the comparand of test_exact_gpu.py, and every case passes through
exact.assert_exact_domain here first.

The W-folded specs (wfold="in" / "out") are stated as the FOLDED conv (vertical taps over folded channels, on the folded
layer's own input and output domains, every folded channel live) in float64, not as the un-folded layer: composing
image_unfold / shiftadd_to_image with the folded conv the way nn/native does needs the executor's border bookkeeping and is
pinned at network level by tests/test_lowering_cpu.py and tests/test_networks_cpu.py.

The sensitivity tests at the end state what the exact comparison sees that the bf16 tolerance of test_ops_gpu.py does not.
"""
import pytest
import torch

from ganslate_amd.nn.native.spec import ConvSpec
from oracle.ops_ref import RefOps
from tests import exact
from tests.test_ops_gpu import CONV_CASES, _ids, close_bf16, make_layer, stats_slots

pytestmark = []          # (test_ops_gpu's module-level gpu mark does not travel with its names)

TRUNK = (ConvSpec("conv", 256, 256, 3, 1, 1, pad_mode="reflect"), 2, 16, 16)
ROUNDING_CASES = [
    TRUNK,                                                                                 # trunk
    (ConvSpec("conv", 64, 128, 3, 2, 1), 2, 32, 32),                                       # stride 2
    (ConvSpec("convT", 256, 128, 3, 2, 1, 1), 2, 16, 16),                                  # transposed
    (ConvSpec("conv", 256, 256, 3, 1, 1, pad_mode="replicate", dims=3), 1, 8, 8, 8),      # 3-D
]

# The persistent kernels of the volume path with MORE THAN ONE unit per workgroup on the 256 CUs of the target, in the slice /
# accumulate form of slice_case (k5 s1 p2 volumes, seed 61): (kernel, cin, cout, N, sizes, launches that run on that kernel,
# units the deepest workgroup walks, whether the shares are uneven). test_exact_gpu.py restates each kernel's launch rule and
# asserts the last two; the smallest shapes that take the branches named.
WALK_CASES = [
    # hconv2_kernel (csrc/hconv.hip), 8 x 8 x 8 boxes
    ("hconv2", 32, 32, 1, (40, 56, 72), ("fwd", "dgrad"), 2, True),     # 315 boxes on 158 workgroups, two chunks per box
    ("hconv2", 64, 64, 1, (17, 40, 72), ("fwd", "dgrad"), 2, True),     # 135 on 68 x 2 channel groups, ragged depth, four chunks
    ("hconv2", 16, 32, 1, (49, 64, 80), ("fwd",), 3, True),             # 560 on 187, one chunk: the halo parity flips per box
    ("hconv2", 32, 16, 1, (49, 64, 80), ("dgrad",), 3, True),           # ... and that walk under the accumulate epilogue
    # hconv5_kernel (csrc/hconv5.hip): 98 columns x 3 segments of 3, 3 and 1 steps on 147 workgroups
    ("hconv5", 16, 16, 2, (28, 112, 112), ("fwd", "dgrad"), 2, False),
]
WALK_SEED = 61
# hstripr_kernel<32,64,32> forward WITH statistics (csrc/hstrip.hip): 3 x 7 x 32 = 672 tiles (ragged rows: 200 = 6 * 32 + 8) on
# 512 workgroups; its data gradient (<64,32,16>) has 3 x 13 x 32 = 1248
WALK_STRIP_CASE = (ConvSpec("conv", 3, 64, 7, 1, 3, pad_mode="reflect", wfold="in"), 3, 200, 256)


def walk_id(case):
    return "%s-%dto%d-%dx%s" % (case[0], case[1], case[2], case[3], "x".join(map(str, case[4])))


def oracle_forward(c, act="none", slope=0.2):
    """oracle forward of a case: (bf16 output, float64 statistics partials summed over slots [N, 2, C])"""
    low, N = c.low, c.N
    y = torch.zeros(N, *low.out_dims, low.fwd[0].Co, dtype=torch.bfloat16)
    slots = len(low.fwd)
    part = torch.full((N * slots * 2 * low.fwd[0].Co,), float("nan"), dtype=torch.float32)
    RefOps().gconv_classes(low.fwd, c.xa, c.fpack, c.bias, y, act=act, slope=slope, stats=part, stats_slots=slots,
                           stats_slot0s=list(range(slots)))
    return y, part.view(N, slots, 2, -1).double().sum(1)


def oracle_dgrad(c):
    gx = torch.zeros(c.N, *c.low.dgrad_dims, c.low.dgrad[0].Co, dtype=torch.bfloat16)
    RefOps().gconv_classes(c.low.dgrad, c.gy, c.dpack, None, gx)
    return gx


def oracle_wgrad(c, prefill_w=0.0, prefill_b=0.0):
    spec = c.spec
    a, gt = (c.gy, c.xa) if spec.kind == "conv" else (c.xa, c.gy)
    dw = torch.full((spec.P * spec.T * spec.Q,), prefill_w, dtype=torch.float32)
    RefOps().wgrad(c.low.wgrad, a, gt, dw)
    db = torch.full((spec.cout_p,), prefill_b, dtype=torch.float32)
    RefOps().bias_grad(c.gy, spec.cout_p, db)
    return dw, db


def slice_case(spec, N, sizes, seed):
    """a narrow volume layer that reads the upper half of a 2 * cin channel buffer and whose data gradient is accumulated into
    the upper half of an integer-filled one (the V-Net couplings)"""
    c = exact.make_case(spec, N, sizes, seed=seed, check=("fwd", "dgrad"))
    g = torch.Generator().manual_seed(seed + 7)
    d = c.dom
    x2 = exact.int_act(N, sizes, 2 * spec.cin, 2 * spec.cin, g, d["dx"], d["mag"])
    x2[..., spec.cin:] = c.xa
    base = exact.int_act(N, sizes, 2 * spec.cin, 2 * spec.cin, g, 0.5, 3)
    # accumulate: bf16(gx) + base, both integers; |gx| <= 256 by the precondition, so the sum (<= 259) rounds RNE on both sides
    return c, x2, base


def run_slice(ops, dev, c, x2, base, act="lrelu", slope=0.25):
    """-> (forward out of the slice, statistics partials summed over slots, the accumulated gradient buffer, slots per image)"""
    spec, low, N = c.spec, c.low, c.N
    y = torch.zeros(N, *low.out_dims, spec.cout_p, dtype=torch.bfloat16, device=dev)
    slots, offs = stats_slots(ops, low, low.fwd, N)
    part = torch.full((N * slots * 2 * spec.cout_p,), float("nan"), dtype=torch.float32, device=dev)
    ops.gconv_classes(low.fwd, x2.to(dev), c.fpack.to(dev), c.bias.to(dev), y, in_co=spec.cin, act=act, slope=slope, stats=part,
                      stats_slots=slots, stats_slot0s=offs)
    G = base.clone().to(dev)
    for gc in low.dgrad:
        ops.gconv(gc, c.gy.to(dev), c.dpack.to(dev), None, G, out_co=spec.cin, accumulate=True)
    if dev != "cpu":
        torch.cuda.synchronize()
    part = part.cpu()
    assert not torch.isnan(part).any()
    return y.cpu(), part.view(N, slots, 2, spec.cout_p).double().sum(1), G.cpu(), slots


_WALK = {}


def walk_slice(case):
    """(case, 2 * cin input buffer, integer base of the gradient buffer, the oracle's run_slice) of a WALK_CASES entry, built
    once per process: the pin below and the forced-path runs of test_exact_gpu.py share it"""
    if case not in _WALK:
        c, x2, base = slice_case(ConvSpec("conv", case[1], case[2], 5, 1, 2, dims=3), case[3], case[4], WALK_SEED)
        _WALK[case] = (c, x2, base, run_slice(RefOps(), "cpu", c, x2, base))
    return _WALK[case]


def padded(t64, c_pad, dtype):
    """float64 reference tensor -> storage dtype with zero padded channels"""
    out = torch.zeros(*t64.shape[:-1], c_pad, dtype=dtype)
    out[..., :t64.shape[-1]] = t64.float().to(dtype)
    return out


@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_oracle_forward_and_statistics_are_exact(case):
    spec, N, sizes = case[0], case[1], case[2:]
    c = exact.make_case(spec, N, sizes, check=("fwd",))
    y, stats = oracle_forward(c)
    ref = exact.conv_ref64(spec, c.xa, c.w, c.b)
    exact.assert_identical(y, padded(ref, spec.cout_p, torch.bfloat16), "oracle forward vs float64",
                           decompose=(spec, c.xa, c.w, c.b))
    co = exact.cout_of(spec)
    want = torch.zeros(N, 2, spec.cout_p, dtype=torch.float64)
    want[:, 0, :co] = ref.reshape(N, -1, co).sum(1)
    want[:, 1, :co] = (ref * ref).reshape(N, -1, co).sum(1)
    exact.assert_identical(stats, want, "oracle statistics partials (sum, sum of squares) vs float64")


@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_oracle_data_gradient_is_exact(case):
    spec, N, sizes = case[0], case[1], case[2:]
    c = exact.make_case(spec, N, sizes, check=("dgrad",))
    ref = exact.dgrad_ref64(spec, sizes, c.gy, c.w)
    exact.assert_identical(oracle_dgrad(c), padded(ref, spec.cin_p, torch.bfloat16), "oracle data gradient vs float64")


@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_oracle_weight_and_bias_gradient_are_exact(case):
    spec, N, sizes = case[0], case[1], case[2:]
    c = exact.make_case(spec, N, sizes, prefill=7.0, check=("wgrad",))
    dw, db = oracle_wgrad(c, 7.0, -5.0)            # accumulate semantics: onto an integer prefill
    want = exact.master_of(spec, exact.wgrad_ref64(spec, c.xa, c.gy).float()) + 7.0
    exact.assert_identical(dw.view(spec.P, spec.T, spec.Q), want, "oracle weight gradient vs float64")
    wb = torch.full((spec.cout_p,), -5.0)
    wb[:exact.cout_of(spec)] += exact.bias_grad_ref64(spec, c.gy).float()
    exact.assert_identical(db, wb, "oracle bias gradient vs float64")


@pytest.mark.parametrize("case", ROUNDING_CASES, ids=_ids)
def test_oracle_rounds_large_outputs_to_nearest_even(case):
    """input magnitudes up to 64: |y| reaches the thousands, where bf16 no longer holds the integer and the stored value
    must be the round-to-nearest-even of the exactly known one"""
    spec, N, sizes = case[0], case[1], case[2:]
    c = exact.make_case(spec, N, sizes, rounding=True, check=("fwd",))
    ref = exact.conv_ref64(spec, c.xa, c.w, c.b)
    assert ref.abs().max() >= 1000 and (exact.rne_bf16(ref).double() != ref).float().mean() > 0.25, \
        "the variant must reach values bf16 cannot hold"
    y, _ = oracle_forward(c)
    exact.assert_identical(y, padded(ref, spec.cout_p, torch.bfloat16), "oracle forward (rounding variant) vs float64")


@pytest.mark.parametrize("act,slope", [("relu", 0.2), ("lrelu", 0.25), ("lrelu", 0.5)])
def test_oracle_epilogue_activations_are_exact(act, slope):
    spec, N, sizes = TRUNK[0], TRUNK[1], TRUNK[2:]
    c = exact.make_case(spec, N, sizes, check=("fwd",))
    ref = exact.conv_ref64(spec, c.xa, c.w, c.b)
    ref = torch.where(ref > 0, ref, ref * (0.0 if act == "relu" else slope))
    y, _ = oracle_forward(c, act, slope)
    exact.assert_identical(y, padded(ref, spec.cout_p, torch.bfloat16), f"oracle forward + {act}({slope}) vs float64")


# ---- the cases of the persistent-walk tests ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WALK_CASES, ids=walk_id)
def test_oracle_slice_and_accumulate_forms_are_exact(case):
    """run_slice on the oracle against float64 stated directly: the forward of the UPPER half of the 2 * cin buffer (the lower
    half is live noise) with bias and lrelu(0.25), statistics of the pre-activation values, and the data gradient plus the
    integer base in the written half only — one RNE rounding of the exactly known sum"""
    c, x2, base, (y, stats, G, _) = walk_slice(case)
    spec, N, cin = c.spec, c.N, c.spec.cin
    assert spec.cin_p == cin and spec.cout_p == spec.cout and torch.equal(x2[..., cin:], c.xa) and x2[..., :cin].any()
    ref = exact.conv_ref64(spec, x2[..., cin:], c.w, c.b)
    exact.assert_identical(y, exact.rne_bf16(torch.where(ref > 0, ref, ref * 0.25)), "oracle forward out of a slice vs float64")
    want = torch.stack([ref.reshape(N, -1, spec.cout).sum(1), (ref * ref).reshape(N, -1, spec.cout).sum(1)], 1)
    exact.assert_identical(stats, want, "oracle statistics partials (sum, sum of squares) vs float64")
    gx = exact.dgrad_ref64(spec, c.sizes, c.gy, c.w)
    assert base[..., cin:].any() and base[..., :cin].any() and gx.any(), "both halves of the base and the gradient must be live"
    wantG = base.clone()
    wantG[..., cin:] = exact.rne_bf16(gx + base[..., cin:].double())
    exact.assert_identical(G, wantG, "oracle data gradient accumulated into a slice vs float64 + base, other half untouched")


def test_oracle_is_exact_on_the_strip_walk_case():
    """forward with statistics and data gradient of WALK_STRIP_CASE (the folded conv itself, as for CONV_CASES)"""
    spec, N, sizes = WALK_STRIP_CASE[0], WALK_STRIP_CASE[1], WALK_STRIP_CASE[2:]
    c = exact.make_case(spec, N, sizes, seed=WALK_SEED, check=("fwd", "dgrad"))
    y, stats = oracle_forward(c)
    ref = exact.conv_ref64(spec, c.xa, c.w, c.b)
    exact.assert_identical(y, padded(ref, spec.cout_p, torch.bfloat16), "oracle forward vs float64")
    co = exact.cout_of(spec)
    want = torch.zeros(N, 2, spec.cout_p, dtype=torch.float64)
    want[:, 0, :co] = ref.reshape(N, -1, co).sum(1)
    want[:, 1, :co] = (ref * ref).reshape(N, -1, co).sum(1)
    exact.assert_identical(stats, want, "oracle statistics partials (sum, sum of squares) vs float64")
    gx = exact.dgrad_ref64(spec, sizes, c.gy, c.w)
    exact.assert_identical(oracle_dgrad(c), padded(gx, spec.cin_p, torch.bfloat16), "oracle data gradient vs float64")


# ---- sensitivity: what the exact comparison sees ----------------------------------------------------------------------------
def _faults(spec, xa, w, b):
    """the trunk layer's float64 output with (a) one (tap, channel) product at one pixel replaced by its neighbour channel's,
    (b) one reflect-border index shifted by one at the image corner (pixel (0, 0), tap (0, 0) reads row 0 instead of row 1)"""
    x = xa[..., :spec.cin].double()
    ref = exact.conv_ref64(spec, xa, w, b)
    n, i, j, co, ci = 1, 7, 9, 33, 100
    a = ref.clone()         # tap (1, 1) is the pixel itself
    a[n, i, j, co] += float(w[co, ci, 1, 1]) * float(x[n, i, j, ci + 1] - x[n, i, j, ci])
    bb = ref.clone()        # output (0, 0), tap (0, 0): reflect reads x[1, 1]; the faulty table reads x[0, 1]
    bb[0, 0, 0] += (w[:, :, 0, 0].double() * (x[0, 0, 1] - x[0, 1, 1])[None, :]).sum(1)
    return ref, a, bb


def test_exact_comparison_notices_single_element_faults():
    spec, N, sizes = TRUNK[0], TRUNK[1], TRUNK[2:]
    for seed in range(20):
        c = exact.make_case(spec, N, sizes, seed=100 + seed, check=("fwd",))
        x, w = c.xa.clone(), c.w.clone()
        # a fault that changes nothing (equal neighbours, dead weight) is no fault: make the operands it touches live
        x[1, 7, 9, 100], x[1, 7, 9, 101], w[33, 100, 1, 1] = 1.0, -2.0, 1.0
        x[0, 0, 1, 5], x[0, 1, 1, 5], w[:, 5, 0, 0] = 2.0, -1.0, 1.0
        exact.assert_exact_domain(spec, x=x, w=w, bias=c.b)
        ref, a, bb = _faults(spec, x, w, c.b)
        good = exact.rne_bf16(ref)
        assert exact.first_mismatch(exact.rne_bf16(a), good) is not None, f"seed {seed}: wrong product not noticed"
        assert exact.first_mismatch(exact.rne_bf16(bb), good) is not None, f"seed {seed}: wrong border index not noticed"
        with pytest.raises(AssertionError, match="first at"):
            exact.assert_identical(exact.rne_bf16(a), good, "forward", decompose=(spec, x, w, c.b))


def test_exact_comparison_notices_truncation_instead_of_rounding():
    spec, N, sizes = TRUNK[0], TRUNK[1], TRUNK[2:]
    for seed in range(20):
        c = exact.make_case(spec, N, sizes, seed=100 + seed, rounding=True, check=("fwd",))
        ref = exact.conv_ref64(spec, c.xa, c.w, c.b).float()
        trunc = (ref.view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)       # drops the low 16 bits
        assert exact.first_mismatch(trunc, ref.to(torch.bfloat16)) is not None, f"seed {seed}: truncation not noticed"


def randn_tolerance_detection_share(seeds=20):
    """the randn twin of faults (a) and (b) under test_ops_gpu.close_bf16: over `seeds` seeds, how often the tolerance
    comparison notices each. A measurement (DESIGN.md §7 quotes it: python -c "from tests.test_exact_cpu import *;
    print(randn_tolerance_detection_share())"), not a test."""
    spec, N, sizes = TRUNK[0], TRUNK[1], TRUNK[2:]
    seen = {"product": 0, "border": 0}
    for seed in range(seeds):
        low, master, bias, fpack, dpack = make_layer(spec, sizes, 200 + seed)
        w = spec.torch_from_master(master).to(torch.bfloat16).float()
        xa = torch.randn(N, *sizes, spec.cin_p, generator=torch.Generator().manual_seed(300 + seed)).to(torch.bfloat16)
        ref, a, bb = _faults(spec, xa, w, bias)
        for name, bad in (("product", a), ("border", bb)):
            try:
                close_bf16(bad.to(torch.bfloat16), ref.to(torch.bfloat16), name)
            except AssertionError:
                seen[name] += 1
    return {k: v / seeds for k, v in seen.items()}
