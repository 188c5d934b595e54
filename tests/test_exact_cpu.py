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
from tests.test_ops_gpu import CONV_CASES, _ids, close_bf16, make_layer

pytestmark = []          # (test_ops_gpu's module-level gpu mark does not travel with its names)

TRUNK = (ConvSpec("conv", 256, 256, 3, 1, 1, pad_mode="reflect"), 2, 16, 16)
ROUNDING_CASES = [
    TRUNK,                                                                                 # trunk
    (ConvSpec("conv", 64, 128, 3, 2, 1), 2, 32, 32),                                       # stride 2
    (ConvSpec("convT", 256, 128, 3, 2, 1, 1), 2, 16, 16),                                  # transposed
    (ConvSpec("conv", 256, 256, 3, 1, 1, pad_mode="replicate", dims=3), 1, 8, 8, 8),      # 3-D
]


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
