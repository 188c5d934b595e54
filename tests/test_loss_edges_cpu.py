"""The yardstick of tests/test_loss_edges_gpu.py, pinned on the CPU.

tests/loss_ref.py states every operation of csrc/loss.hip in float64, from the mathematics. This module shows that those
statements are the oracle's operation (RefOps, oracle/torch_ref.adversarial_loss) and the reference's (the recorded vectors
of tests/golden/adv_modes.json), at the shapes the GPU module uses and to what fp32 torch earns against float64; asserts,
from the float64 statements alone, the conditions the GPU tests rely on (the integer-domain cases sum exactly, no random
SSIM case comes near the kink of sqrt(relu(.)), the constant-image case is the closed form); and measures, per case, the
error of RefOps (fp32 torch on the CPU) against float64 — the yardstick the GPU module holds the device's SSIM and
transcendental results to. The case lists and input builders live in tests/loss_ref.py.
"""
import functools
import json
import math
from pathlib import Path

import pytest
import torch

from oracle import torch_ref
from oracle.ops_ref import RefOps
from tests import loss_ref as R

GOLD = json.loads((Path(__file__).parent / "golden" / "adv_modes.json").read_text())["ops"]
U = 2.0 ** -24                # unit roundoff of fp32


# ---- RefOps through the kernels' interface ----------------------------------------------------------------------------
def refops_reduction(op, a, b=None, grad_scale=None):
    """(loss, gradient) of one reduction op by RefOps, fp32"""
    ops, loss, grad = RefOps(), torch.zeros(()), torch.empty_like(a)
    if op == "l1":
        ops.l1(a, b, loss=loss)
        ops.l1(a, b, grad_a=grad, grad_scale=grad_scale)
    elif op in ("mse0", "mse1"):
        ops.mse_const(a, R.op_target(op), loss=loss, grad=grad, grad_scale=grad_scale)
    elif op == "mean":
        ops.mean(a, loss)
        grad = None
    else:
        mode, side = op.split("_")
        ops.adv_loss(a, mode, side == "real", R.op_target(op) or 0.0, loss=loss, grad=grad, grad_scale=grad_scale)
    return loss, grad


# ---- the measured yardsticks (imported by the GPU module) ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def transcendental_case(mode, real, n):
    """vanilla on logits(n): inputs, float64 loss and gradient, and RefOps's error against them: the loss in ulp of the
    reference loss, the gradient as the largest elementwise error in ulp of the reference element (`cpu_grad_ulp`) and in
    ulp of the factor 1 / n every element carries (`cpu_grad_abs`: sigmoid(x) - t cancels for large logits, where an ulp of
    the tiny reference element says little)"""
    x = R.logits(n).reshape(n, 1)
    loss64, grad64 = R.adv(x, mode, real)
    loss, grad = torch.zeros(()), torch.empty_like(x)
    RefOps().adv_loss(x, mode, real, 1.0 if real else 0.0, loss=loss, grad=grad)
    unit = R.ulp32(torch.tensor(1.0 / n))
    return dict(x=x, loss64=loss64, grad64=grad64, unit=unit,
                cpu_loss_ulp=float(R.err_ulp32(loss, loss64)),
                cpu_grad_ulp=float(R.err_ulp32(grad, grad64).max()),
                cpu_grad_abs=float(((grad.double() - grad64).abs() / unit).max()))


@functools.lru_cache(maxsize=None)
def nonsat_case(real, rows, per):
    """nonsaturating on row_logits(rows, per) with the per-row upstream gradients row_scales(rows): as transcendental_case,
    the loss error as the largest over the rows"""
    x, s = R.row_logits(rows, per), R.row_scales(rows)
    loss64, grad64 = R.adv(x, "nonsaturating", real)
    grad64 = grad64 * s.double()[:, None]
    loss, grad = torch.zeros(rows), torch.empty_like(x)
    RefOps().adv_loss(x, "nonsaturating", real, 0.0, loss=loss, grad=grad, grad_scale=s)
    unit = R.ulp32(s.double() / per)[:, None]
    return dict(x=x, scales=s, loss64=loss64, grad64=grad64, unit=unit,
                cpu_loss_ulp=float(R.err_ulp32(loss, loss64).max()),
                cpu_grad_ulp=float(R.err_ulp32(grad, grad64).max()),
                cpu_grad_abs=float(((grad.double() - grad64).abs() / unit).max()))


def _largest(cases):
    return {k: max(c[k] for c in cases) for k in ("cpu_loss_ulp", "cpu_grad_ulp", "cpu_grad_abs")}


@functools.lru_cache(maxsize=None)
def vanilla_yardstick(real):
    """RefOps's LARGEST error against float64 over the vanilla cases of one label (every n of TRANSCENDENTAL_LENGTHS): the
    loss of one case is a single number whose fp32 error is anywhere in [0, its bound) by the luck of the last rounding
    (0.03 ulp at n = 1, 2.1 ulp at n = 2049), so the yardstick of an implementation is the largest it shows on the inputs"""
    return _largest([transcendental_case("vanilla", real, n) for n in R.TRANSCENDENTAL_LENGTHS])


@functools.lru_cache(maxsize=None)
def nonsat_yardstick(real):
    """as vanilla_yardstick, over every rows x per case of one sign"""
    return _largest([nonsat_case(real, rows, per) for rows in R.NONSAT_ROWS for per in R.NONSAT_PER])


SSIM_SCALE = 1.7


def _ssim_case(x, y, scaled):
    s = torch.tensor(SSIM_SCALE) if scaled else None
    k = float(s.double()) if scaled else 1.0
    ops, val = RefOps(), torch.zeros(())
    gy, gx = torch.empty_like(y), torch.empty_like(x)
    ops.ssim_distance(x, y, val)
    ops.ssim_distance_backward(x, y, gy, grad_scale=s)
    ops.ssim_distance_backward(y, x, gx, grad_scale=s)
    val64, gy64, gx64 = R.ssim_distance(x, y), R.ssim_grad_y(x, y) * k, R.ssim_grad_y(y, x) * k
    return dict(x=x, y=y, scale=s, val64=val64, gy64=gy64, gx64=gx64,
                cpu_val=float((val.double() - val64).abs() / val64.abs()),
                cpu_gy=R.per_plane_rel_err(gy, gy64), cpu_gx=R.per_plane_rel_err(gx, gx64))


@functools.lru_cache(maxsize=None)
def ssim_case(shape, scaled=False):
    """random SSIM case: inputs, float64 value and gradients (d/dy, d/dx), and RefOps's error against them: the value
    relative, the gradients as the largest absolute error over the largest absolute reference value per plane"""
    return _ssim_case(*R.ssim_inputs(shape), scaled)


@functools.lru_cache(maxsize=None)
def ssim_constant_case(a, b):
    return _ssim_case(*R.ssim_constant_inputs(a, b), False)


# ---- loss_ref is the oracle's operation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.REDUCTION_LENGTHS)
def test_reductions_are_the_oracles(n):
    """RefOps (fp32 torch) against the float64 statements on the dense data of the GPU module. torch sums fp32 in a cascade:
    serial runs of a few elements per vector lane under a pairwise tree, so an element passes at most log2(n) + 16 adds;
    with the t roundings of a term and the division by n that is (log2(n) + 16 + t) * 2^-24 * mean|term| + 2^-23 |ref|.
    Gradients: one rounding each for the difference, the scaling and the division, 2 ulp of the reference element."""
    for op in R.REDUCTION_OPS:
        a, b = R.dense_case(op, n)
        loss, grad = refops_reduction(op, a, b)
        loss64, grad64 = R.reference(op, a, b)
        depth = math.ceil(math.log2(n)) + 16 + R.TERM_ROUNDINGS[op] if n > 1 else 4
        bound = depth * U * float(R.terms64(op, a, b).abs().mean()) + 2 * U * abs(float(loss64))
        assert abs(float(loss.double() - loss64)) <= bound, (op, n, float(loss), float(loss64), bound)
        if grad is not None:
            a, b = R.dense_case(op, n, grid=True)           # exact differences: the roundings left are those counted
            _, grad = refops_reduction(op, a, b)
            assert float(R.err_ulp32(grad, R.reference(op, a, b)[1]).max()) <= 2.0, (op, n)


@pytest.mark.parametrize("mode", ["lsgan", "vanilla", "wgangp"])
@pytest.mark.parametrize("real", [True, False])
def test_objectives_are_the_references(mode, real):
    """the float64 statement against the REAL reference's vectors (fp32, 7200 logits: 1e-6 is what the existing oracle test
    holds the fp32 oracle to) and against oracle/torch_ref.adversarial_loss"""
    g = GOLD[f"{mode}_{'real' if real else 'fake'}"]
    x = torch.randn(8, 1, 30, 30, generator=torch.Generator().manual_seed(21)) * 3.0
    loss64, grad64 = R.adv(x, mode, real)
    assert float(loss64) == pytest.approx(g["loss"], rel=1e-6, abs=1e-7)
    assert float(grad64.norm()) == pytest.approx(g["grad_norm"], rel=1e-6)
    assert torch.allclose(grad64.flatten()[g["idx"]], torch.tensor(g["grad_samples"], dtype=torch.float64), rtol=1e-5,
                          atol=1e-9)
    xr = x.clone().requires_grad_()
    val = torch_ref.adversarial_loss(xr, real, mode)
    (gx,) = torch.autograd.grad(val, xr)
    assert float(val.detach()) == pytest.approx(float(loss64), rel=1e-6, abs=1e-7)
    assert torch.allclose(gx.double(), grad64, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("mode", ["vanilla", "nonsaturating"])
@pytest.mark.parametrize("real", [True, False])
def test_transcendental_objectives_are_the_oracles(mode, real):
    """RefOps on the special logits: where sigmoid(x) - t does not cancel the fp32 result is within a few ulp of float64;
    everywhere it is within a few ulp of the factor 1 / n (the measured values are the GPU module's yardstick)"""
    cases = ([transcendental_case(mode, real, n) for n in R.TRANSCENDENTAL_LENGTHS] if mode == "vanilla" else
             [nonsat_case(real, rows, per) for rows in R.NONSAT_ROWS for per in R.NONSAT_PER])
    for c in cases:
        assert c["cpu_loss_ulp"] <= 16.0, c["cpu_loss_ulp"]
        assert c["cpu_grad_abs"] <= 4.0, c["cpu_grad_abs"]
        assert math.isfinite(c["cpu_grad_ulp"])


@pytest.mark.parametrize("shape", R.SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_is_the_oracles(shape):
    """RefOps's SSIM distance and both gradients against float64. The fp32 evaluation loses 1 / (2 sqrt(S)) and the
    cancellation of the variances (of order 2^-24 / C2 = 7e-5 of S2) on top of its roundings: 1e-3 of the plane's largest
    gradient, 1e-4 of the value. The exact figures are the GPU module's yardstick."""
    for scaled in (False, True):
        c = ssim_case(shape, scaled)
        assert c["cpu_val"] <= 1e-4, c["cpu_val"]
        assert float(c["cpu_gy"].max()) <= 1e-3 and float(c["cpu_gx"].max()) <= 1e-3, (c["cpu_gy"], c["cpu_gx"])


# ---- the conditions the GPU tests rely on, from float64 alone -------------------------------------------------------------
@pytest.mark.parametrize("n", R.REDUCTION_LENGTHS)
def test_integer_domain(n):
    """every term of a sparse case is an integer and the magnitudes of all terms sum to less than 2^24: every partial sum,
    in any order, is an exactly representable integer. n itself is below 2^24, so (float)n is exact."""
    assert n < 2 ** 24
    for op in R.REDUCTION_OPS:
        a, b = R.sparse_case(op, n)
        t = R.terms64(op, a, b)
        assert torch.equal(t, t.round()), op
        assert float(t.abs().sum()) < 2 ** 24, op
        marked = R.marked_positions(n)
        assert int((t != 0).sum()) == len(marked) and {0, n - 1} <= set(marked), (op, n)
        assert len(set(t.abs()[marked].tolist())) == len(marked), "marked positions carry distinct terms"


@pytest.mark.parametrize("shape", R.SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_ssim_cases_stay_away_from_the_kink(shape):
    x, y = R.ssim_inputs(shape)
    assert float(R.ssim_s_map(x, y).min()) >= R.SSIM_MIN_S


@pytest.mark.parametrize("pair", R.SSIM_CONSTANT_PAIRS)
def test_constant_images_are_the_closed_form(pair):
    """float64 leaves 2^-53 of the squared means in the variances, 1e-13 of C2 and so of S2: 1e-11 of S, which is not small"""
    x, y = R.ssim_constant_inputs(*pair)
    S = R.ssim_s_map(x, y)
    want = R.ssim_constant_closed_form(*pair)
    assert want >= R.SSIM_MIN_S
    assert float((S - want).abs().max()) <= 1e-11 * want
    assert float(R.ssim_distance(x, y)) == pytest.approx(math.sqrt(want), rel=1e-11)


def test_identical_images_have_no_distance():
    """the reference's own arithmetic: S1 = S2 = 1 bit for bit, S = 0, and relu passes no gradient (ssim.py:85-98)"""
    x, _ = R.ssim_inputs((1, 3, 27, 75))
    val, g = torch.zeros(()), torch.full_like(x, float("nan"))
    RefOps().ssim_distance(x, x.clone(), val)
    RefOps().ssim_distance_backward(x, x.clone(), g)
    assert float(val) == 0.0 and not g.any()
    assert float(R.ssim_distance(x, x.clone())) == 0.0 and not R.ssim_grad_y(x, x.clone()).any()


def test_scalar_affine_statement():
    vals, rows, consts = R.scalar_affine_case()
    xs = [None if v is None else torch.tensor(v) for v in vals]
    want, big = R.scalar_affine(vals, rows, consts)
    got = RefOps().scalar_affine(xs, rows, consts)
    assert ((got.double() - want).abs() <= 2 * len(vals) * U * big).all()
