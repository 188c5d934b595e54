"""csrc/loss.hip against the float64 statements of tests/loss_ref.py, at the edges of its launch geometry.

Every tolerance here is an equality, a bound computed in the test from n and the kernel's summation shape, or a multiple
of the error RefOps (fp32 torch on the CPU) measures against float64 on the same inputs
(tests/test_loss_edges_cpu.py, which also asserts the conditions on the inputs from float64 alone). None is taken from the
device's output. Output buffers hold NaN before every call: a slot the kernel leaves unwritten stays NaN.
"""
import math

import pytest
import torch

from ganslate_amd.hip import lib as L
from ganslate_amd.hip.ops import _ptr, _stream
from tests import loss_ref as R
from tests.test_loss_edges_cpu import (nonsat_case, nonsat_yardstick, ssim_case, ssim_constant_case, transcendental_case,
                                       vanilla_yardstick)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
_ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def nan_scalar(dev):
    return torch.full((), NAN, device=dev)


def hip_loss(ops, op, a, b=None, out=None):
    """one reduction op of loss.hip on device tensors -> the NaN-prefilled device scalar it wrote (no synchronisation)"""
    out = nan_scalar(a.device) if out is None else out
    if op == "l1":
        ops.l1(a, b, loss=out)
    elif op in ("mse0", "mse1"):
        ops.mse_const(a, R.op_target(op), loss=out)
    elif op == "mean":
        ops.mean(a, out)
    else:
        mode, side = op.split("_")
        ops.adv_loss(a, mode, side == "real", R.op_target(op) or 0.0, loss=out)
    return out


def hip_grad(ops, op, a, b=None, grad_scale=None):
    grad = torch.full_like(a, NAN)
    if op == "l1":
        ops.l1(a, b, grad_a=grad, grad_scale=grad_scale)
    elif op in ("mse0", "mse1"):
        ops.mse_const(a, R.op_target(op), grad=grad, grad_scale=grad_scale)
    else:
        mode, side = op.split("_")
        ops.adv_loss(a, mode, side == "real", R.op_target(op) or 0.0, grad=grad, grad_scale=grad_scale)
    return grad


def dev_pair(a, b, dev):
    return a.to(dev), (b.to(dev) if b is not None else None)


# ---- reductions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.REDUCTION_LENGTHS)
def test_reduction_sparse_integers(hip_ops, n):
    """Integer domain: the neutral value everywhere and a distinct small integer at each marked position (both ends, the
    wavefront, workgroup and 8-per-thread edges, the first wrap of the grid-stride loop, ~50 random ones), so the fp32 sum
    is exact in any order and the only roundings are 1.0f / (float)n ((float)n is exact below 2^24) and the double product
    rounded to float: |got - ref64| <= 2^-23 |ref64|. The data is sparse because with dense data of these sizes one
    element is below that bound (1 / n of the sum against 2^-23): here one dropped or doubled position moves the sum of
    ~60 small integers by at least one part in a few thousand."""
    dev = hip_ops.device
    for op in R.REDUCTION_OPS:
        a, b = R.sparse_case(op, n)
        ref = float(R.reference(op, a, b)[0])
        got = float(hip_loss(hip_ops, op, *dev_pair(a, b, dev)))
        assert not math.isnan(got), f"{op} n={n}: loss not written"
        assert abs(got - ref) <= 2 * U * abs(ref), f"{op} n={n}: {got!r} vs {ref!r}"


@pytest.mark.parametrize("n", R.REDUCTION_LENGTHS)
def test_reduction_dense(hip_ops, n):
    """Dense random fp32 data against float64. An element passes k = ceil(n / (G * 256)) serial adds in its thread, 6
    shuffle levels in its wavefront, 4 serial adds in its workgroup (k + 10 roundings of at most 2^-24 of a partial sum
    each; 2 more cover their second order), then double; forming the term rounds t times (1 mean, 2 l1, 2 squared
    differences). So |got - ref64| <= (k + 12 + t) * 2^-24 * mean|term| + 2^-23 |ref64| (the scaling by 1.0f / n)."""
    dev = hip_ops.device
    for op in R.REDUCTION_OPS:
        a, b = R.dense_case(op, n)
        ref = float(R.reference(op, a, b)[0])
        bound = dense_bound(op, n, a, b, ref)
        got = float(hip_loss(hip_ops, op, *dev_pair(a, b, dev)))
        assert not math.isnan(got), f"{op} n={n}: loss not written"
        assert abs(got - ref) <= bound, f"{op} n={n}: {got!r} vs {ref!r}, bound {bound:.3e}"


@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "grad_scale"])
@pytest.mark.parametrize("n", R.REDUCTION_LENGTHS)
def test_reduction_gradients(hip_ops, n, scaled):
    """Every gradient element within 2 ulp of the float64 value rounded to fp32: the factor (grad_scale * c / n) is formed
    with at most two roundings and applied with one multiply; the data lies on a grid where the differences a - b and
    x - target are exact. L1: every element is 0 or +-k for ONE k, k within 2 ulp of grad_scale / n, the sign that of
    a - b in float64 (a == b gives 0)."""
    dev = hip_ops.device
    s = torch.tensor(2.5) if scaled else None
    for op in R.GRAD_OPS:
        a, b = R.dense_case(op, n, grid=True)
        ref = R.reference(op, a, b)[1] * (2.5 if scaled else 1.0)
        got = hip_grad(hip_ops, op, *dev_pair(a, b, dev), grad_scale=s.to(dev) if scaled else None).cpu()
        assert not torch.isnan(got).any(), f"{op} n={n}: gradient elements not written"
        worst = float(R.err_ulp32(got, ref).max())
        assert worst <= 2.0, f"{op} n={n}: {worst} ulp"
        if op == "l1":
            mags = got[got != 0].abs().unique()
            assert mags.numel() <= 1, f"l1 n={n}: magnitudes {mags}"
            assert torch.equal(torch.sign(got).double(), torch.sign(ref)), f"l1 n={n}: signs"


def test_l1_gradient_of_a_subnormal_difference(hip_ops):
    """a - b = +-1e-40 is a subnormal: its sign must survive (torch.sign(a - b) on the CPU keeps it), +-k exactly"""
    dev = hip_ops.device
    a = torch.tensor([1e-40, 0.0, 1e-40, 0.0, -1e-40, 1.0, 1.0 + 2.0 ** -23], dtype=torch.float32)
    b = torch.tensor([0.0, 1e-40, 1e-40, 0.0, 0.0, 1.0 + 2.0 ** -23, 1.0], dtype=torch.float32)
    assert float(a[0]) > 0.0, "the host keeps subnormals"
    want = torch.tensor([1.0, -1.0, 0.0, 0.0, -1.0, -1.0, 1.0], dtype=torch.float64)
    for scale in (None, 3.0):
        got = hip_grad(hip_ops, "l1", a.to(dev), b.to(dev),
                       grad_scale=torch.tensor(scale, device=dev) if scale else None).cpu()
        k = torch.tensor(scale or 1.0) / torch.tensor(7.0)                     # fp32 division, correctly rounded
        assert torch.equal(got.double(), want * k.double()), (got, k)


# ---- vanilla / nonsaturating ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.TRANSCENDENTAL_LENGTHS)
@pytest.mark.parametrize("real", [True, False], ids=["real", "fake"])
def test_vanilla_at_the_special_logits(hip_ops, real, n):
    """BCE-with-logits on +-0, +-1e-8, +-19.999, +-20 and its neighbours, +-30, +-88, +-104, +-1e4 and randn * 6 (both labels,
    both signs of every logit). Tolerance: twice RefOps's LARGEST error against float64 over the cases of this label (all
    four n; tests/test_loss_edges_cpu.vanilla_yardstick), in ulp of the reference value — the device's expf / log1pf and torch's vectorised ones are different implementations of the same
    fp32 functions. The gradient is held to that elementwise in ulp of the reference element, and (sigmoid(x) - 1 cancels
    for large logits, where both fp32 results are 0 and the ulp of the tiny reference says little) to twice RefOps's
    largest error in ulp of the factor 1 / n.
    Measured (CPU RefOps): loss up to 2.5 ulp, gradient up to 1.9 ulp for label 0 and 1.7e7 ulp (the cancellation) for label
    1, 1.9 ulp of 1 / n. The device's figures are printed by the test."""
    c = transcendental_case("vanilla", real, n)
    dev = hip_ops.device
    x = c["x"].to(dev)
    loss, grad = nan_scalar(dev), torch.full_like(x, NAN)
    hip_ops.adv_loss(x, "vanilla", real, 1.0 if real else 0.0, loss=loss, grad=grad)
    assert not math.isnan(float(loss)) and not torch.isnan(grad).any(), "output not written"
    dev_loss = float(R.err_ulp32(loss, c["loss64"]))
    dev_grad = float(R.err_ulp32(grad, c["grad64"]).max())
    dev_abs = float(((grad.cpu().double() - c["grad64"]).abs() / c["unit"]).max())
    print(f"vanilla real={real} n={n}: loss ulp cpu {c['cpu_loss_ulp']:.3f} device {dev_loss:.3f}; grad ulp cpu "
          f"{c['cpu_grad_ulp']:.3f} device {dev_grad:.3f}; grad / ulp(1/n) cpu {c['cpu_grad_abs']:.3f} device {dev_abs:.3f}")
    y = vanilla_yardstick(real)
    assert dev_loss <= 2 * y["cpu_loss_ulp"], (dev_loss, y)
    assert dev_grad <= 2 * y["cpu_grad_ulp"], (dev_grad, y)
    assert dev_abs <= 2 * y["cpu_grad_abs"], (dev_abs, y)


@pytest.mark.parametrize("per", R.NONSAT_PER)
@pytest.mark.parametrize("rows", R.NONSAT_ROWS)
@pytest.mark.parametrize("real", [True, False], ids=["real", "fake"])
def test_nonsaturating_rows(hip_ops, real, rows, per):
    """soft-plus per sample on the special logits (the z > 20 branch on both sides of 20), one workgroup per row, with a
    distinct upstream gradient per row: the gradient of row r must carry grad_scale[r]. Tolerances as for vanilla (twice
    RefOps's largest error over all rows x per cases of this sign, nonsat_yardstick); the loss as the largest error over
    the rows.
    Measured (CPU RefOps): loss up to 5.6 ulp, gradient up to 3.0 ulp, 1.9 ulp of grad_scale[r] / per."""
    c = nonsat_case(real, rows, per)
    dev = hip_ops.device
    x = c["x"].to(dev)
    loss, grad = torch.full((rows,), NAN, device=dev), torch.full_like(x, NAN)
    hip_ops.adv_loss(x, "nonsaturating", real, 0.0, loss=loss)
    hip_ops.adv_loss(x, "nonsaturating", real, 0.0, grad=grad, grad_scale=c["scales"].to(dev))
    assert not torch.isnan(loss).any() and not torch.isnan(grad).any(), "output not written"
    dev_loss = float(R.err_ulp32(loss, c["loss64"]).max())
    dev_grad = float(R.err_ulp32(grad, c["grad64"]).max())
    dev_abs = float(((grad.cpu().double() - c["grad64"]).abs() / c["unit"]).max())
    print(f"nonsaturating real={real} rows={rows} per={per}: loss ulp cpu {c['cpu_loss_ulp']:.3f} device {dev_loss:.3f}; "
          f"grad ulp cpu {c['cpu_grad_ulp']:.3f} device {dev_grad:.3f}; grad / ulp(scale/per) cpu {c['cpu_grad_abs']:.3f} "
          f"device {dev_abs:.3f}")
    y = nonsat_yardstick(real)
    assert dev_loss <= 2 * y["cpu_loss_ulp"], (dev_loss, y)
    assert dev_grad <= 2 * y["cpu_grad_ulp"], (dev_grad, y)
    assert dev_abs <= 2 * y["cpu_grad_abs"], (dev_abs, y)


# ---- the workspace ---------------------------------------------------------------------------------------------------
def dense_bound(op, n, a, b, ref):
    """the bound of test_reduction_dense"""
    return (R.serial_adds(n) + 12 + R.TERM_ROUNDINGS[op]) * U * float(R.terms64(op, a, b).abs().mean()) + 2 * U * abs(ref)


def test_workspace_after_a_larger_launch(hip_ops):
    """One stream, no synchronisation between the launches: a 1024-workgroup mean, a 1-workgroup mean of another value, a
    3-workgroup L1, a 2-workgroup MSE. The last-arriving workgroup must sum gridDim.x partials, not the stale ones of the
    larger launch before it, and find the arrival counter reset: each result is bit-equal to the same call made alone
    (the calls alone run in the opposite order, so each has another predecessor) and within the bound of
    test_reduction_dense of float64 (a stale partial of the large launch is a sum of 2048 elements)."""
    dev = hip_ops.device
    calls = [("mean", 2 ** 21 + 1), ("mean", 1), ("l1", 4097), ("mse1", 2049)]
    host = []
    for i, (op, n) in enumerate(calls):
        a, b = R.dense_case(op, n)
        host.append((a + float(i), b))                                   # (the n = 1 mean sees another value)
    data = [dev_pair(a, b, dev) for a, b in host]
    alone = [None] * len(calls)
    for i in reversed(range(len(calls))):
        alone[i] = float(hip_loss(hip_ops, calls[i][0], *data[i]))
        torch.cuda.synchronize()
    outs = [hip_loss(hip_ops, op, a, b) for (op, n), (a, b) in zip(calls, data)]
    torch.cuda.synchronize()
    for (op, n), (a, b), o, want in zip(calls, host, outs, alone):
        ref = float(R.reference(op, a, b)[0])
        assert abs(float(o) - ref) <= dense_bound(op, n, a, b, ref), f"{op} n={n} in sequence {float(o)!r} vs {ref!r}"
        assert float(o) == want, f"{op} n={n} in sequence {float(o)!r}, alone {want!r}"


def test_reductions_on_two_streams(hip_ops):
    """csrc/api.hip keeps one workspace per launching stream, because the discriminator pass runs beside the generators'
    backward: 8 interleaved rounds of a 3 * 2^21 + 77 L1 on one stream and a 2^21 + 262147 MSE on another, one
    synchronize, every result bit-equal to the same call alone on the default stream."""
    dev = hip_ops.device
    n1, n2 = 3 * 2 ** 21 + 77, 2 ** 21 + 262_147
    a, b = dev_pair(*R.dense_case("l1", n1), dev)
    x, _ = dev_pair(*R.dense_case("mse1", n2), dev)
    want1 = float(hip_loss(hip_ops, "l1", a, b))
    want2 = float(hip_loss(hip_ops, "mse1", x))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    o1 = [nan_scalar(dev) for _ in range(8)]
    o2 = [nan_scalar(dev) for _ in range(8)]
    torch.cuda.synchronize()                                                # the NaN fills ran on the default stream
    for r in range(8):
        with torch.cuda.stream(s1):
            hip_loss(hip_ops, "l1", a, b, out=o1[r])
        with torch.cuda.stream(s2):
            hip_loss(hip_ops, "mse1", x, out=o2[r])
    torch.cuda.synchronize()
    assert [float(o) for o in o1] == [want1] * 8
    assert [float(o) for o in o2] == [want2] * 8


# ---- SSIM distance -----------------------------------------------------------------------------------------------------
SSIM_FLOOR = 4 * 2.0 ** -23        # a few fp32 ulp of the reference value, where RefOps's own error is near zero


def hip_ssim(ops, x, y, scale=None):
    """-> (value, d/dy, d/dx) of the device, NaN-prefilled outputs checked for full overwrite"""
    dev = ops.device
    xd, yd = x.to(dev), y.to(dev)
    val, gy, gx = nan_scalar(dev), torch.full_like(yd, NAN), torch.full_like(xd, NAN)
    s = scale.to(dev) if scale is not None else None
    ops.ssim_distance(xd, yd, val)
    ops.ssim_distance_backward(xd, yd, gy, grad_scale=s)
    ops.ssim_distance_backward(yd, xd, gx, grad_scale=s)                     # the distance is symmetric: d/dx
    assert not math.isnan(float(val)), "distance not written"
    assert not torch.isnan(gy).any() and not torch.isnan(gx).any(), "gradient elements not written"
    return val.cpu(), gy.cpu(), gx.cpu()


@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "grad_scale"])
@pytest.mark.parametrize("shape", R.SSIM_SHAPES, ids=_ids)
def test_ssim_at_the_tile_edges(hip_ops, shape, scaled):
    """Forward value and both gradients against float64 at: one output pixel (11x11); one row of output (11x43); a valid map
    of exactly one 16x32 tile whose backward needs 2x2 tiles (26x42); 2x3 forward tiles with one-pixel ragged edges over
    three planes (27x75); 5-D input (N*C*D planes); 64x64. min S >= 1e-3 on every case (asserted on the CPU).
    Tolerance: the device's error is at most 4 times RefOps's error against float64 on the same case — both are fp32
    evaluations of one formula and differ in summation order and contraction — with a floor of 4 fp32 ulp; the value
    relative, the gradients as the largest absolute error over the largest absolute reference value PER PLANE (a wrong
    plane decode in a small plane hides in a whole-tensor norm) and over the whole tensor.
    Measured (CPU RefOps): value 0.9e-7 .. 1.8e-7, gradient per plane 2.3e-7 .. 1.3e-6 (d/dy), up to 2.0e-6 (d/dx). The
    device's figures are printed by the test."""
    c = ssim_case(shape, scaled)
    val, gy, gx = hip_ssim(hip_ops, c["x"], c["y"], c["scale"])
    dev_val = float((val.double() - c["val64"]).abs() / c["val64"].abs())
    print(f"ssim {shape} scaled={scaled}: value cpu {c['cpu_val']:.3e} device {dev_val:.3e}")
    assert dev_val <= max(4 * c["cpu_val"], SSIM_FLOOR)
    for what, got, ref, cpu in (("d/dy", gy, c["gy64"], c["cpu_gy"]), ("d/dx", gx, c["gx64"], c["cpu_gx"])):
        err = R.per_plane_rel_err(got, ref)
        print(f"  {what} per plane: cpu {[f'{v:.2e}' for v in cpu.tolist()]} device {[f'{v:.2e}' for v in err.tolist()]}")
        assert (err <= torch.clamp_min(4 * cpu, SSIM_FLOOR)).all(), f"{what} per plane: device {err}, cpu {cpu}"
        whole = float((got.double() - ref).abs().max() / ref.abs().max())
        cpu_whole = float(cpu.max())            # (a plane's largest reference value is at most the tensor's)
        assert whole <= max(4 * cpu_whole, SSIM_FLOOR), f"{what} whole tensor: device {whole}, cpu {cpu_whole}"


@pytest.mark.parametrize("shape", R.SSIM_IDENTICAL_SHAPES, ids=_ids)
def test_ssim_of_identical_images_is_exactly_zero(hip_ops, shape):
    """y = x.clone(): in the reference's arithmetic 2 mu1 mu2 and mu1^2 + mu2^2 are the same doubling of one rounded product
    and 2 s12 equals s1 + s2 bit for bit, so S1 = S2 = 1, S = 0, the distance is 0.0 and relu passes no gradient
    (ssim.py:85-98; asserted for the oracle on the CPU). A kernel that contracts 2 m1 m2 + C1 into one fma but rounds
    m1 m1 + m2 m2 + C1 twice gets S = +-1.2e-7 on about half the pixels, a distance of 1e-4 and gradients of 1 / (2 sqrt(S))."""
    x, _ = R.ssim_inputs(shape)
    val, gy, gx = hip_ssim(hip_ops, x, x.clone())
    print(f"identical {shape}: distance {float(val)!r}, nonzero gradient elements {int((gy != 0).sum())}, "
          f"largest {float(gy.abs().max())!r}")
    assert float(val) == 0.0
    assert not gy.any() and not gx.any()


def test_validation_ssim_of_identical_images_is_exactly_one(hip_ops):
    """csrc/valmetrics.hip scores SSIM with the same shape of expression in fp64 ((2 ux uy + C1) against
    (ux ux + uy uy + C1)); structural_similarity's numpy statements give every pixel of two identical images exactly 1,
    and a mean of ones is 1.0"""
    x, _ = R.ssim_inputs((2, 3, 27, 75))
    xd = x.to(hip_ops.device)
    table = hip_ops.valmetrics(xd, xd.clone(), ssim=True, hist=False).cpu()
    col = hip_ops.VALMETRIC_COLUMNS.index("ssim")
    assert table[:, col].tolist() == [1.0, 1.0], table[:, col].tolist()


@pytest.mark.parametrize("pair", R.SSIM_CONSTANT_PAIRS, ids=_ids)
def test_ssim_of_constant_images(hip_ops, pair):
    """two constant images a != b: S = 1 - (2ab + C1) / (a^2 + b^2 + C1) on the mapped values, the distance its root (float64
    agrees with the closed form, asserted on the CPU). Same measured rule as the random cases: 4 times RefOps's error
    against the closed form, floor 4 ulp. Measured (CPU RefOps): 2.9e-7, 1.4e-4, 2.7e-5, 4.0e-7 — an fp32 evaluation
    leaves 2^-24 of the squared means in the variances, up to 7e-5 of S2."""
    c = ssim_constant_case(*pair)
    want = math.sqrt(R.ssim_constant_closed_form(*pair))
    val, _, _ = hip_ssim(hip_ops, c["x"], c["y"])
    err = abs(float(val) - want) / want
    print(f"constant {pair}: cpu {c['cpu_val']:.3e} device {err:.3e}")
    assert err <= max(4 * c["cpu_val"], SSIM_FLOOR)


@pytest.mark.parametrize("shape", [(1, 1, 10, 20), (1, 1, 20, 10), (2, 3, 10, 10)], ids=_ids)
def test_ssim_refuses_planes_without_a_valid_pixel(hip_ops, shape):
    dev = hip_ops.device
    x = torch.zeros(shape, device=dev)
    out, g = nan_scalar(dev), torch.full(shape, NAN, device=dev)
    with pytest.raises(L.HipError, match="gs_ssim_distance: bad argument"):
        hip_ops.ssim_distance(x, x, out)
    with pytest.raises(L.HipError, match="gs_ssim_distance_backward: bad argument"):
        hip_ops.ssim_distance_backward(x, x, g)
    torch.cuda.synchronize()
    assert math.isnan(float(out)) and torch.isnan(g).all()


# ---- the small neighbours -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 4 * 256 * 4096 + 5])
def test_sum2(hip_ops, n):
    """out = a + b bit for bit: below one float4, a ragged tail, and past the 4096-workgroup cap of the launch"""
    g = torch.Generator().manual_seed(n % 1000)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    got = hip_ops.sum2(a.to(hip_ops.device), b.to(hip_ops.device)).cpu()
    assert torch.equal(got, a + b)


def test_sum2_refuses_an_unaligned_view(hip_ops):
    dev = hip_ops.device
    base = torch.ones(1029, device=dev)
    b = torch.ones(1028, device=dev)
    out = torch.full((1028,), NAN, device=dev)
    assert base[1:].data_ptr() % 16 != 0 and out.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    with pytest.raises(L.HipError, match="16-byte aligned"):
        hip_ops.sum2(base[1:], b)
    rc = hip_ops.lib.gs_sum2_f32(_ptr(base[1:]), _ptr(b), _ptr(out), 1028, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and torch.isnan(out).all()


def test_scalar_affine_at_its_maxima(hip_ops):
    """K = 16 scalars (three of them None) into R = 8 rows against float64 accumulated in k order: each of the K steps
    rounds once (an fma) by at most 2^-24 of the larger of the partial sum and the product"""
    dev = hip_ops.device
    vals, rows, consts = R.scalar_affine_case()
    xs = [None if v is None else torch.tensor(v, device=dev) for v in vals]
    want, big = R.scalar_affine(vals, rows, consts)
    got = hip_ops.scalar_affine(xs, rows, consts).cpu().double()
    assert not torch.isnan(got).any()
    assert ((got - want).abs() <= len(vals) * U * big).all(), (got, want)


def test_scalar_affine_refuses_more_than_its_maxima(hip_ops):
    dev = hip_ops.device
    x = torch.tensor(1.0, device=dev)
    with pytest.raises(L.HipError, match=r"gs_scalar_affine: bad argument \(K <= 16, R <= 8\)"):
        hip_ops.scalar_affine([x] * 17, [[1.0] * 17])
    with pytest.raises(L.HipError, match=r"gs_scalar_affine: bad argument \(K <= 16, R <= 8\)"):
        hip_ops.scalar_affine([x] * 2, [[1.0, 1.0]] * 9)
