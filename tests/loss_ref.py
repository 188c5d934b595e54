"""float64 statements of what csrc/loss.hip computes, written from the mathematics, plus the case lists and input
builders of tests/test_loss_edges_cpu.py and tests/test_loss_edges_gpu.py. Nothing here calls the oracle (RefOps,
oracle/) or anything of the package: the CPU module pins these statements to the oracle and to recorded reference vectors,
the GPU module holds the kernels to them.

Every function takes the fp32 tensors the kernel takes, widens them to float64 first and returns float64.
  l1, mse_const, mean        nn.L1Loss / nn.MSELoss against a constant / tensor.mean() (cyclegan_losses.py:64,75,97-101,
                             adversarial_loss.py:28-29,60-62, train_metrics.py:27-33)
  adv                        the four branches of AdversarialLoss.calculate_loss (adversarial_loss.py:52-73)
  ssim_*                     SSIMLoss.forward (nn/losses/utils/ssim.py:65-99) on (x + 1) / 2, used as a loss
                             (cyclegan_losses.py:78-90)
"""
import math

import torch

F64 = torch.float64


# ---- reductions and their gradients --------------------------------------------------------------------------------
def l1(a, b):
    d = a.to(F64) - b.to(F64)
    return d.abs().mean(), torch.sign(d) / d.numel()


def mse_const(x, target):
    d = x.to(F64) - float(target)
    return (d * d).mean(), 2.0 * d / d.numel()


def mean(x):
    x = x.to(F64)
    return x.mean(), torch.full_like(x, 1.0 / x.numel())


def softplus(z):
    """log(1 + exp(z)) without a threshold: max(z, 0) + log1p(exp(-|z|)) loses nothing in float64"""
    return z.clamp_min(0.0) + torch.log1p(torch.exp(-z.abs()))


def adv(x, mode, target_is_real):
    """-> (loss, d loss / d x). loss is a scalar, for nonsaturating one value per sample x[r] (and the gradient that of
    sum_r loss[r], so a per-row upstream gradient multiplies row r)"""
    x = x.to(F64)
    n = x.numel()
    t = 1.0 if target_is_real else 0.0
    if mode == "lsgan":
        return ((x - t) ** 2).mean(), 2.0 * (x - t) / n
    if mode == "vanilla":
        f = x.clamp_min(0.0) - x * t + torch.log1p(torch.exp(-x.abs()))
        return f.mean(), (torch.sigmoid(x) - t) / n
    if mode == "wgangp":
        s = -1.0 if target_is_real else 1.0
        return s * x.mean(), torch.full_like(x, s / n)
    if mode == "nonsaturating":
        s = -1.0 if target_is_real else 1.0
        rows = x.shape[0]
        z = s * x.reshape(rows, -1)
        return softplus(z).mean(dim=1), (s * torch.sigmoid(z) / z.shape[1]).reshape(x.shape)
    raise ValueError(mode)


# ---- SSIM distance -----------------------------------------------------------------------------------------------------
C1, C2 = 0.01 ** 2, 0.03 ** 2


def gauss11():
    c = torch.arange(11, dtype=F64) - 5.0
    g = torch.exp(-(c * c) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def _planes(t):
    """(N, C, H, W) or (N, C, D, H, W) -> (planes, 1, H, W): every channel (and depth slice) is blurred on its own"""
    return t.to(F64).reshape(-1, 1, t.shape[-2], t.shape[-1])


def _blur(t):
    g = gauss11()
    t = torch.nn.functional.conv2d(t, g.view(1, 1, 1, 11))
    return torch.nn.functional.conv2d(t, g.view(1, 1, 11, 1))


def ssim_s_map(x, y):
    """S = 2 - S1 - S2 per valid pixel, (planes, H - 10, W - 10); the distance is mean(sqrt(relu(S)))"""
    X, Y = (_planes(x) + 1.0) / 2.0, (_planes(y) + 1.0) / 2.0
    mu1, mu2 = _blur(X), _blur(Y)
    s1 = _blur(X * X) - mu1 * mu1
    s2 = _blur(Y * Y) - mu2 * mu2
    s12 = _blur(X * Y) - mu1 * mu2
    S1 = (2.0 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)
    S2 = (2.0 * s12 + C2) / (s1 + s2 + C2)
    return (2.0 - (S1 + S2))[:, 0]


def ssim_distance(x, y):
    return torch.sqrt(torch.relu(ssim_s_map(x, y))).mean()


def ssim_grad_y(x, y):
    """d ssim_distance / d y by autograd in float64, in y's shape"""
    yy = y.to(F64).clone().requires_grad_()
    with torch.enable_grad():
        d = ssim_distance(x.to(F64), yy)
    (g,) = torch.autograd.grad(d, yy)
    return g


def ssim_constant_closed_form(a, b):
    """S for two constant images of values a and b (in [-1, 1]): the variances vanish, S2 = 1 and S = 1 - S1"""
    a, b = (a + 1.0) / 2.0, (b + 1.0) / 2.0
    return 1.0 - (2.0 * a * b + C1) / (a * a + b * b + C1)


# ---- fp32 ulp arithmetic ------------------------------------------------------------------------------------------------
def ulp32(ref64):
    """spacing of fp32 at the float64 value(s) rounded to fp32 (the subnormal spacing 2^-149 at and below the subnormals)"""
    v = torch.as_tensor(ref64, dtype=F64).float().double().abs()
    _, e = torch.frexp(v)                                   # v = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), (e - 24).clamp_min(-149))


def err_ulp32(got, ref64):
    """|got - ref64| in units of ulp32(ref64), elementwise, float64"""
    ref64 = torch.as_tensor(ref64, dtype=F64)
    return (got.detach().cpu().double().reshape(ref64.shape) - ref64).abs() / ulp32(ref64)


# ---- reduction cases --------------------------------------------------------------------------------------------------
REDUCTION_LENGTHS = [1, 63, 65, 255, 257, 2047, 2048, 2049, 4097, 262_145, 2 ** 21, 2 ** 21 + 1, 2 ** 21 + 262_147,
                     3 * 2 ** 21 + 77]
REDUCTION_OPS = ["l1", "mse0", "mse1", "mean", "lsgan_real", "lsgan_fake", "wgangp_real", "wgangp_fake"]
GRAD_OPS = [op for op in REDUCTION_OPS if op != "mean"]
TERM_ROUNDINGS = {"mean": 1, "l1": 2, "mse0": 2, "mse1": 2, "lsgan_real": 2, "lsgan_fake": 2, "wgangp_real": 1,
                  "wgangp_fake": 1}


def red_blocks(n):
    """workgroups of 256 threads a reduction over n elements is launched with: 2048 elements each, at most 1024"""
    return max(1, min(1024, (n + 2047) // 2048))


def serial_adds(n):
    """k: elements one thread adds up serially, ceil(n / (G * 256))"""
    g = red_blocks(n) * 256
    return (n + g - 1) // g


def op_target(op):
    """the constant an operation subtracts (None: it has none)"""
    return {"mse0": 0.0, "mse1": 1.0, "lsgan_real": 1.0, "lsgan_fake": 0.0}.get(op)


def reference(op, a, b=None):
    """(loss, gradient) in float64 of one reduction op on fp32 inputs"""
    if op == "l1":
        return l1(a, b)
    if op in ("mse0", "mse1"):
        return mse_const(a, op_target(op))
    if op == "mean":
        return mean(a)
    mode, side = op.split("_")
    return adv(a, mode, side == "real")


def terms64(op, a, b=None):
    """the per-element terms the kernel sums, in float64"""
    a = a.to(F64)
    if op == "l1":
        return (a - b.to(F64)).abs()
    if op == "mean":
        return a
    if op.startswith("wgangp"):
        return -a if op.endswith("real") else a
    return (a - op_target(op)) ** 2


def marked_positions(n, seed=0):
    """where a reduction over n elements can drop or double an element: both ends, the wavefront / workgroup / 8-per-thread
    edges, the first wrap of the grid-stride loop (G * 256 with G = red_blocks(n)) and ~50 seeded random positions"""
    G = red_blocks(n)
    fixed = [0, 1, 63, 64, 255, 256, 2047, 2048, G * 256 - 1, G * 256, G * 256 + 1, n - 2, n - 1]
    g = torch.Generator().manual_seed(1000 + seed + n % 9973)
    rnd = torch.randint(0, n, (50,), generator=g).tolist()
    return sorted({p for p in fixed + rnd if 0 <= p < n})


def sparse_case(op, n, seed=0):
    """Integer-domain input of one reduction: the neutral value everywhere (0, or the constant the op subtracts), and at the
    marked positions a distinct small integer away from it, with alternating sign. Every term (|d|, d, d^2) is an integer
    and the sum of the terms' magnitudes stays far below 2^24 (asserted from float64 in test_loss_edges_cpu.py), so the
    fp32 sum is exact in any order. -> (a, b or None)"""
    pos = marked_positions(n, seed)
    t = op_target(op) or 0.0
    a = torch.full((n,), t, dtype=torch.float32)
    b = torch.zeros(n, dtype=torch.float32) if op == "l1" else None
    for j, p in enumerate(pos):
        v = float(j + 1) * (1.0 if j % 2 == 0 else -1.0)
        if op == "l1" and j % 3 == 2:
            b[p] = v                                           # the second operand carries some of the differences
        else:
            a[p] = t + v
    return a, b


_DENSE = {}


def dense_case(op, n, grid=False):
    """Dense data of one reduction: seeded uniform fp32 values in (-4, 4). With `grid` they lie on the grid of 2^-12, so that
    every difference a gradient kernel forms (a - b, x - 0, x - 1) is exact in fp32 and the roundings counted in the
    gradient tests' bound (the factor k, one multiply) are the only ones. One base tensor per operand is drawn once and
    sliced."""
    if not _DENSE:
        g = torch.Generator().manual_seed(77)
        nmax = max(REDUCTION_LENGTHS)
        for k in ("a", "b"):
            _DENSE[k] = torch.rand(nmax, generator=g) * 8.0 - 4.0
            _DENSE[k + "_grid"] = torch.randint(-(2 ** 14) + 1, 2 ** 14, (nmax,), generator=g).float() / 4096.0
    s = "_grid" if grid else ""
    return _DENSE["a" + s][:n], (_DENSE["b" + s][:n] if op == "l1" else None)


# ---- transcendental objectives ------------------------------------------------------------------------------------------
def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def special_logits():
    """logits at which vanilla / nonsaturating change branch, saturate or cancel: around the soft-plus threshold 20, where
    exp(-|x|) drops below the fp32 ulp of 1 (about 16.6), underflows (88, 104) and far beyond"""
    up, down = _f32(float("inf")), _f32(float("-inf"))
    t20 = _f32(20.0)
    vals = [torch.nextafter(t20, up), t20, torch.nextafter(t20, down), -torch.nextafter(t20, up), -t20,
            -torch.nextafter(t20, down)]
    vals += [_f32(v) for v in (0.0, -0.0, 1e-8, -1e-8, 19.999, -19.999, 30.0, -30.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)]
    return torch.stack(vals)


TRANSCENDENTAL_LENGTHS = [1, 257, 2049, 7200]
NONSAT_ROWS = [1, 3, 8]
NONSAT_PER = [1, 255, 257, 900]


def logits(n, seed=5):
    """n logits: the special values first (n = 1 gets the float just above the threshold 20), seeded randn * 6 after"""
    s = special_logits()
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed + n)) * 6.0
    m = min(n, s.numel())
    x[:m] = s[:m]
    return x


def row_logits(rows, per, seed=9):
    """rows x per logits with the special values spread over the rows (row r starts at special value r * 3)"""
    s = special_logits()
    x = torch.randn(rows, per, generator=torch.Generator().manual_seed(seed + rows * 1000 + per)) * 6.0
    for r in range(rows):
        m = min(per, s.numel())
        x[r, :m] = s.roll(-3 * r)[:m]
    return x


def row_scales(rows):
    """distinct per-row upstream gradients"""
    return torch.tensor([0.5 + 0.75 * r for r in range(rows)], dtype=torch.float32)


# ---- SSIM cases --------------------------------------------------------------------------------------------------------
SSIM_SHAPES = [(1, 1, 11, 11), (1, 1, 11, 43), (2, 1, 26, 42), (1, 3, 27, 75), (1, 2, 3, 12, 47), (2, 3, 64, 64)]
SSIM_IDENTICAL_SHAPES = [(1, 3, 27, 75), (2, 3, 64, 64)]
SSIM_CONSTANT_PAIRS = [(-1.0, 1.0), (-0.5, 0.75), (0.25, -0.75), (1.0, 0.0)]
SSIM_CONSTANT_SHAPE = (1, 2, 27, 43)
SSIM_MIN_S = 1e-3
SSIM_SEED = 12


def ssim_inputs(shape, seed=SSIM_SEED):
    """y = 0.6 x + 0.4 noise, both in [-1, 1] (as test_ops_gpu.test_ssim_distance_backward draws them)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g) * 2 - 1
    y = x * 0.6 + (torch.rand(shape, generator=g) * 2 - 1) * 0.4
    return x, y


def ssim_constant_inputs(a, b, shape=SSIM_CONSTANT_SHAPE):
    return torch.full(shape, a, dtype=torch.float32), torch.full(shape, b, dtype=torch.float32)


def per_plane_rel_err(got, ref64):
    """largest |got - ref| over largest |ref|, per H x W plane -> float64 [planes]"""
    H, W = ref64.shape[-2:]
    r = ref64.reshape(-1, H * W)
    g = got.detach().cpu().double().reshape(-1, H * W)
    return (g - r).abs().amax(dim=1) / r.abs().amax(dim=1)


# ---- scalar_affine -----------------------------------------------------------------------------------------------------
def scalar_affine_case(K=16, R=8, seed=31):
    """values (None at a few k), rows, consts of a K x R scalar_affine at the library's maxima"""
    g = torch.Generator().manual_seed(seed)
    vals = (torch.randn(K, generator=g) * 3.0).float().tolist()
    vals = [None if k in (2, 7, K - 1) else v for k, v in enumerate(vals)]
    rows = torch.randn(R, K, generator=g).float().tolist()
    consts = torch.randn(R, generator=g).float().tolist()
    return vals, rows, consts


def scalar_affine(vals, rows, consts):
    """-> (float64 [R] accumulated in k order, float64 [R] sum of the magnitudes of the partial sums: K roundings of at
    most half an ulp of a partial sum each bound the fp32 error by K * 2^-24 * the largest partial sum's magnitude)"""
    out, big = [], []
    for row, c in zip(rows, consts):
        acc, m = float(c), abs(float(c))
        for w, v in zip(row, vals):
            if v is not None:
                acc += float(w) * float(v)
                m = max(m, abs(acc), abs(float(w) * float(v)))
        out.append(acc)
        big.append(m)
    return torch.tensor(out, dtype=F64), torch.tensor(big, dtype=F64)


assert math.isclose(float(gauss11().sum()), 1.0)
