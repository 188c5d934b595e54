"""The volumetric structure-consistency (MIND) loss restated from its formulas in plain torch, for tests/test_mind3d_cpu.py
and tests/test_mind3d_gpu.py, modelled on tests/mind_ref.py. Nothing here calls the package's kernels or the reference's
code (the reference has no volumetric MIND: include/ganslate_hip.h holds the definition): shifts and patch sums are slices of
zero-padded tensors. The same code runs in float64 (the judge) and in float32 (the yardstick: how far one honest fp32
evaluation lies from float64 on a given input).

Per volume I (a sample with C > 1 channels is reduced by the mean over its channels), zero outside:
  S_a(r) = I(r + a) for the 27 shifts a of the 3x3x3 region; d_a = S_a - I
  D_a(p) = sum_{q in 5^3, p+q inside} g(q) d_a(p+q)^2,  g(q) = exp(-|q|_2 / sigma^2) (Euclidean distance, not squared; the
           125 weights are rounded as the 2-D ones: distance and quotient in fp32, exp in double, stored as fp32)
  B_b(p) = sum_{q in 5^3, p+q inside} S_b(p+q) for the 27 shifts b of the 3^3 neighbourhood; V = unbiased variance of the 27
  n_a = exp(-D_a / (V + 1e-8)); f_a = n_a / sum_c n_c
  channel i <-> depth offset i % 3 - 1, row offset (i // 3) % 3 - 1, column offset i // 9 - 1
  L(X, Y) = sum_{n,a,p} |f_a^X - f_a^Y| / (D H W 27)      (a sum over the batch; lambda_structure multiplies it outside)

`border="clamp"` and `drop_tap=(tz, ty, tx)` are deliberately WRONG variants (edge replication instead of zeros for the
shifted volumes; one patch weight left out): the CPU tests use them to show that the tolerances can see such a mistake."""
import functools
import math

import torch
import torch.nn.functional as TF

from oracle.ops_ref import RefOps

F64, F32 = torch.float64, torch.float32
NL, PATCH, NBR, SIGMA, EPS = 3, 5, 3, 2.0, 1e-8
NS = NL ** 3


def patch_weights(sigma=SIGMA, dtype=F64):
    q = torch.arange(PATCH, dtype=F32) - (PATCH - 1) // 2
    dist = torch.sqrt(q[:, None, None] ** 2 + q[None, :, None] ** 2 + q[None, None, :] ** 2)   # fp32, exact integers under the root
    e = -dist / torch.tensor(sigma * sigma, dtype=F32)                                          # fp32 quotient
    return torch.exp(e.to(F64)).to(F32).to(dtype)                                               # exp in double, stored as fp32


def _volume(img):
    if img.dim() != 5:
        raise ValueError(f"[N, C, D, H, W] expected, got {tuple(img.shape)}")
    return img.mean(dim=1) if img.shape[1] > 1 else img[:, 0]


def _shifted(I, border):
    """[N, 27, D, H, W]: channel i = I(r + a), a = (i % 3 - 1, (i // 3) % 3 - 1, i // 9 - 1) in (depth, row, column)"""
    N, D, H, W = I.shape
    if border == "zero":
        Ip = TF.pad(I, (1,) * 6)
    else:
        Ip = TF.pad(I[:, None], (1,) * 6, mode="replicate")[:, 0]
    return torch.stack([Ip[:, i % 3:i % 3 + D, (i // 3) % 3:(i // 3) % 3 + H, i // 9:i // 9 + W] for i in range(NS)], dim=1)


def _patch_sum(maps, g):
    """sum_q g(q) maps(p + q) over the 5x5x5 patch, zero outside"""
    D, H, W = maps.shape[-3:]
    r = (PATCH - 1) // 2
    mp = TF.pad(maps, (r,) * 6)
    out = torch.zeros_like(maps)
    for tz in range(PATCH):
        for ty in range(PATCH):
            for tx in range(PATCH):
                if g[tz, ty, tx] != 0:
                    out = out + g[tz, ty, tx] * mp[..., tz:tz + D, ty:ty + H, tx:tx + W]
    return out


def descriptor(img, sigma=SIGMA, border="zero", drop_tap=None):
    """[N, C, D, H, W] -> [N, 27, D, H, W] in img's dtype"""
    I = _volume(img)
    g = patch_weights(sigma, I.dtype)
    if drop_tap is not None:
        g = g.clone()
        g[drop_tap] = 0
    d = _shifted(I, border) - I[:, None]
    Dm = _patch_sum(d * d, g)
    B = _patch_sum(_shifted(I, border), torch.ones_like(g))
    V = ((B - B.mean(dim=1, keepdim=True)) ** 2).sum(dim=1, keepdim=True) / (NBR ** 3 - 1)
    n = torch.exp(-Dm / (V + EPS))
    return n / n.sum(dim=1, keepdim=True)


def structure_l1(X, Y, **kw):
    """sum |f^X - f^Y| / (D H W 27), without lambda_structure"""
    D, H, W = X.shape[-3:]
    return (descriptor(X, **kw) - descriptor(Y, **kw)).abs().sum() / (D * H * W * NS)


def loss_and_grads(X, Y, dtype, **kw):
    """(features of X, loss, dL/dX, dL/dY), all in `dtype`"""
    X, Y = X.to(dtype).clone().requires_grad_(), Y.to(dtype).clone().requires_grad_()
    loss = structure_l1(X, Y, **kw)
    gx, gy = torch.autograd.grad(loss, (X, Y))
    with torch.no_grad():
        feat = descriptor(X, **kw)
    return feat.detach(), loss.detach(), gx, gy


# ---- the backend of the CPU recipe tests -------------------------------------------------------------------------------
class Mind3dRefOps(RefOps):
    """RefOps plus the three volumetric MIND methods of HipOps, on the float32 restatement"""

    def mind3d_descriptor(self, x, out=None, cfg=None):
        f = descriptor(x.detach().float())
        return f if out is None else out.copy_(f)

    def mind3d_l1(self, x, y, out, cfg=None):
        out.copy_(structure_l1(x.detach().float(), y.detach().float()))

    def mind3d_l1_backward(self, x, y, grad_y, grad_scale=None, cfg=None):
        yy = y.detach().float().clone().requires_grad_()
        with torch.enable_grad():
            (g,) = torch.autograd.grad(structure_l1(x.detach().float(), yy), yy)
        grad_y.copy_(g * (grad_scale if grad_scale is not None else 1.0))


# ---- cases ----------------------------------------------------------------------------------------------------------------
def _random(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _smooth(shape, seed):
    """a few low-frequency waves plus a little noise, in (-1, 1)"""
    N, C, D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.arange(D, dtype=F32)[:, None, None] / max(D, 2)
    y = torch.arange(H, dtype=F32)[None, :, None] / max(H, 2)
    x = torch.arange(W, dtype=F32)[None, None, :] / max(W, 2)
    p = torch.rand((N, C, 4), generator=g) * 6.0
    out = torch.empty(shape)
    for n in range(N):
        for c in range(C):
            a, b, cc, d = p[n, c].tolist()
            out[n, c] = 0.45 * torch.sin(2 * math.pi * (1.5 * y + 0.8 * z + a / 6)) * torch.cos(2 * math.pi * (x + b / 6)) + \
                0.35 * torch.sin(2 * math.pi * (0.7 * x + 1.3 * y + 1.1 * z + cc / 6) + d)
    return (out + 0.05 * _random(shape, seed + 1)).clamp(-0.999, 0.999)


def _ball(shape, seed, centre, radius):
    """constant -1 background (a tanh-saturated medical volume) around a textured ball"""
    N, C, D, H, W = shape
    zz = torch.arange(D, dtype=F32)[:, None, None] - centre[0]
    yy = torch.arange(H, dtype=F32)[None, :, None] - centre[1]
    xx = torch.arange(W, dtype=F32)[None, None, :] - centre[2]
    inside = (zz * zz + yy * yy + xx * xx) <= radius * radius
    tex = 0.2 + 0.6 * _random(shape, seed)
    return torch.where(inside, tex, torch.full(shape, -1.0))


# name -> (X, Y): the shapes the kernels are tested at. tiny: every extent below the halo; odd: odd extents, partial boxes;
# tiles: several boxes with remainders on all three axes for any box edge up to 8 in depth and rows and 16 in columns, three
# channels reduced by their mean; ball: V = 0 and D = 0 exactly over the background
CASES = {
    "tiny_1x1x2x3x5": lambda: (_random((1, 1, 2, 3, 5), 11), _random((1, 1, 2, 3, 5), 12)),
    "odd_2x1x5x11x13": lambda: (_smooth((2, 1, 5, 11, 13), 21), _smooth((2, 1, 5, 11, 13), 22)),
    "tiles_2x3x18x21x37": lambda: (_random((2, 3, 18, 21, 37), 31), _random((2, 3, 18, 21, 37), 32)),
    "ball_1x1x10x20x22": lambda: (_ball((1, 1, 10, 20, 22), 41, (4.0, 9.0, 10.0), 3.5),
                                  _ball((1, 1, 10, 20, 22), 42, (5.0, 10.0, 12.0), 4.25)),
}
# two different constant volumes: every n is 1 in the interior, the float32 evaluation alone is off by 100 % in the
# gradient there — loss and gradient must only be finite
CONSTANT_PAIR = lambda: (torch.full((1, 1, 6, 9, 10), 0.25), torch.full((1, 1, 6, 9, 10), -0.5))      # noqa: E731
GRAD_SCALE = 0.5          # a power of two: scaling the float64 gradient by it is exact
# the deliberately wrong variants a case can see. On tiny (depth 2) the patch tap (0, 1, 2) — two planes up — never lands
# inside the volume, so leaving it out changes nothing there: that case sees only the border rule.
WRONG_TAP = (0, 1, 2)
VISIBLE_WRONG = {
    "tiny_1x1x2x3x5": (dict(border="clamp"),),
    "odd_2x1x5x11x13": (dict(border="clamp"), dict(drop_tap=WRONG_TAP)),
    "tiles_2x3x18x21x37": (dict(border="clamp"), dict(drop_tap=WRONG_TAP)),
    "ball_1x1x10x20x22": (dict(border="clamp"), dict(drop_tap=WRONG_TAP)),
}
FLIPS = ((), (2,), (3,), (4,))          # the identity and the three single-axis flips: L is exactly flip-invariant


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 results of a case and the yardstick e32 = max |float32 restatement - float64| per quantity; for the scalar
    loss the largest |l32 - l64| over the case and its three single-axis flips (the borders are zero and the weights and
    shift sets symmetric, so the flips are the same quantity summed in another order: one e32 can be small by chance).
    Computed once per process; callers must not modify the tensors."""
    X, Y = CASES[name]()
    f64, l64, gx64, gy64 = loss_and_grads(X, Y, F64)
    f32, l32, gx32, gy32 = loss_and_grads(X, Y, F32)
    fy64 = descriptor(Y.to(F64))
    err = lambda a, b: float((a.to(F64) - b).abs().max())      # noqa: E731
    return {
        "X": X, "Y": Y, "feat_x": f64, "feat_y": fy64, "loss": l64, "grad_x": gx64, "grad_y": gy64,
        "e32": {"feat": max(err(f32, f64), err(descriptor(Y), fy64)), "loss": loss_e32(X, Y),
                "grad": max(err(gx32, gx64), err(gy32, gy64))},
        "max": {"feat": float(max(f64.abs().max(), fy64.abs().max())), "loss": float(l64.abs()),
                "grad": float(max(gx64.abs().max(), gy64.abs().max()))},
    }


def loss_e32(X, Y):
    """the loss yardstick on a pair: max over the pair and its three single-axis flips of |l32 - l64|"""
    with torch.no_grad():
        return max(abs(float(structure_l1(X.flip(f).float(), Y.flip(f).float())) -
                       float(structure_l1(X.flip(f).to(F64), Y.flip(f).to(F64)))) for f in FLIPS)


def bound(ref, what, factor=4.0):
    """the GPU tolerance of a case: factor * e32 + one fp32 ulp of the quantity's maximum"""
    return factor * ref["e32"][what] + ref["max"][what] * 2.0 ** -23
