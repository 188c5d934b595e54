"""The structure-consistency (MIND) loss restated from its formulas in plain torch, for tests/test_mind_cpu.py and
tests/test_mind_gpu.py. Nothing here calls the package's kernels or the reference's code: shifts and patch sums are slices
of zero-padded tensors. The same code runs in float64 (the judge) and in float32 (the yardstick: how far one honest fp32
evaluation lies from float64 on a given input).

Per plane I (an image with C > 1 channels is reduced by the mean over its channels), zero outside:
  S_a(r) = I(r + a) for the 81 shifts a of the 9x9 region; d_a = S_a - I
  D_a(p) = sum_{q in 7x7, p+q inside} g(q) d_a(p+q)^2,  g(q) = exp(-|q|_2 / sigma^2) (Euclidean distance, not squared; the
           reference builds these 49 weights in fp32 — distance and quotient in fp32, exp in double, stored as fp32 — and
           that rounding is part of what it computes, so it is restated too)
  B_b(p) = sum_{q in 7x7, p+q inside} S_b(p+q) for the 9 shifts b of the 3x3 neighbourhood; V = unbiased variance of the nine
  n_a = exp(-D_a / (V + 1e-8)); f_a = n_a / sum_c n_c;  channel i <-> row offset i % 9 - 4, column offset i // 9 - 4
  L(X, Y) = sum_{n,a,p} |f_a^X - f_a^Y| / (H W 81)      (a sum over the batch; lambda_structure multiplies it outside)

`border="clamp"` and `drop_tap=(ty, tx)` are deliberately WRONG variants (edge replication instead of zeros for the shifted
images; one patch weight left out): the CPU tests use them to show that the tolerances can see such a mistake."""
import functools
import math

import torch
import torch.nn.functional as TF

from oracle.ops_ref import RefOps

F64, F32 = torch.float64, torch.float32
NL, PATCH, NBR, SIGMA, EPS = 9, 7, 3, 2.0, 1e-8


def patch_weights(sigma=SIGMA, dtype=F64):
    q = torch.arange(PATCH, dtype=F32) - (PATCH - 1) // 2
    dist = torch.sqrt(q[:, None] ** 2 + q[None, :] ** 2)                  # fp32, exact integers under the root
    e = -dist / torch.tensor(sigma * sigma, dtype=F32)                     # fp32 quotient
    return torch.exp(e.to(F64)).to(F32).to(dtype)                          # exp in double, stored as fp32


def _plane(img):
    if img.dim() != 4:
        raise ValueError(f"[N, C, H, W] expected, got {tuple(img.shape)}")
    return img.mean(dim=1) if img.shape[1] > 1 else img[:, 0]


def _shifted(I, radius, border):
    """[N, (2 radius + 1)^2, H, W]: channel i = I(r + a), a = (i % k - radius, i // k - radius)"""
    N, H, W = I.shape
    k = 2 * radius + 1
    if border == "zero":
        Ip = TF.pad(I, (radius,) * 4)
    else:
        Ip = TF.pad(I[:, None], (radius,) * 4, mode="replicate")[:, 0]
    return torch.stack([Ip[:, i % k:i % k + H, i // k:i // k + W] for i in range(k * k)], dim=1)


def _patch_sum(maps, g):
    """sum_q g(q) maps(p + q) over the 7x7 patch, zero outside"""
    H, W = maps.shape[-2:]
    r = (PATCH - 1) // 2
    mp = TF.pad(maps, (r,) * 4)
    out = torch.zeros_like(maps)
    for ty in range(PATCH):
        for tx in range(PATCH):
            if g[ty, tx] != 0:
                out = out + g[ty, tx] * mp[..., ty:ty + H, tx:tx + W]
    return out


def descriptor(img, sigma=SIGMA, border="zero", drop_tap=None):
    """[N, C, H, W] -> [N, 81, H, W] in img's dtype"""
    I = _plane(img)
    g = patch_weights(sigma, I.dtype)
    if drop_tap is not None:
        g = g.clone()
        g[drop_tap] = 0
    d = _shifted(I, (NL - 1) // 2, border) - I[:, None]
    D = _patch_sum(d * d, g)
    B = _patch_sum(_shifted(I, (NBR - 1) // 2, border), torch.ones_like(g))
    V = ((B - B.mean(dim=1, keepdim=True)) ** 2).sum(dim=1, keepdim=True) / (NBR * NBR - 1)
    n = torch.exp(-D / (V + EPS))
    return n / n.sum(dim=1, keepdim=True)


def structure_l1(X, Y, **kw):
    """sum |f^X - f^Y| / (H W 81), without lambda_structure"""
    H, W = X.shape[-2:]
    return (descriptor(X, **kw) - descriptor(Y, **kw)).abs().sum() / (H * W * NL * NL)


def loss_and_grads(X, Y, dtype, **kw):
    """(features of X, loss, dL/dX, dL/dY), all in `dtype`"""
    X, Y = X.to(dtype).clone().requires_grad_(), Y.to(dtype).clone().requires_grad_()
    loss = structure_l1(X, Y, **kw)
    gx, gy = torch.autograd.grad(loss, (X, Y))
    with torch.no_grad():
        feat = descriptor(X, **kw)
    return feat.detach(), loss.detach(), gx, gy


# ---- the backend of the CPU recipe tests -------------------------------------------------------------------------------
class MindRefOps(RefOps):
    """RefOps plus the three MIND methods of HipOps, on the float32 restatement"""

    def mind_descriptor(self, x, out=None, cfg=None):
        f = descriptor(x.detach().float())
        return f if out is None else out.copy_(f)

    def mind_l1(self, x, y, out, cfg=None):
        out.copy_(structure_l1(x.detach().float(), y.detach().float()))

    def mind_l1_backward(self, x, y, grad_y, grad_scale=None, cfg=None):
        yy = y.detach().float().clone().requires_grad_()
        with torch.enable_grad():
            (g,) = torch.autograd.grad(structure_l1(x.detach().float(), yy), yy)
        grad_y.copy_(g * (grad_scale if grad_scale is not None else 1.0))


# ---- cases ----------------------------------------------------------------------------------------------------------------
def _random(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _smooth(shape, seed):
    """a few low-frequency waves plus a little noise, in (-1, 1)"""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(H, dtype=F32)[:, None] / max(H, 2)
    x = torch.arange(W, dtype=F32)[None, :] / max(W, 2)
    p = torch.rand((N, C, 4), generator=g) * 6.0
    out = torch.empty(shape)
    for n in range(N):
        for c in range(C):
            a, b, cc, d = p[n, c].tolist()
            out[n, c] = 0.45 * torch.sin(2 * math.pi * (1.5 * y + a / 6)) * torch.cos(2 * math.pi * (x + b / 6)) + \
                0.35 * torch.sin(2 * math.pi * (0.7 * x + 1.3 * y + cc / 6) + d)
    return (out + 0.05 * _random(shape, seed + 1)).clamp(-0.999, 0.999)


def _disc(shape, seed, centre, radius):
    """constant -1 background (a tanh-saturated medical slice) around a textured disc"""
    N, C, H, W = shape
    yy = torch.arange(H, dtype=F32)[:, None] - centre[0]
    xx = torch.arange(W, dtype=F32)[None, :] - centre[1]
    inside = (yy * yy + xx * xx) <= radius * radius
    tex = 0.2 + 0.6 * _random(shape, seed)
    return torch.where(inside, tex, torch.full(shape, -1.0))


# name -> (X, Y): the shapes the kernels are tested at. tiny: smaller than the halo; odd: odd extents, one partial tile;
# tiles: at least three tiles with remainders on both axes for any tile up to 32, three channels reduced by the mean;
# disc: V = 0 and D = 0 exactly over the background
CASES = {
    "tiny_1x1x7x9": lambda: (_random((1, 1, 7, 9), 11), _random((1, 1, 7, 9), 12)),
    "odd_2x1x19x23": lambda: (_smooth((2, 1, 19, 23), 21), _smooth((2, 1, 19, 23), 22)),
    "tiles_3x3x70x75": lambda: (_random((3, 3, 70, 75), 31), _random((3, 3, 70, 75), 32)),
    "disc_1x1x40x48": lambda: (_disc((1, 1, 40, 48), 41, (19.0, 22.0), 11.0), _disc((1, 1, 40, 48), 42, (21.0, 25.0), 12.5)),
}
# two different constant images: every n is 1 in the interior, the float32 evaluation alone is off by 100 % in the
# gradient there — loss and gradient must only be finite
CONSTANT_PAIR = lambda: (torch.full((1, 1, 20, 21), 0.25), torch.full((1, 1, 20, 21), -0.5))      # noqa: E731
GRAD_SCALE = 0.5          # a power of two: scaling the float64 gradient by it is exact


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 results of a case and the yardstick e32 = max |float32 restatement - float64| per quantity. Computed once per
    process; callers must not modify the tensors."""
    X, Y = CASES[name]()
    f64, l64, gx64, gy64 = loss_and_grads(X, Y, F64)
    f32, l32, gx32, gy32 = loss_and_grads(X, Y, F32)
    fy64 = descriptor(Y.to(F64))
    err = lambda a, b: float((a.to(F64) - b).abs().max())      # noqa: E731
    return {
        "X": X, "Y": Y, "feat_x": f64, "feat_y": fy64, "loss": l64, "grad_x": gx64, "grad_y": gy64,
        "e32": {"feat": max(err(f32, f64), err(descriptor(Y), fy64)), "loss": err(l32, l64),
                "grad": max(err(gx32, gx64), err(gy32, gy64))},
        "max": {"feat": float(max(f64.abs().max(), fy64.abs().max())), "loss": float(l64.abs()),
                "grad": float(max(gx64.abs().max(), gy64.abs().max()))},
    }


def bound(ref, what, factor=4.0):
    """the GPU tolerance of a case: factor * e32 + one fp32 ulp of the quantity's maximum"""
    return factor * ref["e32"][what] + ref["max"][what] * 2.0 ** -23
