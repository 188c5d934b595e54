"""Float64 oracle of the multi-modal 2-D image path (data/multimodal_images.py, csrc/imgstack.hip): the tap tables of
torch's bicubic tensor resize (align_corners=False, no antialiasing, cubic convolution A = -0.75), the resize, the
clamp / min-max / noise chain, the Philox4x32-10 + Box-Muller noise plane, and the per-element envelope
E = sum |w_y w_x x| that every error bound of tests/test_mmimg_*.py is stated in. Written from the formulas alone, in
numpy float64 and Python integers; nothing here calls the code under test."""
import math

import numpy as np

A = -0.75
EPS32 = 2.0 ** -23
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def c1(x):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def c2(x):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def taps(n_in, n_out):
    """(idx int64 [n_out, 4], w float64 [n_out, 4]) of one axis"""
    o = np.arange(n_out, dtype=np.float64)
    s = (o + 0.5) * n_in / n_out - 0.5
    f = np.floor(s)
    t = s - f
    idx = np.clip(f[:, None].astype(np.int64) + np.arange(-1, 3)[None, :], 0, n_in - 1)
    w = np.stack([c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)], 1)
    return idx, w


def resize(x, out_h, out_w):
    """x float64 [C, h, w] -> (r, E) float64 [C, out_h, out_w]: the 4 x 4 weighted sum and the sum of the absolute values of
    its 16 terms"""
    x = np.asarray(x, np.float64)
    iy, wy = taps(x.shape[1], out_h)
    ix, wx = taps(x.shape[2], out_w)
    g = x[:, iy[:, :, None, None], ix[None, None, :, :]]                     # [C, out_h, 4, out_w, 4]
    w = wy[:, :, None, None] * wx[None, None, :, :]
    return (g * w).sum(axis=(2, 4)), (np.abs(g) * np.abs(w)).sum(axis=(2, 4))


def chain(r, lo, hi, rescale=True, noise_std=0.0, z=None):
    """clamp -> min-max to [-1, 1] -> + noise_std * z, clamp(-1, 1); float64"""
    v = np.clip(np.asarray(r, np.float64), lo, hi)
    if rescale:
        v = 2.0 * ((v - lo) / (hi - lo)) - 1.0
    if noise_std:
        v = np.clip(v + noise_std * z, -1.0, 1.0)
    return v


def scale(lo, hi, rescale=True):
    """the factor s by which the chain stretches an error of the resize"""
    return 2.0 / (hi - lo) if rescale else 1.0


def to_chw(array):
    a = np.asarray(array)
    return (a[None] if a.ndim == 2 else np.moveaxis(a, 2, 0)).astype(np.float64)


def philox4x32_10(counter, key):
    """the four output words of Philox4x32-10 (Salmon et al., Random123)"""
    c = [int(v) & MASK for v in counter]
    k = [int(v) & MASK for v in key]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return tuple(c)


def noise_plane(h, w, key):
    """z float64 [h, w]: z(p) = sqrt(-2 ln u1) cos(2 pi u2), u1 = ((r0 >> 9) + 0.5) 2^-23, u2 = (r1 >> 8) 2^-24 from
    the counter (p, 0, 0, 0), p = y * w + x"""
    z = np.empty(h * w, np.float64)
    for p in range(h * w):
        r = philox4x32_10((p, 0, 0, 0), key)
        u1 = ((r[0] >> 9) + 0.5) * 2.0 ** -23
        u2 = (r[1] >> 8) * 2.0 ** -24
        z[p] = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
    return z.reshape(h, w)
