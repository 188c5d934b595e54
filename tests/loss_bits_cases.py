"""The cases of the bit pin on csrc/loss.hip (tests/test_loss_bits_gpu.py, tools/gen_golden_loss_bits.py): every scalar result as
its uint32 bit pattern, every gradient array as the sha256 of its bytes, recorded once from the library of the commit named in
tests/golden/loss_bits.json. The float64 tests bound the error; these notice a changed summation order or a product that
moved into or out of an fma, which stay far inside those bounds.

Inputs are closed-form in numpy (no RNG of any library): x[i] = ((i * (2654435761 + 81006 * salt) + 1013904242 * salt) mod 2^32)
/ 2^31 - 1 as float32; the salt changes the multiplier too, so that two tensors of one case are not one sequence shifted.
Shapes are the smallest at which each structure of the file can go wrong:
  flat reductions   n = 1; 255 and 257 (partial wave, partial block); 256*8*3 + 5 (several workgroups, at most 8 elements per
                    thread); 1024*2048 + 77 (the cap of 1024 workgroups, the grid-stride loop wraps)
  nonsaturating     3 rows of 1, 257 and 1000 elements (one workgroup per row)
  window L1         (N, C, window, S): (3, 4, [1,3), 1000) ~7.3 elements per thread, step < per; (700, 3, [2,3), 7) step > per,
                    several samples end inside one stride; (2, 2, [0,1), 1100000) the workgroup cap with per > step
  SSIM              planes of 11x11 (one valid pixel), 12x11, 26x42 (exactly one tile), 27x43 (four tiles with one-pixel
                    remainders); 3 planes dense, windows [1,2) and [1,3) of a 4-channel x with N = 2; once y == x, where the
                    value and every gradient element are exactly 0
"""
import hashlib

import numpy as np

FLAT_N = (1, 255, 257, 256 * 8 * 3 + 5, 1024 * 2048 + 77)
FLAT_OPS = (("mse", None, None), ("lsgan", True, 1.0), ("lsgan", False, 0.0), ("vanilla", True, 1.0), ("vanilla", False, 0.0),
            ("wgangp", True, 0.0), ("wgangp", False, 0.0), ("l1", None, None))
ROWS, ROW_PER = 3, (1, 257, 1000)
WINDOW_L1 = ((3, 4, (1, 3), 1000), (700, 3, (2, 3), 7), (2, 2, (0, 1), 1100000))
SSIM_PLANES = ((11, 11), (12, 11), (26, 42), (27, 43))
SSIM_WINDOWS = ((1, 2), (1, 3))
GRAD_SCALE = 0.37
ROW_SCALES = (0.37, -1.25, 2.0)
ZERO_BITS = "00000000"
GROUPS = ("flat", "rows", "window_l1", "ssim")


def values(shape, salt):
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64)
    mult, add = np.uint64(2654435761 + 81006 * salt), np.uint64(1013904242 * salt)
    return (((i * mult + add) % np.uint64(2 ** 32)).astype(np.float64) / 2.0 ** 31 - 1.0).astype(np.float32).reshape(shape)


def bits(t):
    """the uint32 patterns of a small fp32 device tensor, hex, space-separated"""
    return " ".join(f"{int(v):08x}" for v in t.detach().cpu().contiguous().numpy().view(np.uint32).ravel())


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def zeros_digest(shape):
    return hashlib.sha256(np.zeros(shape, dtype=np.float32).tobytes()).hexdigest()


def _flat(ops, dev, out):
    import torch
    scale = torch.tensor(GRAD_SCALE, device=dev)
    for n in FLAT_N:
        x = torch.from_numpy(values((n,), 1)).to(dev)
        y = torch.from_numpy(values((n,), 2)).to(dev)
        m = torch.empty((), device=dev)
        ops.mean(x, m)
        out[f"flat/mean/n{n}/value"] = bits(m)
        for op, real, label in FLAT_OPS:
            name = f"flat/{op}" + ("" if real is None else "_real" if real else "_fake") + f"/n{n}"
            for tag, s in (("value", None), ("grad", None), ("grad_scaled", scale)):
                loss = torch.empty((), device=dev) if tag == "value" else None
                grad = torch.empty_like(x) if tag != "value" else None
                if op == "mse":
                    ops.mse_const(x, 1.0, loss=loss, grad=grad, grad_scale=s)
                elif op == "l1":
                    ops.l1(x, y, loss=loss, grad_a=grad, grad_scale=s)
                else:
                    ops.adv_loss(x, op, real, label, loss=loss, grad=grad, grad_scale=s)
                out[f"{name}/{tag}"] = bits(loss) if tag == "value" else digest(grad)


def _rows(ops, dev, out):
    import torch
    scales = torch.tensor(ROW_SCALES, device=dev)
    for per in ROW_PER:
        x = torch.from_numpy(values((ROWS, per), 3)).to(dev)
        for real in (True, False):
            name = f"rows/nonsaturating_{'real' if real else 'fake'}/per{per}"
            loss = torch.empty(ROWS, device=dev)
            ops.adv_loss(x, "nonsaturating", real, 0.0, loss=loss)
            out[f"{name}/value"] = bits(loss)
            for tag, s in (("grad", None), ("grad_scaled", scales)):
                grad = torch.empty_like(x)
                ops.adv_loss(x, "nonsaturating", real, 0.0, grad=grad, grad_scale=s)
                out[f"{name}/{tag}"] = digest(grad)


def _window_l1(ops, dev, out):
    import torch
    scale = torch.tensor(GRAD_SCALE, device=dev)
    for N, C, (c0, c1), S in WINDOW_L1:
        a = torch.from_numpy(values((N, C, 1, S), 4)).to(dev)
        b = torch.from_numpy(values((N, c1 - c0, 1, S), 5)).to(dev)
        name = f"window_l1/{N}x{C}x{S}_{c0}-{c1}"
        loss = torch.empty((), device=dev)
        ops.l1_window(a, c0, c1, b, loss=loss)
        out[f"{name}/value"] = bits(loss)
        for tag, s in (("grad_b", None), ("grad_b_scaled", scale)):
            grad = torch.empty_like(b)
            ops.l1_window(a, c0, c1, b, grad_b=grad, grad_scale=s)
            out[f"{name}/{tag}"] = digest(grad)


def _ssim_dense(ops, x, y, name, out):
    import torch
    scale = torch.tensor(GRAD_SCALE, device=x.device)
    val = torch.empty((), device=x.device)
    ops.ssim_distance(x, y, val)
    out[f"{name}/value"] = bits(val)
    for tag, s in (("", None), ("_scaled", scale)):
        gy, gx = torch.empty_like(y), torch.empty_like(x)
        ops.ssim_distance_backward(x, y, gy, grad_scale=s)
        ops.ssim_distance_backward(y, x, gx, grad_scale=s)                  # the distance is symmetric: d/dx
        out[f"{name}/grad_y{tag}"] = digest(gy)
        out[f"{name}/grad_x{tag}"] = digest(gx)


def _ssim_window(ops, x, c0, c1, y, name, out):
    import torch
    scale = torch.tensor(GRAD_SCALE, device=x.device)
    val = torch.empty((), device=x.device)
    ops.ssim_distance_window(x, c0, c1, y, val)
    out[f"{name}/value"] = bits(val)
    for tag, s in (("", None), ("_scaled", scale)):
        gy = torch.empty_like(y)
        ops.ssim_distance_window_backward(x, c0, c1, y, gy, grad_scale=s)
        out[f"{name}/grad_y{tag}"] = digest(gy)


def _ssim(ops, dev, out):
    import torch
    for H, W in SSIM_PLANES:
        x = torch.from_numpy(values((1, 3, H, W), 6)).to(dev)
        y = torch.from_numpy(values((1, 3, H, W), 7)).to(dev)
        _ssim_dense(ops, x, y, f"ssim/dense/{H}x{W}", out)
        xw = torch.from_numpy(values((2, 4, H, W), 8)).to(dev)
        for c0, c1 in SSIM_WINDOWS:
            yw = torch.from_numpy(values((2, c1 - c0, H, W), 9)).to(dev)
            _ssim_window(ops, xw, c0, c1, yw, f"ssim/window_{c0}-{c1}/{H}x{W}", out)
    H, W = SSIM_PLANES[-1]
    x = torch.from_numpy(values((1, 3, H, W), 6)).to(dev)
    _ssim_dense(ops, x, x.clone(), f"ssim/dense_identical/{H}x{W}", out)
    xw = torch.from_numpy(values((2, 4, H, W), 8)).to(dev)
    _ssim_window(ops, xw, 1, 3, xw[:, 1:3].contiguous(), f"ssim/window_identical_1-3/{H}x{W}", out)


RUNNERS = {"flat": _flat, "rows": _rows, "window_l1": _window_l1, "ssim": _ssim}


def run_group(ops, group):
    """{case name: bit pattern(s) or digest} of one group on the library behind `ops`"""
    out = {}
    RUNNERS[group](ops, ops.device, out)
    return out
