"""Patch-wise (sliding-window) inference — ganslate/utils/sliding_window_inferer.py:8-52 without MONAI.

The reference subclasses `monai.inferers.SlidingWindowInferer` (third-party, unpinned, absent here); what that class
does is restated from MONAI's published algorithm (monai/inferers/utils.py `sliding_window_inference`,
monai/data/utils.py `dense_patch_slices` / `compute_importance_map`, MONAI 0.5-0.8):

  1. an image smaller than the window is padded symmetrically (half before, rest after) with `cval`;
  2. window starts per axis: interval = roi if roi == size else max(int(roi * (1 - overlap)), 1);
     count = ceil((size - roi) / interval) + 1; start_k = min(k * interval, size - roi); windows in row-major order;
  3. importance map: ones ("constant") or a Gaussian ("gaussian": separable erf-integrated kernel with
     sigma = 0.125 * roi, centred at roi // 2, normalised to max 1, floored at max(smallest non-zero value, 1e-3));
  4. windows are run `sw_batch_size` at a time; out[window] += map * prediction, count[window] += map;
  5. result = out / count, with the padding of step 1 cropped away.

The ganslate layer on top (kept verbatim in behaviour): a 2-D `roi_size` on a volume is broadcast to [1, H, W] and the
network then sees [N, C, H, W] slices (`network_wrapper`, sliding_window_inferer.py:36-52). The predictor is the HIP
generator's no-grad forward; windows of one batch go through it as ONE launch sequence (batch = sw_batch_size).

On the device the stitching around the predictor runs as three HIP kernels (csrc/slidewin.hip, `HipOps.sw_gather` /
`sw_accumulate` / `sw_finalize`): per chunk one gather (the padded input of step 1 is never built), the predictor, one
ordered blend into the accumulator; after the last chunk one normalising pass that recomputes `count` per voxel from the
window table instead of keeping it as a volume. Same roundings and summation order as the torch code below, which stays
as the CPU path and as the `device_kernels=False` comparison path."""
import math

import torch


def _gaussian_1d(sigma: float) -> torch.Tensor:
    """monai.networks.layers.gaussian_1d(sigma, truncated=4.0, approx='erf'), normalised"""
    tail = int(max(float(sigma) * 4.0, 0.5) + 0.5)
    x = torch.arange(-tail, tail + 1, dtype=torch.float32)
    t = 0.70710678 / abs(float(sigma))
    out = 0.5 * ((t * (x + 0.5)).erf() - (t * (x - 0.5)).erf())
    out = out.clamp(min=0)
    return out / out.sum()


def importance_map(roi, mode, device):
    if mode == "constant":
        return torch.ones(tuple(roi), dtype=torch.float32, device=device)
    if mode != "gaussian":
        raise ValueError(f"sliding window mode `{mode}` (expected `constant` or `gaussian`)")
    m = None
    for n in roi:
        # a delta at n // 2 filtered with the (zero-padded) kernel = the kernel centred there, cropped to the axis
        k = _gaussian_1d(0.125 * n)
        tail = (k.numel() - 1) // 2
        axis = torch.zeros(n)
        for i in range(n):
            j = i - n // 2 + tail
            if 0 <= j < k.numel():
                axis[i] = k[j]
        m = axis if m is None else m[..., None] * axis
    m = m / m.max()
    floor = max(m[m != 0].min().item(), 1e-3)
    return m.clamp(min=floor).to(device)


def window_starts(size, roi, overlap):
    starts = []
    for s, r in zip(size, roi):
        interval = r if r == s else max(int(r * (1 - overlap)), 1)
        num = int(math.ceil(float(s - r) / interval)) + 1 if interval > 0 else 1
        starts.append([min(k * interval, s - r) for k in range(num)])
    out = [[]]
    for axis in starts:                      # row-major product
        out = [p + [v] for p in out for v in axis]
    return out


def window_table(size, roi, overlap, batch):
    """The windows of one call as an int32 [n, 4] tensor of (batch item, z, y, x), in the order the inferer visits them
    (start-major, batch item inner). `size` is the padded size, max(image, roi) per axis; an image (two axes) gets z = 0."""
    starts = window_starts(size, roi, overlap)
    rows = [[b] + [0] * (3 - len(st)) + st for st in starts for b in range(batch)]
    return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 4)


class SlidingWindowInferer:

    def __init__(self, roi_size, sw_batch_size=1, overlap=0.25, mode="constant", cval=0.0, device_kernels=None):
        """device_kernels: None = the HIP kernels for fp32 device tensors, the torch code otherwise; False = always the torch
        code; True = the kernels or an error (there is no CPU form of them)."""
        self.roi_size = list(roi_size)
        self.sw_batch_size, self.overlap, self.mode, self.cval = int(sw_batch_size), float(overlap), mode, float(cval)
        self.device_kernels = device_kernels
        self._imaps = {}                         # (roi, mode, device) -> importance map
        if not 0 <= self.overlap < 1:
            raise ValueError("overlap must be >= 0 and < 1.")

    def __call__(self, inputs, network, *args, **kwargs):
        if len(self.roi_size) != len(inputs.shape[2:]):
            if len(self.roi_size) == 2:          # 2-D model over a volume: slice-wise windows
                self.roi_size = [1, *self.roi_size]
            else:
                raise RuntimeError("Unsupported roi size, cannot broadcast to volume. ")
        return self._infer(inputs, lambda x: self.network_wrapper(network, x, *args, **kwargs))

    def network_wrapper(self, network, x, *args, **kwargs):
        if len(self.roi_size) == 3 and self.roi_size[0] == 1:
            return network(x.squeeze(dim=2), *args, **kwargs).unsqueeze(dim=2)
        return network(x, *args, **kwargs)

    def _use_kernels(self, inputs):
        if self.device_kernels is False:
            return False
        fits = inputs.is_cuda and inputs.dtype == torch.float32 and inputs.dim() in (4, 5)
        if self.device_kernels and not fits:
            raise RuntimeError(f"device_kernels=True needs an fp32 image or volume batch on the GPU (got {inputs.dtype} "
                               f"{tuple(inputs.shape)} on {inputs.device}); the kernels have no CPU form")
        if not fits:
            return False
        from ..nn.native.backend import get_ops
        loaded = hasattr(get_ops(), "sw_gather")         # the HIP backend (a missing library raises in get_ops)
        if self.device_kernels and not loaded:
            raise RuntimeError("device_kernels=True, but the active backend is not the HIP library")
        return loaded

    def _importance_map(self, roi, device):
        key = (tuple(roi), self.mode, str(device))
        if key not in self._imaps:
            self._imaps[key] = importance_map(roi, self.mode, device)
        return self._imaps[key]

    def _infer(self, inputs, predictor):
        if self._use_kernels(inputs):
            return self._infer_device(inputs, predictor)
        return self._infer_torch(inputs, predictor)

    def _infer_device(self, inputs, predictor):
        """gather -> predictor -> accumulate per chunk, then finalize: what _infer_torch computes, bit for bit"""
        from ..nn.native.backend import get_ops
        ops = get_ops()
        nd = inputs.dim() - 2
        size0 = list(inputs.shape[2:])
        roi = [r if r > 0 else s for r, s in zip(self.roi_size, size0)]          # fall_back_tuple
        size = [max(s, r) for s, r in zip(size0, roi)]
        pad3 = [0] * (3 - nd) + [(p - s) // 2 for p, s in zip(size, size0)]
        roi3, size3 = [1] * (3 - nd) + roi, [1] * (3 - nd) + size
        B = inputs.shape[0]
        x = inputs.detach().contiguous()
        x = x if nd == 3 else x.unsqueeze(2)
        table_host = window_table(size, roi, self.overlap, B)
        table = table_host.to(x.device)                                          # uploaded once per call
        imap = self._importance_map(roi, x.device).reshape(roi3)
        acc = None
        for g0 in range(0, table.shape[0], self.sw_batch_size):
            rows, rows_host = table[g0:g0 + self.sw_batch_size], table_host[g0:g0 + self.sw_batch_size]
            win = ops.sw_gather(x, rows, roi3, pad3, self.cval)
            pred = predictor(win if nd == 3 else win.squeeze(2)).float().contiguous()
            if pred.dim() != nd + 2 or pred.shape[0] != win.shape[0] or list(pred.shape[2:]) != roi:
                raise ValueError(f"the predictor returned {tuple(pred.shape)} for windows {tuple(win.shape)}")
            pred = pred if nd == 3 else pred.unsqueeze(2)
            if acc is None:
                acc = ops.zero_fill(torch.empty((B, pred.shape[1], *size3), dtype=torch.float32, device=x.device))
            ops.sw_accumulate(acc, pred, imap, rows, rows_host)
            del win, pred                        # the chunk's buffers go back before the next gather / the result
        out = ops.sw_finalize(acc, imap, table, [1] * (3 - nd) + size0, pad3)
        return out if nd == 3 else out.squeeze(2)

    def _infer_torch(self, inputs, predictor):
        nd = inputs.dim() - 2
        size0 = list(inputs.shape[2:])
        roi = [r if r > 0 else s for r, s in zip(self.roi_size, size0)]          # fall_back_tuple
        pad = []
        for k in range(nd - 1, -1, -1):                                          # F.pad order: last axis first
            diff = max(roi[k] - size0[k], 0)
            pad.extend([diff // 2, diff - diff // 2])
        if any(pad):
            inputs = torch.nn.functional.pad(inputs, pad, mode="constant", value=self.cval)
        size = list(inputs.shape[2:])
        starts = window_starts(size, roi, self.overlap)
        imap = importance_map(roi, self.mode, inputs.device)
        B = inputs.shape[0]
        windows = [(b, st) for st in starts for b in range(B)]                   # MONAI: slice_g -> (window, batch item)
        out = count = None
        for g0 in range(0, len(windows), self.sw_batch_size):
            chunk = windows[g0:g0 + self.sw_batch_size]
            sl = [(slice(b, b + 1), slice(None)) + tuple(slice(s, s + r) for s, r in zip(st, roi)) for b, st in chunk]
            pred = predictor(torch.cat([inputs[s] for s in sl], dim=0)).float()
            if out is None:
                out = torch.zeros((B, pred.shape[1], *size), dtype=torch.float32, device=inputs.device)
                count = torch.zeros((B, pred.shape[1], *size), dtype=torch.float32, device=inputs.device)
            for i, s in enumerate(sl):
                out[s] += imap * pred[i:i + 1]
                count[s] += imap
        out = out / count
        crop = [slice(None), slice(None)]
        for k in range(nd):
            before = pad[2 * (nd - 1 - k)] if pad else 0
            crop.append(slice(before, before + size0[k]))
        return out[tuple(crop)]
