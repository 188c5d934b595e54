#!/usr/bin/env python
"""Time of one sliding-window inference call (utils/sliding_window_inferer.py) with the stitching as torch code
(`device_kernels=False`, the baseline) and as HIP kernels (`device_kernels=True`, csrc/slidewin.hip), in one process:
    python tools/sw_infer_time.py [--iters 20] [--net-iters 5] [--out FILE]
Shape: the brats validation volume 1x1x155x240x240, window 32x176x176, overlap 0.25, gaussian, window batch 2.
Reading 1: identity predictor (the stitching alone). Reading 2: the brats Vnet3D generator as predictor (the call a
Validator makes). Every call sits between its own pair of HIP events; the two paths alternate call by call after a warm-up
of each, and min / median / max over the calls are reported, the spread of the baseline being the run's noise margin.
Also reported, per path: peak device memory above the input (torch's allocator), what is launched per chunk (library
calls of the kernel path, counted at the ctypes boundary; aten operators of the torch path that compute — views and
metadata operators excluded — counted with a dispatch mode in a call of their own, outside the timed ones), and whether the
two paths return the same bits. No profiler and no counters are involved."""
import argparse
import sys
from collections import Counter
from pathlib import Path

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from ganslate_amd.nn.native.backend import get_ops  # noqa: E402
from ganslate_amd.utils.sliding_window_inferer import SlidingWindowInferer, window_table  # noqa: E402

SHAPE, ROI, OVERLAP, MODE, SW = (1, 1, 155, 240, 240), (32, 176, 176), 0.25, "gaussian", 2
VIEWS = {"slice", "select", "view", "_unsafe_view", "expand", "unsqueeze", "squeeze", "alias", "detach", "t", "permute",
         "transpose", "as_strided", "empty", "empty_like", "empty_strided", "_local_scalar_dense", "reshape", "unbind",
         "lift_fresh", "is_same_size", "sym_size", "sym_stride", "sym_numel", "new_empty"}


class AtenCounter(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = Counter()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func.overloadpacket.__name__
        flat = list(args) + list((kwargs or {}).values()) + [out]
        flat = [t for a in flat for t in (a if isinstance(a, (list, tuple)) else [a])]
        if name not in VIEWS and any(isinstance(t, torch.Tensor) and t.is_cuda for t in flat):      # device work only
            self.ops[name] += 1
        return out


class LibCounter:
    """counts calls of the library's entry points while active"""

    def __init__(self, lib, names):
        self.lib, self.names, self.calls, self._saved = lib, names, Counter(), {}

    def __enter__(self):
        for n in self.names:
            fn = getattr(self.lib, n)
            self._saved[n] = fn

            def counted(*a, _fn=fn, _n=n):
                self.calls[_n] += 1
                return _fn(*a)
            setattr(self.lib, n, counted)
        return self

    def __exit__(self, *exc):
        for n, fn in self._saved.items():
            setattr(self.lib, n, fn)


def timed(fns, iters):
    """{label: sorted ms per call}; the labelled calls alternate, each between its own HIP events"""
    pairs = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
             for k in fns}
    torch.cuda.synchronize()
    for i in range(iters):
        for k, fn in fns.items():
            e0, e1 = pairs[k][i]
            e0.record()
            fn()
            e1.record()
    torch.cuda.synchronize()
    return {k: sorted(e0.elapsed_time(e1) for e0, e1 in pairs[k]) for k in fns}


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def reading(title, x, predictor, iters, say):
    infs = {"torch path (device_kernels=False)": SlidingWindowInferer(ROI, SW, OVERLAP, MODE, cval=-1, device_kernels=False),
            "HIP kernels (device_kernels=True)": SlidingWindowInferer(ROI, SW, OVERLAP, MODE, cval=-1, device_kernels=True)}
    fns = {k: (lambda inf=inf: inf(x, predictor)) for k, inf in infs.items()}
    outs = {k: fn() for k, fn in fns.items()}                  # warm-up of every shape either path uses
    for fn in fns.values():
        fn()
    a, b = outs.values()
    same = torch.equal(a, b)
    say(f"\n== {title} ==")
    say(f"outputs of the two paths: {'bitwise equal' if same else f'DIFFERENT, max |diff| {(a - b).abs().max().item():.3e}'}")
    del outs, a, b
    ms = timed(fns, iters)
    for k, v in ms.items():
        say(f"{k:36s} min {v[0]:9.3f} ms | median {v[len(v) // 2]:9.3f} ms | max {v[-1]:9.3f} ms   ({iters} calls)")
    (base, new) = ms.values()
    spread = base[-1] - base[0]
    diff = base[len(base) // 2] - new[len(new) // 2]
    say(f"median difference (torch - kernels) {diff:+.3f} ms = {diff / base[len(base) // 2] * 100:+.1f} % of the torch path; "
        f"noise margin (torch path max - min) {spread:.3f} ms")
    for k, fn in fns.items():
        say(f"{k:36s} peak device memory above the input {peak_bytes(fn) / 2 ** 20:9.1f} MiB")
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--net-iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sw_infer_time.py measures on the GPU; no GPU is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ops = get_ops()
    x = (torch.rand(SHAPE, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(ops.device)
    n_windows = window_table(list(SHAPE[2:]), list(ROI), OVERLAP, SHAPE[0]).shape[0]
    chunks = -(-n_windows // SW)
    say(f"device: {torch.cuda.get_device_name()}; volume {'x'.join(map(str, SHAPE))}, window {'x'.join(map(str, ROI))}, "
        f"overlap {OVERLAP}, {MODE}, window batch {SW}: {n_windows} windows in {chunks} chunks; "
        f"one output volume = {x.numel() * 4 / 2 ** 20:.1f} MiB")

    fns = reading("identity predictor: the stitching alone", x, lambda w: w, args.iters, say)

    # what each path launches (identity predictor, one call each, outside the timed ones)
    torch_fn, hip_fn = fns.values()
    with AtenCounter() as c:
        torch_fn()
    total = sum(c.ops.values())
    say(f"\ntorch path: {total} computing aten operators per call = {total / chunks:.1f} per chunk "
        f"({', '.join(f'{k} {v}' for k, v in sorted(c.ops.items()))})")
    names = ("gs_sw_gather", "gs_sw_accumulate", "gs_sw_finalize", "gs_zero_bytes")
    with LibCounter(ops.lib, names) as lc, AtenCounter() as c:
        hip_fn()
    per_chunk = (lc.calls["gs_sw_gather"] + lc.calls["gs_sw_accumulate"]) / chunks
    say(f"HIP kernels: {dict(lc.calls)} library calls per call (one launch each) = {per_chunk:.1f} per chunk + "
        f"{lc.calls['gs_zero_bytes'] + lc.calls['gs_sw_finalize']} per call; computing aten operators left: "
        f"{dict(c.ops) or 'none'} (_to_copy / copy_: the table upload)")

    from ganslate_amd.nn.generators import Vnet3D
    torch.manual_seed(0)
    net = Vnet3D(1, 1, "instance", 16, (2, 2, 3), (3, 3, 3), use_memory_saving=False, use_inverse=False)
    net.eval()

    def generator(w):
        with torch.no_grad():
            return net(w)
    reading("Vnet3D generator (brats blocks 16, (2, 2, 3), (3, 3, 3)) as predictor", x, generator, args.net_iters, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
