#!/usr/bin/env python
"""Timing of the device validation / test metrics (valmetrics.hip via HipOps.valmetrics) with every metric enabled,
at a 2-D batch (8x3x256x256) and a brats-sized volume (1x1x155x240x240), next to the float64 host restatement
(tests/valmetrics_ref.py) run on a pool of 16 threads (one task per sample and metric):
    python tools/bench_valmetrics.py [--iters 50] [--host-reps 1]
Device times are HIP events around `iters` calls on the current stream after a warm-up; the HBM floor counts the
three passes that read t and p (moments, SSIM, histograms) at the 8.0 TB/s peak.

    python tools/bench_valmetrics.py --masks L [--iters 50]
times instead, per shape and with one HIP event pair per call (min / median / max over the iterations): the unmasked
call, HipOps.valmetrics_masked with L masks (a box, then random 40 % masks), and the route without the masked kernels:
L unmasked calls on t*m and p*m multiplied by torch. The spread of the unmasked figure is the run's noise margin."""
import argparse
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from ganslate_amd.hip.ops import HipOps  # noqa: E402
from tests import valmetrics_ref as ref  # noqa: E402

SHAPES = [(8, 3, 256, 256), (1, 1, 155, 240, 240)]
HBM_PEAK = 8.0e12


def device_us(ops, t, p, iters, **flags):
    for _ in range(3):
        ops.valmetrics(t, p, **flags)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        ops.valmetrics(t, p, **flags)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def per_call_us(fn, iters):
    """(min, median, max) in us of `iters` calls, each between its own pair of HIP events"""
    for _ in range(3):
        fn()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs)
    return us[0], us[len(us) // 2], us[-1]


def bench_masks(ops, shape, n_masks, iters, rng):
    t = rng.uniform(-1000, 3000, shape).astype(np.float32)
    p = (t + rng.normal(0, 60, shape)).astype(np.float32)
    td, pd = torch.from_numpy(t).to(ops.device), torch.from_numpy(p).to(ops.device)
    box = np.zeros(shape, dtype=bool)
    box[(slice(None), slice(None)) + tuple(slice(s // 4, 3 * s // 4) for s in shape[2:])] = True
    masks = [torch.from_numpy(m).to(ops.device) for m in [box] + [rng.random(shape) < 0.4 for _ in range(n_masks - 1)]]

    def torch_route():
        return [ops.valmetrics(td * m, pd * m) for m in masks]

    name = "x".join(map(str, shape))
    rows = [("unmasked call", lambda: ops.valmetrics(td, pd)),
            (f"masked call, L = {n_masks}", lambda: ops.valmetrics_masked(td, pd, masks)),
            (f"{n_masks} unmasked calls on torch's t*m, p*m", torch_route)]
    out = {}
    for label, fn in rows:
        out[label] = per_call_us(fn, iters)
        lo, med, hi = out[label]
        print(f"{name}: {label:42s} min {lo:8.1f} us | median {med:8.1f} us | max {hi:8.1f} us")
    (ulo, _, uhi), (_, mmed, _), (_, tmed, _) = out.values()
    print(f"{name}: masked / torch route (medians) = {mmed / tmed:.2f}; noise margin (unmasked max - min) "
          f"{uhi - ulo:.1f} us; difference {tmed - mmed:+.1f} us")


def host_s(t, p, reps):
    tasks = [(i, k) for i in range(t.shape[0]) for k in ref.COLUMNS]
    best = float("inf")
    with ThreadPoolExecutor(16) as pool:
        for _ in range(reps):
            t0 = time.perf_counter()
            list(pool.map(lambda ik: ref.FNS[ik[1]](t[ik[0]], p[ik[0]]), tasks))
            best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--masks", type=int, default=0, metavar="L",
                    help="time the masked call with L masks beside the unmasked one and the torch route")
    args = ap.parse_args()
    ops = HipOps()
    rng = np.random.default_rng(0)
    print(f"device: {torch.cuda.get_device_name()}  iters={args.iters}")
    if args.masks:
        for shape in SHAPES:
            bench_masks(ops, shape, args.masks, args.iters, rng)
        return
    for shape in SHAPES:
        t = rng.uniform(-1000, 3000, shape).astype(np.float32)
        p = (t + rng.normal(0, 60, shape)).astype(np.float32)
        td, pd = torch.from_numpy(t).to(ops.device), torch.from_numpy(p).to(ops.device)
        full = device_us(ops, td, pd, args.iters)
        scal = device_us(ops, td, pd, args.iters, ssim=False, hist=False)
        ssim = device_us(ops, td, pd, args.iters, hist=False)
        floor = 3 * 2 * t.nbytes / HBM_PEAK * 1e6
        name = "x".join(map(str, shape))
        print(f"{name}: device all metrics {full:9.1f} us | scalars only {scal:8.1f} us | + ssim {ssim:8.1f} us | "
              f"3-pass HBM floor {floor:6.1f} us ({full / floor:4.1f}x)")
        if not args.no_host:
            hs = host_s(t, p, args.host_reps)
            print(f"{name}: host float64 restatement, 16 threads {hs * 1e3:9.1f} ms ({hs * 1e6 / full:7.0f}x device)")


if __name__ == "__main__":
    main()
