#!/usr/bin/env python
"""Time of one logged image grid on the GPU (run on the GPU box): HipOps.visuals_grid against the reference's torch op
sequence (tests/visgrid_ref.py, here on the same device tensors) for six 128^3 single-channel visuals with all slices
stacked — the visuals of a 3-D CycleGAN step. Device events around `--iters` back-to-back calls, the two alternating over
`--rounds` rounds after a warm-up; the outputs are compared byte for byte first.

    python tools/visgrid_bench.py [--size 128] [--visuals 6] [--out profiles/visgrid_bench.json]

Bytes per call of the kernel, from the shapes: K * D * H * W * 4 read, K * D * H * W * 3 written."""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from ganslate_amd.hip.ops import HipOps  # noqa: E402


def torch_grid(visuals):
    """process_visuals_for_logging + torchvision.utils.save_image up to the uint8 HWC tensor, for N == 1, C == 1"""
    grid = torch.cat(tuple(visuals.values()), dim=4)[0]
    grid = grid.permute(1, 0, 2, 3)
    grid = torch.cat(tuple(grid), dim=1)
    grid = (grid + 1) / 2
    grid = torch.cat((grid, grid, grid), 0)                     # make_grid: a gray image becomes three channels
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--visuals", type=int, default=6)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops = HipOps()
    g = torch.Generator().manual_seed(0)
    s = a.size
    visuals = {f"v{i}": (torch.rand((1, 1, s, s, s), generator=g) * 2 - 1).cuda() for i in range(a.visuals)}
    out = torch.empty((1, s * s, a.visuals * s, 3), dtype=torch.uint8, device="cuda")
    hip = lambda: ops.visuals_grid(visuals, out=out)            # noqa: E731
    ref = lambda: torch_grid(visuals)                           # noqa: E731
    hip()
    same = bool(torch.equal(out[0], ref()))
    for _ in range(10):
        hip(), ref()
    torch.cuda.synchronize()
    t_hip, t_ref = [], []
    for _ in range(a.rounds):
        t_hip.append(timed(hip, a.iters))
        t_ref.append(timed(ref, a.iters))
    elems = a.visuals * s ** 3
    best = min(t_hip)
    result = {"workload": f"{a.visuals} visuals of 1x1x{s}x{s}x{s} fp32, all slices stacked", "outputs_equal": same,
              "iters_per_round": a.iters, "hip_ms_per_call": [round(t, 4) for t in t_hip],
              "torch_ms_per_call": [round(t, 4) for t in t_ref], "hip_ms_min": round(best, 4),
              "torch_ms_min": round(min(t_ref), 4), "torch_over_hip": round(min(t_ref) / best, 2),
              "bytes_read": elems * 4, "bytes_written": elems * 3,
              "hip_achieved_GBps": round(elems * 7 / (best * 1e-3) / 1e9, 1), "timer": "device events",
              "device": torch.cuda.get_device_name(0)}
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
