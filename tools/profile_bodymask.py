"""Times of the whole-case evaluation path on one synthetic CT-like case (profiles/bodymask_mi355x.txt): gs_body_mask and
gs_volume_prepare on the device (HIP events, median of a few runs after warm-up) next to the host utility get_body_mask on
the same volume. The case: an int16 ellipsoid body with an air cavity and a detached table slab at (96, 512, 512), padded
to (128, 512, 512).

    python tools/profile_bodymask.py [--shape 96 512 512] [--runs 5] [--no-host | --host-only]
"""
import argparse
import hashlib
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def synthetic_ct(shape, seed=0):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[(np.arange(s, dtype=np.float32) - (s - 1) / 2) / (0.5 * s) for s in shape], indexing="ij")
    body = (g[0] / 0.98) ** 2 + (g[1] / 0.55) ** 2 + (g[2] / 0.8) ** 2 <= 1.0
    cavity = (g[0] / 0.6) ** 2 + ((g[1] + 0.1) / 0.15) ** 2 + ((g[2] - 0.2) / 0.2) ** 2 <= 1.0       # a lung-like air pocket
    table = (g[1] > 0.7) & (g[1] < 0.76) & (np.abs(g[2]) < 0.9)                                        # below the body, detached
    ct = rng.integers(-1050, -850, size=shape).astype(np.int16)
    ct[body] = rng.integers(-150, 250, size=int(body.sum())).astype(np.int16)
    ct[cavity] = rng.integers(-1000, -800, size=int(cavity.sum())).astype(np.int16)
    ct[table] = 300
    return ct


def device_ms(fn, runs):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(96, 512, 512))
    ap.add_argument("--pad-to", type=int, nargs=3, default=(128, 512, 512))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-only", action="store_true", help="no GPU needed; the digests tell whether the masks agree")
    args = ap.parse_args()
    from ganslate_amd.data.utils.body_mask import get_body_mask
    shape = tuple(args.shape)
    ct = synthetic_ct(shape)
    if args.host_only:
        t0 = time.perf_counter()
        host = get_body_mask(ct, -300)
        print(f"host get_body_mask (numpy) on {shape}: {time.perf_counter() - t0:.2f} s; {int(host.sum())} voxels in the mask, "
              f"sha1 {hashlib.sha1(host.tobytes()).hexdigest()[:16]}")
        return
    from ganslate_amd.hip.ops import HipOps
    ops = HipOps()
    dev = torch.from_numpy(ct).to(ops.device)
    pet = torch.rand(shape, device=ops.device) * 6
    mask, info, rounds = ops.body_mask(dev, -300, return_rounds=True)
    print(f"case {shape} int16, padded to {tuple(args.pad_to)}; body mask: {int(info[0])} voxels in the component, "
          f"{int(mask.sum())} in the mask, sha1 {hashlib.sha1(mask.cpu().numpy().tobytes()).hexdigest()[:16]}")
    launches = 1 + 2 * 8 * sum(-(-r // 8) for r in rounds) + 7
    print(f"gs_body_mask: {device_ms(lambda: ops.body_mask(dev, -300), args.runs):.2f} ms (median of {args.runs}), rounds "
          f"{rounds[0]} (3-D) + {rounds[1]} (per slice), {launches} launches enqueued, "
          f"{sum(-(-r // 8) for r in rounds)} stream synchronisations")
    prep = lambda: ops.volume_prepare([pet, dev], mask, [mask], args.pad_to, [0.0, -1024.0], [1.0, 1.0], [0.0, -1000.0],
                                      [6.0, 2000.0])
    print(f"gs_volume_prepare (2 volumes, 2 masks): {device_ms(prep, args.runs):.2f} ms")
    if not args.no_host:
        t0 = time.perf_counter()
        host = get_body_mask(ct, -300)
        print(f"host get_body_mask (numpy): {time.perf_counter() - t0:.2f} s; equal to the device mask: "
              f"{bool(np.array_equal(host, mask.cpu().numpy()))}")


if __name__ == "__main__":
    main()
