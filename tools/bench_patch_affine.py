"""Time of the augmented patch launch next to the plain crop it replaces (profiles/patch_affine.txt): gs_patch_affine_clip_minmax
through a 30 degrees x 1.1 matrix and gs_patch_clip_minmax, both for the HX4 patch (32, 128, 128) with C = 2 int16 volumes of a
resident (128, 256, 256) case and its body mask. The plain crop is the yardstick; the ratio is reported, nothing is gated.

Each measurement is a child process of its own under its own time limit (10 warm-up launches, then 100 launches between HIP
events: one pair per launch for the median, one pair round a second window of 100 back-to-back launches for the mean), the
two kernels alternating over the rounds so that a drift of the machine shows as spread between rounds and not as a
difference between kernels. The first child that fails ends the run.

    python tools/bench_patch_affine.py [--rounds 3] [--out profiles/patch_affine.txt]
    python tools/bench_patch_affine.py --step affine        # one measurement, one JSON line
"""
import argparse
import json
import math
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPE, PATCH, C_MOD = (128, 256, 256), (32, 128, 128), 2
WARMUP, LAUNCHES = 10, 100
STEP_LIMIT_S = 180


def matrix():
    th = math.radians(30.0)
    return [1.1, 0.0, 0.0, 0.0, 1.1 * math.cos(th), -1.1 * math.sin(th), 0.0, 1.1 * math.sin(th), 1.1 * math.cos(th)]


def step(kind):
    import numpy as np
    import torch
    from ganslate_amd.hip.ops import HipOps
    if not torch.cuda.is_available():
        raise SystemExit("bench_patch_affine: no GPU; a timing needs the MI355X")
    ops = HipOps()
    dev = ops.device
    rng = np.random.default_rng(0)
    g = np.meshgrid(*[(np.arange(s) - (s - 1) / 2) / (0.46 * s) for s in SHAPE], indexing="ij")
    mask = torch.from_numpy(((g[0] ** 2 + g[1] ** 2 + g[2] ** 2 <= 1.0) & (rng.random(SHAPE) > 0.08)).astype(np.uint8)).to(dev)
    vols = [torch.from_numpy(rng.integers(-1100, 2200, size=SHAPE).astype(np.int16)).to(dev) for _ in range(C_MOD)]
    point = torch.tensor([s // 2 for s in SHAPE] + [0], dtype=torch.int32, device=dev)
    out = torch.empty((C_MOD, *PATCH), dtype=torch.float32, device=dev)
    cols = ([-1024.0] * C_MOD, [1.0] * C_MOD, [-1000.0] * C_MOD, [2000.0] * C_MOD)
    M = matrix()
    if kind == "plain":
        fn = lambda: ops.patch_clip_minmax(vols, mask, point, PATCH, *cols, out)
    else:
        fn = lambda: ops.patch_affine_clip_minmax(vols, mask, point, PATCH, M, *cols, out)
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(LAUNCHES)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    each = [a.elapsed_time(b) * 1e3 for a, b in pairs]                       # microseconds
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    print(json.dumps({"kind": kind, "median_us": statistics.median(each), "min_us": min(each),
                      "window_mean_us": a.elapsed_time(b) * 1e3 / LAUNCHES}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["plain", "affine"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "patch_affine.txt"))
    args = ap.parse_args()
    if args.step:
        step(args.step)
        return
    rows = {"plain": [], "affine": []}
    for r in range(args.rounds):
        for kind in ("plain", "affine"):
            done = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--step", kind], capture_output=True, text=True,
                                  timeout=STEP_LIMIT_S, cwd=str(ROOT))
            if done.returncode != 0:                   # nothing more is started on the device after a failure
                raise SystemExit(f"round {r} step {kind} ended with status {done.returncode}:\n{done.stdout}\n{done.stderr}")
            rows[kind].append(json.loads(done.stdout.strip().splitlines()[-1]))
            print(rows[kind][-1], flush=True)
    out_bytes = C_MOD * PATCH[0] * PATCH[1] * PATCH[2] * 4
    med = {k: statistics.median(r["median_us"] for r in v) for k, v in rows.items()}
    win = {k: statistics.median(r["window_mean_us"] for r in v) for k, v in rows.items()}
    lines = [
        "tools/bench_patch_affine.py on one MI355X",
        f"Resident {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]} case: {C_MOD} int16 volumes and a uint8 body mask; patch "
        f"({PATCH[0]}, {PATCH[1]}, {PATCH[2]}) around the centre, C = {C_MOD}: {out_bytes / 1e6:.2f} MB of fp32 output per launch.",
        f"Per measurement a process of its own: {WARMUP} warm-up launches, {LAUNCHES} launches with a HIP event pair each (median),",
        f"then {LAUNCHES} back-to-back launches between one event pair (window mean, launch gaps included). {args.rounds} rounds, the two",
        "kernels alternating; the figures below are medians over the rounds, the per-round values follow.",
        "The matrix is a 30 degree rotation about the depth axis times a source step of 1.1.",
        "",
    ]
    for kind, name in (("plain", "gs_patch_clip_minmax (plain crop)"), ("affine", "gs_patch_affine_clip_minmax (30 deg x 1.1)")):
        lines.append(f"{name:46s} median {med[kind]:8.1f} us  {out_bytes / med[kind] / 1e3:7.1f} GB/s of output   "
                     f"window mean {win[kind]:8.1f} us  {out_bytes / win[kind] / 1e3:7.1f} GB/s")
    lines.append(f"ratio affine / plain: {med['affine'] / med['plain']:.2f} (median per launch), "
                 f"{win['affine'] / win['plain']:.2f} (window mean). Reported, not gated.")
    lines.append("")
    for kind in ("plain", "affine"):
        for r, row in enumerate(rows[kind]):
            lines.append(f"round {r} {kind:6s} median {row['median_us']:8.1f} us  min {row['min_us']:8.1f} us  "
                         f"window mean {row['window_mean_us']:8.1f} us")
    lines.append("Not measured: kernel times from a profiler trace, achieved HBM read bandwidth, and a blockIdx.y = modality mapping "
                 "of the gather (not built).")
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
