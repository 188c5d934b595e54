"""Time of the augmented patch launches next to the plain crop they replace (profiles/patch_elastic.txt; profiles/patch_affine.txt
is the run of this tool before the elastic launch existed): gs_patch_clip_minmax, gs_patch_affine_clip_minmax through a
30 degrees x 1.1 matrix, and gs_patch_elastic_clip_minmax through the same matrix behind a 7 x 7 x 7 lattice of random
displacements within 0.3 of the control spacing — in its row-shared form (the one launched) and, forced by the library option
elastic_rows = 0, in its per-voxel form — and gs_patch_augment_clip_minmax, the same elastic gather with the intensity chain
(bias field on a 4 x 4 x 4 lattice, contrast, brightness, gamma, noise) on both modalities, in both forms. All for the HX4 patch (32, 128, 128) with C = 2 int16 volumes of a resident
(128, 256, 256) case and its body mask. The plain crop is the yardstick; the ratios are reported, nothing is gated.

Each measurement is a child process of its own under its own time limit (10 warm-up launches, then 100 launches between HIP
events: one pair per launch for the median, one pair round a second window of 100 back-to-back launches for the mean), the
kernels alternating over the rounds so that a drift of the machine shows as spread between rounds and not as a
difference between kernels. The first child that fails ends the run.

    python tools/bench_patch_affine.py [--rounds 3] [--out profiles/patch_elastic.txt]
    python tools/bench_patch_affine.py --step affine        # one measurement, one JSON line
"""
import argparse
import json
import math
import re
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPE, PATCH, C_MOD = (128, 256, 256), (32, 128, 128), 2
WARMUP, LAUNCHES = 10, 100
STEP_LIMIT_S = 180
GRID, FRACTION = (7, 7, 7), 0.3
KINDS = (("plain", "gs_patch_clip_minmax (plain crop)"), ("affine", "gs_patch_affine_clip_minmax (30 deg x 1.1)"),
         ("elastic", "gs_patch_elastic_clip_minmax, row-shared"), ("elastic_voxel", "gs_patch_elastic_clip_minmax, per voxel"),
         ("augment", "gs_patch_augment_clip_minmax, row-shared"), ("augment_voxel", "gs_patch_augment_clip_minmax, per voxel"))
BIAS_GRID = (4, 4, 4)
INTENSITY = [(0.8, 1.2, -0.05, 0.03, 0.3, 5, 6), (1.3, 0.9, 0.05, 0.02, 0.3, 7, 8)]       # every step of the chain on


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
    elif kind == "affine":
        fn = lambda: ops.patch_affine_clip_minmax(vols, mask, point, PATCH, M, *cols, out)
    else:
        bound = np.array([FRACTION * (PATCH[a] - 1) / (GRID[a] - 3) for a in range(3)]).reshape(3, 1, 1, 1)
        field = torch.from_numpy((2.0 * rng.random((3, *GRID)) - 1.0) * bound).to(dev)
        if kind.endswith("_voxel"):
            ops.set_option("elastic_rows", 0)
        if kind.startswith("augment"):                  # the same field, plus bias field, contrast, gamma and noise
            beta = torch.from_numpy(2.0 * rng.random(BIAS_GRID) - 1.0).to(dev)
            fn = lambda: ops.patch_augment_clip_minmax(vols, mask, point, PATCH, M, field, INTENSITY, beta, *cols, out)
        else:
            fn = lambda: ops.patch_elastic_clip_minmax(vols, mask, point, PATCH, M, field, *cols, out)
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
    ap.add_argument("--step", choices=[k for k, _ in KINDS])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "patch_elastic.txt"))
    args = ap.parse_args()
    if args.step:
        step(args.step)
        return
    rows = {k: [] for k, _ in KINDS}
    for r in range(args.rounds):
        for kind, _ in KINDS:
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
        f"then {LAUNCHES} back-to-back launches between one event pair (window mean, launch gaps included). {args.rounds} rounds, the",
        "kernels alternating; the figures below are medians over the rounds, the per-round values follow.",
        "The matrix is a 30 degree rotation about the depth axis times a source step of 1.1; the elastic lattice has "
        f"{GRID[0]} x {GRID[1]} x {GRID[2]}",
        f"control points with random displacements within {FRACTION} of the control spacing. The per-voxel form of the elastic launch is",
        "forced with the library option elastic_rows = 0; the row-shared form is what this patch and lattice launch by themselves.",
        "",
    ]
    for kind, name in KINDS:
        lines.append(f"{name:46s} median {med[kind]:8.1f} us  {out_bytes / med[kind] / 1e3:7.1f} GB/s of output   "
                     f"window mean {win[kind]:8.1f} us  {out_bytes / win[kind] / 1e3:7.1f} GB/s")
    for kind in ("affine", "elastic", "elastic_voxel"):
        lines.append(f"ratio {kind} / plain: {med[kind] / med['plain']:.2f} (median per launch), "
                     f"{win[kind] / win['plain']:.2f} (window mean). Reported, not gated.")
    lines.append(f"ratio elastic / affine, this session: {med['elastic'] / med['affine']:.2f} (median per launch), "
                 f"{win['elastic'] / win['affine']:.2f} (window mean); per voxel / row-shared: "
                 f"{med['elastic_voxel'] / med['elastic']:.2f}, {win['elastic_voxel'] / win['elastic']:.2f}.")
    lines.append(f"ratio augment / elastic (the intensity chain on both modalities, a {BIAS_GRID[0]} x {BIAS_GRID[1]} x {BIAS_GRID[2]} bias "
                 f"lattice): {med['augment'] / med['elastic']:.2f} (median per launch), {win['augment'] / win['elastic']:.2f} (window mean); "
                 f"per voxel: {med['augment_voxel'] / med['elastic_voxel']:.2f}, {win['augment_voxel'] / win['elastic_voxel']:.2f}.")
    before = re.search(r"^gs_patch_affine_clip_minmax.*?median\s+([\d.]+) us.*?window mean\s+([\d.]+) us",
                       (ROOT / "profiles" / "patch_affine.txt").read_text(), flags=re.M)
    if before:
        b_med, b_win = float(before.group(1)), float(before.group(2))
        lines.append(f"Against the affine gather before the elastic variant existed (profiles/patch_affine.txt: {b_med} / {b_win} us): "
                     f"affine now {med['affine'] / b_med:.2f} / {win['affine'] / b_win:.2f}, elastic {med['elastic'] / b_med:.2f} / "
                     f"{win['elastic'] / b_win:.2f}.")
    lines.append("")
    for kind, _ in KINDS:
        for r, row in enumerate(rows[kind]):
            lines.append(f"round {r} {kind:13s} median {row['median_us']:8.1f} us  min {row['min_us']:8.1f} us  "
                         f"window mean {row['window_mean_us']:8.1f} us")
    lines.append("Not measured: kernel times from a profiler trace, achieved HBM read bandwidth, LDS bank conflicts of the row table, "
                 "other patch sizes and lattices (short rows, wide lattices), the upload of the fields, and the effect on a training "
                 "step (a 3-D step is about 50 ms; these launches are tens of microseconds per sample).")
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
