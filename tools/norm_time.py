#!/usr/bin/env python
"""Per-entry-point timings of the elementwise-norm kernels (csrc/norm.hip, norm_ex.hip, prelu.hip) at the workloads' shapes:

    GANSLATE_HIP_LIB=<library> python tools/norm_time.py > one.json            # one process: {entry: us per call}
    python tools/norm_time.py --merge A1.json B1.json A2.json B2.json A3.json B3.json > profiles/<name>_time.json

HIP events round 50 calls, median of 15 rounds. For an A/B of two builds run the first form once per library and round,
alternating A B A B A B, one process each; --merge lays the six files out like profiles/loss_refactor_time.json and lists the
entries whose B median is above A's by more than the spread (max - min) of A's own three medians."""
import argparse
import json
import statistics
import sys
from pathlib import Path

CALLS, ROUNDS = 50, 15


def merge(files):
    runs = [json.loads(Path(f).read_text()) for f in files]
    a_runs, b_runs = runs[0::2], runs[1::2]
    entries, worse = {}, []
    for name in a_runs[0]:
        a, b = [r[name] for r in a_runs], [r[name] for r in b_runs]
        am, bm = statistics.median(a), statistics.median(b)
        spread = max(a) - min(a)
        entries[name] = {"parent_us": a, "new_us": b, "parent_median": am, "new_median": bm,
                         "parent_spread": round(spread, 3), "new_minus_parent": round(bm - am, 3)}
        if bm - am > spread:
            worse.append(name)
    return {"timer": f"HIP events round {CALLS} calls, median of {ROUNDS} rounds per process, us per call",
            "order": "ABABAB", "A": "parent library", "B": "refactored library", "entries": entries,
            "worse_than_parent_by_more_than_its_spread": worse,
            "processes": "one process per library, alternating A B A B A B; parent_spread = max - min of A's three medians"}


def measure():
    import torch
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    from ganslate_amd.hip.ops import HipOps
    ops = HipOps()
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *s, dtype=torch.bfloat16: torch.randn(*s, generator=gen).to(dtype).cuda()
    out = {}

    def timed(name, fn):
        for _ in range(5):
            fn()
        rounds = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(ROUNDS):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            rounds.append(e0.elapsed_time(e1) / CALLS * 1e3)
        out[name] = round(statistics.median(rounds), 3)

    def stats(y):
        N, C = y.shape[0], y.shape[-1]
        f = y.float().reshape(N, -1, C)
        part = torch.stack([f.sum(1), (f * f).sum(1)], 1).reshape(-1).contiguous()
        mr = torch.zeros(N * 2 * C, device="cuda")
        ops.inorm_finalize(part, N, 1, C, f.shape[1], mr)
        return mr

    # norm.hip: what tools/bench_norm.py runs — the residual-block shape (N 8, 64 x 64, C 256) and its --vol 32 cases
    N, H, W, C = 8, 64, 64, 256
    y, x, res, g0, g2, dy, gsum = (rnd(N, H, W, C) for _ in range(7))
    gpad = rnd(N, H + 2, W + 2, C)
    mr = stats(y)
    part = rnd(N * 16 * 2 * C, dtype=torch.float32).abs()
    mr2 = torch.zeros_like(mr)
    timed("norm/inorm_finalize", lambda: ops.inorm_finalize(part, N, 16, C, H * W, mr2))
    timed("norm/fwd act", lambda: ops.inorm_act_forward(y, mr, None, x, act="relu"))
    timed("norm/fwd act+res", lambda: ops.inorm_act_forward(y, mr, res, x, act="none"))
    timed("norm/stats fwd act", lambda: ops.inorm_stats_act_forward(y, part, 16, mr2, None, x, act="relu"))
    timed("norm/bwd fold1", lambda: ops.inorm_act_backward(gpad, None, y, mr, dy, None, fold=1, act="relu"))
    timed("norm/bwd fold1+g2+gsum", lambda: ops.inorm_act_backward(gpad, g2, y, mr, dy, gsum, fold=1, act="none"))
    timed("norm/bwd nofold", lambda: ops.inorm_act_backward(g0, None, y, mr, dy, None, fold=0, act="relu"))
    V = 32
    y, dy, g0, gpad = rnd(1, V, V, V, C), rnd(1, V, V, V, C), rnd(1, V, V, V, C), rnd(1, V + 2, V + 2, V + 2, C)
    mr = stats(y)
    timed("norm/3d bwd replicate fold", lambda: ops.inorm_act_backward(gpad, None, y, mr, dy, None, fold=1,
                                                                     fold_mode="replicate", act="relu"))
    timed("norm/3d bwd nofold", lambda: ops.inorm_act_backward(g0, None, y, mr, dy, None, fold=0, act="relu"))

    # norm_ex.hip: an outer and an inner level of the pix2pix U-Net (256 x 512 input, ngf 128): both activations, channel slices
    for tag, (H, W, C), drop in (("outer", (64, 128, 256), 0.0), ("inner", (2, 4, 1024), 0.5)):
        y, g1, g2 = rnd(1, H, W, C), rnd(1, H, W, C), rnd(1, H, W, 2 * C)
        x1, x2, dy = torch.zeros_like(y), torch.zeros(1, H, W, 2 * C, dtype=torch.bfloat16, device="cuda"), torch.zeros_like(y)
        mr, db = stats(y), torch.zeros(C, device="cuda")
        timed(f"norm_ex/{tag} fwd", lambda: ops.norm_act_forward_ex(y, mr, x1, x2, act1="lrelu", act2="relu", x2_co=C,
                                                                   drop_p=drop, seed=5))
        timed(f"norm_ex/{tag} bwd", lambda: ops.norm_act_backward_ex(g1, g2, y, mr, dy, act1="lrelu", act2="relu", g2_co=C,
                                                                    drop_p=drop, seed=5, bias_grad=db))

    # prelu.hip: the 16-channel full-resolution level and the 128-channel coarse level of the brats V-Net (128^3 patches)
    for tag, sp, C in (("16ch full", (128, 128, 128), 16), ("128ch coarse", (16, 16, 16), 128)):
        y, g, res = rnd(1, *sp, C), rnd(1, *sp, C), rnd(1, *sp, C)
        o, dy = torch.zeros_like(y), torch.zeros_like(y)
        mr, slope = stats(y), torch.full((C,), 0.25, device="cuda")
        dslope, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        timed(f"prelu/{tag} fwd", lambda: ops.pnorm_forward(y, mr, o, C=C, slope=slope, res=res, res_mode=2))
        timed(f"prelu/{tag} bwd+dslope", lambda: ops.pnorm_backward(g, y, mr, dy, C=C, slope=slope, dslope=dslope, res=res,
                                                                   res_mode=2, bias_grad=db))
        mr2 = torch.zeros_like(mr)
        timed(f"prelu/{tag} slice_stats", lambda: ops.slice_stats(y, 0, C, mr2))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs=6, metavar="JSON", help="A1 B1 A2 B2 A3 B3 of six single runs")
    args = ap.parse_args()
    if args.merge:
        print(json.dumps(merge(args.merge), indent=1))
    else:
        measure()
