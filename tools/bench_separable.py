"""Measurements for `is_separable=True` (report, not a gate):

  python tools/bench_separable.py kernel     # the row-axis classes through gs_gconv_forward, option `daxis` on against off
  python tools/bench_separable.py step       # the brats CycleGAN step (bench.py --workload brats networks), separable vs dense

Each figure is the median of REPS launches / iterations timed with events on the launch stream after WARMUP untimed ones;
one JSON line per measurement."""
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WARMUP, REPS = 5, 30


def _median_us(fn, reps=REPS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), min(times)


def kernel():
    from ganslate_amd.nn.native.backend import get_ops
    from ganslate_amd.nn.native.spec import ConvSpec, lower
    ops = get_ops()
    dev = ops.device
    for c, v in ((16, 128), (32, 128), (32, 64), (64, 32)):
        spec = ConvSpec("conv", c, c, 5, 1, 2, dims=3, axes="axis")
        low = lower(spec, v, v, v)
        g = low.fwd[0]
        x = torch.randn(1, v, v * v, c, device=dev).to(torch.bfloat16)
        y = torch.empty_like(x)
        pack = (torch.randn(low.fwd_index.size + 64, device=dev) * 0.05).to(torch.bfloat16)
        bias = torch.zeros(c, device=dev)
        nbytes = 2 * x.numel() * 2
        for stats in (False, True):
            row = {"class": f"{c}->{c} (5,1,1) at {v}^3", "stats": stats, "bytes_moved": nbytes}
            for on in (0, 1):
                with ops.options(daxis=on):                 # (1: every launch of 64 voxels or more)
                    slots = ops.stat_slots(g, 1) if stats else 0
                    part = torch.empty(max(slots * 2 * c, 1), dtype=torch.float32, device=dev)
                    fn = lambda: ops.gconv(g, x, pack, bias, y, stats=part if stats else None, stats_slots=slots)
                    med, best = _median_us(fn)
                row[f"daxis={on}"] = {"median_us": round(med, 1), "min_us": round(best, 1),
                                      "TB_per_s": round(nbytes / med * 1e-6, 3)}
            print(json.dumps(row), flush=True)


def step():
    import bench
    from ganslate_amd.utils.builders import build_gan
    size = 128
    for sep in (False, True):
        conf = bench.make_volume_conf(1, size, 1000, "vnet")
        conf.train.gan.generator.is_separable = sep
        torch.manual_seed(0)
        model = build_gan(conf)
        g = torch.Generator().manual_seed(1)
        A, B = (torch.rand(1, 1, size, size, size, generator=g) * 2 - 1 for _ in range(2))
        A, B = A.to(model.device), B.to(model.device)

        def it():
            model.set_input({"A": A, "B": B})
            model.optimize_parameters()
        med, best = _median_us(it, reps=15, warmup=5)
        print(json.dumps({"workload": "brats CycleGAN step, 128^3, batch 1", "is_separable": sep,
                          "daxis": model.networks["G_AB"].ops.get_option("daxis"),
                          "median_ms": round(med / 1e3, 2), "min_ms": round(best / 1e3, 2),
                          "volumes_per_s": round(1e6 / med, 2)}), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    {"kernel": kernel, "step": step}[sys.argv[1]]()
