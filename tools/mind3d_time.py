#!/usr/bin/env python
"""Time of the volumetric structure-consistency (MIND) loss, csrc/mind3d.hip (run on the GPU box):

  * `loss`: at 1 x 1 x 128 x 128 x 128 and 1 x 1 x 32 x 176 x 176, one loss (gs_mind3d_l1) and one gradient w.r.t. the
    generated volume (gs_mind3d_l1_backward), each alone and as the pair a CycleGAN direction launches;
  * `step`: one `bench.py --workload cyclegan3d`-shaped iteration (Resnet3D-9 + PatchGAN3D-3, batch 1, S^3, the bench's
    config) with lambda_structure 0 and 0.5.

    python tools/mind3d_time.py [--iters 10] [--rounds 5] [--step-size 128] [--out profiles/mind3d_time.json]

Device time between HIP events round `--iters` calls after a warm-up, per call, the minimum and the median over `--rounds`
rounds, the variants alternating."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from ganslate_amd.hip.ops import HipOps  # noqa: E402
from tools.mind_time import alternate, timed  # noqa: E402

SHAPES = ((1, 1, 128, 128, 128), (1, 1, 32, 176, 176))


def loss_case(ops, shape, a):
    dev = ops.device
    g = torch.Generator().manual_seed(0)
    real, fake = ((torch.rand(shape, generator=g) * 2 - 1).to(dev) for _ in range(2))
    one = torch.ones((), device=dev)
    loss, grad = torch.empty((), device=dev), torch.empty_like(fake)

    def forward():
        ops.mind3d_l1(real, fake, loss)

    def backward():
        ops.mind3d_l1_backward(real, fake, grad, grad_scale=one)

    def pair():
        forward()
        backward()

    res = alternate({"forward": forward, "backward": backward, "pair": pair}, a.iters, a.rounds)
    N, _, D, H, W = shape
    return {"shape": list(shape), "work": "one loss + one gradient w.r.t. the generated volume (one CycleGAN direction)",
            "loss": float(loss), "grad_abs_max": float(grad.abs().max()),
            "scratch_bytes_backward": int(ops.lib.gs_mind3d_scratch_bytes(N, D, H, W, 1)),
            "workgroups": int(ops.lib.gs_mind3d_scratch_bytes(N, D, H, W, 0)) // 4, **res}


def step_case(a):
    import bench
    from ganslate_amd.utils.builders import build_gan
    dev = torch.device("cuda:0")
    out = {"shape": [1, 1, a.step_size, a.step_size, a.step_size], "networks": "Resnet3D-9 + PatchGAN3D-3"}
    for lam in (0, 0.5):
        conf = bench.make_volume_conf(1, a.step_size, 10 ** 6)
        conf.train.gan.optimizer.lambda_structure = lam
        torch.manual_seed(0)
        model = build_gan(conf)
        g = torch.Generator().manual_seed(0)
        shape = (1, 1, a.step_size, a.step_size, a.step_size)
        batch = {"A": (torch.rand(shape, generator=g) * 2 - 1).to(dev), "B": (torch.rand(shape, generator=g) * 2 - 1).to(dev)}

        def step():
            model.set_input(batch)
            model.optimize_parameters()
            model.update_learning_rate()
        for _ in range(a.step_warmup):
            step()
        times = [timed(step, a.step_iters) for _ in range(a.rounds)]
        row = {"ms_min": round(min(times), 3), "ms_median": round(statistics.median(times), 3),
               "ms_rounds": [round(t, 3) for t in times], "captured": model._graph is not None}
        if lam:
            row["structure_AB"] = float(model.losses["structure_AB"].detach())
            row["structure_BA"] = float(model.losses["structure_BA"].detach())
        out[f"lambda_structure={lam}"] = row
        del model
        torch.cuda.empty_cache()
    out["added_ms_min"] = round(out["lambda_structure=0.5"]["ms_min"] - out["lambda_structure=0"]["ms_min"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-size", type=int, default=128)
    ap.add_argument("--step-iters", type=int, default=4)
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops = HipOps()
    result = {"workload": "volumetric structure-consistency (MIND) loss", "timer": "HIP events round the calls, per call",
              "iters_per_round": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
              "loss": [loss_case(ops, s, a) for s in SHAPES]}
    if not a.no_step:
        result["step"] = step_case(a)
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
