#!/usr/bin/env python
"""Time of the structure-consistency (MIND) loss (run on the GPU box):

  * `fused`: the library's kernels for the four descriptors of one CycleGAN iteration at N x 3 x S x S — StructureLoss(real_A,
    fake_B) and StructureLoss(real_B, fake_A), each forward (gs_mind_l1) plus the gradient w.r.t. the generated image
    (gs_mind_l1_backward);
  * `torch`: the same work written in float32 torch operators with autograd — shifted copies, an 81-channel depthwise 7x7
    convolution, exp, a channel sum — which is what a recipe gets whose criterion is written by hand;
  * `step`: one `bench.py`-shaped CycleGAN iteration (batch N, S x S, the bench's config) with lambda_structure 0 and 0.5.

    python tools/mind_time.py [--batch 8] [--size 256] [--iters 20] [--rounds 5] [--out profiles/mind_time.json]

Device time between HIP events round `--iters` calls after a warm-up, per call, the minimum and the median over `--rounds`
rounds, the variants alternating. Loss and gradient of the two forms are compared first."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as TF

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from ganslate_amd.hip.ops import HipOps  # noqa: E402


def torch_descriptor(img, sigma=2.0):
    """the descriptor in torch operators: one plane per image, 81 shifted copies, depthwise patch convolutions"""
    I = img.mean(dim=1, keepdim=True)
    N, _, H, W = I.shape
    q = torch.arange(7, dtype=torch.float32, device=img.device) - 3
    g = torch.exp(-torch.sqrt(q[:, None] ** 2 + q[None, :] ** 2) / (sigma * sigma))
    Ip = TF.pad(I, (4, 4, 4, 4))
    shifted = torch.cat([Ip[:, :, i % 9:i % 9 + H, i // 9:i // 9 + W] for i in range(81)], dim=1)
    D = TF.conv2d((shifted - I) ** 2, g.expand(81, 1, 7, 7).contiguous(), padding=3, groups=81)
    Ip1 = TF.pad(I, (1, 1, 1, 1))
    nb = torch.cat([Ip1[:, :, i % 3:i % 3 + H, i // 3:i // 3 + W] for i in range(9)], dim=1)
    B = TF.conv2d(nb, torch.ones((9, 1, 7, 7), device=img.device), padding=3, groups=9)
    n = torch.exp(-D / (B.var(dim=1, keepdim=True) + 1e-8))
    return n / n.sum(dim=1, keepdim=True)


def torch_structure(X, Y):
    H, W = X.shape[-2:]
    return (torch_descriptor(X) - torch_descriptor(Y)).abs().sum() / (H * W * 81)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def alternate(variants, iters, rounds, warmup=3):
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    return {k: {"ms_min": round(min(v), 4), "ms_median": round(statistics.median(v), 4), "ms_rounds": [round(t, 4) for t in v]}
            for k, v in times.items()}


def loss_case(ops, a):
    dev = ops.device
    g = torch.Generator().manual_seed(0)
    shape = (a.batch, 3, a.size, a.size)
    real_A, fake_B, real_B, fake_A = ((torch.rand(shape, generator=g) * 2 - 1).to(dev) for _ in range(4))
    pairs = ((real_A, fake_B), (real_B, fake_A))
    one = torch.ones((), device=dev)
    loss = [torch.empty((), device=dev) for _ in pairs]
    grad = [torch.empty_like(y) for _, y in pairs]

    def fused():
        for k, (x, y) in enumerate(pairs):
            ops.mind_l1(x, y, loss[k])
            ops.mind_l1_backward(x, y, grad[k], grad_scale=one)

    tl, tg = [None, None], [None, None]

    def torch_form():
        for k, (x, y) in enumerate(pairs):
            yy = y.detach().requires_grad_()
            tl[k] = torch_structure(x, yy)
            (tg[k],) = torch.autograd.grad(tl[k], yy)

    fused()
    torch_form()
    torch.cuda.synchronize()
    agree = {"loss_rel": max(abs(float(loss[k]) - float(tl[k])) / abs(float(tl[k])) for k in range(2)),
             "grad_rel_to_max": max(float((grad[k] - tg[k]).abs().max() / tg[k].abs().max()) for k in range(2))}
    res = alternate({"fused": fused, "torch": torch_form}, a.iters, a.rounds)
    res["torch_over_fused_min"] = round(res["torch"]["ms_min"] / res["fused"]["ms_min"], 2)
    parts = alternate({"forward": lambda: ops.mind_l1(real_A, fake_B, loss[0]),
                       "backward": lambda: ops.mind_l1_backward(real_A, fake_B, grad[0], grad_scale=one)}, a.iters, a.rounds)
    return {"shape": list(shape), "work": "2 x (loss + gradient w.r.t. the generated image) = four descriptors, forward and backward",
            "agreement": agree, **res, "fused_one_pair": parts}


def step_case(a):
    sys.path.insert(0, str(ROOT))
    import bench
    from ganslate_amd.utils.builders import build_gan
    dev = torch.device("cuda:0")
    out = {}
    for lam in (0, 0.5):
        conf = bench.make_conf(a.batch, a.size, 10 ** 6)
        conf.train.gan.optimizer.lambda_structure = lam
        torch.manual_seed(0)
        model = build_gan(conf)
        g = torch.Generator().manual_seed(0)
        shape = (a.batch, 3, a.size, a.size)
        batch = {"A": (torch.rand(shape, generator=g) * 2 - 1).to(dev), "B": (torch.rand(shape, generator=g) * 2 - 1).to(dev)}

        def step():
            model.set_input(batch)
            model.optimize_parameters()
            model.update_learning_rate()
        for _ in range(a.step_warmup):
            step()
        times = [timed(step, a.step_iters) for _ in range(a.rounds)]
        out[f"lambda_structure={lam}"] = {"ms_min": round(min(times), 3), "ms_median": round(statistics.median(times), 3),
                                          "ms_rounds": [round(t, 3) for t in times], "captured": model._graph is not None}
        del model
        torch.cuda.empty_cache()
    a0, a1 = out["lambda_structure=0"]["ms_min"], out["lambda_structure=0.5"]["ms_min"]
    out["added_ms_min"] = round(a1 - a0, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--step-warmup", type=int, default=6)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops = HipOps()
    result = {"workload": "structure-consistency (MIND) loss", "timer": "HIP events round the calls, per call",
              "iters_per_round": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
              "loss": loss_case(ops, a)}
    if not a.no_step:
        result["step"] = step_case(a)
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
