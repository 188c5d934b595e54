#!/usr/bin/env python
"""Time of one DeviceImagePipeline.__call__ on a batch of decoded images (run on the GPU box): the per-image path (two
launches, two device tensors and one pinned upload per image; the Trainer's path) against the batched path (one staging
upload, one descriptor table, two launches per batch; the path of the val / test / infer engines), on the same host-resident
uint8 images with the same draws. Two cases: 32 RGB images of 256x256, and a mixed set of 480x640 and 1024x768 images, both
through `resize` 286 -> `random_crop` 256 -> `random_flip`.

    python tools/imgbatch_time.py [--batch 32] [--iters 200] [--rounds 5] [--out profiles/imgbatch_time.json]

Per path and case: device time between HIP events recorded round the call's work on the stream, host wall clock round the
whole call including a synchronise, both per call as the minimum over `--rounds` rounds of `--iters` calls after a
warm-up, the two paths alternating; images/s from the wall clock; kernel launches and host-to-device copies per batch,
counted on the calls the pipeline makes. The outputs of the two paths are compared bit for bit first."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from ganslate_amd.data.device_transforms import DeviceImagePipeline, RawImage  # noqa: E402
from ganslate_amd.hip.ops import HipOps  # noqa: E402

LAUNCHES = {"u8_resample_h": 1, "u8_resample_v": 1, "u8_resample_v_crop_normalize": 1, "u8_batch_resample": 2}


class D(dict):
    __getattr__ = dict.__getitem__


class Counting:
    """the backend with its image-transform calls counted"""

    def __init__(self, ops):
        self._ops, self.launches = ops, 0

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if name not in LAUNCHES:
            return fn

        def counted(*a, **kw):
            self.launches += LAUNCHES[name]
            return fn(*a, **kw)
        return counted


def raws(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [RawImage(torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)), (rng.random(), rng.random()),
                     bool(k % 2)) for k, (h, w) in enumerate(sizes)]


def timed(fn, iters):
    """(device ms, host wall ms) per call"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / iters
    return start.elapsed_time(end) / iters, wall


def case(name, sizes, ops, a):
    conf = D(mode="val", val=D(dataset=D(preprocess=["resize", "random_crop", "random_flip"], load_size=[286, 286],
                                         final_size=[256, 256])))
    batch = {"A": raws(sizes)}
    paths, outs, counts = {}, {}, {}
    for path, batched in (("per_image", False), ("batched", True)):
        counter = Counting(ops)
        pipe = DeviceImagePipeline(conf, ops.device, ops=counter, batched=batched)
        outs[path] = pipe(batch)["A"]
        # uploads: one per image, or the staging buffer and the descriptor table
        counts[path] = {"launches_per_batch": counter.launches, "h2d_copies_per_batch": 2 if batched else len(sizes)}
        paths[path] = lambda p=pipe: p(batch)
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["per_image"], outs["batched"]))
    for _ in range(5):
        for fn in paths.values():
            fn()
    times = {p: [] for p in paths}
    for _ in range(a.rounds):
        for p, fn in paths.items():
            times[p].append(timed(fn, a.iters))
    result = {"case": name, "images": len(sizes), "outputs_equal": same}
    for p in paths:
        dev, wall = min(t[0] for t in times[p]), min(t[1] for t in times[p])
        result[p] = dict(counts[p], device_ms_per_call=round(dev, 4), wall_ms_per_call=round(wall, 4),
                         images_per_s=round(len(sizes) / (wall * 1e-3)),
                         wall_ms_rounds=[round(t[1], 4) for t in times[p]])
    result["per_image_over_batched_wall"] = round(result["per_image"]["wall_ms_per_call"] /
                                                  result["batched"]["wall_ms_per_call"], 2)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops = HipOps()
    cases = [case(f"{a.batch} x 256x256 RGB", [(256, 256)] * a.batch, ops, a),
             case(f"{a.batch} x mixed 480x640 / 1024x768 RGB", [(480, 640), (1024, 768)] * (a.batch // 2), ops, a)]
    result = {"workload": "DeviceImagePipeline.__call__, host-resident decoded images -> resize 286 -> crop 256 -> flip -> "
                          "fp32 NCHW batch on the device", "iters_per_round": a.iters, "rounds": a.rounds,
              "timer": "device events round the calls; host wall clock round the calls and a synchronise", "cases": cases,
              "device": torch.cuda.get_device_name(0)}
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
