#!/usr/bin/env python
"""Writes tests/golden/loss_bits.json: the bit patterns and gradient digests of every case of tests/loss_bits_cases.py, from the
library of the commit the file then names (run on the GPU box):

    GANSLATE_HIP_LIB=<libganslate_hip.so built from that commit> python tools/gen_golden_loss_bits.py --commit <its hash>

The file pins what csrc/loss.hip computes bit for bit, so it is recorded from the library BEFORE a change that must not move
a bit (a worktree of the parent commit, built apart), never from the library under test; tests/test_loss_bits_gpu.py then runs
the same cases on the tree's library. Re-record only with a change that alters results on purpose, and say so there."""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from ganslate_amd.hip.ops import HipOps  # noqa: E402
from tests import loss_bits_cases as B  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit the library in GANSLATE_HIP_LIB was built from")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "loss_bits.json"))
    a = ap.parse_args()
    ops = HipOps()
    results = {}
    for group in B.GROUPS:
        results.update(B.run_group(ops, group))
    torch.cuda.synchronize()
    out = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "results": results}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
    print(a.out, len(results), "entries")


if __name__ == "__main__":
    main()
