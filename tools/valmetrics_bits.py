#!/usr/bin/env python
"""Digests of everything HipOps.valmetrics / valmetrics_masked (csrc/valmetrics.hip) return, on fixed seeded inputs:

    GANSLATE_HIP_LIB=<library> python tools/valmetrics_bits.py > digests.json
    python tools/valmetrics_bits.py --join parent.json branch.json > profiles/<name>_bits.json

Run it once per build of the library, each in its own process, and join the two files: one sha256 per output (the table; the
t, p and joint counts), so a refactor of that file that claims bit identity has every digest equal ("different": []). The cases:
every case of tests/valmetrics_edges_ref.py through the wrappers (run), its GUARDED cases through the library calls on 0xFF
buffers with the table's extra row (run_guarded), one plain and one L = 8 case with ssim only, histograms only and neither, and
the two shapes of tools/bench_valmetrics.py with its data, plain and under its three masks."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BENCH_SHAPES = [(8, 3, 256, 256), (1, 1, 155, 240, 240)]        # tools/bench_valmetrics.py SHAPES
FLAG_CASES = ("tiles_3x2", "m_L8")
OUT = {}


def put(name, **arrays):
    for key, a in arrays.items():
        assert f"{name}/{key}" not in OUT, name
        OUT[f"{name}/{key}"] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def put_call(name, table, words):
    """table and the count words [.., 100 + 100 + 100 * 100] of one call"""
    put(name, table=table, t_counts=words[..., :100], p_counts=words[..., 100:200], joint_counts=words[..., 200:])


def edge_cases(ops, R):
    for case in R.CASES:
        td, pd, md = R.to_device(case, *R.data(case), ops.device)
        put_call(f"run/{case.name}", *R.run(ops, case, td, pd, md))
        if case.name in R.GUARDED:
            table, words, extra, nbytes = R.run_guarded(ops, case, td, pd, md)
            put_call(f"run_guarded/{case.name}", table, words)
            put(f"run_guarded/{case.name}", extra_row=extra, scratch_bytes=np.int64(nbytes))
        if case.name in FLAG_CASES:
            for ssim, hist in ((True, False), (False, True), (False, False)):
                fn = (lambda **kw: ops.valmetrics_masked(td, pd, md, **kw)) if case.masks else (lambda **kw: ops.valmetrics(td, pd, **kw))
                put(f"flags/{case.name}/ssim{int(ssim)}_hist{int(hist)}", table=fn(ssim=ssim, hist=hist).cpu().numpy())


def bench_cases(ops):
    """the data of tools/bench_valmetrics.py --masks 3: a box and two random 40 % masks"""
    import torch
    rng = np.random.default_rng(0)
    for shape in BENCH_SHAPES:
        t = rng.uniform(-1000, 3000, shape).astype(np.float32)
        p = (t + rng.normal(0, 60, shape)).astype(np.float32)
        box = np.zeros(shape, dtype=bool)
        box[(slice(None), slice(None)) + tuple(slice(s // 4, 3 * s // 4) for s in shape[2:])] = True
        masks = [torch.from_numpy(m).to(ops.device) for m in [box] + [rng.random(shape) < 0.4 for _ in range(2)]]
        td, pd = torch.from_numpy(t).to(ops.device), torch.from_numpy(p).to(ops.device)
        name = "x".join(map(str, shape))
        for kind, (table, (ht, hp, hj)) in (("plain", ops.valmetrics(td, pd, return_counts=True)),
                                            ("masks3", ops.valmetrics_masked(td, pd, masks, return_counts=True))):
            put(f"bench/{name}/{kind}", table=table.cpu().numpy(), t_counts=ht.cpu().numpy(), p_counts=hp.cpu().numpy(),
                joint_counts=hj.cpu().numpy())


def join(parent, branch):
    a, b = (json.loads(Path(f).read_text()) for f in (parent, branch))
    return {"what": "sha256 of every output of HipOps.valmetrics / valmetrics_masked on the seeded cases of "
                    "tools/valmetrics_bits.py, MI355X; one process per library",
            "digests": len(b), "different": sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k)),
            "parent": a, "branch": b}


def main():
    if sys.argv[1:2] == ["--join"]:
        print(json.dumps(join(*sys.argv[2:4]), indent=1, sort_keys=True))
        return
    from ganslate_amd.hip.ops import HipOps
    from tests import valmetrics_edges_ref as R
    ops = HipOps()
    edge_cases(ops, R)
    bench_cases(ops)
    print(json.dumps(OUT, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
