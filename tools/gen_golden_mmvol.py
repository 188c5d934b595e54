"""Writes tests/golden/mmvol_draws.json from the IMPORTED reference's own patch samplers
(projects/maastro_hx4_pet_translation/datasets/utils/patch_samplers.py: PairedPatchSampler3D, UnpairedPatchSampler3D) and
its min_max_normalize (ganslate/data/utils/normalization.py); needs the reference checkout:

    python tools/gen_golden_mmvol.py

The sampler module imports `loguru`, which is not installed: a stand-in module whose logger counts warnings is registered
first — the reference warns exactly when its stochastic-focal draw falls back to the whole body, so the count is the
fallback flag. The image dicts are the seeded volumes of tests/mmvol_ref.py::synthetic_case with the body mask applied the way
basic.py's apply_body_mask does (np.where(mask, image, fill)), plus an `index` volume holding every voxel's own flat index:
the sampler crops it like any other entry and its first value reveals the patch start.

Per case and seed: np.random.seed(seed), DRAWS consecutive get_patch_pair calls. Recorded per call: start_A / start_B, the
fallback flag and, per modality, the normalised patch (divisor, torch.clamp, min_max_normalize) at SAMPLES seeded flat
positions. Recorded per seed: how many np.random uniforms the calls consumed (the state afterwards equals the state after
that many random_sample() calls) and the next uniform of the stream. The file holds numbers and names only."""
import importlib.util
import json
import os
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("GANSLATE_REFERENCE", ROOT.parent / "reference"))      # the reference checkout
sys.path.insert(0, str(ROOT))

from tests.mmvol_ref import synthetic_case  # noqa: E402

DRAWS, SAMPLES = 3, 6
# reference dict key -> (file stem / synthetic_case key, clip range, value outside the body)
MODS = {"FDG-PET": ("pet", (0.0, 6.0), 0.0), "pCT": ("ct", (-1000.0, 2000.0), -1024.0),
        "HX4-PET": ("hx4", (0.0, 3.0), 0.0), "ldCT": ("ct", (-1000.0, 2000.0), -1024.0)}
HX4_DIVISOR = 1.75
CASES = {
    "paired_uniform": dict(paired=True, scheme="uniform-random-within-body", shape_A=[16, 40, 40], patch=[8, 16, 16]),
    "paired_weighted": dict(paired=True, scheme="fdg-pet-weighted", shape_A=[16, 40, 40], patch=[8, 16, 16]),
    "paired_odd": dict(paired=True, scheme="uniform-random-within-body", shape_A=[9, 17, 13], patch=[3, 5, 7]),
    "unpaired_uniform": dict(paired=False, scheme="uniform-random-within-body-sf", shape_A=[16, 40, 40],
                             shape_B=[18, 36, 44], patch=[8, 16, 16], proportion=[0.6, 0.3, 0.3]),
    "unpaired_weighted": dict(paired=False, scheme="fdg-pet-weighted-sf", shape_A=[16, 40, 40], shape_B=[18, 36, 44],
                              patch=[8, 16, 16], proportion=[0.6, 0.3, 0.3]),
    "unpaired_odd": dict(paired=False, scheme="uniform-random-within-body-sf", shape_A=[9, 17, 13], shape_B=[11, 15, 14],
                         patch=[3, 5, 7], proportion=[0.5, 0.4, 0.6]),
    # B's body lies in the corner opposite to A's: every focal box misses it and the reference falls back
    "unpaired_fallback": dict(paired=False, scheme="uniform-random-within-body-sf", shape_A=[16, 40, 40],
                              shape_B=[18, 36, 44], patch=[8, 16, 16], proportion=[0.3, 0.2, 0.2], body_A="high",
                              body_B="low"),
}
SEEDS = [11, 12, 13]


class _Logger:
    warnings = 0

    def warning(self, *a, **k):
        _Logger.warnings += 1

    info = debug = error = warning


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def image_dict(vols, names):
    d = {"body-mask": vols["body"], "index": vols["index"]}
    for n in names:
        key, _, fill = MODS[n]
        d[n] = np.where(vols["body"], vols[key], fill)               # apply_body_mask
    return d


def uniforms_consumed(seed, state_after):
    np.random.seed(seed)
    for k in range(0, 4 * DRAWS + 1):
        s = np.random.get_state()
        if s[2] == state_after[2] and np.array_equal(s[1], state_after[1]):
            return k
        np.random.random_sample()
    raise RuntimeError("the reference consumed something else than whole uniforms")


def main():
    stub = types.ModuleType("loguru")
    stub.logger = _Logger()
    sys.modules["loguru"] = stub
    ps = load(REF / "projects" / "maastro_hx4_pet_translation" / "datasets" / "utils" / "patch_samplers.py", "ref_samplers")
    norm = load(REF / "ganslate" / "data" / "utils" / "normalization.py", "ref_normalization")
    out = {"draws": DRAWS, "hx4_divisor": HX4_DIVISOR, "modalities": {k: [v[0], list(v[1]), v[2]] for k, v in MODS.items()},
           "cases": {}}
    for name, c in CASES.items():
        names_A = ["FDG-PET", "pCT"]
        names_B = ["HX4-PET"] if c["paired"] else ["HX4-PET", "ldCT"]
        rec = dict(c, names_A=names_A, names_B=names_B, seeds={})
        patch = np.array(c["patch"])
        for seed in SEEDS:
            A = synthetic_case(c["shape_A"], seed, c.get("body_A", "ellipsoid"))
            B = A if c["paired"] else synthetic_case(c["shape_B"], seed + 100, c.get("body_B", "ellipsoid"))
            dict_A, dict_B = image_dict(A, names_A), image_dict(B, names_B)
            sampler = (ps.PairedPatchSampler3D(patch, c["scheme"]) if c["paired"] else
                       ps.UnpairedPatchSampler3D(patch, c["scheme"], c["proportion"]))
            at = np.random.default_rng(seed + 7).choice(int(np.prod(patch)), SAMPLES, replace=False)
            np.random.seed(seed)
            calls = []
            for _ in range(DRAWS):
                before = _Logger.warnings
                pa, pb = sampler.get_patch_pair(dict(dict_A), dict(dict_B))
                call = {"fallback": _Logger.warnings - before, "values": {}}
                for key, patches, shape in (("A", pa, c["shape_A"]), ("B", pb, c.get("shape_B", c["shape_A"]))):
                    assert patches["index"].shape == tuple(patch), patches["index"].shape
                    call["start_" + key] = [int(v) for v in np.unravel_index(int(patches["index"][0, 0, 0]), shape)]
                    for n in (names_A if key == "A" else names_B):
                        lo, hi = MODS[n][1]
                        t = torch.tensor(np.ascontiguousarray(patches[n]))
                        if n == "HX4-PET":
                            t = t / HX4_DIVISOR
                        t = norm.min_max_normalize(torch.clamp(t, lo, hi), lo, hi)
                        assert t.dtype == torch.float32
                        call["values"][n] = [float(v) for v in t.flatten()[torch.from_numpy(at)]]
                calls.append(call)
            state = np.random.get_state()
            probe = float(np.random.random_sample())
            rec["seeds"][str(seed)] = {"values_at": [int(v) for v in at], "calls": calls,
                                       "uniforms_consumed": uniforms_consumed(seed, state), "next_uniform": probe}
        out["cases"][name] = rec
    path = ROOT / "tests" / "golden" / "mmvol_draws.json"
    path.write_text(json.dumps(out, indent=None, separators=(",", ":")) + "\n")
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
