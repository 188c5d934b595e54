"""Writes tests/golden/mind.json from the IMPORTED reference's own MINDDescriptor and StructureLoss
(projects/cleargrasp_depth_estimation/modules/old/cyclegan_losses_with_structure.py; needs the reference checkout next to
the stand-in modules of oracle/ref_stubs, like tools/gen_golden_separable.py):

    python tools/gen_golden_mind.py

Everything runs in float64 (`MINDDescriptor(...).double()`; its patch weights were built in fp32 and are widened). Cases:
  small    1 x 1 x 4 x 5   smaller than every halo; the features of X in full
  plain    1 x 1 x 12 x 14
  mean3    2 x 3 x 10 x 13 against 2 x 1 x 10 x 13: the 3 channels are reduced by the mean, as the reference does with its
           normal maps
The loss goes through StructureLoss(lambda_structure, use_cuda=False, "v1"), whose v1 branch takes the descriptor of `fake`
(1 channel) and of the mean of `input_[:, 3:]`: X rides in channels 3.. of an `input_` whose first three channels are noise
the loss must not see. The file holds numbers only: the inputs (fp32 values), per case the loss, the 81 channel sums of
both descriptors and, for the larger cases, a seeded sample of feature elements [flat index, value]."""
import importlib.util
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("GANSLATE_REFERENCE", ROOT.parent / "reference"))      # the reference checkout
sys.path.insert(0, str(ROOT / "oracle" / "ref_stubs"))
sys.path.insert(1, str(REF))
sys.path.insert(2, str(ROOT))

import ganslate.configs.base  # noqa: E402,F401

LAMBDA = 0.5
SAMPLES = 200
CASES = {"small": ((1, 1, 4, 5), (1, 1, 4, 5), 5), "plain": ((1, 1, 12, 14), (1, 1, 12, 14), 6),
         "mean3": ((2, 3, 10, 13), (2, 1, 10, 13), 7)}


def load_module():
    path = REF / "projects" / "cleargrasp_depth_estimation" / "modules" / "old" / "cyclegan_losses_with_structure.py"
    spec = importlib.util.spec_from_file_location("ref_structure", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def f64(t):
    return [float(v) for v in t.detach().double().flatten().tolist()]


def main():
    torch.set_num_threads(1)
    mod = load_module()
    cfg = dict(mod.MIND_DESCRIPTOR_CONFIG)
    desc = mod.MINDDescriptor(**cfg).double()
    crit = mod.StructureLoss(LAMBDA, False, "v1")
    crit.mind_descriptor = crit.mind_descriptor.double()
    out = {"config": cfg, "lambda_structure": LAMBDA,
           "patch_weights": f64(desc.summation_patcher.weight[0, 0]), "cases": {}}
    for name, (sx, sy, seed) in CASES.items():
        g = torch.Generator().manual_seed(seed)
        X = torch.rand(sx, generator=g) * 2 - 1
        Y = torch.rand(sy, generator=g) * 2 - 1
        noise = torch.rand((sx[0], 3, sx[2], sx[3]), generator=g).double()
        with torch.no_grad():
            fx = desc(X.double().mean(dim=1, keepdim=True))
            fy = desc(Y.double())
            loss = crit(torch.cat([noise, X.double()], dim=1), Y.double())
        c = {"x_shape": list(sx), "y_shape": list(sy), "x": f64(X), "y": f64(Y), "loss": float(loss),
             "channel_sums_x": f64(fx.sum(dim=(0, 2, 3))), "channel_sums_y": f64(fy.sum(dim=(0, 2, 3)))}
        if name == "small":
            c["features_x"] = f64(fx)
        else:
            idx = torch.randint(0, fx.numel(), (SAMPLES,), generator=g)
            c["feature_samples_x"] = [[int(i), float(fx.flatten()[i])] for i in idx]
            c["feature_samples_y"] = [[int(i), float(fy.flatten()[i])] for i in idx]
        out["cases"][name] = c
    path = ROOT / "tests" / "golden" / "mind.json"
    path.write_text(json.dumps(out, separators=(",", ":")))
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
