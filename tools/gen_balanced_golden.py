#!/usr/bin/env python
"""Golden losses of the balanced multi-modal CycleGAN from the REFERENCE's own project modules (build container only: the
reference checkout is read next to the stand-in modules of oracle/ref_stubs, like tools/gen_golden_mind.py):

    python tools/gen_balanced_golden.py            # writes tests/golden/balanced_steps.json

Runs step 0 of the two cases of tests/balanced_ref.py — cg2d on projects/cleargrasp_depth_estimation/modules/
cyclegan_multimodal_v3.py (CycleGANMultiModalV3), hx3d on projects/maastro_hx4_pet_translation/modules/hx4_cyclegan_balanced.py
(HX4CycleGANBalanced) — with the seeded weights and inputs the tests use, and records the losses only.
tests/test_balanced_cpu.py holds the plain-torch restatement (BalancedStep) to them."""
import json
import os
import random
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("GANSLATE_REFERENCE", ROOT.parent / "reference"))      # the reference checkout
sys.path.insert(0, str(ROOT / "oracle" / "ref_stubs"))
sys.path.insert(1, str(REF))
sys.path.insert(2, str(ROOT))

from omegaconf import DictConfig  # noqa: E402  (the stand-in)
import ganslate.configs.base  # noqa: E402,F401
from projects.cleargrasp_depth_estimation.modules.cyclegan_multimodal_v3 import CycleGANMultiModalV3  # noqa: E402
from projects.maastro_hx4_pet_translation.modules.hx4_cyclegan_balanced import HX4CycleGANBalanced  # noqa: E402

from oracle.torch_ref import seeded_state_dict  # noqa: E402
from tests import balanced_ref as B  # noqa: E402

MODULES = {"cg2d": CycleGANMultiModalV3, "hx3d": HX4CycleGANBalanced}


def make_conf(c):
    d = "2D" if c["dims"] == 2 else "3D"
    t = {X: c["win"][X][1] - c["win"][X][0] for X in "AB"}
    return DictConfig({
        "mode": "train",
        "train": {
            "output_dir": "/tmp/ganslate_ref_out", "cuda": False, "mixed_precision": False, "opt_level": "O1",
            "batch_size": c["batch"], "n_iters": c["n_iters"], "n_iters_decay": c["n_iters_decay"],
            "checkpointing": {"load_iter": None, "freq": 10 ** 9, "start_after": 0, "load_optimizers": True},
            "metrics": {"discriminator_evolution": True, "ssim": c["metrics_ssim"]},
            "gan": {
                "_target_": "project.modules.CycleGANBalanced", "norm_type": "instance",
                "weight_init_type": "normal", "weight_init_gain": 0.02, "pool_size": c["pool_size"],
                "generator": {"_target_": f"ganslate.nn.generators.Unet{d}", "num_downs": c["num_downs"], "ngf": c["ngf"],
                              "use_dropout": False,
                              "in_out_channels": {"AB": [c["C"]["A"], t["B"]], "BA": [c["C"]["B"], t["A"]]}},
                "discriminator": {"_target_": f"ganslate.nn.discriminators.PatchGAN{d}", "ndf": c["ndf"],
                                  "n_layers": c["n_layers"], "kernel_size": [4] * c["dims"],
                                  "in_channels": {"B": t["B"], "A": t["A"]}},
                "optimizer": {"adversarial_loss_type": "lsgan", "beta1": 0.5, "beta2": 0.999, "lr_D": 0.0002,
                              "lr_G": 0.0002, "lambda_AB": 10.0, "lambda_BA": 10.0, "lambda_identity": 0,
                              "proportion_ssim": c["proportion_ssim"]},
            },
        },
    })


def run_case(name, c):
    torch.manual_seed(c["seed"])
    model = MODULES[name](make_conf(c))
    for k, (n, net) in enumerate(model.networks.items()):
        net.load_state_dict(seeded_state_dict(net, c["seed"] + k))
    random.seed(c["seed"])
    A, Bt = B.case_inputs(c, 0)
    model.set_input({"A": A, "B": Bt})
    model.optimize_parameters()
    _, losses, _, _ = model.get_loggable_data()
    losses = {k: float(v.detach()) for k, v in losses.items() if v is not None}
    print(name, losses, flush=True)
    return {"module": f"{MODULES[name].__module__}.{MODULES[name].__name__}", "losses": losses}


def main():
    torch.set_num_threads(8)
    out = {name: run_case(name, c) for name, c in B.CASES.items()}
    path = ROOT / "tests" / "golden" / "balanced_steps.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
