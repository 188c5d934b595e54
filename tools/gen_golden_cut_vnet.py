"""Records tests/golden/cut_vnet.json: a few iterations of the REAL reference's CUT recipe on Vnet3D + PatchGAN3D
(the networks of projects/brats_mri_sequence_translation/experiments/cut.yaml at reduced depth and size), on the CPU.
Build container only — the reference is imported the way oracle/gen_golden.py does (through oracle/ref_stubs), and the
fixture holds data only: the case's settings, learning rates and losses per iteration.

    python -m tools.gen_golden_cut_vnet

Weights come from oracle.torch_ref.seeded_state_dict(net, seed + k) in the order of `model.networks` (G, D, mlp), inputs
from the seeded generator of gen_golden.inputs_3d, and torch.manual_seed(1000 + s) in front of iteration s pins the
torch.randperm patch ids (CPU generator), all as for tests/golden/cut_steps.json.

`nce_layers` lists one index more than the encoder has modules, like the brats yaml ([0..4] for [in_ab] + 3 downs): the
reference's assert lets it through (cut.py:301), one feature level fewer comes out, and the loss is divided by the length
of the list (cut.py:226). The two cases differ in `num_patches`: 256 gives the deepest level fewer patches than the
others (min(num_patches, voxels), cut.py:267), 32 gives every level the same count."""
import json
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "cut_vnet.json"

VNET = dict(first_layer_channels=16, down_blocks=[1, 1], up_blocks=[1, 1])
CASES = {
    "cutv_16x24x32_p256": dict(size=[16, 24, 32], batch=2, steps=3, n_iters=100, n_iters_decay=100, num_patches=256,
                               nce_layers=[0, 1, 2, 3], d_layers=2, lr_G=0.0004, lr_D=0.0002, seed=71, vnet=VNET),
    "cutv_16x24x32_p32": dict(size=[16, 24, 32], batch=1, steps=3, n_iters=100, n_iters_decay=100, num_patches=32,
                              nce_layers=[0, 1, 2, 3], d_layers=2, lr_G=0.0004, lr_D=0.0002, seed=72, vnet=VNET),
}


def make_conf(G, c):
    conf = G.make_conf_3d(dict(c, pool_size=0, lambda_identity=0.0, proportion_ssim=0.0))
    gan = conf.train.gan
    gan["_target_"] = "ganslate.nn.gans.unpaired.CUT"
    gan["nce_layers"] = c["nce_layers"]
    gan["mlp_nc"] = 256
    gan["num_patches"] = c["num_patches"]
    gan["use_equivariance_flip"] = False
    gan.generator["in_channels"] = 1      # the key cut.py:83 reads; absent from the schema
    gan["optimizer"] = G.DictConfig({"adversarial_loss_type": "lsgan", "beta1": 0.5, "beta2": 0.999, "lr_D": c["lr_D"],
                                     "lr_G": c["lr_G"], "lambda_adv": 1, "lambda_nce": 1, "lambda_nce_idt": 0.5,
                                     "nce_T": 0.07})
    return conf


def run_case(G, name, c):
    from oracle.torch_ref import seeded_state_dict
    torch.manual_seed(c["seed"])
    model = G.CUT(make_conf(G, c))
    for k, (n, net) in enumerate(model.networks.items()):
        net.load_state_dict(seeded_state_dict(net, c["seed"] + k))
    levels = len(model.networks["mlp"].mlps)
    rec = []
    for s in range(c["steps"]):
        A, B = G.inputs_3d(c, s)
        torch.manual_seed(1000 + s)
        model.set_input({"A": A, "B": B})
        model.optimize_parameters()
        lrs, losses, visuals, metrics = model.get_loggable_data()
        rec.append({"lrs": {k: float(v) for k, v in lrs.items()},
                    "losses": {k: float(v) for k, v in losses.items() if v is not None}})
        model.update_learning_rate()
        print(name, s, rec[-1]["losses"], flush=True)
    return {"config": c, "feature_levels": levels, "steps": rec}


def main():
    from oracle import gen_golden as G          # puts the reference on sys.path and imports it
    torch.set_num_threads(8)
    OUT.write_text(json.dumps({name: run_case(G, name, c) for name, c in CASES.items()}, indent=1))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
