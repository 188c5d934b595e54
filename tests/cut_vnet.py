"""Shared helpers of the CUT-on-V-Net tests (CPU oracle backend and GPU): the golden cases of tests/golden/cut_vnet.json
(tools/gen_golden_cut_vnet.py: the real reference's CUT on Vnet3D + PatchGAN3D) and the product configured like them."""
import json
from pathlib import Path

import torch

GOLD = Path(__file__).parent / "golden" / "cut_vnet.json"
CONF = Path(__file__).parent / "configs" / "cut_vnet3d_synthetic.yaml"


def load_golden_cut_vnet():
    return json.loads(GOLD.read_text())


def _list(v):
    return "[" + ",".join(str(x) for x in v) + "]"


def cpu_drawn_ids(model):
    """patch ids drawn on the CPU generator (as the reference does on CPU), whatever the device"""
    G = model.networks["G"]

    def sample(*sizes):
        ids = []
        for e in model.tap_layers:
            pid = torch.randperm(G.tap_extent(e, *sizes))
            ids.append(pid[:int(min(model.num_patches, len(pid)))].to(model.device))
        return ids

    model.sample_patch_ids = sample
    return model


def build_product_cut_vnet(c, extra=()):
    """product CUT configured like golden case `c`, with the oracle's seeded weights loaded"""
    from ganslate_amd.utils.builders import build_conf, build_gan
    from oracle import torch_ref
    v = c["vnet"]
    conf = build_conf([f"config={CONF}", f"train.batch_size={c['batch']}", f"train.n_iters={c['n_iters']}",
                       f"train.n_iters_decay={c['n_iters_decay']}", f"train.gan.num_patches={c['num_patches']}",
                       f"train.gan.nce_layers={_list(c['nce_layers'])}",
                       f"train.gan.generator.first_layer_channels={v['first_layer_channels']}",
                       f"train.gan.generator.down_blocks={_list(v['down_blocks'])}",
                       f"train.gan.generator.up_blocks={_list(v['up_blocks'])}",
                       f"train.gan.discriminator.n_layers={c['d_layers']}",
                       f"train.gan.optimizer.lr_G={c['lr_G']}", f"train.gan.optimizer.lr_D={c['lr_D']}",
                       f"train.dataset.final_size={_list(c['size'])}", *extra])
    torch.manual_seed(c["seed"])
    model = build_gan(conf)
    G = torch_ref.Vnet3D(1, 1, v["first_layer_channels"], tuple(v["down_blocks"]), tuple(v["up_blocks"]))
    channels = [v["first_layer_channels"] << e for e in model.tap_layers]
    shadow = {"G": G, "D": torch_ref.PatchGAN3D(1, 64, c["d_layers"]),
              "mlp": torch_ref._PatchMLP(channels, c["num_patches"], 256)}
    for k, name in enumerate(["G", "D", "mlp"]):
        model.networks[name].load_state_dict(torch_ref.seeded_state_dict(shadow[name], c["seed"] + k))
    return cpu_drawn_ids(model)


def cut_vnet_inputs(c, step):
    g = torch.Generator().manual_seed(c["seed"] * 100 + step)
    shape = (c["batch"], 1, *c["size"])
    return torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1


def run_product_cut_vnet_steps(model, c, n_steps):
    out = []
    for s in range(n_steps):
        A, B = cut_vnet_inputs(c, s)
        torch.manual_seed(1000 + s)          # pins the torch.randperm patch ids of this step, as the recording did
        model.set_input({"A": A, "B": B})
        model.optimize_parameters()
        lrs, losses, visuals, metrics = model.get_loggable_data()
        out.append({"lrs": dict(lrs), "losses": {k: float(v.detach()) for k, v in losses.items() if v is not None}})
        model.update_learning_rate()
    return out
