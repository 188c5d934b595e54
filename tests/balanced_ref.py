"""The balanced multi-modal CycleGAN restated in plain torch, for tests/test_balanced_cpu.py and tests/test_balanced_gpu.py.

`BalancedRefOps` adds plain-torch versions of the channel-window ops of HipOps to the CPU oracle backend (slices, torch.cat and
zeros are exactly what the kernels replace). `BalancedStep` is an fp32 restatement of one training iteration on the
oracle's networks, written from the recipe's semantics: each domain tensor is [guide | translated] (or the other way round),
the generators read a whole tensor and emit the translated channels, the return trip reads the generated channels spliced
next to the REAL guide channels, discriminators and cycle losses see the translated channels only, the logged visuals are
the generated channels padded with zero guide channels. Nothing here calls the package's kernels."""
import random
from collections import OrderedDict
from pathlib import Path

import torch

from oracle import torch_ref
from oracle.ops_ref import RefOps, ssim_distance
from tests import loss_ref

CONFIGS = Path(__file__).parent / "configs"


class BalancedRefOps(RefOps):
    """RefOps plus the channel-window methods of HipOps that only this recipe calls"""

    def channel_embed(self, src, dst, c0):
        dst.zero_()
        dst[:, c0:c0 + src.shape[1]] = src

    def l1_window(self, a, c0, c1, b, loss=None, grad_b=None, grad_scale=None):
        aw = a[:, c0:c1]
        if loss is not None:
            loss.copy_((aw - b).abs().mean())
        if grad_b is not None:
            s = grad_scale if grad_scale is not None else 1.0
            grad_b.copy_(s * torch.sign(b - aw) / b.numel())

    def ssim_distance_window(self, x, c0, c1, y, out):
        self.ssim_distance(x[:, c0:c1], y, out)

    def ssim_distance_window_backward(self, x, c0, c1, y, grad_y, grad_scale=None):
        self.ssim_distance_backward(x[:, c0:c1], y, grad_y, grad_scale=grad_scale)


# ---- cases -----------------------------------------------------------------------------------------------------------------
# cg2d: ClearGrasp-shaped, A = [rgb | normal], B = [rgb | depth]; hx3d: HX4-shaped, [PET | CT] volumes in both domains.
# (the reference's U-Nets have at least five stride-2 levels whatever num_downs says, so the volume is 32 deep)
CASES = {
    "cg2d": dict(yaml="cyclegan_balanced_cg2d.yaml", dims=2, batch=2, size=(64, 64), C={"A": 6, "B": 4},
                 win={"A": (3, 6), "B": (3, 4)}, num_downs=6, ngf=8, ndf=8, n_layers=2, pool_size=3, proportion_ssim=0.84,
                 metrics_ssim=True, n_iters=4, n_iters_decay=4, seed=7),
    "hx3d": dict(yaml="cyclegan_balanced_hx3d.yaml", dims=3, batch=1, size=(32, 32, 32), C={"A": 2, "B": 2},
                 win={"A": (0, 1), "B": (0, 1)}, num_downs=5, ngf=8, ndf=8, n_layers=2, pool_size=3, proportion_ssim=0.0,
                 metrics_ssim=False, n_iters=4, n_iters_decay=4, seed=11),
}


def case_inputs(c, step):
    """seeded uniform [-1, 1]; A and B (guides included) are independent draws"""
    g = torch.Generator().manual_seed(c["seed"] * 100 + step)
    A = torch.rand((c["batch"], c["C"]["A"], *c["size"]), generator=g) * 2 - 1
    B = torch.rand((c["batch"], c["C"]["B"], *c["size"]), generator=g) * 2 - 1
    return A, B


def shadow_networks(c):
    """the oracle's networks of a case with their seeded weights (seed + k in the order G_AB, G_BA, D_B, D_A)"""
    G, D = (torch_ref.Unet2D, torch_ref.PatchGAN2D) if c["dims"] == 2 else (torch_ref.Unet3D, torch_ref.PatchGAN3D)
    t = {X: c["win"][X][1] - c["win"][X][0] for X in "AB"}
    nets = OrderedDict(G_AB=G(c["C"]["A"], t["B"], c["num_downs"], c["ngf"], False),
                       G_BA=G(c["C"]["B"], t["A"], c["num_downs"], c["ngf"], False),
                       D_B=D(t["B"], c["ndf"], c["n_layers"]), D_A=D(t["A"], c["ndf"], c["n_layers"]))
    for k, net in enumerate(nets.values()):
        net.load_state_dict(torch_ref.seeded_state_dict(net, c["seed"] + k))
    return nets


def build_product(c, extra=()):
    """the product recipe of a case with the same seeded weights"""
    from ganslate_amd.utils.builders import build_conf, build_gan
    conf = build_conf([f"config={CONFIGS / c['yaml']}", *extra])
    torch.manual_seed(c["seed"])
    model = build_gan(conf)
    for name, net in shadow_networks(c).items():
        if name in model.networks:
            model.networks[name].load_state_dict(net.state_dict())
    random.seed(c["seed"])
    return model


def run_product_steps(model, c, n_steps):
    out = []
    for s in range(n_steps):
        A, B = case_inputs(c, s)
        model.set_input({"A": A, "B": B})
        model.optimize_parameters()
        lrs, losses, visuals, metrics = model.get_loggable_data()
        out.append({"lrs": dict(lrs),
                    "losses": {k: float(v.detach()) for k, v in losses.items() if v is not None},
                    "metrics": {k: float(v) for k, v in metrics.items() if v is not None}})
        model.update_learning_rate()
    return out


def _guide(win, C):
    return (win[1], C) if win[0] == 0 else (0, win[0])


def splice(generated, real, win, C):
    """generated channels at the translated position, the real image's guide channels at the guide position"""
    g0, g1 = _guide(win, C)
    parts = [generated, real[:, g0:g1]] if win[0] == 0 else [real[:, g0:g1], generated]
    return torch.cat(parts, dim=1)


def embed(generated, win, C):
    out = torch.zeros((generated.shape[0], C) + tuple(generated.shape[2:]), dtype=generated.dtype)
    out[:, win[0]:win[1]] = generated
    return out


class BalancedStep:
    """fp32 restatement of one iteration of the balanced CycleGAN (lsgan, Adam, linear decay, image pools of translated images)"""

    def __init__(self, c, lr_G=2e-4, lr_D=2e-4, beta1=0.5, beta2=0.999, lambda_AB=10.0, lambda_BA=10.0, dtype=torch.float32):
        """dtype=torch.float64: the same step evaluated in float64 (inputs are widened by step()) — the yardstick for how far
        one honest fp32 evaluation lies from the exact gradients"""
        self.c, self.dtype = c, dtype
        self.nets = shadow_networks(c)
        for net in self.nets.values():
            net.to(dtype)
        self.hp = dict(lambda_AB=lambda_AB, lambda_BA=lambda_BA, proportion_ssim=c["proportion_ssim"])
        pG = list(self.nets["G_AB"].parameters()) + list(self.nets["G_BA"].parameters())
        pD = list(self.nets["D_B"].parameters()) + list(self.nets["D_A"].parameters())
        self.opt_G = torch.optim.Adam(pG, lr=lr_G, betas=(beta1, beta2))
        self.opt_D = torch.optim.Adam(pD, lr=lr_D, betas=(beta1, beta2))
        n_iters, n_decay = c["n_iters"], c["n_iters_decay"]
        rule = lambda it: 1.0 - max(0, it + 1 - n_iters) / float(n_decay + 1)      # noqa: E731
        self.sched = [torch.optim.lr_scheduler.LambdaLR(o, rule) for o in (self.opt_G, self.opt_D)]
        self.pool_A, self.pool_B = torch_ref.ImagePool(c["pool_size"]), torch_ref.ImagePool(c["pool_size"])
        self.visuals, self.translated = {}, {}

    def _set_D_grad(self, flag):
        for n in ("D_B", "D_A"):
            for p in self.nets[n].parameters():
                p.requires_grad = flag

    def _ssim(self, x, y):
        # (the oracle's fp32 statement, or tests/loss_ref.py's float64 one)
        return ssim_distance(x, y) if self.dtype == torch.float32 else loss_ref.ssim_distance(x, y)

    def _cycle(self, real, rec):
        if self.dtype == torch.float32:
            return torch_ref.cycle_loss(real, rec, self.hp["proportion_ssim"])
        p, l1 = self.hp["proportion_ssim"], (rec - real).abs().mean()
        return p * self._ssim(rec, real) + (1 - p) * l1 if p > 0 else l1

    def step(self, real_A, real_B, update=True):
        c, hp, nets = self.c, self.hp, self.nets
        real_A, real_B = real_A.to(self.dtype), real_B.to(self.dtype)
        wA, wB, CA, CB = c["win"]["A"], c["win"]["B"], c["C"]["A"], c["C"]["B"]
        losses, metrics = {}, {}
        fake_Bt = nets["G_AB"](real_A)
        rec_At = nets["G_BA"](splice(fake_Bt, real_A, wA, CA))      # domain-B layout: A's and B's windows lie on one side
        fake_At = nets["G_BA"](real_B)
        rec_Bt = nets["G_AB"](splice(fake_At, real_B, wB, CB))
        self.translated = dict(fake_B=fake_Bt, rec_A=rec_At, fake_A=fake_At, rec_B=rec_Bt)
        self.visuals = dict(real_A=real_A, real_B=real_B,
                            fake_B=embed(fake_Bt.detach(), wB, CB), rec_A=embed(rec_At.detach(), wA, CA),
                            fake_A=embed(fake_At.detach(), wA, CA), rec_B=embed(rec_Bt.detach(), wB, CB))
        if c["metrics_ssim"]:
            with torch.no_grad():
                metrics["ssim_A"] = 1 - self._ssim(real_A, self.visuals["rec_A"])
                metrics["ssim_B"] = 1 - self._ssim(real_B, self.visuals["rec_B"])
        # ---- generators ----
        self._set_D_grad(False)
        self.opt_G.zero_grad(set_to_none=True)
        losses["G_AB"] = torch_ref.adversarial_loss(nets["D_B"](fake_Bt), True)
        losses["G_BA"] = torch_ref.adversarial_loss(nets["D_A"](fake_At), True)
        losses["cycle_A"] = hp["lambda_AB"] * self._cycle(real_A[:, wA[0]:wA[1]], rec_At)
        losses["cycle_B"] = hp["lambda_BA"] * self._cycle(real_B[:, wB[0]:wB[1]], rec_Bt)
        (losses["cycle_A"] + losses["cycle_B"] + losses["G_AB"] + losses["G_BA"]).backward()
        if update:
            self.opt_G.step()
        # ---- discriminators ----
        self._set_D_grad(True)
        self.opt_D.zero_grad(set_to_none=True)
        for name, real, fake, pool in (("D_B", real_B[:, wB[0]:wB[1]], fake_Bt, self.pool_B),
                                       ("D_A", real_A[:, wA[0]:wA[1]], fake_At, self.pool_A)):
            fake = pool.query(fake)
            pred_real, pred_fake = nets[name](real), nets[name](fake.detach())
            losses[name] = torch_ref.adversarial_loss(pred_real, True) + torch_ref.adversarial_loss(pred_fake, False)
            losses[name].backward()
            metrics[f"{name}_real"] = pred_real.detach().mean()
            metrics[f"{name}_fake"] = pred_fake.detach().mean()
        if update:
            self.opt_D.step()
        return {k: float(v.detach()) for k, v in losses.items()}, {k: float(v) for k, v in metrics.items()}

    def grads(self):
        """{network: {state_dict name: .grad}} left by the last step(update=False)"""
        return {n: {k: p.grad.detach().clone() for k, p in net.named_parameters()} for n, net in self.nets.items()}

    def update_learning_rate(self):
        for s in self.sched:
            s.step()

    def lrs(self):
        return {"lr_G": self.opt_G.param_groups[0]["lr"], "lr_D": self.opt_D.param_groups[0]["lr"]}
