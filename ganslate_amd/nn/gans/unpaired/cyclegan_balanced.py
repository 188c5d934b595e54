"""Balanced multi-modal CycleGAN ("CycleGAN-balanced") — the design the reference's projects implement as CycleGAN
subclasses: projects/maastro_hx4_pet_translation/modules/hx4_cyclegan_balanced.py:18-127 with its losses
hx4_cyclegan_balanced_losses.py:7-35 (experiments/cyclegan_balanced.yaml), and the cleargrasp project's
experiments/cyclegan_balanced.yaml ([rgb | normal] <-> [rgb | depth], generators 6 -> 1 and 4 -> 3 channels).

Each domain tensor is a GUIDE modality next to a TRANSLATED modality along the channel axis (HX4: [PET | CT], translated
[0, 1) of 2 channels in both domains; ClearGrasp: [rgb | normal] and [rgb | depth], translated [3, 6) of 6 and [3, 4) of 4).
`translated_channels: {A: [start, stop], B: [start, stop]}` (half-open, required) names the translated channels. With
C_A, t_B = generator.in_out_channels.AB and C_B, t_A = generator.in_out_channels.BA:
  * range X has width t_X and is a prefix or a suffix of its domain's channels, on the same side in both domains;
  * the guides have the same width, C_A - t_A == C_B - t_B >= 1;
  * discriminator.in_channels is {B: t_B, A: t_A}.
A violation, `lambda_identity > 0` (the reference's subclasses build no identity criterion and silently ignore the value,
hx4_cyclegan_balanced_losses.py:12-20; it is refused here) and `lambda_structure > 0` (not defined for this design) raise a
ValueError that names the field.

Forward (hx4_cyclegan_balanced.py:35-60), xt = the translated channels of x, guide(x) the others:
  fake_Bt = G_AB(real_A);  rec_At = G_BA(splice(fake_Bt, guide(real_A)))
  fake_At = G_BA(real_B);  rec_Bt = G_AB(splice(fake_At, guide(real_B)))
splice puts the generated channels at the translated position and the REAL guide channels at the guide position (:43,48).
visuals["fake_B" | "rec_A" | "fake_A" | "rec_B"] are the generated channels at the translated position of a tensor whose guide
channels are zero (:54-60), so fake_B has C_B channels and logging.multi_modality_split and the validators see the reference's
shapes; compute_metrics_G runs on these padded visuals as it does there (cyclegan.py:95-98 inherited).
Discriminators (:62-90): D_B sees real_B[:, tB] and pool_B.query(fake_Bt) — the pools hold t-channel images; D_B's update runs
first, so pool and RNG order are the stock recipe's. Generator step (:92-115): adversarial terms on D_B(fake_Bt), D_A(fake_At);
cycle_A = lambda_AB * CycleLoss(real_A[:, tA], rec_At), cycle_B = lambda_BA * CycleLoss(real_B[:, tB], rec_Bt)
(hx4_cyclegan_balanced_losses.py:23-35), proportion_ssim honoured; no identity or structure term, idt_* stay None.
infer (:119-127) returns G(input) embedded in zeros like the visuals; with is_train=False only G_AB exists.

None of the reference's torch.cat / channel slices / zeros_like exists here as a launch of torch's: the splice and the
discriminators' real windows are converted straight into the first activation (gs_image_cat_to_act through
NativeNet.forward_sources; the gradient of the generated source comes back dense and joins the discriminator's through
fanout), the cycle losses read the real window in place (gs_l1_window, gs_ssim_distance_window), the padded visuals are one
pass each (gs_channel_embed). Generators: Unet2D and Unet3D (any executor whose images enter through the plain image
conversion); Resnet2D and Resnet3D (W-folded k7 stems), the V-Net family and Piresnet3D raise NotImplementedError at
construction.
Scheduling is the stock recipe's with GS_TWIN=0: graph_capturable, second cycle and discriminator update on side streams;
twin passes are not built."""
from dataclasses import dataclass, field
from typing import Tuple

import torch

from .... import configs
from ....configs.omegalite import MISSING, MissingMandatoryValue
from ...losses.functional import (channel_embed, fanout, l1_window_loss, scalar_affine, scalar_sum,
                                  ssim_distance_window_autograd)
from . import cyclegan


@dataclass
class TranslatedChannelsConfig:
    A: Tuple[int, int] = MISSING
    B: Tuple[int, int] = MISSING


@dataclass
class CycleGANBalancedConfig(cyclegan.CycleGANConfig):
    # half-open channel ranges [start, stop) of the translated modality in domain A and in domain B
    translated_channels: TranslatedChannelsConfig = field(default_factory=TranslatedChannelsConfig)


class BalancedLayout:
    """channel bookkeeping of the two domains, checked against the network configs"""

    def __init__(self, gan):
        ioc, dch = gan.generator.in_out_channels, gan.discriminator.in_channels if gan.discriminator is not None else None
        (C_A, t_B), (C_B, t_A) = (int(v) for v in ioc.AB), (int(v) for v in ioc.BA)
        tc = gan.translated_channels
        self.C = {"A": C_A, "B": C_B}
        self.t = {"A": t_A, "B": t_B}
        self.win, side = {}, {}
        for X in ("A", "B"):
            try:
                rng = [int(v) for v in tc[X]]
            except MissingMandatoryValue:
                raise ValueError(f"translated_channels.{X} is required: the half-open channel range [start, stop) of the "
                                 f"translated modality in domain {X}") from None
            if len(rng) != 2 or not 0 <= rng[0] < rng[1] <= self.C[X]:
                raise ValueError(f"translated_channels.{X} = {rng}: a half-open range [start, stop) inside the domain's "
                                 f"{self.C[X]} channels expected")
            if rng[1] - rng[0] != self.t[X]:
                raise ValueError(f"translated_channels.{X} = {rng} is {rng[1] - rng[0]} wide, but the generator towards {X} "
                                 f"(generator.in_out_channels) emits {self.t[X]} channels")
            if rng[0] != 0 and rng[1] != self.C[X]:
                raise ValueError(f"translated_channels.{X} = {rng} must be a prefix or a suffix of the domain's {self.C[X]} channels")
            side[X] = "prefix" if rng[0] == 0 else "suffix"
            self.win[X] = (rng[0], rng[1])
        guide = {X: self.C[X] - self.t[X] for X in ("A", "B")}
        if min(guide.values()) < 1 or guide["A"] != guide["B"]:
            raise ValueError(f"generator.in_out_channels: the guide widths C_A - t_A = {guide['A']} and C_B - t_B = {guide['B']} "
                             "must be equal and at least 1")
        if side["A"] != side["B"]:
            raise ValueError(f"translated_channels: A is a {side['A']} and B a {side['B']} of its domain; both must lie on the "
                             "same side")
        self.prefix = side["A"] == "prefix"
        self.guide = {X: ((self.t[X], self.C[X]) if self.prefix else (0, guide[X])) for X in ("A", "B")}
        if dch is not None and (int(dch.B), int(dch.A)) != (t_B, t_A):
            raise ValueError(f"discriminator.in_channels must be {{B: {t_B}, A: {t_A}}} (the translated channels), got "
                             f"{{B: {int(dch.B)}, A: {int(dch.A)}}}")

    def splice(self, generated, real, real_domain):
        """channel sources of torch.cat of `generated` (at the translated position) and guide(real) (at the guide position)"""
        g = (generated, 0, generated.shape[1])
        r = (real,) + self.guide[real_domain]
        return [g, r] if self.prefix else [r, g]


class BalancedLosses:
    """cycle_A / cycle_B on the translated channels only (hx4_cyclegan_balanced_losses.py:23-35): the weighted terms of
    CycleLoss (cyclegan_losses.py:70-90) with the real image read through its channel window, one launch for the scalar algebra"""

    def __init__(self, conf, layout):
        opt = conf.train.gan.optimizer
        self.lambda_AB, self.lambda_BA = opt.lambda_AB, opt.lambda_BA
        self.alpha, self.beta = opt.proportion_ssim, 1 - opt.proportion_ssim
        self.layout = layout

    def is_using_identity(self):
        return False

    def is_using_structure(self):
        return False

    def terms(self, real, window, rec):
        l1 = l1_window_loss(real, window, rec)
        if self.alpha > 0:
            return [(self.alpha, ssim_distance_window_autograd(real, window, rec)), (self.beta, l1)]
        return [(1.0, l1)]

    def __call__(self, real_A, real_B, rec_At, rec_Bt):
        parts = [[(self.lambda_AB * w, x) for w, x in self.terms(real_A, self.layout.win["A"], rec_At)],
                 [(self.lambda_BA * w, x) for w, x in self.terms(real_B, self.layout.win["B"], rec_Bt)]]
        xs = [x for p in parts for _, x in p]
        rows, k = [], 0
        for p in parts:
            rows.append([0.0] * k + [w for w, _ in p] + [0.0] * (len(xs) - k - len(p)))
            k += len(p)
        return dict(zip(["cycle_A", "cycle_B"], scalar_affine(xs, rows)))


class CycleGANBalanced(cyclegan.CycleGAN):

    def __init__(self, conf):
        gan = conf.train.gan
        self.layout = BalancedLayout(gan)
        for name in ("lambda_identity", "lambda_structure"):
            if (getattr(gan.optimizer, name, 0) or 0) > 0:
                raise ValueError(f"optimizer.{name} = {getattr(gan.optimizer, name)}: the balanced CycleGAN has no "
                                 f"{name.split('_')[1]} term ({name} must be 0)")
        self._translated = {}
        super().__init__(conf)
        for name, net in self.networks.items():
            supports = getattr(net, "supports_channel_sources", None)
            if supports is None or not supports():
                raise NotImplementedError(f"CycleGANBalanced: {type(net).__name__} ({name}) does not take its images through "
                                          "the plain image conversion; channel sources are not supported for it")

    def _init_twins(self):
        self.twin_G = self.twin_D = None      # twin passes are not built for this recipe

    def init_criterions(self):
        super().init_criterions()
        self.criterion_G = BalancedLosses(self.conf, self.layout)

    def _embed(self, generated, domain):
        return channel_embed(generated, self.layout.C[domain], self.layout.win[domain][0])

    def forward(self):
        """the stock recipe's two cycles (second one on its own stream), the return trips reading channel sources"""
        real_A, real_B = self.visuals["real_A"], self.visuals["real_B"]
        G_AB, G_BA, lay = self.networks["G_AB"], self.networks["G_BA"], self.layout
        for net in (G_AB, G_BA):
            net.refresh_packs(real_A)
            net.multi_stream_passes = True
        self.fork_side_work("cycle_B")
        fake_Bt, fake_Bt2 = fanout(G_AB(real_A))
        rec_At, = G_BA.forward_sources([lay.splice(fake_Bt2, real_A, "A")])
        vis = {"fake_B": self._embed(fake_Bt, "B"), "rec_A": self._embed(rec_At, "A")}
        with self.side_work("cycle_B"):
            fake_At, fake_At2 = fanout(G_BA(real_B))
            rec_Bt, = G_AB.forward_sources([lay.splice(fake_At2, real_B, "B")])
            vis.update({"fake_A": self._embed(fake_At, "A"), "rec_B": self._embed(rec_Bt, "B")})
        self.join_side_work("cycle_B", last=False)
        self._translated = {"fake_B": fake_Bt, "rec_A": rec_At, "fake_A": fake_At, "rec_B": rec_Bt}
        self.visuals.update(vis, idt_A=None, idt_B=None)

    def backward_D(self, discriminator):
        if discriminator == "D_B":
            real, win, fake = self.visuals["real_B"], self.layout.win["B"], self.fake_B_pool.query(self._translated["fake_B"])
        elif discriminator == "D_A":
            real, win, fake = self.visuals["real_A"], self.layout.win["A"], self.fake_A_pool.query(self._translated["fake_A"])
        else:
            raise ValueError('The discriminator has to be either "D_A" or "D_B".')
        D = self.networks[discriminator]
        fake = fake.detach()
        # D(real[:, t]) and D(fake) as one pass over both batches; the real window is read in place
        self.pred_real, self.pred_fake = D.forward_sources([[(real,) + win], [(fake, 0, fake.shape[1])]])
        loss_real = self.criterion_adv(self.pred_real, target_is_real=True)
        loss_fake = self.criterion_adv(self.pred_fake, target_is_real=False)
        self.losses[discriminator] = scalar_sum((loss_real, loss_fake))
        self.backward(loss=self.losses[discriminator], optimizer=self.optimizers["D"], loss_id=2)

    def backward_G(self):
        tr = self._translated
        pred_B = self.networks["D_B"](tr["fake_B"])
        pred_A = self.networks["D_A"](tr["fake_A"])
        self.fork_side_work()
        self.losses["G_AB"] = self.criterion_adv(pred_B, target_is_real=True)
        self.losses["G_BA"] = self.criterion_adv(pred_A, target_is_real=True)
        losses_G = self.criterion_G(self.visuals["real_A"], self.visuals["real_B"], tr["rec_A"], tr["rec_B"])
        self.losses.update(losses_G)
        combined_loss_G = scalar_sum(list(losses_G.values()) + [self.losses["G_AB"], self.losses["G_BA"]])
        self.backward(loss=combined_loss_G, optimizer=self.optimizers["G"], loss_id=0)
        self.join_side_work("cycle_B")

    def infer(self, input, direction="AB"):
        assert direction in ["AB", "BA"], "Specify which generator direction, AB or BA, to use."
        assert f"G_{direction}" in self.networks.keys()
        with torch.no_grad():
            return self._embed(self.networks[f"G_{direction}"](input), direction[1])
