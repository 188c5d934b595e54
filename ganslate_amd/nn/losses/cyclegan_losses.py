"""Cycle-consistency and identity losses — interface and weighting of ganslate/nn/losses/cyclegan_losses.py:7-101:
cycle_A = lambda_AB * [alpha*SSIMdist + (1-alpha)*L1](real_A, rec_A); idt_B = lambda_AB * lambda_idt * L1(idt_B, real_B)
(note the reference pairs idt_B with lambda_AB and idt_A with lambda_BA, :50-52). With `lambda_structure > 0` also the
structure-consistency terms of the reference's cleargrasp project (cyclegan_losses_with_structure.py:25-38):
structure_AB = lambda_AB * StructureLoss(real_A, fake_B), structure_BA = lambda_BA * StructureLoss(real_B, fake_A); on
[N, C, D, H, W] visuals the same two names carry StructureLoss3D, the volumetric definition."""
from .functional import l1_loss, scalar_affine, ssim_distance_autograd
from .structure_loss import StructureLoss, StructureLoss3D


class CycleGANLosses:

    def __init__(self, conf):
        opt = conf.train.gan.optimizer
        self.lambda_AB, self.lambda_BA = opt.lambda_AB, opt.lambda_BA
        self.criterion_cycle = CycleLoss(opt.proportion_ssim)
        self.criterion_idt = IdentityLoss(opt.lambda_identity) if opt.lambda_identity > 0 else None
        lambda_structure = getattr(opt, "lambda_structure", 0) or 0
        # one criterion per rank of the visuals: [N, C, H, W] images / [N, C, D, H, W] volumes
        self.criterion_structure = StructureLoss(lambda_structure) if lambda_structure > 0 else None
        self.criterion_structure_3d = StructureLoss3D(lambda_structure) if lambda_structure > 0 else None

    def is_using_identity(self):
        return bool(self.criterion_idt)

    def is_using_structure(self):
        return bool(self.criterion_structure)

    def _structure_criterion(self, real):
        """the structure criterion for visuals of real's rank; a criterion put in place of the library's own is used as is"""
        if type(self.criterion_structure) is StructureLoss and real.dim() == 5:
            return self.criterion_structure_3d
        return self.criterion_structure

    def __call__(self, visuals):
        real_A, real_B = visuals["real_A"], visuals["real_B"]
        rec_A, rec_B = visuals["rec_A"], visuals["rec_B"]
        idt_A, idt_B = visuals["idt_A"], visuals["idt_B"]
        if self.criterion_idt and (idt_A is None or idt_B is None):
            raise ValueError("idt_A and/or idt_B is not computed but the identity loss is defined.")
        criterion_structure = self._structure_criterion(real_A)
        if type(self.criterion_cycle) is CycleLoss and type(self.criterion_idt) in (IdentityLoss, type(None)) and \
                type(criterion_structure) in (StructureLoss, StructureLoss3D, type(None)):
            # the library's own criterions: every weighted term of every loss, then ONE launch for the scalar algebra
            names = ["cycle_A", "cycle_B"]
            parts = [[(self.lambda_AB * w, x) for w, x in self.criterion_cycle.terms(real_A, rec_A)],
                     [(self.lambda_BA * w, x) for w, x in self.criterion_cycle.terms(real_B, rec_B)]]
            if self.criterion_idt:
                names += ["idt_B", "idt_A"]
                parts += [[(self.lambda_AB * w, x) for w, x in self.criterion_idt.terms(idt_B, real_B)],
                          [(self.lambda_BA * w, x) for w, x in self.criterion_idt.terms(idt_A, real_A)]]
            if criterion_structure:
                names += ["structure_AB", "structure_BA"]
                parts += [[(self.lambda_AB * w, x) for w, x in criterion_structure.terms(real_A, visuals["fake_B"])],
                          [(self.lambda_BA * w, x) for w, x in criterion_structure.terms(real_B, visuals["fake_A"])]]
            xs = [x for p in parts for _, x in p]
            rows, k = [], 0
            for p in parts:
                rows.append([0.0] * k + [w for w, _ in p] + [0.0] * (len(xs) - k - len(p)))
                k += len(p)
            return dict(zip(names, scalar_affine(xs, rows)))
        losses = {
            "cycle_A": self.lambda_AB * self.criterion_cycle(real_A, rec_A),
            "cycle_B": self.lambda_BA * self.criterion_cycle(real_B, rec_B),
        }
        if self.criterion_idt:
            losses["idt_B"] = self.lambda_AB * self.criterion_idt(idt_B, real_B)
            losses["idt_A"] = self.lambda_BA * self.criterion_idt(idt_A, real_A)
        if criterion_structure:
            losses["structure_AB"] = self.lambda_AB * criterion_structure(real_A, visuals["fake_B"])
            losses["structure_BA"] = self.lambda_BA * criterion_structure(real_B, visuals["fake_A"])
        return losses


class CycleLoss:

    def __init__(self, proportion_ssim):
        self.alpha = proportion_ssim
        self.beta = 1 - proportion_ssim

    def terms(self, real, reconstructed):
        """[(weight, 0-d loss)] whose weighted sum is the loss"""
        l1 = l1_loss(reconstructed, real)
        if self.alpha > 0:
            return [(self.alpha, ssim_distance_autograd(reconstructed, real)), (self.beta, l1)]
        return [(1.0, l1)]

    def __call__(self, real, reconstructed):
        t = self.terms(real, reconstructed)
        return scalar_affine([x for _, x in t], [[w for w, _ in t]])[0] if len(t) > 1 else t[0][1]


class IdentityLoss:

    def __init__(self, lambda_identity):
        self.lambda_identity = lambda_identity

    def terms(self, idt, real):
        return [(self.lambda_identity, l1_loss(idt, real))]

    def __call__(self, idt, real):
        (w, x), = self.terms(idt, real)
        return scalar_affine([x], [[w]])[0]
