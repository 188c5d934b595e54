"""The structure-consistency (MIND) loss without a GPU: the float64 restatement of tests/mind_ref.py against vectors recorded
from the reference's own module (tests/golden/mind.json, tools/gen_golden_mind.py), the config field and loss names, the
recipe wiring on the CPU ops, and the yardstick that the GPU tolerances of tests/test_mind_gpu.py stand on."""
import json
from pathlib import Path

import pytest
import torch

from ganslate_amd.nn.native import backend
from ganslate_amd.utils.builders import build_conf
from oracle.ops_ref import RefOps

from . import mind_ref as M
from .helpers import build_product_cyclegan, golden_inputs, load_golden_steps

GOLD = json.loads((Path(__file__).parent / "golden" / "mind.json").read_text())
CONFIGS = Path(__file__).parent / "configs"
STRUCTURE = ("train.gan.optimizer.lambda_structure=0.5",)
STOCK_NAMES = ["G_AB", "D_B", "cycle_A", "idt_A", "G_BA", "D_A", "cycle_B", "idt_B"]


def _t64(values, shape):
    return torch.tensor(values, dtype=torch.float64).reshape(shape)


# ---- the restatement against the reference's own numbers -----------------------------------------------------------
# 1e-10 relative: both sides are float64 evaluations of one formula; a patch sum has ~4e3 terms (relative error of the sum
# ~4e3 * 2^-53 = 4e-13) and exp(-t) carries t's error times t (t up to ~1e2 here): < 1e-10 with room to spare
REL = 1e-10


def test_patch_weights_are_the_references():
    assert torch.equal(M.patch_weights().flatten(), torch.tensor(GOLD["patch_weights"], dtype=torch.float64))
    assert GOLD["config"] == {"non_local_region_size": M.NL, "patch_size": M.PATCH, "neighbor_size": M.NBR,
                              "gaussian_patch_sigma": M.SIGMA}


@pytest.mark.parametrize("name", sorted(GOLD["cases"]))
def test_restatement_matches_reference_vectors(name):
    c = GOLD["cases"][name]
    X, Y = _t64(c["x"], c["x_shape"]), _t64(c["y"], c["y_shape"])
    fx, fy = M.descriptor(X), M.descriptor(Y)
    assert fx.shape == (c["x_shape"][0], 81, *c["x_shape"][2:])
    loss = GOLD["lambda_structure"] * M.structure_l1(X, Y)
    assert float(loss) == pytest.approx(c["loss"], rel=REL, abs=0)
    for f, key in ((fx, "channel_sums_x"), (fy, "channel_sums_y")):
        want = torch.tensor(c[key], dtype=torch.float64)
        assert float(((f.sum(dim=(0, 2, 3)) - want).abs() / want).max()) <= REL, key
    if "features_x" in c:          # every element, hence also the channel order
        want = _t64(c["features_x"], fx.shape)
        assert float(((fx - want).abs() / want.abs()).max()) <= REL
    for f, key in ((fx, "feature_samples_x"), (fy, "feature_samples_y")):
        for i, v in c.get(key, ()):
            assert float(f.flatten()[i]) == pytest.approx(v, rel=REL, abs=0), (key, i)


def test_multi_channel_inputs_are_reduced_by_their_mean():
    X = M._random((2, 3, 9, 11), 5).double()
    assert torch.equal(M.descriptor(X), M.descriptor(X.mean(dim=1, keepdim=True)))
    with pytest.raises(ValueError):
        M.descriptor(torch.zeros(1, 1, 4, 8, 8))


# ---- config and loss names ---------------------------------------------------------------------------------------------
def test_stock_yamls_load_and_lambda_structure_defaults_to_zero():
    for path in (CONFIGS / "cyclegan_synthetic.yaml", Path(__file__).parent / "golden" / "horse2zebra_default.yaml"):
        conf = build_conf([f"config={path}", "train.batch_size=2"])
        assert conf.train.gan.optimizer.lambda_structure == 0
    conf = build_conf([f"config={CONFIGS / 'cyclegan_synthetic.yaml'}", *STRUCTURE])
    assert conf.train.gan.optimizer.lambda_structure == 0.5


@pytest.fixture()
def mind_backend():
    ops = RecordingOps(act_dtype=torch.float32)
    backend.set_ops(ops)
    yield ops
    backend.set_ops(None)


class RecordingOps(M.MindRefOps):
    """the CPU ops with every gs_sum2_f32 call written down"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.sums = []

    def sum2(self, a, b):
        out = super().sum2(a, b)
        self.sums.append((a.detach().clone(), b.detach().clone(), out.detach().clone()))
        return out


def test_loss_names_follow_lambda_structure(mind_backend):
    c = dict(load_golden_steps()["c64_default"]["config"])
    assert list(build_product_cyclegan(c).losses) == STOCK_NAMES
    assert list(build_product_cyclegan(c, ("train.gan.optimizer.lambda_structure=0",)).losses) == STOCK_NAMES
    assert list(build_product_cyclegan(c, STRUCTURE).losses) == STOCK_NAMES + ["structure_AB", "structure_BA"]


def test_off_the_step_is_the_stock_step(mind_backend):
    c = dict(load_golden_steps()["c64_default"]["config"])
    model = build_product_cyclegan(c)
    A, B = golden_inputs(c, 0)
    model.set_input({"A": A, "B": B})
    model.optimize_parameters()
    assert "structure_AB" not in model.losses and "structure_BA" not in model.losses
    assert len(mind_backend.sums) == 2          # one join per generated image: discriminator + other generator
    assert model._structure_fakes == {}


def test_backend_without_the_kernels_is_refused():
    from ganslate_amd.nn.losses.structure_loss import MINDDescriptor, StructureLoss
    backend.set_ops(RefOps(act_dtype=torch.float32))
    try:
        X = M._random((1, 1, 8, 8), 1)
        with pytest.raises(NotImplementedError, match="MIND"):
            StructureLoss(0.5)(X, X.clone().requires_grad_())
        with pytest.raises(NotImplementedError, match="MIND"):
            MINDDescriptor()(X)
    finally:
        backend.set_ops(None)


def test_volumes_are_refused_before_any_kernel(mind_backend):
    from ganslate_amd.nn.losses.structure_loss import MINDDescriptor, StructureLoss
    V = torch.zeros(1, 1, 4, 8, 8)
    with pytest.raises(ValueError):
        StructureLoss(0.5)(V, V)
    with pytest.raises(ValueError):
        MINDDescriptor()(V)


def test_recipe_adds_the_terms_and_joins_three_gradients(mind_backend):
    """64 x 64 product CycleGAN with lambda_structure = 0.5 on the CPU ops: structure_AB is lambda_AB * lambda_structure * the
    restatement on the step's own real_A / fake_B, and the gradient that reaches fake_B is the sum of its three consumers'
    gradients (discriminator, structure term, other generator), joined by two gs_sum2_f32 calls."""
    c = dict(load_golden_steps()["c64_default"]["config"])
    model = build_product_cyclegan(c, STRUCTURE)
    opt = model.conf.train.gan.optimizer
    A, B = golden_inputs(c, 0)
    model.set_input({"A": A, "B": B})
    model.optimize_parameters()
    v = {k: t.detach().float() for k, t in model.visuals.items() if t is not None}
    for name, lam, real, fake in (("structure_AB", opt.lambda_AB, "real_A", "fake_B"),
                                  ("structure_BA", opt.lambda_BA, "real_B", "fake_A")):
        want = lam * 0.5 * float(M.structure_l1(v[real], v[fake]))
        assert want > 0 and float(model.losses[name].detach()) == pytest.approx(want, rel=1e-5), name
    assert len(mind_backend.sums) == 4
    for lam, real, fake in ((opt.lambda_AB, "real_A", "fake_B"), (opt.lambda_BA, "real_B", "fake_A")):
        Y = v[fake].clone().requires_grad_()
        (g_structure,) = torch.autograd.grad(lam * 0.5 * M.structure_l1(v[real], Y), Y)
        inner = [s for s in mind_backend.sums
                 if any(torch.allclose(t, g_structure, rtol=1e-4, atol=1e-6 * float(g_structure.abs().max())) for t in s[:2])]
        assert len(inner) == 1, fake
        a, b, joined = inner[0]
        outer = [s for s in mind_backend.sums if any(torch.equal(t, joined) for t in s[:2])]
        assert len(outer) == 1, fake
        third = outer[0][1] if torch.equal(outer[0][0], joined) else outer[0][0]
        assert float(third.abs().max()) > 0 and float(a.abs().max()) > 0 and float(b.abs().max()) > 0
        assert torch.equal(outer[0][2], (a + b) + third) or torch.equal(outer[0][2], third + (a + b))


# ---- the yardstick of the GPU tolerances --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.CASES))
def test_gpu_cases_are_well_conditioned_and_their_bounds_see_a_wrong_tap_or_border(name):
    """From float64 alone: (i) one fp32 evaluation of the formulas lies within 1e-3 of the quantity's magnitude, so the input
    is well conditioned; (ii) two deliberately wrong variants — edge replication instead of zeros, one patch weight left
    out — lie more than 100 e32 away from float64 in descriptor, loss and gradient: the 4 e32 the GPU tests allow cannot
    hide either."""
    ref = M.reference(name)
    for what in ("feat", "loss", "grad"):
        assert ref["max"][what] > 0
        assert ref["e32"][what] <= 1e-3 * ref["max"][what], (what, ref["e32"][what], ref["max"][what])
    for wrong in (dict(border="clamp"), dict(drop_tap=(0, 0))):
        f, loss, gx, gy = M.loss_and_grads(ref["X"], ref["Y"], torch.float64, **wrong)
        off = {"feat": float((f - ref["feat_x"]).abs().max()), "loss": float((loss - ref["loss"]).abs()),
               "grad": float(max((gx - ref["grad_x"]).abs().max(), (gy - ref["grad_y"]).abs().max()))}
        for what, d in off.items():
            assert d > 100 * ref["e32"][what], (wrong, what, d, ref["e32"][what])


def test_constant_pair_is_finite():
    """two different constant images: where every difference vanishes V = 0 and D = 0, n = exp(-0 / 1e-8) = 1 — loss and
    gradient stay finite (no comparison of gradients here: the fp32 evaluation alone is 100 % off on this input)"""
    X, Y = M.CONSTANT_PAIR()
    for dtype in (torch.float64, torch.float32):
        for t in M.loss_and_grads(X, Y, dtype):
            assert bool(torch.isfinite(t).all())
