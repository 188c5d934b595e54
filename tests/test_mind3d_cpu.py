"""The volumetric structure-consistency (MIND) loss without a GPU: the float64 restatement of tests/mind3d_ref.py against a
second, convolution-based formulation (the reference has no volumetric MIND to record vectors from), the yardstick that
the GPU tolerances of tests/test_mind3d_gpu.py stand on, the new classes' refusals, the config field and the recipe wiring
of a 3-D CycleGAN on the CPU ops."""
import pytest
import torch
import torch.nn.functional as TF

from ganslate_amd.nn.native import backend
from oracle.ops_ref import RefOps

from . import mind3d_ref as M
from .helpers import build_product_cyclegan3d, load_golden_volumes, volume_inputs

F64 = torch.float64
STRUCTURE = ("train.gan.optimizer.lambda_structure=0.5",)
STOCK_NAMES = ["G_AB", "D_B", "cycle_A", "idt_A", "G_BA", "D_A", "cycle_B", "idt_B"]
SMALLEST_RESNET3D = "v16x24x32_idt"          # 3 residual blocks at 16 x 24 x 32, batch 2


# ---- the restatement against a second formulation ----------------------------------------------------------------------
def _descriptor_by_convolution(img, sigma=M.SIGMA):
    """The same definition from conv3d instead of slices: the shifted volumes come from one-hot 3x3x3 kernels, the patch
    sums from a depthwise 5x5x5 convolution of the volumes masked to the inside (conv3d pads with zeros, which is the
    `p+q inside` rule for d_a^2 — zeroed where r is outside by construction — and for the shifted volumes alike)."""
    I = (img.mean(dim=1) if img.shape[1] > 1 else img[:, 0])[:, None]                 # [N, 1, D, H, W]
    onehot = torch.zeros(27, 1, 3, 3, 3, dtype=I.dtype)
    for i in range(27):
        onehot[i, 0, i % 3, (i // 3) % 3, i // 9] = 1
    S = TF.conv3d(I, onehot, padding=1)                                               # S_a(r) = I(r + a), zero outside
    d2 = (S - I) ** 2
    q = torch.arange(5, dtype=torch.float32) - 2
    dist = (q[:, None, None] ** 2 + q[None, :, None] ** 2 + q[None, None, :] ** 2).sqrt()
    g = torch.exp((-dist / torch.tensor(sigma * sigma, dtype=torch.float32)).to(F64)).float().to(I.dtype)
    Dm = TF.conv3d(d2, g[None, None].repeat(27, 1, 1, 1, 1), padding=2, groups=27)
    B = TF.conv3d(S, torch.ones(27, 1, 5, 5, 5, dtype=I.dtype), padding=2, groups=27)
    V = B.var(dim=1, unbiased=True, keepdim=True)
    n = torch.exp(-Dm / (V + M.EPS))
    return n / n.sum(dim=1, keepdim=True)


def test_patch_weights_are_rounded_as_the_2d_ones():
    g = M.patch_weights()
    assert g.shape == (5, 5, 5) and float(g[2, 2, 2]) == 1.0
    assert torch.equal(g, g.flip(0)) and torch.equal(g, g.permute(2, 0, 1))
    assert torch.equal(g.float().double(), g)          # stored as fp32
    # |q| = 2 along one axis: exp(-2 / 4) evaluated in double from fp32 operands
    assert float(g[0, 2, 2]) == float(torch.tensor(-0.5, dtype=F64).exp().float())


def test_restatement_matches_the_convolution_formulation():
    """1e-10 relative, as tests/test_mind_cpu.py allows between two float64 evaluations of one formula (a patch sum has 125
    terms, exp(-t) carries t's error times t)"""
    X, Y = M.CASES["odd_2x1x5x11x13"]()
    for img in (X.to(F64), Y.to(F64), torch.cat([X, Y, X * Y], dim=1).to(F64)):
        f, want = M.descriptor(img), _descriptor_by_convolution(img)
        assert f.shape == (img.shape[0], 27, *img.shape[2:])
        assert float(((f - want).abs() / want.abs()).max()) <= 1e-10


def test_channel_order_depth_runs_fastest():
    """One bright voxel c in an empty 7^3 volume: d_a is non-zero at r = c - a and at r = c only. For an axis shift a the
    patch of p = c - 3a reaches c - a (distance 2) but not c, so D_a(p) = g(2) > 0, while for the opposite shift both
    voxels (c + a and c) lie outside that patch and D_{-a}(p) = 0: f_a(p) < f_{-a}(p). Channel of (dz, dy, dx) is
    (dz + 1) + 3 (dy + 1) + 9 (dx + 1)."""
    I = torch.zeros(1, 1, 7, 7, 7, dtype=F64)
    I[0, 0, 3, 3, 3] = 1.0
    f = M.descriptor(I)[0]
    ch = lambda dz, dy, dx: (dz + 1) + 3 * (dy + 1) + 9 * (dx + 1)      # noqa: E731
    assert f[ch(1, 0, 0), 0, 3, 3] < f[ch(-1, 0, 0), 0, 3, 3] and f[ch(-1, 0, 0), 6, 3, 3] < f[ch(1, 0, 0), 6, 3, 3]
    assert f[ch(0, 1, 0), 3, 0, 3] < f[ch(0, -1, 0), 3, 0, 3] and f[ch(0, -1, 0), 3, 6, 3] < f[ch(0, 1, 0), 3, 6, 3]
    assert f[ch(0, 0, 1), 3, 3, 0] < f[ch(0, 0, -1), 3, 3, 0] and f[ch(0, 0, -1), 3, 3, 6] < f[ch(0, 0, 1), 3, 3, 6]


def test_multi_channel_inputs_are_reduced_by_their_mean():
    X = M._random((2, 3, 4, 6, 7), 5).double()
    assert torch.equal(M.descriptor(X), M.descriptor(X.mean(dim=1, keepdim=True)))
    with pytest.raises(ValueError):
        M.descriptor(torch.zeros(1, 1, 8, 8))


@pytest.mark.parametrize("name", ["tiny_1x1x2x3x5", "odd_2x1x5x11x13", "ball_1x1x10x20x22"])
def test_loss_is_flip_invariant_in_float64(name):
    """zero borders, symmetric weights and shift sets: flipping both volumes along one axis permutes the summands of L and
    nothing else — the basis of the loss yardstick (mind3d_ref.loss_e32). 1e-12 relative: the sum has up to 1e5 terms."""
    X, Y = (t.to(F64) for t in M.CASES[name]())
    want = float(M.structure_l1(X, Y))
    for f in M.FLIPS[1:]:
        assert float(M.structure_l1(X.flip(f), Y.flip(f))) == pytest.approx(want, rel=1e-12, abs=0), f


# ---- the yardstick of the GPU tolerances --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.CASES))
def test_gpu_cases_are_well_conditioned_and_their_bounds_see_a_wrong_tap_or_border(name):
    """From float64 alone: (i) one fp32 evaluation of the formulas lies within 1e-3 of the quantity's magnitude, so the input
    is well conditioned; (ii) the deliberately wrong variants the case can see (mind3d_ref.VISIBLE_WRONG: edge replication
    instead of zeros everywhere; one patch weight left out wherever the depth lets that tap land inside) lie more than
    100 e32 away from float64 in descriptor, loss and gradient: the 4 e32 the GPU tests allow cannot hide either."""
    ref = M.reference(name)
    for what in ("feat", "loss", "grad"):
        assert ref["max"][what] > 0
        assert ref["e32"][what] <= 1e-3 * ref["max"][what], (what, ref["e32"][what], ref["max"][what])
    for wrong in M.VISIBLE_WRONG[name]:
        f, loss, gx, gy = M.loss_and_grads(ref["X"], ref["Y"], F64, **wrong)
        off = {"feat": float((f - ref["feat_x"]).abs().max()), "loss": float((loss - ref["loss"]).abs()),
               "grad": float(max((gx - ref["grad_x"]).abs().max(), (gy - ref["grad_y"]).abs().max()))}
        for what, d in off.items():
            print(f"{name} {wrong} {what}: {d / ref['e32'][what]:.3g} e32")
            assert d > 100 * ref["e32"][what], (wrong, what, d, ref["e32"][what])


def test_the_tap_tiny_cannot_see_changes_nothing_there():
    ref = M.reference("tiny_1x1x2x3x5")
    f, loss, gx, gy = M.loss_and_grads(ref["X"], ref["Y"], F64, drop_tap=M.WRONG_TAP)
    assert torch.equal(f, ref["feat_x"]) and torch.equal(loss, ref["loss"]) and torch.equal(gy, ref["grad_y"])


def test_constant_pair_is_finite():
    """two different constant volumes: where every difference vanishes V = 0 and D = 0, n = exp(-0 / 1e-8) = 1 — loss and
    gradient stay finite (no comparison of gradients here: the fp32 evaluation alone is 100 % off on this input)"""
    X, Y = M.CONSTANT_PAIR()
    for dtype in (torch.float64, torch.float32):
        for t in M.loss_and_grads(X, Y, dtype):
            assert bool(torch.isfinite(t).all())


# ---- classes, config and loss names -------------------------------------------------------------------------------------
class RecordingOps(M.Mind3dRefOps):
    """the CPU ops with every gs_sum2_f32 call written down"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.sums = []

    def sum2(self, a, b):
        out = super().sum2(a, b)
        self.sums.append((a.detach().clone(), b.detach().clone(), out.detach().clone()))
        return out


@pytest.fixture()
def mind3d_backend():
    ops = RecordingOps(act_dtype=torch.float32)
    backend.set_ops(ops)
    yield ops
    backend.set_ops(None)


def test_classes_are_exported_next_to_the_2d_ones():
    from ganslate_amd.nn.losses import structure_loss as S
    assert S.MIND3D_DESCRIPTOR_CONFIG == {"non_local_region_size": M.NL, "patch_size": M.PATCH, "neighbor_size": M.NBR,
                                          "gaussian_patch_sigma": M.SIGMA}
    assert S.MINDDescriptor3D().config == S.MIND3D_DESCRIPTOR_CONFIG
    with pytest.raises(TypeError):
        S.MINDDescriptor3D(radius=2)
    from ganslate_amd.hip.ops import HipOps
    assert HipOps.MIND3D_CONFIG == S.MIND3D_DESCRIPTOR_CONFIG
    for m in ("mind3d_descriptor", "mind3d_l1", "mind3d_l1_backward"):
        assert callable(getattr(HipOps, m))


def test_entry_points_refuse_bad_arguments_in_host_code():
    """the refusals of the four C entry points come before any launch, so they answer without a GPU: null pointers, sizes
    other than 3 / 5 / 3, non-positive extents, a sample of 2^31 voxels, 2^31 workgroups (one per 4 x 8 x 8 box)"""
    import ctypes
    from ganslate_amd.hip import lib as L
    if not L.library_path().is_file():
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)          # never dereferenced: every call below is refused first

    def refused(rc, words):
        assert rc != 0
        msg = lib.gs_last_error().decode()
        assert words in msg, msg

    refused(lib.gs_mind3d_descriptor(None, 1, 1, 4, 8, 8, 3, 5, 3, 2.0, p, None), "bad argument")
    refused(lib.gs_mind3d_l1(p, None, 1, 1, 1, 4, 8, 8, 3, 5, 3, 2.0, p, p, None), "bad argument")
    refused(lib.gs_mind3d_l1(p, p, 1, 1, 1, 4, 8, 8, 3, 5, 3, 2.0, p, None, None), "bad argument")
    refused(lib.gs_mind3d_l1_backward(p, p, 1, 1, 1, 4, 8, 8, 3, 5, 3, 2.0, None, None, p, None), "bad argument")
    for sizes in ((9, 7, 3), (3, 7, 3), (3, 5, 5), (5, 5, 3)):
        refused(lib.gs_mind3d_l1(p, p, 1, 1, 1, 4, 8, 8, *sizes, 2.0, p, p, None), "patch_size 5")
        refused(lib.gs_mind3d_descriptor(p, 1, 1, 4, 8, 8, *sizes, 2.0, p, None), "patch_size 5")
        refused(lib.gs_mind3d_l1_backward(p, p, 1, 1, 1, 4, 8, 8, *sizes, 2.0, None, p, p, None), "patch_size 5")
    for ext in ((0, 1, 4, 8, 8), (1, 0, 4, 8, 8), (1, 1, 0, 8, 8), (1, 1, 4, -1, 8), (1, 1, 4, 8, 0)):
        N, Cc, D, H, W = ext
        refused(lib.gs_mind3d_descriptor(p, N, Cc, D, H, W, 3, 5, 3, 2.0, p, None), "bad argument")
        refused(lib.gs_mind3d_l1(p, p, N, Cc, Cc, D, H, W, 3, 5, 3, 2.0, p, p, None), "bad argument")
    refused(lib.gs_mind3d_l1(p, p, 1, 1, 1, 4, 8, 8, 3, 5, 3, 0.0, p, p, None), "bad argument")
    refused(lib.gs_mind3d_l1(p, p, 1, 1, 1, 2048, 1024, 1024, 3, 5, 3, 2.0, p, p, None), "2^31 or more voxels")
    refused(lib.gs_mind3d_l1_backward(p, p, 1, 1, 1, 2048, 1024, 1024, 3, 5, 3, 2.0, None, p, p, None), "2^31 or more voxels")
    # 512 x 8 x 8 voxels = 128 boxes per sample: 2^24 samples are 2^31 boxes, one fewer sample is not refused for its grid
    refused(lib.gs_mind3d_descriptor(p, 1 << 24, 1, 512, 8, 8, 3, 5, 3, 2.0, p, None), "too many boxes")
    assert lib.gs_mind3d_scratch_bytes(2, 5, 11, 13, 0) == 2 * 2 * 2 * 2 * 4          # one fp32 partial per box
    assert lib.gs_mind3d_scratch_bytes(2, 5, 11, 13, 1) == 2 * 81 * 5 * 11 * 13 * 4   # 81 volumes per sample
    assert lib.gs_mind3d_scratch_bytes(0, 5, 11, 13, 1) == 0


def test_images_are_refused_before_any_kernel(mind3d_backend):
    from ganslate_amd.nn.losses.functional import mind3d_structure_autograd
    from ganslate_amd.nn.losses.structure_loss import MINDDescriptor3D, StructureLoss3D
    I = torch.zeros(1, 1, 8, 8)
    with pytest.raises(ValueError):
        StructureLoss3D(0.5)(I, I)
    with pytest.raises(ValueError):
        MINDDescriptor3D()(I)
    with pytest.raises(ValueError):
        mind3d_structure_autograd(I, I)


def test_backend_without_the_kernels_is_refused():
    from ganslate_amd.nn.losses.structure_loss import MINDDescriptor3D, StructureLoss3D
    backend.set_ops(RefOps(act_dtype=torch.float32))
    try:
        X = M._random((1, 1, 3, 4, 5), 1)
        with pytest.raises(NotImplementedError, match="MIND"):
            StructureLoss3D(0.5)(X, X.clone().requires_grad_())
        with pytest.raises(NotImplementedError, match="MIND"):
            MINDDescriptor3D()(X)
    finally:
        backend.set_ops(None)


def test_classes_compute_the_restatement_on_the_cpu_ops(mind3d_backend):
    from ganslate_amd.nn.losses.structure_loss import MINDDescriptor3D, StructureLoss3D
    X, Y = M.CASES["tiny_1x1x2x3x5"]()
    assert torch.equal(MINDDescriptor3D()(X), M.descriptor(X))
    Yg = Y.clone().requires_grad_()
    loss = StructureLoss3D(0.5)(X, Yg)
    loss.backward()
    _, l32, _, gy32 = M.loss_and_grads(X, Y, torch.float32)
    assert float(loss.detach()) == pytest.approx(0.5 * float(l32), rel=1e-6)
    assert torch.allclose(Yg.grad, 0.5 * gy32, rtol=1e-5, atol=1e-9)


def test_config_field_reaches_a_3d_cyclegan_and_names_follow_it(mind3d_backend):
    from ganslate_amd.nn.losses.structure_loss import StructureLoss3D
    c = dict(load_golden_volumes()["steps"][SMALLEST_RESNET3D]["config"])
    off = build_product_cyclegan3d(c)
    assert list(off.losses) == STOCK_NAMES and not off.criterion_G.is_using_structure()
    assert list(build_product_cyclegan3d(c, ("train.gan.optimizer.lambda_structure=0",)).losses) == STOCK_NAMES
    on = build_product_cyclegan3d(c, STRUCTURE)
    assert on.conf.train.gan.optimizer.lambda_structure == 0.5
    assert list(on.losses) == STOCK_NAMES + ["structure_AB", "structure_BA"]
    assert on.criterion_G.is_using_structure()
    V = torch.zeros(1, 1, 2, 3, 4)
    assert type(on.criterion_G._structure_criterion(V)) is StructureLoss3D
    assert on.criterion_G._structure_criterion(V).lambda_structure == 0.5


def test_balanced_recipe_keeps_refusing_lambda_structure():
    import inspect
    from ganslate_amd.nn.gans.unpaired import cyclegan_balanced
    assert '"lambda_structure"' in inspect.getsource(cyclegan_balanced)


@pytest.mark.parametrize("twin", ["1", "0"])
def test_recipe_adds_the_terms_and_joins_three_gradients(mind3d_backend, monkeypatch, twin):
    """The smallest Resnet3D product CycleGAN with lambda_structure = 0.5 on the CPU ops, as twin passes and as two passes
    (GS_TWIN=0): structure_AB is lambda_AB * lambda_structure * the restatement on the step's own real_A / fake_B, and the
    gradient that reaches fake_B is the sum of its three consumers' gradients (discriminator, structure term, other
    generator), joined by two gs_sum2_f32 calls."""
    monkeypatch.setenv("GS_TWIN", twin)
    c = dict(load_golden_volumes()["steps"][SMALLEST_RESNET3D]["config"])
    model = build_product_cyclegan3d(c, STRUCTURE)
    assert (model.twin_G is not None) == (twin == "1")
    opt = model.conf.train.gan.optimizer
    A, B = volume_inputs(c, 0)
    model.set_input({"A": A, "B": B})
    model.optimize_parameters()
    v = {k: t.detach().float() for k, t in model.visuals.items() if t is not None}
    assert v["fake_B"].dim() == 5
    for name, lam, real, fake in (("structure_AB", opt.lambda_AB, "real_A", "fake_B"),
                                  ("structure_BA", opt.lambda_BA, "real_B", "fake_A")):
        want = lam * 0.5 * float(M.structure_l1(v[real], v[fake]))
        assert want > 0 and float(model.losses[name].detach()) == pytest.approx(want, rel=1e-5), name
    assert len(mind3d_backend.sums) == 4
    for lam, real, fake in ((opt.lambda_AB, "real_A", "fake_B"), (opt.lambda_BA, "real_B", "fake_A")):
        Y = v[fake].clone().requires_grad_()
        (g_structure,) = torch.autograd.grad(lam * 0.5 * M.structure_l1(v[real], Y), Y)
        inner = [s for s in mind3d_backend.sums
                 if any(t.shape == g_structure.shape and
                        torch.allclose(t, g_structure, rtol=1e-4, atol=1e-6 * float(g_structure.abs().max())) for t in s[:2])]
        assert len(inner) == 1, fake
        a, b, joined = inner[0]
        outer = [s for s in mind3d_backend.sums if any(torch.equal(t, joined) for t in s[:2])]
        assert len(outer) == 1, fake
        third = outer[0][1] if torch.equal(outer[0][0], joined) else outer[0][0]
        assert float(third.abs().max()) > 0 and float(a.abs().max()) > 0 and float(b.abs().max()) > 0
        assert torch.equal(outer[0][2], (a + b) + third) or torch.equal(outer[0][2], third + (a + b))


def test_off_the_volume_step_is_the_stock_step(mind3d_backend, monkeypatch):
    calls = []
    for m in ("mind3d_descriptor", "mind3d_l1", "mind3d_l1_backward"):
        monkeypatch.setattr(type(mind3d_backend), m, lambda self, *a, _m=m, **k: calls.append(_m))
    c = dict(load_golden_volumes()["steps"][SMALLEST_RESNET3D]["config"])
    model = build_product_cyclegan3d(c)
    A, B = volume_inputs(c, 0)
    model.set_input({"A": A, "B": B})
    model.optimize_parameters()
    assert calls == [] and "structure_AB" not in model.losses
    assert len(mind3d_backend.sums) == 2          # one join per generated volume: discriminator + other generator
    assert model._structure_fakes == {}
