"""The volumetric MIND structure-consistency kernels (csrc/mind3d.hip) on the GPU against the float64 restatement of
tests/mind3d_ref.py.

Tolerance of every comparison: 4 e32 + one fp32 ulp of the quantity's maximum (mind3d_ref.bound), e32 being the distance
of the float32 restatement from float64 on that very input; for the scalar loss the largest such distance over the case
and its three single-axis flips, which are the same sum in another order (mind3d_ref.loss_e32). The kernel and the float32
restatement are two fp32 evaluations of one formula that differ in summation order and in the exp implementation; the
factor 4 covers the spread between two such evaluations, and tests/test_mind3d_cpu.py shows per case that a wrong tap or
border rule lies beyond 100 e32."""
import random

import pytest
import torch

from . import mind3d_ref as M
from .helpers import build_product_cyclegan3d, load_golden_volumes, volume_inputs

pytestmark = pytest.mark.gpu

STRUCTURE = ("train.gan.optimizer.lambda_structure=0.5",)
SMALLEST_RESNET3D = "v16x24x32_idt"          # 3 residual blocks at 16 x 24 x 32, batch 2
F64 = torch.float64


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _err(got, want):
    assert bool(torch.isfinite(got).all()), "NaN left in the output: an element was not written"
    return float((got.detach().cpu().to(F64) - want).abs().max())


@pytest.mark.parametrize("name", list(M.CASES))
def test_descriptor_matches_float64(hip_ops, name):
    ref = M.reference(name)
    dev = hip_ops.device
    for img, want in ((ref["X"], ref["feat_x"]), (ref["Y"], ref["feat_y"])):
        x = img.to(dev)
        out = _nan((x.shape[0], 27, *x.shape[2:]), dev)
        hip_ops.mind3d_descriptor(x, out=out)
        again = _nan(out.shape, dev)
        hip_ops.mind3d_descriptor(x, out=again)
        e, b = _err(out, want), M.bound(ref, "feat")
        print(f"{name}: descriptor error {e:.3e}, bound {b:.3e} (e32 {ref['e32']['feat']:.3e})")
        assert e <= b
        assert torch.equal(out, again), "two calls differ"


@pytest.mark.parametrize("name", list(M.CASES))
def test_loss_and_both_gradients_match_float64(hip_ops, name):
    ref = M.reference(name)
    dev = hip_ops.device
    X, Y = ref["X"].to(dev), ref["Y"].to(dev)
    scale = torch.tensor(M.GRAD_SCALE, dtype=torch.float32, device=dev)          # the upstream gradient: a device scalar
    runs = []
    for _ in range(2):
        loss, gx, gy = _nan((), dev), _nan(X.shape, dev), _nan(Y.shape, dev)
        hip_ops.mind3d_l1(X, Y, loss)
        hip_ops.mind3d_l1_backward(X, Y, gy, grad_scale=scale)
        hip_ops.mind3d_l1_backward(Y, X, gx, grad_scale=scale)        # symmetric: the other side with the arguments swapped
        runs.append((loss, gx, gy))
    loss, gx, gy = runs[0]
    e, b = _err(loss, ref["loss"]), M.bound(ref, "loss")
    print(f"{name}: loss error {e:.3e}, bound {b:.3e} (e32 {ref['e32']['loss']:.3e}, loss {float(ref['loss']):.6e})")
    eg = max(_err(gx, M.GRAD_SCALE * ref["grad_x"]), _err(gy, M.GRAD_SCALE * ref["grad_y"]))
    bg = M.GRAD_SCALE * M.bound(ref, "grad")
    print(f"{name}: gradient error {eg:.3e}, bound {bg:.3e} (e32 {ref['e32']['grad']:.3e}, max {ref['max']['grad']:.3e})")
    assert e <= b
    assert eg <= bg
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c), "two calls differ"


def test_autograd_function_asks_only_for_the_needed_side(hip_ops, monkeypatch):
    from ganslate_amd.nn.losses.functional import mind3d_structure_autograd
    ref = M.reference("odd_2x1x5x11x13")
    dev = hip_ops.device
    calls = []
    real = type(hip_ops).mind3d_l1_backward
    monkeypatch.setattr(type(hip_ops), "mind3d_l1_backward", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    X, Y = ref["X"].to(dev), ref["Y"].to(dev).requires_grad_()
    loss = mind3d_structure_autograd(X, Y)
    (2.0 * loss).backward()
    assert len(calls) == 1 and X.grad is None
    assert _err(loss, ref["loss"]) <= M.bound(ref, "loss")
    assert _err(Y.grad, 2.0 * ref["grad_y"]) <= 2.0 * M.bound(ref, "grad")


def test_constant_pair_is_finite(hip_ops):
    X, Y = (t.to(hip_ops.device) for t in M.CONSTANT_PAIR())
    loss, gy = _nan((), hip_ops.device), _nan(Y.shape, hip_ops.device)
    hip_ops.mind3d_l1(X, Y, loss)
    hip_ops.mind3d_l1_backward(X, Y, gy)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(gy).all())


def test_bad_arguments_raise_before_any_launch(hip_ops):
    from ganslate_amd.hip.lib import HipError
    dev = hip_ops.device
    x = torch.zeros((1, 1, 4, 8, 9), device=dev)
    out = torch.zeros((), device=dev)
    with pytest.raises(ValueError):
        hip_ops.mind3d_descriptor(torch.zeros((1, 1, 8, 9), device=dev))                       # rank
    with pytest.raises(ValueError):
        hip_ops.mind3d_descriptor(x, out=torch.zeros((1, 81, 4, 8, 9), device=dev))            # the 2-D channel count
    with pytest.raises(ValueError):
        hip_ops.mind3d_l1(x, torch.zeros((1, 1, 4, 8, 10), device=dev), out)                   # extent
    with pytest.raises(ValueError):
        hip_ops.mind3d_l1(x, torch.zeros((1, 1, 5, 8, 9), device=dev), out)
    with pytest.raises(ValueError):
        hip_ops.mind3d_l1(x, x.double(), out)                                                  # dtype
    with pytest.raises(ValueError):
        hip_ops.mind3d_l1(x, torch.zeros((1, 1, 4, 9, 8), device=dev).transpose(3, 4), out)    # stride
    with pytest.raises(ValueError):
        hip_ops.mind3d_l1_backward(x, x, torch.zeros((1, 2, 4, 8, 9), device=dev))
    with pytest.raises(HipError, match="patch_size 5"):
        hip_ops.mind3d_l1(x, x, out, cfg={"patch_size": 7})
    with pytest.raises(HipError, match="patch_size 5"):
        hip_ops.mind3d_descriptor(x, cfg={"patch_size": 7})
    with pytest.raises(HipError, match="patch_size 5"):
        hip_ops.mind3d_l1_backward(x, x, torch.zeros_like(x), cfg={"patch_size": 7})
    # the 2-D entry points keep refusing volumes
    with pytest.raises(ValueError):
        hip_ops.mind_l1(x, x, out)


# ---- the recipe ---------------------------------------------------------------------------------------------------------
def _run(model, c, n_steps):
    random.seed(c["seed"])
    out = []
    for s in range(n_steps):
        A, B = volume_inputs(c, s)
        model.set_input({"A": A, "B": B})
        model.optimize_parameters()
        _, losses, visuals, _ = model.get_loggable_data()
        torch.cuda.synchronize()
        out.append(({k: float(v.detach()) for k, v in losses.items() if v is not None},
                    {k: visuals[k].detach().float().cpu().clone() for k in ("real_A", "fake_B", "real_B", "fake_A")}))
        model.update_learning_rate()
    return out


def test_structure_step_replays_bit_for_bit_and_matches_float64(hip_ops):
    """lambda_structure = 0.5 on the smallest Resnet3D recipe: four launch-by-launch steps against four graph-replayed steps
    agree bit for bit on losses, fake_B and master weights; the two structure losses are finite and positive, and at step 0
    they are the float64 restatement on the volumes read back."""
    c = dict(load_golden_volumes()["steps"][SMALLEST_RESNET3D]["config"])
    c["pool_size"] = 3
    n_steps = 4
    eager = build_product_cyclegan3d(c, STRUCTURE)
    eager.step_graph_enabled = False
    want = _run(eager, c, n_steps)
    graphed = build_product_cyclegan3d(c, STRUCTURE)
    assert graphed.step_graph_enabled
    got = _run(graphed, c, n_steps)
    assert graphed._graph is not None, "the step was never captured"
    for s in range(n_steps):
        assert got[s][0] == want[s][0], s
        assert torch.equal(got[s][1]["fake_B"], want[s][1]["fake_B"]), s
        for k in ("structure_AB", "structure_BA"):
            assert want[s][0][k] > 0 and want[s][0][k] == want[s][0][k] and want[s][0][k] != float("inf"), (s, k)
    for name in eager.networks:
        assert torch.equal(eager.networks[name].master.detach(), graphed.networks[name].master.detach()), name
    assert want[0][1]["fake_B"].dim() == 5
    _assert_is_the_restatement(want[0][0], want[0][1], eager.conf.train.gan.optimizer, 0.5)


def _assert_is_the_restatement(losses, visuals, opt, lambda_structure):
    """structure_AB / structure_BA against float64 on the volumes read back: the kernel's bound on L (4 e32 over the pair
    and its flips + one ulp) times the weight, plus one rounding of the weighted value (gs_scalar_affine)"""
    for k, lam, real, fake in (("structure_AB", opt.lambda_AB, "real_A", "fake_B"),
                               ("structure_BA", opt.lambda_BA, "real_B", "fake_A")):
        X, Y = visuals[real].detach().float().cpu(), visuals[fake].detach().float().cpu()
        l64 = float(M.structure_l1(X.to(F64), Y.to(F64)))
        w = lam * lambda_structure
        b = w * (4 * M.loss_e32(X, Y) + l64 * 2.0 ** -23) + w * l64 * 2.0 ** -23
        print(f"{k}: {losses[k]:.8e} vs float64 {w * l64:.8e}, bound {b:.3e}")
        assert losses[k] > 0 and abs(losses[k] - w * l64) <= b, k


def test_separable_vnets_which_never_twin_route_the_structure_gradient(hip_ops, monkeypatch):
    """is_separable V-Nets run as two passes whatever GS_TWIN says: the nested fanout of that path carries the volumetric
    term too. One step of the small separable recipe of tests/test_separable_cpu.py with lambda_structure = 0.5: the two
    losses are the float64 restatement on the volumes read back, and the step differs from the stock one only by them."""
    from .test_separable_cpu import _cyclegan, _steps
    monkeypatch.setenv("GS_TWIN", "all")
    stock = _steps(_cyclegan(), 1)[0]
    model = _cyclegan(STRUCTURE)
    assert model.twin_G is None and model.networks["G_AB"].is_separable
    got = _steps(model, 1)[0]
    torch.cuda.synchronize()
    assert set(got) == set(stock) | {"structure_AB", "structure_BA"}
    for k, v in stock.items():          # same weights, same batch: the forward pass is the stock one
        assert got[k] == pytest.approx(v, rel=1e-6), k
    _assert_is_the_restatement(got, model.visuals, model.conf.train.gan.optimizer, 0.5)
    assert set(model._structure_fakes) == {"fake_B", "fake_A"}


def test_trainer_logs_the_two_structure_losses_on_volumes(hip_ops, tmp_path):
    """a 3-D CycleGAN config with lambda_structure > 0 through engines.init_engine: it used to die at its first step"""
    from ganslate_amd.engines import init_engine
    from .helpers import VOL_CONF
    tr = init_engine("train", [f"config={VOL_CONF}", f"train.output_dir={tmp_path}", "train.n_iters=2",
                               "train.n_iters_decay=1", "train.gan.generator.n_residual_blocks=2",
                               "train.dataset.final_size=[16,16,24]", "train.seed=3", *STRUCTURE])
    tr.run()
    torch.cuda.synchronize()
    assert len(tr.history) == 3
    for _, losses, _ in tr.history:
        assert all(v == v and abs(v) < 1e4 for v in losses.values()), losses
        assert losses["structure_AB"] > 0 and losses["structure_BA"] > 0


def test_off_nothing_of_mind3d_is_launched(hip_ops, monkeypatch):
    calls = []
    for m in ("mind3d_descriptor", "mind3d_l1", "mind3d_l1_backward"):
        monkeypatch.setattr(type(hip_ops), m, lambda self, *a, _m=m, **k: calls.append(_m))
    for name in ("gs_mind3d_descriptor", "gs_mind3d_l1", "gs_mind3d_l1_backward", "gs_mind3d_scratch_bytes"):
        assert hasattr(hip_ops.lib, name)
    c = dict(load_golden_volumes()["steps"][SMALLEST_RESNET3D]["config"])
    for extra in ((), ("train.gan.optimizer.lambda_structure=0",)):
        model = build_product_cyclegan3d(c, extra)
        got = _run(model, c, 2)
        assert calls == []
        assert not any(k.startswith("structure") for k in got[-1][0])
        assert "structure_AB" not in model.losses and model._structure_fakes == {}


def test_two_pass_forward_routes_the_structure_gradient_too(hip_ops, monkeypatch):
    """GS_TWIN=0: the generators run as separate passes, the second cycle on its own stream, and the nested fanout sits on
    that path as well. First-iteration losses against the twin-pass step, within the 2e-3 that tests/test_twin_gpu.py
    allows between the two forms; the generators' weights after the update stay as close as there."""
    c = dict(load_golden_volumes()["steps"][SMALLEST_RESNET3D]["config"])
    runs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GS_TWIN", mode)
        model = build_product_cyclegan3d(c, STRUCTURE)
        assert (model.twin_G is not None) == (mode == "1")
        out = _run(model, c, 1)
        runs[mode] = (out[0][0], {n: net.master.detach().float().cpu().clone() for n, net in model.networks.items()})
    assert "structure_AB" in runs["0"][0] and "structure_BA" in runs["0"][0]
    for k, v in runs["0"][0].items():
        assert runs["1"][0][k] == pytest.approx(v, rel=2e-3, abs=1e-5), k
    for n, w in runs["0"][1].items():
        assert (runs["1"][1][n] - w).abs().mean().item() <= 1e-4, n
