"""The MIND structure-consistency kernels (csrc/mind.hip) on the GPU against the float64 restatement of tests/mind_ref.py.

Tolerance of every comparison: 4 e32 + one fp32 ulp of the quantity's maximum, e32 being the distance of the float32
restatement from float64 on that very input (mind_ref.reference). The kernel and the float32 restatement are two fp32
evaluations of one formula that differ in summation order and in the exp implementation; the factor 4 covers the spread
between two such evaluations, and tests/test_mind_cpu.py shows per case that a wrong tap or border rule lies beyond
100 e32."""
import random

import pytest
import torch

from . import mind_ref as M
from .helpers import build_product_cyclegan, golden_inputs, load_golden_steps

pytestmark = pytest.mark.gpu

STRUCTURE = ("train.gan.optimizer.lambda_structure=0.5",)
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
        out = _nan((x.shape[0], 81, x.shape[2], x.shape[3]), dev)
        hip_ops.mind_descriptor(x, out=out)
        again = _nan(out.shape, dev)
        hip_ops.mind_descriptor(x, out=again)
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
        hip_ops.mind_l1(X, Y, loss)
        hip_ops.mind_l1_backward(X, Y, gy, grad_scale=scale)
        hip_ops.mind_l1_backward(Y, X, gx, grad_scale=scale)          # symmetric: the other side with the arguments swapped
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
    from ganslate_amd.nn.losses.functional import mind_structure_autograd
    ref = M.reference("odd_2x1x19x23")
    dev = hip_ops.device
    calls = []
    real = type(hip_ops).mind_l1_backward
    monkeypatch.setattr(type(hip_ops), "mind_l1_backward", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    X, Y = ref["X"].to(dev), ref["Y"].to(dev).requires_grad_()
    loss = mind_structure_autograd(X, Y)
    (2.0 * loss).backward()
    assert len(calls) == 1 and X.grad is None
    assert _err(loss, ref["loss"]) <= M.bound(ref, "loss")
    assert _err(Y.grad, 2.0 * ref["grad_y"]) <= 2.0 * M.bound(ref, "grad")


def test_constant_pair_is_finite(hip_ops):
    X, Y = (t.to(hip_ops.device) for t in M.CONSTANT_PAIR())
    loss, gy = _nan((), hip_ops.device), _nan(Y.shape, hip_ops.device)
    hip_ops.mind_l1(X, Y, loss)
    hip_ops.mind_l1_backward(X, Y, gy)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(gy).all())


def test_bad_arguments_raise_before_any_launch(hip_ops):
    from ganslate_amd.hip.lib import HipError
    dev = hip_ops.device
    x = torch.zeros((1, 1, 8, 9), device=dev)
    out = torch.zeros((), device=dev)
    with pytest.raises(ValueError):
        hip_ops.mind_descriptor(torch.zeros((1, 1, 4, 8, 9), device=dev))
    with pytest.raises(ValueError):
        hip_ops.mind_l1(x, torch.zeros((1, 1, 8, 10), device=dev), out)
    with pytest.raises(ValueError):
        hip_ops.mind_l1(x, x.double(), out)
    with pytest.raises(ValueError):
        hip_ops.mind_l1(x, torch.zeros((1, 1, 9, 8), device=dev).transpose(2, 3), out)
    with pytest.raises(ValueError):
        hip_ops.mind_l1_backward(x, x, torch.zeros((1, 2, 8, 9), device=dev))
    with pytest.raises(HipError, match="non_local_region_size 9"):
        hip_ops.mind_l1(x, x, out, cfg={"patch_size": 5})


# ---- the recipe ---------------------------------------------------------------------------------------------------------
def _run(model, c, n_steps):
    random.seed(c["seed"])
    out = []
    for s in range(n_steps):
        A, B = golden_inputs(c, s)
        model.set_input({"A": A, "B": B})
        model.optimize_parameters()
        _, losses, visuals, _ = model.get_loggable_data()
        torch.cuda.synchronize()
        out.append(({k: float(v.detach()) for k, v in losses.items() if v is not None},
                    {k: visuals[k].detach().float().cpu().clone() for k in ("real_A", "fake_B", "real_B", "fake_A")}))
        model.update_learning_rate()
    return out


def test_structure_step_replays_bit_for_bit_and_matches_float64(hip_ops):
    """lambda_structure = 0.5: four launch-by-launch steps against four graph-replayed steps agree bit for bit on losses,
    fake_B and master weights (as tests/test_step_graph_gpu.py asserts for the stock step); the two structure losses are
    finite and positive, and at step 0 they are the float64 restatement on the images read back."""
    c = dict(load_golden_steps()["c64_default"]["config"])
    c["pool_size"] = 3
    n_steps = 4
    eager = build_product_cyclegan(c, STRUCTURE)
    eager.step_graph_enabled = False
    want = _run(eager, c, n_steps)
    graphed = build_product_cyclegan(c, STRUCTURE)
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
    opt = eager.conf.train.gan.optimizer
    for k, lam, real, fake in (("structure_AB", opt.lambda_AB, "real_A", "fake_B"),
                               ("structure_BA", opt.lambda_BA, "real_B", "fake_A")):
        X, Y = want[0][1][real], want[0][1][fake]
        l64 = float(M.structure_l1(X.to(F64), Y.to(F64)))
        e32 = abs(float(M.structure_l1(X, Y)) - l64)
        w = lam * 0.5
        # the kernel's bound on L, times the weight, plus one rounding of the weighted value (gs_scalar_affine)
        b = w * (4 * e32 + l64 * 2.0 ** -23) + w * l64 * 2.0 ** -23
        print(f"{k}: {want[0][0][k]:.8e} vs float64 {w * l64:.8e}, bound {b:.3e}")
        assert abs(want[0][0][k] - w * l64) <= b, k


def test_off_nothing_of_mind_is_launched(hip_ops, monkeypatch):
    calls = []
    for m in ("mind_descriptor", "mind_l1", "mind_l1_backward"):
        monkeypatch.setattr(type(hip_ops), m, lambda self, *a, _m=m, **k: calls.append(_m))
    for name in ("gs_mind_descriptor", "gs_mind_l1", "gs_mind_l1_backward"):
        assert hasattr(hip_ops.lib, name)
    c = dict(load_golden_steps()["c64_default"]["config"])
    for extra in ((), ("train.gan.optimizer.lambda_structure=0",)):
        model = build_product_cyclegan(c, extra)
        got = _run(model, c, 2)
        assert calls == []
        assert not any(k.startswith("structure") for k in got[-1][0])
        assert "structure_AB" not in model.losses and model._structure_fakes == {}


def test_two_pass_forward_routes_the_structure_gradient_too(hip_ops, monkeypatch):
    """GS_TWIN=0: the generators run as separate passes, the second cycle on its own stream, and the nested fanout sits on
    that path as well. First-iteration losses against the twin-pass step, within the 2e-3 that
    tests/test_twin_gpu.py allows between the two forms; the generators' weights after the update stay as close as there."""
    c = dict(load_golden_steps()["c64_default"]["config"])
    runs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GS_TWIN", mode)
        model = build_product_cyclegan(c, STRUCTURE)
        assert (model.twin_G is not None) == (mode == "1")
        out = _run(model, c, 1)
        runs[mode] = (out[0][0], {n: net.master.detach().float().cpu().clone() for n, net in model.networks.items()})
    assert "structure_AB" in runs["0"][0] and "structure_BA" in runs["0"][0]
    for k, v in runs["0"][0].items():
        assert runs["1"][0][k] == pytest.approx(v, rel=2e-3, abs=1e-5), k
    for n, w in runs["0"][1].items():
        assert (runs["1"][1][n] - w).abs().mean().item() <= 1e-4, n
