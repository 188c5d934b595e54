"""The channel-window kernels (gs_image_cat_to_act / _backward, gs_channel_embed, gs_l1_window, gs_ssim_distance_window /
_backward) and the balanced CycleGAN recipe on the MI355X.

Kernel tests: every output buffer is pre-filled with NaN (fp32) or the byte 0xA5 (bf16 activations), buffers that must stay
untouched are checked for the fill afterwards, every op runs twice and the two results must be equal. The layout kernels are
bit-exact against the dense kernel on the materialised tensor (gs_image_to_act of torch.cat of the slices) or against plain
torch; the loss kernels are held to float64 with the bounds tests/test_loss_edges_gpu.py uses for their dense forms."""
import math
import random

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from ganslate_amd.hip.lib import HipError
from tests import balanced_ref as B
from tests import loss_ref as R
from tests.test_loss_edges_gpu import SSIM_FLOOR, dense_bound
from tests.test_recipe_gradients_gpu import LAST_CONV, _tier

pytestmark = pytest.mark.gpu

NAN = float("nan")
POISON = 0xA5


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _poisoned_act(dev, N, spatial, Cp):
    return torch.full((N, *spatial, Cp), POISON, dtype=torch.uint8, device=dev).repeat_interleave(2, dim=-1) \
        .view(torch.bfloat16).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- 6. image_cat_to_act ----------------------------------------------------------------------------------------------------
# name -> (N, spatial, [(channels of the source tensor, c0, c1)])
CAT_CASES = {
    "a_window_0_1_of_2": (3, (11, 13), [(2, 0, 1)]),
    "b_window_3_6_of_6_unaligned": (2, (11, 13), [(6, 3, 6)]),
    "c_window_plus_dense": (2, (11, 13), [(6, 0, 3), (1, 0, 1)]),
    "d_dense_plus_window_volume": (2, (3, 12, 11), [(1, 0, 1), (2, 1, 2)]),
    "e_nine_channels_across_the_pack_group": (2, (11, 13), [(3, 0, 3), (7, 0, 6)]),
    "f_grid_stride_514x511": (1, (514, 511), [(1, 0, 1), (2, 1, 2)]),
}


@pytest.mark.parametrize("name", list(CAT_CASES))
def test_image_cat_to_act_bit_exact(hip_ops, name):
    dev = hip_ops.device
    N, spatial, layout = CAT_CASES[name]
    tensors = [_rand((N, C, *spatial), 100 + 7 * k).to(dev) for k, (C, _, _) in enumerate(layout)]
    srcs = [(t, c0, c1) for t, (_, c0, c1) in zip(tensors, layout)]
    chans = [c1 - c0 for _, c0, c1 in layout]
    Cp = (sum(chans) + 7) // 8 * 8
    if name.startswith("b_"):
        assert (tensors[0].data_ptr() + 3 * 11 * 13 * 4) % 16 != 0 and 3 * 11 * 13 * 4 == 1716
    want = _poisoned_act(dev, N, spatial, Cp)
    hip_ops.image_to_act(torch.cat([t[:, c0:c1] for t, c0, c1 in srcs], dim=1).contiguous(), want)
    got = [_poisoned_act(dev, N, spatial, Cp) for _ in range(2)]
    for g in got:
        hip_ops.image_cat_to_act(srcs, g)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got[0]), _bits(want)), "differs from image_to_act of the materialised cat (pad lanes included)"
    assert torch.equal(_bits(got[0]), _bits(got[1])), "two runs differ"
    assert (got[0][..., sum(chans):].float() == 0).all()
    # backward: each requested dense gradient is .float() of its channel slice; a source without a pointer keeps its poison
    gact = torch.randn((N, *spatial, Cp), generator=torch.Generator().manual_seed(5)).to(dev).to(torch.bfloat16)
    offs = [sum(chans[:k]) for k in range(len(chans))]
    for skip in [None] + (list(range(len(chans))) if len(chans) > 1 else []):
        runs = []
        for _ in range(2):
            grads = [torch.full((N, ch, *spatial), NAN, device=dev) for ch in chans]
            hip_ops.image_cat_to_act_backward(gact, [None if k == skip else g for k, g in enumerate(grads)], chans)
            runs.append(grads)
        torch.cuda.synchronize()
        for k, (g, off, ch) in enumerate(zip(runs[0], offs, chans)):
            if k == skip:
                assert torch.isnan(g).all(), f"source {k} asked for no gradient but was written"
                continue
            assert torch.equal(g, gact[..., off:off + ch].float().movedim(-1, 1)), (name, k, skip)
            assert torch.equal(g, runs[1][k])


# ---- 7. channel_embed ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,c0,t,spatial", [(2, 6, 3, 3, (11, 13)), (2, 2, 1, 1, (3, 12, 11)), (1, 2, 1, 1, (514, 511))],
                         ids=["b_3_6_of_6", "d_1_2_of_2_volume", "f_514x511"])
def test_channel_embed_bit_exact(hip_ops, N, C, c0, t, spatial):
    dev = hip_ops.device
    src = _rand((N, t, *spatial), 31).to(dev)
    want = torch.zeros((N, C, *spatial), device=dev)
    want[:, c0:c0 + t] = src
    outs = [torch.full((N, C, *spatial), NAN, device=dev) for _ in range(2)]
    for o in outs:
        hip_ops.channel_embed(src, o, c0)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], want)                      # (NaN != NaN: an element left unwritten fails here)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


# ---- 8. strided L1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,win,spatial", [(2, 3, (1, 3), (11, 13)), (1, 2, (1, 2), (3, 12, 11)), (2, 2, (1, 2), (514, 511))],
                         ids=["2x3_w1_3_11x13", "1x2_w1_2_3x12x11", "2x2_w1_2_514x511"])
def test_l1_window_vs_float64(hip_ops, N, C, win, spatial):
    """loss within dense_bound("l1", n, ...) of tests/test_loss_edges_gpu.py at the same n (the kernel walks the elements in
    gs_l1's order); every gradient element within 2 ulp of the float64 value rounded to fp32, grad_scale a device scalar"""
    dev = hip_ops.device
    a, b = _rand((N, C, *spatial), 41), _rand((N, win[1] - win[0], *spatial), 42)
    aw = a[:, win[0]:win[1]].contiguous()
    n = b.numel()
    ref_loss, ref_grad_a = R.l1(aw, b)                      # gradient w.r.t. the first operand; the dense one is b: negate
    scale = 2.5
    ad, bd, sd = a.to(dev), b.to(dev), torch.tensor(scale, device=dev)
    losses, grads = [], []
    for _ in range(2):
        loss, grad = torch.full((), NAN, device=dev), torch.full_like(bd, NAN)
        hip_ops.l1_window(ad, win[0], win[1], bd, loss=loss)
        hip_ops.l1_window(ad, win[0], win[1], bd, grad_b=grad, grad_scale=sd)
        losses.append(float(loss)); grads.append(grad.cpu())
    bound = dense_bound("l1", n, aw.reshape(-1), b.reshape(-1), float(ref_loss))
    print(f"l1_window n={n}: |loss - float64| {abs(losses[0] - float(ref_loss)):.3e}, bound {bound:.3e}")
    assert not math.isnan(losses[0]) and losses[0] == losses[1]
    assert abs(losses[0] - float(ref_loss)) <= bound
    assert not torch.isnan(grads[0]).any(), "gradient elements not written"
    assert torch.equal(grads[0], grads[1])
    worst = float(R.err_ulp32(grads[0], -ref_grad_a * scale).max())
    print(f"l1_window n={n}: gradient worst {worst:.3f} ulp")
    assert worst <= 2.0


# ---- 9. strided SSIM --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,win,spatial", [(2, 3, (1, 3), (11, 13)), (1, 2, (1, 2), (3, 12, 11))],
                         ids=["2x3_w1_3_11x13", "1x2_w1_2_3x12x11"])
def test_ssim_window_vs_float64(hip_ops, N, C, win, spatial):
    """distance (relative) and dense-side gradient (largest error over the largest reference value, per plane and whole tensor)
    against float64; yardstick as in test_ssim_at_the_tile_edges: 4 x BalancedRefOps's own error on the same input, floored at
    SSIM_FLOOR. The gradient is the dense entry point's on the materialised window bit for bit (the same kernels). The forward
    is evaluated in double with the fp32 Gaussian weights and rounded once: the 3x12x11 case has 3 planes x 2 x 1 = 6 valid
    pixels, where an fp32 evaluation lies 5e-9 .. 1.1e-6 from float64 depending on the draw (the dense kernel: 6.8e-7 on this
    input, against a yardstick of 4.77e-7); what is left in double is the weights' rounding, 1.6e-7 and 1.1e-7 on the two
    cases when evaluated on the CPU."""
    dev = hip_ops.device
    x = _rand((N, C, *spatial), 51)
    y = x[:, win[0]:win[1]] * 0.6 + _rand((N, win[1] - win[0], *spatial), 52) * 0.4
    xw = x[:, win[0]:win[1]].contiguous()
    scale = 0.5
    val64, g64 = R.ssim_distance(xw, y), R.ssim_grad_y(xw, y) * scale
    cpu = B.BalancedRefOps(act_dtype=torch.float32)
    cval, cg = torch.zeros(()), torch.zeros_like(y)
    cpu.ssim_distance_window(x, win[0], win[1], y, cval)
    cpu.ssim_distance_window_backward(x, win[0], win[1], y, cg, grad_scale=torch.tensor(scale))
    cpu_val = float((cval.double() - val64).abs() / val64.abs())
    cpu_g = R.per_plane_rel_err(cg, g64)
    xd, yd, sd = x.to(dev), y.to(dev), torch.tensor(scale, device=dev)
    vals, grads = [], []
    for _ in range(2):
        val, g = torch.full((), NAN, device=dev), torch.full_like(yd, NAN)
        hip_ops.ssim_distance_window(xd, win[0], win[1], yd, val)
        hip_ops.ssim_distance_window_backward(xd, win[0], win[1], yd, g, grad_scale=sd)
        vals.append(val.cpu()); grads.append(g.cpu())
    assert not torch.isnan(vals[0]) and not torch.isnan(grads[0]).any(), "outputs not written"
    assert torch.equal(vals[0], vals[1]) and torch.equal(grads[0], grads[1])
    # the dense gradient entry point on the materialised window: the same kernels, the same bits
    dg = torch.full_like(yd, NAN)
    hip_ops.ssim_distance_backward(xw.to(dev), yd, dg, grad_scale=sd)
    assert torch.equal(dg.cpu(), grads[0])
    dev_val = float((vals[0].double() - val64).abs() / val64.abs())
    err = R.per_plane_rel_err(grads[0], g64)
    whole = float((grads[0].double() - g64).abs().max() / g64.abs().max())
    print(f"ssim_window {spatial}: value cpu {cpu_val:.3e} device {dev_val:.3e}; gradient per plane cpu "
          f"{[f'{v:.2e}' for v in cpu_g.tolist()]} device {[f'{v:.2e}' for v in err.tolist()]}; whole tensor {whole:.3e}")
    assert dev_val <= max(4 * cpu_val, SSIM_FLOOR)
    assert (err <= torch.clamp_min(4 * cpu_g, SSIM_FLOOR)).all()
    assert whole <= max(4 * float(cpu_g.max()), SSIM_FLOOR)


# ---- 10. argument checks ------------------------------------------------------------------------------------------------------
def test_argument_checks_raise_before_any_launch(hip_ops):
    dev = hip_ops.device
    x6, y3 = torch.zeros((2, 6, 12, 13), device=dev), torch.zeros((2, 3, 12, 13), device=dev)
    act = torch.zeros((2, 12, 13, 8), dtype=torch.bfloat16, device=dev)
    out = torch.zeros((), device=dev)
    with pytest.raises(ValueError, match="window"):                                 # a window beyond C
        hip_ops.image_cat_to_act([(x6, 4, 7)], act)
    with pytest.raises(ValueError, match="window"):
        hip_ops.l1_window(x6, 5, 8, y3, loss=out)
    with pytest.raises(ValueError, match="window"):
        hip_ops.ssim_distance_window(x6, 3, 7, y3, out)
    with pytest.raises(ValueError, match="window"):
        hip_ops.channel_embed(y3, x6, 4)
    with pytest.raises(ValueError, match="dense"):                                  # a non-dense operand
        hip_ops.image_cat_to_act([(x6[:, 3:6], 0, 3)], act)
    with pytest.raises(ValueError, match="dense"):
        hip_ops.l1_window(x6, 3, 6, x6[:, :3], loss=out)
    with pytest.raises(ValueError, match="dense"):
        hip_ops.ssim_distance_window_backward(x6, 3, 6, y3, x6[:, :3])
    with pytest.raises(ValueError, match="dense"):
        hip_ops.channel_embed(x6[:, :3], x6, 0)
    with pytest.raises(ValueError, match="fp32"):                                   # an fp64 input
        hip_ops.image_cat_to_act([(x6.double(), 0, 3)], act)
    with pytest.raises(ValueError, match="fp32"):
        hip_ops.l1_window(x6, 3, 6, y3.double(), loss=out)
    with pytest.raises(ValueError, match="fp32"):
        hip_ops.ssim_distance_window(x6.double(), 3, 6, y3, out)
    with pytest.raises(ValueError, match="fp32"):
        hip_ops.channel_embed(y3.double(), x6, 0)
    other_n, other_hw = torch.zeros((1, 3, 12, 13), device=dev), torch.zeros((2, 3, 13, 12), device=dev)
    for bad in (other_n, other_hw):                                                 # mismatched N or extent
        with pytest.raises(ValueError, match="differ"):
            hip_ops.image_cat_to_act([(x6, 0, 3), (bad, 0, 3)], act)
        with pytest.raises(ValueError, match="differ"):
            hip_ops.l1_window(x6, 3, 6, bad, loss=out)
        with pytest.raises(ValueError, match="differ"):
            hip_ops.ssim_distance_window(x6, 3, 6, bad, out)
        with pytest.raises(ValueError, match="differ"):
            hip_ops.channel_embed(bad, x6, 0)
        with pytest.raises(ValueError, match="differ"):
            hip_ops.image_cat_to_act_backward(act, [y3.clone(), bad], [3, 3])
    with pytest.raises(ValueError, match="channels"):                               # window and dense operand of other widths
        hip_ops.l1_window(x6, 2, 6, y3, loss=out)
    with pytest.raises(ValueError, match="10 x 10"):
        hip_ops.ssim_distance_window(torch.zeros((1, 2, 10, 13), device=dev), 0, 1, torch.zeros((1, 1, 10, 13), device=dev), out)
    # the library's own GS_REQUIRE failures surface as HipError (called below the Python checks)
    import ctypes as C
    from ganslate_amd.hip import lib as L
    null, st = C.c_void_p(0), C.c_void_p(0)
    with pytest.raises(HipError, match="gs_channel_embed"):
        L.check(hip_ops.lib.gs_channel_embed(C.c_void_p(y3.data_ptr()), C.c_void_p(x6.data_ptr()), 2, 6, 4, 3, 156, st),
                "gs_channel_embed")
    with pytest.raises(HipError, match="gs_l1_window"):
        L.check(hip_ops.lib.gs_l1_window(C.c_void_p(x6.data_ptr()), 10, C.c_void_p(y3.data_ptr()), 2, 468, null, null, null, st),
                "gs_l1_window")
    with pytest.raises(HipError, match="gs_image_cat_to_act"):
        ptrs, strides, chans = (C.c_void_p * 1)(x6.data_ptr()), (C.c_int64 * 1)(6 * 156), (C.c_int32 * 1)(9)
        L.check(hip_ops.lib.gs_image_cat_to_act(ptrs, strides, chans, 1, C.c_void_p(act.data_ptr()), 2, 156, 8, st),
                "gs_image_cat_to_act")
    with pytest.raises(HipError, match="gs_ssim_distance_window"):
        L.check(hip_ops.lib.gs_ssim_distance_window(C.c_void_p(x6.data_ptr()), 6 * 156, 4, C.c_void_p(y3.data_ptr()), 6, 12, 13,
                                                    C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()), st),
                "gs_ssim_distance_window")
    torch.cuda.synchronize()
    assert float(out) == 0.0 and float(x6.abs().max()) == 0.0 and float(act.float().abs().max()) == 0.0      # nothing ran


# ---- 11. recipe step 0 against the restatement --------------------------------------------------------------------------------
def _product_step0(c):
    from tests.helpers import FROZEN, adam_first_moments
    model = B.build_product(c, FROZEN)
    got = B.run_product_steps(model, c, 1)[0]
    torch.cuda.synchronize()
    beta1 = model.conf.train.gan.optimizer.beta1
    return got["losses"], {net: {k: v / (1 - beta1) for k, v in per.items()} for net, per in adam_first_moments(model).items()}


# Norm ratios of the SAME executor on the CPU oracle backend with bf16 activation storage (BalancedRefOps(act_dtype=torch.bfloat16),
# learning rates frozen, step 0) against the fp32 restatement, for the weight tensors that storage format alone moves past their
# tier. These networks are far smaller than that test's (ngf 8; 64 x 64 images through six stride-2 levels leave 2 x 2 and 1 x 1
# maps, the volumes 2 x 2 x 2 and 1 x 1 x 1, in front of the deepest InstanceNorms): rounding the activations to bf16 moves the
# encoder gradients by up to 23 % (cg2d G_BA) with cosines still >= 0.95. Every other weight tensor of both cases is inside its
# tier on the CPU with bf16 storage and is held to the tier unchanged on the GPU. Measured on the MI355X for the listed tensors,
# in this order: 1.0693; 0.9377, 0.9539, 0.9480, 0.9404, 0.9227; 0.9628; 0.9726.
BF16_STORAGE = {
    "cg2d": {("G_AB", "model.model.1.model.3.model.3.model.3.model.3.model.1.weight"): 1.0440,
             ("G_BA", "model.model.0.weight"): 0.8185,
             ("G_BA", "model.model.1.model.1.weight"): 0.8300,
             ("G_BA", "model.model.1.model.3.model.1.weight"): 0.8066,
             ("G_BA", "model.model.1.model.3.model.3.model.1.weight"): 0.7859,
             ("G_BA", "model.model.1.model.3.model.3.model.3.model.1.weight"): 0.7678},
    "hx3d": {("G_AB", "model.model.1.model.3.model.3.model.3.model.1.weight"): 0.9714,
             ("G_BA", "model.model.1.model.3.model.3.model.1.weight"): 0.9714},
}


def _norm_tier(case, net, n, numel, cos):
    """the tier of tests/test_recipe_gradients_gpu.py; for a tensor of BF16_STORAGE twice the deviation bf16 storage alone
    produces on the CPU (the device's pass and the CPU's are two draws of one noise — other summation orders, other rounding
    points —, and 2 x is what tests/test_loss_edges_gpu.py grants a second fp32 evaluation over the first)"""
    tier = _tier("pix2pix", n, numel, False, cos)
    cpu = BF16_STORAGE[case].get((net, n))
    return tier if cpu is None else max(tier, 2 * abs(cpu - 1))


@pytest.mark.parametrize("name", list(B.CASES))
def test_step0_losses_and_gradients_vs_restatement(hip_ops, name):
    """losses within 2 %; per-tensor gradients through the tiers of tests/test_recipe_gradients_gpu.py for its U-Net family
    (`_tier("pix2pix", ...)`, cosine >= 0.90 generators / 0.96 discriminators), zero-true-gradient biases and the generators'
    tiny last-conv biases absolutely, as there. Eight encoder weight tensors miss the norm tier through bf16 storage alone and
    are held to the CPU evidence instead (BF16_STORAGE)."""
    c = B.CASES[name]
    losses, got = _product_step0(c)
    random.seed(c["seed"])
    ref = B.BalancedStep(c)
    want_losses, _ = ref.step(*B.case_inputs(c, 0), update=False)
    want = ref.grads()
    for k, v in want_losses.items():
        print(f"  loss {k:8s} {losses[k]:.6f} vs {v:.6f}")
        assert losses[k] == pytest.approx(v, rel=2e-2), (k, losses[k], v)
    rows, zero, tiny = [], [], []
    for net, per in want.items():
        wnorm = {n: float(w.double().norm()) for n, w in per.items()}
        for n, w in per.items():
            assert n in got[net], (net, n, sorted(got[net])[:5])
            g, w = got[net][n].double().flatten(), w.double().flatten()
            refn = wnorm[n]
            sibling = wnorm.get(n[:-4] + "weight", 0.0) if n.endswith(".bias") else 0.0
            if n.endswith(".bias") and refn < 1e-4 * max(sibling, 1e-30):
                zero.append((net, n, float(g.norm()), sibling))
                continue
            if w.numel() < 8 and n.endswith(".bias") and net.startswith("G") and any(n.startswith(p) for p in LAST_CONV["pix2pix"]):
                tiny.append((net, n, float((g - w).norm()), sibling, float(g.norm() / (refn + 1e-300))))
                continue
            cos = float(g @ w / (g.norm() * w.norm() + 1e-300))
            rows.append((net, n, cos, float(g.norm() / (refn + 1e-300)), w.numel()))
    print(f"\n[{name}] per-tensor gradient parity vs the fp32 restatement (cosine, norm ratio):")
    for net, n, cos, ratio, numel in rows:
        print(f"  {net:5s} {n:44s} cos {cos:.5f}  norm ratio {ratio:.4f}  ({numel} elements)")
    for net, n, diff, sib, ratio in tiny:
        print(f"  {net:5s} {n:44s} |g - w| / |sibling weight gradient| {diff / sib:.4f}  (norm ratio {ratio:.3f})")
        assert diff <= 0.10 * sib, (net, n, diff, sib)
    for net, n, gn, sib in zero:
        assert gn <= 1e-2 * sib, (net, n, gn, sib)
    bad = [(net, n, round(cos, 4), round(ratio, 4), numel) for net, n, cos, ratio, numel in rows
           if cos < (0.96 if net.startswith("D") else 0.90) or abs(ratio - 1) > _norm_tier(name, net, n, numel, cos)]
    assert not bad, bad


# ---- 12. eager against graph replay ----------------------------------------------------------------------------------------------
def _run(model, c, n_steps):
    random.seed(c["seed"])
    out = []
    for s in range(n_steps):
        A, Bt = B.case_inputs(c, s)
        model.set_input({"A": A, "B": Bt})
        model.optimize_parameters()
        _, losses, visuals, _ = model.get_loggable_data()
        torch.cuda.synchronize()
        out.append(({k: float(v.detach()) for k, v in losses.items() if v is not None}, visuals["fake_B"].detach().cpu().clone()))
        model.update_learning_rate()
    return out


def test_cg2d_step_replays_bit_for_bit(hip_ops):
    c = B.CASES["cg2d"]
    eager = B.build_product(c)
    eager.step_graph_enabled = False
    want = _run(eager, c, 4)
    graphed = B.build_product(c)
    assert graphed.step_graph_enabled
    got = _run(graphed, c, 4)
    assert graphed._graph is not None, "the step was never captured"
    for s in range(4):
        assert got[s][0] == want[s][0], s
        assert torch.equal(got[s][1], want[s][1]), s
        assert got[s][1].shape[1] == c["C"]["B"] and float(got[s][1][:, :3].abs().max()) == 0.0
    for name in eager.networks:
        assert torch.equal(eager.networks[name].master.detach(), graphed.networks[name].master.detach()), name


# ---- 13. no copies left on torch ----------------------------------------------------------------------------------------------
_SKIP = ("empty", "view", "as_strided", "detach", "alias", "_unsafe_view", "reshape", "select", "slice", "expand", "permute",
         "transpose", "t.", "unsqueeze", "squeeze", "narrow", "split", "unbind", "_local_scalar_dense", "is_pinned", "lift_fresh",
         "set_", "resize_", "record_stream", "chunk", "unfold", "contiguous", "_reshape_alias", "zeros_like", "empty_like",
         "empty_strided", "new_empty", "result_type", "is_same_size")          # views, allocations, metadata (tools/torch_rows.py)


class _Rows(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = set()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        base = str(func).replace("aten.", "aten::").split("::")[-1]
        flat = [t for t in torch.utils._pytree.tree_leaves((args, kwargs, out)) if torch.is_tensor(t)]
        if any(t.is_cuda for t in flat) and not any(base.startswith(s) for s in _SKIP):
            self.ops.add(base)
        return out


def _traced_ops(model, inputs):
    model.step_graph_enabled = False
    dev = model.device
    batch = {k: v.to(dev) for k, v in inputs.items()}
    for _ in range(2):                       # pools, packs and optimiser state exist; the traced step is a steady one
        model.set_input(batch)
        model.optimize_parameters()
    torch.cuda.synchronize()
    rows = _Rows()
    with rows:
        model.set_input(batch)
        model.optimize_parameters()
    torch.cuda.synchronize()
    return rows.ops


def test_no_torch_kernel_beyond_the_stock_step(hip_ops, monkeypatch):
    """the aten operators that compute on device tensors in one eager cg2d step are a subset of those of one eager step of the
    stock CycleGAN on the same networks (4-channel domains, GS_TWIN=0, no identity, the same proportion_ssim), measured here"""
    from ganslate_amd.utils.builders import build_conf, build_gan
    monkeypatch.setenv("GS_TWIN", "0")
    c = B.CASES["cg2d"]
    A, Bt = B.case_inputs(c, 0)
    random.seed(c["seed"])
    balanced = _traced_ops(B.build_product(c), {"A": A, "B": Bt})
    torch.manual_seed(c["seed"])
    stock = build_gan(build_conf([f"config={B.CONFIGS / 'cyclegan_unet_4ch.yaml'}"]))
    assert stock.twin_G is None and stock.twin_D is None
    random.seed(c["seed"])
    stock_ops = _traced_ops(stock, {"A": Bt, "B": Bt.flip(0)})
    print(f"stock: {sorted(stock_ops)}\nbalanced: {sorted(balanced)}")
    assert balanced <= stock_ops, sorted(balanced - stock_ops)
    assert not any(op.startswith("cat") for op in balanced)
