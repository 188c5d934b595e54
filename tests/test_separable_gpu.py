"""`is_separable=True` on the HIP path: the streaming row-axis kernel (csrc/daxis.hip, option `daxis`) against the op-level
oracle and against the kernels that take the same class with the option off, bit-exact integer-domain cases for the plane
and axis layers, the reference's golden case through the whole network, and CycleGAN iterations eager / captured."""
import pytest
import torch

from ganslate_amd.nn.native.spec import ConvSpec, lower
from oracle.ops_ref import RefOps

from . import separable_ref
from .test_cyclegan_gpu import rel_l2
from .test_ops_gpu import close_bf16, close_stats, make_layer

pytestmark = pytest.mark.gpu


def _axis_spec(ci, co, T):
    """T = 5: the (5,1,1) pad-2 conv; T = 2: the (2,1,1) stride-2 transposed conv = flipped pad-1 conv on one-row images"""
    if T == 5:
        return ConvSpec("conv", ci, co, 5, 1, 2, dims=3, axes="axis")
    return ConvSpec("convT", ci, co, 2, 2, 0, dims=3, axes="axis")


def _launch(ops, dev, low, g, x, pack, bias, out_shape, N, stats, in_co=0, accumulate=False, init=None):
    C = g.Co
    y = (torch.zeros(out_shape, dtype=torch.bfloat16) if init is None else init.clone()).to(dev)
    slots = ops.stat_slots(g, N) if stats else 0
    part = torch.full((max(N * slots * 2 * C, 1),), float("nan"), dtype=torch.float32, device=dev)
    ops.gconv(g, x.to(dev), pack.to(dev), None if bias is None else bias.to(dev), y, in_co=in_co,
              stats=part if stats else None, stats_slots=slots, accumulate=accumulate)
    mr = None
    if stats:
        mr = torch.empty(N * 2 * C, dtype=torch.float32, device=dev)
        ops.inorm_finalize(part, N, slots, C, y.numel() // (N * C), mr)
    return y, mr, slots


def _own_slots(N, rows, pixels):
    """csrc/daxis.hip daxis_plan: 64-pixel strips x row segments (enough workgroups for 8 per CU, at least 8 rows each)"""
    strips = (pixels + 63) // 64
    nseg = min(max(2048 // (N * strips), 1), max(rows // 8, 1))
    seg_len = -(-rows // nseg)
    return strips * -(-rows // seg_len)


# C (8 -> 16 once), D shorter than / equal to / longer than the tap span and odd, H W = a strip tail smaller than a tile,
# several strips, an exact multiple; both tap forms
AXIS_CASES = [(8, 8, 5, 2, 6, 10), (8, 16, 5, 3, 12, 20), (16, 16, 5, 5, 6, 10), (16, 16, 5, 13, 32, 32),
              (64, 64, 5, 13, 12, 20), (64, 64, 5, 5, 32, 32), (16, 16, 2, 3, 12, 20), (64, 64, 2, 5, 6, 10),
              (8, 16, 2, 13, 32, 32)]


@pytest.mark.parametrize("mirrored", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats_bias"])
@pytest.mark.parametrize("ci,co,T,D,H,W", AXIS_CASES)
def test_axis_kernel_matches_the_oracle_and_the_other_kernels(hip_ops, ci, co, T, D, H, W, stats, mirrored):
    N = 2
    spec = _axis_spec(ci, co, T)
    low, master, bias, fpack, dpack = make_layer(spec, (D, H, W), 7)
    g, pack = (low.dgrad[0], dpack) if mirrored else (low.fwd[0], fpack)
    view_in, view_out = (low.out_view, low.in_view) if mirrored else (low.in_view, low.out_view)
    vol_in = low.out_dims if mirrored else low.in_dims
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(N, *vol_in, g.Ci, generator=gen).to(torch.bfloat16).view(-1, *view_in, g.Ci)
    Nv = x.shape[0]
    b = None
    if stats:
        b = torch.randn(g.Co, generator=gen) * 0.1
    out_shape = (Nv, *view_out, g.Co)
    y_ref, mr_ref, _ = _launch(RefOps(), "cpu", low, g, x, pack, b, out_shape, Nv, stats)
    res = {}
    for on in (1, 0):
        with hip_ops.options(daxis=on):
            res[on] = _launch(hip_ops, hip_ops.device, low, g, x, pack, b, out_shape, Nv, stats)
            torch.cuda.synchronize()
    # the kernel ran: its slot count is strips x row segments, the other kernels count pixel tiles / boxes
    with hip_ops.options(daxis=1):
        own = hip_ops.stat_slots(g, Nv)
    assert own == _own_slots(Nv, g.Ho, H * W)
    if stats:
        assert res[1][2] == own
    for on in (1, 0):
        close_bf16(res[on][0], y_ref, f"axis conv output, daxis={on}")
        if stats:
            close_stats(res[on][1], mr_ref, Nv, g.Co, g.Co, f"daxis={on} ")
    close_bf16(res[1][0], res[0][0].cpu(), "option on against option off")


def test_axis_slots_differ_with_the_option(hip_ops):
    """gs_gconv_stat_slots answers for the kernel that will run: 64-pixel strips x row segments with the option on"""
    low = lower(_axis_spec(16, 16, 5), 13, 12, 20)
    g = low.fwd[0]
    with hip_ops.options(daxis=1):
        on = hip_ops.stat_slots(g, 2)
    with hip_ops.options(daxis=0):
        off = hip_ops.stat_slots(g, 2)
    assert on == 4 and on != off, (on, off)          # 240 pixels = 4 strips, 13 rows = one segment


@pytest.mark.parametrize("what", ["in_co", "accumulate"])
def test_sliced_and_accumulating_launches_stay_right(hip_ops, what):
    """the kernel declines channel slices and accumulate; whichever kernel takes them, the result is the oracle's"""
    N, D, H, W = 2, 5, 6, 10
    low, master, bias, fpack, dpack = make_layer(_axis_spec(16, 16, 5), (D, H, W), 9)
    g = low.fwd[0]
    gen = torch.Generator().manual_seed(10)
    x = torch.randn(N, D, H * W, 32, generator=gen).to(torch.bfloat16)
    init = torch.randn(N, D, H * W, 16, generator=gen).to(torch.bfloat16)
    kw = dict(in_co=16) if what == "in_co" else dict(in_co=16, accumulate=True, init=init)
    y_ref, _, _ = _launch(RefOps(), "cpu", low, g, x, fpack, None, init.shape, N, False, **kw)
    with hip_ops.options(daxis=1):
        y, _, _ = _launch(hip_ops, hip_ops.device, low, g, x, fpack, None, init.shape, N, False, **kw)
        torch.cuda.synchronize()
    close_bf16(y, y_ref, what)


# ---- integer domain (tests/exact.py): every sum exact in fp32, every stored value exact in bf16 -> any kernel gives these bits ----
def _ref64(spec, x, w, b, gy):
    """float64 torch layer from the ConvSpec alone (kernel / stride / padding per axis as ganslate/nn/separable.py builds
    them), on channels-first tensors: output, data gradient, weight gradient"""
    import torch.nn.functional as F
    live = [k > 1 for k in spec.kernel]
    st = tuple(spec.stride if l else 1 for l in live)
    pd = tuple(spec.pad if l else 0 for l in live)
    fn = F.conv3d if spec.kind == "conv" else F.conv_transpose3d
    x, w = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = fn(x, w, b, stride=st, padding=pd)
    y.backward(gy)
    return y.detach(), x.grad, w.grad


@pytest.mark.parametrize("daxis", [0, 1])
@pytest.mark.parametrize("kw,ci,co", [(dict(kind="conv", k=5, stride=1, pad=2, axes="plane"), 8, 16),
                                      (dict(kind="conv", k=2, stride=2, pad=0, axes="plane"), 16, 32),
                                      (dict(kind="convT", k=2, stride=2, pad=0, axes="plane"), 32, 16),
                                      (dict(kind="conv", k=5, stride=1, pad=2, axes="axis"), 16, 16),
                                      (dict(kind="conv", k=2, stride=2, pad=0, axes="axis"), 32, 32),
                                      (dict(kind="convT", k=2, stride=2, pad=0, axes="axis"), 16, 16)])
def test_integer_domain_layers_are_bit_exact(hip_ops, kw, ci, co, daxis):
    """Ternary weights (density 0.25), activations and output gradients of magnitude 1..2 (density 0.25), integer bias: the
    float64 reference must lie in the exact domain — |y|, |dx| <= 256 (integers that bf16 stores exactly), |dw| < 2^24, the
    per-(image, channel) sums of y and y^2 < 2^24 — and then forward, data gradient, weight gradient and the InstanceNorm
    partial sums of the HIP path equal it bit for bit, whichever kernel takes the class."""
    from .exact import int_act, int_layer, int_weights
    N, sizes = 2, (6, 12, 20)
    spec = ConvSpec(cin=ci, cout=co, dims=3, **kw)
    low, master, bias, fpack, dpack = int_layer(spec, sizes, 21, density=0.25)
    w, b = int_weights(spec, 21, 0.25)
    gen = torch.Generator().manual_seed(22)
    x = int_act(N, sizes, ci, spec.cin_p, gen, 0.25, 2)
    gy = int_act(N, low.out_dims, co, spec.cout_p, gen, 0.25, 2)
    cf = lambda t, c: t[..., :c].double().movedim(-1, 1).contiguous()
    y64, gx64, dw64 = _ref64(spec, cf(x, ci), w.double(), b.double(), cf(gy, co))
    s1, s2 = y64.sum((2, 3, 4)), (y64 * y64).sum((2, 3, 4))
    assert 0 < y64.abs().max() <= 256 and 0 < gx64.abs().max() <= 256 and 0 < dw64.abs().max() < 2 ** 24
    assert s1.abs().max() < 2 ** 24 and s2.max() < 2 ** 24
    dev = hip_ops.device
    with hip_ops.options(daxis=daxis):
        y = torch.zeros(N, *low.out_dims, spec.cout_p, dtype=torch.bfloat16, device=dev)
        Nv = N * low.out_images
        slots, offs = 0, []
        for g in low.fwd:
            offs.append(slots)
            slots += hip_ops.stat_slots(g, Nv, multi=low.fwd if len(low.fwd) > 1 else None)
        part = torch.full((Nv * slots * 2 * spec.cout_p,), float("nan"), dtype=torch.float32, device=dev)
        hip_ops.gconv_classes(low.fwd, low.vin(x.to(dev)), fpack.to(dev), bias.to(dev), low.vout(y), stats=part,
                              stats_slots=slots, stats_slot0s=offs)
        gx = torch.zeros(N, *sizes, spec.cin_p, dtype=torch.bfloat16, device=dev)
        hip_ops.gconv_classes(low.dgrad, low.vout(gy.to(dev)), dpack.to(dev), None, low.vin(gx))
        dw = torch.zeros(spec.master_numel, dtype=torch.float32, device=dev)
        a, gg = (low.vout(gy.to(dev)), low.vin(x.to(dev))) if spec.kind == "conv" else (low.vin(x.to(dev)), low.vout(gy.to(dev)))
        hip_ops.wgrad(low.wgrad, a, gg, dw)
        torch.cuda.synchronize()
    assert torch.equal(cf(y.cpu(), co), y64), "forward"
    assert not y.cpu()[..., co:].any(), "padded output channels"
    assert torch.equal(cf(gx.cpu(), ci), gx64), "data gradient"
    assert torch.equal(spec.torch_from_master(dw.cpu()).double(), dw64), "weight gradient"
    sums = part.cpu().view(N, low.out_images * slots, 2, spec.cout_p).double().sum(1)      # (integers: any order is exact)
    assert torch.equal(sums[:, 0, :co], s1) and torch.equal(sums[:, 1, :co], s2), "InstanceNorm partial sums"


# ---- the reference's golden case through the whole network --------------------------------------------------------------
def _zero_gradient_bias(n):
    """exactly-zero true gradient (tests/test_separable_cpu.py::_zero_gradient_biases): rounding noise on every side"""
    return n.endswith(".bias") and ("pointwise" in n or "down_conv" in n) and "conv2." not in n


@pytest.mark.parametrize("daxis", [0, 1])
@pytest.mark.parametrize("memory_saving", [False, True])
@pytest.mark.parametrize("name,inverse", [("plain", False), ("inverse", False), ("inverse", True)])
def test_network_matches_the_oracle_and_the_reference_golden(hip_ops, name, inverse, memory_saving, daxis):
    """The golden case (its weights, its input, loss mean(out^2)) on the HIP path, as tests/test_volumes_gpu.py checks a
    V-Net (test_vnet3d_hip_vs_oracle -> test_cyclegan_gpu._net_case, grad_tol 0.30, grad_cos 0.95): full tensors against the
    same executor on the bf16 CPU emulation (output relative L2 2e-2, gradients 0.30) and against the fp32 restatement that
    tests/test_separable_cpu.py pins to the golden (output 3e-2 and max error 0.12 max|ref|; input gradient and every
    parameter gradient relative L2 0.30 and cosine 0.95). Then the golden itself: output relative L2 5e-2 and |y| sum 2e-2
    as test_vnet2d_matches_reference_golden, the loss at the 2e-2 of a step loss, and the stored gradient samples of every
    tensor taken together at the same relative L2 / cosine."""
    from ganslate_amd.nn.generators import Vnet3D
    from ganslate_amd.nn.native import backend
    from .test_cyclegan_gpu import cosine
    case = separable_ref.golden()[name]
    rec = case["inverse" if inverse else "forward"]
    sd = separable_ref.golden_state_dict(case)
    x = separable_ref.golden_input(case)
    res = {}
    for which, ops in (("hip", hip_ops), ("cpu_bf16", RefOps(act_dtype=torch.bfloat16))):
        backend.set_ops(ops)
        try:
            net = Vnet3D(1, 1, "instance", use_memory_saving=memory_saving, use_inverse=case["use_inverse"],
                         is_separable=True, first_layer_channels=8, down_blocks=(1, 1), up_blocks=(1, 1))
            net.load_state_dict(sd)
            with hip_ops.options(daxis=daxis):
                xi = x.clone().to(ops.device).requires_grad_()
                out = net(xi, inverse=True) if inverse else net(xi)
                loss = (out * out).mean()
                loss.backward()
                if ops.device.type == "cuda":
                    torch.cuda.synchronize()
            res[which] = (out.detach().cpu(), float(loss.detach()), xi.grad.cpu(),
                          {k: v.cpu() for k, v in net.grads_state_dict().items()})
        finally:
            backend.set_ops(hip_ops)
    shadow = separable_ref.vnet3d(1, 1, 8, (1, 1), (1, 1), use_inverse=case["use_inverse"])
    shadow.load_state_dict(sd)
    xa = x.clone().requires_grad_()
    ya = shadow(xa, inverse=inverse)
    (ya * ya).mean().backward()
    ya = ya.detach()
    yh, lh, gxh, gh = res["hip"]
    yc, _, gxc, gc = res["cpu_bf16"]
    assert rel_l2(yh, yc) <= 2e-2, rel_l2(yh, yc)
    assert rel_l2(gxh, gxc) <= 0.30, rel_l2(gxh, gxc)
    assert rel_l2(yh, ya) <= 3e-2 and (ya - yh).abs().max().item() <= 0.12 * ya.abs().max().item()
    assert rel_l2(gxh, xa.grad) <= 0.30 and cosine(gxh, xa.grad) >= 0.95, (rel_l2(gxh, xa.grad), cosine(gxh, xa.grad))
    gold = separable_ref.param_grads(case, rec)
    seen = 0
    for n, p in shadow.named_parameters():
        if n.startswith("encoder.") or p.grad is None or _zero_gradient_bias(n):
            continue
        seen += 1
        got, emu = gh[n].reshape(p.shape), gc[n].reshape(p.shape)
        if p.dim() == 1:
            # Bias and PReLU-slope gradients: per channel ONE sum over the voxels of random-sign terms that largely cancel
            # (3072 voxels at the input resolution, 384 and 48 below; a slope sees the negative half only), so the bf16
            # rounding of the terms stays un-averaged in it — the case _net_case makes for a SelfAttentionBlock's gamma, and
            # checked like it: sign and order of magnitude, against both references. The weight tensors of the same layers
            # are held to the full tolerance below, and so is the input gradient, which every layer's backward feeds.
            for ref in (emu, p.grad):
                ratio = got.norm().item() / ref.norm().item()
                assert cosine(got, ref) > 0 and 0.2 <= ratio <= 5.0, (n, cosine(got, ref), ratio)
            continue
        assert rel_l2(got, emu) <= 0.30, (n, rel_l2(got, emu))
        assert rel_l2(got, p.grad) <= 0.30 and cosine(got, p.grad) >= 0.95, (n, rel_l2(got, p.grad), cosine(got, p.grad))
    assert seen == sum(1 for n in gold if not _zero_gradient_bias(n))
    # the golden itself
    ref = separable_ref.golden_output(rec)
    assert rel_l2(yh.flatten(), ref) <= 5e-2, rel_l2(yh.flatten(), ref)
    assert abs(yh.double().abs().sum().item() - ref.double().abs().sum().item()) <= 2e-2 * ref.double().abs().sum().item()
    assert lh == pytest.approx(rec["loss"], rel=2e-2)
    gin = rec["input_grad"]
    got = gxh.flatten()[gin["idx"]]
    want = torch.tensor(gin["values"])
    assert rel_l2(got, want) <= 0.30 and cosine(got, want) >= 0.95, (rel_l2(got, want), cosine(got, want))
    # (4 elements per tensor say nothing alone; every weight tensor's samples, each scaled by its tensor's norm, do)
    a = torch.cat([gh[n].flatten()[g["idx"]] / g["norm"] for n, g in gold.items() if n.endswith(".weight")])
    b = torch.cat([torch.tensor(g["values"]) / g["norm"] for n, g in gold.items() if n.endswith(".weight")])
    assert rel_l2(a, b) <= 0.30 and cosine(a, b) >= 0.95, (rel_l2(a, b), cosine(a, b))


# ---- CycleGAN iterations ------------------------------------------------------------------------------------------------
def _iterations(hip_ops, monkeypatch, graph, daxis):
    from .test_separable_cpu import _cyclegan, _steps
    monkeypatch.setenv("GS_STEP_GRAPH", "1" if graph else "0")
    monkeypatch.setenv("GS_DAXIS", str(daxis))        # (building a model maps the variables onto the library's options)
    torch.manual_seed(11)
    model = _cyclegan()
    assert hip_ops.get_option("daxis") == daxis
    out = _steps(model, 4)
    torch.cuda.synchronize()
    # iteration 1 runs launch by launch, iteration 2 is the capture, 3 and 4 replay it
    assert (model._graph is not None) == graph, "the step graph was (not) captured"
    return out


@pytest.mark.parametrize("daxis", [0, 1])
def test_cyclegan_iterations_eager_and_captured_agree_bit_for_bit(hip_ops, monkeypatch, daxis):
    eager = _iterations(hip_ops, monkeypatch, False, daxis)
    again = _iterations(hip_ops, monkeypatch, False, daxis)
    graph = _iterations(hip_ops, monkeypatch, True, daxis)
    for s in eager:
        assert all(torch.isfinite(torch.tensor(v)) for v in s.values()), s
    assert eager == again, "two runs from the same seed"
    assert eager == graph, "launch by launch against the captured step graph"
