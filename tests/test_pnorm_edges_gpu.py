"""csrc/prelu.hip against the float64 reference of tests/pnorm_ref.py on every branch of its launch plan: the reduce
kernel's five column counts (ragged and full), both finalize widths with and without the unrolled sweep, the in-kernel
parameter gradients of one image and the separate launch for several, the fixed-group and the e / C8 paths of the forward
and apply loops with and without a wrapped grid; add_views, repeat_backward and slice_stats at their own edges.

Every element of every output is compared (tests/pnorm_ref.py states the criterion):
  bf16   |got - r| <= 2^-8 |r| + K 2^-24 T            fp32   |got - prefill - ref| <= K2 2^-24 sum|terms|
and everything outside the written channel slice must keep its pre-fill bit for bit. Norm cases run with the exact
statistics of y and with mu + 0.05, rstd * 1.1, where S3 = sum yhat is far from zero.

K and K2 are four times the largest excess measured on an MI355X over all cases, rounded up to a power of two (the margin
is for another seed or another legal summation order); the caps are 2^10 and 2^9 (pnorm_ref.K_CAP, K2_CAP).
  bf16 outputs: largest excess 0.640 (out of g_coupling, exact statistics; dy 0.232, gres 0.0)        -> K  = 4
  fp32 outputs: largest excess 4.709 (slice rstd; slice mean 0.648, dslope 1.031, bias_grad 0.892)    -> K2 = 32
An excess below 1 means that no element is further from float64 than its own bf16 rounding plus one fp32 rounding of its
terms; the fp32 oracle (RefOps on the CPU, tests/test_pnorm_edges_cpu.py) measures 0.64 and 1.18 on the same inputs.
"""
import pytest
import torch

from tests import pnorm_ref as R

pytestmark = pytest.mark.gpu

K_MEASURED, K2_MEASURED = 0.640, 4.709
K, K2 = 4, 32
assert K <= R.K_CAP and K2 <= R.K2_CAP


@pytest.mark.parametrize("name,stats", R.CASE_RUNS, ids=[f"{n}-{s}" for n, s in R.CASE_RUNS])
def test_pnorm_case(hip_ops, name, stats):
    """one row of pnorm_ref.CASES (its `reaches` names the branch), forward and backward on pre-filled buffers"""
    b = R.build(name, stats)
    assert b.fwd.ambiguous == 0
    got = R.run_ops(hip_ops, b, hip_ops.device)
    m, touched = R.measure(b, got)
    print(f"PNORM_EXCESS {name} {stats} " + " ".join(f"{k}={v:.3f}" for k, v in m.items()))
    assert not touched, f"{name}: changed outside the slice: {touched}"
    for k, v in m.items():
        assert v <= (K2 if k in ("dslope", "bias") else K), f"{name} ({b.case.reaches}): {k} excess {v:.1f}"
    c, w = b.case, b.case.widths
    if not c.norm and c.res_mode == 0:
        # pure PReLU: one fp32 multiply, one rounding — the same bits as torch on the CPU
        yv = b.y[..., w["y"][1]:w["y"][1] + c.C].float()
        want = torch.where(yv > 0, yv, b.slope * yv).to(torch.bfloat16)
        co = w["out"][1]
        assert torch.equal(got["out"][..., co:co + c.C].view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("i", range(len(R.ADD_VIEWS_CASES)))
def test_add_views_case(hip_ops, i):
    """dst[view] (+)= src[view]: fp32 add, round to nearest even — bit-exact against torch on the CPU, and against float64"""
    sp, C, (dcs, dco), (scs, sco), acc = R.ADD_VIEWS_CASES[i]
    dst, src = R.small_inputs("add", i)
    d = dst.to(hip_ops.device)
    hip_ops.add_views(d, src.to(hip_ops.device), C, dst_co=dco, src_co=sco, accumulate=acc)
    got = d.cpu()
    assert torch.equal(got.view(torch.int16), R.add_views_fp32(dst, src, C, dco, sco, acc).view(torch.int16))
    r, T = R.add_views(dst, src, C, dco, sco, acc)
    assert R.worst(R.bf16_excess(R.view(got, dco, C), r, T)) <= K
    assert R.outside_untouched(got, dst, dco, C)


@pytest.mark.parametrize("i", range(len(R.REPEAT_CASES)))
def test_repeat_backward_case(hip_ops, i):
    """adjoint of x.repeat into a pre-filled image gradient from a sliced g: a sequential fp32 sum in channel order"""
    N, sp, Cin, C, (cs, co) = R.REPEAT_CASES[i]
    g, g_img = R.small_inputs("repeat", i)
    gi = g_img.to(hip_ops.device)
    hip_ops.repeat_backward(g.to(hip_ops.device), gi, C, g_co=co)
    got = gi.cpu()
    assert torch.equal(got, R.repeat_backward_fp32(g, g_img, C, co))
    terms = g_img.double().abs().reshape(N, Cin, -1) + torch.stack(
        [R.view(g, co, C)[..., c0::Cin].abs().sum(-1) for c0 in range(Cin)], 1)
    assert R.worst(R.f32_excess(got.reshape(N, Cin, -1), R.repeat_backward(g, g_img, C, co), terms)) <= K2


@pytest.mark.parametrize("i", range(len(R.SLICE_STATS_CASES)))
def test_slice_stats_case(hip_ops, i):
    """gs_slice_stats<1 | 4 | 8 ragged> + gs_inorm_finalize, one slot and several: mean within K2 2^-24 sum|x| / hw, rstd
    relative to itself with the same constant propagated through var + eps"""
    N, sp, C, (cs, co) = R.SLICE_STATS_CASES[i]
    (x,) = R.small_inputs("stats", i)
    mr = torch.full((N * 2 * C,), float("nan"), device=hip_ops.device)
    hip_ops.slice_stats(x.to(hip_ops.device), co, C, mr)
    mr = mr.cpu().view(N, 2, C).double()
    mean, rstd, mt, rt = R.slice_stats(x, co, C)
    em = R.worst(R.f32_excess(mr[:, 0], mean, mt))
    er = R.worst(R.f32_excess(mr[:, 1] / rstd, torch.ones_like(rstd), rt))
    print(f"PNORM_EXCESS slice_stats {i} mean={em:.3f} rstd={er:.3f}")
    assert em <= K2 and er <= K2
