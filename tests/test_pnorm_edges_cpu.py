"""The float64 reference of tests/pnorm_ref.py checked without a GPU: against float64 autograd of the real composition
(nn.InstanceNorm3d, nn.PReLU, the residual adds, x.repeat), against the fp32 oracle RefOps by the per-element criterion the
GPU test applies to the kernels, and the case table against the library's own launch plan (chunks per image)."""
import ctypes

import pytest
import torch
import torch.nn as nn

from oracle.ops_ref import RefOps
from tests import pnorm_ref as R
from tests.test_pnorm_edges_gpu import K, K2

RUN_IDS = [f"{n}-{s}" for n, s in R.CASE_RUNS]
SMALL_RUNS = [(n, s) for n, s in R.CASE_RUNS if n in R.SMALL]


def rel_close(got, ref, what, scale=None, rel=1e-6):
    scale = float(ref.abs().max()) if scale is None else float(scale)
    err = float((got - ref).abs().max())
    assert err <= rel * scale, f"{what}: {err:.3e} > {rel} * {scale:.3e}"


def composition(b, y, slope, res_img, held_stats):
    """the module composition of the case in float64 on NCDHW tensors -> out. held_stats: (mu, rstd) [N, C] constants in
    place of InstanceNorm3d (the same expression written out)"""
    c = b.case
    bc = lambda t: t.reshape(c.N, c.C, 1, 1, 1)
    if not c.norm:
        yh = y
    elif held_stats is None:
        yh = nn.InstanceNorm3d(c.C, eps=R.EPS, affine=False).double()(y)
    else:
        yh = (y - bc(held_stats[0])) * bc(held_stats[1])
    r = None
    if c.res_mode:
        r = res_img.repeat(1, c.C // c.res_mod, 1, 1, 1) if c.res_mod else res_img
    u = yh + r if c.res_mode == 1 else yh
    if c.slope:
        act = nn.PReLU(c.C).double()
        act.weight = slope
        v = act(u)
    else:
        v = u
    return (v + r if c.res_mode == 2 else r - v if c.res_mode == 3 else v), yh


@pytest.mark.parametrize("name,stats", SMALL_RUNS, ids=[f"{n}-{s}" for n, s in SMALL_RUNS])
def test_reference_is_the_autograd_of_the_composition(name, stats):
    """exact statistics: InstanceNorm3d recomputes them in float64, the reference takes them rounded to fp32, hence 1e-6.
    Detuned statistics are no function of y: autograd with mu and rstd held constant gives out, gu (= gres), dslope and
    rstd * gu; the reference's dy must be that minus the two projection terms formed from autograd's gu, and its bias_grad
    the float64 sum of its own dy (-rstd S2 S3 / hw is that sum, and S3 is not zero here)."""
    b = R.build(name, stats)
    c, w = b.case, b.case.widths
    ncdhw = lambda t: t.reshape(c.N, *c.sp, -1).movedim(-1, 1).contiguous()
    y = ncdhw(R.view(b.y, w["y"][1], c.C)).requires_grad_(True)
    slope = nn.Parameter(b.slope.double().clone()) if c.slope else None
    res_img = None
    if c.res_mode:
        co = w["res"][1]
        res_img = ncdhw(b.res[..., co:co + (c.res_mod or c.C)].double()).requires_grad_(True)
    held = None
    if stats == "detuned":
        mu, rstd = R.split_stats(b.mean_rstd, c.N, c.C)
        held = (mu[:, 0], rstd[:, 0])
    out, yh = composition(b, y, slope, res_img, held)
    gt = R.view(b.g, w["g"][1], c.C) + (R.view(b.g2, w["g2"][1], c.C) if c.g2 else 0)
    flat = lambda t: t.movedim(1, -1).reshape(c.N, c.voxels, -1)
    rel_close(b.fwd.out, flat(out.detach()), "out")
    leaves = [y] + ([slope] if c.slope else []) + ([yh] if held is not None else [])
    grads = list(torch.autograd.grad(out, leaves, ncdhw(gt)))
    dy = flat(grads.pop(0))
    if c.slope:
        rel_close(b.bwd.dslope, grads.pop(0), "dslope", scale=b.bwd.dslope_terms.max())
    if held is not None:
        gu = flat(grads.pop(0))
        rel_close(b.bwd.gu, gu, "gu")
        rstd, hw = held[1][:, None, :], c.voxels
        yhf = flat(yh.detach())
        dy = dy - rstd * gu.sum(1, keepdim=True) / hw - rstd * yhf * (gu * yhf).sum(1, keepdim=True) / hw
    rel_close(b.bwd.dy, dy, "dy")
    if c.norm:
        rel_close(b.bwd.bias, b.bwd.dy.sum((0, 1)), "bias_grad = sum dy", scale=b.bwd.dy.abs().sum((0, 1)).max())
        if stats == "detuned":
            # (S3 is about -0.055 hw for every channel; S2 is a random sum and can be near zero for one channel of hundreds)
            assert float(b.bwd.bias.abs().median()) > 1e-2, "detuned statistics must give a bias gradient that is no rounding noise"
    if c.res_mode == 1:                                           # gres, and through x.repeat the image gradient
        (gr,) = torch.autograd.grad(composition(b, y, slope, res_img, held)[0], [res_img], ncdhw(gt))
        gres = b.bwd.gu
        if c.res_mod:
            gres = torch.stack([gres[..., c0::c.res_mod].sum(-1) for c0 in range(c.res_mod)], -1)
        rel_close(gres, flat(gr), "gres")


@pytest.mark.parametrize("name,stats", R.CASE_RUNS, ids=RUN_IDS)
def test_fp32_oracle_meets_the_criterion(name, stats):
    """RefOps (fp32 torch) against the float64 reference by the criterion and the constants of the GPU test: the two
    references agree, and K / K2 are not so tight that fp32 arithmetic in another order misses them. Also here: the
    reference finds no element whose sign of u fp32 could decide differently, and the case is on its branch."""
    b = R.build(name, stats)
    assert b.fwd.ambiguous == 0, f"{b.fwd.ambiguous} elements with |u| <= 2^-18 (|yhat| + |res|): choose another seed"
    assert b.case.res_mode != 1 or not b.case.norm or b.case.voxels <= 378, "norm + mode 1 stays on the small cases"
    # RefOps forms the bias gradient as the fp32 sum of its dy over the pixels, not as the product -rstd S2 S3 / hw (the
    # same number in exact arithmetic): the absolute summands of THAT sum are those of the elements of dy
    m, touched = R.measure(b, R.run_ops(RefOps(), b), bias_terms=b.bwd.T_dy.sum((0, 1)) if b.case.norm else None)
    assert not touched, f"changed outside the slice: {touched}"
    print(f"PNORM_REFOPS {name} {stats} " + " ".join(f"{k}={v:.2f}" for k, v in m.items()))
    for k, v in m.items():
        assert v <= (K2 if k in ("dslope", "bias") else K), f"{k}: excess {v:.1f}"


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_case_is_on_its_branch(case):
    """chunks from gs_pnorm_backward_scratch_floats = N (chunks + 1) 4 C (host code, no GPU needed) equals the value the
    row claims, and the quantities the launch plan of prelu.hip branches on are what `reaches` says"""
    from ganslate_amd.hip import lib as L
    if not L.library_path().is_file():
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    d = L.PNormDesc()
    d.N, d.C, d.pixels = case.N, case.C, case.voxels
    floats = int(lib.gs_pnorm_backward_scratch_floats(ctypes.byref(d)))
    assert floats % (case.N * 4 * case.C) == 0
    assert floats // (case.N * 4 * case.C) - 1 == case.chunks
    assert case.chunks in (2, 6, 275, 526)
    assert case.reaches
    for cs, co in case.widths.values():
        assert co > 0 and cs != case.C


def test_table_reaches_every_branch():
    """the rows of the branch table, from the numbers of the cases alone (C8 = C / 8, chunks, N, elements per image)"""
    runs = {c.name: c for c in R.CASES}
    reduce_cols = lambda c: 32 if c.C // 8 >= 32 else 8 if c.C // 8 >= 8 else 4 if c.C // 8 >= 4 else 2 if c.C // 8 >= 2 else 1
    reducing = [c for c in R.CASES if c.norm or (c.slope and c.dslope)]
    assert {reduce_cols(c) for c in reducing} == {1, 2, 4, 8, 32}
    assert any((c.C // 8) % reduce_cols(c) for c in reducing if reduce_cols(c) == 2)         # an idle column
    assert any((c.C // 8) % 8 for c in reducing if reduce_cols(c) == 8)
    assert any((c.C // 8) % 32 for c in reducing if reduce_cols(c) == 32)
    pow2 = lambda c: (c.C // 8) & (c.C // 8 - 1) == 0
    assert any(pow2(c) for c in R.CASES) and any(not pow2(c) and c.norm for c in R.CASES)
    fin4 = [c for c in reducing if c.C < 128 and c.chunks > 256]
    fin16 = [c for c in reducing if not (c.C < 128 and c.chunks > 256)]
    assert any(c.chunks > 3 * 64 and c.chunks % 256 for c in fin4)                           # sweep and tail, 64 lanes
    assert any(c.chunks > 3 * 16 and c.chunks % 64 for c in fin16)                           # sweep and tail, 16 lanes
    assert any(c.C >= 128 for c in fin16) and any(c.chunks <= 48 for c in fin16)
    assert any(c.N == 1 and c.norm and c.slope for c in reducing) and any(c.N > 1 and c.norm and c.slope for c in reducing)
    for fixed in (True, False):                                   # both element loops wrap on both paths
        assert any(c.voxels * (c.C // 8) > 2048 * 256 and pow2(c) == fixed and c.norm for c in R.CASES)
    assert any(not c.norm and not c.dslope for c in R.CASES)      # no scratch at all
    assert any(not c.slope for c in R.CASES) and any(not c.g2 for c in R.CASES) and any(not c.gres for c in R.CASES)
    uses = {(c.norm, c.res_mode, c.res_mod) for c in R.CASES}
    assert {(True, 1, 1), (True, 1, 2), (True, 0, 0), (True, 2, 0), (True, 3, 0), (False, 1, 0)} <= uses
    assert runs["a_input"].voxels - 64 == 41


@pytest.mark.parametrize("i", range(len(R.ADD_VIEWS_CASES)))
def test_add_views_reference(i):
    sp, C, (dcs, dco), (scs, sco), acc = R.ADD_VIEWS_CASES[i]
    dst, src = R.small_inputs("add", i)
    r, T = R.add_views(dst, src, C, dco, sco, acc)
    got = R.add_views_fp32(dst, src, C, dco, sco, acc)
    ref_ops = dst.clone()
    RefOps().add_views(ref_ops, src, C, dst_co=dco, src_co=sco, accumulate=acc)
    assert torch.equal(got.view(torch.int16), ref_ops.view(torch.int16))
    assert R.worst(R.bf16_excess(R.view(got, dco, C), r, T)) <= 1.0          # one fp32 add, one rounding to bf16
    assert R.outside_untouched(got, dst, dco, C)


@pytest.mark.parametrize("i", range(len(R.REPEAT_CASES)))
def test_repeat_backward_reference(i):
    N, sp, Cin, C, (cs, co) = R.REPEAT_CASES[i]
    g, g_img = R.small_inputs("repeat", i)
    ref = R.repeat_backward(g, g_img, C, co)
    seq = R.repeat_backward_fp32(g, g_img, C, co)
    terms = g_img.double().abs().reshape(N, Cin, -1) + torch.stack(
        [R.view(g, co, C)[..., c0::Cin].abs().sum(-1) for c0 in range(Cin)], 1)
    assert R.worst(R.f32_excess(seq.reshape(N, Cin, -1), ref, terms)) <= C // Cin + 1
    # the adjoint of x.repeat by autograd
    x = torch.zeros(N, Cin, *sp, dtype=torch.float64, requires_grad=True)
    gv = R.view(g, co, C).reshape(N, *sp, C).movedim(-1, 1)
    (gx,) = torch.autograd.grad(x.repeat(1, C // Cin, 1, 1, 1), [x], gv)
    assert torch.allclose(ref - g_img.double().reshape(N, Cin, -1), gx.reshape(N, Cin, -1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("i", range(len(R.SLICE_STATS_CASES)))
def test_slice_stats_reference(i):
    """mean and rstd of the reference against nn.InstanceNorm3d's own normalisation in float64, and RefOps by the criterion"""
    N, sp, C, (cs, co) = R.SLICE_STATS_CASES[i]
    (x,) = R.small_inputs("stats", i)
    mean, rstd, mt, rt = R.slice_stats(x, co, C)
    v = R.view(x, co, C)
    ref = nn.InstanceNorm3d(C, eps=R.EPS).double()(v.reshape(N, *sp, C).movedim(-1, 1)).movedim(1, -1).reshape(N, -1, C)
    assert torch.allclose((v - mean[:, None]) * rstd[:, None], ref, rtol=0, atol=1e-9)
    mr = torch.empty(N * 2 * C)
    RefOps().slice_stats(x, co, C, mr)
    mr = mr.view(N, 2, C).double()
    assert R.worst(R.f32_excess(mr[:, 0], mean, mt)) <= K2
    assert R.worst(R.f32_excess(mr[:, 1] / rstd, torch.ones_like(rstd), rt)) <= K2
