"""csrc/norm.hip and csrc/norm_ex.hip against the float64 reference of tests/inorm_ref.py on every branch of their launch
plans (each row's `reaches` names its branch; tests/test_inorm_edges_cpu.py proves the rows are on them): both slot-sum
widths with and without the unrolled sweep, the two-in-flight forward loop on the fixed and the e / C8 path, the fused
statistics forward with one to three channel groups and 64 / 128 pixels per workgroup, every column count of the backward
reduction (ragged and full), reflect folds with three sources per axis in 2-D and 3-D, the 64-tap replicate corner, the
channel-group apply with 64 / 96 / 128 pixels per workgroup, pre_slots, the in-kernel bias gradient of one image and the
launch for several, gs_norm_bias_grads over two launches, and the U-Net form with slices, dropout and a device seed.

Every element of every output is compared (tests/pnorm_ref.py states the criterion):
  bf16   |got - r| <= 2^-8 |r| + K 2^-24 T            fp32   |got - prefill - ref| <= K2 2^-24 sum|terms|
Outputs are 16-byte-aligned views into larger allocations: full-tensor outputs start as NaN (every element must be written),
slice outputs start random (everything outside the slice must keep its bits), and the guard elements on either side must
keep their pattern. mean / rstd are held to the bounds DERIVED in inorm_ref's docstring (no constant). Where one rounding
decides, bits are demanded: gsum is the bf16 rounding of the float64 fold, the no-norm ReLU backward is g or 0, and the
no-norm, no-dropout, act none forward is a copy.

K = 4 and K2 = 32 are the project's (tests/test_pnorm_edges_gpu.py: measured for the row fold / slot-sum arithmetic these
kernels share), not fitted here; RefOps meets them on the CPU (0.83 / 0.53 at worst). Largest excess measured on an MI355X:
  x (gs_inorm_act_forward)        0.829  fixed, lrelu, with res        x (fused statistics forward)   0.428  ppb128, relu, with res
  dy (gs_inorm_act_backward)      0.367  c96, exact, without g2        bias_grad (same)               1.547  rep_f3, detuned, g2
  x1 / x2 (norm_ex forward)       0.000  (no element beyond its own bf16 rounding)
  dy (norm_ex backward)           0.066  ex_cols8, detuned             bias_grad (norm_ex)            1.026  ex_cols32, exact
  db (gs_norm_bias_grads)         2.492
  mean: 0.933 of its derived tolerance at worst (groups3, fused), 0.583 for gs_inorm_finalize (row 4); every rstd inside
  its derived interval; gsum bit-exact on every case; dy from given partials and from the own reduction differ by < 0.001 of the allowance.
An excess below 1 means that no element is further from float64 than its own bf16 rounding plus one fp32 rounding of its
terms. No output needed a bound of its own: the long per-thread chains (ppb 320 and 576) stay below 0.1.
The slowest case (wide1, detuned, 9 M scalars) takes 0.97 s, its float64 reference on the CPU included.
"""
import time

import pytest
import torch

from tests import inorm_ref as R
from tests.test_pnorm_edges_gpu import K, K2

pytestmark = pytest.mark.gpu

K_MEASURED = dict(x=0.829, stats_x=0.428, dy=0.367, ex_x=0.0, ex_dy=0.066)
K2_MEASURED = dict(bias=1.547, ex_bias=1.026, bias_grads=2.492)
assert max(K_MEASURED.values()) <= K and max(K2_MEASURED.values()) <= K2
assert K <= R.K_CAP and K2 <= R.K2_CAP


def show(what, m):
    print(f"INORM_EXCESS {what} " + " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in m.items()))


@pytest.mark.parametrize("i", range(len(R.FINALIZE_CASES)))
def test_finalize_case(hip_ops, i):
    """gs_inorm_finalize on synthetic partials, mean_rstd pre-filled with NaN: inside the derived bounds"""
    N, slots, C, const, reaches = R.FINALIZE_CASES[i]
    part, hw = R.finalize_inputs(i)
    mr, whole = R.guarded((N * 2 * C,), torch.float32, hip_ops.device)
    hip_ops.inorm_finalize(part.to(hip_ops.device), N, slots, C, hw, mr, eps=1e-5)
    got = mr.cpu().view(N, 2, C)
    em, inside = R.finalize(part, N, slots, C, hw).check(got)
    show(f"finalize {i}", dict(mean=em, rstd_inside=inside))
    assert R.guards_intact(whole.cpu())
    assert em <= 1 and inside, reaches
    if const:
        want = torch.full((N,), R.EPS32 ** -0.5, dtype=torch.float64).float()
        assert torch.equal(got[:, 1, R.CONST_CHANNEL], want), "var < 0 must be clamped: rstd = eps^-1/2"


@pytest.mark.parametrize("name,act,res", R.FWD_RUNS, ids=[f"{n}-{a}-{'res' if r else 'nores'}" for n, a, r in R.FWD_RUNS])
def test_forward_case(hip_ops, name, act, res):
    t0 = time.perf_counter()
    ex, amb, guards = R.run_fwd(hip_ops, name, act, res, hip_ops.device)
    show(f"fwd {name} {act} res={int(res)}", dict(x=ex, seconds=time.perf_counter() - t0))
    assert amb == 0 and guards
    assert ex <= K, R.FWD_BY_NAME[name][2]


@pytest.mark.parametrize("name", [c[0] for c in R.STATS_FWD_CASES])
@pytest.mark.parametrize("act,res", [("relu", True), ("lrelu", False)])
def test_stats_forward_case(hip_ops, name, act, res):
    """published statistics against the finalize reference; x against the forward reference evaluated WITH the published
    statistics"""
    m = R.run_stats_fwd(hip_ops, name, act, res, hip_ops.device)
    show(f"stats_fwd {name} {act} res={int(res)}", m)
    assert m["ambiguous"] == 0 and m["guards"]
    assert m["mean"] <= 1 and m["rstd_inside"] and m["x"] <= K, R.STATS_FWD_BY_NAME[name][3]


def hip_backward(hip_ops, b, **kw):
    if b.case.ppb:
        with hip_ops.options(norm_bwd_ppb=b.case.ppb):
            return R.run_bwd(hip_ops, b, hip_ops.device, **kw)
    return R.run_bwd(hip_ops, b, hip_ops.device, **kw)


@pytest.mark.parametrize("name,stats,g2", R.BWD_RUNS, ids=[f"{n}-{s}-{'g2' if g else 'nog2'}" for n, s, g in R.BWD_RUNS])
def test_backward_case(hip_ops, name, stats, g2):
    t0 = time.perf_counter()
    b = R.build_bwd(name, stats, g2)
    c = b.case
    if c.cus:      # the plan this row claims depends on the device
        assert torch.cuda.get_device_properties(hip_ops.device).multi_processor_count == c.cus, c.reaches
    assert b.ref.ambiguous == 0
    got = hip_backward(hip_ops, b)
    m = R.measure_bwd(b, got)
    show(f"{name} {stats} g2={int(g2)}", dict(m, seconds=time.perf_counter() - t0))
    assert got["guards"], "guard elements changed"
    assert m.get("gsum_exact", True), f"{name} ({c.reaches}): gsum is not the bf16 rounding of the float64 fold"
    assert m["dy"] <= K, f"{name} ({c.reaches}): dy excess {m['dy']:.1f}"
    assert m.get("bias", 0) <= K2, f"{name} ({c.reaches}): bias excess {m['bias']:.1f}"
    if stats == "none" and c.act == "relu":
        gb = b.ref.g.float().to(R.BF16).float().reshape(c.shape)
        want = torch.where(b.y.float() > 0, gb, torch.zeros_like(gb))
        assert torch.equal(got["dy"].float(), want), "the no-norm ReLU backward is g or 0"


def test_pre_partials_against_own_reduction(hip_ops):
    """dy from pre= partials the test computed itself (the float64 sums rounded to fp32, one slot) against dy from the kernel's
    own reduction: each within K of its float64 statement, and of each other within the two allowances"""
    b = R.build_bwd("cg_f1", "detuned", True)
    c, s = b.case, b.ref.sums
    scratch = torch.zeros(c.N * 2 * 3 * c.C)
    scratch[:c.N * 3 * c.C] = torch.cat([s["S1"], s["S2"], s["S3"]], 1).float().reshape(-1)
    pre = (1, scratch)
    ref_pre = R.backward(b.gpad, b.g2, b.y, b.mean_rstd, dims=c.sp, p=c.fold, mode=c.mode, act=c.act, pre=pre)
    own, given = hip_backward(hip_ops, b), hip_backward(hip_ops, b, pre=pre)
    shape = b.ref.dy.shape
    e_own = R.worst(R.bf16_excess(own["dy"].reshape(shape), b.ref.dy, b.ref.T_dy))
    e_pre = R.worst(R.bf16_excess(given["dy"].reshape(shape), ref_pre.dy, ref_pre.T_dy))
    allow = R.P.HALF_BF16 * (b.ref.dy.abs() + ref_pre.dy.abs()) + K * R.U24 * (b.ref.T_dy + ref_pre.T_dy)
    diff = (own["dy"].double() - given["dy"].double()).reshape(shape).abs()
    show("pre_vs_own", dict(own=e_own, pre=e_pre, worst_ratio=float((diff / allow).max())))
    assert own["guards"] and given["guards"]
    assert e_own <= K and e_pre <= K and bool((diff <= allow).all())
    assert R.worst(R.f32_excess(given["bias"].double() - R.BIAS_PREFILL, ref_pre.bias, ref_pre.bias_terms)) <= K2


def test_default_and_forced_plan_agree(hip_ops):
    """the default plan (17 chunks of 64 pixels, wide slot sum) and the norm_bwd_ppb = 4 plan (264 chunks, narrow slot sum)
    of the same input: both within K of float64"""
    b = R.build_bwd("ppb4", "detuned", True)
    forced = hip_backward(hip_ops, b)
    default = R.run_bwd(hip_ops, b, hip_ops.device)
    mf, md = R.measure_bwd(b, forced), R.measure_bwd(b, default)
    show("ppb4 forced", mf)
    show("ppb4 default", md)
    for m in (mf, md):
        assert m["dy"] <= K and m["bias"] <= K2 and m["gsum_exact"]
    assert torch.equal(forced["gsum"], default["gsum"])


def test_bias_grads_two_launches(hip_ops):
    """gs_norm_bias_grads over 33 items (32 + 1), neighbours of different C (8, 24, 300), N of 1 and 3, db pre-filled"""
    items = R.bias_grads_inputs()
    dev = hip_ops.device
    dbs = [R.guarded((it["C"],), torch.float32, dev, torch.full((it["C"],), R.BIAS_PREFILL)) for it in items]
    held = [(it["sums"].to(dev), it["mr"].to(dev)) for it in items]
    hip_ops.norm_bias_grads([(s, 0, mr, db, it["N"], it["C"], it["hw"]) for it, (s, mr), (db, _) in zip(items, held, dbs)])
    worst = 0.0
    for it, (db, whole) in zip(items, dbs):
        assert R.guards_intact(whole.cpu())
        worst = max(worst, R.worst(R.f32_excess(db.cpu().double() - R.BIAS_PREFILL, it["ref"], it["terms"])))
    show("bias_grads", dict(db=worst))
    assert worst <= K2


@pytest.mark.parametrize("name,stats", R.EX_RUNS, ids=[f"{n}-{s}" for n, s in R.EX_RUNS])
def test_norm_ex_case(hip_ops, name, stats):
    t0 = time.perf_counter()
    b = R.build_ex(name, stats)
    c, w = b.case, b.case.widths
    assert b.ref.ambiguous == 0
    got = R.run_ex(hip_ops, b, hip_ops.device)
    m, touched = R.measure_ex(b, got)
    show(f"{name} {stats}", dict(m, seconds=time.perf_counter() - t0))
    assert got["guards"] and not touched, f"{name}: changed outside the slice: {touched}"
    for k, v in m.items():
        assert v <= (K2 if k == "bias" else K), f"{name} ({c.reaches}): {k} excess {v:.1f}"
    if c.fwd and not c.norm and c.drop_p == 0 and c.act1 == "none":
        co = w["x1"][1]
        assert torch.equal(got["x1"][..., co:co + c.C].view(torch.int16), b.y.view(torch.int16)), "x1 must be a copy of y"
