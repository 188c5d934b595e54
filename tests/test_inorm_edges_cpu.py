"""The float64 reference of tests/inorm_ref.py checked without a GPU: against float64 autograd of the real composition
(nn.InstanceNorm2d/3d, ReLU / LeakyReLU, the residual add, nn.ReflectionPad2d/3d / nn.ReplicationPad3d), against the fp32
oracle RefOps by the per-element criterion and the constants the GPU test applies to the kernels, the dropout mask against
RefOps bit for bit, and the case tables against the launch plans of norm.hip / norm_ex.hip (the chunk counts are the
library's own)."""
import ctypes
import math

import pytest
import torch
import torch.nn as nn

from oracle.ops_ref import RefOps
from tests import inorm_ref as R
from tests.test_pnorm_edges_cpu import rel_close
from tests.test_pnorm_edges_gpu import K, K2

BWD_IDS = [f"{n}-{s}-{'g2' if g else 'nog2'}" for n, s, g in R.BWD_RUNS]
SMALL_RUNS = [r for r in R.BWD_RUNS if r[0] in R.BWD_SMALL and r[1] != "none"]


def library():
    from ganslate_amd.hip import lib as L
    if not L.library_path().is_file():
        import __graft_entry__
        __graft_entry__.build()
    return L, L.load()


@pytest.mark.parametrize("name,stats,g2", SMALL_RUNS, ids=[f"{n}-{s}-{'g2' if g else 'nog2'}" for n, s, g in SMALL_RUNS])
def test_reference_is_the_autograd_of_the_composition(name, stats, g2):
    """x = act(InstanceNorm(y)) + res, padded, through an identity stand-in for the conv; the loss <pad(x), gpad> + <x, g2>
    has the gradient dy at y. Exact statistics: InstanceNorm recomputes them in float64, the reference takes them rounded to
    fp32, hence 1e-6. Detuned statistics are no function of y: autograd with mu and rstd held constant gives x and
    rstd * ghat; the reference's dy must be that minus the two projection terms formed from autograd's ghat, and its bias
    the float64 sum of its own dy. (The cotangents are made contiguous: InstanceNorm's CPU backward was seen to return
    another gradient for a channels-last strided one.)"""
    b = R.build_bwd(name, stats, g2)
    c = b.case
    nd = len(c.sp)
    chf = lambda t: t.reshape(c.N, *c.sp, -1).movedim(-1, 1).contiguous()            # [N, pixels, C] -> N C ...
    back = lambda t: t.movedim(1, -1).reshape(c.N, -1, c.C)
    y = chf(R.flat(b.y)).requires_grad_(True)
    res = chf(R.flat(torch.randn(*c.shape, generator=torch.Generator().manual_seed(5)).to(R.BF16)))
    if stats == "exact":
        yh = (nn.InstanceNorm2d if nd == 2 else nn.InstanceNorm3d)(c.C, eps=R.EPS32).double()(y)
    else:
        mu, rstd = R.P.split_stats(b.mean_rstd, c.N, c.C)
        bc = lambda t: t.reshape(c.N, c.C, *(1,) * nd)
        yh = (y - bc(mu)) * bc(rstd)
    act = {"relu": nn.ReLU(), "lrelu": nn.LeakyReLU(R.SLOPE), "none": nn.Identity()}[c.act]
    x = act(yh) + res
    fwd = R.forward(b.y, b.mean_rstd, back(res), c.act)
    assert fwd.ambiguous == 0
    rel_close(fwd.out, back(x.detach()), "x")
    out = x
    if c.fold:
        pad = {("reflect", 2): nn.ReflectionPad2d, ("reflect", 3): nn.ReflectionPad3d,
               ("replicate", 3): nn.ReplicationPad3d}[(c.mode, nd)](c.fold)
        out = pad(x)
    out = nn.Identity()(out)                                                  # the conv that consumes the padded tensor
    loss = (out * b.gpad.double().movedim(-1, 1).contiguous()).sum()    # (contiguous cotangents: see the docstring)
    if g2:
        loss = loss + (x * b.g2.double().movedim(-1, 1).contiguous()).sum()
    dy, gx, gyh = torch.autograd.grad(loss, [y, x, yh])
    rel_close(b.ref.g, back(gx), "fold(gpad) + g2")
    dy = back(dy)
    if stats == "detuned":
        gh, yhf, hw = back(gyh), back(yh.detach()), math.prod(c.sp)
        dy = dy - rstd * gh.sum(1, keepdim=True) / hw - rstd * yhf * (gh * yhf).sum(1, keepdim=True) / hw
    rel_close(b.ref.dy, dy, "dy")
    rel_close(b.ref.bias, b.ref.dy.sum((0, 1)), "bias = sum dy", scale=b.ref.dy.abs().sum((0, 1)).max())
    if stats == "detuned":
        assert float(b.ref.bias.abs().median()) > 1e-2, "detuned statistics must give a bias gradient that is no rounding noise"


@pytest.mark.parametrize("name,stats,g2", R.BWD_RUNS, ids=BWD_IDS)
def test_fp32_oracle_meets_the_backward_criterion(name, stats, g2):
    """RefOps against the float64 reference with the constants of the GPU test; the folded gradient is exactly representable
    in fp32 (decided by the reference alone: it lets the GPU test demand gsum bit for bit); no ambiguous sign"""
    b = R.build_bwd(name, stats, g2)
    assert b.ref.ambiguous == 0
    assert torch.equal(b.ref.g.float().double(), b.ref.g), "the folded gradient must be exact in fp32"
    got = R.run_bwd(RefOps(), b)
    # RefOps sums its dy for the bias gradient: the absolute summands of THAT sum
    m = R.measure_bwd(b, got, bias_terms=b.ref.T_dy.sum((0, 1)) if stats != "none" else None)
    print(f"INORM_REFOPS {name} {stats} g2={int(g2)} " + " ".join(f"{k}={v:.2f}" for k, v in m.items()))
    assert got["guards"]
    assert m.get("gsum_exact", True)
    assert m["dy"] <= K and m.get("bias", 0) <= K2, m


@pytest.mark.parametrize("name,act,res", R.FWD_RUNS, ids=[f"{n}-{a}-{'res' if r else 'nores'}" for n, a, r in R.FWD_RUNS])
def test_fp32_oracle_meets_the_forward_criterion(name, act, res):
    ex, amb, guards = R.run_fwd(RefOps(), name, act, res)
    print(f"INORM_REFOPS fwd {name} {act} res={int(res)} x={ex:.2f}")
    assert amb == 0 and guards and ex <= K


@pytest.mark.parametrize("name", [c[0] for c in R.STATS_FWD_CASES])
@pytest.mark.parametrize("act,res", [("relu", True), ("lrelu", False)])
def test_fp32_oracle_meets_the_stats_forward_criterion(name, act, res):
    m = R.run_stats_fwd(RefOps(), name, act, res)
    print(f"INORM_REFOPS stats_fwd {name} {act} res={int(res)} mean={m['mean']:.2f} x={m['x']:.2f}")
    assert m["ambiguous"] == 0 and m["guards"]
    assert m["mean"] <= 1 and m["rstd_inside"] and m["x"] <= K


@pytest.mark.parametrize("i", range(len(R.FINALIZE_CASES)))
def test_finalize_reference(i):
    """RefOps (double sums, exact division) lies inside the derived bounds; the statistics are those of nn.InstanceNorm; the
    constant channel is clamped"""
    N, slots, C, const, _ = R.FINALIZE_CASES[i]
    part, hw = R.finalize_inputs(i)
    mr = torch.full((N * 2 * C,), float("nan"))
    RefOps().inorm_finalize(part, N, slots, C, hw, mr, eps=R.EPS32)
    fin = R.finalize(part, N, slots, C, hw)
    em, inside = fin.check(mr.view(N, 2, C))
    print(f"INORM_REFOPS finalize {i} mean={em:.3f}")
    assert em <= 1 and inside
    if const:
        assert torch.equal(mr.view(N, 2, C)[:, 1, R.CONST_CHANNEL].double().float(),
                           torch.full((N,), R.EPS32 ** -0.5, dtype=torch.float64).float())
    assert R.finalize(part, N, slots, C, hw, inv_hw_f32=False).check(mr.view(N, 2, C))[1]


def test_finalize_reference_is_instance_norm():
    y = (torch.randn(2, 6, 5, 16, generator=torch.Generator().manual_seed(3)) * 2 + 0.3).to(R.BF16)
    part = R.partials_of(y, 7, torch.Generator().manual_seed(4))
    fin = R.finalize(part, 2, 7, 16, 30)
    ref = nn.InstanceNorm2d(16, eps=R.EPS32).double()(y.double().movedim(-1, 1)).movedim(1, -1).reshape(2, 30, 16)
    assert torch.allclose((R.flat(y) - fin.mean[:, None]) * fin.rstd[:, None], ref, rtol=0, atol=1e-5)


def test_bias_grads_reference():
    items = R.bias_grads_inputs()
    assert len(items) == 33 and any(a["C"] != b["C"] for a, b in zip(items[:31], items[1:32]))
    dbs = [torch.full((it["C"],), R.BIAS_PREFILL) for it in items]
    RefOps().norm_bias_grads([(it["sums"], 0, it["mr"], db, it["N"], it["C"], it["hw"]) for it, db in zip(items, dbs)])
    for it, db in zip(items, dbs):
        assert R.worst(R.f32_excess(db.double() - R.BIAS_PREFILL, it["ref"], it["terms"])) <= K2


@pytest.mark.parametrize("name,stats", R.EX_RUNS, ids=[f"{n}-{s}" for n, s in R.EX_RUNS])
def test_fp32_oracle_meets_the_norm_ex_criterion(name, stats):
    b = R.build_ex(name, stats)
    assert b.ref.ambiguous == 0
    got = R.run_ex(RefOps(), b)
    m, touched = R.measure_ex(b, got, bias_terms=b.ref.T_dy.sum((0, 1)) if b.case.norm else None)
    print(f"INORM_REFOPS {name} {stats} " + " ".join(f"{k}={v:.2f}" for k, v in m.items()))
    assert got["guards"] and not touched
    for k, v in m.items():
        assert v <= (K2 if k == "bias" else K), f"{k}: excess {v:.1f}"


@pytest.mark.parametrize("case", [c for c in R.EX_CASES if c.drop_p > 0], ids=lambda c: c.name)
def test_dropout_mask_is_the_oracles(case):
    N, H, W, C = case.shape
    dev = torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in R.SEED_DEV], dtype=torch.int32) if case.seed_dev else None
    mine = R.drop_scale(N, H * W * C, case.drop_p, R.SEED, R.SEED_DEV if case.seed_dev else None)
    theirs = RefOps._drop_scale(case.shape, case.drop_p, RefOps._full_seed(R.SEED, dev))
    assert torch.equal(mine.float().view(case.shape), theirs)                 # (1 / (1 - p) in fp32 there, rounded here)
    kept = float((mine > 0).double().mean())
    assert 1 - case.drop_p - 0.05 <= kept <= 1 - case.drop_p + 0.05, kept


# ---- the tables against the launch plans ---------------------------------------------------------------------------------
def lib_chunks(c):
    """chunks of the reduction pass from gs_inorm_backward_scratch_floats = N (chunks + 1) 3 C (host code) under the case's
    norm_bwd_ppb"""
    L, lib = library()
    before = ctypes.c_int(0)
    L.check(lib.gs_get_option(b"norm_bwd_ppb", ctypes.byref(before)), "gs_get_option")
    L.check(lib.gs_set_option(b"norm_bwd_ppb", c.ppb), "gs_set_option")
    try:
        D, H, W = (1,) * (3 - len(c.sp)) + tuple(c.sp)
        floats = int(lib.gs_inorm_backward_scratch_floats(c.N, D, H, W, c.C))
    finally:
        L.check(lib.gs_set_option(b"norm_bwd_ppb", before.value), "gs_set_option")
    assert floats % (c.N * 3 * c.C) == 0
    return floats // (c.N * 3 * c.C) - 1


@pytest.mark.parametrize("case", R.BWD_CASES, ids=lambda c: c.name)
def test_case_is_on_its_branch(case):
    own = lib_chunks(case)
    chunks = case.pre or own
    assert chunks == case.chunks, f"{case.name}: {chunks} chunks"
    plan = R.bwd_plan(case.N, case.sp, case.C, chunks, cus=case.cus or 256, fold=case.fold, mode=case.mode)
    for k, v in case.expect:
        assert plan.get(k) == v, f"{case.name} ({case.reaches}): {k} is {plan.get(k)}, the table says {v}"
    if case.fold and case.mode == "reflect":
        assert all(n > 2 * case.fold for n in case.sp)                        # what the library accepts
    assert case.reaches and (case.scalars > 2_000_000) == case.big


@pytest.mark.parametrize("row", R.FWD_CASES, ids=lambda r: r[0])
def test_forward_case_is_on_its_branch(row):
    name, shape, reaches, expect = row
    plan = R.fwd_plan(shape[0], math.prod(shape[1:-1]), shape[-1])
    for k, v in expect.items():
        assert plan[k] == v, f"{name} ({reaches}): {k} is {plan[k]}, the table says {v}"


@pytest.mark.parametrize("row", R.STATS_FWD_CASES, ids=lambda r: r[0])
def test_stats_forward_case_is_on_its_branch(row):
    name, shape, slots, reaches, expect = row
    plan = R.stats_fwd_plan(shape[0], math.prod(shape[1:-1]), shape[-1], slots)
    assert plan == expect, f"{name} ({reaches}): {plan}"


@pytest.mark.parametrize("case", R.EX_CASES, ids=lambda c: c.name)
def test_norm_ex_case_is_on_its_branch(case):
    L, lib = library()
    N, H, W, C = case.shape
    d = L.NormExDesc()
    d.N, d.H, d.W, d.C = N, H, W, C
    floats = int(lib.gs_norm_backward_ex_scratch_floats(ctypes.byref(d)))
    chunks = floats // (N * 3 * C) - 1
    assert chunks == R.ceil_div(H * W, 64)
    C8 = C // 8
    cols = next((k for k in (32, 8) if C8 >= k), 1)
    assert (cols, C8 % cols != 0) == (case.cols, case.ragged)
    widths = [cs for cs, co in case.widths.values()]
    assert len(set(widths)) == len(widths) and all(co > 0 and co % 8 == 0 and cs % 8 == 0 for cs, co in case.widths.values())
    if case.name == "ex_wrap":
        assert H * W * C8 > 2048 * 256 and C8 & (C8 - 1) and N == 1
        assert R.slot_sum_plan(N, chunks, C) == dict(narrow=True, sweep=True, tail=True, idle=False, edge=False)


def test_table_reaches_every_branch():
    """every branch the old tests of test_ops_gpu.py left out, from the numbers of the tables"""
    ex = {c.name: dict(c.expect) for c in R.BWD_CASES}
    cases = R.BWD_BY_NAME
    # fold_sources with cnt == 3 (extent 2 fold + 1), on both axes and on one; reflect fold in 3-D
    assert ex["r3_7x7"]["cnt"] == (3, 3) and ex["r2_5x7"]["cnt"] == (3, 2) and ex["r3d_f3"]["cnt"] == (3, 2, 2)
    assert any(len(c.sp) == 3 and c.mode == "reflect" and c.fold for c in R.BWD_CASES)
    assert any(c.mode == "replicate" and c.fold == 3 for c in R.BWD_CASES)
    # norm_c8_shift() == -1 in the grid-stride apply (not cg), ragged norm_by_cols for every COLS, non-power-of-two decode
    assert any(e.get("shift") is False and e["cg"] is False for e in ex.values())
    assert {e["cols"] for e in ex.values() if e.get("ragged")} == {2, 4, 8, 32}
    assert any(e.get("groups") == 5 for e in ex.values()) and R.STATS_FWD_BY_NAME["groups3"][4]["groups"] == 3
    # the two-in-flight main loop of the forward on both paths
    assert any(r[3]["fixed"] and 2 in r[3]["mains"] for r in R.FWD_CASES)
    assert any(not r[3]["fixed"] and 1 in r[3]["mains"] for r in R.FWD_CASES)
    # the px = pxb + 32 loops (ppb > 64) of both channel-group kernels, the ppb += 32 bump, pre_slots with many pixels
    assert any(r[4].get("ppb", 0) > 64 for r in R.STATS_FWD_CASES)
    assert ex["bump"]["ppb_cg"] == 96 and ex["bump"]["bumped"] and cases["bump"].cus == 256
    assert ex["pre19"]["ppb_cg"] == 128 and cases["pre19"].pre == 19
    # slot_sum_kernel<2 | 3>: the unrolled sweep wide and narrow, with a tail
    fin = [R.slot_sum_plan(N, s, C) for N, s, C, _, _ in R.FINALIZE_CASES]
    for narrow in (False, True):
        assert any(p["narrow"] == narrow and p["sweep"] and p["tail"] for p in fin)
        assert any(e.get("slot", {}).get("narrow") == narrow for e in ex.values()) or not narrow
    assert any(p["idle"] for p in fin) and any(not p["sweep"] for p in fin)
    # ... and the edge sl + 3 LANES == slots, wide (finalize and backward) and narrow
    assert any(p["edge"] and not p["narrow"] for p in fin)
    assert {e["slot"]["narrow"] for e in ex.values() if e.get("slot", {}).get("edge")} == {False, True}
    assert any(s > 256 and not R.slot_sum_plan(N, s, C)["narrow"] for N, s, C, _, _ in R.FINALIZE_CASES)
    assert sum(e.get("slot", {}).get("narrow", False) and e["slot"]["sweep"] for e in ex.values()) >= 2
    # slot_sum_ordered: 8-unroll with a tail (19) and without (64), and under 8 slots
    assert {(r[4].get("unroll8"), r[4].get("tail")) for r in R.STATS_FWD_CASES if r[4]["fused"]} == \
        {(True, True), (True, False), (False, True)}
    assert {r[2] for r in R.STATS_FWD_CASES} >= {19, 64, 65} and any(r[1][-1] % 64 for r in R.STATS_FWD_CASES)
    # in-kernel db of one image and the parameter-gradient launch for several, on both apply forms
    for cg in (False, True):
        assert {c.N > 1 for c in R.BWD_CASES if ex[c.name]["cg"] == cg} == {False, True}
    # gs_norm_bias_grads: two launches, items of different C side by side, C > 256
    assert R.DB_ITEMS > 32 and max(R.DB_CS) > 256 and len(set(R.DB_CS)) == 3
    # norm_bwd_ppb routes: the two-pixel loop at ROWS 64 and 128, and 256 (COLS 1 at the default plan)
    assert {(c.ppb, ex[c.name].get("cols")) for c in R.BWD_CASES if c.ppb == 576} == {(576, 4), (576, 2)}
    assert ex["wide1"]["cols"] == 1 and cases["wide1"].chunks == 3520
    # norm_ex.hip: every COLS, ragged 8 and 32, x2 = None, g2 = None, no norm, every drop_p, a device seed, tanh, the wrap
    exs = R.EX_CASES
    assert {c.cols for c in exs} == {1, 8, 32} and {c.cols for c in exs if c.ragged} == {8, 32}
    assert any(not c.x2 for c in exs) and any(not c.g2 for c in exs) and any(not c.norm for c in exs)
    assert {c.drop_p for c in exs} == {0.0, 0.5, 0.3} and any(c.seed_dev and c.drop_p for c in exs)
    assert any(c.act1 == "tanh" and not c.norm and not c.fwd for c in exs) and not any(c.act1 == "tanh" and c.fwd for c in exs)
    assert any(not c.norm and c.drop_p == 0 and c.act1 == "none" for c in exs) and any(c.big and c.shape[0] == 1 for c in exs)
    # every activation and both statistics modes, with and without g2, and the no-norm form
    assert {c.act for c in R.BWD_CASES} == {"relu", "lrelu", "none"}
    assert {(s, g) for _, s, g in R.BWD_RUNS} >= {(s, g) for s in R.STATS for g in (True, False)} | {("none", True)}
