"""tests/boundary_ref.py checked without a GPU: the fp32 oracle RefOps meets every criterion on every case (so the float64
statement is right and the bounds are reachable by honest fp32), every row of the tables is on the branch it names (the
dispatch conditions of csrc/wfold.hip, img_grid, the tap block sizes and the two loops of tap_rows_sum_kernel restated in
boundary_ref), the union of the rows' `reaches` is the full list of branches, and every mutant statement is rejected by the
criterion on at least one case. torch's fp32 tanh stays inside the allowance the GPU test gives the kernels' tanhf."""
import ctypes

import pytest
import torch

from oracle.ops_ref import RefOps
from tests import boundary_ref as R
from tests.test_boundary_edges_gpu import TANH_ULPS
from tests.test_pnorm_edges_gpu import K, K2

RUN_IDS = [f"{op}-{n}-{d}" for op, n, d in R.RUNS]


@pytest.mark.parametrize("op,name,data", R.RUNS, ids=RUN_IDS)
def test_fp32_oracle_meets_every_criterion(op, name, data):
    """RefOps on guarded, pre-filled buffers against the float64 statement, with the constants of the GPU test.
    RefOps.image_tap_scatter is autograd of F.pad + indexing: its colliders add up in autograd's order, not in sample order,
    so on random data it is held to the fp32 sum bound (K2 over the colliders' absolute sum) and to the bits on the pixels
    with at most two colliders (a + b is commutative); the sample-order bits are the kernel's promise, not the oracle's."""
    b = R.build(op, name, data)
    got = R.run(RefOps(), b)
    if op == "img_tap":
        ref = b.ref["scatter"]
        mine, want = got["scatter"], R.round_to(ref.value, R.F32)
        count = torch.zeros(b.case.H * b.case.W).index_add_(0, b.tgt, torch.ones(b.case.P)).view(b.case.H, b.case.W)
        assert torch.equal(mine[..., count <= 2], want[..., count <= 2])
        T = torch.zeros(R.N, 3, b.case.H * b.case.W, dtype=torch.float64).index_add_(2, b.tgt, b.g.double().abs().movedim(1, 2))
        assert R.worst(R.f32_excess(mine.view(R.N, 3, -1), ref.value.view(R.N, 3, -1), T)) <= K2
        got["scatter"] = want
    m = R.judge(b, got)
    print(f"BOUNDARY_REFOPS {op} {name} {data} k={m['k']:.3f} k2={m['k2']:.3f} tanh={m['tanh']:.2f}")
    assert R.accept(m, K, K2, TANH_ULPS), (b.case.reaches, m)


def test_rounding_reference():
    """round_to is round-to-nearest-even on the special values; the ties-away mutant differs exactly on the ties whose
    bf16 below is even"""
    want = R._f32_bits(0x3F800000, 0x3F820000, 0xBF800000, 0xBF820000, 0x00000000, 0x80000000, 0x7F7F0000, 0x7F800000,
                       0xFF7F0000, 0xFF800000, 0x3F800000, 0x3F810000)
    got = R.round_to(R.SPECIALS.double(), R.BF16)
    assert R.same_bits(got, want.to(R.BF16)) and R.same_bits(got.float(), want)
    away = R.round_to(R.SPECIALS.double(), R.BF16, ties_away=True)
    differs = (away.view(torch.int16) != got.view(torch.int16)).nonzero().flatten().tolist()
    assert differs == [0, 2]
    assert not R.same_bits(torch.tensor([0.0]), torch.tensor([-0.0])) and R.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]), False)
    r = torch.tensor([1.0, 0.75, 0.0, 2.0 ** -130], dtype=torch.float64)
    assert R.ulp32(r).tolist() == [2.0 ** -23, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149]


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_mutant_is_rejected(mut):
    """the wrong statement, rounded to the outputs' types as a kernel would leave it, fails the criterion on some case"""
    small = [c for c in R.ALL_CASES if c.op != "zeros" and getattr(c, "H", 1) * getattr(c, "W", 1) < 100000
             and getattr(c, "P", 1) <= 65]
    rejected = []
    for c in small:
        b = R.build(c.op, c.name, "random")
        if not R.accept(R.judge(b, R.fake(b, mut)), K, K2, TANH_ULPS):
            rejected.append(f"{c.op}/{c.name}")
            if len(rejected) >= 3:
                break
    print(f"BOUNDARY_MUTANT {mut} rejected on {rejected}")
    assert rejected, f"{mut} passes every case"


def test_the_unmutated_statement_is_accepted():
    """fake() of the right statement passes with K = 0, K2 = 1 and 2 ulps (fake's tanh is of the unrounded s: half an ulp of s,
    carried through a slope <= 1, on top of its own rounding): the mutant test rejects the mutation, not the rounding of fake()"""
    for c in R.ALL_CASES:
        if getattr(c, "H", 1) * getattr(c, "W", 1) < 100000 and getattr(c, "P", 1) <= 65 and c.op != "zeros":
            b = R.build(c.op, c.name, "random")
            assert R.accept(R.judge(b, R.fake(b, None)), 0, 1, 2), (c.op, c.name)


# ---- the tables against the launch plans ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ALL_CASES, ids=lambda c: f"{c.op}-{c.name}")
def test_case_is_on_its_branch(case):
    claimed = set(case.reaches.split(", "))
    assert claimed and claimed <= R.tags_of(case), f"{case.name}: claims {sorted(claimed - R.tags_of(case))}, is on {sorted(R.tags_of(case))}"
    assert claimed <= set(R.BRANCHES)


def test_tables_reach_every_branch():
    reached = set().union(*(set(c.reaches.split(", ")) for c in R.ALL_CASES))
    assert sorted(reached) == R.BRANCHES, (sorted(set(R.BRANCHES) - reached), sorted(reached - set(R.BRANCHES)))


def test_plans_restate_the_dispatch():
    """the numbers the issue names, through the restated conditions"""
    assert R.unfold_plan(3, 257) == dict(row=True, segs=2, last=1) and R.unfold_plan(3, 520)["segs"] == 3
    assert R.unfold_plan(46, 15)["row"] and not R.unfold_plan(47, 15)["row"] and not R.unfold_plan(64, 15)["row"]
    assert not R.unfold_plan(3, 15, rows_opt=0)["row"]
    assert R.unfold_bwd_plan(3, 1024, 24) == dict(row=True, why=None, passes=4, lds=48 * 1024)
    assert [R.unfold_bwd_plan(*a)["why"] for a in ((3, 1025, 24), (4, 800, 32), (5, 15, 40))] == ["W", "lds", "C"]
    assert not R.shiftadd_plan(15, 72)["row"] and R.shiftadd_plan(15, 64)["row"]
    assert R.shiftadd_bwd_plan(4, 256) == dict(row=True, segs=2, last=6) and R.shiftadd_bwd_plan(4, 250) == dict(row=True, segs=1, last=256)
    assert not R.shiftadd_bwd_plan(17, 15)["row"]
    assert not R.img_grid_plan(1024 * 256)["strided"] and R.img_grid_plan(513 * 512)["strided"]
    assert [R.tap_block(c) for c in (1, 64, 65, 255, 256, 300)] == [64, 64, 128, 128, 256, 256]
    assert R.rows_sum_plan(128, 32) == dict(unrolled=32, tail=0, blocks=1, idle=False)
    assert R.rows_sum_plan(97, 33) == dict(unrolled=1, tail=31, blocks=2, idle=True)


def test_single_source_rows():
    c = R.BY_NAME[("unfold_bwd", "reflect3_h5")]
    assert R.single_source_rows(c).tolist() == [[True, False, False, False, True]]
    c = R.BY_NAME[("unfold_bwd", "replicate3_h1")]
    assert R.single_source_rows(c).tolist() == [[False]]


def test_unfold_statement_is_the_stem_conv():
    """conv2d(pad(x), w) == the W-less conv of the unfolded image with the taps moved into the channels"""
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 9, 15, generator=gen, dtype=torch.float64)
    w = torch.randn(5, 3, 7, 7, generator=gen, dtype=torch.float64)
    for mode in ("reflect", "replicate", "zero"):
        want = torch.nn.functional.conv2d(R.pad_sp(x, [(3, 3), (3, 3)], mode), w)
        u = R.unfold64(x, 7, 3, mode, fold_=3)                                        # [N, H + 6, W, 7 C]
        w2 = w.permute(0, 3, 1, 2).reshape(5, 21, 7, 1)                               # [O, (dw, c), kh, 1]
        got = torch.nn.functional.conv2d(u.movedim(-1, 1), w2)
        assert torch.allclose(got, want, rtol=0, atol=1e-12), mode


def test_refusals_come_before_any_launch():
    """the library's checks, called with no GPU in reach: each returns its error code and a message (the pointers are fakes
    that a launch would never get to see)"""
    from ganslate_amd.hip import lib as L
    if not L.library_path().is_file():
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    p = ctypes.c_void_p(4096)
    calls = [
        lib.gs_image_to_act_backward(p, p, 1, 1, 1, 5, 5, 8, 4, L.BORDER["replicate"], 0, None),
        lib.gs_image_unfold_backward(p, p, 1, 1, 1, 5, 15, 8, 7, 3, 4, L.BORDER["replicate"], 0, None),
        lib.gs_image_unfold(p, p, 1, 2, 2, 15, 8, 7, 3, L.BORDER["reflect"], None),
        lib.gs_image_unfold(p, p, 1, 1, 2, 15, 12, 7, 3, L.BORDER["reflect"], None),
        lib.gs_image_cat_to_act((ctypes.c_void_p * 2)(4096, 4096), (ctypes.c_int64 * 2)(3 * 4, 6 * 4), (ctypes.c_int32 * 2)(3, 6), 2,
                                p, 1, 4, 8, None),                   # 3 + 6 source channels, Cp = 8
        lib.gs_image_tap_scatter(p, 1, 1, 4, 4, 0, p, 16385, p, None),
        lib.gs_image_to_act_backward(p, p, 1, 1, 1, 3, 5, 8, 3, L.BORDER["reflect"], 0, None),
        lib.gs_image_to_act_backward(p, p, 1, 1, 2, 5, 5, 8, 2, L.BORDER["reflect"], 0, None),
        lib.gs_image_unfold(p, p, 1, 1, 2, 3, 8, 7, 3, L.BORDER["reflect"], None),
        lib.gs_image_unfold_backward(p, p, 1, 1, 1, 2, 15, 8, 7, 3, 2, L.BORDER["reflect"], 0, None),
        lib.gs_image_unfold_backward(p, p, 1, 1, 2, 5, 15, 8, 7, 3, 2, L.BORDER["reflect"], 0, None),
    ]
    assert all(rc == 2 for rc in calls), calls                       # 2: a refused argument; 1 would be a failed HIP call
    assert b"gs_image_unfold_backward" in lib.gs_last_error()
