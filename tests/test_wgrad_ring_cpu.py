"""The cases of tests/test_wgrad_ring_gpu.py (the K loop of wgrad_kernel, csrc/wgrad.hip: a 3-stage LDS-DMA ring two K-steps
ahead, fragment reads with counted waits) and what licenses them, checked without a GPU:

  * every case lies on the integer domain of tests/exact.py (every partial sum below 2^24), so the kernel must agree with the
    float64 reference bit for bit in any summation order;
  * every case sits on the branch it is meant for: tile shape, depth bookkeeping, number of pixel splits and number of K-steps
    (64 dense-side pixels each) per split, from the split / chunk rule of launch_wgrad_impl restated here — and, where the
    library is built, from the library's own planning call with the halo-resident and pointwise kernels switched off.
"""
import ctypes as C

import pytest
import torch

from ganslate_amd.nn.native.spec import ConvSpec
from tests import exact

BK = 64                                                     # dense-side pixels per K-step
# the library's own switches: nothing but the im2col kernel takes a weight gradient
IM2COL_ONLY = dict(hwgrad=0, hwgrad_wide=0, hwgrad_ft=0, hwgrad2=0, pwise=0)
PREFILL_W, PREFILL_B = 7.0, -5.0


def launch_rule(w, N, nets=1):
    """wgrad_generic's tile choice and launch_wgrad_impl's split / chunk rule (csrc/wgrad.hip) for N images (of `nets` networks)"""
    P, TQ = w.P, w.T * w.Q
    BP = 16 if P <= 16 else 64 if P <= 64 else 128
    tiles = -(-P // BP) * -(-TQ // 256) * nets
    M = N // nets * w.Da * w.Ha * w.Wa
    max_splits = max((M + 1023) // 1024, 1)
    best, splits = 1e30, 1
    for r in range(1, 5):
        s = min(max(256 * r // tiles, 1), max_splits)
        rounds = (tiles * s + 255) // 256
        cost = rounds * (M / s + 512.0)
        if cost < best:
            best, splits = cost, s
    chunk = (-(-M // splits) + 63) // 64 * 64
    splits = -(-M // chunk)
    ksteps = [-(-(min(M, (s + 1) * chunk) - s * chunk) // BK) for s in range(splits)]
    return dict(BP=BP, vol=not (w.Da == 1 and w.Dg == 1), row_tiles=-(-P // BP), col_tiles=-(-TQ // 256), M=M, splits=splits,
                chunk=chunk, ksteps=ksteps, ws_floats=0 if splits == 1 else nets * splits * P * TQ)


K3 = ConvSpec("conv", 16, 128, 3, 1, 1)                     # P = 128, T * Q = 144: one masked column tile
# (id, spec, N, sizes, tile rows BP, volume form, dense-side pixels M, K-steps per split)
CASES = [
    # K-steps per workgroup with one split
    ("1-kstep", K3, 1, (8, 8), 128, False, 64, [1]),                  # the prologue issues stage 0 only
    ("2-ksteps", K3, 2, (8, 8), 128, False, 128, [2]),                # both stages from the prologue, none issued in the loop
    ("3-ksteps", K3, 3, (8, 8), 128, False, 192, [3]),                # the first in-loop issue, then two iterations without one
    ("5-ksteps", K3, 5, (8, 8), 128, False, 320, [5]),                # the ring wraps onto buffer 0
    ("63-pixels", K3, 1, (7, 9), 128, False, 63, [1]),                # one partial K-step
    ("135-pixels", K3, 1, (9, 15), 128, False, 135, [3]),             # the last K-step has 7 real pixels
    # every instantiation and gather form
    ("p8-reflect", ConvSpec("conv", 64, 8, 3, 1, 1, pad_mode="reflect"), 1, (10, 13), 16, False, 130, [3]),   # T * Q = 576: 3 tiles
    ("p40-stride2", ConvSpec("conv", 16, 40, 3, 2, 1), 2, (21, 27), 64, False, 308, [5]),                     # ragged row tile
    ("p128-convT", ConvSpec("convT", 128, 64, 3, 2, 1, 1), 1, (8, 12), 128, False, 96, [2]),                  # dense side = X
    ("p256-k4-stride2", ConvSpec("conv", 64, 256, 4, 2, 1), 3, (16, 16), 128, False, 192, [3]),               # two row tiles
    ("volume-pow2", ConvSpec("conv", 16, 128, 3, 2, 1, dims=3), 2, (8, 8, 16), 128, True, 256, [4]),
    ("volume-3x5x7", ConvSpec("conv", 8, 16, 3, 1, 1, pad_mode="replicate", dims=3), 3, (3, 5, 7), 16, True, 315, [5]),
    ("volume-p40", ConvSpec("conv", 8, 40, 3, 1, 1, dims=3), 1, (3, 5, 7), 64, True, 105, [2]),
]
# several splits: 3 images of 20 x 20 dense pixels = 2 splits of 640 and 560 pixels; the chunk boundary (pixel 640) and the
# image boundaries (400, 800) fall inside K-steps of the lanes' row walk
SPLIT = ("2-splits", ConvSpec("conv", 16, 128, 3, 1, 1, pad_mode="reflect"), 3, (20, 20), 128, False, 1200, [10, 9])
ALL = CASES + [SPLIT]
_ids = lambda c: c[0]


def case_of(case, seed=71):
    return exact.make_case(case[1], case[2], case[3], seed=seed, prefill=PREFILL_W, check=("wgrad",))


_REF = {}


def reference(c):
    """float64 weight and bias gradient of a case from the ConvSpec alone (exact.wgrad_ref64), as float32 [P][T][Q] / [cout_p];
    computed once per case"""
    if id(c) not in _REF:
        sp = c.spec
        dw = exact.master_of(sp, exact.wgrad_ref64(sp, c.xa, c.gy).float()).reshape(sp.P, sp.T, sp.Q)
        db = torch.zeros(sp.cout_p)
        db[:exact.cout_of(sp)] = exact.bias_grad_ref64(sp, c.gy).float()
        _REF[id(c)] = (dw, db)
    return _REF[id(c)]


def wdesc(w, N, a_cs, g_cs):
    from ganslate_amd.hip.ops import HipOps
    return HipOps._wdesc(None, w, N, a_cs, 0, g_cs, 0)


def assert_on_its_branch(lib, case, c, nets=1):
    """the library's own plan (halo-resident / pointwise kernels off: the caller's job) agrees with launch_rule: workspace floats
    = splits x P x T x Q (0 for one split), and a one-split layer is what gs_wgrad_adam_eligible calls a one-split im2col launch"""
    sp, w = c.spec, c.low.wgrad
    rule = launch_rule(w, c.N * nets, nets)
    d = wdesc(w, c.N * nets, sp.P, sp.Q)
    if nets == 2:
        assert lib.gs_wgrad_twin_native(C.byref(d), 0) == 1, "no twin form of the im2col kernel for this layer"
        got = lib.gs_wgrad_ws_floats_twin(C.byref(d), 0)
    else:
        got = lib.gs_wgrad_ws_floats(C.byref(d), 0)
    assert got == rule["ws_floats"], (case[0], got, rule)
    if rule["splits"] == 1 and nets == 1:
        assert lib.gs_wgrad_adam_eligible(C.byref(d)) == 1, f"{case[0]}: not a one-split launch of the im2col kernel"
    return rule


@pytest.mark.parametrize("case", ALL, ids=_ids)
def test_case_lies_on_the_exact_domain(case):
    c = case_of(case)                                       # (make_case runs exact.assert_exact_domain)
    assert c.bounds["wgrad_sum_abs"] < exact.LIMIT and c.bounds["bias_grad_sum_abs"] < exact.LIMIT
    dw, db = reference(c)
    assert dw.abs().max() > 0 and torch.equal(dw, dw.round()), "the reference is not a non-trivial integer gradient"
    assert (dw.abs() + abs(PREFILL_W)).max() < exact.LIMIT and (db.abs() + abs(PREFILL_B)).max() < exact.LIMIT


@pytest.mark.parametrize("case", ALL, ids=_ids)
def test_case_takes_its_branch_by_the_launch_rule(case):
    _, spec, N, sizes, BP, vol, M, ksteps = case
    w = case_of(case).low.wgrad
    assert w.P == spec.P and w.Q == spec.Q and w.T == spec.T
    rule = launch_rule(w, N)
    assert (rule["BP"], rule["vol"], rule["M"], rule["ksteps"]) == (BP, vol, M, ksteps), rule
    assert rule["splits"] == len(ksteps)
    assert M <= 1024 or case is SPLIT


def test_the_cases_reach_every_instantiation_and_gather_form():
    rules = [(c, launch_rule(case_of(c).low.wgrad, c[2])) for c in ALL]
    assert {(r["BP"], r["vol"]) for _, r in rules} == {(bp, v) for bp in (16, 64, 128) for v in (False, True)}
    assert {r["ksteps"][0] for c, r in rules if c[1] is K3} == {1, 2, 3, 5}
    assert any(r["row_tiles"] == 2 for _, r in rules) and any(c[1].P % r["BP"] for c, r in rules)          # two row tiles; ragged
    assert any(r["col_tiles"] > 1 and (c[1].T * c[1].Q) % 256 for c, r in rules)                           # masked last column tile
    assert any(r["M"] % BK for _, r in rules)
    forms = {(c[1].kind, c[1].stride, c[1].pad_mode) for c in ALL}
    assert {("conv", 1, "zero"), ("conv", 2, "zero"), ("conv", 1, "reflect"), ("convT", 2, "zero")} <= forms
    M = [r["M"] for _, r in rules if r["vol"]]
    assert any(m & (m - 1) == 0 for m in M) and any(m & (m - 1) for m in M)                                # volume: 2^k and ragged


def test_the_split_case_and_its_twin():
    w = case_of(SPLIT).low.wgrad
    one, twin = launch_rule(w, 3), launch_rule(w, 6, nets=2)
    for r in (one, twin):
        assert (r["splits"], r["chunk"], r["ksteps"]) == (2, 640, [10, 9])
    assert one["chunk"] % 400 and 400 % BK and 800 % BK and (1200 - 640) % BK            # boundaries inside K-steps, ragged end
    assert one["ws_floats"] == 2 * w.P * w.T * w.Q and twin["ws_floats"] == 2 * one["ws_floats"]


def test_the_library_plans_what_the_rule_says():
    """the same answers from libganslate_hip.so's planning calls (no GPU call is made)"""
    from ganslate_amd.hip import lib as L
    if not L.library_path().is_file():
        pytest.skip("libganslate_hip.so is not built")
    lib = L.load()
    before = {}
    for o in IM2COL_ONLY:
        v = C.c_int(0)
        assert lib.gs_get_option(o.encode(), C.byref(v)) == 0
        before[o] = v.value
    try:
        for o, v in IM2COL_ONLY.items():
            assert lib.gs_set_option(o.encode(), v) == 0
        for case in ALL:
            assert_on_its_branch(lib, case, case_of(case))
        assert_on_its_branch(lib, SPLIT, case_of(SPLIT), nets=2)
    finally:
        for o, v in before.items():
            lib.gs_set_option(o.encode(), v)
