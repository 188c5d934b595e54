"""csrc/valmetrics.hip (HipOps.valmetrics / valmetrics_masked) on every branch of its launch plan against the
extended-precision reference of tests/valmetrics_edges_ref.py (each case's `reaches` names its branches;
tests/test_valmetrics_edges_cpu.py proves the cases are on them, that the float64 statement of the kernels meets the same
bounds, and that the judge rejects six wrong variants).

Per column (the judge is stated in valmetrics_edges_ref's docstring): bin counts exact; NaN and +-inf where the reference has
them; mae / mse within depth * 2^-53 relative and nmse within twice that, depth (25 .. 92 over the cases) derived from the
launch plan; psnr within that bound through the logarithm plus PSNR_ULPS ulps; ssim within K_SSIM * 2^-53 * kappa; nmi and
histogram_chi2 within K_HIST * 2^-53 * (non-empty terms) relative, never looser than 1e-9. Every case runs twice and must
repeat bit for bit; an L = 1 case named `alone` must equal its label of the L = 8 call bit for bit; an all-ones label has the
unmasked call's counts bit for bit and its table within the same bounds. The guarded runs make the library calls on
0xFF-filled table, counts and scratch and must equal the wrapper's results bit for bit, one extra table row untouched.

Measured on an MI355X over all cases, against the extended-precision reference (the largest excess and its case; the float64
statement of the kernels on the CPU has the same excess to the three digits shown on every case, since it keeps their order):
  mae   0.029 of its bound  m_L8_n3_s99          mse   0.096 of its bound  m_L1
  nmse  0.043 of its bound  base_plus_one_float  (these three bounds are derived, depth * 2^-53, and asserted at K = 1)
  psnr  0 ulps beyond the analytic part on every case -> PSNR_ULPS = 1: the floor, one rounding for the product with 10,
        which the analytic part does not count (the cap is 4)
  ssim  2.143  m_L8 (the one-element label of sample 1)  -> K_SSIM = 5 (twice, rounded up; the cap is 64)
  nmi   0.123  m_L8_n3_s99          histogram_chi2  0.042  m_L8_n3_s99  -> K_HIST = 1 (twice 0.123, rounded up)
Every count is exact, every NaN and infinity where the reference has it, every case repeats bit for bit, the L = 1 cases equal
their label of the L = 8 calls, the guarded calls equal the wrapper's. With K_HIST = 1 the loosest histogram bound of a case is
2^-53 * 6 599 terms = 7.3e-13 relative (1e-9 before); the sums are held to 2.8e-15 .. 1.0e-14 (1e-9 before); ssim to
5 * 2^-53 * kappa, at most 5.9e-12 over the cases (1e-5 before).
The slowest case (hist_capped, 4.2 M elements) takes 1.36 s and mom_capped 0.65 s, their references on the CPU included; every
other case at most 0.2 s; the whole file 5.3 s.
"""
import time

import numpy as np
import pytest
import torch

from tests import valmetrics_edges_ref as R

pytestmark = pytest.mark.gpu

SUMS_MEASURED = dict(mae=0.029, mse=0.096, nmse=0.043)      # fractions of the derived bound (K = 1 is asserted)
K_SSIM_MEASURED = 2.143
K_HIST_MEASURED = dict(nmi=0.123, histogram_chi2=0.042)
PSNR_ULPS_MEASURED = 0.0
CPU_STATEMENT_MEASURED = dict(ssim=2.143, nmi=0.123, histogram_chi2=0.042)
K_SSIM = 5                        # twice the measured excess, rounded up to a whole number
K_HIST = 1
PSNR_ULPS = 1                     # nothing measured beyond the analytic part: one ulp for the rounding of 10 * log10
assert 2 * K_SSIM_MEASURED <= K_SSIM <= R.K_SSIM_CAP
assert 2 * max(K_HIST_MEASURED.values()) <= K_HIST
assert 2 * PSNR_ULPS_MEASURED <= PSNR_ULPS <= R.PSNR_ULPS_CAP
assert max(SUMS_MEASURED.values()) <= 1.0

NAMES = [c.name for c in R.CASES]
_RESULTS = {}


def device_run(hip_ops, name):
    """the wrapper's (table, count words) of a case, run twice and required to repeat bit for bit; kept for the cases that
    are compared with each other"""
    if name not in _RESULTS:
        case, t, p, masks, _ = R.built(name)
        td, pd, md = R.to_device(case, t, p, masks, hip_ops.device)
        table, words = R.run(hip_ops, case, td, pd, md)
        table2, words2 = R.run(hip_ops, case, td, pd, md)
        assert np.array_equal(table.view(np.int64), table2.view(np.int64)), f"{name}: the table does not repeat"
        assert np.array_equal(words, words2), f"{name}: the counts do not repeat"
        _RESULTS[name] = (table, words, (td, pd, md))
    return _RESULTS[name]


def check(case, judged, what):
    for where, m, want in judged:
        assert R.accept(m, want, K_SSIM, K_HIST, PSNR_ULPS), (what, where, case.reaches, m, R.hist_k(want, K_HIST))


@pytest.mark.parametrize("name", NAMES)
def test_valmetrics_edge_case(hip_ops, name):
    t0 = time.perf_counter()
    case, t, p, masks, rows = R.built(name)
    table, words, (td, pd, md) = device_run(hip_ops, name)
    judged = R.judge(case, table, words, rows)
    w = R.worst(judged)
    ok = all(m["counts"] and m["special"] for _, m, _ in judged)
    print(f"VALMETRICS_EXCESS {name} " + " ".join(f"{k}={v:.3f}" for k, v in w.items())
          + f" exact={int(ok)} depth={R.depth_of(case)} seconds={time.perf_counter() - t0:.2f}")
    check(case, judged, "wrapper")
    if case.alone:
        other, label = case.alone
        big, big_words, _ = device_run(hip_ops, other)
        assert np.array_equal(table[:, 0].view(np.int64), big[:, label].view(np.int64)), f"L = 1 != label {label} of {other}"
        assert np.array_equal(words[:, 0], big_words[:, label])
    if "ones" in case.masks:
        label = case.masks.index("ones")
        plain = R.Case(case.name, case.shape, case.kind, ssim=case.ssim, offset=case.offset)
        ptable, pwords = R.run(hip_ops, plain, td, pd, [])
        assert np.array_equal(pwords, words[:, label]), "the all-ones label's counts differ from the unmasked call's"
        check(case, R.judge(plain, ptable, pwords, [[r[label]] for r in rows]), "unmasked call against the all-ones label")


@pytest.mark.parametrize("name", R.GUARDED)
def test_guarded_library_calls_write_every_word_they_read(hip_ops, name):
    case = R.BY_NAME[name]
    table, words, (td, pd, md) = device_run(hip_ops, name)
    gtable, gwords, extra, nbytes = R.run_guarded(hip_ops, case, td, pd, md)
    N, P, H, W = case.N, case.P, case.H, case.W
    assert nbytes == (R.masked_scratch_bytes(N, case.L, P, H, W) if case.masks else R.scratch_bytes(N, P, H, W))
    assert np.array_equal(gtable.view(np.int64), table.reshape(-1, 7).view(np.int64)), "a kernel read what no kernel wrote"
    assert np.array_equal(gwords, words.reshape(-1, R.HIST_WORDS))
    assert (extra == -1).all(), "the row past the table was written"


def test_refusals_and_planes_below_the_window(hip_ops):
    dev = hip_ops.device
    t = torch.rand(2, 1, 9, 30, device=dev)
    for n in (0, 9):
        with pytest.raises(ValueError):
            hip_ops.valmetrics_masked(t, t + 1, [torch.ones_like(t, dtype=torch.uint8)] * n)
    for hw in ((6, 9), (9, 6), (1, 1)):
        case = R.Case(f"plane_{hw[0]}x{hw[1]}", (1, 2) + hw, "uniform", masks=("rand40",), ssim=False)
        a, b, masks = R.data(case)
        td, pd, md = R.to_device(case, a, b, masks, dev)
        with pytest.raises(ValueError):
            hip_ops.valmetrics(td, pd)
        with pytest.raises(ValueError):
            hip_ops.valmetrics_masked(td, pd, md)
        check(case, R.judge(case, *R.run(hip_ops, case, td, pd, md), R.reference(case, a, b, masks)), "masked, no ssim")
        plain = R.Case(case.name, case.shape, case.kind, ssim=False)
        check(plain, R.judge(plain, *R.run(hip_ops, plain, td, pd, []), R.reference(plain, a, b, [])), "no ssim")
    torch.cuda.synchronize()
