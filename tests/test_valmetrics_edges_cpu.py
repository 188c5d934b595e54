"""tests/valmetrics_edges_ref.py without a GPU: the case table covers every branch name the plan mirror knows and states what
the mirror computes; the float64 statement of the kernels (their summation order) meets the judge's bounds against the
extended-precision reference on every case; the older restatements agree with the reference inside their own tolerances; numpy
accepts every histogram case and its 1-D and 2-D histograms agree; and the judge rejects six wrong variants of the statement,
each on a named case."""
import numpy as np
import pytest

from tests import valmetrics_edges_ref as R
from tests import valmetrics_masked_ref as mref
from tests import valmetrics_ref as ref
from tests.test_valmetrics_edges_gpu import K_HIST, K_SSIM, PSNR_ULPS

NAMES = [c.name for c in R.CASES]
SMALL = [c.name for c in R.CASES if c.S * c.N <= 1 << 16]


def test_every_branch_is_reached_and_every_row_states_what_the_mirror_computes():
    reached = set()
    for c in R.CASES:
        got = R.mirror(c, *R.built(c.name)[1:4])
        assert got <= set(R.BRANCHES), (c.name, got - set(R.BRANCHES))
        assert set(c.reaches) == got, (c.name, sorted(got))
        reached |= got
    assert reached == set(R.BRANCHES), set(R.BRANCHES) - reached
    assert not set(R.UNREACHABLE) & set(R.BRANCHES)
    assert len(set(NAMES)) == len(NAMES) and set(R.GUARDED) <= set(NAMES) and set(R.MUTANTS.values()) <= set(NAMES)
    assert all(c.alone[0] in R.BY_NAME for c in R.CASES if c.alone)


def test_the_plan_mirror_on_the_shapes_the_cases_were_chosen_for():
    assert R.moment_blocks(65537) == 9 and [R.chunk(65537, b, 9)[:2] for b in (7, 8)] == [(57344, 65536), (65536, 65537)]
    S = 8 * 262145
    assert (R.moment_blocks(S), R.hist_blocks(S), R.chunk_len(S, 256), R.chunk_len(S, 257)) == (256, 257, 9216, 8192)
    assert R.chunk(S, 227, 256) == (227 * 9216, S, False) and R.chunk(S, 228, 256) == (S, S, True)
    assert R.chunk(S, 256, 257) == (256 * 8192, S, False)               # the 257th histogram chunk holds eight elements
    S = 8 * 524289
    assert (R.moment_blocks(S), R.hist_blocks(S), R.chunk_len(S, 512)) == (256, 512, 9216)
    assert R.chunk(S, 455, 512)[2] is False and R.chunk(S, 456, 512) == (S, S, True)
    for S in (1, 147, 8192, 8193, 65537, 8 * 262145):                   # the chunks tile [0, S) in order, whatever nb is
        for nb in (R.moment_blocks(S), R.hist_blocks(S)):
            ends = [R.chunk(S, b, nb)[:2] for b in range(nb)]
            assert ends[0][0] == 0 and ends[-1][1] == S and all(a[1] == b[0] for a, b in zip(ends, ends[1:]))
            assert all(b0 % 1024 == 0 or b0 == S for b0, _ in ends)
    assert R.vec_load(128, 0) and not R.vec_load(128, 4) and not R.vec_load(147, 0)
    assert R.word_pack([0, 4]) and not R.word_pack([0, 2])
    assert R.pack_grid(1, 147, True) == (36, 1) and R.pack_grid(1, 128, False) == (0, 1)
    assert R.pack_grid(1, 8 * 262145, False) == (0, 2048) and R.pack_grid(2, 4096, True) == (2048, 2)
    assert R.ssim_tiles(14, 20) == {"group_full", "group_idle", "cols_partial"}
    assert R.ssim_tiles(15, 20) >= {"group_full", "group_partial", "group_one_row", "group_idle"}
    assert R.ssim_tiles(38, 70) == {"group_full", "cols_full"}
    assert R.ssim_tiles(39, 71) >= {"group_one_row", "cols_one", "group_idle"}
    assert R.scratch_bytes(2, 2, 71, 76) == (2 * 2 * 8 + 2 * 2 * 3 * 2) * 8
    assert R.masked_scratch_bytes(2, 8, 2, 71, 76) == (2 * 2 * 8 * 10 + 2 * 2 * 6 * 8) * 8 + 2 * 10792 + 0


@pytest.mark.parametrize("name", NAMES)
def test_the_float64_statement_meets_the_judge(name):
    case, t, p, masks, rows = R.built(name)
    assert R.LD_OK or case.S <= 4096
    assert R.terms_are_exact(t, p)
    table, counts = R.statement(case, t, p, masks)
    judged = R.judge(case, table, counts, rows)
    print(f"VALMETRICS_CPU_EXCESS {name} " + " ".join(f"{k}={v:.3f}" for k, v in R.worst(judged).items()))
    for where, m, want in judged:
        assert R.accept(m, want, K_SSIM, K_HIST, PSNR_ULPS), (where, m)
        for k, terms in (("nmi", "n_nmi"), ("histogram_chi2", "n_chi2")):          # no hist bound looser than the older 1e-9
            assert R.hist_k(want, K_HIST)[k] * R.U * max(want[terms], 1) <= R.HIST_REL_CAP * (1 + 1e-12)


@pytest.mark.parametrize("name", SMALL)
def test_the_older_restatements_agree_with_the_reference(name):
    case, t, p, masks, rows = R.built(name)
    fin = lambda a, b: np.isfinite(float(a)) and np.isfinite(float(b))
    for n in range(case.N):
        for l in range(max(case.L, 1)):
            want = rows[n][l]
            names = [k for k in R.COLUMNS if case.ssim or k != "ssim"]
            old = {}
            for k in names:                       # the older nmi divides Python floats: 0 / 0 raises where the kernel has NaN
                try:
                    with np.errstate(all="ignore"):
                        old[k] = mref.metrics(t[n], p[n], masks[l][n] != 0, [k])[k] if masks else ref.FNS[k](t[n], p[n])
                except ZeroDivisionError:
                    old[k] = float("nan")
            for k, v in old.items():
                if not fin(v, want[k]):
                    assert R._same_special(v, want[k]) or k in ("ssim", "nmi"), (n, l, k, v, want[k])
                elif k == "ssim":
                    assert abs(v - float(want[k])) <= 1e-5, (n, l, v, want[k])
                else:
                    assert v == pytest.approx(float(want[k]), rel=1e-9, abs=0), (n, l, k)


@pytest.mark.parametrize("name", NAMES)
def test_numpy_accepts_every_histogram_case_and_its_histograms_agree(name):
    case, t, p, masks, rows = R.built(name)
    for n in range(case.N):
        for l in range(max(case.L, 1)):
            tm, pm = mref.products(t[n], p[n], masks[l][n] != 0) if masks else (t[n], p[n])
            ht, hp, hj = rows[n][l]["counts"]                                           # np.histogram / np.histogramdd raised nothing
            assert ht.sum() == hp.sum() == hj.sum() == case.S
            assert (hj.sum(1) == ht).all() and (hj.sum(0) == hp).all()
            if case.S <= 1 << 16:
                tt, _ = np.histogramdd([tm.reshape(-1), tm.reshape(-1)], bins=R.BINS)
                assert (np.diag(tt) == ht).all() and tt.sum() == case.S
            for x in (tm, pm):                                                          # vm_edge is numpy's edge, bit for bit
                e, _ = np.histogram(x, bins=R.BINS)[1], None
                assert e.dtype == np.float32 and (np.diff(e) > 0).all()
                assert np.array_equal(R.vm_edges(x.min(), x.max())[0].view(np.int32), e.view(np.int32))


def test_the_edge_cases_put_values_on_and_next_to_every_edge():
    for c in R.CASES:
        if c.kind != "edges":
            continue
        t = R.built(c.name)[1].reshape(-1)
        e = R.f32_edges(*c.rng)
        assert t.min() == e[0] == np.float32(c.rng[0]) and t.max() == e[-1] == np.float32(c.rng[1])
        assert np.isin(e, t).all()
        assert np.isin(np.nextafter(e[1:], np.float32(-np.inf)), t).all()
        assert np.isin(np.nextafter(e[:-1], np.float32(np.inf)), t).all()


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_the_judge_rejects_a_wrong_statement(mutant):
    case, t, p, masks, rows = R.built(R.MUTANTS[mutant])
    ok = lambda judged: all(R.accept(m, want, K_SSIM, K_HIST, PSNR_ULPS) for _, m, want in judged)
    assert ok(R.judge(case, *R.statement(case, t, p, masks), rows))
    assert not ok(R.judge(case, *R.statement(case, t, p, masks, mutant=mutant), rows)), mutant


def test_the_judge_rejects_one_wrongly_scored_pixel_and_one_ulp_of_a_sum():
    """what the older tolerances let through: one SSIM pixel of 3 x 71 x 76 scored 0 instead of about 1, and a relative 1e-11 on
    a sum"""
    case, t, p, masks, rows = R.built("tiles_3x2")
    table, counts = R.statement(case, t, p, masks)
    ok = lambda tab: all(R.accept(m, want, K_SSIM, K_HIST, PSNR_ULPS) for _, m, want in R.judge(case, tab, counts, rows))
    assert ok(table)
    for col, delta in ((4, -1.0 / (case.P * (case.H - 6) * (case.W - 6))), (0, table[0, 0] * 1e-11), (5, table[0, 5] * 1e-9)):
        bad = table.copy()
        bad[0, col] += delta
        assert abs(delta) < 2e-4 and not ok(bad), col
