"""Branch-complete edge cases for csrc/valmetrics.hip (gs_valmetrics / gs_valmetrics_masked): a plain Python mirror of the
launch plan, a case table, an extended-precision reference, a float64 statement in the kernels' summation order, and the
judge that tests/test_valmetrics_edges_cpu.py (no GPU) and tests/test_valmetrics_edges_gpu.py share.

Plan mirror: moment_blocks / hist_blocks / chunk / plan / mplan restate vm_moment_blocks, vm_hist_blocks, vm_chunk, vm_plan
and vmm_plan; vec_load / word_pack / pack_grid the `vec` and `words` decisions and the pack grid; ssim_tiles the tile and
row-group predicates of vm_ssim_tile. mirror(case) returns the branch names a case reaches (BRANCHES lists them all);
every CASES row states them in `reaches`, and the CPU test proves the two equal and that every name is reached.

Not reachable through the wrapper (so no case; UNREACHABLE says why): the scalar tail of a *vector* chunk. `vec` needs
S % 4 == 0, chunks start and end on multiples of 1024 or at S, so (b1 - b0) % 4 == 0 on every vector chunk and the tail
loop of vm_for_chunk runs only where it is the whole loop (the scalar path). The misaligned `bits` base is unreachable too:
the packed bits follow two slabs of doubles in a scratch buffer the allocator aligns.

Reference (per sample and label):
- counts: np.histogram / np.histogramdd through valmetrics_ref.bin_counts / valmetrics_masked_ref.bin_counts
- the three sums: math.fsum over exactly formed float64 terms. For float32 t, p every product t*t, t*p, p*p has at most
  48 significant bits, so it is exact in float64: sum (t-p)^2 = fsum(t*t, -2*t*p, p*p), sum |t-p| = fsum(s*t, -s*p) with
  s = sign(t - p), sum t^2 = fsum(t*t). terms_are_exact asserts that against np.longdouble (64-bit significand). fsum runs
  in blocks of 2^20 elements; every block result is the correctly rounded sum of a non-negative quantity, so the blocks add
  at most two roundings (counted in `depth`).
- ssim: the direct 7 x 7 window statement in np.longdouble (no cumulative sums), with the sample's condition number
  kappa = mean over interior pixels of |S| * ((uxx+uyy)/(vx+vy+C2) + (|uxy|+|ux*uy|)/|2*vxy+C2| + 1)
- nmi / histogram_chi2 from the integer counts in np.longdouble with numpy's float32 bin widths

Judge (per column; `excess` = error / bound at K = 1, so a column passes when excess <= its K):
- counts exact; NaN and +-inf in the reference's positions with its signs
- mae, mse: relative depth * 2^-53; nmse: twice that (a ratio of two such sums). depth = the per-thread terms of the largest
  chunk + the workgroup tree + the slab loop and its tree + the final division + the roundings that form a term (3) + the
  reference's own (3): derived from the plan mirror (sum_depth), not fitted
- psnr: absolute (depth + 2) * 2^-53 * 10 / ln 10 (the error of R^2 / mse through the logarithm), plus PSNR_ULPS ulps of
  the value for the device log10 and the multiplication by 10
- ssim: |got - ref| <= K_SSIM * 2^-53 * kappa
- nmi, histogram_chi2: relative K_HIST * 2^-53 * (non-empty terms), never looser than HIST_REL_CAP = 1e-9
"""
import functools
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from tests import valmetrics_masked_ref as mref
from tests import valmetrics_ref as ref

LD = np.longdouble
LD_OK = np.finfo(np.longdouble).nmant >= 63
U = 2.0 ** -53
THREADS, BINS, TW, TH, GROUP, MAX_LABELS, VM_MOM, VMM_MOM = 256, 100, 64, 32, 8, 8, 8, 10
HIST_WORDS = 2 * BINS + BINS * BINS
COLUMNS = ref.COLUMNS
K_SSIM_CAP = 64                 # the order of the count of roundings per pixel in vm_ssim_tile (28 per window moment + the formula)
PSNR_ULPS_CAP = 4
HIST_REL_CAP = 1e-9             # the tolerance of tests/test_valmetrics_gpu.py: no case may be judged looser


# ---- plan mirror ----------------------------------------------------------------------------------------------------
def moment_blocks(S):
    return min(max((S + 8191) // 8192, 1), 256)


def hist_blocks(S):
    return min(max((S + 8191) // 8192, 1), 512)


def chunk_len(S, nb):
    return ((S + nb - 1) // nb + 1023) // 1024 * 1024


def chunk(S, b, nb):
    """(b0, b1, clamped) of workgroup b of nb"""
    per = chunk_len(S, nb)
    b0 = b * per
    b1 = b0 + per if b0 + per < S else S
    clamped = b0 > S
    return (S if clamped else b0), b1, clamped


def plan(N, P, H, W):
    S = P * H * W
    q = dict(S=S, nb_mom=moment_blocks(S), nb_hist=hist_blocks(S), tiles_w=(W - 6 + TW - 1) // TW if W > 6 else 0,
             tiles_h=(H - 6 + TH - 1) // TH if H > 6 else 0)
    q["mom_doubles"] = N * q["nb_mom"] * VM_MOM
    q["ssim_doubles"] = N * P * q["tiles_w"] * q["tiles_h"]
    return q


def mplan(N, L, P, H, W):
    q = plan(N, P, H, W)
    q["mom_doubles"] = N * q["nb_mom"] * L * VMM_MOM
    q["ssim_doubles"] *= L
    q["bit_bytes"] = (N * q["S"] + 15) // 16 * 16
    return q


def scratch_bytes(N, P, H, W):
    q = plan(N, P, H, W)
    return (q["mom_doubles"] + q["ssim_doubles"]) * 8


def masked_scratch_bytes(N, L, P, H, W):
    q = mplan(N, L, P, H, W)
    return (q["mom_doubles"] + q["ssim_doubles"]) * 8 + q["bit_bytes"]


def vec_load(S, base_offset_bytes):
    return base_offset_bytes % 16 == 0 and S % 4 == 0


def word_pack(mask_offsets):
    return all(o % 4 == 0 for o in mask_offsets)


def pack_grid(N, S, words):
    """(nwords, blocks) of vmm_pack_kernel"""
    total = N * S
    nwords = total // 4 if words else 0
    items = nwords if nwords > 0 else total
    return nwords, min((items + 4 * THREADS - 1) // (4 * THREADS), 2048)


def ssim_tiles(H, W):
    """facts of the tile and row-group predicates of vm_ssim_tile over one plane"""
    Ho, Wo = H - 6, W - 6
    f = set()
    for y0 in range(0, Ho, TH):
        for g in range(TH // GROUP):
            rows = min(max(Ho - (y0 + g * GROUP), 0), GROUP)
            f.add("group_idle" if rows == 0 else "group_full" if rows == GROUP else "group_partial")
            if rows == 1:
                f.add("group_one_row")
    for x0 in range(0, Wo, TW):
        f.add("cols_full" if Wo - x0 >= TW else "cols_partial")
        if Wo - x0 == 1:
            f.add("cols_one")
    return f


def sum_depth(S, nb, vec, masked):
    """the count of roundings on the longest path of one of the three sums, from a term to its column"""
    longest = min(chunk_len(S, nb), S)
    terms = -(-longest // (4 * THREADS)) * 4 if vec else -(-longest // THREADS)
    tree = 9 if masked else 8                   # 8 halvings of 256, or 6 butterflies and 3 wave adds
    return terms + tree + -(-nb // THREADS) + tree + 1 + 3 + 3


BRANCHES = (
    # launch plan and loads
    "nb1", "nb_many", "mom_capped", "hist_ne_mom", "hist_capped", "vec", "scalar_misaligned", "scalar_s_mod4",
    "scalar_s_mod4_multi", "chunk_ragged", "chunk_one", "mom_chunk_empty", "mom_chunk_clamped", "hist_chunk_empty",
    "hist_chunk_clamped", "thread_loops",
    # ssim
    "ssim_off", "ssim_one_pixel", "rows_8", "rows_9", "tile_exact", "tile_plus_one", "group_idle", "group_partial",
    "cols_partial", "tiles_decode", "ssim_partials_gt_256",
    # data
    "ranges_differ", "r_nonpositive", "identical", "t_const", "p_const", "both_const_unequal", "both_const_equal", "t_zero",
    "all_zero", "on_edge", "next_to_edge",
    # masks
    "L1", "L_mid", "L8", "pack_words", "pack_tail", "pack_bytes", "pack_grid_capped", "pack_byte_values", "mask_ones",
    "mask_empty_sample", "mask_one_element", "mask_empty_chunks", "mask_last_chunk_only", "zero_first_edge",
    "zero_last_edge", "zero_mid_edge", "rm_negative",
)
UNREACHABLE = {
    "vec_tail": "vec needs S % 4 == 0 and chunks are multiples of 1024, so a vector chunk has no scalar tail",
    "bits_misaligned": "the packed bits follow two slabs of doubles in an aligned scratch buffer",
}


# ---- case table -----------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    shape: tuple                # N, C, H, W or N, C, D, H, W
    kind: str                   # data kind (data())
    masks: tuple = ()           # mask kinds (make_mask()); empty: the unmasked call
    reaches: tuple = ()
    ssim: bool = True
    offset: int = 0             # floats past a 16-byte boundary at which t and p start
    mask_offset: int = 0        # bytes past a 4-byte boundary at which every mask starts
    rng: tuple = ()             # (lo, hi) of the "edges" kind
    alone: tuple = ()           # (case name, label): this L = 1 case is that label of that case, bit for bit

    @property
    def N(self):
        return self.shape[0]

    @property
    def H(self):
        return self.shape[-2]

    @property
    def W(self):
        return self.shape[-1]

    @property
    def P(self):
        return int(np.prod(self.shape[1:-2]))

    @property
    def S(self):
        return self.P * self.H * self.W

    @property
    def L(self):
        return len(self.masks)


EDGE_RANGES = ((-1.0, 1.0), (0.0, 100.0), (-1000.5, 3000.25), (-1.0, 0.0), (1.0, 1.0 + 2e-5), (2.0 ** 24, 2.0 ** 24 + 200.0))
L8 = ("ones", "rand40", "one", "last_chunk", "box", "rand5", "checker", "empty0")

CASES = (
    # plan and load paths
    Case("s147_one_block", (1, 3, 7, 7), "uniform", reaches=("nb1", "scalar_s_mod4", "ssim_one_pixel", "group_idle",
                                                               "group_partial", "cols_partial")),
    Case("n3_s99", (3, 1, 9, 11), "ranges", reaches=("nb1", "scalar_s_mod4", "scalar_s_mod4_multi", "ranges_differ",
                                                       "group_idle", "group_partial", "cols_partial")),
    Case("base_plus_one_float", (2, 1, 8, 16), "uniform", offset=1,
         reaches=("nb1", "scalar_misaligned", "group_idle", "group_partial", "cols_partial")),
    Case("ragged_last_chunk", (1, 1, 95, 100), "ct", reaches=("nb_many", "vec", "chunk_ragged", "thread_loops",
                                                                "group_partial", "cols_partial")),
    Case("one_element_chunk", (1, 1, 1, 65537), "uniform", ssim=False,
         reaches=("nb_many", "scalar_s_mod4", "chunk_one", "thread_loops", "ssim_off")),
    Case("mom_capped", (1, 1, 8, 262145), "ct", ssim=False,
         reaches=("mom_capped", "hist_ne_mom", "vec", "chunk_ragged", "mom_chunk_empty", "mom_chunk_clamped", "thread_loops",
                  "ssim_off")),
    Case("hist_capped", (1, 1, 8, 524289), "uniform", ssim=False,
         reaches=("mom_capped", "hist_ne_mom", "hist_capped", "vec", "chunk_ragged", "mom_chunk_empty", "mom_chunk_clamped",
                  "hist_chunk_empty", "hist_chunk_clamped", "thread_loops", "ssim_off")),
    # ssim interior and tiling
    Case("rows_8", (1, 1, 14, 20), "uniform", reaches=("nb1", "vec", "rows_8", "group_idle", "cols_partial")),
    Case("rows_9", (1, 2, 15, 20), "ct", reaches=("nb1", "vec", "rows_9", "group_idle", "group_partial", "cols_partial")),
    Case("tile_exact", (1, 1, 38, 70), "uniform", reaches=("nb1", "vec", "tile_exact", "thread_loops")),
    Case("tile_plus_one", (1, 1, 39, 71), "ct", reaches=("nb1", "scalar_s_mod4", "tile_plus_one", "group_idle",
                                                          "group_partial", "cols_partial", "thread_loops")),
    Case("tiles_3x2", (2, 2, 71, 76), "ranges", reaches=("nb_many", "vec", "chunk_ragged", "ranges_differ",
                                                          "group_idle", "group_partial", "cols_partial", "tiles_decode",
                                                          "thread_loops")),
    Case("p300", (2, 300, 7, 7), "uniform", reaches=("nb_many", "vec", "chunk_ragged", "ssim_one_pixel", "group_idle",
                                                      "group_partial", "cols_partial", "ssim_partials_gt_256",
                                                      "thread_loops")),
    # data kinds
    Case("negative_target", (1, 1, 9, 12), "negative", reaches=("nb1", "vec", "r_nonpositive", "group_idle",
                                                                 "group_partial", "cols_partial")),
    Case("identical", (1, 2, 16, 20), "identical", reaches=("nb1", "vec", "identical", "group_idle", "group_partial",
                                                             "cols_partial")),
    Case("t_const", (1, 1, 9, 12), "t_const", reaches=("nb1", "vec", "t_const", "group_idle", "group_partial",
                                                        "cols_partial")),
    Case("p_const", (1, 1, 9, 12), "p_const", reaches=("nb1", "vec", "p_const", "group_idle", "group_partial",
                                                        "cols_partial")),
    Case("both_const_unequal", (1, 1, 9, 12), "const_unequal",
         reaches=("nb1", "vec", "t_const", "p_const", "both_const_unequal", "group_idle", "group_partial", "cols_partial")),
    Case("both_const_equal", (1, 1, 9, 12), "const_equal",
         reaches=("nb1", "vec", "t_const", "p_const", "both_const_equal", "identical", "group_idle", "group_partial",
                  "cols_partial")),
    Case("t_zero", (1, 1, 9, 12), "t_zero", reaches=("nb1", "vec", "t_const", "t_zero", "r_nonpositive", "group_idle",
                                                      "group_partial", "cols_partial")),
    Case("all_zero", (1, 1, 9, 12), "all_zero",
         reaches=("nb1", "vec", "t_const", "p_const", "both_const_equal", "identical", "t_zero", "all_zero", "r_nonpositive",
                  "group_idle", "group_partial", "cols_partial")),
) + tuple(
    Case(f"edges_{i}", (1, 1, 5, 61), "edges", ssim=False, rng=r,
         reaches=("nb1", "scalar_s_mod4", "thread_loops", "on_edge", "next_to_edge", "ssim_off") + (("r_nonpositive",) if r[1] <= 0 else ()))
    for i, r in enumerate(EDGE_RANGES)
) + (
    # masked
    Case("m_L1", (1, 3, 7, 7), "uniform", masks=("rand40",),
         reaches=("nb1", "scalar_s_mod4", "ssim_one_pixel", "group_idle", "group_partial", "cols_partial", "L1", "pack_words",
                  "pack_tail", "zero_mid_edge")),
    Case("m_L8", (2, 2, 71, 76), "uniform", masks=L8,
         reaches=("nb_many", "vec", "chunk_ragged", "group_idle", "group_partial", "cols_partial",
                  "tiles_decode", "thread_loops", "L8", "pack_words", "mask_ones", "mask_empty_sample", "mask_one_element",
                  "mask_empty_chunks", "mask_last_chunk_only", "zero_mid_edge", "zero_first_edge", "zero_last_edge",
                  "rm_negative")),
    Case("m_L8_label3_alone", (2, 2, 71, 76), "uniform", masks=("last_chunk",), alone=("m_L8", 3),
         reaches=("nb_many", "vec", "chunk_ragged", "group_idle", "group_partial", "cols_partial",
                  "tiles_decode", "thread_loops", "L1", "pack_words", "mask_empty_chunks", "mask_last_chunk_only",
                  "zero_mid_edge")),
    Case("m_L8_n3_s99", (3, 1, 9, 11), "ranges", masks=L8,
         reaches=("nb1", "scalar_s_mod4", "scalar_s_mod4_multi", "ranges_differ", "group_idle", "group_partial",
                  "cols_partial", "L8", "pack_words", "pack_tail", "mask_ones", "mask_empty_sample", "mask_one_element",
                  "zero_mid_edge", "zero_first_edge", "zero_last_edge", "rm_negative")),
    Case("m_L8_n3_s99_label5_alone", (3, 1, 9, 11), "ranges", masks=("rand5",), alone=("m_L8_n3_s99", 5),
         reaches=("nb1", "scalar_s_mod4", "scalar_s_mod4_multi", "ranges_differ", "group_idle", "group_partial",
                  "cols_partial", "L1", "pack_words", "pack_tail", "mask_one_element", "zero_mid_edge", "zero_first_edge")),
    Case("m_byte_values", (1, 1, 32, 32), "uniform", masks=("bytes", "bytes_sparse"),
         reaches=("nb1", "vec", "group_partial", "cols_partial", "L_mid", "pack_words", "pack_byte_values",
                  "zero_mid_edge")),
) + tuple(
    Case(f"m_tail_{r}", (1, r, 7, 7), "uniform", masks=("rand40", "ones"),
         reaches=("nb1", "scalar_s_mod4", "ssim_one_pixel", "group_idle", "group_partial", "cols_partial", "L_mid",
                  "pack_words", "pack_tail", "mask_ones", "zero_mid_edge"))
    for r in (1, 2, 3)
) + tuple(
    Case(f"m_mask_plus_{o}", (1, 1, 8, 16), "uniform", masks=("rand40", "box"), mask_offset=o,
         reaches=("nb1", "vec", "group_idle", "group_partial", "cols_partial", "L_mid", "pack_bytes", "zero_mid_edge"))
    for o in (1, 2, 3)
) + (
    Case("m_inside_positive", (1, 1, 9, 12), "inside_positive", masks=("box",),
         reaches=("nb1", "vec", "group_idle", "group_partial", "cols_partial", "L1", "pack_words", "zero_first_edge")),
    Case("m_inside_negative", (1, 1, 9, 12), "inside_negative", masks=("box",),
         reaches=("nb1", "vec", "group_idle", "group_partial", "cols_partial", "L1", "pack_words", "zero_last_edge",
                  "rm_negative")),
    Case("m_symmetric", (1, 1, 9, 12), "symmetric", masks=("box",),
         reaches=("nb1", "vec", "group_idle", "group_partial", "cols_partial", "L1", "pack_words", "zero_mid_edge",
                  "on_edge")),
    Case("m_mom_capped", (1, 1, 8, 262145), "ct", masks=("from_chunk_200",), ssim=False, mask_offset=1,
         reaches=("mom_capped", "hist_ne_mom", "vec", "chunk_ragged", "mom_chunk_empty", "mom_chunk_clamped",
                  "thread_loops", "ssim_off", "L1", "pack_bytes", "pack_grid_capped", "mask_empty_chunks", "zero_mid_edge")),
)
BY_NAME = {c.name: c for c in CASES}
GUARDED = ("mom_capped", "hist_capped", "m_mom_capped", "m_L8", "tiles_3x2")


# ---- data -----------------------------------------------------------------------------------------------------------
def f32_edges(lo, hi):
    """the 101 float32 bin edges numpy builds for float32 data spanning [lo, hi]"""
    e = np.histogram_bin_edges(np.array([lo, hi], np.float32), bins=BINS)
    assert e.dtype == np.float32 and e.shape == (BINS + 1,)
    return e


def edge_values(lo, hi):
    """every edge and its float32 neighbours, clipped to the range, plus lo and hi (305 values)"""
    lo, hi = np.float32(lo), np.float32(hi)
    e = f32_edges(lo, hi)
    v = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf)), [lo, hi]])
    return np.clip(v, lo, hi).astype(np.float32)


def make_mask(kind, case, rng):
    """a uint8 mask of the case's shape (non-zero = inside)"""
    shape, N, S = case.shape, case.N, case.S
    m = np.zeros((N, S), np.uint8)
    nb = moment_blocks(S)
    per = chunk_len(S, nb)
    last = (S - 1) // per * per                                     # start of the last non-empty chunk
    if kind == "ones":
        m[:] = 1
    elif kind == "rand40":
        m[:] = rng.random((N, S)) < 0.4
    elif kind == "rand5":
        m[:] = rng.random((N, S)) < 0.05
        m[:, S // 2] = 1
        m[0] = 0                                                    # one element in sample 0
        m[0, S // 3] = 1
    elif kind == "one":
        m[:, S // 2 + 1] = 255
    elif kind == "last_chunk":
        m[:, last:] = rng.random((N, S - last)) < 0.5
        m[:, S - 1] = 1
    elif kind == "box":
        b = np.zeros(shape, np.uint8)
        b[(slice(None), slice(None)) + tuple(slice(s // 4, max(s // 4 + 1, 3 * s // 4)) for s in shape[2:])] = 1
        m[:] = b.reshape(N, S)
    elif kind == "checker":
        m[:] = (np.arange(S) % 2 == 0) * 3
    elif kind == "empty0":
        m[1:, S // 5] = 1
    elif kind in ("bytes", "bytes_sparse"):
        pattern = np.concatenate([(np.arange(256) + s) % 256 for s in range(4)]).astype(np.uint8)
        if kind == "bytes_sparse":
            pattern = pattern * (np.arange(1024) % 3 == 0).astype(np.uint8)
        m[:] = np.resize(pattern, S)
    elif kind.startswith("from_chunk_"):
        b0 = int(kind.rsplit("_", 1)[1]) * per
        m[:, b0:] = rng.random((N, S - b0)) < 0.5
    else:
        raise KeyError(kind)
    return m.reshape(shape)


def data(case):
    """(t, p, masks): float32 arrays of the case's shape and its uint8 masks; the same for a case and its `alone` partner"""
    src = BY_NAME[case.alone[0]] if case.alone else case
    shape, N = case.shape, case.N
    rng = np.random.default_rng(sum(map(ord, src.name)))
    masks = [make_mask(k, src, np.random.default_rng(1000 + i)) for i, k in enumerate(src.masks)]
    if case.alone:
        masks = [masks[case.alone[1]]]
    kind = case.kind
    if kind == "uniform":
        t = rng.uniform(-1, 1, shape)
        p = np.clip(t + rng.normal(0, 0.2, shape), -1, 1)
    elif kind == "ct":
        t = rng.uniform(-1000, 3000, shape)
        t[..., : shape[-2] // 2, : shape[-1] // 2] = 40.0
        p = t + rng.normal(0, 60, shape)
    elif kind == "ranges":                          # every sample its own range and maximum
        scale = np.array([1.0, 2500.0, 0.01, 40.0])[np.arange(N) % 4].reshape((N,) + (1,) * (len(shape) - 1))
        shift = np.array([0.0, -700.0, 0.25, 3.0])[np.arange(N) % 4].reshape(scale.shape)
        t = rng.uniform(-1, 1, shape) * scale + shift
        p = t + rng.normal(0, 0.1, shape) * scale
    elif kind == "negative":
        t = -rng.uniform(0.5, 2, shape)
        p = t + rng.normal(0, 0.1, shape)
    elif kind == "identical":
        t = rng.uniform(-1000, 3000, shape)
        p = t
    elif kind in ("t_const", "p_const", "const_unequal", "const_equal", "t_zero", "all_zero"):
        t = rng.uniform(-1, 1, shape)
        p = rng.uniform(-1, 1, shape)
        if kind in ("t_const", "const_unequal", "const_equal"):
            t[:] = 0.25
        if kind in ("t_zero", "all_zero"):
            t[:] = 0.0
        if kind == "p_const":
            p[:] = -0.5
        if kind == "const_unequal":
            p[:] = 0.75
        if kind == "const_equal":
            p[:] = 0.25
        if kind == "all_zero":
            p[:] = 0.0
    elif kind == "edges":
        v = edge_values(*case.rng)
        assert v.size == int(np.prod(shape))
        t, p = rng.permutation(v).reshape(shape), rng.permutation(v).reshape(shape)
    elif kind in ("inside_positive", "inside_negative", "symmetric"):
        inside = masks[0] != 0
        t = rng.uniform(-2, 2, shape)
        p = rng.uniform(-2, 2, shape)
        if kind == "inside_positive":
            t[inside], p[inside] = rng.uniform(0.5, 2, inside.sum()), rng.uniform(0.25, 3, inside.sum())
        elif kind == "inside_negative":
            t[inside], p[inside] = -rng.uniform(0.5, 2, inside.sum()), -rng.uniform(0.25, 3, inside.sum())
        else:
            vals = rng.uniform(-1, 1, inside.sum())
            vals[:4] = (-1.0, 1.0, 0.0, np.nextafter(np.float32(0), np.float32(-1)))
            t[inside], p[inside] = vals, rng.permutation(vals)
    else:
        raise KeyError(kind)
    if masks and kind in ("uniform", "ranges", "ct"):
        # kappa does not cover a cancellation in 2 ux uy + C1 (window means of opposite sign against a small Rm): where a mask
        # holds one element of a sample, p has t's sign there
        tf, pf = t.reshape(N, -1), p.reshape(N, -1)
        for m in masks:
            mf = m.reshape(N, -1) != 0
            for n in np.flatnonzero(mf.sum(1) <= 1):
                pf[n, mf[n]] = tf[n, mf[n]] * 1.25
    return np.ascontiguousarray(t, np.float32), np.ascontiguousarray(p, np.float32), masks


def mirror(case, t=None, p=None, masks=None):
    """the set of BRANCHES names the case reaches, from the plan mirror and the case's data"""
    if t is None:
        t, p, masks = data(case)
    N, P, H, W, S, L = case.N, case.P, case.H, case.W, case.S, case.L
    q = plan(N, P, H, W)
    r = set()
    blocks = (S + 8191) // 8192
    r.add("nb1" if q["nb_mom"] == 1 else "mom_capped" if blocks > 256 else "nb_many")
    if q["nb_hist"] != q["nb_mom"]:
        r.add("hist_ne_mom")
    if blocks > 512:
        r.add("hist_capped")
    vec = vec_load(S, 4 * case.offset)
    if vec:
        r.add("vec")
    elif S % 4 == 0:
        r.add("scalar_misaligned")
    else:
        r.add("scalar_s_mod4")
        if N > 1:
            r.add("scalar_s_mod4_multi")
    for which, nb in (("mom", q["nb_mom"]), ("hist", q["nb_hist"])):
        per = chunk_len(S, nb)
        for b in range(nb):
            b0, b1, clamped = chunk(S, b, nb)
            n = b1 - b0
            if clamped:
                r.add(f"{which}_chunk_clamped")
            if n == 0:
                r.add(f"{which}_chunk_empty")
            elif n == 1:
                r.add("chunk_one")
            elif n < per and nb > 1:
                r.add("chunk_ragged")
            if n > (4 * THREADS if vec else THREADS):
                r.add("thread_loops")
    if not case.ssim:
        r.add("ssim_off")
    else:
        Ho, Wo = H - 6, W - 6
        f = ssim_tiles(H, W)
        r |= f & {"group_idle", "group_partial", "cols_partial"}
        if Ho == 1 and Wo == 1:
            r.add("ssim_one_pixel")
        if Ho % TH == 8:
            r.add("rows_8")
        if Ho % TH == 9:
            r.add("rows_9")
        if Ho % TH == 0 and Wo % TW == 0:
            r.add("tile_exact")
        if Ho % TH == 1 and Wo % TW == 1 and Ho > TH and Wo > TW:
            r.add("tile_plus_one")
        if q["tiles_w"] != q["tiles_h"] and P >= 2 and N >= 2:
            r.add("tiles_decode")
        if P * q["tiles_w"] * q["tiles_h"] > 256:
            r.add("ssim_partials_gt_256")
    tf, pf = t.reshape(N, S), p.reshape(N, S)
    if N > 1 and len({(float(a.min()), float(a.max())) for a in tf}) == N and float(tf.max(1).max()) > 4 * float(tf.max(1).min()):
        r.add("ranges_differ")
    if not L and (tf.max(1) <= 0).any():
        r.add("r_nonpositive")
    if (tf.view(np.int32) == pf.view(np.int32)).all():
        r.add("identical")
    tc, pc = (tf.min(1) == tf.max(1)).all(), (pf.min(1) == pf.max(1)).all()
    if tc:
        r.add("t_const")
    if pc:
        r.add("p_const")
    if tc and pc:
        r.add("both_const_equal" if (tf == pf).all() else "both_const_unequal")
    if not tf.any():
        r.add("t_zero")
        if not pf.any():
            r.add("all_zero")

    def edge_facts(x):
        e = f32_edges(x.min(), x.max())[1:-1]
        if np.isin(x, e).any():
            r.add("on_edge")
        if np.isin(x, np.nextafter(e, np.float32(-np.inf))).any() and np.isin(x, np.nextafter(e, np.float32(np.inf))).any():
            r.add("next_to_edge")

    if not L:
        if case.kind == "edges":
            edge_facts(tf[0])
        return r
    r.add("L1" if L == 1 else "L8" if L == MAX_LABELS else "L_mid")
    words = word_pack([case.mask_offset] * L)
    nwords, pblocks = pack_grid(N, S, words)
    if nwords:
        r.add("pack_words")
        if N * S % 4:
            r.add("pack_tail")
    else:
        r.add("pack_bytes")
    if pblocks == 2048 and (nwords or N * S) > 2048 * THREADS:
        r.add("pack_grid_capped")
    nb = q["nb_mom"]
    per = chunk_len(S, nb)
    for m in masks:
        mf = m.reshape(N, S)
        inside = mf != 0
        if len(np.unique(mf)) == 256 and all(len(np.unique(mf.reshape(-1)[k::4])) == 256 for k in range(4)):
            r.add("pack_byte_values")
        if inside.all():
            r.add("mask_ones")
        cnt = inside.sum(1)
        if (cnt == 0).any() and (cnt > 0).any():
            r.add("mask_empty_sample")
        if (cnt == 1).any():
            r.add("mask_one_element")
        for n in range(N):
            if cnt[n] == 0:
                continue
            live = [inside[n, b * per:(b + 1) * per].any() for b in range(-(-S // per))]
            if len(live) > 1 and not all(live):
                r.add("mask_empty_chunks")
                if live.index(True) == len(live) - 1:
                    r.add("mask_last_chunk_only")
            if cnt[n] == S:
                continue
            tm = tf[n] * inside[n]
            lo, hi = float(tm.min()), float(tm.max())
            r.add("zero_first_edge" if lo == 0 else "zero_last_edge" if hi == 0 else "zero_mid_edge")
            if tf[n][inside[n]].max() < 0:
                r.add("rm_negative")
            if case.kind == "symmetric":
                edge_facts(tm)
                r.discard("next_to_edge")
    return r


# ---- extended-precision reference ---------------------------------------------------------------------------------
def terms_are_exact(t, p):
    """the float64 terms handed to fsum equal the longdouble products (64-bit significand) bit for bit"""
    if not LD_OK:
        return True
    a, b = t.reshape(-1).astype(np.float64), p.reshape(-1).astype(np.float64)
    al, bl = a.astype(LD), b.astype(LD)
    return bool(((a * a).astype(LD) == al * al).all() and ((a * b).astype(LD) == al * bl).all()
                and ((b * b).astype(LD) == bl * bl).all())


def _fsum(*terms):
    parts = []
    n = terms[0].size
    for i in range(0, n, 1 << 20):
        parts.append(math.fsum(np.concatenate([x[i:i + (1 << 20)] for x in terms]).tolist()))
    return math.fsum(parts)


def exact_sums(t, p):
    """(sum |t-p|, sum (t-p)^2, sum t^2) of float32 vectors, each a correctly rounded float64 (see the module docstring)"""
    a, b = t.astype(np.float64), p.astype(np.float64)
    s = np.where(a >= b, 1.0, -1.0)
    if a.size == 0:
        return 0.0, 0.0, 0.0
    return _fsum(s * a, -s * b), _fsum(a * a, -2.0 * a * b, b * b), _fsum(a * a)


def _ssim_fraction(t, p, R):
    """exact rational 7 x 7 SSIM for platforms whose longdouble is a double (small shapes only)"""
    P, H, W = t.shape
    assert P * H * W <= 4096, "no extended precision on this platform: the Fraction fallback covers small shapes only"
    F = Fraction
    C1, C2 = (F(0.01) * F(R)) ** 2, (F(0.03) * F(R)) ** 2
    tot, kap, bad = F(0), F(0), False
    for k in range(P):
        x = [[F(float(v)) for v in row] for row in t[k]]
        y = [[F(float(v)) for v in row] for row in p[k]]
        for i in range(H - 6):
            for j in range(W - 6):
                wx = [x[i + a][j + b] for a in range(7) for b in range(7)]
                wy = [y[i + a][j + b] for a in range(7) for b in range(7)]
                ux, uy = sum(wx) / 49, sum(wy) / 49
                uxx, uyy, uxy = sum(v * v for v in wx) / 49, sum(v * v for v in wy) / 49, sum(a * b for a, b in zip(wx, wy)) / 49
                c = F(49, 48)
                vx, vy, vxy = c * (uxx - ux * ux), c * (uyy - uy * uy), c * (uxy - ux * uy)
                den = (ux * ux + uy * uy + C1) * (vx + vy + C2)
                if den == 0 or 2 * vxy + C2 == 0:
                    bad = True
                    continue
                s = (2 * ux * uy + C1) * (2 * vxy + C2) / den
                tot += s
                kap += abs(s) * ((uxx + uyy) / (vx + vy + C2) + (abs(uxy) + abs(ux * uy)) / abs(2 * vxy + C2) + 1)
    n = P * (H - 6) * (W - 6)
    return (float("nan"), float("nan")) if bad else (float(tot / n), float(kap / n))


def ssim_direct(t, p, R):
    """(ssim, kappa) of planes t, p [P, H, W] with data range R: the direct window statement in longdouble"""
    if not LD_OK:
        return _ssim_fraction(t, p, R)
    from numpy.lib.stride_tricks import sliding_window_view
    x, y = t.astype(LD), p.astype(LD)

    def box(a):
        return sliding_window_view(a, (7, 7), axis=(-2, -1)).sum(axis=(-2, -1)) / LD(49)

    with np.errstate(all="ignore"):
        ux, uy, uxx, uyy, uxy = box(x), box(y), box(x * x), box(y * y), box(x * y)
        cov = LD(49) / LD(48)
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        C1, C2 = (LD(0.01) * LD(R)) ** 2, (LD(0.03) * LD(R)) ** 2
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        kappa = np.abs(S) * ((uxx + uyy) / (vx + vy + C2) + (np.abs(uxy) + np.abs(ux * uy)) / np.abs(2 * vxy + C2) + 1)
        return S.mean(dtype=LD), kappa.mean(dtype=LD)


def hist_scores(ht, hp, hj, S, et, ep, dtype=LD):
    """(nmi, chi2, terms of nmi, terms of chi2) from integer counts and numpy's float32 edges"""
    with np.errstate(all="ignore"):
        g, q = ht.astype(dtype) / dtype(S), hp.astype(dtype) / dtype(S)
        keep = (g + q) != 0
        chi2 = (((q - g) ** 2)[keep] / (q + g)[keep]).sum(dtype=dtype)
        wt, wp = np.diff(et).astype(dtype), np.diff(ep).astype(dtype)
        d = hj.astype(dtype) / wt[:, None] / wp[None, :] / dtype(S)

        def entropy(x):
            x = x.reshape(-1) / x.sum(dtype=dtype)
            x = x[x > 0]
            return -(x * np.log(x)).sum(dtype=dtype)

        rows, cols = d.sum(axis=1, dtype=dtype), d.sum(axis=0, dtype=dtype)
        nmi = (entropy(cols) + entropy(rows)) / entropy(d)
    return nmi, chi2, int((hj > 0).sum() + (rows > 0).sum() + (cols > 0).sum()), int(keep.sum())


def reference_row(case, t, p, m):
    """one (sample, label): t, p float32 [P, H, W]; m bool of that shape or None. A dict of the columns in longdouble
    (or float), kappa, the term counts and the bin counts."""
    S = t.size
    if m is None:
        ti, pi, tm, pm = t.reshape(-1), p.reshape(-1), t, p
        counts = ref.bin_counts(t, p)
    else:
        ti, pi = t[m], p[m]
        tm, pm = mref.products(t, p, m)
        counts = mref.bin_counts(t, p, m)
    out = dict(counts=counts)
    n = ti.size
    if n == 0:
        out.update({k: float("nan") for k in COLUMNS}, kappa=0.0, n_nmi=0, n_chi2=0)
        return out
    sad, ssd, stt = exact_sums(ti, pi)
    R = float(ti.max())
    with np.errstate(all="ignore"):
        out["mae"], out["mse"] = LD(sad) / LD(n), LD(ssd) / LD(n)
        out["nmse"] = LD(ssd) / LD(stt)
        out["psnr"] = LD(10) * np.log10(LD(R) * LD(R) / (LD(ssd) / LD(S)))
    out["ssim"], out["kappa"] = ssim_direct(tm.reshape(case.P, case.H, case.W), pm.reshape(case.P, case.H, case.W), R) \
        if case.ssim else (float("nan"), 0.0)
    et, ep = f32_edges(tm.min(), tm.max()), f32_edges(pm.min(), pm.max())
    out["nmi"], out["histogram_chi2"], out["n_nmi"], out["n_chi2"] = hist_scores(*counts, S, et, ep)
    return out


def reference(case, t, p, masks):
    """rows[n][l] (l = 0 only for the unmasked call)"""
    N = case.N
    sample = lambda a, n: a[n].reshape(case.P, case.H, case.W)
    if not masks:
        return [[reference_row(case, sample(t, n), sample(p, n), None)] for n in range(N)]
    return [[reference_row(case, sample(t, n), sample(p, n), sample(m, n) != 0) for m in masks] for n in range(N)]


@functools.lru_cache(maxsize=None)
def built(name):
    """(case, t, p, masks, reference rows) of a case, computed once and shared (treat as read-only)"""
    case = BY_NAME[name]
    t, p, masks = data(case)
    for a in (t, p, *masks):
        a.setflags(write=False)
    return case, t, p, masks, reference(case, t, p, masks)


# ---- the float64 statement in the kernels' summation order -----------------------------------------------------------
def _tree256(v):
    """vm_block_sum: sh[i] += sh[i + o] for o = 128 .. 1"""
    o = THREADS // 2
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o //= 2
    return v[..., 0]


def _waves256(v):
    """vmm_block_reduce as a sum: xor butterflies inside each wave of 64, then the four waves in index order"""
    v = v.reshape(v.shape[:-1] + (4, 64))
    o = 32
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o //= 2
    v = v[..., 0]
    return ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]


def _pad(v, n):
    out = np.zeros(v.shape[:-1] + (n,), v.dtype)
    out[..., :v.shape[-1]] = v
    return out


def _chunk_sums(x, nb, vec, reduce, mutant):
    """the slab column of one sum: x = the S non-negative float64 terms of a sample (0 where masked out)"""
    S = x.size
    per = chunk_len(S, nb)
    a = _pad(x, nb * per).reshape(nb, per)
    if mutant == "tail_skipped":                        # the elements after the last whole group of four of every chunk
        a = a.copy()
        for b in range(nb):
            b0, b1, _ = chunk(S, b, nb)
            a[b, (b1 - b0) // 4 * 4:] = 0.0
    acc = np.zeros((nb, THREADS))
    if vec:
        a = a.reshape(nb, per // (4 * THREADS), THREADS, 4)
        for i in range(a.shape[1]):
            for k in range(4):
                acc = acc + a[:, i, :, k]
    else:
        a = a.reshape(nb, per // THREADS, THREADS)
        for i in range(a.shape[1]):
            acc = acc + a[:, i]
    return reduce(acc)


def _slab_sum(col, reduce):
    nb = col.size
    rounds = -(-nb // THREADS)
    a = _pad(col, rounds * THREADS).reshape(rounds, THREADS)
    acc = np.zeros(THREADS)
    for i in range(rounds):
        acc = acc + a[i]
    return float(reduce(acc))


def vm_edges(lo, hi):
    """vm_outer_edges and vm_edge in float32: (edges [101], first, last)"""
    lo, hi = np.float32(lo), np.float32(hi)
    first, last = (lo - np.float32(0.5), hi + np.float32(0.5)) if lo == hi else (lo, hi)
    delta = np.float32(last - first)
    step = np.float32(delta / np.float32(BINS))
    k = np.arange(BINS + 1, dtype=np.float32)
    y = (k / np.float32(BINS)).astype(np.float32) * delta if step == 0 else k * step
    e = (y.astype(np.float32) + first).astype(np.float32)
    e[BINS] = last
    return e, first, last


def vm_bin(x, e, first, last, mutant=None):
    """vm_bin: the clamped first guess, then the walk down and up"""
    with np.errstate(all="ignore"):
        scale = np.float32(np.float32(BINS) / np.float32(last - first))
        g = (x - first).astype(np.float32) * scale
    i = np.minimum(np.maximum(g, np.float32(0)), np.float32(BINS - 1)).astype(np.int64)
    lower = mutant == "edge_lower"
    while True:
        down = (i > 0) & ((x <= e[i]) if lower else (x < e[i]))
        if not down.any():
            break
        i = i - down
    while True:
        nxt = e[np.minimum(i + 1, BINS)]
        up = (i < BINS - 1) & ((x > nxt) if lower else (x >= nxt))
        if not up.any():
            break
        i = i + up
    return i


def _hist_scores64(c, S, rg):
    """vm_hist_scores: (nmi, chi2) from the count words in the kernel's order, float64"""
    ht, hp, hj = c[:BINS].astype(np.float64), c[BINS:2 * BINS].astype(np.float64), c[2 * BINS:].astype(np.float64)
    with np.errstate(all="ignore"):
        g, q = ht / float(S), hp / float(S)
        chi = np.where(g + q != 0.0, (q - g) * (q - g) / (q + g), 0.0)
        chi2 = _tree256(_pad(chi, THREADS))
        et, _, _ = vm_edges(rg[0], rg[1])
        ep, _, _ = vm_edges(rg[2], rg[3])
        wt, wp = np.diff(et).astype(np.float64), np.diff(ep).astype(np.float64)
        d = ((hj.reshape(BINS, BINS) / wt[:, None]) / wp[None, :]) / float(S)
        rows, cols = np.zeros(BINS), np.zeros(BINS)
        for k in range(BINS):
            rows = rows + d[:, k]
            cols = cols + d[k, :]

        def strided(v):
            a = _pad(v.reshape(-1), 40 * THREADS).reshape(40, THREADS)
            acc = np.zeros(THREADS)
            for k in range(40):
                acc = acc + a[k]
            return acc

        entr = lambda x: np.where(x > 0.0, -x * np.log(np.where(x > 0.0, x, 1.0)), 0.0)
        Tr, Tc, Tj = _tree256(_pad(rows, THREADS)), _tree256(_pad(cols, THREADS)), _tree256(strided(d))
        H1, H0 = _tree256(_pad(entr(rows / Tr), THREADS)), _tree256(_pad(entr(cols / Tc), THREADS))
        H01 = _tree256(strided(entr(d / Tj)))
        return float((H0 + H1) / H01), float(chi2)


def _ssim_pixel(ux, uy, uxx, uyy, uxy, C1, C2, cov):
    pxx, pyy, pxy = ux * ux, uy * uy, ux * uy
    vx, vy, vxy = cov * (uxx - pxx), cov * (uyy - pyy), cov * (uxy - pxy)
    return ((2.0 * pxy + C1) * (2.0 * vxy + C2)) / (((pxx + pyy) + C1) * ((vx + vy) + C2))


def _ssim64(t, p, R, mutant):
    """the partials of vm_ssim_kernel for planes t, p [P, H, W] (float32), in [plane][tile row][tile col] order"""
    P, H, W = t.shape
    Ho, Wo = H - 6, W - 6
    tiles_h, tiles_w = -(-Ho // TH), -(-Wo // TW)
    a, b = t.astype(np.float64), p.astype(np.float64)
    rows = tiles_h * TH + 6
    h = np.zeros((5, P, rows, tiles_w * TW))
    for k in range(7):                                  # vm_row7: seven taps left to right
        for q, x in enumerate((a, b, a * a, b * b, a * b)):
            h[q, :, :H, :Wo] += x[:, :, k:k + Wo]
    R = float(R)
    C1, C2 = (0.01 * R) * (0.01 * R), (0.03 * R) * (0.03 * R)
    inv, cov = 1.0 / 49.0, 49.0 / 48.0
    acc = np.zeros((P, tiles_h * (TH // GROUP), tiles_w * TW))       # [plane][row group][column]
    with np.errstate(all="ignore"):
        for G in range(acc.shape[1]):
            Y = G * GROUP
            if Y >= Ho:
                continue
            v = np.zeros((5, P, tiles_w * TW))
            for r in range(GROUP + 6):
                v = v + h[:, :, Y + r]
                if r >= 7:
                    v = v - h[:, :, Y + r - 7]
                y = Y + r - 6
                if r >= 6 and y < Ho and not (mutant == "last_row_dropped" and (y % TH == TH - 1 or y == Ho - 1)):
                    u = v * inv
                    acc[:, G] = acc[:, G] + _ssim_pixel(u[0], u[1], u[2], u[3], u[4], C1, C2, cov)
    acc[:, :, Wo:] = 0.0
    tiles = acc.reshape(P, tiles_h, TH // GROUP, tiles_w, TW).transpose(0, 1, 3, 2, 4).reshape(P, tiles_h, tiles_w, THREADS)
    return _tree256(tiles).reshape(-1)


def statement(case, t, p, masks, mutant=None):
    """(table [N, 7] or [N, L, 7] float64, counts [N, (L,) 10200] int64): what the kernels compute, restated in float64
    numpy in their summation order. `mutant` names one deliberate mistake (MUTANTS)."""
    N, P, H, W, S = case.N, case.P, case.H, case.W, case.S
    masked = bool(masks)
    L = max(case.L, 1)
    q = plan(N, P, H, W)
    vec = vec_load(S, 4 * case.offset)
    reduce = _waves256 if masked else _tree256
    table = np.full((N, L, 7), np.nan)
    counts = np.zeros((N, L, HIST_WORDS), np.int64)
    tf, pf = t.reshape(N, S), p.reshape(N, S)
    a, b = tf.astype(np.float64), pf.astype(np.float64)
    d = a - b
    for n in range(N):
        for l in range(L):
            if masked:
                bit = l - 1 if mutant == "label_shifted" else l
                inside = (masks[bit].reshape(N, S)[n] != 0) if bit >= 0 else np.zeros(S, bool)
            else:
                inside = np.ones(S, bool)
            w = inside.astype(np.float64)
            sad, ssd, stt = (_slab_sum(_chunk_sums(x * w, q["nb_mom"], vec, reduce, mutant), reduce)
                             for x in (np.abs(d[n]), d[n] * d[n], a[n] * a[n]))
            cnt = int(inside.sum())
            tm, pm = np.where(inside, tf[n], np.float32(0)), np.where(inside, pf[n], np.float32(0))
            R = -np.inf if not cnt else float(tf.max()) if mutant == "batch_range" else float(tf[n][inside].max())
            if masked and mutant == "range_inside_only" and cnt:
                rg = (tf[n][inside].min(), tf[n][inside].max(), pf[n][inside].min(), pf[n][inside].max())
            else:
                rg = (tm.min(), tm.max(), pm.min(), pm.max())
            et, ft, lt = vm_edges(rg[0], rg[1])
            ep, fp, lp = vm_edges(rg[2], rg[3])
            keep = np.ones(S, bool)
            if mutant == "tail_skipped":
                for k in range(q["nb_hist"]):
                    b0, b1, _ = chunk(S, k, q["nb_hist"])
                    keep[b0 + (b1 - b0) // 4 * 4:b1] = False
            i, j = vm_bin(tm[keep], et, ft, lt, mutant), vm_bin(pm[keep], ep, fp, lp, mutant)
            counts[n, l, :BINS] = np.bincount(i, minlength=BINS)
            counts[n, l, BINS:2 * BINS] = np.bincount(j, minlength=BINS)
            counts[n, l, 2 * BINS:] = np.bincount(i * BINS + j, minlength=BINS * BINS)
            if cnt == 0:
                continue
            with np.errstate(all="ignore"):
                den = float(cnt) if masked else float(S)
                row = table[n, l]
                row[0], row[1], row[2] = sad / den, ssd / den, np.float64(ssd) / np.float64(stt)
                row[3] = 10.0 * np.log10(np.float64(R * R) / np.float64(ssd / float(S)))
                if case.ssim:
                    part = _ssim64(tm.reshape(P, H, W), pm.reshape(P, H, W), R, mutant)
                    row[4] = _slab_sum(part, _tree256) / (float(P) * float(H - 6) * float(W - 6))
                row[5], row[6] = _hist_scores64(counts[n, l], S, rg)
    return (table if masked else table[:, 0]), (counts if masked else counts[:, 0])


MUTANTS = {            # mistake -> the case that must reject it
    "last_row_dropped": "tile_plus_one",
    "batch_range": "tiles_3x2",
    "tail_skipped": "one_element_chunk",
    "edge_lower": "edges_0",
    "range_inside_only": "m_inside_positive",
    "label_shifted": "m_L8_n3_s99",
}


# ---- judge ----------------------------------------------------------------------------------------------------------
def depth_of(case):
    return sum_depth(case.S, moment_blocks(case.S), vec_load(case.S, 4 * case.offset), bool(case.masks))


def _same_special(got, want):
    """NaN and +-inf where the reference has them, with its sign"""
    got, want = float(got), float(want)
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    if math.isinf(want) or math.isinf(got):
        return got == want
    return True


def judge_row(case, got_row, got_counts, want):
    """one table row and its count words against reference_row's dict: {column: excess} (error / bound at K = 1; psnr in
    ulps beyond its analytic part), 'counts' and 'special' (booleans)"""
    depth = depth_of(case)
    ht, hp, hj = want["counts"]
    m = dict(counts=bool((got_counts[:BINS] == ht).all() and (got_counts[BINS:2 * BINS] == hp).all()
                         and (got_counts[2 * BINS:].reshape(BINS, BINS) == hj).all()),
             special=True)
    for c, k in enumerate(COLUMNS):
        got, w = got_row[c], want[k]
        if k == "ssim" and not case.ssim:
            m["special"] &= math.isnan(float(got))
            m[k] = 0.0
            continue
        if not _same_special(got, w):
            m["special"] = False
        if not (math.isfinite(float(w)) and math.isfinite(float(got))):
            m[k] = 0.0
            continue
        err = float(abs(LD(got) - LD(w)))
        if k in ("mae", "mse", "nmse"):
            bound = (2 if k == "nmse" else 1) * depth * U * float(abs(w))
        elif k == "psnr":
            analytic = (depth + 2) * U * 10.0 / math.log(10.0)
            m[k] = max(err - analytic, 0.0) / float(np.spacing(np.float64(abs(float(w)))))
            continue
        elif k == "ssim":
            bound = U * float(want["kappa"])
        else:
            bound = U * want["n_nmi" if k == "nmi" else "n_chi2"] * float(abs(w))
        m[k] = 0.0 if err == 0.0 else err / bound if bound > 0 else math.inf
    return m


def hist_k(want, k_hist):
    """the K of the histogram columns of one row: K_HIST, lowered where K_HIST * 2^-53 * terms would pass HIST_REL_CAP"""
    return {k: min(k_hist, HIST_REL_CAP / (U * max(want[n], 1))) for k, n in (("nmi", "n_nmi"), ("histogram_chi2", "n_chi2"))}


def accept(m, want, k_ssim, k_hist, psnr_ulps):
    hk = hist_k(want, k_hist)
    return (m["counts"] and m["special"] and max(m["mae"], m["mse"], m["nmse"]) <= 1.0 and m["psnr"] <= psnr_ulps
            and m["ssim"] <= k_ssim and m["nmi"] <= hk["nmi"] and m["histogram_chi2"] <= hk["histogram_chi2"])


def judge(case, table, counts, rows):
    """every (sample, label) of a call: a list of ((n, l), judge_row dict, reference row)"""
    N, L = case.N, max(case.L, 1)
    table = np.asarray(table).reshape(N, L, 7)
    counts = np.asarray(counts).reshape(N, L, HIST_WORDS)
    return [((n, l), judge_row(case, table[n, l], counts[n, l], rows[n][l]), rows[n][l]) for n in range(N) for l in range(L)]


def worst(judged):
    """{column: largest excess} over the rows of a call"""
    return {k: max(m[k] for _, m, _ in judged) for k in COLUMNS}


# ---- device runs ----------------------------------------------------------------------------------------------------
def to_device(case, t, p, masks, device):
    """the case's tensors on the device, t and p `offset` floats and the masks `mask_offset` bytes past an aligned base"""
    import torch

    def place(a, off, dtype):
        flat = torch.zeros(a.size + off + 16, dtype=dtype, device=device)
        flat[off:off + a.size] = torch.from_numpy(np.array(a)).reshape(-1).to(device)
        v = flat[off:off + a.size].view(a.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == (off * v.element_size()) % 16
        return v

    return (place(t, case.offset, torch.float32), place(p, case.offset, torch.float32),
            [place(m, case.mask_offset, torch.uint8) for m in masks])


def run(ops, case, td, pd, md):
    """(table, count words) through the wrapper, as numpy"""
    import torch
    if case.masks:
        table, (ht, hp, hj) = ops.valmetrics_masked(td, pd, md, ssim=case.ssim, return_counts=True)
    else:
        table, (ht, hp, hj) = ops.valmetrics(td, pd, ssim=case.ssim, return_counts=True)
    words = torch.cat([ht, hp, hj.flatten(-2)], dim=-1)
    return table.cpu().numpy(), words.cpu().numpy()


def run_guarded(ops, case, td, pd, md):
    """the library calls as HipOps makes them, on a table (with one extra row), counts and scratch filled with 0xFF bytes:
    (table rows, count words, extra row as int64, the library's scratch size)"""
    import ctypes as C

    import torch
    from ganslate_amd.hip import lib as L
    from ganslate_amd.hip.ops import _ptr, _stream
    N, P, H, W, nl = case.N, case.P, case.H, case.W, max(case.L, 1)
    dev = td.device
    ff = lambda n: torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)
    rows = N * nl
    table, counts = ff((rows + 1) * 7 * 8), ff(rows * HIST_WORDS * 4)
    flags = (L.VM_FLAGS["ssim"] if case.ssim else 0) | L.VM_FLAGS["hist"]
    if case.masks:
        nbytes = ops.lib.gs_valmetric_masked_scratch_bytes(N, nl, P, H, W)
        scratch = ff(nbytes)
        ptrs = (C.c_void_p * nl)(*[m.data_ptr() for m in md])
        L.check(ops.lib.gs_valmetrics_masked(_ptr(td), _ptr(pd), ptrs, nl, N, P, H, W, flags, _ptr(table), _ptr(counts),
                                             _ptr(scratch), _stream()), "gs_valmetrics_masked")
    else:
        nbytes = ops.lib.gs_valmetric_scratch_bytes(N, P, H, W)
        scratch = ff(nbytes)
        L.check(ops.lib.gs_valmetrics(_ptr(td), _ptr(pd), N, P, H, W, flags, _ptr(table), _ptr(counts), _ptr(scratch),
                                      _stream()), "gs_valmetrics")
    tab = table.view(torch.float64).view(rows + 1, 7).cpu()
    return (tab[:rows].numpy(), counts.view(torch.int32).view(rows, HIST_WORDS).long().cpu().numpy(),
            tab[rows].view(torch.int64).numpy(), nbytes)
