"""csrc/wfold.hip, the to/from-activation and fold-adjoint entry points of csrc/image.hip and csrc/taps.hip against the
float64 statement of tests/boundary_ref.py on every branch of their launch plans (each row's `reaches` names its branches;
tests/test_boundary_edges_cpu.py proves the rows are on them): one, two and three row segments with a full, a ragged and a
one-pixel last segment, the halo across a segment boundary, one to four MAXJ passes of the unfold backward and its three
fall-backs, the fall-backs of the shift-add pair, the LDS guard of gs_image_unfold, the strided pass of img_grid, every tap
block size, both loops of tap_rows_sum_kernel, and the image taps with constructed collisions up to the 64 KiB LDS table.

Every element of every output is judged by its kind (boundary_ref's docstring): bits for moves and single roundings, the
fp32 sum bound K2 (and exact equality on integer data), the bf16 bound K for the tanh backward, fp32 ulps against float64
tanh of the kernel's own pre-activation for the tanh forward. Outputs are guarded views, NaN or pre-filled.

Every wfold case runs with the default options and under wfold_rows = 0; the three forward-style transforms must agree bit for
bit between the row and the per-pixel form, the unfold backward on every output row with one source row.

K = 4 and K2 = 32 are the project's (tests/test_pnorm_edges_gpu.py), not fitted here; RefOps meets them on the CPU (0.14 / 1.75
at worst, torch's tanh 0.56 ulp). Largest excess measured on an MI355X over all cases, the row and the per-pixel form alike:
  g_img (gs_image_unfold_backward)      0.983  c4q32_w257_replicate0_d1_acc     img (gs_shiftadd_to_image)  1.222  co17p120_w250
  g_img (gs_image_to_act_backward)      0.999  replicate3_2d_acc                db (gs_tap_rows_sum)        2.361  r31_c130
  g_act / gz (the tanh backwards)       0.000  (no element beyond its own bf16 rounding)
  tanh, fp32 ulps against float64 tanh of the kernel's own pre-activation:
    gs_shiftadd_to_image                1.313  co17p120_w520_nobias             gs_act_to_image             0.929  c1p8_hw255
  -> TANH_ULPS = 3 (twice 1.313, rounded up to a whole ulp; the cap is 8)
Every bits output is bit-exact, every integer-data sum exact, the row forms equal the per-pixel forms bit for bit (the unfold
backward on the rows with one source row), the P = 16384 launch of gs_image_tap_scatter (64 KiB of LDS) is accepted.
The slowest case (unfold_bwd c1q8_w4_reflect0_d2, the first to switch wfold_rows) takes 0.77 s, from_act c9p16_hw513x512 0.56 s,
its float64 reference on the CPU included; the whole file 5 s.
"""
import time

import pytest
import torch

from tests import boundary_ref as R
from tests.test_pnorm_edges_gpu import K, K2

pytestmark = pytest.mark.gpu

TANH_ULPS_MEASURED = dict(shiftadd=1.313, act_to_image=0.929)
TANH_ULPS = 3                      # twice the measured error, rounded up to a whole ulp
K_MEASURED = dict(act_to_image_backward=0.0, shiftadd_backward=0.0)
K2_MEASURED = dict(unfold_backward=0.983, shiftadd=1.222, to_act_backward=0.999, rows_sum=2.361)
assert 2 * max(TANH_ULPS_MEASURED.values()) <= TANH_ULPS <= R.TANH_CAP
assert max(K_MEASURED.values()) <= K and max(K2_MEASURED.values()) <= K2

RUN_IDS = [f"{op}-{n}-{d}" for op, n, d in R.RUNS]


def show(what, m, **more):
    print(f"BOUNDARY_EXCESS {what} k={m['k']:.3f} k2={m['k2']:.3f} tanh_ulps={m['tanh']:.3f} bits={int(m['bits'])} "
          f"guards={int(m['guards'])} " + " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in more.items()))


@pytest.mark.parametrize("op,name,data", R.RUNS, ids=RUN_IDS)
def test_boundary_case(hip_ops, op, name, data):
    t0 = time.perf_counter()
    b = R.build(op, name, data)
    c = b.case
    got = R.run(hip_ops, b, hip_ops.device)
    m = R.judge(b, got)
    if op not in R.WFOLD_OPS:
        show(f"{op} {name} {data}", m, seconds=time.perf_counter() - t0)
        assert R.accept(m, K, K2, TANH_ULPS), (c.reaches, m)
        return
    with hip_ops.options(wfold_rows=0):
        got0 = R.run(hip_ops, b, hip_ops.device)
    m0 = R.judge(b, got0)
    show(f"{op} {name} {data} rows", m, seconds=time.perf_counter() - t0)
    show(f"{op} {name} {data} pixel", m0)
    assert R.accept(m, K, K2, TANH_ULPS), ("row form", c.reaches, m)
    assert R.accept(m0, K, K2, TANH_ULPS), ("per-pixel form", c.reaches, m0)
    if op == "unfold_bwd":
        one = R.single_source_rows(c).view(-1)                             # [D * H]
        rows = lambda t: t.reshape(R.N, c.C, c.D * c.H, c.W)[:, :, one]
        assert R.same_bits(rows(got["g_img"]), rows(got0["g_img"])), "row form != per-pixel form on rows with one source row"
    else:
        for key in b.ref:
            assert R.same_bits(got[key], got0[key]), f"{key}: row form != per-pixel form"


def test_refusals(hip_ops):
    """each raises the library's error (rc = 2: a refused argument, before any launch), or the wrapper's ValueError where
    the wrapper looks at the condition before the library does"""
    from ganslate_amd.hip.lib import HipError
    for what, call, who in R.refusals(hip_ops, hip_ops.device):
        with pytest.raises(HipError, match=r"rc=2") if who == "library" else pytest.raises(ValueError, match="do not fit"):
            call()
        print(f"BOUNDARY_REFUSED {what}")
    torch.cuda.synchronize()
