"""csrc/attn.hip stage by stage against the float64 reference of tests/attn_ref.py: every case of its table runs forward on a
scratch tensor filled with a NaN pattern, reads the scratch, runs backward into pre-filled gradients and reads it again; each
of the 14 stages is then checked per element against float64 applied to the bits the kernel stored as that stage's input
(tests/attn_ref.py states the criterion), and everything outside what the stages document as written must keep its pre-fill.

K and K2 are four times the largest excess measured on an MI355X over all cases, rounded up to a power of two; the caps are
2^8 (attn_ref.K_CAP, K2_CAP).
  bf16 outputs: largest excess 0.399 (stage 10 dS, case n65_c64; stage 2 v 0.127, stage 8 dv 0.066, stage 5 O 0.021,
                stage 11 dq / dk 0.007, stage 13 dx 0.002, stages 4 P, 6 out and 7 dO 0.0)                        -> K  = 2
  fp32 outputs: largest excess 2.384 (stage 14 dW / db, case n130_c72; stage 1 q / k 1.986, stage 3 S 1.871,
                stage 9 dP 1.693, stage 7 dgamma 0.070)                                                           -> K2 = 16
An excess of 0.0 means that every element is within its own bf16 rounding of float64; stage 7 is listed once per output
type. The fp32 emulation on the CPU (tests/test_attn_stages_cpu.py) measures up to 3.31 (stage 14) on the same inputs.
"""
import ctypes

import pytest
import torch

from tests import attn_ref as R

pytestmark = pytest.mark.gpu

K_MEASURED, K2_MEASURED = 0.399, 2.384
K, K2 = 2, 16
assert K <= R.K_CAP and K2 <= R.K2_CAP
assert 4 * K_MEASURED <= K < 8 * K_MEASURED and 4 * K2_MEASURED <= K2 < 8 * K2_MEASURED      # the next power of two


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_attn_stages(hip_ops, name):
    """one row of attn_ref.CASES (its `reaches` names the branch)"""
    inp = R.build(name)
    c, p = inp.case, inp.plan
    st, out_inf, lost, fwd_kept = R.run_gpu(hip_ops, inp, hip_ops.device)
    res, bad = R.measure(inp, st)
    for k, v in res.items():
        print(f"ATTN_EXCESS {name} stage {k}: {v:.3f}")
    assert not bad, bad
    assert lost == (0, 0), f"{name}: bytes changed outside the documented buffers after forward / backward: {lost}"
    assert fwd_kept, "backward changed q, k, v, O or P"
    for k, v in res.items():
        assert v <= (K if R.is_bf16_stage(k) else K2), f"{name} ({c.reaches}): stage {k}: excess {v:.1f}"
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(out_inf), bits(st["out"])), "need_backward=False returns other bits than the training forward"
    if c.gamma == 0:
        assert torch.equal(bits(st["out"]), bits(inp.x)) and torch.equal(bits(st["dx"]), bits(inp.dout))
        for k in R.KEYS[1:]:
            assert bool((st["g_" + k] == R.PREFILL).all()), f"gamma = 0: gradient of {k} moved"
        assert float(st["g_gamma"]) != R.PREFILL
    if c.regime == "wq0":
        want = torch.full_like(st["P"], 1.0 / c.N)
        assert torch.equal(bits(st["P"]), bits(want)), "equal logits: P must be the bf16 rounding of fp32 1 / N"
    if c.regime == "int":
        for k, f in (("q", R.s1_qk), ("k", R.s1_qk), ("v", R.s2_v)):
            assert torch.equal(st[k].double(), f(inp, st, R.bf)[k][0]), f"integer data: {k} must equal float64"


def test_attn_refuses_without_launching(hip_ops):
    """C no multiple of 8 and B N N >= 2^31 raise with the message of check(), which runs first. Descriptors only, every
    pointer null: no tensor of that size is allocated, and nothing can be launched — a VALID descriptor with the same null
    pointers is refused too, but with the other message ("null argument"); that control is what makes the two matches below
    fail if a guard of check() is missing. Through HipOps: a real x with C = 12 and real parameters."""
    import re
    from ganslate_amd.hip import lib as L
    for (B, N, C), reason in (((1, 8, 12), "multiple of 8"), ((2, 32768, 8), "2^31"), ((1, 8, 8), "null argument")):
        d = L.AttnDesc(B, N, C)
        with pytest.raises(RuntimeError, match=re.escape(reason)):
            L.check(hip_ops.lib.gs_attn_forward(ctypes.byref(d), None, None, None, None, None), "gs_attn_forward")
        with pytest.raises(RuntimeError, match=re.escape(reason)):
            L.check(hip_ops.lib.gs_attn_backward(ctypes.byref(d), None, None, None, None, None, None, None),
                    "gs_attn_backward")
    dev = hip_ops.device
    x = torch.zeros(1, 8, 12, dtype=torch.bfloat16, device=dev)
    pd = {"gamma": torch.zeros(1, device=dev), "wq": torch.zeros(1, 12, device=dev), "bq": torch.zeros(1, device=dev),
          "wk": torch.zeros(1, 12, device=dev), "bk": torch.zeros(1, device=dev), "wv": torch.zeros(12, 12, device=dev),
          "bv": torch.zeros(12, device=dev)}
    with pytest.raises(RuntimeError, match="multiple of 8"):
        hip_ops.attn_forward(x, pd)
    torch.cuda.synchronize()
