"""csrc/patchnce.hip stage by stage against the float64 reference of tests/nce_ref.py: every case of its table runs forward on
scratch filled with a NaN pattern, reads the scratch, runs backward into a pre-filled flat gradient and reads it again; each of
the 7 stages of every level is checked per element against float64 applied to the bits the kernels stored as that stage's
input (tests/attn_ref.py states the criterion, tests/nce_ref.py the stages and the allowance of stage 4). The k side of the
MLP, which stores no h, is checked by symmetry: a forward with xq and xk exchanged must give the same bits on the q side.

K and K2 are four times the largest excess measured on an MI355X over all cases, rounded up to a power of two; the caps are
2^8 (K_CAP, K2_CAP).
  bf16 outputs: largest excess 0.014 (stage 5 dh, case chunks7; stage 1 h and stage 4 df 0.0)                      -> K  = 2^-4
  fp32 outputs: largest excess 6.315 (stage 7 dW / db, case chunks16_p256; stage 6 dxq 4.122, stage 2 fhat / norms
                1.003, stage 3 loss 0.882)                                                                         -> K2 = 32
An excess of 0.0 means that every element is within its own bf16 rounding (stage 4: and the stated allowance) of float64.
The fp32 emulation on the CPU (tests/test_nce_stages_cpu.py) measures up to 5.45 (stage 6) on the same inputs.
"""
import pytest
import torch

from tests import nce_ref as R

pytestmark = pytest.mark.gpu

K_MEASURED, K2_MEASURED = 0.014, 6.315
K, K2 = 2.0 ** -4, 32
assert K <= R.K_CAP and K2 <= R.K2_CAP
assert 4 * K_MEASURED <= K < 8 * K_MEASURED and 4 * K2_MEASURED <= K2 < 8 * K2_MEASURED      # the next power of two


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_nce_stages(hip_ops, name):
    """one row of nce_ref.CASES (its `reaches` names the branch)"""
    inp = R.build(name)
    c = inp.case
    sts, lost, kept = R.run_gpu(hip_ops, inp, hip_ops.device)
    swapped = R.run_gpu(hip_ops, inp, hip_ops.device, swap=True)
    torch.cuda.synchronize()
    worst = {}
    for l, (lv, st) in enumerate(zip(inp.levels, sts)):
        for k, v in R.measure(lv, st).items():
            print(f"NCE_EXCESS {name} level {l} stage {k}: {v:.3f}")
            worst[k] = max(worst.get(k, 0.0), v)
    assert lost == (0, 0), f"{name}: bytes changed outside the documented buffers after forward / backward: {lost}"
    assert kept, "backward changed fhat, norms, h, df or the loss partials"
    for k, v in worst.items():
        assert v <= (K if R.is_bf16_stage(k) else K2), f"{name} ({c.reaches}): stage {k}: excess {v:.1f}"
    bits = lambda t: t.contiguous().view(torch.int32)
    for l, (lv, st) in enumerate(zip(inp.levels, sts)):
        assert torch.equal(bits(swapped[l]), bits(st["fk"])), f"level {l}: the k side is not the q side's code on xk"
        if c.keys == "same":
            assert torch.equal(bits(st["fq"]), bits(st["fk"]))
        if c.keys == "int":
            assert torch.equal(st["h"].double(), R.s1_h(lv, st, R.bf)["h"][0]), "integer data: h must equal float64"
        if c.gs == 0:
            assert float(st["dxq"].abs().max()) == 0 and float(st["dh"].float().abs().max()) == 0
            for k in ("g_W1", "g_b1", "g_W2", "g_b2"):
                assert bool((st[k] == R.PREFILL).all()), f"grad_scale = 0: {k} moved"
