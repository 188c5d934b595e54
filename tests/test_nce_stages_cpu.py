"""tests/nce_ref.py checked without a GPU: the stage chain with every rounding switched off against float64 autograd of
oracle/ops_ref.patchnce_reference (losses, dxq, every parameter gradient), a plain fp32 emulation through the same stage checks
and criterion as the kernels (excess at or below 2^4), the scratch layout mirror against gs_patchnce_work_bytes, and the case
table against the branches of patchnce.hip's launch plan."""
import ctypes

import pytest
import torch

from oracle.ops_ref import patchnce_reference
from tests import nce_ref as R

NAMES = [c.name for c in R.CASES]


def rel_close(got, ref, what, rel=1e-10):
    scale = max(float(ref.detach().abs().max()), 1e-300)
    err = float((got.detach().reshape(ref.shape) - ref.detach()).abs().max())
    assert err <= rel * scale, f"{what}: {err:.3e} > {rel} * {scale:.3e}"


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_the_autograd_of_the_composition(name, monkeypatch):
    """patchnce_reference casts its patches with x.float() (oracle/ops_ref.py) — the one place that keeps it from running in
    float64. For this evaluation that cast is made the identity on float64; the inputs are built BEFORE the patch, so they
    keep their fp32 values. Should the oracle cast in another way, this test fails with a dtype mismatch, not silently."""
    inp = R.build(name)
    monkeypatch.setattr(torch.Tensor, "float", torch.Tensor.double)
    c = inp.case
    xq = [t.double().requires_grad_() for t in inp.xq]
    params = inp.params.double().requires_grad_()
    losses = patchnce_reference(xq, [t.double() for t in inp.xk], params, c.batch, R.NC, c.T, R.LAMBDA)
    (losses.sum() * (1.0 if c.gs is None else c.gs)).backward()
    for l, lv in enumerate(inp.levels):
        st = R.chain(lv)
        rel_close(st["loss"], losses[l].detach().reshape(1), f"loss of level {l}")
        if c.gs == 0:
            assert float(st["dxq"].abs().max()) == 0 and float(xq[l].grad.abs().max()) == 0
            continue
        rel_close(st["dxq"], xq[l].grad.flatten(0, 1), f"dxq of level {l}")
        for k, ref in R.grads_of_level(params.grad, c.channels, l).items():
            rel_close(st[k], ref, f"{k} of level {l}")


@pytest.mark.parametrize("name", NAMES)
def test_fp32_emulation_meets_the_criterion(name):
    inp = R.build(name)
    worst = {}
    for lv in inp.levels:
        for k, v in R.measure(lv, R.emulate(lv)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"NCE_EMULATION {name} " + " ".join(f"[{k}]={v:.2f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= R.EMU_CAP, f"{name}: stage {k}: excess {v:.1f} of the fp32 emulation: change the inputs, not the cap"
    from tests.test_nce_stages_gpu import K, K2
    assert K <= R.K_CAP and K2 <= R.K2_CAP


@pytest.mark.parametrize("name", NAMES)
def test_layout_mirror_has_the_library_size(name):
    from ganslate_amd.hip import lib as L
    if not L.library_path().is_file():
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    inp = R.build(name)
    for lv in inp.levels:
        d = L.PatchNCEDesc()
        d.levels, d.batch, d.patches, d.nc, d.nce_T, d.lambda_nce = lv.L, lv.B, lv.P, R.NC, lv.T, lv.lam
        chans = inp.case.channels if lv.L > 1 or len(inp.levels) == 1 else (lv.C,)
        for i, ch in enumerate(chans):
            d.channels[i] = ch
        assert int(lib.gs_patchnce_work_bytes(ctypes.byref(d))) == lv.plan.end
        assert int(lib.gs_patchnce_param_floats(ctypes.byref(d))) == sum(R.NC * ch + 2 * R.NC + R.NC * R.NC for ch in chans)


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_branch(name):
    inp = R.build(name)
    c, p = inp.case, inp.levels[0].plan
    assert c.reaches and p.rsplit == c.rsplit and p.empty == c.empty
    assert len(p.ranges) == p.rsplit and all(a < b for a, b in p.ranges[:p.rsplit - p.empty])
    assert sum(b - a for a, b in p.ranges if a < b) == p.R
    if c.keys == "same":
        assert all(torch.equal(q, k) for q, k in zip(inp.xq, inp.xk))
    if c.keys == "int":
        lv = inp.levels[0]
        for t in (lv.xq, lv.W1, lv.b1):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 4
        assert (lv.C + 1) * 16 <= 256                                   # |pre-activation| stays an integer bf16 holds


def test_table_reaches_every_branch():
    cs = R.CASES
    plans = {c.name: R.build(c.name).levels[0].plan for c in cs}
    single = [c for c in cs if not isinstance(c.patches, tuple)]
    assert {(plans[c.name].chunks, c.rsplit, c.empty) for c in single} >= {
        (1, 1, 0), (2, 1, 0), (3, 1, 0), (5, 2, 0), (7, 3, 0), (9, 4, 1), (15, 7, 2), (16, 8, 0)}
    short = plans["chunks5"]
    assert short.ranges[-1][1] - short.ranges[-1][0] < short.per * 64
    assert any(plans[c.name].R % 64 and c.rsplit > 1 for c in single)
    assert {c.patches for c in single} >= {1, 63, 64, 65, 256}
    assert {ch for c in cs for ch in c.channels} >= {1, 3, 63, 64, 65, 256}
    assert {len(c.channels) for c in single} >= {1, 8}
    assert any(isinstance(c.patches, tuple) and len(set(c.patches)) > 1 for c in cs)
    assert {c.gs for c in cs} >= {None, 0.37, 0.0}
    assert {c.keys for c in cs} == {"corr", "same", "indep", "int"}
    assert any(c.T != 0.07 for c in cs)


@pytest.mark.parametrize("name,mutate", [("indep_keys_p2", "lo_hi"), ("warm_T", "diag")])
def test_criterion_sees_a_value_error_in_the_logits(name, mutate):
    """the fp32 emulation with the lo hi product of the logit GEMM left out, or the diagonal masked with -9, misses stage 3
    by more than the GPU test's K2: neither error is below what the criterion resolves on these rows"""
    from tests.test_nce_stages_gpu import K2
    lv = R.build(name).levels[0]
    clean, bad = R.measure(lv, R.emulate(lv))["3 loss"], R.measure(lv, R.emulate(lv, mutate))["3 loss"]
    print(f"NCE_MUTATION {name} {mutate}: stage 3 excess {clean:.2f} -> {bad:.1f}")
    assert clean <= R.EMU_CAP and bad > K2
