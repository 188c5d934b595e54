"""The K loop of wgrad_kernel (csrc/wgrad.hip) — the 3-stage LDS-DMA ring two K-steps ahead, the inline-assembly fragment reads
with counted waits, the carry arithmetic of the staged rows — bit for bit against the float64 reference on the integer domain of
tests/exact.py: every element of dw and db, onto a non-zero integer prefill. The cases, their exactness precondition and the
branch each of them takes by the launch rule are stated and checked in tests/test_wgrad_ring_cpu.py; here every case is forced
onto the im2col kernel with the library's own switches and the library's plan is compared with the launch rule first, so a
later retune cannot move a case off its branch silently.
"""
import pytest
import torch

from ganslate_amd.nn.native.twin import Twin
from tests import exact
from tests.test_wgrad_ring_cpu import (ALL, CASES, IM2COL_ONLY, PREFILL_B, PREFILL_W, SPLIT, _ids, assert_on_its_branch, case_of,
                                       reference)

pytestmark = pytest.mark.gpu


def operands(c, dev):
    """(dense side, gathered side) of the weight gradient: dY and X for a conv, X and dY for a transposed conv"""
    a, g = (c.gy, c.xa) if c.spec.kind == "conv" else (c.xa, c.gy)
    return a.to(dev), g.to(dev)


def run_wgrad(ops, c, prefill=PREFILL_W, **kw):
    sp = c.spec
    a, g = operands(c, ops.device)
    dw = torch.full((sp.P * sp.T * sp.Q,), prefill, dtype=torch.float32, device=ops.device)
    ops.wgrad(c.low.wgrad, a, g, dw, **kw)
    torch.cuda.synchronize()
    return dw.cpu().view(sp.P, sp.T, sp.Q)


@pytest.mark.parametrize("case", ALL, ids=_ids)
def test_weight_and_bias_gradient_of_every_case(hip_ops, case):
    """slab path (several splits) or in-place add (one split), whichever the launch rule gives the case"""
    c = case_of(case)
    dw_ref, db_ref = reference(c)
    with hip_ops.options(**IM2COL_ONLY):
        assert_on_its_branch(hip_ops.lib, case, c)
        dw = run_wgrad(hip_ops, c)
    exact.assert_identical(dw, dw_ref + PREFILL_W, f"{case[0]}: weight gradient [P][T][Q]")
    db = torch.full((c.spec.cout_p,), PREFILL_B, dtype=torch.float32, device=hip_ops.device)
    hip_ops.bias_grad(c.gy.to(hip_ops.device), c.spec.cout_p, db)
    torch.cuda.synchronize()
    exact.assert_identical(db.cpu(), db_ref + PREFILL_B, f"{case[0]}: bias gradient")


@pytest.mark.parametrize("case", [CASES[2], CASES[5], CASES[9], CASES[11]], ids=_ids)
def test_one_split_stores_into_a_fresh_buffer(hip_ops, case):
    """dw_fresh = 1: the caller guarantees zeros, the kernel stores without reading (the one path with no prefill to add to)"""
    c = case_of(case)
    with hip_ops.options(**IM2COL_ONLY):
        rule = assert_on_its_branch(hip_ops.lib, case, c)
        assert rule["splits"] == 1
        dw = run_wgrad(hip_ops, c, prefill=0.0, fresh=True)
    exact.assert_identical(dw, reference(c)[0], f"{case[0]}: weight gradient into a fresh buffer")


@pytest.mark.parametrize("case", [CASES[3], CASES[7]], ids=_ids)
def test_one_split_without_the_row_epilogue(hip_ops, case):
    """wgrad_rows = 0: the accumulator layout goes to dw as it stands (fp32 atomics with a single contributor)"""
    c = case_of(case)
    with hip_ops.options(wgrad_rows=0, **IM2COL_ONLY):
        dw = run_wgrad(hip_ops, c)
    exact.assert_identical(dw, reference(c)[0] + PREFILL_W, f"{case[0]}: wgrad_rows=0")


def test_several_splits_through_slabs_twice(hip_ops):
    c = case_of(SPLIT)
    with hip_ops.options(**IM2COL_ONLY):
        rule = assert_on_its_branch(hip_ops.lib, SPLIT, c)
        assert rule["splits"] == 2 and rule["chunk"] == 640
        one, two = run_wgrad(hip_ops, c), run_wgrad(hip_ops, c)
    assert torch.equal(one, two), "two runs of the slab path differ"
    exact.assert_identical(one, reference(c)[0] + PREFILL_W, "2 splits, slab path")


@pytest.mark.parametrize("rows", [1, 0])
def test_several_splits_through_atomics(hip_ops, rows, monkeypatch):
    """no workspace: both splits add their tiles to dw with fp32 atomics (exact in any order on this domain); rows = 1 keeps
    the library's default, where only a one-split launch would take the row epilogue"""
    monkeypatch.setenv("GS_WGRAD_DET", "0")
    c = case_of(SPLIT)
    with hip_ops.options(wgrad_rows=rows, **IM2COL_ONLY):
        assert_on_its_branch(hip_ops.lib, SPLIT, c)
        dw = run_wgrad(hip_ops, c)
    exact.assert_identical(dw, reference(c)[0] + PREFILL_W, f"2 splits, atomics, wgrad_rows={rows}")


def test_several_splits_without_the_row_epilogue_through_slabs(hip_ops):
    c = case_of(SPLIT)
    with hip_ops.options(wgrad_rows=0, **IM2COL_ONLY):
        dw = run_wgrad(hip_ops, c)
    exact.assert_identical(dw, reference(c)[0] + PREFILL_W, "2 splits, slabs written from the accumulator layout")


def test_twin_batch_splits_each_network_on_its_own(hip_ops):
    """the same shape as a twin batch (gs_wgrad_ws_twin, wgrad_twin = 1): 2 splits per network, no workgroup straddles the two —
    each network's gradient is its own reference, to the bit"""
    ca, cb = case_of(SPLIT, seed=71), case_of(SPLIT, seed=83)
    sp, dev = ca.spec, hip_ops.device
    (a1, g1), (a2, g2) = operands(ca, dev), operands(cb, dev)
    dw = torch.full((2, sp.master_numel), PREFILL_W, dtype=torch.float32, device=dev)
    with hip_ops.options(wgrad_twin=1, **IM2COL_ONLY):
        rule = assert_on_its_branch(hip_ops.lib, SPLIT, ca, nets=2)
        assert rule["splits"] == 2 and rule["ws_floats"] == 4 * sp.master_numel
        hip_ops.wgrad(ca.low.wgrad, torch.cat([a1, a2]), torch.cat([g1, g2]), Twin(dw[0], dw[1]))
        torch.cuda.synchronize()
    for h, c in enumerate((ca, cb)):
        exact.assert_identical(dw[h].cpu().view(sp.P, sp.T, sp.Q), reference(c)[0] + PREFILL_W, f"twin batch, network {h}")


def test_fused_adam_equals_weight_gradient_plus_adam(hip_ops):
    """gs_wgrad_adam on a 5-K-step layer against the weight gradient and the Adam update run separately, bit for bit
    (tests/test_ops_gpu.py::test_weight_gradient_with_fused_adam is the model), and the gradient it used is the reference's:
    an update from the float64 gradient gives the same parameters"""
    ops, dev = hip_ops, hip_ops.device
    case = CASES[3]
    c = case_of(case)
    sp, w = c.spec, c.low.wgrad
    a, gt = operands(c, dev)
    g = torch.Generator().manual_seed(91)
    n, off = sp.master_numel, 64
    tot = n + 2 * off
    p0, m0, v0 = torch.randn(tot, generator=g) * 0.05, torch.randn(tot, generator=g) * 1e-3, torch.rand(tot, generator=g) * 1e-4
    n8 = n // 8
    perm_f, perm_d = torch.randperm(n8, generator=g).int(), torch.randperm(n8, generator=g).int()
    perm_d[::5] = -1
    hyper = torch.tensor([2e-4, 0.5, 0.999, 1e-8, 1 - 0.5 ** 3, (1 - 0.999 ** 3) ** 0.5])
    P, T, Q = w.P, w.T, w.Q
    kp = P + 8
    tr_base = torch.arange(T, dtype=torch.int32) * Q * kp + 16
    tr_base[1] = -1
    tr_kp = torch.full((T,), kp, dtype=torch.int32)
    sl = slice(off, off + n)

    def run(mode):
        p, m, v = p0.clone().to(dev), m0.clone().to(dev), v0.clone().to(dev)
        fpack = torch.zeros(n8 * 8, dtype=torch.bfloat16, device=dev)
        dpack = torch.zeros(n8 * 8, dtype=torch.bfloat16, device=dev)
        tpack = torch.zeros(T * Q * kp + 16, dtype=torch.bfloat16, device=dev)
        packs = (perm_f.to(dev), fpack, perm_d.to(dev), dpack)
        if mode == "fused":
            assert ops.wgrad_adam(w, a, gt, p[sl], m[sl], v[sl], hyper.to(dev), packs, tr=(tr_base.to(dev), tr_kp.to(dev), tpack))
        else:
            if mode == "separate":
                dw = torch.zeros(n, dtype=torch.float32, device=dev)
                ops.wgrad(w, a, gt, dw, fresh=True)
            else:
                dw = reference(c)[0].reshape(-1).clone().to(dev)
            ops.adam_step_dev(p[sl], dw, m[sl], v[sl], hyper.to(dev), grad_scale=1.0, zero_grad=True, packs=packs)
            W = p[sl].view(P, T, Q)
            for t in range(T):
                if int(tr_base[t]) >= 0:
                    dst = int(tr_base[t]) + torch.arange(Q, device=dev)[None, :] * kp + torch.arange(P, device=dev)[:, None]
                    tpack[dst.reshape(-1)] = W[:, t, :].reshape(-1).to(torch.bfloat16)
        torch.cuda.synchronize()
        return [t.cpu() for t in (p, m, v, fpack, dpack, tpack)]

    with ops.options(**IM2COL_ONLY):
        assert_on_its_branch(ops.lib, case, c)
        fused, separate, from_ref = run("fused"), run("separate"), run("reference")
    for k, name in enumerate(("p", "m", "v", "fpack", "dpack", "transposed pack")):
        assert torch.equal(fused[k], separate[k]), f"{name}: fused vs weight gradient + update"
        assert torch.equal(fused[k], from_ref[k]), f"{name}: fused vs update from the float64 gradient"
        if k < 3:
            assert torch.equal(fused[k][:off], (p0, m0, v0)[k][:off]) and torch.equal(fused[k][off + n:], (p0, m0, v0)[k][off + n:])
    assert not torch.equal(fused[0][sl], p0[sl])
