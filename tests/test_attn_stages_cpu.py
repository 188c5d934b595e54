"""tests/attn_ref.py checked without a GPU: the stage chain with every rounding switched off against float64 autograd of
oracle/ops_ref.attention_reference, a plain fp32 emulation of the chain through the same stage checks and criterion as the
kernels (its excess must stay at or below 2^4), the scratch layout mirror against the library's own size functions, and the
case table against the branches of attn.hip's launch plan."""
import ctypes

import pytest
import torch

from oracle.ops_ref import attention_reference
from tests import attn_ref as R

NAMES = [c.name for c in R.CASES]


def library():
    from ganslate_amd.hip import lib as L
    if not L.library_path().is_file():
        import __graft_entry__
        __graft_entry__.build()
    return L, L.load()


def rel_close(got, ref, what, scale=None, rel=1e-10):
    scale = max(float(ref.abs().max()), 1e-300) if scale is None else float(scale)
    err = float((got.reshape(ref.shape) - ref).abs().max())
    assert err <= rel * scale, f"{what}: {err:.3e} > {rel} * {scale:.3e}"


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_the_autograd_of_the_block(name):
    inp = R.build(name)
    st = R.chain(inp)
    x = inp.x.double().requires_grad_()
    pr = {k: v.double().requires_grad_() for k, v in inp.params.items()}
    out = attention_reference(x, pr)
    out.backward(inp.dout.double())
    rel_close(st["out"], out.detach(), "out")
    rel_close(st["dx"], x.grad, "dx")
    for k in R.KEYS:
        ref, scale = pr[k].grad, None
        if k == "bk":
            # the key bias moves every logit of a row alike: its true gradient is zero and autograd's is rounding noise of
            # the terms that cancel, which are of the size of bq's gradient (gamma = 0 or Wq = 0: everything is zero)
            scale = max(float(pr["bq"].grad.abs().max()), 1e-300)
        elif float(ref.abs().max()) == 0:
            assert inp.case.gamma == 0 or inp.case.regime == "wq0" or inp.case.N == 1, k      # (one key: P = 1 whatever q, k)
            assert float(st["g_" + k].abs().max()) == 0, k
            continue
        rel_close(st["g_" + k], ref, k, scale=scale)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_emulation_meets_the_criterion(name):
    inp = R.build(name)
    res, bad = R.measure(inp, R.emulate(inp))
    print(f"ATTN_EMULATION {name} " + " ".join(f"[{k}]={v:.2f}" for k, v in res.items()))
    assert not bad, bad
    for k, v in res.items():
        assert v <= R.EMU_CAP, f"{name}: stage {k}: excess {v:.1f} of the fp32 emulation: change the inputs, not the cap"
    from tests.test_attn_stages_gpu import K, K2
    assert K <= R.K_CAP and K2 <= R.K2_CAP


@pytest.mark.parametrize("name", NAMES)
def test_layout_mirror_has_the_library_sizes(name):
    L, lib = library()
    c, p = R.BY_NAME[name], R.build(name).plan
    d = L.AttnDesc(c.B, c.N, c.C)
    assert int(lib.gs_attn_work_bytes(ctypes.byref(d))) == p.end
    assert int(lib.gs_attn_forward_work_bytes(ctypes.byref(d))) == p.fwd_end
    offs = [v[2] for v in p.views.values()]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs)
    m_f, m_b = R.written_mask(p, False), R.written_mask(p, True)
    assert m_f.numel() == m_b.numel() == p.end and bool((m_b[:p.fwd_end] == m_f[:p.fwd_end]).all()) and not bool(m_f[p.fwd_end:].any())


REFUSALS = [((1, 8, 12), "multiple of 8"), ((1, 8, 4), "multiple of 8"), ((2, 32768, 8), "2^31"), ((1, 46341, 8), "2^31"),
            ((1, 8, 8), "null argument"), ((1, 46340, 8), "null argument")]      # the last two: valid descriptors (control)


def test_refusals_are_host_side():
    """C no multiple of 8 and B N N >= 2^31 are refused by check(), which runs before the null-pointer test and before any
    launch: the library's error text names the reason. The pointers are null, so a valid descriptor is refused as well —
    with the OTHER message: were a guard of check() missing, its rows would read "null argument" and fail here."""
    L, lib = library()
    for (B, N, C), reason in REFUSALS:
        d = L.AttnDesc(B, N, C)
        assert lib.gs_attn_forward(ctypes.byref(d), None, None, None, None, None) != 0, (B, N, C)
        assert reason in lib.gs_last_error().decode(), (B, N, C, lib.gs_last_error())
        assert lib.gs_attn_backward(ctypes.byref(d), None, None, None, None, None, None, None) != 0, (B, N, C)
        assert reason in lib.gs_last_error().decode(), (B, N, C, lib.gs_last_error())


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_branch(name):
    c, inp = R.BY_NAME[name], R.build(name)
    p = inp.plan
    assert c.reaches and p.splits == c.splits and p.kc * p.splits == p.rows
    assert p.tiles == c.tiles and (c.N % 64 == 0) == (p.tiles * 64 == c.N)
    assert p.dout_blocks == min(512, -(-c.B * c.N * c.C // 256))
    if c.regime == "sharp":
        s = R.chain(inp)["S"]
        assert 29.0 <= float(s.abs().max()) <= 31.0
        pmax = torch.softmax(s, -1).max(-1).values
        assert float(pmax.mean()) > (0.5 if c.N <= 130 else 0.3) and float(pmax.max()) > 0.9
    if c.regime == "uniform" and c.N > 1:
        assert float(torch.softmax(R.chain(inp)["S"], -1).max()) < 8.0 / c.N
    if c.regime == "wq0":
        assert float(R.chain(inp)["S"].abs().max()) == 0.0
    if c.regime == "int":
        for k, v in inp.params.items():
            assert k == "gamma" or (torch.equal(v, v.round()) and float(v.abs().max()) <= 8)
        assert torch.equal(inp.x.float(), inp.x.float().round())


def test_table_reaches_every_branch():
    cs = R.CASES
    assert {c.N for c in cs} >= {1, 63, 64, 65, 130, 300}
    assert {c.C for c in cs} >= {8, 24, 40, 64, 72} and {c.C // 8 for c in cs} >= {1, 3, 5, 8, 9}
    assert any(c.B * c.N * c.C > 2048 * 256 for c in cs)                             # the residual kernel's grid wraps
    assert {c.B for c in cs} >= {1, 3}
    assert {c.splits for c in cs} >= {1, 2, 16, 32}
    assert any(c.splits == 1 and (c.B * c.N) % 2 for c in cs)
    assert {c.regime for c in cs} == {"uniform", "sharp", "wq0", "int"}
    assert any(c.gamma == 0 for c in cs)
    assert any(c.N > 256 for c in cs)                                               # the softmax loop's second trip
    assert any(c.N % 32 and c.N > 64 and c.regime == "sharp" for c in cs)           # ragged K = N of the N x N GEMMs
    assert any(R.rup(c.C // 8, 8) == c.C // 8 for c in cs) and any(R.rup(c.C // 8, 8) != c.C // 8 for c in cs)
    assert any((c.B * c.N // c.splits) % 32 for c in cs if c.splits > 1)             # a K split with a ragged last step
    assert {c.tiles for c in cs} >= {1, 2, 3, 4, 5}
    assert any(c.tiles * 64 == c.N for c in cs) and any(c.tiles * 64 - c.N == 63 for c in cs)      # full, and one row of a tile
    blocks = {R.build(c.name).plan.dout_blocks for c in cs}
    assert 1 in blocks and 512 in blocks and any(1 < b < 512 for b in blocks)           # the dgamma partials: 1, some, all 512
