"""Float64 reference of csrc/attn.hip (SelfAttentionBlock), one function per stage, for tests/test_attn_stages_{cpu,gpu}.py.

The kernel keeps every intermediate in the scratch tensor HipOps hands back as `saved`; `plan()` mirrors its layout (written
from the header comment and plan() of attn.hip) and `extract()` reads the named buffers out of it. Every stage below is ONE
float64 function of the bits the kernel itself stored as that stage's input, so no error propagation is budgeted and passing
every stage proves the chain. A stage returns {output name: (r, T)}: the float64 result and, per element, the sum of the
absolute values of the terms that form it. An operand the kernel rounds to bf16 while staging is rounded the same way here
(one fp32 -> bf16 round to nearest even); the split GEMMs are stated as documented, hi hi + hi lo + lo hi with hi = bf16(v),
lo = bf16(v - hi) — NOT as the true product, from which that statement itself is ~2^-17 away.

Criterion, per element (U = 2^-24):
  bf16 outputs   |got - r|            <= 2^-8 |r| + K  U T + 2^-126
  fp32 outputs   |got - prefill - r|  <= K2 U T + 2^-126          (T includes |prefill| where the output is added into one)
`*_excess` return the K (K2) an element needs; the absolute floor covers probabilities in the subnormal range. Everything a
stage does not document as written must keep its pre-fill: `written_mask` is the documented set, byte by byte.

With `rb=ident` (every bf16 rounding switched off) the chain of stages is the SelfAttentionBlock in float64:
tests/test_attn_stages_cpu.py compares it with autograd of oracle/ops_ref.attention_reference.
"""
import zlib
from contextlib import contextmanager
from dataclasses import dataclass
from types import SimpleNamespace

import torch

U24, HALF_BF16, FLOOR = 2.0 ** -24, 2.0 ** -8, 2.0 ** -126
K_CAP = K2_CAP = 2 ** 8          # conditions, not measurements
EMU_CAP = 2 ** 4                 # the fp32 emulation on the committed inputs
PREFILL = 0.25                   # of every gradient tensor (added into)
POISON = 0xFF                    # scratch byte: bf16 0xFFFF and fp32 0xFFFFFFFF are NaNs
DOUT_BLOCKS = 512
KEYS = ("gamma", "wq", "bq", "wk", "bk", "wv", "bv")


# ---- roundings and the criterion ------------------------------------------------------------------------------------------
def bf(t):
    """one fp32 -> bf16 rounding (nearest even), as float64"""
    return t.float().to(torch.bfloat16).double()


def ident(t):
    return t.double()


def split(v, rb):
    """hi = bf16(v), lo = bf16(v - hi) of an fp32 tensor (v - hi is exact in fp32); rb=ident: (v, 0)"""
    if rb is ident:
        return v.double(), torch.zeros_like(v, dtype=torch.float64)
    assert v.dtype == torch.float32
    hi = v.to(torch.bfloat16).float()
    return hi.double(), (v - hi).to(torch.bfloat16).double()


def _units(err, T):
    ex = err / (U24 * T)
    ex = torch.where(T > 0, ex, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return torch.nan_to_num(ex, nan=float("inf"))


def bf16_excess(got, r, T, extra=None):
    """(|got - r| - 2^-8 |r| - extra - 2^-126) / (2^-24 T) per element; T == 0: the element must meet the rest exactly"""
    err = (got.double() - r).abs() - HALF_BF16 * r.abs() - FLOOR
    if extra is not None:
        err = err - extra
    return _units(err, T)


def f32_excess(got, r, T):
    """got: the stored value minus its pre-fill, in float64"""
    return _units((got.double() - r).abs() - FLOOR, T)


def worst(ex):
    return max(float(ex.max()), 0.0) if ex.numel() else 0.0


@contextmanager
def poisoned_scratch():
    """every uint8 tensor HipOps allocates inside (its scratch buffers) starts as a NaN pattern.
    This depends on HipOps allocating its scratch as torch.empty(size, dtype=torch.uint8, ...) with dtype given by keyword
    (hip/ops.py: attn_forward, patchnce_forward). Should that change, the fill silently stops — and `untouched()` then fails,
    since it requires the poison byte everywhere outside the documented buffers: the dependency cannot break unnoticed."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        if k.get("dtype") is torch.uint8:
            t.fill_(POISON)
        return t
    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


# ---- the scratch layout (attn.hip: Plan / plan()) ---------------------------------------------------------------------------
def rup(v, m):
    return (v + m - 1) // m * m


def plan(B, N, C):
    """byte offsets of the named buffers, the sizes of the two scratch variants and the launch plan's branches"""
    p = SimpleNamespace(B=B, N=N, C=C, dq=C // 8, dp=rup(C // 8, 8), rows=B * N, views={})
    p.ct = 2 * p.dp + C
    o = 0

    def take(name, dtype, shape):
        nonlocal o
        n = 1
        for s in shape:
            n *= s
        p.views[name] = (dtype, shape, o)
        o += rup(n * torch.empty((), dtype=dtype).element_size(), 256)
    take("qk", torch.float32, (B, N, 2, p.dp))             # q | k in fp32, dq of dp columns each
    take("qkv", torch.bfloat16, (B, N, p.ct))              # only the v columns [2 dp, ct) are written
    take("O", torch.bfloat16, (B, N, C))
    take("P", torch.bfloat16, (B, N, N))
    take("S", torch.float32, (B, N, N))                    # logits after forward, dP after backward
    p.fwd_end = o
    take("dqkv", torch.bfloat16, (B, N, p.ct))
    take("dO", torch.bfloat16, (B, N, C))
    take("dS", torch.bfloat16, (B, N, N))
    take("part", torch.float32, (DOUT_BLOCKS,))
    take("wcat", torch.float32, (p.ct, C))
    p.splits = next((sp for sp in (32, 16, 8, 4, 2) if p.rows % sp == 0 and p.rows // sp >= 128), 1)
    p.kc = p.rows // p.splits
    take("dws", torch.float32, (p.splits if p.splits > 1 else 0, C, C))
    p.end = o
    p.dout_blocks = min(DOUT_BLOCKS, (p.rows * C + 255) // 256)
    p.tiles = (N + 63) // 64
    return p


def view(work, p, name):
    dtype, shape, off = p.views[name]
    n = 1
    for s in shape:
        n *= s
    return work[off:off + n * torch.empty((), dtype=dtype).element_size()].view(dtype).reshape(shape)


def written_mask(p, backward):
    """bytes of the training scratch a forward (and a backward) documents as written; nothing behind fwd_end after forward"""
    m = torch.zeros(p.end, dtype=torch.bool)
    full = ["O", "P", "S"] + (["dqkv", "dO", "dS", "wcat", "dws"] if backward else [])
    for name in full:
        dtype, shape, off = p.views[name]
        n = torch.empty((), dtype=dtype).element_size()
        for s in shape:
            n *= s
        m[off:off + n] = True
    off = p.views["qk"][2]
    m[off:off + p.rows * 2 * p.dp * 4].view(p.rows, 2, p.dp, 4)[:, :, :p.dq] = True
    off = p.views["qkv"][2]
    m[off:off + p.rows * p.ct * 2].view(p.rows, p.ct, 2)[:, 2 * p.dp:] = True
    if backward:
        off = p.views["part"][2]
        m[off:off + p.dout_blocks * 4] = True
    return m


def untouched(work, p, backward):
    """-> number of bytes outside the documented set that lost their pre-fill"""
    m = written_mask(p, backward)
    assert work.numel() == m.numel(), (work.numel(), m.numel())
    return int((work[~m] != POISON).sum())


def extract(work_fwd, work_bwd, p):
    """the named intermediates (logical shapes) from the scratch as read after forward and again after backward"""
    st = {}
    qk = view(work_fwd, p, "qk")
    st["q"], st["k"] = qk[:, :, 0, :p.dq].contiguous(), qk[:, :, 1, :p.dq].contiguous()
    st["v"] = view(work_fwd, p, "qkv")[:, :, 2 * p.dp:].contiguous()
    for n in ("O", "P", "S"):
        st[n] = view(work_fwd, p, n).clone()
    if work_bwd is not None:
        d = view(work_bwd, p, "dqkv")
        st["dq"], st["dk"], st["dv"] = d[:, :, :p.dq], d[:, :, p.dp:p.dp + p.dq], d[:, :, 2 * p.dp:]
        st["pad"] = torch.stack([d[:, :, p.dq:p.dp], d[:, :, p.dp + p.dq:2 * p.dp]])
        st["dqkv"] = d
        st["dP"] = view(work_bwd, p, "S")
        for n in ("dO", "dS", "wcat"):
            st[n] = view(work_bwd, p, n)
    return st


# ---- the stages -------------------------------------------------------------------------------------------------------------
def mm(a, b):
    """(r, T) of a float64 matrix product over the last / first axes of a [.., m, k] and b [.., k, n]"""
    return a @ b, a.abs() @ b.abs()


def s1_qk(inp, st, rb):
    """q = x (hi(Wq) + lo(Wq))^T + bq, k likewise: fp32, x is exact in bf16 (its lo part is zero)"""
    x, out = inp.x.double(), {}
    for n in "qk":
        hi, lo = split(inp.params["w" + n], rb)
        b = inp.params["b" + n].double()
        out[n] = (x @ hi.t() + x @ lo.t() + b, x.abs() @ hi.abs().t() + x.abs() @ lo.abs().t() + b.abs())
    return out


def s2_v(inp, st, rb):
    """v = bf16(x bf16(Wv)^T + bv)"""
    x, w, b = inp.x.double(), rb(inp.params["wv"]), inp.params["bv"].double()
    return {"v": (x @ w.t() + b, x.abs() @ w.abs().t() + b.abs())}


def s3_S(inp, st, rb):
    """S = q_hi k_hi^T + q_hi k_lo^T + q_lo k_hi^T per image"""
    (qh, ql), (kh, kl) = split(st["q"], rb), split(st["k"], rb)
    t = lambda a: a.transpose(1, 2)
    r = qh @ t(kh) + qh @ t(kl) + ql @ t(kh)
    return {"S": (r, qh.abs() @ t(kh.abs()) + qh.abs() @ t(kl.abs()) + ql.abs() @ t(kh.abs()))}


def s4_P(inp, st, rb):
    """P = bf16(softmax(S)); T = r (1 + |s - max|): exp of an argument known to 2^-24 |s - max|, and the normaliser"""
    s = st["S"].double()
    d = s - s.max(-1, keepdim=True).values
    r = torch.softmax(s, -1)
    return {"P": (r, r * (1 + d.abs()))}


def s5_O(inp, st, rb):
    """O = bf16(P v)"""
    return {"O": mm(st["P"].double(), st["v"].double())}


def s6_out(inp, st, rb):
    """out = bf16(gamma O + x)"""
    g, O, x = inp.params["gamma"].double(), st["O"].double(), inp.x.double()
    return {"out": (g * O + x, (g * O).abs() + x.abs())}


def s7_dO(inp, st, rb):
    """dO = bf16(gamma dout); dgamma += sum dout o O"""
    g, d, O = inp.params["gamma"].double(), inp.dout.double(), st["O"].double()
    return {"dO": (g * d, (g * d).abs()), "g_gamma": ((d * O).sum().reshape(1), (d * O).abs().sum().reshape(1) + PREFILL)}


def s8_dv(inp, st, rb):
    """dv = bf16(P^T dO)"""
    return {"dv": mm(st["P"].double().transpose(1, 2), st["dO"].double())}


def s9_dP(inp, st, rb):
    """dP = dO v^T, fp32"""
    return {"dP": mm(st["dO"].double(), st["v"].double().transpose(1, 2))}


def s10_dS(inp, st, rb):
    """dS = bf16(P o (dP - sum_j P o dP))"""
    P, dP = st["P"].double(), st["dP"].double()
    t, ta = (P * dP).sum(-1, keepdim=True), (P * dP).abs().sum(-1, keepdim=True)
    return {"dS": (P * (dP - t), P.abs() * (dP.abs() + ta))}


def s11_dqdk(inp, st, rb):
    """dq = bf16(dS bf16(k)), dk = bf16(dS^T bf16(q))"""
    dS = st["dS"].double()
    return {"dq": mm(dS, rb(st["k"])), "dk": mm(dS.transpose(1, 2), rb(st["q"]))}


def s13_dx(inp, st, rb):
    """dx = bf16(dout + [dq | 0 | dk | 0 | dv] bf16([Wq; 0; Wk; 0; Wv])) from the stored dqkv and the stored stacked weights"""
    d, w, g = st["dqkv"].double(), rb(st["wcat"]), inp.dout.double()
    return {"dx": (g + d @ w, g.abs() + d.abs() @ w.abs())}


def s14_params(inp, st, rb):
    """dW{q,k,v} += dproj^T x, db{q,k,v} += sum over the rows of dproj, from the stored dqkv"""
    x, out = inp.x.double().flatten(0, 1), {}
    for n in "qkv":
        d = st["d" + n].double().flatten(0, 1)
        out["g_w" + n] = (d.t() @ x, d.abs().t() @ x.abs() + PREFILL)
        out["g_b" + n] = (d.sum(0), d.abs().sum(0) + PREFILL)
    return out


def wcat_expected(inp, p):
    w = torch.zeros(p.ct, p.C)
    w[:p.dq], w[p.dp:p.dp + p.dq], w[2 * p.dp:] = inp.params["wq"], inp.params["wk"], inp.params["wv"]
    return w


FORWARD = (("1 q,k", s1_qk), ("2 v", s2_v), ("3 S", s3_S), ("4 P", s4_P), ("5 O", s5_O), ("6 out", s6_out))
BACKWARD = (("7 dO,dgamma", s7_dO), ("8 dv", s8_dv), ("9 dP", s9_dP), ("10 dS", s10_dS), ("11 dq,dk", s11_dqdk),
            ("13 dx", s13_dx), ("14 dW,db", s14_params))
FP32_OUT = {"q", "k", "S", "dP"}


def chain(inp):
    """all stages in float64 with every bf16 rounding switched off, each fed by the one before: the block and its gradients"""
    p, st = inp.plan, {}
    for _, f in FORWARD + BACKWARD:
        if f is s13_dx:
            z = torch.zeros(p.B, p.N, p.dp - p.dq, dtype=torch.float64)
            st["dqkv"] = torch.cat([st["dq"], z, st["dk"], z, st["dv"]], -1)
            st["wcat"] = wcat_expected(inp, p).double()
        st.update({k: r for k, (r, _) in f(inp, st, ident).items()})
    return st


def measure(inp, st):
    """{"<stage>:bf16" | "<stage>:fp32": the largest excess of the stage's outputs of that type} (stage 7 has one of each:
    dO and dgamma), and the list of exact conditions that failed. Outputs named g_* are gradient tensors as stored (pre-fill
    included). bf16 outputs are held to K, fp32 outputs to K2 (`is_bf16_stage` reads the suffix)."""
    p, res, bad = inp.plan, {}, []
    stages = FORWARD + (BACKWARD if "dx" in st else ())
    for name, f in stages:
        for k, (r, T) in f(inp, st, bf).items():
            if k.startswith("g_"):
                e, kind = f32_excess(st[k].double().reshape(r.shape) - PREFILL, r, T), "fp32"
            elif k in FP32_OUT:
                assert st[k].dtype == torch.float32, k
                e, kind = f32_excess(st[k], r, T), "fp32"
            else:
                assert st[k].dtype == torch.bfloat16, k
                e, kind = bf16_excess(st[k], r, T), "bf16"
            res[f"{name}:{kind}"] = max(res.get(f"{name}:{kind}", 0.0), worst(e))
    if "dx" in st:
        if st["pad"].numel() and not bool((st["pad"].view(torch.int16) == 0).all()):      # stage 12
            bad.append("pad columns of dqkv are not zero")
        if not torch.equal(st["wcat"].view(torch.int32), wcat_expected(inp, p).view(torch.int32)):
            bad.append("wcat is not [Wq; 0; Wk; 0; Wv]")
    return res, bad


def is_bf16_stage(key):
    return key.endswith(":bf16")


def emulate(inp):
    """the chain in plain torch fp32 with the documented roundings: what a correct fp32 implementation stores"""
    p, P_, st = inp.plan, inp.params, {}
    b16 = lambda t: t.to(torch.bfloat16)
    sp = lambda t: (b16(t).float(), b16(t - b16(t).float()).float())
    x, dout, g = inp.x.float(), inp.dout.float(), P_["gamma"]
    for n in "qk":
        hi, lo = sp(P_["w" + n])
        st[n] = x @ hi.t() + x @ lo.t() + P_["b" + n]
    st["v"] = b16(x @ b16(P_["wv"]).float().t() + P_["bv"])
    (qh, ql), (kh, kl) = sp(st["q"]), sp(st["k"])
    t = lambda a: a.transpose(1, 2)
    st["S"] = ql @ t(kh) + qh @ t(kl) + qh @ t(kh)
    st["P"] = b16(torch.softmax(st["S"], -1))
    st["O"] = b16(st["P"].float() @ st["v"].float())
    st["out"] = b16(g * st["O"].float() + x)
    st["dO"] = b16(g * dout)
    grads = {k: torch.full_like(v, PREFILL) for k, v in P_.items()}
    grads["gamma"] += (dout * st["O"].float()).sum()
    st["dv"] = b16(t(st["P"].float()) @ st["dO"].float())
    st["dP"] = st["dO"].float() @ t(st["v"].float())
    Pf = st["P"].float()
    st["dS"] = b16(Pf * (st["dP"] - (Pf * st["dP"]).sum(-1, keepdim=True)))
    st["dq"] = b16(st["dS"].float() @ b16(st["k"]).float())
    st["dk"] = b16(t(st["dS"].float()) @ b16(st["q"]).float())
    z = torch.zeros(p.B, p.N, p.dp - p.dq, dtype=torch.bfloat16)
    st["pad"] = torch.stack([z, z])
    st["dqkv"] = torch.cat([st["dq"], z, st["dk"], z, st["dv"]], -1)
    st["wcat"] = wcat_expected(inp, p)
    st["dx"] = b16(dout + st["dqkv"].float() @ b16(st["wcat"]).float())
    xr = x.flatten(0, 1)
    for n in "qkv":
        d = st["d" + n].float().flatten(0, 1)
        grads["w" + n] += d.t() @ xr
        grads["b" + n] += d.sum(0)
    st.update({"g_" + k: v for k, v in grads.items()})
    return st


# ---- the cases --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    B: int
    N: int
    C: int
    regime: str          # uniform (logits rescaled to a spread of +-1) | sharp (rescaled to +-30: the typical row gives one key
                         # more than half of the weight — a third at N = 300 — and some rows are one-hot to 0.9) | wq0 | int
    gamma: float
    reaches: str
    splits: int          # asserted against the plan
    tiles: int           # 64-row tiles of N, asserted against the plan


CASES = [
    Case("one_voxel", 1, 1, 8, "uniform", 0.7, "N = 1: one ragged tile of one row, dq = 1 of dp = 8", 1, 1),
    Case("n63_c24", 3, 63, 24, "uniform", 0.7, "N = 63, dq = 3 (dp != dq), batch strides, odd row count", 1, 1),
    Case("n64_c40", 1, 64, 40, "sharp", 0.7, "N = 64: one full tile, dq = 5; logits spread over +-30", 1, 1),
    Case("n65_c64", 3, 65, 64, "sharp", 0.7, "N = 65: a second tile of one row, dq = 8 = dp (no pad), 195 rows: splits 1", 1, 2),
    Case("n130_c72", 1, 130, 72, "sharp", 0.7, "N = 130: N x N GEMMs with K = N ragged over the 32-steps, dq = 9 of dp = 16", 1, 3),
    Case("n300_c8", 1, 300, 8, "sharp", 0.7, "N = 300: softmax rows longer than the 256 threads; 300 rows: splits 2, kc = 150", 2, 5),
    Case("splits16", 32, 64, 8, "uniform", 0.7, "2048 rows: splits 16 of 128 rows, each across two images", 16, 1),
    Case("splits32", 16, 256, 136, "uniform", 0.7, "4096 rows: splits 32; 557056 elements: the residual kernel's 2048 and the "
         "dout kernel's 512 workgroups each walk more than one stride; dq = 17 of dp = 24", 32, 4),
    Case("gamma0", 3, 65, 64, "sharp", 0.0, "gamma = 0, the block's initial value", 1, 2),
    Case("wq0", 1, 64, 40, "wq0", 0.7, "Wq = bq = 0: every logit of a row is equal, P is the rounding of 1 / N", 1, 1),
    Case("integers", 1, 65, 24, "int", 0.7, "integer x and weights: stages 1 and 2 are exact", 1, 2),
]
BY_NAME = {c.name: c for c in CASES}
_BUILT = {}


def build(name):
    """the inputs of a case (cached, never modified): x, dout bf16 [B, N, C], params fp32, plan"""
    if name in _BUILT:
        return _BUILT[name]
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    dq, rn = c.C // 8, lambda *s: torch.randn(*s, generator=g)
    if c.regime == "int":
        ri = lambda m, *s: torch.randint(-m, m + 1, s, generator=g).to(torch.float32)
        x = ri(3, c.B, c.N, c.C).to(torch.bfloat16)
        params = {"wq": ri(8, dq, c.C), "bq": ri(8, dq), "wk": ri(8, dq, c.C), "bk": ri(8, dq), "wv": ri(2, c.C, c.C),
                  "bv": ri(2, c.C)}
    else:
        x = rn(c.B, c.N, c.C).to(torch.bfloat16)
        params = {"wq": rn(dq, c.C) * 0.08, "bq": rn(dq) * 0.1, "wk": rn(dq, c.C) * 0.08, "bk": rn(dq) * 0.1,
                  "wv": rn(c.C, c.C) * 0.05, "bv": rn(c.C) * 0.1}
    if c.regime == "wq0":
        params["wq"], params["bq"] = torch.zeros(dq, c.C), torch.zeros(dq)
    if c.regime in ("sharp", "uniform"):      # logits spread over +-30, or over +-1 (no probability above e^2 / N)
        xd = x.double()
        S = (xd @ params["wq"].double().t() + params["bq"].double()) @ (xd @ params["wk"].double().t()
                                                                          + params["bk"].double()).transpose(1, 2)
        f = float(((30.0 if c.regime == "sharp" else 1.0) / S.abs().max()).sqrt())
        for k in ("wq", "bq", "wk", "bk"):
            params[k] = params[k] * f
    params["gamma"] = torch.tensor([c.gamma])
    dout = rn(c.B, c.N, c.C).to(torch.bfloat16)
    _BUILT[name] = SimpleNamespace(case=c, x=x, dout=dout, params=params, plan=plan(c.B, c.N, c.C))
    return _BUILT[name]


def run_gpu(ops, inp, dev):
    """forward, read the scratch, backward into pre-filled gradients, read again -> (st, out of an inference pass, bytes
    changed outside the documented set after forward / after backward)"""
    p = inp.plan
    pd = {k: v.to(dev) for k, v in inp.params.items()}
    gd = {k: torch.full_like(v, PREFILL) for k, v in pd.items()}
    xd = inp.x.to(dev)
    with poisoned_scratch():
        out, saved = ops.attn_forward(xd, pd)
        out_inf, none = ops.attn_forward(xd, pd, need_backward=False)
    assert none is None
    wf = saved[1].cpu()
    dx = ops.attn_backward(saved, inp.dout.to(dev), pd, gd)
    wb = saved[1].cpu()
    st = extract(wf, wb, p)
    st.update(out=out.cpu(), dx=dx.cpu(), **{"g_" + k: v.cpu() for k, v in gd.items()})
    lost = (untouched(wf, p, False), untouched(wb, p, True))
    fwd_kept = all(torch.equal(view(wf, p, n).view(torch.int16), view(wb, p, n).view(torch.int16))
                   for n in ("qk", "qkv", "O", "P"))
    return st, out_inf.cpu(), lost, fwd_kept
