"""Float64 reference of csrc/patchnce.hip (CUT's patch MLP and PatchNCE loss), one function per stage, for
tests/test_nce_stages_{cpu,gpu}.py. Same construction as tests/attn_ref.py (which states the criterion and holds the shared
helpers): every stage is one float64 function of the bits the kernels stored as that stage's input in the scratch tensor that
HipOps hands back, `plan()` mirrors the scratch layout and the launch plan of fill(), and a stage returns {name: (r, T)} or
{name: (r, T, extra)}.

Stages, per level (R = batch x patches rows, nc = 256):
  1  h = bf16(relu(bf16(X) bf16(W1)^T + b1))                                   q side only: the k side stores no h
  2  F = h bf16(W2)^T + b2, n = ||F||, fhat = F / (n + 1e-7) from the stored h  (fp32)
  3  loss from the stored fhat of both sides: S = Qh Kh^T + Qh Kl^T + Ql Kh^T per image, row logits [S_ii, S_i. with the
     diagonal at -10] / T, columns >= P excluded, cross-entropy against entry 0, partial sums per 64-row tile, times coef
  4  df = bf16((dQ - fhat (fhat . dQ) (n + eps) / n) / (n + eps)),  dQ = bf16(G coef / T) bf16(Khat),
     G = softmax without the positive entry, G_ii = p_pos - 1
  5  dh = bf16(relu'(h) o (bf16(df grad_scale) bf16(W2)))
  6  dxq = dh bf16(W1)                                                         (fp32)
  7  dW2 += bf16(df gs)^T h, db2 += sum bf16(df gs), dW1 += dh^T bf16(X), db1 += sum dh

Stage 4 is the one stage with a rounding that is never stored: g = G coef / T goes to bf16 between the soft-max and the
product with Khat. The reference keeps g unrounded; a bf16 rounding moves every term g_j Khat_jc of dQ_c by at most
2^-8 |g_j Khat_jc| (half an ulp is 2^-9; the other half covers an fp32 g that rounds to the neighbour), so dQ_c by at most
E_c = 2^-8 T_dQ_c with T_dQ = |g| |Khat|. df is linear in dQ: df_c = (dQ_c - fhat_c sum_e fhat_e dQ_e (n + eps) / n) / (n + eps),
so by the triangle inequality it moves by at most (E_c + |fhat_c| sum_e |fhat_e| E_e (n + eps) / n) / (n + eps) — which is 2^-8
times the T of df itself, since T is the same expression in T_dQ. That is the `extra` of stage 4.
"""
import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import torch

from tests.attn_ref import (EMU_CAP, HALF_BF16, K2_CAP, K_CAP, POISON, PREFILL, bf, bf16_excess, f32_excess, ident,  # noqa: F401
                            poisoned_scratch, rup, split, worst)

NC, TM, RSPLIT_MAX = 256, 64, 8
LAMBDA = 1.0
f32 = lambda v: torch.tensor(v, dtype=torch.float32)
EPS32 = float(f32(1e-7))


# ---- the scratch layout and launch plan (patchnce.hip: fill(), gs_patchnce_work_bytes) -------------------------------------
def plan(L, B, P):
    p = SimpleNamespace(L=L, B=B, P=P, R=B * P, tiles=(P + TM - 1) // TM, views={})
    o = 0

    def take(name, dtype, shape, pad=1):
        nonlocal o
        n = torch.empty((), dtype=dtype).element_size()
        for s in shape:
            n *= s
        p.views[name] = (dtype, shape, o)
        o += rup(n, pad)
    take("fhat", torch.float32, (2, L, p.R, NC))
    take("norms", torch.float32, (L, p.R))
    take("h", torch.bfloat16, (L, p.R, NC))
    take("df", torch.bfloat16, (L, p.R, NC))
    take("dh", torch.bfloat16, (L, p.R, NC))
    take("loss_part", torch.float32, (L, B, p.tiles), pad=256)
    p.chunks = (p.R + 63) // 64
    p.rsplit = min(RSPLIT_MAX, RSPLIT_MAX if p.chunks >= 16 else p.chunks // 2 if p.chunks >= 4 else 1)
    p.per = (p.chunks + p.rsplit - 1) // p.rsplit
    p.ranges = [(s * p.per * 64, min(p.R, (s + 1) * p.per * 64)) for s in range(p.rsplit)]
    p.empty = sum(1 for a, b in p.ranges if a >= b)
    p.wstride = NC * NC + NC
    take("wpart", torch.float32, (L, 2, RSPLIT_MAX, p.wstride))
    p.end = o + 256
    return p


def view(work, p, name):
    dtype, shape, off = p.views[name]
    n = torch.empty((), dtype=dtype).element_size()
    for s in shape:
        n *= s
    return work[off:off + n].view(dtype).reshape(shape)


def untouched(work, p, backward, channels):
    """-> bytes outside what a forward (and a backward) documents as written that lost their pre-fill. channels: C of every
    level of the launch group. Of the row-split partial sums [level][which][rsplit][nc x 256 + nc] a backward writes, for
    every range (an empty one: zeros), all of which = 0 (dW2, db2) and of which = 1 the columns n < C of every row of the
    nc x 256 image plus the nc bias sums (dW1, db1); nothing with rsplit = 1."""
    assert work.numel() == p.end and len(channels) == p.L
    m = torch.zeros(p.end, dtype=torch.bool)
    for name in ["fhat", "norms", "h", "df", "loss_part"] + (["dh"] if backward else []):
        dtype, shape, off = p.views[name]
        n = torch.empty((), dtype=dtype).element_size()
        for s in shape:
            n *= s
        m[off:off + n] = True
    if backward and p.rsplit > 1:
        off = p.views["wpart"][2]
        w = m[off:off + p.L * 2 * p.rsplit * p.wstride * 4].view(p.L, 2, p.rsplit, p.wstride, 4)
        w[:, 0] = True
        w[:, 1, :, NC * NC:] = True
        for l, ch in enumerate(channels):
            w[l, 1, :, :NC * NC].view(p.rsplit, NC, NC, 4)[:, :, :ch] = True
    return int((work[~m] != POISON).sum())


# ---- the stages (one level) ---------------------------------------------------------------------------------------------------
def mm(a, b):
    return a @ b, a.abs() @ b.abs()


def consts(lv, rb):
    """(1 / T, coef, eps): exact under ident, the kernel's fp32 values otherwise"""
    if rb is ident:
        return 1.0 / lv.T, lv.lam_exact / (lv.L * lv.R), 1e-7
    return float(f32(1.0) / f32(lv.T)), float(f32(lv.lam) / (f32(float(lv.L)) * f32(float(lv.R)))), EPS32


def s1_h(lv, st, rb, x=None):
    x = rb(lv.xq if x is None else x)
    r, T = mm(x, rb(lv.W1).t())
    b = lv.b1.double()
    return {"h": (torch.relu(r + b), T + b.abs())}


def s2_fhat(lv, st, rb, h=None):
    h = (st["h"] if h is None else h).double()
    F, TF = mm(h, rb(lv.W2).t())
    F, TF = F + lv.b2.double(), TF + lv.b2.double().abs()
    eps = consts(lv, rb)[2]
    n = F.pow(2).sum(1, keepdim=True).sqrt()
    Tn = (F.abs() * TF).sum(1, keepdim=True) / n.clamp_min(1e-300) + n
    fh = F / (n + eps)
    return {"fq": (fh, TF / (n + eps) + fh.abs() * Tn / (n + eps) + fh.abs()), "norms": (n[:, 0], Tn[:, 0])}


def _logits(lv, st, rb):
    """row logits [pos, negatives with the diagonal at -10] / T of every image [B, P, 1 + P], the absolute terms of each"""
    inv_T = consts(lv, rb)[0]
    img = lambda t: t.reshape(lv.B, lv.P, NC)
    (qh, ql), (kh, kl) = split(img(st["fq"]), rb), split(img(st["fk"]), rb)
    t = lambda a: a.transpose(1, 2)
    S = qh @ t(kh) + qh @ t(kl) + ql @ t(kh)
    TS = qh.abs() @ t(kh.abs()) + qh.abs() @ t(kl.abs()) + ql.abs() @ t(kh.abs())
    eye = torch.eye(lv.P, dtype=torch.bool)[None]
    pos, Tpos = S.diagonal(dim1=1, dim2=2)[..., None], TS.diagonal(dim1=1, dim2=2)[..., None]
    lg = torch.cat([pos, S.masked_fill(eye, -10.0)], -1) * inv_T
    Tl = torch.cat([Tpos, TS.masked_fill(eye, 0.0)], -1) * inv_T + lg.abs()
    return lg, Tl


def s3_loss(lv, st, rb):
    lg, Tl = _logits(lv, st, rb)
    coef = consts(lv, rb)[1]
    m = lg.max(-1, keepdim=True).values
    lse = torch.logsumexp(lg, -1, keepdim=True)
    p = (lg - lse).exp()
    row = (lse - lg[..., :1])[..., 0]                                             # [B, P]
    Trow = ((lse - m).abs() + m.abs() + lg[..., :1].abs() + Tl[..., :1])[..., 0] + (p * (1 + (lg - m).abs() + Tl)).sum(-1)
    pad = lv.tiles * TM - lv.P
    tile = lambda t: torch.nn.functional.pad(t, (0, pad)).reshape(lv.B, lv.tiles, TM).sum(-1)
    part, Tpart = tile(row), tile(Trow + row.abs())
    return {"loss_part": (part, Tpart), "loss": (coef * part.sum().reshape(1), coef * Tpart.sum().reshape(1))}


def s4_df(lv, st, rb):
    lg, _ = _logits(lv, st, rb)
    inv_T, coef, eps = consts(lv, rb)
    p = torch.softmax(lg, -1)
    eye = torch.eye(lv.P, dtype=torch.bool)[None]
    G = torch.where(eye, p[..., :1] - 1.0, p[..., 1:]) * (inv_T * coef)
    K = rb(st["fk"]).reshape(lv.B, lv.P, NC)
    dQ, TdQ = mm(G, K)
    Q = st["fq"].double().reshape(lv.B, lv.P, NC)
    n = st["norms"].double().reshape(lv.B, lv.P, 1)
    ne, nn = n + eps, n.clamp_min(1e-30)
    r = (dQ - Q * ((Q * dQ).sum(-1, keepdim=True) * ne / nn)) / ne
    T = (TdQ + Q.abs() * ((Q.abs() * TdQ).sum(-1, keepdim=True) * ne / nn)) / ne
    return {"df": (r.reshape(lv.R, NC), T.reshape(lv.R, NC), HALF_BF16 * T.reshape(lv.R, NC))}


def scaled_df(lv, st, rb):
    """bf16(df grad_scale): one fp32 multiply, one rounding"""
    if rb is ident:
        return st["df"].double() * (1.0 if lv.gs is None else lv.gs)
    return (st["df"].float() * f32(1.0 if lv.gs is None else lv.gs)).to(torch.bfloat16).double()


def s5_dh(lv, st, rb):
    r, T = mm(scaled_df(lv, st, rb), rb(lv.W2))
    on = st["h"].double() > 0
    return {"dh": (torch.where(on, r, torch.zeros_like(r)), torch.where(on, T, torch.zeros_like(T)))}


def s6_dxq(lv, st, rb):
    return {"dxq": mm(st["dh"].double(), rb(lv.W1))}


def s7_params(lv, st, rb):
    d, dh, h, x = scaled_df(lv, st, rb), st["dh"].double(), st["h"].double(), rb(lv.xq)
    out = {}
    for k, (r, T) in (("g_W2", mm(d.t(), h)), ("g_b2", (d.sum(0), d.abs().sum(0))), ("g_W1", mm(dh.t(), x)),
                      ("g_b1", (dh.sum(0), dh.abs().sum(0)))):
        out[k] = (r, T + PREFILL)
    return out


STAGES = (("1 h", s1_h), ("2 fhat,norms", s2_fhat), ("3 loss", s3_loss), ("4 df", s4_df), ("5 dh", s5_dh), ("6 dxq", s6_dxq),
          ("7 dW,db", s7_params))
BF16_OUT = {"h", "df", "dh"}


def is_bf16_stage(name):
    return name.split()[0] in ("1", "4", "5")


def chain(lv):
    """all stages of one level in float64 with every rounding switched off (the k side: stages 1 and 2 on xk)"""
    st = {}
    st["fk"] = s2_fhat(lv, st, ident, h=s1_h(lv, st, ident, x=lv.xk)["h"][0])["fq"][0]
    for _, f in STAGES:
        st.update({k: v[0] for k, v in f(lv, st, ident).items()})
    return st


def measure(lv, st):
    """{stage: the largest excess of its outputs} of one level"""
    res = {}
    for name, f in STAGES:
        ex = 0.0
        for k, v in f(lv, st, bf).items():
            r, T = v[0], v[1]
            if k in BF16_OUT:
                assert st[k].dtype == torch.bfloat16, k
                e = bf16_excess(st[k], r, T, v[2] if len(v) > 2 else None)
            else:
                assert st[k].dtype == torch.float32, k
                e = f32_excess(st[k].double().reshape(r.shape) - (PREFILL if k.startswith("g_") else 0.0), r, T)
            ex = max(ex, worst(e))
        res[name] = ex
    return res


def emulate(lv, mutate=""):
    """one level in plain torch fp32 with the documented roundings. mutate: "lo_hi" leaves the lo hi product out of the logit
    GEMM, "diag" masks the diagonal with -9 — value errors of the size the criterion has to see (test_nce_stages_cpu.py)"""
    b16 = lambda t: t.to(torch.bfloat16)
    sp = lambda t: (b16(t).float(), b16(t - b16(t).float()).float())
    r16 = lambda t: b16(t).float()
    inv_T, coef = f32(1.0) / f32(lv.T), f32(lv.lam) / (f32(float(lv.L)) * f32(float(lv.R)))
    st, feats = {}, []
    for x in (lv.xq, lv.xk):
        h = b16(torch.relu(r16(x) @ r16(lv.W1).t() + lv.b1))
        F = h.float() @ r16(lv.W2).t() + lv.b2
        n = F.pow(2).sum(1, keepdim=True).sqrt()
        feats.append((h, F / (n + f32(1e-7)), n[:, 0]))
    st["h"], st["fq"], st["norms"] = feats[0]
    st["fk"] = feats[1][1]
    img = lambda t: t.reshape(lv.B, lv.P, NC)
    (qh, ql), (kh, kl) = sp(img(st["fq"])), sp(img(st["fk"]))
    t = lambda a: a.transpose(1, 2)
    S = (0.0 if mutate == "lo_hi" else ql @ t(kh)) + qh @ t(kl) + qh @ t(kh)
    eye = torch.eye(lv.P, dtype=torch.bool)[None]
    lg = torch.cat([S.diagonal(dim1=1, dim2=2)[..., None], S.masked_fill(eye, -9.0 if mutate == "diag" else -10.0)], -1) * inv_T
    lse = torch.logsumexp(lg, -1, keepdim=True)
    row = (lse - lg[..., :1])[..., 0]
    st["loss_part"] = torch.nn.functional.pad(row, (0, lv.tiles * TM - lv.P)).reshape(lv.B, lv.tiles, TM).sum(-1)
    st["loss"] = (st["loss_part"].sum() * coef).reshape(1)
    p = torch.softmax(lg, -1)
    G = r16(torch.where(eye, p[..., :1] - 1.0, p[..., 1:]) * inv_T * coef)
    dQ = G @ r16(img(st["fk"]))
    Q, n = img(st["fq"]), st["norms"].reshape(lv.B, lv.P, 1)
    ne = n + f32(1e-7)
    st["df"] = b16((dQ - Q * ((Q * dQ).sum(-1, keepdim=True) * ne / n.clamp_min(1e-30))) / ne).reshape(lv.R, NC)
    d = r16(st["df"].float() * f32(1.0 if lv.gs is None else lv.gs))
    st["dh"] = b16(torch.where(st["h"].float() > 0, d @ r16(lv.W2), torch.zeros(())))
    dh = st["dh"].float()
    st["dxq"] = dh @ r16(lv.W1)
    st["g_W2"], st["g_b2"] = PREFILL + d.t() @ st["h"].float(), PREFILL + d.sum(0)
    st["g_W1"], st["g_b1"] = PREFILL + dh.t() @ r16(lv.xq), PREFILL + dh.sum(0)
    return st


# ---- the cases --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    batch: int
    patches: object      # int, or a tuple: patches per level (one launch group per level)
    channels: tuple
    gs: object           # grad_scale: None | float
    keys: str            # corr (xk = xq + noise) | same | indep | int
    reaches: str
    rsplit: int          # asserted against the plan (of the first launch group)
    empty: int = 0       # empty row ranges of the parameter-gradient launch
    T: float = 0.07      # nce_T


CASES = [
    Case("p1_c1", 2, 1, (1,), None, "corr", "P = 1 (the only negative is the masked diagonal), C = 1, 1 chunk", 1),
    Case("p63", 2, 63, (3, 63), 0.37, "corr", "P = 63, C = 63: one short of a 64-column chunk; 2 chunks", 1),
    Case("p64_c64", 1, 64, (64,), 0.37, "corr", "P = 64, C = 64: full tiles, 1 chunk", 1),
    Case("p65_c65", 3, 65, (65,), None, "corr", "P = 65, C = 65: one past a tile / a chunk; 4 chunks: rsplit 2", 2),
    Case("chunks3_gs0", 3, 64, (256,), 0.0, "corr", "3 chunks: rsplit 1; C = 256; grad_scale = 0", 1),
    Case("chunks5", 5, 64, (3,), 0.37, "corr", "5 chunks: rsplit 2, last range short (3 + 2)", 2),
    Case("chunks7", 7, 64, (8,), None, "corr", "7 chunks: rsplit 3 (3 + 3 + 1)", 3),
    Case("chunks9", 9, 64, (3,), 0.37, "corr", "9 chunks: rsplit 4, the last range empty", 4, 1),
    Case("chunks15", 15, 64, (8,), 0.37, "corr", "15 chunks: rsplit 7, the last two ranges empty", 7, 2),
    Case("chunks16_p256", 4, 256, (3,), 0.37, "corr", "16 chunks: rsplit 8; P = 256", 8),
    Case("ragged_rows", 3, 100, (8, 64), 0.37, "corr", "R = 300, no multiple of 64: rsplit 2 with a ragged last chunk", 2),
    Case("levels8", 1, 64, (1, 3, 8, 63, 64, 65, 128, 256), 0.37, "corr", "8 levels in one launch group", 1),
    Case("per_level_patches", 2, (256, 64, 16), (3, 64, 256), 0.37, "corr",
         "a tuple of patch counts: one launch group per level, params[poff:], lambda / levels", 4),
    Case("same_keys", 2, 64, (8,), None, "same", "xk = xq: both sides bit-identical, positive logits at 1", 1),
    Case("integers", 1, 65, (3,), 0.37, "int", "integer X, W1, b1: h is exact", 1),
    # the two below make value errors visible that fp32 cannot show on the rows above: with correlated keys at T = 0.07 the
    # soft-max is saturated (a logit error moves the loss by p_neg ~ 1e-3 of itself) and exp(-10 / T) is 1e-62
    Case("indep_keys_p2", 3, 2, (8,), 0.37, "indep", "independent keys, 2 rows per tile: an unsaturated soft-max, undiluted", 1),
    Case("warm_T", 2, 64, (8,), 0.37, "corr", "nce_T = 4: the masked diagonal's constant carries weight in the soft-max", 1, 0, 4.0),
]
BY_NAME = {c.name: c for c in CASES}
_BUILT = {}


def level_params(params, channels):
    out, off = [], 0
    for c in channels:
        sizes = (NC * c, NC, NC * NC, NC)
        parts = []
        for n in sizes:
            parts.append(params[off:off + n])
            off += n
        out.append((parts[0].view(NC, c), parts[1], parts[2].view(NC, NC), parts[3]))
    return out


def build(name):
    """inputs of a case (cached, never modified): xq / xk per level, the flat params, and per level the record `lv` the
    stages take (its launch group's L, R, lambda and plan)"""
    if name in _BUILT:
        return _BUILT[name]
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    n_lv = len(c.channels)
    per_level = c.patches if isinstance(c.patches, tuple) else (c.patches,) * n_lv
    grouped = len(set(per_level)) == 1
    numel = sum(NC * ch + NC + NC * NC + NC for ch in c.channels)
    if c.keys == "int":
        ri = lambda m, *s: torch.randint(-m, m + 1, s, generator=g).to(torch.float32)
        xq = [ri(4, c.batch, p_, ch) for p_, ch in zip(per_level, c.channels)]
        xk = [ri(4, c.batch, p_, ch) for p_, ch in zip(per_level, c.channels)]
        params = torch.randn(numel, generator=g) * 0.05
        for W1, b1, _, _ in level_params(params, c.channels):
            W1.copy_(ri(4, *W1.shape))
            b1.copy_(ri(4, NC))
    else:
        xq = [torch.randn(c.batch, p_, ch, generator=g) for p_, ch in zip(per_level, c.channels)]
        noise = [torch.randn(q.shape, generator=g) for q in xq]
        xk = [q.clone() if c.keys == "same" else n_ if c.keys == "indep" else q + 0.5 * n_ for q, n_ in zip(xq, noise)]
        params = torch.randn(numel, generator=g) * 0.05
    levels = []
    for l, (W1, b1, W2, b2) in enumerate(level_params(params, c.channels)):
        L = n_lv if grouped else 1
        levels.append(SimpleNamespace(
            xq=xq[l].flatten(0, 1), xk=xk[l].flatten(0, 1), W1=W1, b1=b1, W2=W2, b2=b2, C=c.channels[l], B=c.batch,
            P=per_level[l], R=c.batch * per_level[l], L=L, lam=float(f32(LAMBDA if grouped else LAMBDA / n_lv)),
            lam_exact=LAMBDA if grouped else LAMBDA / n_lv, gs=c.gs, T=c.T, tiles=(per_level[l] + TM - 1) // TM, group=0 if grouped else l, index=l if grouped else 0,
            plan=plan(L, c.batch, per_level[l])))
    _BUILT[name] = SimpleNamespace(case=c, xq=xq, xk=xk, params=params, levels=levels, numel=numel)
    return _BUILT[name]


def grads_of_level(flat, channels, l):
    W1, b1, W2, b2 = level_params(flat, channels)[l]
    return {"g_W1": W1, "g_b1": b1, "g_W2": W2, "g_b2": b2}


def run_gpu(ops, inp, dev, swap=False):
    """forward on poisoned scratch, read it, backward into a pre-filled flat gradient, read again -> per level st, and the
    bytes changed outside the documented buffers after forward / backward (summed over the launch groups)"""
    c = inp.case
    q, k = [t.to(dev) for t in inp.xq], [t.to(dev) for t in inp.xk]
    if swap:
        q, k = k, q
    params = inp.params.to(dev)
    with poisoned_scratch():
        loss, saved = ops.patchnce_forward(q, k, params, batch=c.batch, nc=NC, nce_T=c.T, lambda_nce=LAMBDA)
    wf = [s[2].cpu() for s in saved]
    if swap:
        return [view(wf[lv.group], lv.plan, "fhat")[0, lv.index].clone() for lv in inp.levels]
    grads = torch.full((inp.numel,), PREFILL, dtype=torch.float32, device=dev)
    dxq = ops.patchnce_backward(saved, params, grads, grad_scale=None if c.gs is None else torch.tensor(c.gs, device=dev))
    wb = [s[2].cpu() for s in saved]
    grads, loss = grads.cpu(), loss.cpu()
    plans = {lv.group: lv.plan for lv in inp.levels}
    chans = {g: [lv.C for lv in inp.levels if lv.group == g] for g in plans}
    lost = (sum(untouched(wf[g], p, False, chans[g]) for g, p in plans.items()),
            sum(untouched(wb[g], p, True, chans[g]) for g, p in plans.items()))
    kept = all(torch.equal(view(wf[g], p, n).view(torch.int16), view(wb[g], p, n).view(torch.int16))
               for g, p in plans.items() for n in ("fhat", "norms", "h", "df", "loss_part"))
    sts = []
    for l, lv in enumerate(inp.levels):
        f, b, p, i = wf[lv.group], wb[lv.group], lv.plan, lv.index
        st = {"fq": view(f, p, "fhat")[0, i], "fk": view(f, p, "fhat")[1, i], "norms": view(f, p, "norms")[i],
              "h": view(f, p, "h")[i], "df": view(f, p, "df")[i], "loss_part": view(f, p, "loss_part")[i],
              "dh": view(b, p, "dh")[i], "loss": loss[l:l + 1], "dxq": dxq[l].cpu().flatten(0, 1)}
        st.update(grads_of_level(grads, c.channels, l))
        sts.append(st)
    return sts, lost, kept
