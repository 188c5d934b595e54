"""float64 statement of csrc/prelu.hip (InstanceNorm3d -> [+res] -> PReLU(C) -> [+res] on channel slices, its backward, and
gs_add_views / gs_repeat_backward / gs_slice_stats), the table of cases that reaches every branch of its launch plan, and the
per-element acceptance criterion (tests/test_pnorm_edges_cpu.py, tests/test_pnorm_edges_gpu.py).

The functions follow the header of prelu.hip and include/ganslate_hip.h, not the kernels' code: one pass over whole
float64 tensors, sums by torch.sum in float64. mean / rstd are INPUTS (the fp32 numbers given, cast to double).

Criterion (bf16 outputs), for every element with float64 reference r:   |got - r| <= 2^-8 |r| + K 2^-24 T
  2^-8 |r| covers half a bf16 ulp (pack_bf2 rounds to nearest even); T is the sum of the absolute values of the terms that
  form the element, so K counts fp32 roundings of those terms.
fp32 outputs (dslope, bias_grad, slice mean / rstd):                   |got - prefill - ref| <= K2 2^-24 sum|terms|
K and K2 are set in tests/test_pnorm_edges_gpu.py from a measurement; here they are arguments.
"""
from dataclasses import dataclass, field
from functools import lru_cache

import torch

U24 = 2.0 ** -24
HALF_BF16 = 2.0 ** -8
K_CAP, K2_CAP = 2 ** 10, 2 ** 9
DSLOPE_PREFILL, BIAS_PREFILL = 0.5, -0.25
DETUNE_MU, DETUNE_RSTD = 0.05, 1.1
EPS = 1e-5


# ---- the operation in float64 ------------------------------------------------------------------------------------------
def view(t, co, C):
    """channels [co, co + C) of an N...C buffer as float64 [N, pixels, C]"""
    return t[..., co:co + C].double().reshape(t.shape[0], -1, C)


def res_view(res, co, C, res_mod):
    """the residual a channel reads: channel c of the slice, or channel c % res_mod of it (x.repeat)"""
    if res_mod > 0:
        return res[..., co + torch.arange(C) % res_mod].double().reshape(res.shape[0], -1, C)
    return view(res, co, C)


def split_stats(mean_rstd, N, C):
    mr = mean_rstd.double().view(N, 2, C)
    return mr[:, 0, None, :], mr[:, 1, None, :]


@dataclass
class Fwd:
    yh: torch.Tensor          # normalised y (or y)
    u: torch.Tensor           # pre-activation
    res: torch.Tensor
    out: torch.Tensor
    T: torch.Tensor           # sum of the absolute terms of each element of out
    ambiguous: int            # elements whose sign of u fp32 and float64 may decide differently


def forward(y, mean_rstd, *, C, slope=None, res=None, res_mode=0, res_mod=0, y_co=0, res_co=0):
    yv = view(y, y_co, C)
    N = yv.shape[0]
    if mean_rstd is not None:
        mu, rstd = split_stats(mean_rstd, N, C)
        yh = (yv - mu) * rstd
    else:
        yh = yv
    r = res_view(res, res_co, C, res_mod) if res_mode else None
    u = yh + r if res_mode == 1 else yh
    if slope is not None:
        sl = slope.double()[:C]
        v = torch.where(u > 0, u, sl * u)
        s = torch.where(u > 0, torch.ones_like(u), sl.abs().expand_as(u))
    else:
        v, s = u, torch.ones_like(u)
    if res_mode == 1:
        T = s * (yh.abs() + r.abs())
    elif res_mode in (2, 3):
        T = s * yh.abs() + r.abs()
    else:
        T = s * yh.abs()
    out = v + r if res_mode == 2 else r - v if res_mode == 3 else v
    amb = 0
    if mean_rstd is not None and res_mode == 1:
        amb = int((u.abs() <= 2.0 ** -18 * (yh.abs() + r.abs())).sum())
    return Fwd(yh, u, r, out, T, amb)


@dataclass
class Bwd:
    gu: torch.Tensor          # = gres
    T_gu: torch.Tensor
    dy: torch.Tensor
    T_dy: torch.Tensor
    dslope: torch.Tensor      # [C] sum over the images of S4 (None without a slope)
    dslope_terms: torch.Tensor
    bias: torch.Tensor        # [C] sum over the images of -rstd S2 S3 / hw (None without a norm)
    bias_terms: torch.Tensor
    sums: dict = field(default_factory=dict)


def backward(g, y, mean_rstd, *, C, slope=None, g2=None, res=None, res_mode=0, res_mod=0, g_co=0, g2_co=0, y_co=0,
             res_co=0):
    f = forward(y, mean_rstd, C=C, slope=slope, res=res, res_mode=res_mode, res_mod=res_mod, y_co=y_co, res_co=res_co)
    yh, u = f.yh, f.u
    N, hw = yh.shape[0], yh.shape[1]
    gt = view(g, g_co, C)
    if g2 is not None:
        gt = gt + view(g2, g2_co, C)
    if res_mode == 3:
        gt = -gt
    dslope = dslope_terms = None
    if slope is not None:
        sl = slope.double()[:C]
        gu = torch.where(u > 0, gt, sl * gt)
        neg = u <= 0
        dslope = torch.where(neg, gt * u, torch.zeros_like(u)).sum((0, 1))
        # the summand gt*u is gt*yhat (+ gt*res in mode 1): its absolute summands
        mag = yh.abs() + f.res.abs() if res_mode == 1 else yh.abs()
        dslope_terms = torch.where(neg, gt.abs() * mag, torch.zeros_like(u)).sum((0, 1))
    else:
        gu = gt
    T_gu = gu.abs()
    if mean_rstd is None:
        return Bwd(gu, T_gu, gu, T_gu, dslope, dslope_terms, None, None)
    _, rstd = split_stats(mean_rstd, N, C)
    S1, A1 = gu.sum(1, keepdim=True), gu.abs().sum(1, keepdim=True)
    S2, A2 = (gu * yh).sum(1, keepdim=True), (gu * yh).abs().sum(1, keepdim=True)
    S3, A3 = yh.sum(1, keepdim=True), yh.abs().sum(1, keepdim=True)
    dy = rstd * (gu - S1 / hw - yh * S2 / hw)
    T_dy = rstd * (gu.abs() + A1 / hw + yh.abs() * A2 / hw)
    bias = (-rstd * S2 * S3 / hw).sum((0, 1))
    # d(S2 S3) <= |S3| dS2 + |S2| dS3 with dS2 <= k u A2, dS3 <= k u A3; the product's own roundings are relative to |S2 S3|
    bias_terms = (rstd / hw * (S3.abs() * A2 + S2.abs() * A3 + (S2 * S3).abs())).sum((0, 1))
    return Bwd(gu, T_gu, dy, T_dy, dslope, dslope_terms, bias, bias_terms,
               dict(S1=S1, S2=S2, S3=S3, A1=A1, A2=A2, A3=A3))


def add_views(dst, src, C, dst_co=0, src_co=0, accumulate=True):
    """-> (float64 value of dst's slice, T)"""
    s = view(src, src_co, C)
    if not accumulate:
        return s, s.abs()
    d = view(dst, dst_co, C)
    return s + d, s.abs() + d.abs()


def repeat_backward(g, g_img, C, g_co=0):
    """g_img [N, Cin, ...] + sum over c = c0 (mod Cin) of g's slice -> float64 [N, Cin, pixels]"""
    N, Cin = g_img.shape[0], g_img.shape[1]
    gv = view(g, g_co, C)
    add = torch.stack([gv[..., c0::Cin].sum(-1) for c0 in range(Cin)], 1)
    return g_img.double().reshape(N, Cin, -1) + add


def slice_stats(x, co, C, eps=EPS):
    """-> mean, rstd = 1 / sqrt(var + eps) [N, C] from float64 sums, and the sums of absolute summands behind their bounds:
    mean_terms = sum|x| / hw;  rstd_rel_terms = (sum x^2 / hw + 2 |mean| sum|x| / hw) / (2 (var + eps)), the first-order
    propagation of an error of k u (those terms) in var = E x^2 - mean^2 through (var + eps)^-1/2, relative to rstd"""
    v = view(x, co, C)
    hw = v.shape[1]
    mean = v.sum(1) / hw
    ex2 = (v * v).sum(1) / hw
    var = (ex2 - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    mean_terms = v.abs().sum(1) / hw
    rstd_rel_terms = (ex2 + 2 * mean.abs() * mean_terms) / (2 * (var + eps))
    return mean, rstd, mean_terms, rstd_rel_terms


# ---- the criterion -----------------------------------------------------------------------------------------------------
def bf16_excess(got, r, T):
    """per element (|got - r| - 2^-8 |r|) / (2^-24 T): the number of fp32 roundings of T the element needs beyond its own
    bf16 rounding. An element with T == 0 must be exact."""
    err = (got.double() - r).abs() - HALF_BF16 * r.abs()
    ex = err / (U24 * T)
    ex = torch.where(T > 0, ex, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return torch.nan_to_num(ex, nan=float("inf"))


def f32_excess(got, ref, terms):
    err = (got.double() - ref).abs()
    ex = err / (U24 * terms)
    ex = torch.where(terms > 0, ex, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return torch.nan_to_num(ex, nan=float("inf"))


def worst(ex):
    return float(ex.max())


# ---- the case table ----------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    N: int
    sp: tuple
    C: int
    res_mode: int
    res_mod: int
    norm: bool
    slope: bool
    g2: bool
    gres: bool
    dslope: bool
    bias_grad: bool
    chunks: int               # ceil(voxels / pn_pix_per_block): 2, 6, 275 or 526
    reaches: str
    seed: int = 0
    pad: int = 8              # every buffer is C + 2 * pad (+ 8 for some) channels wide, the slice starts at pad or 2 * pad

    @property
    def voxels(self):
        return self.sp[0] * self.sp[1] * self.sp[2]

    @property
    def widths(self):
        """channel stride and offset of every operand: slices at non-zero offsets of wider buffers, no two alike"""
        C, p = self.C, self.pad
        w = dict(y=(C + 2 * p, p), out=(C + p, p), g=(C + 3 * p, 2 * p), g2=(C + 2 * p, p), dy=(C + 2 * p, 2 * p),
                 gres=(C + p, p), res=(C + 3 * p, p))
        if self.res_mod:
            w["res"] = (16, 5)                # the image buffer of InputBlock: res_mod channels at an odd offset
        return w


def _c(name, N, sp, C, use, chunks, reaches, *, res_mod=0, slope=True, g2=True, gres=None, dslope=None, bias_grad=None,
       seed=0):
    mode, norm = {"input": (1, True), "conv": (0, True), "coupling": (2, True), "inverse": (3, True),
                  "tail": (1, False), "prelu": (0, False)}[use]
    gres = (use in ("input", "tail")) if gres is None else gres          # the residual's gradient, where there is one
    dslope = slope if dslope is None else dslope
    bias_grad = norm if bias_grad is None else bias_grad                 # the conv in front of the norm
    return Case(name, N, sp, C, mode, res_mod, norm, slope, g2, gres, dslope, bias_grad, chunks, reaches, seed)


CASES = [
    _c("a_input", 1, (3, 5, 7), 8, "input", 2, res_mod=1,
       reaches="reduce<1>; ragged last chunk (41 px); N=1: db and dslope inside the finalize kernel; InputBlock, repeat of 1"),
    _c("a_tail", 1, (3, 5, 7), 8, "tail", 2,
       reaches="block tail (no norm, mode 1) at N=1: dslope inside the finalize kernel without statistics"),
    _c("b_conv", 2, (6, 7, 9), 32, "conv", 6, g2=False,
       reaches="reduce<4>; N>1: parameter gradients by gs_launch_norm_param_grads; down/up conv (mode 0), no g2"),
    _c("b_input", 2, (6, 7, 9), 32, "input", 6, res_mod=2,
       reaches="InputBlock with a repeat of 2 at N>1; reduce<4>"),
    _c("c_coupling", 1, (6, 7, 9), 24, "coupling", 6,
       reaches="C8=3: e / C8 path with per-element channel numbers; reduce<2> with an idle column in the last z-block"),
    _c("c_inverse", 3, (6, 7, 9), 24, "inverse", 6,
       reaches="C8=3 at N=3; mode 3 forward (res - v) and backward (negated gradient)"),
    _c("c_prelu", 3, (6, 7, 9), 24, "prelu", 6, g2=False,
       reaches="no norm, no residual: pure PReLU, bit-exact forward; reduce for dslope alone"),
    _c("d_conv", 2, (5, 5, 5), 256, "conv", 2, slope=False,
       reaches="reduce<32>; finalize<16> with C >= 128; slope=None"),
    _c("e_coupling", 1, (5, 5, 5), 320, "coupling", 2, gres=True,
       reaches="C8=40: reduce<32> ragged and non-power-of-two; gres next to a norm"),
    _c("e_tail", 1, (5, 5, 5), 320, "tail", 2, dslope=False, gres=False,
       reaches="no norm and dslope=None: no scratch, reduce and finalize skipped; gres=None; C8=40 apply without sums"),
    _c("f_conv", 1, (26, 26, 26), 64, "conv", 275, g2=False,
       reaches="chunks=275: finalize<4>, unrolled sweep plus tail"),
    _c("g_coupling", 1, (26, 26, 26), 128, "coupling", 275,
       reaches="chunks=275: finalize<16>, unrolled sweep plus tail"),
    _c("h_conv", 1, (40, 41, 41), 64, "conv", 526,
       reaches="ppb=128, chunks=526; forward (> 524288 elements) and apply wrap their grids on the fixed-group path"),
    _c("i_inverse", 1, (40, 41, 41), 96, "inverse", 526, g2=False,
       reaches="C8=12: reduce<8> ragged; finalize<4>; forward and apply wrap on the non-power-of-two path"),
]
CASE_BY_NAME = {c.name: c for c in CASES}
STATS = ("exact", "detuned")
CASE_RUNS = [(c.name, s) for c in CASES for s in (STATS if c.norm else ("none",))]
SMALL = [c.name for c in CASES if c.voxels <= 378]


@dataclass
class Built:
    case: Case
    stats: str
    y: torch.Tensor
    res: torch.Tensor
    g: torch.Tensor
    g2: torch.Tensor
    slope: torch.Tensor
    mean_rstd: torch.Tensor
    out0: torch.Tensor        # pre-fills of the output buffers
    dy0: torch.Tensor
    gres0: torch.Tensor
    fwd: Fwd
    bwd: Bwd

    def fwd_kw(self, to=lambda t: t):
        c, w = self.case, self.case.widths
        return dict(C=c.C, slope=to(self.slope) if c.slope else None, res=to(self.res) if c.res_mode else None,
                    res_mode=c.res_mode, res_mod=c.res_mod, y_co=w["y"][1], res_co=w["res"][1] if c.res_mode else 0)

    def bwd_kw(self, to=lambda t: t):
        c, w = self.case, self.case.widths
        kw = self.fwd_kw(to)
        kw.update(g_co=w["g"][1], g2=to(self.g2) if c.g2 else None, g2_co=w["g2"][1] if c.g2 else 0)
        return kw


def exact_stats(y, co, C):
    mean, rstd, _, _ = slice_stats(y, co, C)
    return torch.stack([mean, rstd], 1).float()                # [N, 2, C]


@lru_cache(maxsize=3)
def build(name, stats):
    """inputs (bf16 / fp32, on the CPU) and the float64 reference of one run of the table, built once and shared"""
    c = CASE_BY_NAME[name]
    w = c.widths
    gen = torch.Generator().manual_seed(1000 + 17 * CASES.index(c) + c.seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    buf = lambda key, scale=1.0, shift=0.0: (rnd(c.N, *c.sp, w[key][0]) * scale + shift).to(torch.bfloat16)
    y = buf("y", 2.0, 0.3)
    res = buf("res") if c.res_mode else None
    g, g2 = buf("g"), (buf("g2") if c.g2 else None)
    slope = rnd(c.C) * 0.3 if c.slope else None
    out0, dy0, gres0 = buf("out", 3.0), buf("dy", 3.0), (buf("gres", 3.0) if c.gres else None)
    mr = None
    if c.norm:
        mr = exact_stats(y, w["y"][1], c.C)
        if stats == "detuned":
            mr[:, 0] += DETUNE_MU
            mr[:, 1] *= DETUNE_RSTD
        mr = mr.reshape(-1).contiguous()
    b = Built(c, stats, y, res, g, g2, slope, mr, out0, dy0, gres0, None, None)
    b.fwd = forward(y, mr, **b.fwd_kw())
    b.bwd = backward(g, y, mr, **b.bwd_kw())
    return b


def run_ops(ops, b, dev="cpu"):
    """forward and backward of one run through an ops object (RefOps or HipOps) on pre-filled buffers -> outputs on the CPU"""
    c, w = b.case, b.case.widths
    to = lambda t: t.to(dev)
    y, mr = to(b.y), (to(b.mean_rstd) if c.norm else None)
    out = to(b.out0.clone())
    ops.pnorm_forward(y, mr, out, out_co=w["out"][1], **b.fwd_kw(to))
    dy = to(b.dy0.clone())
    gres = to(b.gres0.clone()) if c.gres else None
    dslope = torch.full((c.C,), DSLOPE_PREFILL, device=dev) if c.dslope else None
    bias = torch.full((c.C,), BIAS_PREFILL, device=dev) if c.bias_grad else None
    ops.pnorm_backward(to(b.g), y, mr, dy, dslope=dslope, gres=gres, bias_grad=bias, dy_co=w["dy"][1],
                       gres_co=w["gres"][1] if c.gres else 0, **b.bwd_kw(to))
    cpu = lambda t: None if t is None else t.cpu()
    return dict(out=cpu(out), dy=cpu(dy), gres=cpu(gres), dslope=cpu(dslope), bias=cpu(bias))


def outside_untouched(buf, buf0, co, C):
    """everything outside channels [co, co + C) is bit-identical to the pre-fill"""
    keep = torch.ones(buf.shape[-1], dtype=torch.bool)
    keep[co:co + C] = False
    return torch.equal(buf[..., keep].view(torch.int16), buf0[..., keep].view(torch.int16))


def measure(b, got, bias_terms=None):
    """the worst excess of every output of one run: {"out" | "dy" | "gres": K-scale, "dslope" | "bias": K2-scale}, and the
    list of buffers whose surroundings changed. bias_terms: the absolute summands of a bias gradient that was not formed as
    the product -rstd S2 S3 / hw"""
    c, w = b.case, b.case.widths
    shape = (c.N, c.voxels, c.C)
    m, touched = {}, []
    for key, r, T, buf0 in (("out", b.fwd.out, b.fwd.T, b.out0), ("dy", b.bwd.dy, b.bwd.T_dy, b.dy0),
                            ("gres", b.bwd.gu, b.bwd.T_gu, b.gres0)):
        if got[key] is None:
            continue
        co = w[key][1]
        m[key] = worst(bf16_excess(got[key][..., co:co + c.C].reshape(shape), r, T))
        if not outside_untouched(got[key], buf0, co, c.C):
            touched.append(key)
    if c.dslope:
        m["dslope"] = worst(f32_excess(got["dslope"].double() - DSLOPE_PREFILL, b.bwd.dslope, b.bwd.dslope_terms))
    if c.bias_grad:
        terms = b.bwd.bias_terms if bias_terms is None else bias_terms
        m["bias"] = worst(f32_excess(got["bias"].double() - BIAS_PREFILL, b.bwd.bias, terms))
    return m, touched


# ---- the three small kernels -------------------------------------------------------------------------------------------
ADD_VIEWS_CASES = [          # (voxels as a shape, C, dst width / offset, src width / offset, accumulate)
    ((3, 5, 7), 8, (24, 8), (16, 8), True),
    ((3, 5, 7), 8, (24, 16), (16, 0), False),
    ((6, 7, 9), 128, (144, 16), (136, 8), True),
    ((40, 41, 41), 128, (136, 8), (136, 0), True),           # 67240 * 16 elements: the 4096-workgroup loop wraps
    ((40, 41, 41), 128, (136, 0), (136, 8), False),
]
REPEAT_CASES = [             # (N, shape, Cin, C, g width / offset)
    (2, (3, 5, 7), 1, 16, (32, 8)),
    (1, (6, 7, 9), 2, 16, (24, 8)),
    (2, (6, 7, 9), 3, 24, (40, 16)),
]
SLICE_STATS_CASES = [        # (N, shape, C, width / offset): 105 voxels are one slot, 378 two, 17576 sixty-nine
    (1, (3, 5, 7), 8, (24, 8)),
    (2, (6, 7, 9), 8, (16, 8)),
    (2, (3, 5, 7), 32, (48, 8)),
    (1, (6, 7, 9), 32, (40, 8)),
    (2, (6, 7, 9), 96, (112, 16)),
    (1, (26, 26, 26), 96, (104, 8)),
]


def small_inputs(kind, i):
    gen = torch.Generator().manual_seed(7000 + 100 * ("add", "repeat", "stats").index(kind) + i)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    if kind == "add":
        sp, C, (dcs, dco), (scs, sco), acc = ADD_VIEWS_CASES[i]
        return rnd(1, *sp, dcs).to(torch.bfloat16), rnd(1, *sp, scs).to(torch.bfloat16)
    if kind == "repeat":
        N, sp, Cin, C, (cs, co) = REPEAT_CASES[i]
        return rnd(N, *sp, cs).to(torch.bfloat16), rnd(N, Cin, *sp)
    N, sp, C, (cs, co) = SLICE_STATS_CASES[i]
    return ((rnd(N, *sp, cs) * 1.7 + 0.4).to(torch.bfloat16),)


def add_views_fp32(dst, src, C, dst_co, src_co, accumulate):
    """the kernel's arithmetic with torch on the CPU: fp32 add, round to nearest even"""
    v = src[..., src_co:src_co + C].float()
    if accumulate:
        v = v + dst[..., dst_co:dst_co + C].float()
    out = dst.clone()
    out[..., dst_co:dst_co + C] = v.to(torch.bfloat16)
    return out


def repeat_backward_fp32(g, g_img, C, g_co):
    """the kernel's documented order: per pixel and image channel c0, s = 0; s += g[c] for c = c0, c0 + Cin, ...; g_img += s"""
    N, Cin = g_img.shape[0], g_img.shape[1]
    gv = g[..., g_co:g_co + C].float()
    out = g_img.clone()
    for c0 in range(Cin):
        s = torch.zeros(gv.shape[:-1])
        for c in range(c0, C, Cin):
            s = s + gv[..., c]
        out[:, c0] += s
    return out
