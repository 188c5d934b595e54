"""float64 statement of the kernels that carry every image into and out of every network: csrc/wfold.hip (the W-fold boundary
transforms of the k7 stem / last layer and their adjoints, row-staged and per-pixel), the to/from-activation and fold-adjoint
entry points of csrc/image.hip and the feature taps of csrc/taps.hip; the tables of cases that reach every branch of their
launch plans, the per-element criteria and the mutants (tests/test_boundary_edges_cpu.py, tests/test_boundary_edges_gpu.py).

Written from the headers of the three .hip files and include/ganslate_hip.h, not from the kernels' loops: unfold is F.pad along
W followed by Tensor.unfold, the pad adjoints are float64 autograd of F.pad (inorm_ref.fold for gs_image_to_act_backward), the
adjoints of unfold and shift-add are float64 autograd of the forward statement, each once more on |g| for T, the sum of the
absolute terms of every element. The image taps take their target pixels by sending an index image through the same F.pad.

Every output of a case is an `Out` of one kind; judge() applies the kind's criterion to every element:
  bits   pure moves and single roundings: the bits of the reference rounded to the output's type (float64 -> fp32 -> bf16,
         both to nearest even; for gs_tap_scatter_add this is the double rounding bf16(fp32(d + s)) of its header). The
         sequential fp32 sum of gs_image_tap_scatter (sample order, promised by its header) is stated in fp32 and is of this
         kind. zero_sign = False where the statement comes out of autograd, whose accumulation 0 + (-0) loses the sign of a
         zero the kernel moves: there +0 and -0 compare equal.
  sum    fp32 sums: |got - prefill - ref| <= K2 2^-24 (sum|terms| + |prefill|), the prefill only where the entry point
         accumulates. Every such case runs a second time on integer data (|v| <= 8: every partial sum exact) and must then
         equal the reference exactly, whatever the order.
  bf16   bf16 outputs with arithmetic (the tanh backward g (1 - o^2)): |got - r| <= 2^-8 |r| + K 2^-24 T, T = |g| (1 + o^2).
  tanh   forward tanh: the act-none run of the same input gives the kernel's own pre-activation s (itself judged as bits or
         sum); the tanh run is compared with float64 tanh(s) in fp32 ulps of that reference. The ulp has the absolute floor
         2^-149 (the spacing of subnormals: below 2^-126 an fp32 result cannot be closer). The allowance is set in
         tests/test_boundary_edges_gpu.py from a measurement and may not exceed TANH_CAP = 8.
Outputs are inorm_ref.guarded() views: NaN before a full write, random (integer on integer data) before an accumulation or a
scatter, and the guard elements must keep their pattern. N = 2 wherever a sample stride exists.

Inputs of the `bits` kind carry SPECIALS: bf16 ties of both parities, +-0, the largest fp32 that rounds to a finite bf16
(0x7F7F7FFF) and the first that rounds to inf (0x7F7F8000, a tie whose even neighbour is inf), each with both signs.

MUTANTS are deliberately wrong statements (refs(mut=...)): fake() rounds what they give to the output types as a kernel
would, and the criterion must reject each on at least one case.

The tables are products of the value sets where the product is small (unfold: 5 x 3 x 6), otherwise every value of every axis
with the remaining parameters dealt out cyclically. `reaches` names the branch tags a row claims; tags_of() derives a row's
tags from the restated dispatch conditions (the plan functions below), and the CPU test holds one against the other.
"""
import math
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from tests.inorm_ref import BF16, fold, guarded, guards_intact
from tests.pnorm_ref import bf16_excess, f32_excess, worst

F32 = torch.float32
KW, PW = 7, 3                      # k = 7, p = 3 throughout
WF_SEG = 256
TANH_CAP = 8
N = 2


# ---- rounding, bits, ulps ------------------------------------------------------------------------------------------------
def round_to(v, dtype, ties_away=False):
    """float64 -> fp32 (nearest even) -> dtype (nearest even; ties_away: the mutant's rounding half away from zero)"""
    f = v.float()
    if dtype == F32:
        return f
    if not ties_away:
        return f.to(BF16)
    u = ((f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF) + 0x8000) >> 16 & 0xFFFF
    return torch.where(u >= 32768, u - 65536, u).to(torch.int16).view(BF16)


def same_bits(a, b, zero_sign=True):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = torch.int16 if a.dtype == BF16 else torch.int32
    ai, bi = a.contiguous().view(it), b.contiguous().view(it)
    if not zero_sign:
        ai, bi = torch.where(a == 0, torch.zeros_like(ai), ai), torch.where(b == 0, torch.zeros_like(bi), bi)
    return torch.equal(ai, bi)


def ulp32(r):
    """the spacing of fp32 numbers at |r| (float64), floored at 2^-149"""
    _, e = torch.frexp(r.abs())
    e = torch.where(r == 0, torch.full_like(e, -200), e - 1).clamp_min(-126)
    return torch.ldexp(torch.ones_like(r), e - 23)


def _f32_bits(*words):
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32).view(F32)


# ties (low half 0x8000) above an even and an odd bf16, +-0, the last finite and the first inf rounding, both signs
SPECIALS = _f32_bits(0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x7F7F7FFF, 0x7F7F8000,
                     0xFF7F7FFF, 0xFF7F8000, 0x3F807FFF, 0x3F808001)


def rnd32(gen, *shape, specials=True):
    x = torch.randn(*shape, generator=gen) * 1.5
    if specials:
        f = x.view(-1)
        n = min(f.numel(), SPECIALS.numel())
        f[:n] = SPECIALS[:n]
        f[f.numel() - n:] = SPECIALS[:n].flip(0)
    return x


def rndbf(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF16)


def ints(gen, *shape, dtype=F32):
    return torch.randint(-8, 9, shape, generator=gen).to(dtype)


# ---- outputs and the criterion -------------------------------------------------------------------------------------------
@dataclass
class Out:
    kind: str                       # bits | sum | bf16 | tanh
    dtype: torch.dtype
    value: torch.Tensor             # float64, in the layout of the output buffer
    T: torch.Tensor = None
    prefill: torch.Tensor = None    # what an accumulating `sum` output holds before (bits outputs carry it in value)
    pre: str = None                 # tanh: the output that holds the kernel's pre-activation
    zero_sign: bool = True

    @property
    def shape(self):
        return tuple(self.value.shape)


def out_buffer(o, dev):
    """the guarded buffer an output is written into: NaN, or the prefill"""
    return guarded(o.shape, o.dtype, dev, o.prefill)


def judge(b, got):
    """-> dict(bits=, k=, k2=, tanh=, guards=, bad=[names]) over every element of every output of the built case"""
    m = dict(bits=True, k=0.0, k2=0.0, tanh=0.0, guards=bool(got["guards"]), bad=[])
    for name, o in b.ref.items():
        g, ok = got[name], True
        if tuple(g.shape) != o.shape or g.dtype != o.dtype:
            ok = False
        elif o.kind == "bits":
            ok = same_bits(g, round_to(o.value, o.dtype), o.zero_sign)
        elif o.kind == "sum":
            pf = o.prefill.double() if o.prefill is not None else torch.zeros_like(o.value)
            m["k2"] = max(m["k2"], worst(f32_excess(g.double() - pf, o.value, o.T + pf.abs())))
            if b.data == "int":
                ok = torch.equal(g.double(), o.value + pf)
        elif o.kind == "bf16":
            m["k"] = max(m["k"], worst(bf16_excess(g, o.value, o.T)))
        elif o.kind == "tanh":
            r = torch.tanh(got[o.pre].double())
            err = torch.nan_to_num((g.double() - r).abs() / ulp32(r), nan=float("inf"))
            m["tanh"] = max(m["tanh"], float(err.max()))
        if not ok:
            m["bits"] = False
            m["bad"].append(name)
    return m


def accept(m, K, K2, ulps):
    return m["guards"] and m["bits"] and m["k"] <= K and m["k2"] <= K2 and m["tanh"] <= ulps


def fake(b, mut):
    """what a kernel that computed the mutant statement would leave in the buffers"""
    got = dict(guards=True)
    for name, o in b.refs(mut).items():
        v = o.value + o.prefill.double() if o.kind == "sum" and o.prefill is not None else o.value
        got[name] = round_to(v, o.dtype, ties_away=mut == "ties_away")
    return got


MUTANTS = ["reflect_off_by_one", "replicate_as_reflect", "drop_last_tap", "halo_from_first_segment", "channel_order_c_dw",
           "ties_away", "colliders_reversed", "pad_lanes_nonzero", "bias_after_act"]


# ---- the operations in float64 -------------------------------------------------------------------------------------------
def pad_sp(x, pads, mode):
    """F.pad of the spatial axes of x [N, C, *sp] by pads = [(lo, hi)] per axis"""
    flat = [v for lo_hi in reversed(pads) for v in lo_hi]
    if not any(flat):
        return x
    return F.pad(x, flat) if mode == "zero" else F.pad(x, flat, mode=mode)


def pad_w(x, lo, hi, mode, mut=None):
    """F.pad along W; the mutants change the border rule"""
    W = x.shape[-1]
    zeros = [(0, 0)] * (x.dim() - 3)
    if mut == "replicate_as_reflect" and mode == "replicate" and W > max(lo, hi):
        mode = "reflect"
    if mut == "reflect_off_by_one" and mode == "reflect" and W > max(lo, hi) + 1:
        wide = pad_sp(x, zeros + [(lo + 1, hi + 1)], mode)           # -1 -> 2 instead of 1: the pad cells one further out
        return torch.cat([wide[..., :lo], x, wide[..., wide.shape[-1] - hi:]], -1)
    return pad_sp(x, zeros + [(lo, hi)], mode)


def lanes(v, width, mut=None):
    """channels-last v padded with zero lanes to `width`"""
    extra = width - v.shape[-1]
    if extra == 0:
        return v
    fill = torch.ones if mut == "pad_lanes_nonzero" else torch.zeros
    return torch.cat([v, fill(*v.shape[:-1], extra, dtype=v.dtype)], -1)


def unfold64(x, k, p, mode, fold_=0, mut=None):
    """x [N, C, *sp] float64 -> x'[n, ..., j][dw C + c] = pad(x)[n, c, ..., j + dw] on the domain padded by fold_ along
    depth (if D > 1) and rows, [N, *sp', W, k C]"""
    sp = x.shape[2:]
    C = x.shape[1]
    outer = [(fold_, fold_) if n > 1 or i == len(sp) - 2 else (0, 0) for i, n in enumerate(sp[:-1])]
    xp = pad_w(pad_sp(x, outer + [(0, 0)], mode), p, k - 1 - p, mode, mut)
    u = xp.unfold(-1, k, 1)                                           # [N, C, ..., W, k]
    if mut == "drop_last_tap":
        u = torch.cat([u[..., :k - 1], torch.zeros_like(u[..., :1])], -1)
    u = u.movedim(1, -2) if mut == "channel_order_c_dw" else u.movedim(1, -1)
    out = u.reshape(*u.shape[:-2], k * C)
    if mut == "halo_from_first_segment" and out.shape[-2] > WF_SEG:
        out = out.clone()
        for j in range(WF_SEG, min(WF_SEG + p, out.shape[-2])):       # taps of the second segment that reach back over j0
            n_back = p - (j - WF_SEG)
            out[..., j, :n_back * C] = out[..., j - WF_SEG, :n_back * C]
    return out


def adjoint(fwd, shape, cot):
    """float64 autograd of fwd at a zero leaf of `shape` with cotangent cot, and the same with |cot| -> (g, T)"""
    outs = []
    for c in (cot, cot.abs()):
        with torch.enable_grad():
            x = torch.zeros(*shape, dtype=torch.float64, requires_grad=True)
            (gx,) = torch.autograd.grad(fwd(x), [x], c)
        outs.append(gx)
    return outs


def shiftadd64(z, bias, k, Co, W, mut=None):
    """z [N, ..., W + k - 1, Pp] float64 -> s[n, co, ..., j] = bias[co] + sum_dw z[n, ..., j + dw][dw Co + co]"""
    taps = k - 1 if mut == "drop_last_tap" else k
    s = sum(z[..., dw:dw + W, dw * Co:(dw + 1) * Co] for dw in range(taps))
    if bias is not None and mut != "bias_after_act":
        s = s + bias
    return s.movedim(-1, 1)


# ---- launch plans, restated from the entry points' dispatch conditions ----------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def unfold_plan(C, W, k=KW, rows_opt=1):
    segs = ceil_div(W, WF_SEG)
    return dict(row=bool(rows_opt) and C * (WF_SEG + k - 1) * 4 <= 48 * 1024, segs=segs, last=W - (segs - 1) * WF_SEG)


def unfold_bwd_plan(C, W, Qp, rows_opt=1):
    why = "C" if C > 4 else "W" if W > 1024 else "Qp" if Qp % 8 else "lds" if W * Qp * 2 > 48 * 1024 else None
    return dict(row=bool(rows_opt) and why is None, why=why, passes=ceil_div(W, 256), lds=W * Qp * 2)


def shiftadd_plan(W, Pp, rows_opt=1):
    segs = ceil_div(W, WF_SEG)
    return dict(row=bool(rows_opt) and Pp % 8 == 0 and Pp <= 64, segs=segs, last=W - (segs - 1) * WF_SEG)


def shiftadd_bwd_plan(Co, W, k=KW, rows_opt=1):
    Wx = W + k - 1
    segs = ceil_div(Wx, WF_SEG)
    return dict(row=bool(rows_opt) and Co <= 16, segs=segs, last=Wx - (segs - 1) * WF_SEG)


def img_grid_plan(hw):
    bx = min(ceil_div(hw, 256), 1024)
    return dict(blocks=bx, strided=bx * 256 < hw)


def tap_block(c):
    return 256 if c >= 256 else 128 if c > 64 else 64


def rows_sum_plan(rows, c):
    """tap_rows_sum_kernel: which of the 32 row lanes run the four-in-flight loop, which the one-by-one tail"""
    unrolled, tail = set(), set()
    for part in range(32):
        r = part
        while r + 96 < rows:
            r += 128
            unrolled.add(part)
        if r < rows:
            tail.add(part)
    return dict(unrolled=len(unrolled), tail=len(tail), blocks=ceil_div(c, 32), idle=c % 32 != 0)


def axis_sources(n, p, mode):
    """the largest number of padded positions one position of an axis of length n collects (the adjoint of the pad of ones)"""
    if p == 0:
        return 1
    cnt, _ = adjoint(lambda x: pad_sp(x, [(0, 0), (p, p)], mode), (1, 1, 1, n), torch.ones(1, 1, 1, n + 2 * p, dtype=torch.float64))
    return int(cnt.max())


def _segs(prefix, plan):
    t = {f"{prefix}:row:{min(plan['segs'], 3)}seg"}
    if plan["segs"] > 1 and plan["last"] == 1:
        t.add(f"{prefix}:row:last1")
    if plan["last"] == WF_SEG:
        t.add(f"{prefix}:row:full")
    return t


def tags_of(c):
    """the branches a case is on, from its numbers alone"""
    t = set()
    if c.op == "unfold":
        pl = unfold_plan(c.C, c.W)
        t |= _segs("unfold", pl) if pl["row"] else {"unfold:pixel:lds"}
        t.add("unfold:pixel:switch")
        t |= {"unfold:W<k"} if c.W < KW else set()
        t |= {"unfold:padlanes"} if c.Qp > ceil_div(KW * c.C, 8) * 8 else set()
        t |= {"unfold:5d"} if c.vol else set()
    elif c.op == "unfold_bwd":
        pl = unfold_bwd_plan(c.C, c.W, c.Qp)
        if pl["row"]:
            t.add(f"unfold_bwd:row:pass{pl['passes']}")
            t |= {"unfold_bwd:row:48k"} if pl["lds"] == 48 * 1024 else set()
            srcs = axis_sources(c.H, c.fold, c.border)
            t.add(f"unfold_bwd:row:src{srcs}")
            t |= {"unfold_bwd:row:depth"} if c.D > 1 and c.fold else set()
        else:
            t.add(f"unfold_bwd:pixel:{pl['why']}")
        t.add("unfold_bwd:pixel:switch")
        t.add("unfold_bwd:accumulate" if c.acc else "unfold_bwd:overwrite")
    elif c.op == "shiftadd":
        pl, bl = shiftadd_plan(c.W, c.Pp), shiftadd_bwd_plan(c.Co, c.W)
        t |= _segs("shiftadd", pl) if pl["row"] else {"shiftadd:pixel:Pp"}
        if bl["row"]:
            t |= _segs("shiftadd_bwd", bl)
            t |= {"shiftadd_bwd:row:last6"} if bl["segs"] == 2 and bl["last"] == 6 else set()
        else:
            t.add("shiftadd_bwd:pixel:Co")
        t |= {"shiftadd:pixel:switch", "shiftadd_bwd:pixel:switch", "shiftadd:bias" if c.bias else "shiftadd:nobias"}
    elif c.op in ("to_act", "from_act", "pair", "to_act_bwd"):
        hw = math.prod(c.sp) if c.op == "to_act_bwd" else c.H * c.W
        t.add(f"{c.op}:{'strided' if img_grid_plan(hw)['strided'] else 'single'}")
        if c.op == "to_act_bwd":
            t.add(f"to_act_bwd:{c.mode}{c.fold}:{len(c.sp)}d")
            t |= {"to_act_bwd:extent1"} if 1 in c.sp else set()
            t.add("to_act_bwd:accumulate" if c.acc else "to_act_bwd:overwrite")
    elif c.op == "tap":
        t.add(f"tap:block{tap_block(c.c)}")
        t |= {"tap:wrap"} if c.c > tap_block(c.c) else set()
        t |= {"tap:ragged"} if c.c % tap_block(c.c) else set()
    elif c.op == "rows_sum":
        pl = rows_sum_plan(c.rows, c.c)
        t.add("rows_sum:" + ("tail_only" if not pl["unrolled"] else "unrolled_only" if not pl["tail"] else
                             "unrolled+tail" if pl["tail"] == 32 else "unrolled+some_tails"))
        t |= {"rows_sum:idle_lanes"} if pl["tail"] < 32 and not pl["unrolled"] else set()
        t |= {"rows_sum:blocks>1"} if pl["blocks"] > 1 else set()
        t |= {"rows_sum:ragged_c"} if pl["idle"] else set()
    elif c.op == "img_tap":
        t.add(f"img_tap:pad{c.pad}")
        t.add("img_tap:P1" if c.P == 1 else "img_tap:lds64k" if c.P * 4 == 64 * 1024 else
              "img_tap:P<=64" if c.P <= 64 else "img_tap:P>64")
        t |= {"img_tap:collide4", "img_tap:collide2"} if c.pad and c.P >= 64 else set()
    elif c.op == "flip":
        t.add(f"flip:{c.flag}:w{c.W}")
    elif c.op == "zeros":
        t.add(f"zeros:{c.path}")
    return t


BRANCHES = sorted(
    [f"unfold:row:{s}" for s in ("1seg", "2seg", "3seg", "last1", "full")] +
    ["unfold:pixel:lds", "unfold:pixel:switch", "unfold:W<k", "unfold:padlanes", "unfold:5d"] +
    [f"unfold_bwd:row:pass{i}" for i in (1, 2, 3, 4)] +
    [f"unfold_bwd:row:{s}" for s in ("48k", "src1", "src2", "src3", "src4", "src7", "depth")] +
    [f"unfold_bwd:pixel:{s}" for s in ("C", "W", "lds", "switch")] + ["unfold_bwd:accumulate", "unfold_bwd:overwrite"] +
    [f"shiftadd:row:{s}" for s in ("1seg", "2seg", "3seg", "last1", "full")] +
    ["shiftadd:pixel:Pp", "shiftadd:pixel:switch", "shiftadd:bias", "shiftadd:nobias"] +
    [f"shiftadd_bwd:row:{s}" for s in ("1seg", "2seg", "3seg", "full", "last6")] +
    ["shiftadd_bwd:pixel:Co", "shiftadd_bwd:pixel:switch"] +
    [f"{op}:{g}" for op in ("to_act", "from_act", "pair", "to_act_bwd") for g in ("single", "strided")] +
    [f"to_act_bwd:{m}:{d}d" for m in ("reflect0", "reflect1", "reflect3", "replicate1", "replicate2", "replicate3")
     for d in (2, 3)] + ["to_act_bwd:extent1", "to_act_bwd:accumulate", "to_act_bwd:overwrite"] +
    ["tap:block64", "tap:block128", "tap:block256", "tap:wrap", "tap:ragged"] +
    [f"rows_sum:{s}" for s in ("tail_only", "unrolled_only", "unrolled+tail", "unrolled+some_tails", "idle_lanes",
                               "blocks>1", "ragged_c")] +
    [f"img_tap:{s}" for s in ("pad0", "pad1", "pad3", "P1", "P<=64", "P>64", "lds64k", "collide4", "collide2")] +
    [f"flip:{f}:w{w}" for f in (0, 1) for w in (1, 2, 33)] + ["zeros:kernel", "zeros:kernel_strided", "zeros:torch"])


# ---- the case tables -----------------------------------------------------------------------------------------------------
def case(op, name, reaches, **p):
    return NS(op=op, name=name, reaches=reaches, **p)


def _join(*parts):
    return ", ".join(p for p in parts if p)


CQ = [(1, 8), (2, 16), (3, 32), (4, 32), (1, 16)]
WS = [4, 15, 256, 257, 300, 520]
BORDERS = ["reflect", "replicate", "zero"]
UNFOLD_W = {4: "unfold:row:1seg, unfold:W<k", 15: "unfold:row:1seg", 256: "unfold:row:1seg, unfold:row:full",
            257: "unfold:row:2seg, unfold:row:last1", 300: "unfold:row:2seg", 520: "unfold:row:3seg"}
UNFOLD_CASES = [
    case("unfold", f"c{C}q{Qp}_{b}_w{W}", _join(UNFOLD_W[W], "unfold:padlanes" if (C, Qp) == (1, 16) else "",
                                                "unfold:pixel:switch"), C=C, Qp=Qp, W=W, border=b, vol=False)
    for C, Qp in CQ for b in BORDERS for W in WS
] + [
    case("unfold", "vol_c2q16_reflect_w257", "unfold:5d, unfold:row:2seg", C=2, Qp=16, W=257, border="reflect", vol=True),
    case("unfold", "c64q448_reflect_w15", "unfold:pixel:lds", C=64, Qp=448, W=15, border="reflect", vol=False),
]

UB_W = {4: "unfold_bwd:row:pass1", 15: "unfold_bwd:row:pass1", 256: "unfold_bwd:row:pass1", 257: "unfold_bwd:row:pass2",
        300: "unfold_bwd:row:pass2", 520: "unfold_bwd:row:pass3"}


def _ub(name, reaches, C, Qp, W, fold_, border, acc, D=1, H=None):
    H = H if H is not None else (fold_ + 1 if border == "reflect" else 2)
    return case("unfold_bwd", name, _join(reaches, "unfold_bwd:pixel:switch", "unfold_bwd:accumulate" if acc else ""), C=C, Qp=Qp, W=W, fold=fold_, border=border,
                acc=acc, D=D, H=H)


UNFOLD_BWD_CASES = []
for _i, ((_C, _Qp), _W) in enumerate((cq, w) for cq in CQ for w in WS):
    _f, _b = (0, 1, 3)[_i % 3], BORDERS[(_i // 3) % 3]
    _D = 1 if _i % 5 else max(_f + 1, 2)
    UNFOLD_BWD_CASES.append(_ub(f"c{_C}q{_Qp}_w{_W}_{_b}{_f}_d{_D}" + ("_acc" if _i % 2 else ""), UB_W[_W], _C, _Qp, _W, _f, _b,
                                bool(_i % 2), D=_D, H=_f + 2 if _b == "reflect" else 2))
UNFOLD_BWD_CASES += [
    _ub("w1024_q24_48k", "unfold_bwd:row:pass4, unfold_bwd:row:48k", 3, 24, 1024, 1, "reflect", False, H=3),
    _ub("w1025_fallback", "unfold_bwd:pixel:W", 3, 24, 1025, 1, "reflect", True, H=3),
    _ub("w800_q32_fallback", "unfold_bwd:pixel:lds", 4, 32, 800, 1, "replicate", False),
    _ub("c5_q40_fallback", "unfold_bwd:pixel:C", 5, 40, 15, 3, "reflect", True, H=5),
    _ub("reflect3_h4", "unfold_bwd:row:src3", 3, 32, 15, 3, "reflect", False, H=4),
    _ub("reflect3_h5", "unfold_bwd:row:src3", 2, 16, 257, 3, "reflect", True, H=5),
    _ub("reflect3_h5_d4", "unfold_bwd:row:src3, unfold_bwd:row:depth", 1, 8, 15, 3, "reflect", False, D=4, H=5),
    _ub("replicate3_h1", "unfold_bwd:row:src7", 3, 32, 15, 3, "replicate", True, H=1),
    _ub("replicate3_h2_d2", "unfold_bwd:row:src4, unfold_bwd:row:depth", 4, 32, 300, 3, "replicate", False, D=2, H=2),
    _ub("reflect1_h4", "unfold_bwd:row:src2", 3, 32, 15, 1, "reflect", False, H=4),
    _ub("fold0", "unfold_bwd:row:src1, unfold_bwd:overwrite", 3, 32, 15, 0, "reflect", False, H=3),
]

COP = [(1, 8), (3, 32), (4, 32), (4, 64), (3, 72), (17, 120)]
SA_WS = [4, 15, 250, 256, 257, 520]
SA_W = {4: "shiftadd:row:1seg, shiftadd_bwd:row:1seg", 15: "shiftadd:row:1seg, shiftadd_bwd:row:1seg",
        250: "shiftadd:row:1seg, shiftadd_bwd:row:1seg, shiftadd_bwd:row:full",
        256: "shiftadd:row:1seg, shiftadd:row:full, shiftadd_bwd:row:2seg, shiftadd_bwd:row:last6",
        257: "shiftadd:row:2seg, shiftadd:row:last1, shiftadd_bwd:row:2seg", 520: "shiftadd:row:3seg, shiftadd_bwd:row:3seg"}
SA_C = {(3, 72): "shiftadd:pixel:Pp", (17, 120): "shiftadd:pixel:Pp, shiftadd_bwd:pixel:Co"}


def _sa_reaches(Co, Pp, W, bias):
    keep = [t for t in SA_W[W].split(", ")
            if not (t.startswith("shiftadd:row") and Pp > 64) and not (t.startswith("shiftadd_bwd:row") and Co > 16)]
    return _join(", ".join(keep), SA_C.get((Co, Pp), ""), "shiftadd:pixel:switch, shiftadd_bwd:pixel:switch",
                 "shiftadd:bias" if bias else "shiftadd:nobias")


SHIFTADD_CASES = [
    case("shiftadd", f"co{Co}p{Pp}_w{W}" + ("" if (i + j) % 2 else "_nobias"), _sa_reaches(Co, Pp, W, bool((i + j) % 2)), Co=Co, Pp=Pp, W=W,
         bias=bool((i + j) % 2))
    for i, (Co, Pp) in enumerate(COP) for j, W in enumerate(SA_WS)
]

CCP = [(1, 8), (3, 8), (3, 16), (8, 8), (9, 16)]
HW = {1: (1, 1), 255: (15, 17), 257: (1, 257), 513 * 512: (513, 512)}


def _act_cases(op):
    rows = [case(op, f"c{C}p{Cp}_hw{hw}", f"{op}:single", C=C, Cp=Cp, H=HW[hw][0], W=HW[hw][1])
            for C, Cp in CCP for hw in (1, 255, 257)]
    return rows + [case(op, f"c{C}p{Cp}_hw513x512", f"{op}:strided", C=C, Cp=Cp, H=513, W=512) for C, Cp in ((3, 8), (9, 16))]


TO_ACT_CASES = _act_cases("to_act")
FROM_ACT_CASES = _act_cases("from_act")
PAIR_CASES = [case("pair", f"a3b6p16_hw{h}x{w}", "pair:strided" if h * w > 1024 * 256 else "pair:single", Ca=3, Cb=6, Cp=16,
                   H=h, W=w) for h, w in HW.values()]

TO_ACT_BWD_CASES = []
for _i, (_m, _f) in enumerate([("reflect", 0), ("reflect", 1), ("reflect", 3), ("replicate", 1), ("replicate", 2),
                               ("replicate", 3)]):
    for _nd in (2, 3):
        _sp = (_f + 1, _f + 2) if _nd == 2 else (max(_f + 1, 2), _f + 1, _f + 2)
        _acc = bool((_i + _nd) % 2)
        TO_ACT_BWD_CASES.append(case(
            "to_act_bwd", f"{_m}{_f}_{_nd}d" + ("_acc" if _acc else ""),
            _join(f"to_act_bwd:{_m}{_f}:{_nd}d", "to_act_bwd:accumulate" if _acc else "to_act_bwd:overwrite",
                  "to_act_bwd:single"),
            C=(3, 9)[_i % 2], Cp=(8, 16)[_i % 2], sp=_sp, fold=_f, mode=_m, acc=_acc))
TO_ACT_BWD_CASES += [
    case("to_act_bwd", "replicate3_h1", "to_act_bwd:extent1", C=3, Cp=8, sp=(1, 5), fold=3, mode="replicate", acc=False),
    case("to_act_bwd", "replicate2_d2_h1_w1", "to_act_bwd:extent1", C=1, Cp=8, sp=(2, 1, 1), fold=2, mode="replicate",
         acc=True),
    case("to_act_bwd", "reflect1_513x512", "to_act_bwd:strided", C=1, Cp=8, sp=(513, 512), fold=1, mode="reflect", acc=False),
]

TAP_H, TAP_W = 9, 11                                   # 99 pixels: P = 97 distinct ids
TAP_C = {1: "tap:block64, tap:ragged", 64: "tap:block64", 65: "tap:block128, tap:ragged", 128: "tap:block128",
         255: "tap:block128, tap:wrap", 256: "tap:block256", 300: "tap:block256, tap:wrap, tap:ragged"}
TAP_CASES = [case("tap", f"c{c}_p{P}_f{(0, 1, 3)[(i + j) % 3]}", TAP_C[c], c=c, cs=ceil_div(c + 1, 8) * 8, P=P,
                  f0=(0, 1, 3)[(i + j) % 3], last=bool(i % 2))
             for i, c in enumerate(TAP_C) for j, P in enumerate((1, 97))]

RS_ROWS = {1: "rows_sum:tail_only, rows_sum:idle_lanes", 31: "rows_sum:tail_only, rows_sum:idle_lanes",
           32: "rows_sum:tail_only", 33: "rows_sum:tail_only", 97: "rows_sum:unrolled+some_tails",
           128: "rows_sum:unrolled_only", 129: "rows_sum:unrolled+some_tails", 2053: "rows_sum:unrolled+some_tails"}
RS_C = {1: "rows_sum:ragged_c", 32: "", 33: "rows_sum:blocks>1, rows_sum:ragged_c", 130: "rows_sum:blocks>1"}
ROWS_SUM_CASES = [case("rows_sum", f"r{r}_c{c}", _join(RS_ROWS[r], RS_C[c]), rows=r, c=c) for r in RS_ROWS for c in RS_C]
ROWS_SUM_CASES.append(case("rows_sum", "r224_c8", "rows_sum:unrolled+tail", rows=224, c=8))

IMG_TAP_CASES = [
    case("img_tap", f"pad{pad}_p{P}", _join(f"img_tap:pad{pad}", {1: "img_tap:P1", 64: "img_tap:P<=64", 65: "img_tap:P>64"}[P],
                                           "img_tap:collide4, img_tap:collide2" if pad and P > 1 else ""),
         pad=pad, P=P, H=8, W=9)
    for pad in (0, 1, 3) for P in (1, 64, 65)
] + [case("img_tap", "pad3_p16384", "img_tap:lds64k, img_tap:collide4", pad=3, P=16384, H=122, W=122)]

FLIP_CASES = [case("flip", f"flag{f}_w{w}", f"flip:{f}:w{w}", flag=f, W=w) for f in (0, 1) for w in (1, 2, 33)]
ZEROS_CASES = [
    case("zeros", "16_bytes", "zeros:kernel", shape=(1, 1, 1, 8), path="kernel"),
    case("zeros", "2x9x11x24", "zeros:kernel", shape=(2, 9, 11, 24), path="kernel"),
    case("zeros", "odd_bytes", "zeros:torch", shape=(1, 3, 5, 3), path="torch"),
    case("zeros", "wrapped_grid", "zeros:kernel_strided", shape=(2, 1025, 1024, 8), path="kernel_strided"),
]

TABLES = dict(unfold=UNFOLD_CASES, unfold_bwd=UNFOLD_BWD_CASES, shiftadd=SHIFTADD_CASES, to_act=TO_ACT_CASES,
              from_act=FROM_ACT_CASES, pair=PAIR_CASES, to_act_bwd=TO_ACT_BWD_CASES, tap=TAP_CASES, rows_sum=ROWS_SUM_CASES,
              img_tap=IMG_TAP_CASES, flip=FLIP_CASES, zeros=ZEROS_CASES)
ALL_CASES = [c for t in TABLES.values() for c in t]
BY_NAME = {(c.op, c.name): c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)
WFOLD_OPS = ("unfold", "unfold_bwd", "shiftadd")
SUM_OPS = ("unfold_bwd", "shiftadd", "to_act_bwd", "rows_sum")          # these run a second time on integer data
RUNS = [(c.op, c.name, d) for c in ALL_CASES for d in (("random", "int") if c.op in SUM_OPS else ("random",))]


def _gen(c, data):
    return torch.Generator().manual_seed(7000 + 17 * ALL_CASES.index(c) + (data == "int"))


def _to(dev):
    return lambda t: None if t is None else t.to(dev)


def _finish(got, wholes):
    out = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in got.items()}
    out["guards"] = all(guards_intact(w.cpu()) for w in wholes)
    return out


def _bufs(b, dev, names):
    bufs = {n: out_buffer(b.ref[n], dev) for n in names}
    return {n: v[0] for n, v in bufs.items()}, [v[1] for v in bufs.values()]


def _hip(ops):
    return hasattr(ops, "lib")


# ---- unfold ----------------------------------------------------------------------------------------------------------------
def _build_unfold(c, data):
    gen = _gen(c, data)
    img = rnd32(gen, *((N, c.C, 2, 2, c.W) if c.vol else (N, c.C, 2, c.W)))

    def refs(mut=None):
        return dict(act=Out("bits", BF16, lanes(unfold64(img.double(), KW, PW, c.border, mut=mut), c.Qp, mut)))
    return NS(img=img, refs=refs)


def _run_unfold(ops, b, dev):
    o, wh = _bufs(b, dev, ["act"])
    ops.image_unfold(b.img.to(dev), o["act"], KW, PW, b.case.border)
    return _finish(o, wh)


# ---- unfold backward ---------------------------------------------------------------------------------------------------
def _build_unfold_bwd(c, data):
    gen = _gen(c, data)
    fd = c.fold if c.D > 1 else 0
    sp = (c.D, c.H, c.W) if c.D > 1 else (c.H, c.W)
    gsp = ((c.D + 2 * fd,) if c.D > 1 else ()) + (c.H + 2 * c.fold, c.W)
    g = ints(gen, N, *gsp, c.Qp, dtype=BF16) if data == "int" else rndbf(gen, N, *gsp, c.Qp)
    shape = (N, c.C, *sp)
    pre = None if not c.acc else ints(gen, *shape) if data == "int" else torch.randn(*shape, generator=gen)
    kC = KW * c.C

    def refs(mut=None):
        v, T = adjoint(lambda x: unfold64(x, KW, PW, c.border, c.fold, mut), shape, g.double()[..., :kC])
        return dict(g_img=Out("sum", F32, v, T, pre))
    return NS(g=g, refs=refs)


def _run_unfold_bwd(ops, b, dev):
    c = b.case
    o, wh = _bufs(b, dev, ["g_img"])
    ops.image_unfold_backward(b.g.to(dev), o["g_img"], KW, PW, c.fold, c.border, accumulate=c.acc)
    return _finish(o, wh)


def single_source_rows(c):
    """bool [D, H]: the output rows of an unfold-backward case that collect ONE source row (from the adjoint of the pad of ones)"""
    if c.fold == 0:
        return torch.ones(c.D, c.H, dtype=torch.bool)
    fd = c.fold if c.D > 1 else 0
    cnt, _ = adjoint(lambda x: pad_sp(x, [(fd, fd), (c.fold, c.fold)], c.border), (1, 1, c.D, c.H),
                     torch.ones(1, 1, c.D + 2 * fd, c.H + 2 * c.fold, dtype=torch.float64))
    return cnt[0, 0] == 1


# ---- shift-add and its backward ----------------------------------------------------------------------------------------
def _build_shiftadd(c, data):
    gen = _gen(c, data)
    Wx = c.W + KW - 1
    if data == "int":
        z, bias = ints(gen, N, 2, Wx, c.Pp, dtype=BF16), ints(gen, c.Co) if c.bias else None
    else:
        z, bias = rndbf(gen, N, 2, Wx, c.Pp, scale=0.5), torch.randn(c.Co, generator=gen) * 0.5 if c.bias else None
    shape = (N, c.Co, 2, c.W)
    g_s, g = rnd32(gen, *shape), rnd32(gen, *shape, specials=False)
    o_img = torch.tanh(torch.randn(*shape, generator=gen) * 1.5)
    b64 = None if bias is None else bias.double()

    def refs(mut=None):
        zd = z.double()
        s = shiftadd64(zd, b64, KW, c.Co, c.W, mut)
        T = shiftadd64(zd.abs(), None if b64 is None else b64.abs(), KW, c.Co, c.W)
        th = torch.tanh(s)
        if mut == "bias_after_act" and b64 is not None:
            th = th + b64.view(1, -1, 1, 1)
        fwd = lambda x: shiftadd64(x, None, KW, c.Co, c.W, mut)
        od = o_img.double()
        gz_s, _ = adjoint(fwd, z.shape, g_s.double())
        gz_t, _ = adjoint(fwd, z.shape, g.double() * (1 - od * od))
        _, T_t = adjoint(fwd, z.shape, g.double().abs() * (1 + od * od))
        if mut == "pad_lanes_nonzero":
            gz_s = lanes(gz_s[..., :KW * c.Co], c.Pp, mut)
        return dict(img_none=Out("sum", F32, s, T), img_tanh=Out("tanh", F32, th, pre="img_none"),
                    gz_none=Out("bits", BF16, gz_s, zero_sign=False), gz_tanh=Out("bf16", BF16, gz_t, T_t))
    return NS(z=z, bias=bias, g_s=g_s, g=g, o_img=o_img, refs=refs)


def _run_shiftadd(ops, b, dev):
    to = _to(dev)
    o, wh = _bufs(b, dev, ["img_none", "img_tanh", "gz_none", "gz_tanh"])
    z, bias = to(b.z), to(b.bias)
    ops.shiftadd_to_image(z, bias, o["img_none"], KW, act="none")
    ops.shiftadd_to_image(z, bias, o["img_tanh"], KW, act="tanh")
    ops.shiftadd_to_image_backward(to(b.g_s), None, o["gz_none"], KW, act="none")
    ops.shiftadd_to_image_backward(to(b.g), to(b.o_img), o["gz_tanh"], KW, act="tanh")
    return _finish(o, wh)


# ---- image <-> activation ------------------------------------------------------------------------------------------------
def _build_to_act(c, data):
    img = rnd32(_gen(c, data), N, c.C, c.H, c.W)
    return NS(img=img, refs=lambda mut=None: dict(act=Out("bits", BF16, lanes(img.double().movedim(1, -1), c.Cp, mut))))


def _run_to_act(ops, b, dev):
    o, wh = _bufs(b, dev, ["act"])
    ops.image_to_act(b.img.to(dev), o["act"])
    return _finish(o, wh)


def _build_pair(c, data):
    gen = _gen(c, data)
    a, bb = rnd32(gen, N, c.Ca, c.H, c.W), rnd32(gen, N, c.Cb, c.H, c.W)
    g = rnd32(gen, N, c.H, c.W, c.Cp).to(BF16)

    def refs(mut=None):
        ga, gb = g.double()[..., :c.Ca].movedim(-1, 1), g.double()[..., c.Ca:c.Ca + c.Cb].movedim(-1, 1)
        return dict(act=Out("bits", BF16, lanes(torch.cat([a, bb], 1).double().movedim(1, -1), c.Cp, mut)),
                    ga=Out("bits", F32, ga), gb=Out("bits", F32, gb), ga_only=Out("bits", F32, ga), gb_only=Out("bits", F32, gb))
    return NS(a=a, b=bb, g=g, refs=refs)


def _run_pair(ops, b, dev):
    c, to = b.case, _to(dev)
    o, wh = _bufs(b, dev, ["act", "ga", "gb", "ga_only", "gb_only"])
    ops.image_cat_to_act([(to(b.a), 0, c.Ca), (to(b.b), 0, c.Cb)], o["act"])
    g = to(b.g)
    ops.image_cat_to_act_backward(g, [o["ga"], o["gb"]], [c.Ca, c.Cb])
    ops.image_cat_to_act_backward(g, [o["ga_only"], None], [c.Ca, c.Cb])
    ops.image_cat_to_act_backward(g, [None, o["gb_only"]], [c.Ca, c.Cb])
    return _finish(o, wh)


TANH_INPUTS = torch.tensor([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 2.0 ** -8, 0.5, -0.5, 1.0, 5.0, -5.0, 9.0, -9.0, 20.0, -20.0, 88.0])


def _build_from_act(c, data):
    gen = _gen(c, data)
    act = rnd32(gen, N, c.H, c.W, c.Cp).to(BF16)                       # for the act-none move: every special bf16 value
    act_t = torch.randn(N, c.H, c.W, c.Cp, generator=gen) * 2
    n = min(act_t.numel(), TANH_INPUTS.numel())
    act_t.view(-1)[:n] = TANH_INPUTS[:n]
    act_t = act_t.to(BF16)
    shape = (N, c.C, c.H, c.W)
    g_s, g = rnd32(gen, *shape), rnd32(gen, *shape, specials=False)
    o_img = torch.tanh(torch.randn(*shape, generator=gen) * 1.5)

    def refs(mut=None):
        od, gd = o_img.double(), g.double()
        return dict(img_none=Out("bits", F32, act.double()[..., :c.C].movedim(-1, 1)),
                    img_pre=Out("bits", F32, act_t.double()[..., :c.C].movedim(-1, 1)),
                    img_tanh=Out("tanh", F32, torch.tanh(act_t.double()[..., :c.C].movedim(-1, 1)), pre="img_pre"),
                    ga_none=Out("bits", BF16, lanes(g_s.double().movedim(1, -1), c.Cp, mut)),
                    ga_tanh=Out("bf16", BF16, lanes((gd * (1 - od * od)).movedim(1, -1), c.Cp),
                                lanes((gd.abs() * (1 + od * od)).movedim(1, -1), c.Cp)))
    return NS(act=act, act_t=act_t, g_s=g_s, g=g, o_img=o_img, refs=refs)


def _run_from_act(ops, b, dev):
    to = _to(dev)
    o, wh = _bufs(b, dev, ["img_none", "img_pre", "img_tanh", "ga_none", "ga_tanh"])
    ops.act_to_image(to(b.act), o["img_none"], act="none")
    ops.act_to_image(to(b.act_t), o["img_pre"], act="none")
    ops.act_to_image(to(b.act_t), o["img_tanh"], act="tanh")
    ops.act_to_image_backward(to(b.g_s), None, o["ga_none"], act="none")
    ops.act_to_image_backward(to(b.g), to(b.o_img), o["ga_tanh"], act="tanh")
    return _finish(o, wh)


def _build_to_act_bwd(c, data):
    gen = _gen(c, data)
    psp = tuple(n + 2 * c.fold for n in c.sp)
    gpad = ints(gen, N, *psp, c.Cp, dtype=BF16) if data == "int" else rndbf(gen, N, *psp, c.Cp)
    shape = (N, c.C, *c.sp)
    pre = None if not c.acc else ints(gen, *shape) if data == "int" else torch.randn(*shape, generator=gen)

    def refs(mut=None):
        v, T = fold(gpad, c.sp, c.fold, c.mode)
        back = lambda t: t[..., :c.C].reshape(N, *c.sp, c.C).movedim(-1, 1)
        return dict(g_img=Out("sum", F32, back(v), back(T), pre))
    return NS(gpad=gpad, refs=refs)


def _run_to_act_bwd(ops, b, dev):
    c = b.case
    o, wh = _bufs(b, dev, ["g_img"])
    ops.image_to_act_backward(b.gpad.to(dev), o["g_img"], fold=c.fold, fold_mode=c.mode, accumulate=c.acc)
    return _finish(o, wh)


# ---- taps ------------------------------------------------------------------------------------------------------------------
def _build_tap(c, data):
    gen = _gen(c, data)
    px = TAP_H * TAP_W
    if c.P == 1:
        ids = torch.tensor([px - 1 if c.last else 0])
    else:
        mid = torch.randperm(px - 2, generator=gen)[:c.P - 2] + 1
        ids = torch.cat([torch.tensor([0, px - 1]), mid])[torch.randperm(c.P, generator=gen)]
    src = rnd32(gen, N, TAP_H, TAP_W, c.cs).to(BF16)
    Hp, Wp = TAP_H + 2 * c.f0, TAP_W + 2 * c.f0
    dst0 = rndbf(gen, N, Hp, Wp, c.cs)
    g = torch.randn(N, c.P, c.c, generator=gen)
    flat = (ids // TAP_W + c.f0) * Wp + ids % TAP_W + c.f0
    n = min(c.c, SPECIALS.numel())
    dst0.view(N, -1, c.cs)[:, flat[0], :n] = 0                         # 0 + s: the roundings of the specials themselves
    g[:, 0, :n] = SPECIALS[:n]

    def refs(mut=None):
        d = dst0.double().view(N, -1, c.cs).clone()
        d[:, flat, :c.c] += g.double()
        return dict(gather=Out("bits", F32, src.double().view(N, -1, c.cs)[:, ids, :c.c]),
                    scatter=Out("bits", BF16, d.view(N, Hp, Wp, c.cs), prefill=dst0))
    return NS(ids=ids, src=src, g=g, refs=refs)


def _run_tap(ops, b, dev):
    c, to = b.case, _to(dev)
    o, wh = _bufs(b, dev, ["gather", "scatter"])
    ids, src = to(b.ids), to(b.src)
    if _hip(ops):
        from ganslate_amd.hip import lib as L
        from ganslate_amd.hip.ops import _ptr, _stream
        L.check(ops.lib.gs_tap_gather(_ptr(src), N, TAP_H * TAP_W, c.cs, _ptr(ids), c.P, c.c, _ptr(o["gather"]), _stream()),
                "gs_tap_gather")
    else:
        o["gather"].copy_(ops.tap_gather(src, ids, c.c))
    ops.tap_scatter_add(o["scatter"], ids, to(b.g), TAP_W, f0=c.f0)
    return _finish(o, wh)


def _build_rows_sum(c, data):
    gen = _gen(c, data)
    g = ints(gen, c.rows, c.c) if data == "int" else torch.randn(c.rows, c.c, generator=gen)
    pre = ints(gen, c.c) if data == "int" else torch.randn(c.c, generator=gen)
    return NS(g=g, refs=lambda mut=None: dict(db=Out("sum", F32, g.double().sum(0), g.double().abs().sum(0), pre)))


def _run_rows_sum(ops, b, dev):
    o, wh = _bufs(b, dev, ["db"])
    ops.tap_rows_sum(b.g.to(dev), o["db"])
    return _finish(o, wh)


def _padded_index(H, W, pad):
    """the unpadded pixel every padded position reflects onto: the index image through the same F.pad"""
    idx = torch.arange(H * W, dtype=torch.float64).view(1, 1, H, W)
    return pad_sp(idx, [(pad, pad), (pad, pad)], "reflect").view(-1).long()


def _build_img_tap(c, data):
    gen = _gen(c, data)
    H, W, pad, P, C = c.H, c.W, c.pad, c.P, 3
    Wp = W + 2 * pad
    tgt_of = _padded_index(H, W, pad)
    pos = lambda y, x: (y + pad) * Wp + x + pad                         # padded id of image coordinate (y, x), pads negative
    if P == 1:
        ids = torch.tensor([0])                                        # the padded corner
    elif P == tgt_of.numel():
        ids = torch.randperm(P, generator=gen)                         # every padded position: every class, many times
    else:
        # pixel (1, 1) receives 4 samples, pixel (1, 4) two, the others one each; shuffled sample order
        first = [pos(1, 1), pos(-1, 1), pos(1, -1), pos(-1, -1), pos(1, 4), pos(-1, 4)] if pad else [pos(1, 1), pos(1, 4)]
        used = {int(tgt_of[i]) for i in first}
        rest = [pos(y, x) for y in range(H) for x in range(W) if y * W + x not in used]
        rest = [rest[i] for i in torch.randperm(len(rest), generator=gen)[:P - len(first)]]
        ids = torch.tensor(first + rest)[torch.randperm(P, generator=gen)]
    assert ids.numel() == P and ids.unique().numel() == P
    tgt = tgt_of[ids]
    x = rnd32(gen, N, C, H, W)
    g = torch.randn(N, P, C, generator=gen)

    def refs(mut=None):
        xp = pad_sp(x.double(), [(pad, pad), (pad, pad)], "reflect")
        acc = torch.zeros(N, C, H * W)                                  # fp32: the header's sequential sum in sample order
        order = range(P - 1, -1, -1) if mut == "colliders_reversed" else range(P)
        for q in order:
            acc[:, :, tgt[q]] += g[:, q, :]
        return dict(gather=Out("bits", F32, xp.permute(0, 2, 3, 1).flatten(1, 2)[:, ids, :]),
                    scatter=Out("bits", F32, acc.double().view(N, C, H, W), zero_sign=False))
    return NS(ids=ids, tgt=tgt, x=x, g=g, refs=refs)


def _run_img_tap(ops, b, dev):
    c, to = b.case, _to(dev)
    o, wh = _bufs(b, dev, ["gather", "scatter"])
    ids, x, g = to(b.ids), to(b.x), to(b.g)
    if _hip(ops):
        from ganslate_amd.hip import lib as L
        from ganslate_amd.hip.ops import _ptr, _stream
        L.check(ops.lib.gs_image_tap_gather(_ptr(x), N, 3, c.H, c.W, c.pad, _ptr(ids), c.P, _ptr(o["gather"]), _stream()),
                "gs_image_tap_gather")
        L.check(ops.lib.gs_image_tap_scatter(_ptr(g), N, 3, c.H, c.W, c.pad, _ptr(ids), c.P, _ptr(o["scatter"]), _stream()),
                "gs_image_tap_scatter")
    else:
        o["gather"].copy_(ops.image_tap_gather(x, ids, c.pad))
        o["scatter"].copy_(ops.image_tap_scatter(g, ids, (N, 3, c.H, c.W), c.pad))
    return _finish(o, wh)


def _build_flip(c, data):
    x = rnd32(_gen(c, data), N, 3, c.W)
    return NS(x=x, refs=lambda mut=None: dict(out=Out("bits", F32, (x.flip(-1) if c.flag else x).double())))


def _run_flip(ops, b, dev):
    c = b.case
    o, wh = _bufs(b, dev, ["out"])
    x, flag = b.x.to(dev), torch.tensor([c.flag], dtype=torch.int32, device=dev)
    if _hip(ops):
        from ganslate_amd.hip import lib as L
        from ganslate_amd.hip.ops import _ptr, _stream
        L.check(ops.lib.gs_flip_w_if(_ptr(x), _ptr(o["out"]), N * 3, c.W, _ptr(flag), _stream()), "gs_flip_w_if")
    else:
        o["out"].copy_(ops.flip_w_if(x, flag))
    return _finish(o, wh)


def _build_zeros(c, data):
    return NS(refs=lambda mut=None: dict(out=Out("bits", BF16, torch.zeros(*c.shape, dtype=torch.float64))))


def _run_zeros(ops, b, dev):
    o, wh = _bufs(b, dev, ["out"])
    if _hip(ops):
        ops.zero_fill(o["out"])                                        # what zeros_like_act runs on its fresh tensor
    else:
        o["out"].copy_(ops.zeros_like_act(o["out"]))
    return _finish(o, wh)


OPS = dict(unfold=(_build_unfold, _run_unfold), unfold_bwd=(_build_unfold_bwd, _run_unfold_bwd),
           shiftadd=(_build_shiftadd, _run_shiftadd), to_act=(_build_to_act, _run_to_act), pair=(_build_pair, _run_pair),
           from_act=(_build_from_act, _run_from_act), to_act_bwd=(_build_to_act_bwd, _run_to_act_bwd), tap=(_build_tap, _run_tap),
           rows_sum=(_build_rows_sum, _run_rows_sum), img_tap=(_build_img_tap, _run_img_tap), flip=(_build_flip, _run_flip),
           zeros=(_build_zeros, _run_zeros))


@lru_cache(maxsize=2)
def build(op, name, data="random"):
    c = BY_NAME[(op, name)]
    b = OPS[op][0](c, data)
    b.case, b.data = c, data
    b.ref = b.refs()
    return b


def run(ops, b, dev="cpu"):
    return OPS[b.case.op][1](ops, b, dev)


# ---- refusals: each raises before any launch ------------------------------------------------------------------------------
def refusals(ops, dev):
    """[(what, call, who)]; the tensors are real and large enough for what is asked, so that nothing but the check decides.
    who = "library": the entry point's own error (rc = 2); "wrapper": HipOps' ValueError, raised before the library is asked
    (the library's rc = 2 for the same condition: tests/test_boundary_edges_cpu.py)"""
    f32 = lambda *s: torch.zeros(*s, device=dev)
    bf = lambda *s: torch.zeros(*s, dtype=BF16, device=dev)
    ids = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)
    return [
        ("replicate fold 4 (gs_image_to_act_backward)",
         lambda: ops.image_to_act_backward(bf(1, 13, 13, 8), f32(1, 1, 5, 5), fold=4, fold_mode="replicate"), "library"),
        ("replicate fold 4 (gs_image_unfold_backward)",
         lambda: ops.image_unfold_backward(bf(1, 13, 15, 8), f32(1, 1, 5, 15), KW, PW, 4, "replicate"), "library"),
        ("Qp < k C", lambda: ops.image_unfold(f32(1, 2, 2, 15), bf(1, 2, 15, 8), KW, PW, "reflect"), "library"),
        ("Qp < k C (backward)", lambda: ops.image_unfold_backward(bf(1, 2, 15, 8), f32(1, 2, 2, 15), KW, PW, 0, "reflect"), "library"),
        ("Qp no multiple of 8", lambda: ops.image_unfold(f32(1, 1, 2, 15), bf(1, 2, 15, 12), KW, PW, "reflect"), "library"),
        ("pair with Cp < Ca + Cb",
         lambda: ops.image_cat_to_act([(f32(1, 3, 2, 2), 0, 3), (f32(1, 6, 2, 2), 0, 6)], bf(1, 2, 2, 8)), "wrapper"),
        ("P = 16385", lambda: ops.image_tap_scatter(f32(1, 16385, 1), ids(16385), (1, 1, 4, 4), 0), "library"),
        ("reflect fold 3 with H = 3 (gs_image_to_act_backward)",
         lambda: ops.image_to_act_backward(bf(1, 9, 11, 8), f32(1, 1, 3, 5), fold=3, fold_mode="reflect"), "library"),
        ("reflect fold 2 with W = 2 (gs_image_to_act_backward)",
         lambda: ops.image_to_act_backward(bf(1, 9, 6, 8), f32(1, 1, 5, 2), fold=2, fold_mode="reflect"), "library"),
        ("reflect fold 2 with D = 2 (gs_image_to_act_backward)",
         lambda: ops.image_to_act_backward(bf(1, 6, 9, 9, 8), f32(1, 1, 2, 5, 5), fold=2, fold_mode="reflect"), "library"),
        ("reflect unfold with W = 3 = p", lambda: ops.image_unfold(f32(1, 1, 2, 3), bf(1, 2, 3, 8), KW, PW, "reflect"), "library"),
        ("reflect unfold backward with W = 3 = p",
         lambda: ops.image_unfold_backward(bf(1, 2, 3, 8), f32(1, 1, 2, 3), KW, PW, 0, "reflect"), "library"),
        ("reflect unfold backward with H = fold",
         lambda: ops.image_unfold_backward(bf(1, 6, 15, 8), f32(1, 1, 2, 15), KW, PW, 2, "reflect"), "library"),
        ("reflect unfold backward with D = fold",
         lambda: ops.image_unfold_backward(bf(1, 6, 9, 15, 8), f32(1, 1, 2, 5, 15), KW, PW, 2, "reflect"), "library"),
    ]
