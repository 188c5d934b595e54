"""float64 statement of csrc/norm.hip (InstanceNorm2d/3d -> ReLU / LeakyReLU -> [+res], its backward with the adjoint of
nn.ReflectionPad2d / nn.ReplicationPad3d folded in, the statistics finalize, the batched bias gradients) and of
csrc/norm_ex.hip (the U-Net form: two activations into channel slices, dropout regenerated from a hash), the tables of cases
that reach every branch of their launch plans, and the measurement (tests/test_inorm_edges_cpu.py,
tests/test_inorm_edges_gpu.py). The criterion is the one of tests/pnorm_ref.py, imported, not restated.

Written from the headers of norm.hip / norm_ex.hip and include/ganslate_hip.h, not from the kernels' loops: one pass over
whole float64 tensors, sums by torch.sum in float64.

Statistics: mean_rstd is an INPUT of apply and backward (the fp32 numbers given, cast to double). The sign of yhat is then
structurally unambiguous: fp32 y - mu has the true sign (one rounding of an exact difference keeps it), rstd > 0, and the
residual is added after the activation. `ambiguous` counts the elements where fp32 would decide otherwise; it must be 0.

Fold: fold() is float64 autograd of F.pad(mode="reflect" | "replicate") on a zero leaf, which shares no index arithmetic with
the kernel or with oracle/ops_ref._fold. The gradients of the table are multiples of 2^-6 below 4, so every folded sum (at
most 64 + 1 terms) is exact in fp32 in any order: gsum must be the bf16 rounding of the float64 fold, bit for bit.

Finalize (derived, not measured): the kernel adds the fp32 partials in double and rounds mean and rstd to fp32 once. With
S0, S1 the float64 sums of the partials, mean = S0/hw, var0 = S1/hw - mean^2, u = 2^-24 and d the relative error of the
1/hw the kernel multiplies by (gs_inorm_finalize takes 1/hw as a float: d = 2^-24; the fused kernel divides in double: d = 0):
  |mean' - mean| <= e_m (1 + u) + u |mean|,   e_m = d |mean| + (slots + 4) 2^-53 sum|p0| / hw
  |var' - var0|  <= e_v = d S1/hw + (2d + d^2) mean^2 + 4 (slots + 4) 2^-53 (sum|p1|/hw + (sum|p0|/hw)^2)
  rstd' in [(max(var0 + e_v, 0) + eps)^-1/2 (1 - u'), (max(var0 - e_v, 0) + eps)^-1/2 (1 + u')],  u' = u + 2^-50
(the cancellation of E[x^2] - mean^2 propagated through (var + eps)^-1/2 exactly, not to first order). eps is the float given.

Dropout (norm_ex.hip header): h = murmur3 finaliser of idx ^ fin(lo + 0x9e3779b9 (n + 1)) ^ hi with (hi, lo) the 64-bit seed
(host part + device part), idx counting the scalars of one image of y in NHWC order; u = (h >> 8) 2^-24; keep iff
u >= float32(drop_p); kept elements are scaled by 1 / (1 - float32(drop_p)), here in float64.

tanh in the FORWARD of norm_ex is left out: the accuracy of gs_tanh_call / tanhf is not the subject of these tests. The
backward's general form (act' from a stored tanh output) is covered by one backward-only case.
"""
import math
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

from tests import pnorm_ref as P
from tests.pnorm_ref import (BIAS_PREFILL, DETUNE_MU, DETUNE_RSTD, K2_CAP, K_CAP, STATS, U24,  # noqa: F401 (re-exported)
                             bf16_excess, f32_excess, outside_untouched, worst)

EPS32 = float(np.float32(1e-5))          # eps as the float the entry points take
SLOPE = 0.2
BF16 = torch.bfloat16
GUARD = 4096                             # guard elements on each side of every output buffer
PATTERN = {torch.bfloat16: (torch.int16, 0x5A3C), torch.float32: (torch.int32, 0x5A3C5A3C)}


# ---- guarded output buffers --------------------------------------------------------------------------------------------
def guarded(shape, dtype, dev, fill=None):
    """a 16-byte-aligned view of `shape` inside a larger allocation whose GUARD elements on either side hold a fixed bit
    pattern; the payload is NaN, or a copy of `fill` -> (view, whole allocation)"""
    n = math.prod(shape)
    whole = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
    it, pat = PATTERN[dtype]
    whole.view(it).fill_(pat)
    pay = whole[GUARD:GUARD + n].view(shape)
    assert pay.data_ptr() % 16 == 0
    if fill is None:
        pay.fill_(float("nan"))
    else:
        pay.copy_(fill)
    return pay, whole


def guards_intact(whole):
    it, pat = PATTERN[whole.dtype]
    w = whole.view(it)
    return bool((w[:GUARD] == pat).all()) and bool((w[-GUARD:] == pat).all())


# ---- the operations in float64 -----------------------------------------------------------------------------------------
def flat(t):
    """[N, ..., C] -> float64 [N, pixels, C]"""
    return t.double().reshape(t.shape[0], -1, t.shape[-1])


def fold(gpad, dims, p, mode):
    """adjoint of F.pad(x, p on every axis of dims, mode) applied to gpad [N, *padded dims, C] -> (g, T) float64
    [N, pixels, C]; T is the same adjoint of |gpad| (the sum of the absolute terms of each element of g)"""
    gp = gpad.double()
    if p == 0:
        return flat(gp), flat(gp).abs()
    N, C = gp.shape[0], gp.shape[-1]
    outs = []
    for src in (gp, gp.abs()):
        with torch.enable_grad():
            x = torch.zeros(N, C, *dims, dtype=torch.float64, requires_grad=True)
            (gx,) = torch.autograd.grad(F.pad(x, (p, p) * len(dims), mode=mode), [x], src.movedim(-1, 1).contiguous())
        outs.append(gx.movedim(1, -1).reshape(N, -1, C))
    return outs[0], outs[1]


def act_of(yh, act, slope=SLOPE):
    """-> (act(yh), act'(yh)) for relu / lrelu / none; act' is also the factor s of the absolute term"""
    if act == "none":
        return yh, torch.ones_like(yh)
    neg = 0.0 if act == "relu" else slope
    d = torch.where(yh > 0, torch.ones_like(yh), torch.full_like(yh, neg))
    return yh * d, d


def normalise(y, mean_rstd):
    """-> (yhat, rstd or None, ambiguous)"""
    yv = flat(y)
    if mean_rstd is None:
        return yv, None, 0
    mu, rstd = P.split_stats(mean_rstd, yv.shape[0], yv.shape[2])
    yh = (yv - mu) * rstd
    amb = int((((yv.float() - mu.float()) > 0) != (yh > 0)).sum()) + int((rstd <= 0).sum())
    return yh, rstd, amb


@dataclass
class Fwd:
    out: torch.Tensor
    T: torch.Tensor
    ambiguous: int


def forward(y, mean_rstd, res=None, act="none", slope=SLOPE):
    """x = act(yhat) [+ res];  T = s |yhat| (+ |res|), s = 1 or the slope (0 for the clipped side of relu: exact zero)"""
    yh, _, amb = normalise(y, mean_rstd)
    v, s = act_of(yh, act, slope)
    T = s * yh.abs()
    if res is not None:
        r = flat(res)
        v, T = v + r, T + r.abs()
    return Fwd(v, T, amb)


@dataclass
class Bwd:
    g: torch.Tensor           # folded gradient + g2 (= gsum)
    dy: torch.Tensor
    T_dy: torch.Tensor
    bias: torch.Tensor        # [C] sum over the images of -rstd S2 S3 / hw (None without a norm)
    bias_terms: torch.Tensor
    sums: dict = field(default_factory=dict)
    ambiguous: int = 0


def norm_core(gh, T_gh, yh, rstd, S=None):
    """dy = rstd (ghat - S1/hw - yhat S2/hw) with the T's and the bias terms of pnorm_ref.backward. S: (S1, S2, S3) given
    from outside (the pre_slots form) in place of the sums of ghat, ghat yhat, yhat"""
    hw = yh.shape[1]
    p = gh * yh
    S1, A1 = gh.sum(1, keepdim=True), gh.abs().sum(1, keepdim=True)
    S2, A2 = p.sum(1, keepdim=True), p.abs().sum(1, keepdim=True)
    S3, A3 = yh.sum(1, keepdim=True), yh.abs().sum(1, keepdim=True)
    own = dict(S1=S1, S2=S2, S3=S3)
    if S is not None:
        S1, S2, S3 = S
    dy = rstd * (gh - S1 / hw - yh * S2 / hw)
    T_dy = rstd * (T_gh + A1 / hw + yh.abs() * A2 / hw)
    bias = (-rstd * S2 * S3 / hw).sum((0, 1))
    bias_terms = (rstd / hw * (S3.abs() * A2 + S2.abs() * A3 + (S2 * S3).abs())).sum((0, 1))
    return dy, T_dy, bias, bias_terms, dict(own, A1=A1, A2=A2, A3=A3)


def pre_sums(partial, N, slots, C):
    """the float64 sums of given fp32 partials [N][slots][3][C] -> (S1, S2, S3) each [N, 1, C]"""
    s = partial[:N * slots * 3 * C].double().view(N, slots, 3, C).sum(1)
    return s[:, 0, None], s[:, 1, None], s[:, 2, None]


def backward(gpad, g2, y, mean_rstd, dims, p=0, mode="reflect", act="none", slope=SLOPE, pre=None):
    """g = fold(gpad) + g2; ghat = g act'(yhat); dy as norm_core; without a norm dy = g act'(y). pre = (slots, partials)"""
    g, T_g = fold(gpad, dims, p, mode)
    if g2 is not None:
        g, T_g = g + flat(g2), T_g + flat(g2).abs()
    yh, rstd, amb = normalise(y, mean_rstd)
    _, d = act_of(yh, act, slope)
    gh, T_gh = g * d, T_g * d
    if rstd is None:
        return Bwd(g, gh, T_gh, None, None, ambiguous=amb)
    S = pre_sums(pre[1], yh.shape[0], pre[0], yh.shape[2]) if pre is not None else None
    dy, T_dy, bias, terms, sums = norm_core(gh, T_gh, yh, rstd, S)
    return Bwd(g, dy, T_dy, bias, terms, sums, amb)


@dataclass
class Fin:
    mean: torch.Tensor
    rstd: torch.Tensor
    mean_tol: torch.Tensor
    rstd_lo: torch.Tensor
    rstd_hi: torch.Tensor

    def check(self, mr):
        """mr: published fp32 [N, 2, C] -> (worst |mean error| / tolerance, rstd inside its interval). A NaN fails both"""
        m, r = mr[:, 0].double(), mr[:, 1].double()
        em = torch.nan_to_num((m - self.mean).abs() / self.mean_tol, nan=float("inf"))
        inside = bool(((r >= self.rstd_lo) & (r <= self.rstd_hi)).all())
        return float(em.max()), inside


def finalize(partial, N, slots, C, hw, eps=EPS32, inv_hw_f32=True):
    """mean, rstd from the float64 sums of the given fp32 partials [N][slots][2][C], with the derived bounds of the docstring"""
    p = partial.double().view(N, slots, 2, C)
    S, A = p.sum(1), p.abs().sum(1)
    mean, ex2 = S[:, 0] / hw, S[:, 1] / hw
    var0 = ex2 - mean * mean
    rstd = 1.0 / torch.sqrt(var0.clamp_min(0) + eps)
    d = U24 if inv_hw_f32 else 0.0
    dbl = (slots + 4) * 2.0 ** -53
    e_m = d * mean.abs() + dbl * A[:, 0] / hw
    mean_tol = e_m * (1 + U24) + U24 * mean.abs() + 1e-300
    e_v = d * ex2.abs() + (2 * d + d * d) * mean * mean + 4 * dbl * (A[:, 1] / hw + (A[:, 0] / hw) ** 2)
    u1 = U24 + 2.0 ** -50
    lo = (1 - u1) / torch.sqrt((var0 + e_v).clamp_min(0) + eps)
    hi = (1 + u1) / torch.sqrt((var0 - e_v).clamp_min(0) + eps)
    return Fin(mean, rstd, mean_tol, lo, hi)


def partials_from(yv, owner, slots):
    """fp32 statistics partials [N][slots][2][C] as a producing conv leaves them: pixel i belongs to slot owner[i], each slot's
    sums rounded to fp32. yv: float64 [N, pixels, C]"""
    N, hw, C = yv.shape
    part = torch.zeros(N, slots, 2, C, dtype=torch.float64)
    part[:, :, 0].index_add_(1, owner, yv)
    part[:, :, 1].index_add_(1, owner, yv * yv)
    return part.float()


def partials_of(y, slots, gen):
    """the pixels of y dealt out to the slots at random -> flat fp32 partials"""
    yv = flat(y)
    return partials_from(yv, torch.randint(0, slots, (yv.shape[1],), generator=gen), slots).reshape(-1).contiguous()


# ---- the dropout mask --------------------------------------------------------------------------------------------------
def _fin32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16); x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13); x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def drop_scale(N, per_img, drop_p, seed, seed_dev=None):
    """mask / (1 - p) as float64 [N, per_img]; seed_dev: (lo, hi) words added to the 64-bit host seed"""
    if drop_p <= 0:
        return torch.ones(N, per_img, dtype=torch.float64)
    with np.errstate(over="ignore"):
        s = np.uint64(seed & 0xFFFFFFFFFFFFFFFF)
        if seed_dev is not None:
            lo, hi = (int(v) & 0xFFFFFFFF for v in seed_dev)
            s = s + np.uint64(hi << 32 | lo)
        lo, hi = np.uint32(s & np.uint64(0xFFFFFFFF)), np.uint32(s >> np.uint64(32))
        idx = np.arange(per_img, dtype=np.uint32)
        out = np.empty((N, per_img))
        p32 = float(np.float32(drop_p))
        for n in range(N):
            inner = _fin32(np.array([lo], dtype=np.uint32) + np.uint32(0x9E3779B9) * np.uint32(n + 1))
            h = _fin32(idx ^ inner ^ hi)
            u = (h >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
            out[n] = np.where(u >= p32, 1.0 / (1.0 - p32), 0.0)
    return torch.from_numpy(out)


def dact_of(yh, act, slope=SLOPE):
    """-> (act'(yh) from the OUTPUT yh, the sum of the absolute terms of that derivative)"""
    if act == "tanh":
        return 1 - yh * yh, 1 + yh * yh
    d = act_of(yh, act, slope)[1]
    return d, d


def ex_forward(y, mean_rstd, act, drop, slope=SLOPE):
    """act(drop(norm(y))) -> Fwd; drop: float64 [N, pixels, C] scale"""
    yh, _, amb = normalise(y, mean_rstd)
    v = yh * drop
    o, s = act_of(v, act, slope)
    return Fwd(o, s * v.abs(), amb)


def ex_backward(g1, g2, y, mean_rstd, act1, act2, drop, slope=SLOPE):
    """ghat = drop (g1 act1'(yhat) + g2 act2'(yhat)); dy as norm_core, or ghat without a norm. g1, g2: float64 slices"""
    yh, rstd, amb = normalise(y, mean_rstd)
    d1, t1 = dact_of(yh, act1, slope)
    gh, T_gh = g1 * d1, g1.abs() * t1
    if g2 is not None:
        d2, t2 = dact_of(yh, act2, slope)
        gh, T_gh = gh + g2 * d2, T_gh + g2.abs() * t2
    gh, T_gh = gh * drop, T_gh * drop
    if rstd is None:
        return Bwd(None, gh, T_gh, None, None, ambiguous=amb)
    dy, T_dy, bias, terms, sums = norm_core(gh, T_gh, yh, rstd)
    return Bwd(None, dy, T_dy, bias, terms, sums, amb)


# ---- the launch plan, restated from the numbers of a case (the branch tests compare it with `expect`) --------------------
def ceil_div(a, b):
    return -(-a // b)


def slot_sum_plan(N, slots, C):
    """slot_sum_kernel<R, CH>: narrow (CH = 4, 64 slot lanes) or wide (CH = 16, 16 lanes); the 4x-unrolled sweep runs when a
    lane has four slots, the tail when slots are left after the sweeps; idle: channels of the last workgroup beyond C; edge:
    some lane's fourth slot of a sweep would be the first slot past the end (it must take the tail instead)"""
    narrow = slots > 256 and N * ceil_div(C, 16) < 128
    lanes, ch = (64, 4) if narrow else (16, 16)
    sweep = tail = False
    for lane in range(lanes):                                        # each lane's walk over its slots
        sl = lane
        while sl + 3 * lanes < slots:
            sl, sweep = sl + 4 * lanes, True
        tail |= sl < slots
    return dict(narrow=narrow, sweep=sweep, tail=tail, idle=C % ch != 0, edge=slots % (4 * lanes) >= 3 * lanes)


def ordered_plan(slots):
    """slot_sum_ordered: eight slots at a time, then one by one"""
    return dict(unroll8=slots >= 8, tail=slots % 8 != 0)


def fwd_plan(N, hw, C):
    """gs_inorm_act_forward: the fixed-group path, and how many threads run 2 / 1 / 0 main iterations and the tail"""
    C8 = C // 8
    per = hw * C8
    bx = min(max(ceil_div(per, 2048), ceil_div(2048, N)), ceil_div(per, 256), 2048)
    stride = bx * 256
    main = lambda e0: 0 if e0 + stride >= per else ceil_div(per - stride - e0, 2 * stride)
    mains = {main(e0) for e0 in range(0, min(stride, per))}
    tails = {e0 + 2 * stride * main(e0) < per for e0 in range(0, min(stride, per))}
    return dict(fixed=256 % C8 == 0, stride=stride, per=per, mains=mains, tail=True in tails, no_tail=False in tails)


def cg_ppb(N, HW, C, cus):
    ppb = 64
    while ceil_div(HW, ppb) > 1024:
        ppb *= 2
    doubled = ppb > 64
    slots, per = cus * 6, (C // 64) * N
    bumped = False
    while ppb < 256 and per * ceil_div(HW, ppb) > slots and per * ceil_div(HW, ppb + 32) >= slots // 2:
        ppb += 32
        bumped = True
    return ppb, doubled, bumped


def stats_fwd_plan(N, hw, C, slots):
    fused = C % 64 == 0 and slots <= 64
    plan = dict(fused=fused)
    if fused:
        ppb = 64
        while ceil_div(hw, ppb) > 1024:
            ppb *= 2
        plan.update(ppb=ppb, groups=C // 64, last=hw - (ceil_div(hw, ppb) - 1) * ppb, **ordered_plan(slots))
    return plan


def fold_cnt(n, p):
    """the largest number of padded positions one unpadded position of an axis collects under reflection"""
    return max(1 + (1 <= x <= p) + (n - 1 - p <= x <= n - 2) for x in range(n)) if p else 1


def bwd_plan(N, sp, C, chunks, norm=True, cus=256, fold=0, mode="reflect"):
    """gs_inorm_act_backward from the chunk count of the reduction pass (the library's, or pre_slots)"""
    C8, HW = C // 8, math.prod(sp)
    cols = next((c for c in (32, 8, 4, 2) if C8 >= c), 1)
    plan = dict(cols=cols, ragged=C8 % cols != 0, shift=(C8 & (C8 - 1)) == 0 and C8 <= 256, cg=False,
                cnt=tuple(fold_cnt(n, fold) if mode == "reflect" else 1 for n in sp))
    if not norm:
        return plan
    plan["cg"] = C % 64 == 0 and chunks <= 64
    if plan["cg"]:
        ppb, doubled, bumped = cg_ppb(N, HW, C, cus)
        plan.update(ppb_cg=ppb, doubled=doubled, bumped=bumped, groups=C // 64,
                    last=HW - (ceil_div(HW, ppb) - 1) * ppb, **ordered_plan(chunks))
    else:
        plan.update(slot=slot_sum_plan(N, chunks, C), in_kernel_db=N == 1)
    return plan


# ---- the case tables ---------------------------------------------------------------------------------------------------
FINALIZE_CASES = [     # (N, slots, C, constant channel, reaches)
    (1, 1, 8, False, "minimal: one slot, one workgroup, no sweep"),
    (2, 70, 24, False, "CH = 16: unrolled sweep + tail (70 = 64 + 6), 8 idle columns in the second workgroup"),
    (1, 300, 24, False, "narrow CH = 4 (slots > 256, N ceil(C/16) = 2 < 128): sweep + tail (300 = 256 + 44)"),
    (1, 777, 100, False, "narrow, three sweeps + tail (777 = 768 + 9)"),
    (40, 300, 64, False, "slots > 256 but N ceil(C/16) = 160 >= 128: stays CH = 16, four sweeps + tail"),
    (2, 5, 16, True, "channel 3 constant with sum x^2 a hair short: var < 0 is clamped, rstd = eps^-1/2"),
    (2, 63, 24, False, "63 slots: lane 15 would read slot 63 as the fourth of its sweep (sl + 3 LANES == slots): tail instead"),
]
CONST_CHANNEL = 3


def finalize_inputs(i):
    """-> (flat fp32 partials, hw): 1 to 3 pixels per slot of x = m + sd * randn per channel"""
    N, slots, C, const, _ = FINALIZE_CASES[i]
    gen = torch.Generator().manual_seed(4100 + i)
    owner = torch.repeat_interleave(torch.arange(slots), torch.randint(1, 4, (slots,), generator=gen))
    hw = owner.numel()
    x = (torch.randn(N, hw, C, generator=gen) * (torch.rand(N, 1, C, generator=gen) + 0.3)
         + torch.randn(N, 1, C, generator=gen) * 1.5 + 0.4).float().double()
    if const:
        x[..., CONST_CHANNEL] = float(np.float32(1.1))
    part = partials_from(x, owner, slots)
    if const:
        part[:, :, 1, CONST_CHANNEL] *= 1 - 2.0 ** -20
    return part.reshape(-1).contiguous(), hw


ACTS = ("relu", "lrelu", "none")
FWD_CASES = [          # (name, shape, reaches, expect)
    ("tiny", (1, 5, 7, 8), "35 elements, one workgroup: tail only",
     dict(fixed=True, mains={0}, tail=True)),
    ("ragged", (64, 53, 53, 24), "non-fixed path (C8 = 3); stride 8192 < 8427 elements: one main iteration for e0 < 235 and "
     "no tail, tail only for the rest", dict(fixed=False, mains={0, 1}, tail=True, no_tail=True)),
    ("fixed", (64, 50, 63, 64), "fixed path; 25200 elements, stride 8192: two main iterations for e0 < 624, main + tail "
     "otherwise. 12.9 M scalars: ONE OF THE THREE LARGE CASES", dict(fixed=True, mains={1, 2}, tail=True, no_tail=True)),
]
FWD_RUNS = [(c[0], a, r) for c in FWD_CASES for a in ACTS for r in (False, True)]

STATS_FWD_CASES = [    # (name, shape, slots, reaches, expect)
    ("groups3", (2, 17, 13, 192), 19, "three channel groups (non-power-of-two block decode); last chunk 29 px (< 32 lanes); "
     "slot sum 8-unroll + tail", dict(fused=True, ppb=64, groups=3, last=29, unroll8=True, tail=True)),
    ("ppb128", (1, 257, 256, 64), 5, "ppb doubles to 128 and the px += 32 loop runs; fewer than 8 slots",
     dict(fused=True, ppb=128, groups=1, last=128, unroll8=False, tail=True)),
    ("slots64", (1, 9, 11, 64), 64, "the largest fused slot count, 8-unroll without a tail",
     dict(fused=True, ppb=64, groups=1, last=35, unroll8=True, tail=False)),
    ("slots65", (1, 9, 11, 64), 65, "falls back to two launches: slots > 64", dict(fused=False)),
    ("c72", (2, 9, 11, 72), 3, "falls back to two launches: C % 64 != 0", dict(fused=False)),
]


@dataclass(frozen=True)
class BCase:
    name: str
    shape: tuple              # (N, H, W, C) or (N, D, H, W, C)
    reaches: str
    expect: tuple             # items of the dict the plan must contain
    fold: int = 0
    mode: str = "reflect"
    act: str = "relu"
    chunks: int = 0           # of the reduction pass (gs_inorm_backward_scratch_floats), or pre_slots
    ppb: int = 0              # hip_ops.options(norm_bwd_ppb=...)
    pre: int = 0
    big: bool = False
    cus: int = 0              # the plan claimed holds on a device with this many compute units only

    @property
    def N(self):
        return self.shape[0]

    @property
    def sp(self):
        return self.shape[1:-1]

    @property
    def C(self):
        return self.shape[-1]

    @property
    def scalars(self):
        return math.prod(self.shape)


def _b(name, shape, reaches, fold=0, mode="reflect", act="relu", chunks=0, **kw):
    extra = {k: kw.pop(k) for k in ("ppb", "pre", "big", "cus") if k in kw}
    return BCase(name, shape, reaches, tuple(sorted(kw.items())), fold, mode, act, chunks, **extra)


BWD_CASES = [
    _b("r3_7x7", (1, 7, 7, 8), "reflect fold 3 with extent 2 fold + 1: cnt == 3 on both axes, 9 taps at the centre pixel",
       3, chunks=1, cols=1, cg=False, cnt=(3, 3), in_kernel_db=True),
    _b("r2_5x7", (1, 5, 7, 8), "cnt == 3 on one axis; N = 1: db inside the slot-sum kernel", 2, act="lrelu", chunks=1,
       cols=1, cg=False, cnt=(3, 2), in_kernel_db=True),
    _b("c24", (2, 9, 11, 24), "COLS 2 ragged (idle column), c8_shift = -1 (e / C8 and the c8 != c8h reload), N > 1: "
       "parameter-gradient launch", 1, chunks=2, cols=2, ragged=True, shift=False, cg=False, in_kernel_db=False),
    _b("c40", (2, 9, 11, 40), "COLS 4 ragged", act="none", chunks=2, cols=4, ragged=True, shift=False, cg=False),
    _b("c96", (1, 9, 11, 96), "COLS 8 ragged", act="lrelu", chunks=2, cols=8, ragged=True, shift=False, cg=False),
    _b("c320", (1, 9, 11, 320), "COLS 32 ragged; cg apply with 5 channel groups (non-power-of-two block decode)",
       chunks=2, cols=32, ragged=True, cg=True, groups=5, ppb_cg=64),
    _b("cg_f0", (2, 17, 13, 64), "cg apply, last chunk 29 px, no fold", 0, chunks=4, cg=True, last=29),
    _b("cg_f1", (2, 17, 13, 64), "cg apply, last chunk 29 px, fold 1", 1, act="lrelu", chunks=4, cg=True, last=29),
    _b("cg_f3", (2, 17, 13, 64), "cg apply, last chunk 29 px, fold 3", 3, act="none", chunks=4, cg=True, last=29),
    _b("r3d_f1", (1, 7, 8, 9, 64), "FM 2 (reflect 3-D), fold 1", 1, chunks=8, cg=True, cnt=(2, 2, 2)),
    _b("r3d_f3", (1, 7, 8, 9, 64), "FM 2, fold 3 with D = 7 = 2 fold + 1: cnt == 3 along depth", 3, act="lrelu", chunks=8,
       cg=True, cnt=(3, 2, 2)),
    _b("rep_f3", (1, 5, 6, 7, 16), "replicate fold 3: 64-tap corner", 3, "replicate", chunks=4, cols=2, cg=False),
    _b("bump", (4, 50, 80, 512), "256-CU device: the ppb += 32 bump gives 96 px per workgroup and the third pixel loop runs; "
       "8.2 M scalars: ONE OF THE THREE LARGE CASES", chunks=63, cg=True, ppb_cg=96, bumped=True, big=True, cus=256),
    _b("pre19", (1, 257, 256, 64), "pre_slots = 19 synthetic partials: cg apply with ppb 128 (doubled), slot sum 8-unroll + "
       "tail", act="lrelu", chunks=19, cg=True, ppb_cg=128, doubled=True, unroll8=True, tail=True, pre=19, big=True),
    _b("wide1", (1, 1024, 1100, 8), "default plan: ppb 320, 3520 slots: narrow slot_sum<3, 4> with sweep + tail; COLS 1 "
       "two-pixel loop; apply grid wraps; 9 M scalars: ONE OF THE THREE LARGE CASES", chunks=3520, cols=1, cg=False,
       slot=dict(narrow=True, sweep=True, tail=True, idle=False, edge=True), big=True),
    _b("ppb4", (1, 33, 32, 8), "norm_bwd_ppb = 4: 264 slots, the cheap route to the narrow slot sum (sweep + tail)",
       act="lrelu", chunks=264, ppb=4, cg=False, slot=dict(narrow=True, sweep=True, tail=True, idle=False, edge=False)),
    _b("ppb576_r64", (1, 30, 40, 32), "norm_bwd_ppb = 576: two-pixel loop at ROWS = 64", 1, chunks=3, ppb=576, cols=4,
       cg=False),
    _b("ppb576_r128", (1, 30, 40, 16), "norm_bwd_ppb = 576: two-pixel loop at ROWS = 128", act="none", chunks=3, ppb=576,
       cols=2, cg=False),
    _b("slots63", (2, 63, 64, 8), "63 slots through the wide slot_sum<3, 16>: sweep + tail, and lane 15 meets sl + 3 LANES == "
       "slots; N > 1", chunks=63, cols=1, cg=False, slot=dict(narrow=False, sweep=True, tail=True, idle=True, edge=True)),
]
BWD_BY_NAME = {c.name: c for c in BWD_CASES}


def _bwd_variants(c):
    """(stats, with g2 / gsum): both statistics modes, both with and without g2 / gsum; the no-norm form on the small
    cases. The cases above 2 M scalars take one run of each statistics mode (time)"""
    if c.big:
        return [("detuned", True), ("exact", False)]
    v = [(s, g) for s in STATS for g in (True, False)]
    return v + ([("none", True)] if not c.ppb else [])


BWD_RUNS = [(c.name, s, g) for c in BWD_CASES for s, g in _bwd_variants(c)]
BWD_SMALL = [c.name for c in BWD_CASES if c.scalars <= 40000]


def quantised(gen, *shape):
    """bf16 gradients that are multiples of 2^-6 below 4: any fp32 sum of up to 2^9 of them is exact. (+ 0.0: no negative
    zero among them, so that no sum is one either: a kernel that starts its sum from +0 returns +0 for -0 + -0)"""
    return ((torch.randn(*shape, generator=gen).clamp(-3.9, 3.9) * 64).round().div(64) + 0.0).to(BF16)


def stats_for(y, stats):
    mr = P.exact_stats(y, 0, y.shape[-1])
    if stats == "detuned":
        mr[:, 0] += DETUNE_MU
        mr[:, 1] *= DETUNE_RSTD
    return mr.reshape(-1).contiguous()


@dataclass
class BuiltB:
    case: BCase
    stats: str
    gpad: torch.Tensor
    g2: torch.Tensor
    y: torch.Tensor
    mean_rstd: torch.Tensor
    pre: tuple
    ref: Bwd


@lru_cache(maxsize=2)
def build_bwd(name, stats, with_g2):
    c = BWD_BY_NAME[name]
    gen = torch.Generator().manual_seed(2000 + 31 * BWD_CASES.index(c))
    y = (torch.randn(*c.shape, generator=gen) * 2 + 0.3).to(BF16)
    gpad = quantised(gen, c.N, *(n + 2 * c.fold for n in c.sp), c.C)
    g2 = quantised(gen, *c.shape) if with_g2 else None
    mr = stats_for(y, stats) if stats != "none" else None
    kw = dict(dims=c.sp, p=c.fold, mode=c.mode, act=c.act)
    pre = None
    if c.pre and mr is not None:
        # the partials of a producing launch: the exact sums dealt out to the slots with random weights, rounded to fp32,
        # followed by room for the totals
        s = backward(gpad, g2, y, mr, **kw).sums
        wgt = torch.rand(c.pre, generator=gen).double() + 0.5
        wgt = (wgt / wgt.sum()).view(1, c.pre, 1, 1)
        part = torch.stack([s["S1"], s["S2"], s["S3"]], 2) * wgt            # [N, slots, 3, C]
        scratch = torch.zeros(c.N * (c.pre + 1) * 3 * c.C)
        scratch[:c.N * c.pre * 3 * c.C] = part.float().reshape(-1)
        pre = (c.pre, scratch)
    return BuiltB(c, stats, gpad, g2, y, mr, pre, backward(gpad, g2, y, mr, pre=pre, **kw))


def run_bwd(ops, b, dev="cpu", bias=True, pre="case"):
    """one backward through RefOps or HipOps on guarded, NaN-filled outputs -> dict of CPU tensors and `guards`"""
    c = b.case
    to = lambda t: None if t is None else t.to(dev)
    dy, dy_w = guarded(c.shape, BF16, dev)
    gsum, gsum_w = guarded(c.shape, BF16, dev) if b.g2 is not None else (None, None)
    db = db_w = None
    if bias and b.mean_rstd is not None:
        db, db_w = guarded((c.C,), torch.float32, dev, torch.full((c.C,), BIAS_PREFILL))
    pre = b.pre if pre == "case" else pre
    pre = None if pre is None else (pre[0], to(pre[1].clone()))
    ops.inorm_act_backward(to(b.gpad), to(b.g2), to(b.y), to(b.mean_rstd), dy, gsum, fold=c.fold, fold_mode=c.mode,
                           act=c.act, slope=SLOPE, bias_grad=db, pre=pre)
    cpu = lambda t: None if t is None else t.cpu()
    return dict(dy=cpu(dy), gsum=cpu(gsum), bias=cpu(db),
                guards=all(guards_intact(w.cpu()) for w in (dy_w, gsum_w, db_w) if w is not None))


def measure_bwd(b, got, bias_terms=None):
    """-> {"dy": K-scale, "bias": K2-scale, "gsum_exact": bool}"""
    c = b.case
    shape = b.ref.dy.shape
    m = dict(dy=worst(bf16_excess(got["dy"].reshape(shape), b.ref.dy, b.ref.T_dy)))
    if got["gsum"] is not None:
        want = b.ref.g.float().to(BF16).reshape(c.shape)
        m["gsum_exact"] = torch.equal(got["gsum"].view(torch.int16), want.view(torch.int16))
    if got["bias"] is not None:
        terms = b.ref.bias_terms if bias_terms is None else bias_terms
        m["bias"] = worst(f32_excess(got["bias"].double() - BIAS_PREFILL, b.ref.bias, terms))
    return m


# ---- gs_norm_bias_grads ------------------------------------------------------------------------------------------------
DB_ITEMS = 33                                                  # two launches: 32 + 1
DB_CS, DB_NS = (8, 24, 300), (1, 3)


def bias_grads_inputs():
    """33 items (sums [N][3][C], mean_rstd [N][2][C], N, C, hw) with neighbours of different C, and their float64 result"""
    gen = torch.Generator().manual_seed(4300)
    items = []
    for i in range(DB_ITEMS):
        C, N, hw = DB_CS[i % 3], DB_NS[(i // 3) % 2], 50 + 7 * i
        sums = torch.randn(N, 3, C, generator=gen) * 20
        mr = torch.stack([torch.randn(N, C, generator=gen), torch.rand(N, C, generator=gen) + 0.5], 1)
        inv = float(np.float32(1.0 / hw))                      # the item carries 1 / hw as a float
        t = -mr[:, 1].double() * sums[:, 1].double() * sums[:, 2].double() * inv
        items.append(dict(sums=sums.reshape(-1).contiguous(), mr=mr.reshape(-1).contiguous(), N=N, C=C, hw=hw,
                          ref=t.sum(0), terms=t.abs().sum(0) + abs(BIAS_PREFILL)))
    return items


# ---- norm_ex.hip -------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ExCase:
    name: str
    shape: tuple              # (N, H, W, C)
    reaches: str
    norm: bool = True
    x2: bool = True
    g2: bool = True
    act1: str = "lrelu"
    act2: str = "relu"
    drop_p: float = 0.0
    seed_dev: bool = False
    fwd: bool = True
    cols: int = 1
    ragged: bool = False
    big: bool = False

    @property
    def C(self):
        return self.shape[-1]

    @property
    def widths(self):
        """channel stride and offset of every sliced operand: non-zero offsets in wider buffers, no two widths alike"""
        C = self.C
        return dict(x1=(C + 8, 8), x2=(2 * C + 24, C + 8), g1=(C + 24, 16), g2=(2 * C + 8, 8))


SEED, SEED_DEV = 0x1234567F9ABCDEF1, (0xFFFFFFF0, 0x7)          # the low words carry into the high word when added
EX_CASES = [
    ExCase("ex_cols1", (2, 5, 7, 8), "COLS 1: three of the four pipeline slots hold a valid pixel that is loaded and not "
           "used; dropout 0.5", drop_p=0.5),
    ExCase("ex_cols8", (2, 9, 11, 72), "COLS 8 ragged; x2 = None; drop_p = 0.3 (no power of two) with a device seed",
           x2=False, drop_p=0.3, seed_dev=True, cols=8, ragged=True),
    ExCase("ex_cols32", (1, 9, 11, 320), "COLS 32 ragged; N = 1: in-kernel db; g2 = None", g2=False, act1="relu", cols=32,
           ragged=True),
    ExCase("ex_copy", (2, 5, 7, 8), "mean_rstd = None, drop_p = 0, act1 none: x1 is a copy", norm=False, act1="none"),
    ExCase("ex_nonorm_drop", (2, 9, 11, 72), "mean_rstd = None with dropout 0.3", norm=False, drop_p=0.3, cols=8,
           ragged=True),
    ExCase("ex_wrap", (1, 419, 420, 24), "527940 elements of a non-power-of-two C8: forward (> 2048 * 256) and apply "
           "(> 1024 * 256) grids wrap; 2750 slots take the narrow slot sum; N = 1: in-kernel db", big=True),
    ExCase("ex_tanh", (2, 5, 7, 8), "backward only: act1 tanh without a norm, y holds bf16 tanh outputs: the general form of "
           "ex_ghat_from, with dropout", norm=False, act1="tanh", drop_p=0.5, fwd=False),
]
EX_BY_NAME = {c.name: c for c in EX_CASES}
EX_RUNS = [(c.name, s) for c in EX_CASES for s in (STATS if c.norm else ("none",))]


@dataclass
class BuiltEx:
    case: ExCase
    stats: str
    y: torch.Tensor
    g1: torch.Tensor
    g2: torch.Tensor
    x1_0: torch.Tensor
    x2_0: torch.Tensor
    mean_rstd: torch.Tensor
    drop: torch.Tensor
    f1: Fwd
    f2: Fwd
    ref: Bwd


def ex_view(t, key, c):
    cs, co = c.widths[key]
    return flat(t[..., co:co + c.C])


@lru_cache(maxsize=2)
def build_ex(name, stats):
    c = EX_BY_NAME[name]
    N, H, W, C = c.shape
    w = c.widths
    gen = torch.Generator().manual_seed(3000 + 13 * EX_CASES.index(c))
    rnd = lambda *s: torch.randn(*s, generator=gen)
    y = rnd(*c.shape) * 1.5 + 0.3
    y = (torch.tanh(y) if c.act1 == "tanh" else y).to(BF16)
    buf = lambda key, scale=1.0: (rnd(N, H, W, w[key][0]) * scale).to(BF16)
    g1, g2 = buf("g1"), (buf("g2") if c.g2 else None)
    x1_0, x2_0 = buf("x1", 3.0), (buf("x2", 3.0) if c.x2 else None)
    mr = stats_for(y, stats) if c.norm else None
    drop = drop_scale(N, H * W * C, c.drop_p, SEED, SEED_DEV if c.seed_dev else None).view(N, H * W, C)
    f1 = f2 = None
    if c.fwd:
        f1 = ex_forward(y, mr, c.act1, drop)
        f2 = ex_forward(y, mr, c.act2, drop) if c.x2 else None
    ref = ex_backward(ex_view(g1, "g1", c), ex_view(g2, "g2", c) if c.g2 else None, y, mr, c.act1, c.act2, drop)
    return BuiltEx(c, stats, y, g1, g2, x1_0, x2_0, mr, drop, f1, f2, ref)


def run_ex(ops, b, dev="cpu"):
    c, w = b.case, b.case.widths
    to = lambda t: None if t is None else t.to(dev)
    cpu = lambda t: None if t is None else t.cpu()
    kw = dict(act1=c.act1, act2=c.act2, slope=SLOPE, drop_p=c.drop_p, seed=SEED,
              seed_dev=torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in SEED_DEV], dtype=torch.int32,
                                    device=dev) if c.seed_dev else None)
    out = dict(x1=None, x2=None, bias=None)
    whole = []
    y, mr = to(b.y), to(b.mean_rstd)
    if c.fwd:
        x1, x1_w = guarded(b.x1_0.shape, BF16, dev, b.x1_0)
        x2, x2_w = guarded(b.x2_0.shape, BF16, dev, b.x2_0) if c.x2 else (None, None)
        ops.norm_act_forward_ex(y, mr, x1, x2, x1_co=w["x1"][1], x2_co=w["x2"][1] if c.x2 else 0, **kw)
        out.update(x1=cpu(x1), x2=cpu(x2))
        whole += [x1_w, x2_w]
    dy, dy_w = guarded(c.shape, BF16, dev)
    db = db_w = None
    if c.norm:
        db, db_w = guarded((c.C,), torch.float32, dev, torch.full((c.C,), BIAS_PREFILL))
    ops.norm_act_backward_ex(to(b.g1), to(b.g2), y, mr, dy, g1_co=w["g1"][1], g2_co=w["g2"][1] if c.g2 else 0,
                             bias_grad=db, **kw)
    out.update(dy=cpu(dy), bias=cpu(db))
    out["guards"] = all(guards_intact(t.cpu()) for t in whole + [dy_w, db_w] if t is not None)
    return out


def measure_ex(b, got, bias_terms=None):
    c, w = b.case, b.case.widths
    m, touched = {}, []
    for key, f, buf0 in (("x1", b.f1, b.x1_0), ("x2", b.f2, b.x2_0)):
        if got[key] is None:
            continue
        m[key] = worst(bf16_excess(ex_view(got[key], key, c), f.out, f.T))
        if not outside_untouched(got[key], buf0, w[key][1], c.C):
            touched.append(key)
    m["dy"] = worst(bf16_excess(flat(got["dy"]), b.ref.dy, b.ref.T_dy))
    if got["bias"] is not None:
        terms = b.ref.bias_terms if bias_terms is None else bias_terms
        m["bias"] = worst(f32_excess(got["bias"].double() - BIAS_PREFILL, b.ref.bias, terms))
    return m, touched


# ---- forward runs ------------------------------------------------------------------------------------------------------
FWD_BY_NAME = {c[0]: c for c in FWD_CASES}
STATS_FWD_BY_NAME = {c[0]: c for c in STATS_FWD_CASES}


@lru_cache(maxsize=1)
def fwd_inputs(name):
    """y, res (bf16) and the exact statistics of y rounded to fp32, shared by the six runs of a shape"""
    shape = FWD_BY_NAME[name][1]
    gen = torch.Generator().manual_seed(5000 + [c[0] for c in FWD_CASES].index(name))
    y = (torch.randn(*shape, generator=gen) * 2 + 0.3).to(BF16)
    res = torch.randn(*shape, generator=gen).to(BF16)
    return y, res, stats_for(y, "exact")


def forward_by_image(y, mean_rstd, res, act):
    """forward() one image at a time (the 12.9 M scalar case): -> Fwd over the whole batch"""
    N, C = y.shape[0], y.shape[-1]
    mr = mean_rstd.view(N, 2 * C)
    parts = [forward(y[n:n + 1], mr[n], None if res is None else res[n:n + 1], act) for n in range(N)]
    return Fwd(torch.cat([p.out for p in parts]), torch.cat([p.T for p in parts]), sum(p.ambiguous for p in parts))


def run_fwd(ops, name, act, with_res, dev="cpu"):
    """-> (worst excess of x, ambiguous, guards intact)"""
    y, res, mr = fwd_inputs(name)
    res = res if with_res else None
    to = lambda t: None if t is None else t.to(dev)
    x, x_w = guarded(y.shape, BF16, dev)
    ops.inorm_act_forward(to(y), to(mr), to(res), x, act=act, slope=SLOPE)
    f = forward_by_image(y, mr, res, act)
    return worst(bf16_excess(flat(x.cpu()), f.out, f.T)), f.ambiguous, guards_intact(x_w.cpu())


@lru_cache(maxsize=1)
def stats_fwd_inputs(name):
    _, shape, slots, _, _ = STATS_FWD_BY_NAME[name]
    gen = torch.Generator().manual_seed(5100 + [c[0] for c in STATS_FWD_CASES].index(name))
    y = (torch.randn(*shape, generator=gen) * 2 + 0.3).to(BF16)
    res = torch.randn(*shape, generator=gen).to(BF16)
    return y, res, partials_of(y, slots, gen)


def run_stats_fwd(ops, name, act, with_res, dev="cpu"):
    """the published statistics against finalize(), and x against forward() evaluated WITH the published statistics, so that a
    statistics error and an apply error cannot mask each other -> dict(mean=, rstd_inside=, x=, ambiguous=, guards=)"""
    _, shape, slots, _, expect = STATS_FWD_BY_NAME[name]
    y, res, part = stats_fwd_inputs(name)
    res = res if with_res else None
    N, C = shape[0], shape[-1]
    hw = math.prod(shape[1:-1])
    to = lambda t: None if t is None else t.to(dev)
    x, x_w = guarded(shape, BF16, dev)
    mr, mr_w = guarded((N * 2 * C,), torch.float32, dev)
    ops.inorm_stats_act_forward(to(y), to(part), slots, mr, to(res), x, act=act, slope=SLOPE, eps=1e-5)
    mr = mr.cpu()
    em, inside = finalize(part, N, slots, C, hw, inv_hw_f32=not expect["fused"]).check(mr.view(N, 2, C))
    f = forward(y, mr, res, act)
    return dict(mean=em, rstd_inside=inside, x=worst(bf16_excess(flat(x.cpu()), f.out, f.T)), ambiguous=f.ambiguous,
                guards=guards_intact(x_w.cpu()) and guards_intact(mr_w.cpu()))
