"""Integer-domain inputs, a plain float64 reference and the exactness precondition for the conv / dgrad / wgrad tests
(tests/test_exact_cpu.py, tests/test_exact_gpu.py).

bf16 holds every integer up to 256, the product of two of them is exact in fp32, and an fp32 sum of integers is exact in ANY
order (any split of K, any MFMA accumulation tree, any atomics order) as long as every partial sum stays below 2^24 in
magnitude. On such data kernel, oracle and a float64 reference must agree bit for bit, so `torch.equal` replaces a tolerance.

The float64 reference here is stated from the ConvSpec alone with torch.nn.functional (F.pad, F.conv*, F.conv_transpose*,
autograd for the two gradients). It does not import oracle/ops_ref.py and does not use the lowering (taps, packs, folds):
it is the independent third party.
"""
import torch
import torch.nn.functional as F

LIMIT = float(2 ** 24)          # fp32 holds every integer of smaller magnitude
BF16_INT = 256.0                # bf16 holds every integer of at most this magnitude


# ---- integer data ------------------------------------------------------------------------------------------------------
def ternary(shape, gen, density):
    """float32 tensor of {-1, 0, +1}; an element is non-zero with probability `density`"""
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    return sign * (torch.rand(shape, generator=gen) < density).float()


def int_values(shape, gen, density, mag):
    """ternary sign pattern times an integer magnitude in 1..mag"""
    return ternary(shape, gen, density) * torch.randint(1, mag + 1, shape, generator=gen).float()


def int_act(N, dims, c_real, c_pad, gen, density, mag, dtype=torch.bfloat16):
    """channels-last integer activation / gradient [N, *dims, c_pad]; zero in the padded channels like the randn tests"""
    assert mag <= BF16_INT
    t = torch.zeros(N, *dims, c_pad, dtype=dtype)
    t[..., :c_real] = int_values((N, *dims, c_real), gen, density, mag).to(dtype)
    return t


_LADDER = [(0.5, 0.5, 3), (0.5, 0.25, 3), (0.25, 0.25, 3), (0.25, 0.25, 1), (0.25, 0.125, 1), (0.125, 0.125, 1),
           (0.125, 0.0625, 1), (0.0625, 0.0625, 1), (0.0625, 0.03125, 1), (0.03125, 0.03125, 1)]


def domain(spec, N, sizes, rounding=False):
    """densities and magnitudes of one case: dict(dx, dw, mag, dg, gmag) — activations non-zero with probability dx and of
    magnitude 1..mag, ternary weights of density dw, output gradients of density dg and magnitude 1..gmag. Chosen from the
    layer shape alone so that the reference is expected to satisfy assert_exact_domain: an output is a sum of about
    K * dx * dw non-zero products of variance E[m^2] (m uniform in 1..mag: 14/3 for mag 3), and the tightest bounds are
    max |y| <= 256 (variance <= 1024: 256 is 8 sigma) and sum(y^2) per (image, channel) < 2^24 (variance <= 2^23 / pixels:
    a factor 2 of room, 16 set aside for the squared bias). Richest admissible step of the ladder; the gradient's density
    by the same rule on the transposed operation (a quarter of the variance where a pad layer folds up to four values of
    the gradient into one in the 2-D ring form)."""
    taps = spec.k ** spec.dims
    per_out = max(1, taps // spec.stride ** spec.dims)
    Kf = (taps if spec.kind == "conv" else per_out) * spec.cin
    Kd = (per_out if spec.kind == "conv" else taps) * spec.cout
    if rounding:
        # outputs in the thousands (sigma about 700: variance K * dx * dw * mag^2 / 3 = 5e5), where bf16 keeps 8 of their 10-12
        # bits: only the conv-on-magnitudes bound applies (about K * dx * dw * mag / 2, some 1e4), outputs are compared alone
        mag = min(int(BF16_INT), int((5e5 * 3 / (Kf * 0.25)) ** 0.5) + 1)
        return dict(dx=0.5, dw=0.5, mag=mag, dg=0.25, gmag=3)
    pixels = 1
    for x in spec.out_hw(*sizes):
        pixels *= x
    budget = min(1024.0, 2 ** 23 / pixels - 16)
    em2 = lambda m: 14 / 3 if m == 3 else 1
    for dx, dw, mag in _LADDER:
        if Kf * dx * dw * em2(mag) <= budget:
            break
    else:
        raise AssertionError(f"no integer domain for {spec} at {N} x {sizes}")
    gbudget = 1024.0 / (1 if spec.pad_mode == "zero" else 4)
    for dg, gmag in ((0.5, 3), (0.25, 3), (0.25, 1), (0.125, 1), (0.0625, 1), (0.03125, 1), (0.015625, 1)):
        if Kd * dg * dw * em2(gmag) <= gbudget:
            break
    else:
        raise AssertionError(f"no integer gradient domain for {spec} at {N} x {sizes}")
    return dict(dx=dx, dw=dw, mag=mag, dg=dg, gmag=gmag)


def int_weights(spec, seed, density, bias_mag=3):
    """(weight in torch layout OI[D]HW / IO[D]HW, bias [cout]): ternary weights, integer bias in [-bias_mag, bias_mag]"""
    g = torch.Generator().manual_seed(seed)
    w = ternary(spec.torch_weight_shape(), g, density)
    b = torch.randint(-bias_mag, bias_mag + 1, (spec.cout,), generator=g).float()
    return w, b


def int_layer(spec, sizes, seed, density=0.25, bias_mag=3):
    """the integer twin of test_ops_gpu.make_layer, same returns: (low, master, bias, fpack, dpack); the weight in torch
    layout is int_weights(spec, seed, density, bias_mag)[0]."""
    from ganslate_amd.nn.native.spec import lower
    from oracle.ops_ref import RefOps
    low = lower(spec, *sizes)
    w, b = int_weights(spec, seed, density, bias_mag)
    master = spec.master_from_torch(w)
    bias = torch.zeros(spec.cout_p)
    bias[:spec.cout] = b
    ref = RefOps()
    fpack = torch.empty(low.fwd_index.size, dtype=torch.bfloat16)
    ref.repack(master, torch.from_numpy(low.fwd_index), fpack)
    dpack = torch.empty(low.dgrad_index.size, dtype=torch.bfloat16)
    ref.repack(master, torch.from_numpy(low.dgrad_index), dpack)
    return low, master, bias, fpack, dpack


# ---- float64 reference, from the ConvSpec alone ----------------------------------------------------------------------------
def _cf(t):
    """channels-last [N, *dims, C] -> float64 [N, C, *dims]"""
    return t.double().movedim(-1, 1).contiguous()


def _cl(t):
    return t.movedim(1, -1).contiguous()


def cin_of(spec):
    """channels of the conv that runs: a W-folded layer is stated as the folded conv itself (vertical taps over folded channels)"""
    return spec.cin_p if spec.wfold else spec.cin


def cout_of(spec):
    return spec.cout_p if spec.wfold else spec.cout


def ref_weight(spec, master):
    """the weight the float64 reference takes: torch layout OI[D]HW / IO[D]HW; for a W-folded spec the folded conv's own
    [cout_p][cin_p][k]([k])[1] kernel (the master [P][T][Q] with the tap axis unrolled over the un-folded axes)"""
    if not spec.wfold:
        return spec.torch_from_master(master)
    return master.reshape(spec.P, spec.T, spec.Q).permute(0, 2, 1).reshape(spec.P, spec.Q, *(spec.k,) * (spec.dims - 1), 1)


def master_of(spec, w):
    """inverse of ref_weight: reference weight (gradient) -> padded master [P][T][Q]"""
    if not spec.wfold:
        return spec.master_from_torch(w)
    return w.reshape(spec.P, spec.Q, spec.T).permute(0, 2, 1).contiguous()


def _pad(spec, x):
    """the explicit pad layer of a conv with a reflect / replicate border (zero borders stay with the conv call). W-folded: the
    W border was applied by the unfold ("in": none here) or is part of the folded domain ("out": all W + 2 pad columns)"""
    if spec.pad_mode == "zero" or spec.pad == 0:
        assert not spec.wfold
        return x
    if spec.wfold:
        pw = spec.pad if spec.wfold == "out" else 0
        return F.pad(x, (pw, pw) + (spec.pad,) * (2 * spec.dims - 2), mode=spec.pad_mode)
    return F.pad(x, (spec.pad,) * (2 * spec.dims), mode=spec.pad_mode)


def _conv(spec, xp, w, b):
    """xp: input AFTER the explicit pad layer, channels first, float64"""
    if spec.kind == "conv":
        f = F.conv2d if spec.dims == 2 else F.conv3d
        return f(xp, w, b, stride=spec.stride, padding=spec.pad if spec.pad_mode == "zero" else 0)
    f = F.conv_transpose2d if spec.dims == 2 else F.conv_transpose3d
    return f(xp, w, b, stride=spec.stride, padding=spec.pad, output_padding=spec.out_pad)


def conv_ref64(spec, x, w, bias):
    """x channels-last [N, *sizes, >= cin] (real channels first), w as ref_weight gives it, bias [cout] or None
    -> float64 channels-last [N, *out, cout]"""
    b = None if bias is None else bias[:cout_of(spec)].double()
    return _cl(_conv(spec, _pad(spec, _cf(x[..., :cin_of(spec)])), w.double(), b))


def dgrad_ref64(spec, sizes, gy, w, folded=False):
    """gradient of the layer with respect to its input, channels-last float64 with cin channels: on the domain AFTER the
    explicit pad layer (what the data-gradient launch of a reflect / replicate layer writes; the consumer applies the pad
    adjoint), or with folded=True through the pad layer onto the layer's own input"""
    N = gy.shape[0]
    x = torch.zeros(N, cin_of(spec), *sizes, dtype=torch.float64, requires_grad=True)
    xp = _pad(spec, x)
    if not folded and xp is not x:
        xp = torch.zeros(xp.shape, dtype=torch.float64, requires_grad=True)
    y = _conv(spec, xp, w.double(), None)
    gx, = torch.autograd.grad(y, x if folded or xp is x else xp, _cf(gy[..., :cout_of(spec)]))
    return _cl(gx)


def wgrad_ref64(spec, x, gy):
    """gradient with respect to the weight, in ref_weight's layout, float64"""
    shape = ref_weight(spec, torch.zeros(spec.master_numel)).shape
    w = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    y = _conv(spec, _pad(spec, _cf(x[..., :cin_of(spec)])), w, None)
    gw, = torch.autograd.grad(y, w, _cf(gy[..., :cout_of(spec)]))
    return gw


def bias_grad_ref64(spec, gy):
    return gy[..., :cout_of(spec)].double().reshape(-1, cout_of(spec)).sum(0)


def rne_bf16(t64):
    """the one documented storage rounding: float64 integers below 2^24 are exact in fp32, fp32 -> bf16 rounds to nearest even"""
    return t64.float().to(torch.bfloat16)


# ---- the precondition -----------------------------------------------------------------------------------------------------
def assert_exact_domain(spec, *, x=None, w=None, bias=None, gy=None, sizes=None, stats=False, stored_exact=True, prefill=0.0,
                        folded=False, fused=None):
    """Fails unless the float64 reference ALONE shows that every fp32 partial sum of every summation order is an integer
    below 2^24: the same operation on magnitudes bounds them. Checked, whichever operands are given:
      forward (x, w[, bias])     conv(|x|, |w|, |bias|) < 2^24; stored_exact: max |y| + prefill <= 256 (bf16 holds the integer);
                                 stats: sum(y^2) per (image, channel) < 2^24 (>= sum |y|: the values are integers)
      dgrad (gy, w, sizes)       the transposed conv on magnitudes < 2^24; stored_exact: max |gx| <= 256 (folded: through the
                                 pad layer, as the ring form stores it)
      wgrad (x, gy)              sum |a| * |g| per weight element + prefill < 2^24; bias gradient: sum |gy| per channel + prefill
      fused = (gh, yh)           the norm-backward sums: sum |gh|, sum |gh * yh|, sum |yh| per (image, channel) < 2^24
    Returns the measured bounds (for the record; nothing is derived from code under test)."""
    out = {}
    for name, t in (("x", x), ("w", w), ("bias", bias), ("gy", gy)):
        if t is not None:
            td = t.double()
            assert torch.equal(td, td.round()) and td.abs().max().item() <= BF16_INT, f"{name} is not bf16-exact integer data"
    if x is not None and w is not None:
        y = conv_ref64(spec, x, w, bias)
        bound = conv_ref64(spec, x.abs(), w.abs(), None if bias is None else bias.abs()).max().item()
        out["fwd_sum_abs"], out["fwd_max"] = bound, y.abs().max().item()
        assert bound + prefill < LIMIT, f"forward: sum of |products| {bound} reaches 2^24"
        if stored_exact:
            assert out["fwd_max"] + prefill <= BF16_INT, f"forward: max |y| {out['fwd_max']} is not a bf16 integer"
        if stats:
            sq = (y * y).reshape(y.shape[0], -1, y.shape[-1]).sum(1).max().item()
            out["stats_sumsq"] = sq
            assert sq < LIMIT, f"statistics: sum of squares {sq} reaches 2^24"
    if gy is not None and w is not None:
        assert sizes is not None
        gx = dgrad_ref64(spec, sizes, gy, w, folded)
        bound = dgrad_ref64(spec, sizes, gy.abs(), w.abs(), folded).max().item()
        out["dgrad_sum_abs"], out["dgrad_max"] = bound, gx.abs().max().item()
        assert bound < LIMIT, f"dgrad: sum of |products| {bound} reaches 2^24"
        if stored_exact:
            assert out["dgrad_max"] <= BF16_INT, f"dgrad: max |gx| {out['dgrad_max']} is not a bf16 integer"
    if gy is not None and x is not None:
        bound = wgrad_ref64(spec, x.abs(), gy.abs()).max().item() + prefill
        out["wgrad_sum_abs"] = bound
        assert bound < LIMIT, f"wgrad: sum of |a| * |g| {bound} reaches 2^24"
        bb = bias_grad_ref64(spec, gy.abs()).max().item() + prefill
        out["bias_grad_sum_abs"] = bb
        assert bb < LIMIT, f"bias gradient: sum of |gy| {bb} reaches 2^24"
    if fused is not None:
        gh, yh = (t.double() for t in fused)
        n, c = gh.shape[0], gh.shape[-1]
        for name, t in (("gh", gh.abs()), ("gh*yh", (gh * yh).abs()), ("yh", yh.abs())):
            assert torch.equal(t, t.round()), f"fused sums: {name} is not integer"
            s = t.reshape(n, -1, c).sum(1).max().item()
            out[f"fused_{name}"] = s
            assert s < LIMIT, f"fused norm sums: sum |{name}| {s} reaches 2^24"
    return out


# ---- one case, checked ------------------------------------------------------------------------------------------------------
_CASES = {}


class Case:
    """a layer on the integer domain with its operands (xa: input, gy: output gradient, both channels-last bf16 with zero padded
    channels), already through assert_exact_domain (`bounds` holds what the reference measured)"""


def make_case(spec, N, sizes, seed=1, rounding=False, stats=True, prefill=0.0, check=("fwd", "dgrad", "wgrad")):
    """the case of (spec, N, sizes, seed), built once per process. A W-folded spec is the folded conv itself: operands on the
    folded layer's own domains (Lowered.in_dims / out_dims) with every folded channel live, c.w its [cout_p][cin_p][k]([k])[1]
    kernel, c.b its bias over cout_p channels — stated by the same float64 reference and through the same precondition."""
    key = (repr(spec), N, tuple(sizes), seed, rounding, stats, prefill, tuple(check))
    if key in _CASES:
        return _CASES[key]
    c = Case()
    c.spec, c.N, c.sizes, c.dom = spec, N, tuple(sizes), domain(spec, N, sizes, rounding)
    d = c.dom
    c.low, c.master, c.bias, c.fpack, c.dpack = int_layer(spec, sizes, seed, d["dw"])
    low = c.low
    c.w, c.b = ref_weight(spec, c.master), c.bias[:cout_of(spec)].clone()
    g = torch.Generator().manual_seed(seed + 1000)
    c.bounds = {}
    if spec.wfold:
        c.xa = int_act(N, low.in_dims, spec.cin_p, spec.cin_p, g, d["dx"], d["mag"])
        c.gy = int_act(N, low.out_dims, spec.cout_p, spec.cout_p, g, d["dg"], d["gmag"])
    else:
        c.xa = int_act(N, sizes, spec.cin, spec.cin_p, g, d["dx"], d["mag"])
        c.gy = int_act(N, low.out_dims, spec.cout, spec.cout_p, g, d["dg"], d["gmag"])
    if "fwd" in check:
        c.bounds.update(assert_exact_domain(spec, x=c.xa, w=c.w, bias=c.b, stats=stats and not rounding,
                                            stored_exact=not rounding, prefill=prefill))
    if "dgrad" in check:
        c.bounds.update(assert_exact_domain(spec, gy=c.gy, w=c.w, sizes=sizes))
    if "wgrad" in check:
        c.bounds.update(assert_exact_domain(spec, x=c.xa, gy=c.gy, prefill=prefill))
    _CASES[key] = c
    return c


# ---- reporting a mismatch (a finding, not noise) --------------------------------------------------------------------------
def first_mismatch(got, want):
    """None, or (coordinates, got, want, number of differing elements) of the first differing element (NaN differs from NaN
    only where the other side is not NaN)"""
    g, r = got.detach().cpu(), want.detach().cpu()
    assert g.shape == r.shape, (g.shape, r.shape)
    bad = (g != r) & ~(torch.isnan(g) & torch.isnan(r))
    if not bool(bad.any()):
        return None
    at = tuple(int(v) for v in bad.nonzero()[0])
    return at, g[at].item(), r[at].item(), int(bad.sum())


def tap_decomposition(spec, x, w, bias, at):
    """per-tap contributions (summed over input channels) of the float64 reference at output coordinate
    at = (image, [z,] y, x, channel) of a forward conv; the pattern names the table at fault"""
    if spec.kind != "conv" or spec.wfold or at[-1] >= spec.cout:
        return "(no tap decomposition: transposed or W-folded conv, or padded channel)"
    xp = _pad(spec, _cf(x[..., :spec.cin]))
    if spec.pad_mode == "zero" and spec.pad:
        xp = F.pad(xp, (spec.pad,) * (2 * spec.dims))
    n, pos, co = at[0], at[1:-1], at[-1]
    sl = tuple(slice(p * spec.stride, p * spec.stride + spec.k) for p in pos)
    contrib = (xp[(n, slice(None)) + sl] * w[co].double()).sum(0)
    return f"bias {0.0 if bias is None else float(bias[co])}, taps (summed over input channels):\n{contrib}"


def assert_identical(got, want, what, decompose=None):
    """torch.equal with a report: first differing coordinates (image, [z,] y, x, channel), got, want, and for a forward conv
    the tap-level decomposition of the reference at that pixel (decompose = (spec, x, w, bias))"""
    m = first_mismatch(got, want)
    if m is None:
        return
    at, g, r, n = m
    msg = f"{what}: {n} of {got.numel()} elements differ; first at {at}: got {g!r}, want {r!r}"
    if decompose is not None and len(at) == decompose[0].dims + 2:
        msg += "\n" + tap_decomposition(*decompose, at)
    raise AssertionError(msg)
