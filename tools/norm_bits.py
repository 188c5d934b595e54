#!/usr/bin/env python
"""Digests of everything the elementwise-norm entry points (csrc/norm.hip, norm_ex.hip, prelu.hip) write, on fixed seeded inputs:

    GANSLATE_HIP_LIB=<library> python tools/norm_bits.py > digests.json

Run it once per build of the library, each in its own process, and compare the files: one sha256 per output tensor, so a
refactor of those files that claims bit identity has every digest equal. The cases are small and chosen so that every kernel
instantiation and every host branch is launched: channel counts for every column count of the reduce kernels and both forms of
the pixel index, the four fold modes, pixel counts off every tile size, few and many chunks, one and two images, all options
of the V-Net and U-Net descriptors, and parameter-gradient buffers that are not zero before the call."""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from ganslate_amd.hip import lib as L  # noqa: E402
from ganslate_amd.hip import ops as O  # noqa: E402

GEN = torch.Generator().manual_seed(20240607)
OUT = {}


def rnd(*shape, dtype=torch.bfloat16, scale=1.0):
    return (torch.randn(*shape, generator=GEN) * scale).to(dtype).cuda()


def put(name, **tensors):
    torch.cuda.synchronize()
    for key, t in tensors.items():
        if t is not None:
            raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
            assert f"{name}/{key}" not in OUT, name
            OUT[f"{name}/{key}"] = hashlib.sha256(raw).hexdigest()


def stats(ops, y):
    """mean / rstd [N][2][C] of y through gs_inorm_finalize on one slot of exact sums"""
    N, Cc = y.shape[0], y.shape[-1]
    f = y.float().reshape(N, -1, Cc)
    part = torch.stack([f.sum(1), (f * f).sum(1)], 1).reshape(-1).contiguous()
    mr = torch.zeros(N * 2 * Cc, device=y.device)
    ops.inorm_finalize(part, N, 1, Cc, f.shape[1], mr)
    return mr


def inorm_cases(ops):
    for N, slots, Cc in ((1, 1, 8), (2, 7, 264), (1, 300, 8), (2, 300, 32), (8, 300, 256)):     # CH = 16 and CH = 4 forms
        mr = torch.zeros(N * 2 * Cc, device="cuda")
        ops.inorm_finalize(rnd(N * slots * 2 * Cc, dtype=torch.float32).abs(), N, slots, Cc, 1000, mr)
        put(f"inorm_finalize/N{N}s{slots}C{Cc}", mean_rstd=mr)
    for i, (shape, act, with_res) in enumerate((((1, 5, 7, 8), "relu", False), ((2, 17, 13, 64), "lrelu", True),
                                                ((2, 17, 13, 264), "none", True), ((1, 5, 7, 192), "relu", False),
                                                ((1, 3, 5, 7, 16), "none", True), ((8, 64, 64, 256), "relu", True))):
        y, res = rnd(*shape), rnd(*shape) if with_res else None
        x = torch.zeros_like(y)
        ops.inorm_act_forward(y, stats(ops, y), res, x, act=act)
        put(f"inorm_act_forward/{i}", x=x)
    for i, (shape, slots, act, with_res) in enumerate((((2, 5, 7, 64), 16, "relu", True), ((1, 17, 13, 256), 3, "none", False),
                                                       ((1, 9, 9, 32), 4, "relu", False), ((2, 9, 9, 64), 65, "lrelu", True),
                                                       ((1, 300, 300, 64), 64, "relu", False))):
        y, res = rnd(*shape), rnd(*shape) if with_res else None
        N, Cc = shape[0], shape[-1]
        hw = y.numel() // (N * Cc)
        part = rnd(N * slots * 2 * Cc, dtype=torch.float32).abs() * (hw / slots)
        mr, x = torch.zeros(N * 2 * Cc, device="cuda"), torch.zeros_like(y)
        ops.inorm_stats_act_forward(y, part, slots, mr, res, x, act=act)
        put(f"inorm_stats_act_forward/{i}", x=x, mean_rstd=mr)


def inorm_backward(ops, name, shape, fold, fold_mode, act, with_g2, with_gsum, with_db, norm=True, pre_slots=0):
    N, Cc = shape[0], shape[-1]
    sp = tuple(shape[1:-1])
    pad = tuple(s + 2 * fold if (len(sp) == 2 or len(sp) == 3 and (i > 0 or s > 1)) else s for i, s in enumerate(sp))
    y, gpad = rnd(*shape), rnd(N, *pad, Cc)
    g2 = rnd(*shape) if with_g2 else None
    dy = torch.zeros_like(y)
    gsum = torch.zeros_like(y) if with_gsum else None
    db = rnd(Cc, dtype=torch.float32) if with_db else None
    mr = stats(ops, y) if norm else None
    pre = None
    if pre_slots:
        pre = (pre_slots, torch.cat([rnd(N * pre_slots * 3 * Cc, dtype=torch.float32), torch.zeros(N * 3 * Cc, device="cuda")]))
    D, H, W = (1,) * (3 - len(sp)) + sp
    if norm and not pre_slots:      # the wrapper's scratch is torch.empty: a zeroed one of the same size, so all of it can be hashed
        pre_scratch = torch.zeros(ops.lib.gs_inorm_backward_scratch_floats(N, D, H, W, Cc), device="cuda")
        L.check(ops.lib.gs_inorm_act_backward(O._ptr(gpad), O._ptr(g2), O._ptr(y), O._ptr(mr), O._ptr(dy), O._ptr(gsum),
                                              O._ptr(pre_scratch), O._ptr(db), N, D, H, W, Cc, fold, L.BORDER[fold_mode],
                                              L.ACT[act], 0.2, 0, O._stream()), "gs_inorm_act_backward")
        scratch = pre_scratch
    else:
        r = ops.inorm_act_backward(gpad, g2, y, mr, dy, gsum, fold=fold, fold_mode=fold_mode, act=act, bias_grad=db, pre=pre)
        scratch = r[0] if r else None
    sums = scratch[scratch.numel() - N * 3 * Cc:] if scratch is not None else None
    partial = scratch[:scratch.numel() - N * 3 * Cc] if scratch is not None and not pre_slots else None
    put(name, dy=dy, gsum=gsum, bias_grad=db, sums=sums, partial=partial)


def inorm_backward_cases(ops):
    folds = ((0, "reflect"), (1, "reflect"), (2, "reflect"), (1, "replicate"))      # fold modes 0, 1, 2 (on volumes), 3
    k = 0
    for Cc in (8, 16, 32, 64, 256, 264, 192):                # COLS 1 / 2 / 4 / 8 / 32 / 32 / 8; 264, 192: no shift form
        for fm in range(4):
            fold, mode = folds[fm]
            N = 1 + (k & 1)
            shape = (N, 5, 7, Cc) if fm == 0 else (N, 17, 13, Cc) if fm == 1 else (N, 5, 6, 7, Cc)
            inorm_backward(ops, f"inorm_act_backward/C{Cc}fm{fm}", shape, fold, mode, ("relu", "lrelu", "none")[k % 3],
                           with_g2=bool(k & 2), with_gsum=bool(k & 4) or fm == 0, with_db=True)
            k += 1
    # more than 64 chunks at C % 64 == 0: the slot-sum + apply route for wide layers, every fold mode, one and two images
    for fm, shape in ((0, (1, 72, 72, 64)), (1, (2, 72, 72, 64)), (2, (1, 12, 20, 24, 64)), (3, (2, 12, 20, 24, 128))):
        inorm_backward(ops, f"inorm_act_backward/many_chunks_fm{fm}", shape, folds[fm][0] and 1, folds[fm][1], "relu",
                       with_g2=fm == 1, with_gsum=fm == 2, with_db=True)
    # more than 256 slots at few channels: 4 channels per workgroup in the slot sum
    inorm_backward(ops, "inorm_act_backward/vol_C8", (1, 24, 24, 32, 8), 1, "replicate", "relu", False, False, True)
    inorm_backward(ops, "inorm_act_backward/vol_C16_fold3", (1, 24, 24, 32, 16), 3, "replicate", "lrelu", True, False, True)
    # the residual-block shape: more workgroups than one round of the channel-group apply kernel
    inorm_backward(ops, "inorm_act_backward/trunk", (8, 64, 64, 256), 1, "reflect", "relu", True, True, False)
    inorm_backward(ops, "inorm_act_backward/flat_volume", (1, 1, 9, 11, 16), 1, "replicate", "relu", False, True, True)
    inorm_backward(ops, "inorm_act_backward/no_norm", (2, 17, 13, 24), 1, "reflect", "lrelu", True, True, False, norm=False)
    # C8 = 512, a power of two above 256: the element-loop apply kernel takes the division form of the pixel index
    inorm_backward(ops, "inorm_act_backward/no_norm_C4096", (1, 5, 7, 4096), 1, "reflect", "relu", False, True, False, norm=False)
    inorm_backward(ops, "inorm_act_backward/many_chunks_C4096", (1, 72, 72, 4096), 0, "reflect", "relu", False, False, True)
    inorm_backward(ops, "inorm_act_backward/pre_slots_cg", (2, 16, 16, 64), 1, "reflect", "relu", False, False, True, pre_slots=4)
    inorm_backward(ops, "inorm_act_backward/pre_slots", (1, 16, 16, 32), 0, "reflect", "relu", False, False, True, pre_slots=300)
    # gs_norm_bias_grads over two layers
    items, dbs = [], []
    for N, Cc, hw in ((2, 64, 35), (1, 264, 221)):
        holder, mr, db = rnd(5 + N * 3 * Cc, dtype=torch.float32), rnd(N * 2 * Cc, dtype=torch.float32), rnd(Cc, dtype=torch.float32)
        items.append((holder, 5, mr, db, N, Cc, hw))
        dbs.append(db)
    ops.norm_bias_grads(items)
    put("norm_bias_grads", db0=dbs[0], db1=dbs[1])


def norm_ex_cases(ops):
    k = 0
    for Cc in (8, 32, 64, 256, 264):                          # COLS 1 / 1 / 8 / 32 / 32
        for N, H, W in ((1, 5, 7), (2, 17, 13)):
            for act1, act2, drop in (("lrelu", "relu", 0.0), ("tanh", "none", 0.5), ("relu", "lrelu", 0.5)):
                norm, two = bool(k % 4), bool(k % 3)
                y = rnd(N, H, W, Cc)
                mr = stats(ops, y) if norm else None
                x1 = torch.zeros(N, H, W, Cc + 16, dtype=torch.bfloat16, device="cuda")
                x2 = torch.zeros(N, H, W, 2 * Cc, dtype=torch.bfloat16, device="cuda") if two else None
                seed_dev = torch.tensor([k, 7], dtype=torch.int32, device="cuda") if k & 1 else None
                ops.norm_act_forward_ex(y, mr, x1, x2, act1=act1, act2=act2, x1_co=8, x2_co=Cc, drop_p=drop, seed=1234 + k,
                                        seed_dev=seed_dev)
                put(f"norm_act_forward_ex/{k}", x1=x1, x2=x2)
                g1 = rnd(N, H, W, Cc + 8)
                g2 = rnd(N, H, W, 2 * Cc) if two else None
                dy = torch.zeros_like(y)
                db = rnd(Cc, dtype=torch.float32) if norm else None
                d = ops._norm_ex_desc(y, act1, act2, 0.2, drop, 1234 + k, seed_dev)
                d.g1_cs, d.g1_co = g1.shape[-1], 8
                if two:
                    d.g2_cs, d.g2_co = g2.shape[-1], Cc
                scratch = torch.zeros(ops.lib.gs_norm_backward_ex_scratch_floats(C.byref(d)), device="cuda") if norm else None
                L.check(ops.lib.gs_norm_act_backward_ex(C.byref(d), O._ptr(g1), O._ptr(g2), O._ptr(y), O._ptr(mr), O._ptr(dy),
                                                        O._ptr(scratch), O._ptr(db), O._stream()), "gs_norm_act_backward_ex")
                put(f"norm_act_backward_ex/{k}", dy=dy, bias_grad=db, scratch=scratch)
                k += 1


def pnorm_backward(ops, name, N, sp, Cc, res_mode, res_mod, norm, with_slope, with_g2, with_gres):
    wide = Cc + 16
    y, g = rnd(N, *sp, wide), rnd(N, *sp, wide)
    g2 = rnd(N, *sp, Cc) if with_g2 else None
    res = None
    if res_mode:
        res = rnd(N, *sp, res_mod if res_mod else wide)
    mr = stats(ops, y[..., 8:8 + Cc].contiguous()) if norm else None
    slope = rnd(Cc, dtype=torch.float32, scale=0.25) if with_slope else None
    out = torch.zeros(N, *sp, wide, dtype=torch.bfloat16, device="cuda")
    ops.pnorm_forward(y, mr, out, C=Cc, slope=slope, res=res, res_mode=res_mode, res_mod=res_mod, y_co=8,
                      res_co=0 if res_mod else 16, out_co=16)
    put(name + "/forward", out=out)
    dy = torch.zeros(N, *sp, wide, dtype=torch.bfloat16, device="cuda")
    gres = torch.zeros(N, *sp, Cc, dtype=torch.bfloat16, device="cuda") if with_gres else None
    dslope = rnd(Cc, dtype=torch.float32) if with_slope else None
    db = rnd(Cc, dtype=torch.float32) if norm else None
    d = ops._pdesc(y, Cc, 8, res, res_mode, res_mod, 0 if res_mod else 16)
    d.g_cs, d.g_co = wide, 16
    if with_g2:
        d.g2_cs, d.g2_co = Cc, 0
    d.dy_cs, d.dy_co = wide, 0
    if with_gres:
        d.gres_cs, d.gres_co = Cc, 0
    scratch = None
    if norm or with_slope:
        scratch = torch.zeros(ops.lib.gs_pnorm_backward_scratch_floats(C.byref(d)), device="cuda")
    L.check(ops.lib.gs_pnorm_backward(C.byref(d), O._ptr(g), O._ptr(g2), O._ptr(y), O._ptr(mr), O._ptr(res), O._ptr(slope),
                                      O._ptr(dy), O._ptr(gres), O._ptr(dslope), O._ptr(db), O._ptr(scratch), O._stream()),
            "gs_pnorm_backward")
    put(name + "/backward", dy=dy, gres=gres, dslope=dslope, bias_grad=db, scratch=scratch)


def pnorm_cases(ops):
    k = 0
    for Cc in (8, 16, 32, 64, 256, 264):                      # COLS 1 / 2 / 4 / 8 / 32 / 32
        for N, sp in ((1, (3, 5, 7)), (2, (17, 13))):
            for res_mode in (0, 1, 2, 3):
                res_mod = 2 if res_mode == 1 and k & 1 else 0
                pnorm_backward(ops, f"pnorm/C{Cc}N{N}m{res_mode}", N, sp, Cc, res_mode, res_mod, norm=bool(k % 3),
                               with_slope=bool(k % 4 != 1), with_g2=bool(k & 2), with_gres=res_mode == 1)
                k += 1
    # more than 256 chunks at C < 128 (4 channels per workgroup in the slot sum), one and two images
    pnorm_backward(ops, "pnorm/vol_C8", 1, (24, 24, 32), 8, 0, 0, True, True, False, False)
    pnorm_backward(ops, "pnorm/vol_C16_N2", 2, (24, 24, 32), 16, 2, 0, True, True, True, False)
    pnorm_backward(ops, "pnorm/vol_C128", 1, (24, 24, 32), 128, 1, 0, True, True, False, True)
    pnorm_backward(ops, "pnorm/no_norm_no_slope", 1, (5, 7), 16, 1, 0, False, False, False, True)
    for Cc, co, wide, N, sp in ((8, 8, 24, 1, (3, 5, 7)), (16, 0, 16, 2, (17, 13)), (32, 16, 64, 1, (40, 40)), (64, 8, 80, 2, (9, 9)),
                                (264, 8, 272, 1, (300,)), (8, 0, 8, 1, (300, 300))):
        x = rnd(N, *sp, wide)
        pixels = x.numel() // (N * wide)
        slots = int(ops.lib.gs_slice_stats_slots(pixels))
        part = torch.zeros(N * slots * 2 * Cc, device="cuda")
        L.check(ops.lib.gs_slice_stats(O._ptr(x), N, pixels, wide, co, Cc, O._ptr(part), O._stream()), "gs_slice_stats")
        put(f"slice_stats/C{Cc}N{N}p{pixels}", partial=part)
    for acc in (0, 1):
        dst, src = rnd(2, 5, 7, 40), rnd(2, 5, 7, 24)
        ops.add_views(dst, src, 16, dst_co=8, src_co=8, accumulate=bool(acc))
        put(f"add_views/{acc}", dst=dst)
    g, g_img = rnd(2, 3, 5, 7, 24), rnd(2, 2, 3, 5, 7, dtype=torch.float32)
    ops.repeat_backward(g, g_img, 16, g_co=8)
    put("repeat_backward", g_img=g_img)


def main():
    ops = O.HipOps()
    inorm_cases(ops)
    inorm_backward_cases(ops)
    norm_ex_cases(ops)
    pnorm_cases(ops)
    print(json.dumps(OUT, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
