"""The host-side plans of the conv / data-gradient / weight-gradient launchers, without a GPU: every plan-only entry point of
csrc/gconv.hip and csrc/wgrad.hip (which kernel takes a layer, how many statistics slots it writes, whether and how far K is
split, whether a twin batch is one launch, how much workspace the deterministic weight gradient wants) answers for every conv
layer of the six bench.py workloads at bench.py's shapes — and for a table of edge descriptors — exactly what the commit named
in the fixture's header answered. The fixture (test_conv_plans_cpu.json, next to this file) is this project's own output:

    GANSLATE_HIP_LIB=<libganslate_hip.so of that commit> python tests/test_conv_plans_cpu.py <commit>

rewrites it; a change of a kernel-selection rule is then a reviewed diff of that file."""
import ctypes as C
import json
import sys
import types
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
FIXTURE = Path(__file__).with_suffix(".json")


# ---- the descriptors --------------------------------------------------------------------------------------------------------
def bench_networks():
    """(workload, network, constructor, input size, batch) of bench.py's six workloads (bench.py:main / make_*_conf)"""
    from ganslate_amd.nn import discriminators as D, generators as G
    res2, pg2 = lambda: G.Resnet2D(3, 3, "instance", 9), lambda: D.PatchGAN2D(3, 64, 3, 4, "instance")
    pg3_2 = lambda: D.PatchGAN3D(1, 64, 2, 4, "instance")
    return [
        ("cyclegan", "G", res2, (256, 256), 8), ("cyclegan", "D", pg2, (256, 256), 8),
        ("cut", "G", res2, (256, 256), 8), ("cut", "D", pg2, (256, 256), 8),
        ("pix2pix", "G", lambda: G.Unet2D(3, 3, 7, "instance", 128, True), (256, 512), 1),
        ("pix2pix", "D", lambda: D.PatchGAN2D(6, 64, 4, 4, "instance"), (256, 512), 1),
        ("cyclegan3d", "G", lambda: G.Resnet3D(1, 1, "instance", 9), (128, 128, 128), 1),
        ("cyclegan3d", "D", lambda: D.PatchGAN3D(1, 64, 3, 4, "instance"), (128, 128, 128), 1),
        ("brats", "G", lambda: G.Vnet3D(1, 1, "instance", 16, (2, 2, 3), (3, 3, 3), use_memory_saving=False,
                                        use_inverse=False), (128, 128, 128), 1),
        ("brats", "D", pg3_2, (128, 128, 128), 1),
        ("revgan", "G", lambda: G.Piresnet3D(1, 1, "instance", 5, 32, True, True), (32, 176, 176), 1),
        ("revgan", "D", pg3_2, (32, 176, 176), 1),
    ]


def edge_layers():
    """(name, ConvSpec, input size, batch): planning cases the six workloads do not reach, lowered like a network's layers"""
    from ganslate_amd.nn.native.spec import ConvSpec as S
    out = []
    for co in (8, 16, 64, 72, 128):                      # output-channel tile classes of pick_tile, and P of the weight gradient
        out.append((f"k4s2_co{co}", S("conv", 64, co, 4, 2, 1), (64, 64), 8))
        out.append((f"k3_co{co}", S("conv", 128, co, 3, 1, 1), (32, 32), 8))
    for cin, cout, hw in ((64, 128, 16), (64, 128, 15), (64, 128, 17), (128, 64, 64), (1024, 512, 2), (512, 1024, 4), (32, 16, 16)):
        # the four parity classes of the k3 / k4 stride-2 layers, even and odd extents: hconvt, merged im2col, merged split-K
        out.append((f"k3T_{cin}_{cout}_{hw}", S("convT", cin, cout, 3, 2, 1, out_pad=1), (hw, hw), 8))
        out.append((f"k4T_{cin}_{cout}_{hw}", S("convT", cin, cout, 4, 2, 1), (hw, hw), 8))
        out.append((f"k4s2_{cin}_{cout}_{hw}", S("conv", cin, cout, 4, 2, 1), (2 * hw, 2 * hw), 8))
        out.append((f"k3s2_{cin}_{cout}_{hw}", S("conv", cin, cout, 3, 2, 1), (2 * hw, 2 * hw), 8))
    out.append(("k2T_vol_32_16", S("convT", 32, 16, 2, 2, 0, dims=3), (16, 32, 32), 2))     # eight one-tap classes
    out.append(("k2T_vol_256_128", S("convT", 256, 128, 2, 2, 0, dims=3), (4, 4, 4), 1))
    out.append(("k2s2_vol_16_32", S("conv", 16, 32, 2, 2, 0, dims=3), (32, 64, 64), 2))
    out.append(("k3_vol_64_64", S("conv", 64, 64, 3, 1, 1, dims=3), (16, 32, 32), 2))       # 27 taps
    out.append(("k3_vol_128_128", S("conv", 128, 128, 3, 1, 1, dims=3, pad_mode="reflect"), (8, 16, 16), 2))
    out.append(("k5_vol_16_16", S("conv", 16, 16, 5, 1, 2, dims=3), (64, 64, 64), 1))
    out.append(("k5_axis_16_16", S("conv", 16, 16, 5, 1, 2, dims=3, axes="axis"), (64, 128, 128), 1))   # (5,1,1): daxis
    out.append(("k5_plane_16_16", S("conv", 16, 16, 5, 1, 2, dims=3, axes="plane"), (64, 128, 128), 1))
    out.append(("k7_fold_in", S("conv", 3, 64, 7, 1, 3, pad_mode="reflect", wfold="in"), (256, 256), 8))   # hstrip
    out.append(("k7_fold_out", S("conv", 64, 3, 7, 1, 3, pad_mode="reflect", wfold="out"), (256, 256), 8))
    # a wide 3x3 layer whose hconvw box count (288) is not the im2col tile count (256 tiles of 288 pixels): see slots_answerer
    out.append(("k3_wide_288", S("conv", 64, 128, 3, 1, 1, pad_mode="reflect"), (256, 288), 1))
    for p in (1, 16, 64, 128):                           # P of 8, 16, 64, 128 against a wide gathered side
        out.append((f"wg_p{p}", S("conv", 256, p, 4, 1, 1), (31, 31), 8))
    return out


def raw_gdesc(N, H, W, Ci, Co, kh, kw):
    """a stride-1, same-size, zero-border class with a kh x kw tap grid, written out by hand"""
    from ganslate_amd.hip import lib as L
    d = L.GConvDesc()
    d.N, d.Hi, d.Wi, d.Ci, d.in_cs, d.in_co = N, H, W, Ci, Ci, 0
    d.Di = d.Do = d.Dc = 1
    d.Ho, d.Wo, d.Co, d.out_cs, d.out_co, d.Hc, d.Wc = H, W, Co, Co, 0, H, W
    d.so = d.si = 1
    d.T, d.Kp, d.w_rows = kh * kw, (kh * kw * Ci + 63) // 64 * 64, Co
    for t in range(kh * kw):
        d.dh[t], d.dw[t], d.dd[t] = t // kw - kh // 2, t % kw - kw // 2, 0
    return d


def edge_descs():
    """name -> descriptor: tile-choice thresholds and K-loop lengths that no lowered layer lands on"""
    out = {}
    # 256-pixel tile count x channel tiles just below / at gconv_big (192), and the 257..512 window where 288 / 320 tiles win
    for name, (N, H, W) in {"big190": (1, 152, 160), "big192": (1, 128, 192), "win288": (8, 66, 66), "win320": (8, 69, 70),
                            "big512": (8, 64, 64), "big576": (8, 96, 96), "big256": (8, 64, 32)}.items():
        out[f"tile_{name}"] = raw_gdesc(N, H, W, 256, 256, 4, 4)
    for hw in (2, 4, 8, 16, 32):                         # Kp / 64 of 15 (3 x 5 taps) and 16 (4 x 4 taps): split-K needs 16 K-steps
        for co in (16, 64, 512):
            out[f"kp15_{hw}_{co}"] = raw_gdesc(1, hw, hw, 64, co, 3, 5)
            out[f"kp16_{hw}_{co}"] = raw_gdesc(1, hw, hw, 64, co, 4, 4)
            out[f"kp256_{hw}_{co}"] = raw_gdesc(1, hw, hw, 1024, co, 4, 4)
    return out


# ---- the answers ------------------------------------------------------------------------------------------------------------
RESIDENT = (("daxis", ("daxis",)), ("hconv", ("hconv", "hconv5")), ("hconvw", ("hconv_wide",)), ("hstrip", ("hstrip",)))


def slots_answerer(lib, d):
    """which kernel answers gs_gconv_stat_slots: the kernels are switched off in the order the library asks them until the
    answer moves (options restored). A kernel whose count equals what the next one in line says goes unnoticed (16 x 16 boxes
    and 256-pixel tiles of a 64 x 64 image): this under-reports a kernel and never over-reports one."""
    base, saved, who = lib.gs_gconv_stat_slots(C.byref(d)), {}, "im2col"
    try:
        for name, opts in RESIDENT:
            for o in opts:
                v = C.c_int(0)
                assert lib.gs_get_option(o.encode(), C.byref(v)) == 0
                saved[o] = v.value
                assert lib.gs_set_option(o.encode(), 0) == 0
            if lib.gs_gconv_stat_slots(C.byref(d)) != base:
                who = name
                break
    finally:
        for o, v in saved.items():
            assert lib.gs_set_option(o.encode(), v) == 0
    return who


def is_twin_batch(d):
    """the twin questions are about a batch of two networks' images: callers ask them for an even N >= 2 only (None otherwise)"""
    return d.N >= 2 and d.N % 2 == 0


COLUMNS = {"gconv": ("tile_m", "slots", "by", "splitk", "twin", "twin_fused", "twin_ring", "ring_slots"),
           "multi": ("fused_slots", "splitk", "twin"), "wgrad": ("ws", "twin", "ws_twin", "adam")}


def gconv_answers(lib, d):
    from ganslate_amd.hip import lib as L
    plain, ring = L.GConvFuse(), L.GConvFuse()           # (fold 0 on a padded domain; fold 1 on the unpadded domain: the ring form)
    ring.Dy, ring.Hy, ring.Wy, ring.fold = d.Do, d.Ho, d.Wo, 1
    p = C.byref(d)
    twin = (lambda f: lib.gs_gconv_twin_native(p, f)) if is_twin_batch(d) else (lambda f: None)
    return [lib.gs_tile_m(p), lib.gs_gconv_stat_slots(p), slots_answerer(lib, d), lib.gs_gconv_splitk_ws_floats(p),
            twin(None), twin(C.byref(plain)), twin(C.byref(ring)), lib.gs_gconv_ring_slots(p)]


def multi_answers(lib, descs):
    from ganslate_amd.hip import lib as L
    arr = (C.POINTER(L.GConvDesc) * len(descs))(*[C.pointer(d) for d in descs])
    return [lib.gs_gconv_multi_fused_slots(arr, len(descs)), lib.gs_gconv_multi_splitk_ws_floats(arr, len(descs)),
            lib.gs_gconv_multi_twin_native(arr, len(descs)) if is_twin_batch(descs[0]) else None]


def wgrad_answers(lib, d):
    p, pairs = C.byref(d), (0, 1)
    tw = is_twin_batch(d)
    return [[lib.gs_wgrad_ws_floats(p, i) for i in pairs], [lib.gs_wgrad_twin_native(p, i) if tw else None for i in pairs],
            [lib.gs_wgrad_ws_floats_twin(p, i) if tw else None for i in pairs], lib.gs_wgrad_adam_eligible(p)]


def collect():
    """{"gconv" | "multi" | "wgrad": {layer: {class and batch: answers in COLUMNS' order}}} from the library
    ganslate_amd.hip.lib loads. A descriptor that an earlier layer already asked about (the nine residual blocks of a ResNet, the
    second workload on the same networks) is not asked again."""
    import torch
    from ganslate_amd.hip import lib as L
    from ganslate_amd.hip.ops import HipOps
    from ganslate_amd.nn.native import backend
    from ganslate_amd.nn.native.spec import lower
    from oracle.ops_ref import RefOps
    lib = L.load()
    shim = types.SimpleNamespace(_desc_cache={})
    out, seen = {"gconv": {}, "multi": {}, "wgrad": {}}, set()

    def put(group, label, sub, descs, answer):
        key = (group, b"".join(bytes(d) for d in descs))
        if key not in seen:
            seen.add(key)
            out[group].setdefault(label, {})[sub] = answer(lib, descs if group == "multi" else descs[0])

    def layer(label, lw, batches):
        for N in batches:
            for kind in ("fwd", "dgrad", "dgrad_ring"):
                classes = getattr(lw, kind)
                classes = [] if classes is None else classes if isinstance(classes, list) else [classes]
                descs = [HipOps._gdesc(shim, g, N, g.Ci, 0, g.Co, 0, "none", 0.0, 0, 0) for g in classes]
                for c, d in enumerate(descs):
                    put("gconv", label, f"{kind}{c}/N{N}", [d], gconv_answers)
                if len(descs) > 1:
                    put("multi", label, f"{kind}/N{N}", descs, multi_answers)
            if lw.wgrad is not None:
                w = lw.wgrad
                put("wgrad", label, f"N{N}", [HipOps._wdesc(shim, w, N, w.P, 0, w.Q, 0)], wgrad_answers)

    backend.set_ops(RefOps(act_dtype=torch.float32))     # networks build without a GPU; nothing is run on them
    try:
        for workload, role, make, size, batch in bench_networks():
            net = make()
            # the launch of one network's batch, of both networks' (a twin batch), and the half a twin launch's probe asks about
            batches = sorted({2 * batch, batch, max(batch // 2, 1)})
            for nd, lw in zip(net.nodes, net._lowered(*size)):
                if lw is not None:
                    layer(f"{workload}/{role}/{nd.name}", lw, batches)
            del net
    finally:
        backend.set_ops(None)
    for name, spec, size, batch in edge_layers():
        layer(f"edge/{name}", lower(spec, *size), sorted({2 * batch, batch, max(batch // 2, 1)}))
    for name, d in edge_descs().items():
        put("gconv", "edge/" + name.split("_")[0], name.split("_", 1)[1], [d], gconv_answers)
    return out


def dump_fixture(commit, how, answers):
    """one line per layer"""
    groups = []
    for group in COLUMNS:
        rows = ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in sorted(answers[group].items()))
        groups.append(f"{json.dumps(group)}: {{\n{rows}\n}}")
    head = {"recorded_from": commit, "how": how, "columns": COLUMNS}
    return "{\n" + ",\n".join([f"{json.dumps(k)}: {json.dumps(v)}" for k, v in head.items()] + groups) + "\n}\n"


@pytest.fixture(scope="module")
def plans():
    from ganslate_amd.hip import lib as L
    if not L.library_path().is_file():
        import __graft_entry__
        __graft_entry__.build()
    return collect(), json.loads(FIXTURE.read_text())


def test_every_plan_answer_is_the_recorded_one(plans):
    got, want = plans
    assert want["recorded_from"], "the fixture names the commit whose library produced it"
    assert want["columns"] == {k: list(v) for k, v in COLUMNS.items()}
    for group in COLUMNS:
        flat = lambda x: {f"{layer}/{sub}": a for layer, subs in x[group].items() for sub, a in subs.items()}
        g, w = flat(got), flat(want)
        assert sorted(g) == sorted(w), f"{group}: the set of descriptors changed; re-record the fixture"
        diff = {k: (g[k], w[k]) for k in w if g[k] != w[k]}
        assert not diff, f"{group}: {len(diff)} plans changed (got, recorded; columns {COLUMNS[group]}), e.g. {list(diff.items())[:3]}"


def test_the_descriptors_reach_every_outcome(plans):
    """read off the RECORDED answers, so a fixture that lost an outcome fails here whatever the library says"""
    want = plans[1]
    g, m, w = ([dict(zip(COLUMNS[group], a)) for subs in want[group].values() for a in subs.values()] for group in COLUMNS)
    assert {a["by"] for a in g} == {"daxis", "hconv", "hconvw", "hstrip", "im2col"}
    assert {a["tile_m"] for a in g} == {128, 256, 288, 320}
    assert {a["splitk"] > 0 for a in g} == {True, False}
    assert {a["splitk"] > 0 for a in m} == {True, False}
    assert {a["fused_slots"] > 0 for a in m} == {True, False} and {a["twin"] for a in m} == {0, 1, None}
    for key in ("twin", "twin_ring"):                    # (twin_fused is the option gconv_twin on a padded domain: 1 throughout)
        assert {a[key] for a in g} == {0, 1, None}, key
    assert {a["ring_slots"] > 0 for a in g} == {True, False}
    # (with a second operand pair only the wide kernel and the im2col kernel are in play, and both have a twin form: pair 0)
    assert {a["twin"][0] for a in w} == {0, 1, None} and {a["twin"][1] for a in w} >= {1}
    assert {a["ws_twin"][0] >= 0 for a in w if a["ws_twin"][0] is not None} == {True, False}
    for pair in (0, 1):
        assert {a["ws"][pair] > 0 for a in w} == {True, False}
        assert all(a["ws"][pair] >= 0 for a in w), "a plan is host code: no descriptor of the table is refused"
    assert {a["adam"] for a in w} == {0, 1}


if __name__ == "__main__":
    FIXTURE.write_text(dump_fixture(sys.argv[1], "python tests/test_conv_plans_cpu.py <commit>, with GANSLATE_HIP_LIB naming that "
                                    "commit's libganslate_hip.so", collect()))
    print(FIXTURE, FIXTURE.stat().st_size, "bytes")
