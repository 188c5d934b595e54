"""Tensor-level wrappers over the C ABI (include/ganslate_hip.h). Every call enqueues on torch's current
stream; tensors are device tensors owned by the caller. No fallback: a missing library raises in lib.load()."""
import ctypes as C
import contextlib

import torch

import functools

from . import lib as L
from .. import switches
from ..nn.native.spec import GConv, WGrad
from ..nn.native.twin import Twin, TwinSplit, is_twin


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's current HIP stream as a raw handle. torch.cuda.current_stream() costs ~8 us of Python per call, which at
    ~1100 launches per step was half of the host's enqueue time; the C accessor is ~0.3 us."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class HipOps(TwinSplit):
    """The product backend: hand-written gfx950 kernels behind libganslate_hip.so."""
    name = "hip"
    act_dtype = torch.bfloat16   # storage type of activations and weight packs

    def __init__(self, device=None):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise RuntimeError("HipOps needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        L.check(self.lib.gs_init(self.device.index or 0), "gs_init")
        self._desc_cache = {}        # descriptors: built from the layer spec alone, valid whatever the options
        self._plans = {}             # answers of the library's planning queries: depend on the options (set_option clears them)
        self._timing_filter, self._timing_events, self._timing_images = None, {}, {}
        self.sync_options()

    # ---- kernel-selection switches ------------------------------------------------------------------------
    # The library reads no environment variable (gs_set_option, include/ganslate_hip.h); the GS_* variables of the
    # host side are mapped onto its options here (switches.LIBRARY_OPTIONS), when the backend is created and whenever a
    # model is built.
    def set_option(self, name, value):
        L.check(self.lib.gs_set_option(name.encode(), int(value)), "gs_set_option")
        self._plans.clear()

    def get_option(self, name):
        v = C.c_int(0)
        L.check(self.lib.gs_get_option(name.encode(), C.byref(v)), "gs_get_option")
        return v.value

    @contextlib.contextmanager
    def options(self, **values):
        """`with ops.options(hconv=0, hstrip=0): ...` runs the block with these option values and puts the previous ones back,
        whatever the block raises"""
        before = {name: self.get_option(name) for name in values}
        try:
            for name, value in values.items():
                self.set_option(name, value)
            yield self
        finally:
            for name, value in before.items():
                self.set_option(name, value)

    def sync_options(self):
        """every option follows its environment variable, or returns to the library's default where the variable is unset or
        the option has none"""
        if not hasattr(self, "_option_defaults"):
            self._option_defaults = {}
            for opt in switches.LIBRARY_OPTIONS:       # (an older build of the library — GANSLATE_HIP_LIB in an A/B — may not know
                try:                                   # the newest switches: those are skipped)
                    self._option_defaults[opt] = self.get_option(opt)
                except L.HipError:
                    pass
        for opt, default in self._option_defaults.items():
            want = switches.library_value(opt)
            if want is None:
                want = default
            if want != self.get_option(opt):
                self.set_option(opt, want)

    # ---- per-kernel timing with HIP events on the launch stream (used by bench.py) ------------------
    def enable_kernel_timing(self, select):
        """select(kind, spec, flag) -> label or None. kind "gconv": spec = GConv class, flag = fused norm-backward
        epilogue; kind "wgrad": spec = WGrad, flag = merged pair launch. Launches with a label are bracketed by HIP
        events on the stream they are launched on."""
        self._timing_filter, self._timing_events, self._timing_images = select, {}, {}
        return self._timing_events

    def disable_kernel_timing(self):
        self._timing_filter = None

    def _time_begin(self, kind, spec, flag, N=None):
        if self._timing_filter is None:
            return None
        label = self._timing_filter(kind, spec, flag)
        if label is None:
            return None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self._timing_events.setdefault(label, []).append((e0, e1))
        self._timing_images.setdefault(label, []).append(N)       # images per launch (a twin launch covers both networks)
        return e1

    def kernel_timing_result(self):
        """{label: (launches, average milliseconds)}"""
        torch.cuda.synchronize()
        return {label: (len(ev), sum(a.elapsed_time(b) for a, b in ev) / max(len(ev), 1))
                for label, ev in self._timing_events.items()}

    def kernel_timing_images(self):
        """{label: average number of images per timed launch}"""
        return {label: sum(v for v in ns if v) / max(sum(1 for v in ns if v), 1) for label, ns in self._timing_images.items()}

    # ---- descriptors ------------------------------------------------------------------------------------
    def _gdesc(self, g: GConv, N, in_cs, in_co, out_cs, out_co, act, slope, stats_slots, stats_slot0, accumulate=False):
        key = (id(g), N, in_cs, in_co, out_cs, out_co, act, slope, stats_slots, stats_slot0, accumulate)
        d = self._desc_cache.get(key)
        if d is None:
            d = L.GConvDesc()
            d.N, d.Hi, d.Wi, d.Ci, d.in_cs, d.in_co = N, g.Hi, g.Wi, g.Ci, in_cs, in_co
            d.Di, d.Do, d.Dc, d.pz = g.Di, g.Do, g.Dc, g.pz
            d.Ho, d.Wo, d.Co, d.out_cs, d.out_co = g.Ho, g.Wo, g.Co, out_cs, out_co
            d.Hc, d.Wc, d.so, d.py, d.px, d.si = g.Hc, g.Wc, g.so, g.py, g.px, g.si
            d.T, d.Kp, d.w_rows = g.T, g.Kp, g.w_rows
            d.border, d.act, d.slope = L.BORDER[g.border], L.ACT[act], slope
            d.stats_slots, d.stats_slot0, d.accumulate = stats_slots, stats_slot0, int(accumulate)
            for i, (a, b, c) in enumerate(zip(g.dh, g.dw, g.dd)):
                d.dh[i], d.dw[i], d.dd[i] = a, b, c
            self._desc_cache[key] = (d, g)   # keep g alive so id() stays unique
            return d
        return d[0]

    def _splitk_floats(self, d) -> int:
        """workspace floats the split-K form of this launch wants (0: no split); cached per descriptor"""
        key = ("splitk", id(d))
        n = self._plans.get(key)
        if n is None:
            n = int(self.lib.gs_gconv_splitk_ws_floats(C.byref(d)))
            self._plans[key] = n
        return n

    def _cout1(self, d) -> bool:
        """the dot-product kernels of the one-output-channel layer take this launch"""
        if not switches.on("GS_COUT1"):
            return False
        key = ("cout1", id(d))
        v = self._plans.get(key)
        if v is None:
            v = bool(self.lib.gs_conv_cout1_eligible(C.byref(d)))
            self._plans[key] = v
        return v

    def tile_m(self, g: GConv, N: int) -> int:
        """pixel-tile height the kernel will pick for this class at batch N (the choice depends on the grid size)"""
        return self.lib.gs_tile_m(C.byref(self._gdesc(g, N, g.Ci, 0, g.Co, 0, "none", 0.0, 0, 0)))

    # ---- twin batches (nn/native/twin.py): which batch a launch sees --------------------------------------------
    # Kernel choice — and with it the number of statistics / partial-sum slots per image — depends on the batch of the
    # LAUNCH. A twin batch of N images is one launch of N where the kernel picks the weight set per image
    # (gs_gconv_twin_native) and two launches of N / 2 otherwise; the planning calls below take `twin` and answer for the
    # launches that will actually run, while their buffers are sized for all N images.
    def twin_native(self, g: GConv, N: int, ring: bool = False, fused: bool = False) -> bool:
        """ring: the fused data gradient on the unpadded domain (hconvw RING); fused: the padded-domain fused launch"""
        if not switches.on("GS_TWIN_NATIVE"):
            return False
        d = self._gdesc(g, N, g.Ci, 0, g.Co, 0, "none", 0.0, 0, 0)
        if ring:
            return self.lib.gs_gconv_ring_slots(C.byref(d)) > 0
        if not fused and getattr(g, "co_real", 0) == 1 and self._cout1(d):
            return True
        if fused:
            if not switches.on("GS_TWIN_FUSED"):
                return False
            f = L.GConvFuse()           # (fold 0 on a padded output domain: not the ring form)
            return bool(self.lib.gs_gconv_twin_native(C.byref(d), C.byref(f)))
        return bool(self.lib.gs_gconv_twin_native(C.byref(d), None))

    def fused_norm_plan(self, g: GConv, N: int, C_: int, force: bool = False, twin: bool = False):
        """(slots, scratch) for fusing the reduction pass of the consumer's InstanceNorm backward into the data-gradient
        launch of class g, or None when this backend / layer shape does not fuse (narrow layers run on the halo kernel)"""
        if g.so != 1 or g.si not in (1, 2) or g.Co <= 64 or g.Co != C_ or not switches.on("GS_FUSE_NORM"):
            return None
        if g.si == 2 and not switches.on("GS_FUSE_SI2"):
            return None
        Nl = N // 2 if (twin and not self.twin_native(g, N, fused=True)) else N        # the batch of the launch(es)
        d = self._gdesc(g, Nl, g.Ci, 0, g.Co, 0, "none", 0.0, 0, 0)
        if self._splitk_floats(d) and not force:   # few output tiles, long K: split-K wins over the fused epilogue
            return None
        tm = self.tile_m(g, Nl)
        slots = (g.pixels + tm - 1) // tm
        return slots, torch.empty(N * (slots + 1) * 3 * C_, dtype=torch.float32, device=self.device)

    @staticmethod
    def _fuse_struct(fuse):
        f = L.GConvFuse()
        f.y, f.mean_rstd, f.partial = fuse["y"].data_ptr(), fuse["mean_rstd"].data_ptr(), fuse["partial"].data_ptr()
        f.g2 = fuse["g2"].data_ptr() if fuse.get("g2") is not None else None
        yd = fuse["y"].shape[1:-1]
        f.Dy, f.Hy, f.Wy = (1,) + tuple(yd) if len(yd) == 2 else tuple(yd)
        f.fold, f.fold_mode, f.act, f.slope = fuse["fold"], L.BORDER[fuse["fold_mode"]], L.ACT[fuse["act"]], \
            float(fuse.get("slope", 0.2))
        return f

    def _multi_descs(self, classes, N, in_cs, out_cs):
        key = ("multi_fused", tuple(id(g) for g in classes), N, in_cs, out_cs)
        ent = self._desc_cache.get(key)
        if ent is None:
            descs = [self._gdesc(g, N, in_cs, 0, out_cs, 0, "none", 0.0, 0, 0) for g in classes]
            arr = (C.POINTER(L.GConvDesc) * len(descs))(*[C.pointer(d) for d in descs])
            ent = (arr, descs)
            self._desc_cache[key] = ent
        return ent

    def fused_multi_plan(self, classes, N: int, C_: int, twin: bool = False):
        """(slots, scratch) when the output-parity classes of a stride-2 conv's data gradient run as ONE halo-resident launch
        that can carry the reduction pass of the consumer's InstanceNorm backward in its epilogue (hconvt.hip), else None"""
        g = classes[0]
        if len(classes) != 4 or g.Co != C_ or not switches.on("GS_FUSE_NORM") or not switches.on("GS_FUSE_MULTI"):
            return None
        Nl = N // 2 if (twin and not self.multi_twin_native(classes, N)) else N      # the batch of the launch(es)
        arr, _ = self._multi_descs(classes, Nl, g.Ci, g.Co)
        slots = self.lib.gs_gconv_multi_fused_slots(arr, len(classes))
        if slots <= 0:
            return None
        return slots, torch.empty(N * (slots + 1) * 3 * C_, dtype=torch.float32, device=self.device)

    def fused_ring_plan(self, g: GConv, N: int, C_: int, twin: bool = False):
        """(slots, scratch) when the fused data gradient of a reflect-padded 3x3 layer can run on the unpadded domain
        (class g = Lowered.dgrad_ring; the launch folds the ring itself, hconvw.hip RING), else None"""
        if g is None or g.Co != C_ or not switches.on("GS_FUSE_NORM"):
            return None
        Nl = N // 2 if (twin and not self.twin_native(g, N, ring=True)) else N
        slots = self.lib.gs_gconv_ring_slots(C.byref(self._gdesc(g, Nl, g.Ci, 0, g.Co, 0, "none", 0.0, 0, 0)))
        if slots <= 0:
            return None
        return slots, torch.empty(N * (slots + 1) * 3 * C_, dtype=torch.float32, device=self.device)

    def multi_twin_native(self, classes, N: int) -> bool:
        """a twin batch of N images over the output-parity classes of one layer runs as ONE launch (the halo-resident class
        kernel picks the packs per box, gs_gconv_multi_twin_native) — else as two launches of N / 2"""
        if not switches.on("GS_TWIN_NATIVE") or not switches.on("GS_TWIN_MULTI") or N % 2:
            return False
        g = classes[0]
        key = ("multi_twin", tuple(id(c) for c in classes), N)
        v = self._plans.get(key)
        if v is None:
            arr, _ = self._multi_descs(classes, N, g.Ci, g.Co)
            v = bool(self.lib.gs_gconv_multi_twin_native(arr, len(classes)))
            self._plans[key] = v
        return v

    def stat_slots(self, g: GConv, N: int, twin: bool = False, multi=None) -> int:
        """partial-statistics slots per image the kernel writes for this class at batch N. multi: the classes of the layer
        when g is one of several output-parity classes (gconv_classes): a twin batch of those runs as ONE launch where
        multi_twin_native says so and as two launches of N / 2 otherwise, whatever a single-class launch of g would do"""
        if twin and multi:
            Nl = N if self.multi_twin_native(multi, N) else N // 2
        else:
            Nl = N // 2 if (twin and not self.twin_native(g, N)) else N
        return self.lib.gs_gconv_stat_slots(C.byref(self._gdesc(g, Nl, g.Ci, 0, g.Co, 0, "none", 0.0, 0, 0)))

    # ---- convolution family -------------------------------------------------------------------------------
    def gconv(self, g: GConv, x, wpack, bias, out, *, in_cs=None, in_co=0, out_cs=None, out_co=0, act="none",
              slope=0.2, stats=None, stats_slots=0, stats_slot0=0, accumulate=False, fuse=None):
        N = x.shape[0]
        in_cs = in_cs if in_cs is not None else x.shape[-1]
        out_cs = out_cs if out_cs is not None else out.shape[-1]
        d = self._gdesc(g, N, in_cs, in_co, out_cs, out_co, act, float(slope), stats_slots, stats_slot0, accumulate)
        if getattr(g, "co_real", 0) == 1 and fuse is None and stats is None and self._cout1(d):
            # one output channel (the PatchGAN's last layer): the dot-product kernel on the vector ALUs (csrc/cout1.hip)
            tw = None
            if is_twin(wpack, bias):
                tw = L.Twin()
                tw.n_split, tw.w_delta = N // 2, wpack.delta()
                tw.bias_delta = bias.delta() if isinstance(bias, Twin) else 0
            w0 = wpack.a if isinstance(wpack, Twin) else wpack
            b0 = bias.a if isinstance(bias, Twin) else bias
            L.check(self.lib.gs_conv_cout1_forward(C.byref(d), _ptr(x), C.c_void_p(w0.data_ptr() + 2 * g.pack_offset),
                                                   _ptr(b0), _ptr(out), C.byref(tw) if tw is not None else None, _stream()),
                    "gs_conv_cout1_forward")
            return
        if is_twin(wpack, bias):      # two networks' weights over one batch (nn/native/twin.py)
            f = self._fuse_struct(fuse) if fuse is not None else None
            ring = f is not None and f.fold > 0 and tuple(fuse["y"].shape[-3:-1]) == (g.Ho, g.Wo)
            if isinstance(wpack, Twin) and not accumulate and \
                    self.twin_native(g, N, ring=ring, fused=f is not None and not ring):
                # the kernel picks the weight set per image: one launch over both networks' images
                tw = L.Twin()
                tw.n_split, tw.w_delta = N // 2, wpack.delta()
                tw.bias_delta = bias.delta() if isinstance(bias, Twin) else 0
                b0 = bias.a if isinstance(bias, Twin) else bias
                t_end = self._time_begin("gconv", g, fuse is not None, N)
                L.check(self.lib.gs_gconv_forward_twin(C.byref(d), _ptr(x), C.c_void_p(wpack.a.data_ptr() + 2 * g.pack_offset),
                                                       _ptr(b0), _ptr(out), _ptr(stats),
                                                       C.byref(f) if f is not None else None, C.byref(tw), _stream()),
                        "gs_gconv_forward_twin")
                if t_end is not None:
                    t_end.record()
                return
            return self.twin_gconv(functools.partial(self.gconv, g), x, wpack, bias, out, in_cs=in_cs, in_co=in_co,
                                   out_cs=out_cs, out_co=out_co, act=act, slope=slope, stats=stats,
                                   stats_slots=stats_slots, stats_slot0=stats_slot0, accumulate=accumulate, fuse=fuse,
                                   C_=g.Co)
        w = C.c_void_p(wpack.data_ptr() + 2 * g.pack_offset)
        t_end = self._time_begin("gconv", g, fuse is not None, N)
        if fuse is not None:     # data gradient + first pass of the consumer's InstanceNorm backward (fused_norm_plan)
            f = self._fuse_struct(fuse)
            L.check(self.lib.gs_gconv_forward_fused(C.byref(d), _ptr(x), w, _ptr(bias), _ptr(out), _ptr(stats),
                                                    C.byref(f), _stream()), "gs_gconv_forward_fused")
            if t_end is not None:
                t_end.record()
            return
        nws = self._splitk_floats(d)
        if nws:      # few output tiles, long K: split-K with a per-launch workspace (stream-safe through the allocator)
            ws = torch.empty(nws, dtype=torch.float32, device=self.device)
            L.check(self.lib.gs_gconv_forward_ws(C.byref(d), _ptr(x), w, _ptr(bias), _ptr(out), _ptr(stats), _ptr(ws),
                                                 nws, _stream()), "gs_gconv_forward_ws")
        else:
            L.check(self.lib.gs_gconv_forward(C.byref(d), _ptr(x), w, _ptr(bias), _ptr(out), _ptr(stats), _stream()),
                    "gs_gconv_forward")
        if t_end is not None:
            t_end.record()

    def gconv_classes(self, classes, x, wpack, bias, out, *, in_co=0, out_co=0, act="none", slope=0.2, stats=None,
                      stats_slots=0, stats_slot0s=None, accumulate=False, fuse=None):
        """every output-parity class of one layer (Lowered.fwd / .dgrad). More than one class: gs_gconv_forward_multi, one
        launch when the classes are mergeable (the library decides; it runs them one by one otherwise). Layers so small
        that even the merged grid leaves the chip empty keep the per-class launches, which split K."""
        if is_twin(wpack, bias) and len(classes) == 1 and fuse is None:
            return self.gconv(classes[0], x, wpack, bias, out, in_co=in_co, out_co=out_co, act=act, slope=slope, stats=stats,
                              stats_slots=stats_slots, stats_slot0=(stats_slot0s[0] if stats_slot0s else 0),
                              accumulate=accumulate)
        if is_twin(wpack, bias):
            N2 = x.shape[0]
            if isinstance(wpack, Twin) and not accumulate and in_co == 0 and out_co == 0 and \
                    self.multi_twin_native(classes, N2):
                # the class kernel picks the packs per box: one launch over both networks' images
                descs = [self._gdesc(g, N2, x.shape[-1], 0, out.shape[-1], 0, act, float(slope), stats_slots,
                                     (stats_slot0s[i] if stats_slot0s else 0)) for i, g in enumerate(classes)]
                arr = (C.POINTER(L.GConvDesc) * len(descs))(*[C.pointer(d) for d in descs])
                ws = (C.c_void_p * len(classes))(*[wpack.a.data_ptr() + 2 * g.pack_offset for g in classes])
                tw = L.Twin()
                tw.n_split, tw.w_delta = N2 // 2, wpack.delta()
                tw.bias_delta = bias.delta() if isinstance(bias, Twin) else 0
                b0 = bias.a if isinstance(bias, Twin) else bias
                f = self._fuse_struct(fuse) if fuse is not None else None
                t_end = self._time_begin("gconv_multi", classes, f is not None, N2)
                L.check(self.lib.gs_gconv_forward_multi_twin(arr, len(classes), _ptr(x), ws, _ptr(None if f is not None else b0),
                                                             _ptr(out), _ptr(None if f is not None else stats),
                                                             C.byref(f) if f is not None else None, C.byref(tw), _stream()),
                        "gs_gconv_forward_multi_twin")
                if t_end is not None:
                    t_end.record()
                return
            return self.twin_gconv(functools.partial(self.gconv_classes, classes), x, wpack, bias, out, in_co=in_co,
                                   out_co=out_co, act=act, slope=slope, stats=stats, stats_slots=stats_slots,
                                   stats_slot0s=stats_slot0s, accumulate=accumulate, fuse=fuse, C_=classes[0].Co)
        N = x.shape[0]
        if fuse is not None:     # fused_multi_plan said yes: all classes + the consumer's norm-backward sums in one launch
            arr, _ = self._multi_descs(classes, N, x.shape[-1], out.shape[-1])
            base = wpack.data_ptr()
            ws = (C.c_void_p * len(classes))(*[base + 2 * g.pack_offset for g in classes])
            t_end = self._time_begin("gconv_multi", classes, True, N)
            L.check(self.lib.gs_gconv_forward_multi_fused(arr, len(classes), _ptr(x), ws, _ptr(out),
                                                          C.byref(self._fuse_struct(fuse)), _stream()),
                    "gs_gconv_forward_multi_fused")
            if t_end is not None:
                t_end.record()
            return
        slot0 = lambda i: stats_slot0s[i] if stats_slot0s else 0
        g0 = classes[0]
        merged = len(classes) > 1 and not accumulate
        if merged:
            key = ("multi", tuple(id(g) for g in classes), N, x.shape[-1], in_co, out.shape[-1], out_co, act, float(slope),
                   stats_slots, tuple(stats_slot0s or ()))
            ent = self._desc_cache.get(key)
            if ent is None:
                descs = [self._gdesc(g, N, x.shape[-1], in_co, out.shape[-1], out_co, act, float(slope), stats_slots,
                                     slot0(i)) for i, g in enumerate(classes)]
                arr = (C.POINTER(L.GConvDesc) * len(descs))(*[C.pointer(d) for d in descs])
                ent = (arr, descs)
                self._desc_cache[key] = ent
            plan = self._plans.get(key)
            if plan is None:
                arr, descs = ent
                tn = 16 if g0.Co <= 16 else (64 if g0.Co <= 64 else 128)
                tm = self.tile_m(g0, N)
                blocks = len(classes) * N * ((g0.pixels + tm - 1) // tm) * ((g0.Co + tn - 1) // tn)
                use = blocks >= 128 or not any(self._splitk_floats(d) for d in descs)
                # a merged grid that still leaves the chip empty: split K over it (one launch + one finalize for all classes)
                nws = 0 if use else int(self.lib.gs_gconv_multi_splitk_ws_floats(arr, len(descs)))
                plan = self._plans[key] = (use or nws > 0, nws)
            merged = plan[0]
        if not merged:
            for i, g in enumerate(classes):
                self.gconv(g, x, wpack, bias, out, in_co=in_co, out_co=out_co, act=act, slope=slope, stats=stats,
                           stats_slots=stats_slots, stats_slot0=slot0(i), accumulate=accumulate)
            return
        base = wpack.data_ptr()
        ws = (C.c_void_p * len(classes))(*[base + 2 * g.pack_offset for g in classes])
        t_end = self._time_begin("gconv_multi", classes, False, N)
        nws = plan[1]
        if nws:
            part = torch.empty(nws, dtype=torch.float32, device=self.device)
            L.check(self.lib.gs_gconv_forward_multi_ws(ent[0], len(classes), _ptr(x), ws, _ptr(bias), _ptr(out), _ptr(stats),
                                                       _ptr(part), nws, _stream()), "gs_gconv_forward_multi_ws")
        else:
            L.check(self.lib.gs_gconv_forward_multi(ent[0], len(classes), _ptr(x), ws, _ptr(bias), _ptr(out), _ptr(stats),
                                                    _stream()), "gs_gconv_forward_multi")
        if t_end is not None:
            t_end.record()

    @staticmethod
    def can_merge_wgrad(w: WGrad) -> bool:
        """two backward passes of this layer can share one launch (the wide halo kernel's eligibility, hwgrad.hip)"""
        if w.si != 1 or w.P % 64 or w.Q % 64 or not switches.on("GS_WGRAD_PAIR"):
            return False
        if w.T == 9 and w.Da == 1:
            return True
        # 3x3x3 layers of volumes run as three depth planes of the same kernel (hwgrad.hip)
        return (w.T == 27 and w.Da > 1 and switches.on("GS_HWGRAD_PLANES")
                and all(w.dd[9 * k + t] == w.dd[9 * k] and w.dh[9 * k + t] == w.dh[t] and w.dw[9 * k + t] == w.dw[t]
                        for k in range(3) for t in range(9)))

    def _wdesc(self, w: WGrad, N, a_cs, a_co, g_cs, g_co, fresh=False):
        d = L.WGradDesc()
        d.dw_fresh = int(fresh)
        d.N, d.Ha, d.Wa, d.P = N, w.Ha, w.Wa, w.P
        d.Da, d.Dg = w.Da, w.Dg
        d.a_cs, d.a_co = a_cs, a_co
        d.Hg, d.Wg, d.Q = w.Hg, w.Wg, w.Q
        d.g_cs, d.g_co = g_cs, g_co
        d.si, d.T, d.border, d.dw_ld = w.si, w.T, L.BORDER[w.border], w.T * w.Q
        for i, (p, q, r) in enumerate(zip(w.dh, w.dw, w.dd)):
            d.dh[i], d.dw_[i], d.dd[i] = p, q, r
        return d

    def wgrad_adam(self, w: WGrad, a, g, p, m, v, hyper_dev, packs=None, tr=None) -> bool:
        """weight gradient + Adam of ONE layer in one launch (gs_wgrad_adam): p / m / v are the layer's slices of the flat
        buffers, packs = (inv_f slice, fpack, inv_d slice, dpack) as for adam_step_dev; tr = (base int32[T], kp int32[T], pack):
        the layer's transposed pack, written by the same launch (gs_adam_fuse.tr_*). Returns False (nothing launched) where
        the layer does not run as a one-split im2col launch — the caller then runs wgrad() and the optimiser as usual."""
        key = ("wadam", id(w), a.shape[0], a.shape[-1], g.shape[-1])
        ent = self._desc_cache.get(key)
        if ent is None:
            ent = self._desc_cache[key] = (self._wdesc(w, a.shape[0], a.shape[-1], 0, g.shape[-1], 0), w)
        ok = self._plans.get(key)
        if ok is None:
            ok = self._plans[key] = bool(self.lib.gs_wgrad_adam_eligible(C.byref(ent[0]))) and getattr(w, "p_real", 0) != 1
        if not ok:
            return False
        ad = L.AdamFuse()
        ad.p, ad.m, ad.v, ad.hyper = p.data_ptr(), m.data_ptr(), v.data_ptr(), hyper_dev.data_ptr()
        if packs is not None:
            inv_f, fpack, inv_d, dpack = packs
            if inv_f is not None:
                ad.inv_f, ad.fpack = inv_f.data_ptr(), fpack.data_ptr()
            if inv_d is not None:
                ad.inv_d, ad.dpack = inv_d.data_ptr(), dpack.data_ptr()
        if tr is not None:
            ad.tr_base, ad.tr_kp, ad.tr_pack = tr[0].data_ptr(), tr[1].data_ptr(), tr[2].data_ptr()
        t_end = self._time_begin("wgrad", w, False, a.shape[0])
        L.check(self.lib.gs_wgrad_adam(C.byref(ent[0]), _ptr(a), _ptr(g), C.byref(ad), _stream()), "gs_wgrad_adam")
        if t_end is not None:
            t_end.record()
        return True

    def wgrad(self, w: WGrad, a, g, dw, *, a_cs=None, a_co=0, g_cs=None, g_co=0, pair=None, fresh=False):
        """dw += the weight gradient. fresh: the caller guarantees that dw holds zeros (the layer's first weight gradient since
        the optimiser cleared the buffer, NativeNet.wgrad_fresh) — a hint (gs_wgrad_desc.dw_fresh), never a requirement"""
        twin = is_twin(dw)
        fresh = bool(fresh) and not twin and pair is None and switches.on("GS_WGRAD_FRESH")
        if twin and (not switches.on("GS_WGRAD_DET") or not switches.on("GS_TWIN_NATIVE")
                     or not switches.on("GS_TWIN_WGRAD")):
            return self.twin_wgrad(w, a, g, dw, a_cs=a_cs, a_co=a_co, g_cs=g_cs, g_co=g_co, pair=pair)
        key = ("w", id(w), a.shape[0], a_cs, a_co, g_cs, g_co, fresh)
        ent = self._desc_cache.get(key)
        if ent is None:
            d = self._wdesc(w, a.shape[0], a_cs if a_cs is not None else a.shape[-1], a_co,
                            g_cs if g_cs is not None else g.shape[-1], g_co, fresh)
            ent = self._desc_cache[key] = (d, w)
        if getattr(w, "p_real", 0) == 1 and switches.on("GS_COUT1") and switches.on("GS_WGRAD_DET"):
            ckey = ("cout1_w", id(ent[0]))
            nws = self._plans.get(ckey)
            if nws is None:
                nws = int(self.lib.gs_wgrad_cout1_ws_floats(C.byref(ent[0])))
                self._plans[ckey] = nws
            if nws > 0 and (not twin or dw.delta() % 16 == 0):
                # one output channel: x[q] times the 4 x 4 patch of dy around q on the vector ALUs (csrc/cout1.hip)
                tw = None
                if twin:
                    tw = L.Twin()
                    tw.n_split, tw.dw_delta = a.shape[0] // 2, dw.delta()
                dw0 = dw.a if twin else dw
                for aa, gg in ((a, g),) + ((tuple(pair),) if pair is not None else ()):
                    ws = torch.empty(nws, dtype=torch.float32, device=self.device)
                    L.check(self.lib.gs_wgrad_cout1_ws(C.byref(ent[0]), _ptr(aa), _ptr(gg), _ptr(dw0), _ptr(ws), nws,
                                                       C.byref(tw) if tw is not None else None, _stream()), "gs_wgrad_cout1_ws")
                return
        if twin:      # both networks' images in one launch where the layer's kernel has the form, else the two halves
            wkey = ("wgrad_ws", id(ent[0]), pair is not None, "twin")
            nws = self._plans.get(wkey)
            if nws is None:
                nws = int(self.lib.gs_wgrad_ws_floats_twin(C.byref(ent[0]), int(pair is not None))) \
                    if self.lib.gs_wgrad_twin_native(C.byref(ent[0]), int(pair is not None)) else -1
                self._plans[wkey] = nws
            if nws <= 0:
                return self.twin_wgrad(w, a, g, dw, a_cs=a_cs, a_co=a_co, g_cs=g_cs, g_co=g_co, pair=pair)
            tw = L.Twin()
            tw.n_split, tw.dw_delta = a.shape[0] // 2, dw.delta()
            ws = torch.empty(nws, dtype=torch.float32, device=self.device)
            a2, g2 = pair if pair is not None else (None, None)
            t_end = self._time_begin("wgrad", w, pair is not None, a.shape[0])
            L.check(self.lib.gs_wgrad_ws_twin(C.byref(ent[0]), _ptr(a), _ptr(g), _ptr(a2), _ptr(g2), _ptr(dw.a), _ptr(ws), nws,
                                              C.byref(tw), _stream()), "gs_wgrad_ws_twin")
            if t_end is not None:
                t_end.record()
            return
        t_end = self._time_begin("wgrad", w, pair is not None, a.shape[0])
        if switches.on("GS_WGRAD_DET"):
            # deterministic accumulation (default): partial sums to a per-launch workspace, fixed-order second stage
            wkey = ("wgrad_ws", id(ent[0]), pair is not None)
            nws = self._plans.get(wkey)
            if nws is None:
                nws = int(self.lib.gs_wgrad_ws_floats(C.byref(ent[0]), int(pair is not None)))
                if nws < 0:
                    L.check(2, "gs_wgrad_ws_floats")
                self._plans[wkey] = nws
            # (0 floats: single-contributor layers accumulate straight into dw, no workspace)
            ws = torch.empty(nws, dtype=torch.float32, device=self.device) if nws else None   # stream-safe via the allocator
            a2, g2 = pair if pair is not None else (None, None)
            L.check(self.lib.gs_wgrad_ws(C.byref(ent[0]), _ptr(a), _ptr(g), _ptr(a2), _ptr(g2), _ptr(dw), _ptr(ws), nws,
                                         _stream()), "gs_wgrad_ws")
        elif pair is not None:      # (a2, g2): the same layer's operands from another backward pass, one launch
            L.check(self.lib.gs_wgrad_pair(C.byref(ent[0]), _ptr(a), _ptr(g), _ptr(pair[0]), _ptr(pair[1]), _ptr(dw),
                                           _stream()), "gs_wgrad_pair")
        else:
            L.check(self.lib.gs_wgrad(C.byref(ent[0]), _ptr(a), _ptr(g), _ptr(dw), _stream()), "gs_wgrad")
        if t_end is not None:
            t_end.record()

    def bias_grad(self, dy, C_, db, *, cs=None, co=0):
        if is_twin(db):
            return self.twin_bias_grad(dy, C_, db, cs=cs, co=co)
        pixels = dy.numel() // dy.shape[-1]
        if C_ % 8:                                          # db has exactly C_ floats: whole octets, then a head of < 8
            full = C_ // 8 * 8
            cs_ = cs if cs is not None else dy.shape[-1]
            if full:
                self.bias_grad(dy, full, db[:full], cs=cs_, co=co)
            nws = int(self.lib.gs_bias_grad_ws_floats(pixels, 8))
            ws = torch.empty(nws, dtype=torch.float32, device=self.device)
            L.check(self.lib.gs_bias_grad_head_ws(_ptr(dy), pixels, cs_, co + full, C_ - full, _ptr(db[full:]),
                                                  _ptr(ws), nws, _stream()), "gs_bias_grad_head_ws")
            return
        if switches.on("GS_WGRAD_DET"):      # deterministic: partial sums + fixed-order second stage
            nws = int(self.lib.gs_bias_grad_ws_floats(pixels, C_))
            ws = torch.empty(nws, dtype=torch.float32, device=self.device)
            L.check(self.lib.gs_bias_grad_ws(_ptr(dy), pixels, C_, cs if cs is not None else dy.shape[-1], co, _ptr(db),
                                             _ptr(ws), nws, _stream()), "gs_bias_grad_ws")
            return
        L.check(self.lib.gs_bias_grad(_ptr(dy), pixels, C_, cs if cs is not None else dy.shape[-1], co, _ptr(db),
                                      _stream()), "gs_bias_grad")

    # ---- InstanceNorm + activation ----------------------------------------------------------------------
    def inorm_finalize(self, partial, N, slots, Cc, hw, mean_rstd, eps=1e-5):
        L.check(self.lib.gs_inorm_finalize(_ptr(partial), N, slots, Cc, hw, eps, _ptr(mean_rstd), _stream()),
                "gs_inorm_finalize")

    def inorm_act_forward(self, y, mean_rstd, res, x, act="none", slope=0.2):
        N, Cc = y.shape[0], y.shape[-1]
        L.check(self.lib.gs_inorm_act_forward(_ptr(y), _ptr(mean_rstd), _ptr(res), _ptr(x), N,
                                              y.numel() // (N * Cc), Cc,
                                              L.ACT[act], slope, _stream()), "gs_inorm_act_forward")

    def inorm_stats_act_forward(self, y, partial, slots, mean_rstd, res, x, act="none", slope=0.2, eps=1e-5):
        """inorm_finalize + inorm_act_forward as one launch (the apply kernel sums the slots of its own channels)"""
        N, Cc = y.shape[0], y.shape[-1]
        L.check(self.lib.gs_inorm_stats_act_forward(_ptr(y), _ptr(partial), slots, eps, _ptr(mean_rstd), _ptr(res),
                                                    _ptr(x), N, y.numel() // (N * Cc), Cc, L.ACT[act], slope,
                                                    _stream()), "gs_inorm_stats_act_forward")

    def inorm_act_backward(self, g_pad, g2, y, mean_rstd, dy, gsum, fold=0, fold_mode="reflect", act="none",
                           slope=0.2, bias_grad=None, pre=None):
        N, D, H, W, Cc = y.shape if y.dim() == 5 else (y.shape[0], 1) + tuple(y.shape[1:])
        scratch, pre_slots = None, 0
        if pre is not None:          # reduction pass already done by the fused data-gradient launch
            pre_slots, scratch = pre
        elif mean_rstd is not None:
            n = self.lib.gs_inorm_backward_scratch_floats(N, D, H, W, Cc)
            scratch = torch.empty(n, dtype=torch.float32, device=y.device)
        L.check(self.lib.gs_inorm_act_backward(_ptr(g_pad), _ptr(g2), _ptr(y), _ptr(mean_rstd), _ptr(dy),
                                               _ptr(gsum), _ptr(scratch), _ptr(bias_grad), N, D, H, W, Cc, fold,
                                               L.BORDER[fold_mode], L.ACT[act], slope, pre_slots, _stream()),
                "gs_inorm_act_backward")
        if mean_rstd is None:
            return None
        # the per-image totals [N][3][C] sit behind the partial slots: (holder tensor, float offset) for norm_bias_grads
        return scratch, scratch.numel() - N * 3 * Cc

    def norm_bias_grads(self, items):
        """bias gradients of the convs in front of InstanceNorms for many layers in one launch;
        items: (sums holder, float offset, mean_rstd, db, N, C, hw)"""
        if not items:
            return
        arr = (L.NormDbItem * len(items))()
        for a, (holder, off, mean_rstd, db, N, Cc, hw) in zip(arr, items):
            a.sums, a.mean_rstd, a.db = holder.data_ptr() + 4 * off, mean_rstd.data_ptr(), db.data_ptr()
            a.N, a.C, a.inv_hw = N, Cc, 1.0 / hw
        L.check(self.lib.gs_norm_bias_grads(arr, len(items), _stream()), "gs_norm_bias_grads")

    # ---- generalised norm / activation for skip-connection graphs (U-Net) ---------------------------------
    def _norm_ex_desc(self, y, act1, act2, slope, drop_p, seed, seed_dev=None):
        d = L.NormExDesc()
        d.seed_dev = seed_dev.data_ptr() if seed_dev is not None else None      # int32[2] device tensor (lo, hi)
        d.N, d.W, d.C = y.shape[0], y.shape[-2], y.shape[-1]       # geometry-free kernels: a volume is D*H rows
        d.H = y.numel() // (d.N * d.W * d.C)
        d.act1, d.act2, d.slope = L.ACT[act1], L.ACT[act2], slope
        d.drop_p, d.seed_lo, d.seed_hi = drop_p, seed & 0xffffffff, (seed >> 32) & 0xffffffff
        return d

    def norm_act_forward_ex(self, y, mean_rstd, x1, x2=None, act1="none", act2="none", slope=0.2, x1_co=0, x2_co=0,
                            drop_p=0.0, seed=0, seed_dev=None):
        d = self._norm_ex_desc(y, act1, act2, slope, drop_p, seed, seed_dev)
        d.x1_cs, d.x1_co = x1.shape[-1], x1_co
        if x2 is not None:
            d.x2_cs, d.x2_co = x2.shape[-1], x2_co
        L.check(self.lib.gs_norm_act_forward_ex(C.byref(d), _ptr(y), _ptr(mean_rstd), _ptr(x1), _ptr(x2), _stream()),
                "gs_norm_act_forward_ex")

    def norm_act_backward_ex(self, g1, g2, y, mean_rstd, dy, act1="none", act2="none", slope=0.2, g1_co=0, g2_co=0,
                             drop_p=0.0, seed=0, bias_grad=None, seed_dev=None):
        d = self._norm_ex_desc(y, act1, act2, slope, drop_p, seed, seed_dev)
        d.g1_cs, d.g1_co = g1.shape[-1], g1_co
        if g2 is not None:
            d.g2_cs, d.g2_co = g2.shape[-1], g2_co
        scratch = None
        if mean_rstd is not None:
            scratch = torch.empty(self.lib.gs_norm_backward_ex_scratch_floats(C.byref(d)), dtype=torch.float32,
                                  device=y.device)
        L.check(self.lib.gs_norm_act_backward_ex(C.byref(d), _ptr(g1), _ptr(g2), _ptr(y), _ptr(mean_rstd), _ptr(dy),
                                                 _ptr(scratch), _ptr(bias_grad), _stream()),
                "gs_norm_act_backward_ex")

    # ---- V-Net elementwise family (InstanceNorm3d -> [+res] -> PReLU -> [+res]) on channel slices ----------------
    @staticmethod
    def _pdesc(y, C_, y_co, res, res_mode, res_mod, res_co):
        d = L.PNormDesc()
        d.N, d.C = y.shape[0], C_
        d.pixels = y.numel() // (y.shape[0] * y.shape[-1])
        d.y_cs, d.y_co = y.shape[-1], y_co
        d.res_mode, d.res_mod = res_mode, res_mod
        if res is not None:
            d.res_cs, d.res_co = res.shape[-1], res_co
        return d

    def pnorm_forward(self, y, mean_rstd, out, *, C, slope=None, res=None, res_mode=0, res_mod=0, y_co=0, res_co=0,
                      out_co=0):
        if is_twin(slope):
            return self.twin_pnorm_forward(y, mean_rstd, out, C=C, slope=slope, res=res, res_mode=res_mode, res_mod=res_mod,
                                           y_co=y_co, res_co=res_co, out_co=out_co)
        d = self._pdesc(y, C, y_co, res, res_mode, res_mod, res_co)
        d.out_cs, d.out_co = out.shape[-1], out_co
        L.check(self.lib.gs_pnorm_forward(L.C.byref(d), _ptr(y), _ptr(mean_rstd), _ptr(res), _ptr(slope), _ptr(out),
                                          _stream()), "gs_pnorm_forward")

    def pnorm_backward(self, g, y, mean_rstd, dy, *, C, slope=None, dslope=None, g2=None, res=None, res_mode=0,
                       res_mod=0, gres=None, bias_grad=None, g_co=0, g2_co=0, y_co=0, res_co=0, dy_co=0, gres_co=0):
        if is_twin(slope, dslope, bias_grad):
            return self.twin_pnorm_backward(g, y, mean_rstd, dy, C=C, slope=slope, dslope=dslope, g2=g2, res=res,
                                            res_mode=res_mode, res_mod=res_mod, gres=gres, bias_grad=bias_grad, g_co=g_co,
                                            g2_co=g2_co, y_co=y_co, res_co=res_co, dy_co=dy_co, gres_co=gres_co)
        d = self._pdesc(y, C, y_co, res, res_mode, res_mod, res_co)
        d.g_cs, d.g_co = g.shape[-1], g_co
        if g2 is not None:
            d.g2_cs, d.g2_co = g2.shape[-1], g2_co
        d.dy_cs, d.dy_co = dy.shape[-1], dy_co
        if gres is not None:
            d.gres_cs, d.gres_co = gres.shape[-1], gres_co
        scratch = None
        if mean_rstd is not None or (slope is not None and dslope is not None):
            scratch = torch.empty(self.lib.gs_pnorm_backward_scratch_floats(L.C.byref(d)), dtype=torch.float32,
                                  device=y.device)
        L.check(self.lib.gs_pnorm_backward(L.C.byref(d), _ptr(g), _ptr(g2), _ptr(y), _ptr(mean_rstd), _ptr(res),
                                           _ptr(slope), _ptr(dy), _ptr(gres), _ptr(dslope), _ptr(bias_grad),
                                           _ptr(scratch), _stream()), "gs_pnorm_backward")

    def slice_stats(self, x, co, C, mean_rstd, eps=1e-5):
        """mean / rstd [N][2][C] of channels [co, co + C) of x (any NHWC / NDHWC activation tensor): gs_slice_stats +
        gs_inorm_finalize"""
        N = x.shape[0]
        pixels = x.numel() // (N * x.shape[-1])
        slots = int(self.lib.gs_slice_stats_slots(pixels))
        part = torch.empty(N * slots * 2 * C, dtype=torch.float32, device=x.device)
        L.check(self.lib.gs_slice_stats(_ptr(x), N, pixels, x.shape[-1], co, C, _ptr(part), _stream()), "gs_slice_stats")
        self.inorm_finalize(part, N, slots, C, pixels, mean_rstd, eps)

    def add_views(self, dst, src, C, dst_co=0, src_co=0, accumulate=True):
        pixels = dst.numel() // dst.shape[-1]
        L.check(self.lib.gs_add_views(_ptr(dst), dst.shape[-1], dst_co, _ptr(src), src.shape[-1], src_co, pixels, C,
                                      int(accumulate), _stream()), "gs_add_views")

    def repeat_backward(self, g, g_img, C, g_co=0):
        N, Cin = g_img.shape[0], g_img.shape[1]
        L.check(self.lib.gs_repeat_backward(_ptr(g), g.shape[-1], g_co, _ptr(g_img), N, Cin, C,
                                            g_img.numel() // (N * Cin), _stream()), "gs_repeat_backward")

    # ---- network boundary -----------------------------------------------------------------------------------
    @staticmethod
    def _img_dims(img):
        """(N, C, rows, W) of an NCHW image or NCDHW volume: the layout-only kernels see a volume as D*H rows"""
        N, Cc = img.shape[0], img.shape[1]
        return N, Cc, img.numel() // (N * Cc * img.shape[-1]), img.shape[-1]

    def image_to_act(self, img, act_t):
        N, Cc, H, W = self._img_dims(img)
        L.check(self.lib.gs_image_to_act(_ptr(img), _ptr(act_t), N, Cc, H, W, act_t.shape[-1], _stream()),
                "gs_image_to_act")

    # ---- channel windows (the balanced CycleGAN, pix2pix's conditional input: csrc/image.hip, csrc/loss.hip) ------------
    @staticmethod
    def _dense_f32(t, what):
        """ValueError before any launch: a dense fp32 [N, C, *spatial] tensor"""
        if not torch.is_tensor(t) or t.dim() not in (4, 5):
            raise ValueError(f"{what}: an [N, C, H, W] or [N, C, D, H, W] tensor expected, got "
                             f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: fp32 expected, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: a dense (contiguous) tensor expected, got strides {t.stride()} for shape {tuple(t.shape)}")
        if t.numel() == 0:
            raise ValueError(f"{what}: empty tensor {tuple(t.shape)}")

    @classmethod
    def _window(cls, t, c0, c1, what):
        """(pointer to channel c0 of sample 0, sample stride in floats, channels, S) of the window [c0, c1) of dense `t`"""
        cls._dense_f32(t, what)
        c0, c1 = int(c0), int(c1)
        if not 0 <= c0 < c1 <= t.shape[1]:
            raise ValueError(f"{what}: the channel window [{c0}, {c1}) does not lie inside the {t.shape[1]} channels")
        S = t.numel() // (t.shape[0] * t.shape[1])
        return C.c_void_p(t.data_ptr() + c0 * S * 4), t.shape[1] * S, c1 - c0, S

    @staticmethod
    def _same_extent(a, b, what):
        if a.shape[0] != b.shape[0] or tuple(a.shape[2:]) != tuple(b.shape[2:]) or a.device != b.device:
            raise ValueError(f"{what}: the tensors differ in batch, spatial extent or device: {tuple(a.shape)} vs "
                             f"{tuple(b.shape)}")

    def image_cat_to_act(self, srcs, act_t):
        """srcs = [(dense fp32 tensor, c0, c1)] (1..4): torch.cat([t[:, c0:c1] for ...], dim=1) -> channels-last act_t in one pass,
        neither the slices nor the concatenation exist in memory (gs_image_cat_to_act)"""
        K = len(srcs)
        if not 1 <= K <= L.CAT_MAX_SRCS:
            raise ValueError(f"image_cat_to_act: 1..{L.CAT_MAX_SRCS} channel sources, got {K}")
        win = [self._window(t, c0, c1, f"image_cat_to_act: source {k}") for k, (t, c0, c1) in enumerate(srcs)]
        for t, _, _ in srcs[1:]:
            self._same_extent(srcs[0][0], t, "image_cat_to_act")
        t0 = srcs[0][0]
        if not act_t.is_contiguous() or act_t.dtype != self.act_dtype:
            raise ValueError("image_cat_to_act: the activation must be a dense channels-last buffer of the activation dtype")
        if act_t.shape[0] != t0.shape[0] or tuple(act_t.shape[1:-1]) != tuple(t0.shape[2:]):
            raise ValueError(f"image_cat_to_act: activation {tuple(act_t.shape)} does not match the sources {tuple(t0.shape)}")
        if sum(w[2] for w in win) > act_t.shape[-1] or act_t.shape[-1] % 8:
            raise ValueError(f"image_cat_to_act: {sum(w[2] for w in win)} source channels do not fit the activation's "
                             f"{act_t.shape[-1]} (a multiple of 8)")
        ptrs = (C.c_void_p * K)(*[w[0] for w in win])
        strides = (C.c_int64 * K)(*[w[1] for w in win])
        chans = (C.c_int32 * K)(*[w[2] for w in win])
        L.check(self.lib.gs_image_cat_to_act(ptrs, strides, chans, K, _ptr(act_t), t0.shape[0], win[0][3], act_t.shape[-1],
                                             _stream()), "gs_image_cat_to_act")

    def image_cat_to_act_backward(self, g, grads, channels):
        """gradient of image_cat_to_act: grads[k] = dense fp32 [N, channels[k], *spatial] or None (left alone)"""
        K = len(channels)
        if len(grads) != K or not 1 <= K <= L.CAT_MAX_SRCS:
            raise ValueError(f"image_cat_to_act_backward: one gradient slot per source (1..{L.CAT_MAX_SRCS}), got {len(grads)} "
                             f"for {K} sources")
        ref = next((t for t in grads if t is not None), None)
        if ref is None:
            raise ValueError("image_cat_to_act_backward: no source asks for a gradient")
        for k, t in enumerate(grads):
            if t is None:
                continue
            self._dense_f32(t, f"image_cat_to_act_backward: gradient {k}")
            self._same_extent(ref, t, "image_cat_to_act_backward")
            if t.shape[1] != channels[k]:
                raise ValueError(f"image_cat_to_act_backward: gradient {k} has {t.shape[1]} channels, its source {channels[k]}")
        if not g.is_contiguous() or g.shape[0] != ref.shape[0] or tuple(g.shape[1:-1]) != tuple(ref.shape[2:]) or \
                sum(channels) > g.shape[-1]:
            raise ValueError(f"image_cat_to_act_backward: activation gradient {tuple(g.shape)} does not match "
                             f"{tuple(ref.shape)} / {sum(channels)} channels")
        ptrs = (C.c_void_p * K)(*[(t.data_ptr() if t is not None else None) for t in grads])
        chans = (C.c_int32 * K)(*[int(c) for c in channels])
        S = ref.numel() // (ref.shape[0] * ref.shape[1])
        L.check(self.lib.gs_image_cat_to_act_backward(_ptr(g), ptrs, chans, K, ref.shape[0], S, g.shape[-1], _stream()),
                "gs_image_cat_to_act_backward")

    def channel_embed(self, src, dst, c0):
        """dst [N, C, *spatial] = zeros with src [N, t, *spatial] at channels [c0, c0 + t), one pass (gs_channel_embed)"""
        self._dense_f32(src, "channel_embed: src")
        self._dense_f32(dst, "channel_embed: dst")
        self._same_extent(src, dst, "channel_embed")
        c0, t, Cd = int(c0), src.shape[1], dst.shape[1]
        if not 0 <= c0 <= c0 + t <= Cd:
            raise ValueError(f"channel_embed: the channel window [{c0}, {c0 + t}) does not lie inside the {Cd} channels")
        if dst.shape[0] * Cd > 65535:
            raise ValueError(f"channel_embed: N * C = {dst.shape[0] * Cd} exceeds 65535")
        S = dst.numel() // (dst.shape[0] * Cd)
        L.check(self.lib.gs_channel_embed(_ptr(src), _ptr(dst), dst.shape[0], Cd, c0, t, S, _stream()), "gs_channel_embed")

    def l1_window(self, a, c0, c1, b, loss=None, grad_b=None, grad_scale=None):
        """gs_l1 of a[:, c0:c1] (a window of a dense tensor, never materialised) and dense b; grad_b = d/db, dense like b"""
        pa, stride, ch, S = self._window(a, c0, c1, "l1_window: a")
        self._dense_f32(b, "l1_window: b")
        self._same_extent(a, b, "l1_window")
        if b.shape[1] != ch:
            raise ValueError(f"l1_window: b has {b.shape[1]} channels, the window [{c0}, {c1}) {ch}")
        if grad_b is not None:
            self._dense_f32(grad_b, "l1_window: grad_b")
            if grad_b.shape != b.shape:
                raise ValueError(f"l1_window: grad_b {tuple(grad_b.shape)} must have b's shape {tuple(b.shape)}")
        L.check(self.lib.gs_l1_window(pa, stride, _ptr(b), a.shape[0], ch * S, _ptr(loss), _ptr(grad_b), _ptr(grad_scale),
                                      _stream()), "gs_l1_window")

    def _ssim_window_args(self, x, c0, c1, y, what):
        px, stride, ch, S = self._window(x, c0, c1, f"{what}: x")
        self._dense_f32(y, f"{what}: y")
        self._same_extent(x, y, what)
        if y.shape[1] != ch:
            raise ValueError(f"{what}: y has {y.shape[1]} channels, the window [{c0}, {c1}) {ch}")
        H, W = y.shape[-2], y.shape[-1]
        if H <= 10 or W <= 10:
            raise ValueError(f"{what}: planes of more than 10 x 10 pixels needed (11-tap window), got {H} x {W}")
        return px, stride, ch * S // (H * W), y.numel() // (H * W), H, W

    def ssim_distance_window(self, x, c0, c1, y, out):
        """gs_ssim_distance of x[:, c0:c1] (a window, never materialised) and dense y; evaluated in double, rounded once"""
        px, stride, planes, NC, H, W = self._ssim_window_args(x, c0, c1, y, "ssim_distance_window")
        scratch = torch.empty(self.lib.gs_ssim_scratch_floats(NC, H, W), dtype=torch.float64, device=y.device)   # one per tile
        L.check(self.lib.gs_ssim_distance_window(px, stride, planes, _ptr(y), NC, H, W, _ptr(out), _ptr(scratch), _stream()),
                "gs_ssim_distance_window")

    def ssim_distance_window_backward(self, x, c0, c1, y, grad_y, grad_scale=None):
        """gradient of ssim_distance_window w.r.t. the dense image y"""
        px, stride, planes, NC, H, W = self._ssim_window_args(x, c0, c1, y, "ssim_distance_window_backward")
        self._dense_f32(grad_y, "ssim_distance_window_backward: grad_y")
        if grad_y.shape != y.shape:
            raise ValueError(f"ssim_distance_window_backward: grad_y {tuple(grad_y.shape)} must have y's shape {tuple(y.shape)}")
        scratch = torch.empty(self.lib.gs_ssim_backward_scratch_floats(NC, H, W), dtype=torch.float32, device=y.device)
        L.check(self.lib.gs_ssim_distance_window_backward(px, stride, planes, _ptr(y), NC, H, W, _ptr(grad_scale), _ptr(grad_y),
                                                          _ptr(scratch), _stream()), "gs_ssim_distance_window_backward")

    def act_to_image(self, act_t, img, act="none"):
        N, Cc, H, W = self._img_dims(img)
        L.check(self.lib.gs_act_to_image(_ptr(act_t), _ptr(img), N, Cc, H, W, act_t.shape[-1], L.ACT[act],
                                         _stream()), "gs_act_to_image")

    def act_to_image_backward(self, g_img, out_img, g_act, act="none"):
        N, Cc, H, W = self._img_dims(g_img)
        L.check(self.lib.gs_act_to_image_backward(_ptr(g_img), _ptr(out_img), _ptr(g_act), N, Cc, H, W,
                                                  g_act.shape[-1], L.ACT[act], _stream()),
                "gs_act_to_image_backward")

    def image_to_act_backward(self, g_pad, g_img, fold=0, fold_mode="reflect", accumulate=False):
        N, Cc = g_img.shape[0], g_img.shape[1]
        D, H, W = g_img.shape[2:] if g_img.dim() == 5 else (1,) + tuple(g_img.shape[2:])
        L.check(self.lib.gs_image_to_act_backward(_ptr(g_pad), _ptr(g_img), N, Cc, D, H, W, g_pad.shape[-1], fold,
                                                  L.BORDER[fold_mode], int(accumulate), _stream()),
                "gs_image_to_act_backward")

    # ---- W-fold boundary transforms of the k7 stem / last layer (csrc/wfold.hip) ---------------------------------
    def image_unfold(self, img, act_t, k, p, border):
        N, Cc, rows, W = self._img_dims(img)
        L.check(self.lib.gs_image_unfold(_ptr(img), _ptr(act_t), N, Cc, rows, W, act_t.shape[-1], k, p,
                                         L.BORDER[border], _stream()), "gs_image_unfold")

    def image_unfold_backward(self, g, g_img, k, p, fold, border, accumulate=False):
        N, Cc = g_img.shape[0], g_img.shape[1]
        D, H, W = g_img.shape[2:] if g_img.dim() == 5 else (1,) + tuple(g_img.shape[2:])
        L.check(self.lib.gs_image_unfold_backward(_ptr(g), _ptr(g_img), N, Cc, D, H, W, g.shape[-1], k, p, fold,
                                                  L.BORDER[border], int(accumulate), _stream()),
                "gs_image_unfold_backward")

    def shiftadd_to_image(self, z, bias, img, k, act="none"):
        if is_twin(bias):
            return self.twin_shiftadd_to_image(z, bias, img, k, act=act)
        N, Cc, rows, W = self._img_dims(img)
        L.check(self.lib.gs_shiftadd_to_image(_ptr(z), _ptr(bias), _ptr(img), N, Cc, rows, W, z.shape[-1], k,
                                              L.ACT[act], _stream()), "gs_shiftadd_to_image")

    def shiftadd_to_image_backward(self, g_img, out_img, gz, k, act="none"):
        N, Cc, rows, W = self._img_dims(g_img)
        L.check(self.lib.gs_shiftadd_to_image_backward(_ptr(g_img), _ptr(out_img), _ptr(gz), N, Cc, rows, W,
                                                       gz.shape[-1], k, L.ACT[act], _stream()),
                "gs_shiftadd_to_image_backward")

    # ---- losses ---------------------------------------------------------------------------------------------
    # ---- device-side image preprocessing (csrc/imgproc.hip) ---------------------------------------------
    def u8_resample_h(self, img, out, bounds, kk):
        """Pillow's horizontal 8-bit pass: img (H, W, C) uint8 -> out (H, W', C) uint8; bounds (W', 2), kk (W', ksize) int32"""
        H, W, Cc = img.shape
        L.check(self.lib.gs_u8_resample_h(_ptr(img), _ptr(out), H, W, out.shape[1], Cc, _ptr(bounds), _ptr(kk),
                                          kk.shape[1], _stream()), "gs_u8_resample_h")

    def u8_resample_v(self, tmp, out, bounds, kk):
        """Pillow's vertical 8-bit pass: tmp (H, W', C) uint8 -> out (H', W', C) uint8 (the image between two resizes)"""
        H, W2, Cc = tmp.shape
        L.check(self.lib.gs_u8_resample_v(_ptr(tmp), _ptr(out), H, W2, out.shape[0], Cc, _ptr(bounds), _ptr(kk),
                                          kk.shape[1], _stream()), "gs_u8_resample_v")

    def u8_resample_v_crop_normalize(self, tmp, out, out_h, bounds, kk, top, left, flip):
        """Pillow's vertical pass on the crop window + flip + ToTensor + Normalize(0.5, 0.5): tmp (H, W', C) uint8 ->
        out (C, fh, fw) fp32 (a contiguous slice of the NCHW batch)"""
        H, W2, Cc = tmp.shape
        assert out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] == Cc
        L.check(self.lib.gs_u8_resample_v_crop_normalize(_ptr(tmp), _ptr(out), H, W2, out_h, Cc, _ptr(bounds), _ptr(kk),
                                                         kk.shape[1], int(top), int(left), out.shape[1], out.shape[2],
                                                         int(bool(flip)), _stream()),
                "gs_u8_resample_v_crop_normalize")

    U8_TMP_ALIGN = 256

    @staticmethod
    def u8_batch_table(items_host, srcs, Cc, guard=0):
        """(ctypes array of GsU8BatchItem, bytes of the tmp arena) for a batch: `items_host` carry the geometry of each
        image (in_h, in_w, rh, rw, row0, rows, top, left, flip) and the (bounds, kk) tensor pairs of both axes, `srcs` the
        (in_h, in_w, C) uint8 tensors. The slices of the arena follow each other, each rounded up to U8_TMP_ALIGN bytes, with
        `guard` bytes in front of, between and behind them. Pure host code."""
        table = (L.U8BatchItem * len(items_host))()
        off = int(guard)
        for d, it, src in zip(table, items_host, srcs):
            (bh, kh), (bv, kv) = it.tables_h, it.tables_v
            assert src.dtype == torch.uint8 and src.is_contiguous() and src.numel() == it.in_h * it.in_w * Cc, src.shape
            assert bh.shape == (it.rw, 2) and bv.shape == (it.rh, 2) and kh.shape[0] == it.rw and kv.shape[0] == it.rh
            assert all(t.dtype == torch.int32 and t.is_contiguous() for t in (bh, kh, bv, kv))
            d.src, d.bounds_h, d.kk_h, d.bounds_v, d.kk_v = (t.data_ptr() for t in (src, bh, kh, bv, kv))
            d.in_h, d.in_w, d.rh, d.rw, d.row0, d.rows = it.in_h, it.in_w, it.rh, it.rw, it.row0, it.rows
            d.top, d.left, d.flip = int(it.top), int(it.left), int(bool(it.flip))
            d.ksize_h, d.ksize_v, d.tmp_off = kh.shape[1], kv.shape[1], off
            size = max(it.rows, 0) * it.rw * Cc
            off += -(-size // HipOps.U8_TMP_ALIGN) * HipOps.U8_TMP_ALIGN + int(guard)
        return table, off

    def u8_batch_check(self, table, Cc, fh, fw, tmp_bytes):
        """the library's validation of a HOST descriptor table; raises its error (the kernels cannot report one)"""
        L.check(self.lib.gs_u8_batch_check(table, len(table), Cc, fh, fw, tmp_bytes), "gs_u8_batch_check")

    def u8_batch_resample(self, items_host, srcs, out, Cc, tmp=None, guard=0):
        """Both Pillow passes + crop + flip + ToTensor + Normalize(0.5, 0.5) for a whole batch of decoded images of different
        sizes in two launches: srcs[i] (in_h, in_w, C) uint8 on the device -> out[i] of the fp32 (n, C, fh, fw) batch. One
        descriptor table, validated on the host and uploaded with one copy; one tmp arena that holds, per image, only the
        rows its vertical pass reads. Returns (host table, tmp arena); `tmp` / `guard` let a test own the arena."""
        n = len(items_host)
        assert n == len(srcs) == out.shape[0] and out.dim() == 4 and out.shape[1] == Cc, (n, len(srcs), out.shape, Cc)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.is_cuda and all(s.is_cuda for s in srcs)
        fh, fw = out.shape[2], out.shape[3]
        table, nbytes = self.u8_batch_table(items_host, srcs, Cc, guard)
        self.u8_batch_check(table, Cc, fh, fw, nbytes)
        if tmp is None:
            tmp = torch.empty(nbytes, dtype=torch.uint8, device=out.device)
        assert tmp.dtype == torch.uint8 and tmp.is_contiguous() and tmp.numel() >= nbytes and tmp.device == out.device
        staged = torch.empty(C.sizeof(table), dtype=torch.uint8, pin_memory=True)
        staged.copy_(torch.frombuffer(table, dtype=torch.uint8))
        dev = staged.to(out.device, non_blocking=True)
        L.check(self.lib.gs_u8_batch_resample_h(_ptr(dev), n, Cc, _ptr(tmp), max(it.rw for it in items_host),
                                                max(it.rows for it in items_host), _stream()), "gs_u8_batch_resample_h")
        L.check(self.lib.gs_u8_batch_resample_v_crop_normalize(_ptr(dev), n, Cc, _ptr(tmp), fh, fw, _ptr(out), _stream()),
                "gs_u8_batch_resample_v_crop_normalize")
        return table, tmp

    # ---- device-side multi-modal 2-D samples (csrc/imgstack.hip) ------------------------------------------
    IMG_DTYPES = {torch.uint8: L.IMG_DTYPES["uint8"], torch.float32: L.IMG_DTYPES["float32"]}

    @staticmethod
    def img_stack_table(items_host):
        """ctypes array of GsImgStackItem for a batch. Each of `items_host` carries `src` — a contiguous (in_h, in_w) or
        (in_h, in_w, c) uint8 / fp32 tensor ((c, in_h, in_w) with `hwc` False), or None for `c` zero channels — `taps_y` / `taps_x` (the tap tables of its two
        axes: objects with `idx` int32 [n_out, 4], `w` fp32 [n_out, 4] and the `n_in` they were built for), `c`, `item`,
        `c0`, `lo`, `hi`, `rescale`, `noise_std` and `key` (two 32-bit words). A table built for another source size is
        refused here: its indices are the only thing between the kernel and a read outside the image. Pure host code."""
        table = (L.ImgStackItem * len(items_host))()
        for d, it in zip(table, items_host):
            d.item, d.c0, d.c = int(it.item), int(it.c0), int(it.c)
            if it.src is None:
                continue
            src, hwc = it.src, bool(getattr(it, "hwc", True))       # hwc False: a (c, in_h, in_w) source, planes apart
            assert src.dtype in HipOps.IMG_DTYPES and src.is_contiguous() and src.dim() in (2, 3), (src.dtype, src.shape)
            assert hwc or src.dim() == 3, src.shape
            in_h, in_w = src.shape[:2] if hwc else src.shape[1:]
            assert (1 if src.dim() == 2 else src.shape[2 if hwc else 0]) == d.c, (src.shape, d.c)
            for taps, n_in in ((it.taps_y, in_h), (it.taps_x, in_w)):
                assert taps.n_in == n_in and taps.idx.shape == taps.w.shape == (taps.idx.shape[0], 4), (taps.n_in, n_in)
                assert taps.idx.dtype == torch.int32 and taps.w.dtype == torch.float32
                assert taps.idx.is_contiguous() and taps.w.is_contiguous()
            d.src, d.idx_y, d.w_y, d.idx_x, d.w_x = (t.data_ptr() for t in (src, it.taps_y.idx, it.taps_y.w, it.taps_x.idx,
                                                                            it.taps_x.w))
            d.dtype, d.hwc, d.in_h, d.in_w = HipOps.IMG_DTYPES[src.dtype], int(hwc), in_h, in_w
            d.lo, d.hi, d.rescale, d.noise_std = float(it.lo), float(it.hi), int(bool(it.rescale)), float(it.noise_std or 0.0)
            d.key0, d.key1 = int(it.key[0]) & 0xFFFFFFFF, int(it.key[1]) & 0xFFFFFFFF
        return table

    def img_stack_check(self, table, N, Cc, H, W):
        """the library's validation of a HOST descriptor table; raises its error (the kernel cannot report one)"""
        L.check(self.lib.gs_img_stack_check(table, len(table), N, Cc, H, W), "gs_img_stack_check")

    def img_stack(self, items_host, out):
        """Bicubic tensor resize + clamp + min-max + noise plane + channel concat of every (sample, modality) of a batch in
        one launch: out fp32 (N, C, H, W) on the device, every element written once (zeros where an item has no source).
        One descriptor table, validated on the host and uploaded with one copy; nothing synchronises. Returns the host
        table. The caller vouches for the tap tables: every `idx` of `taps_y` / `taps_x` must lie in [0, in_h) / [0, in_w)
        of its source. The tables live on the device and are not read back; what is checked here is only the `n_in` they
        were declared for, so build them with data/multimodal_images.py `bicubic_taps`, as the pipeline does."""
        assert out.dim() == 4 and out.is_contiguous() and out.dtype == torch.float32 and out.is_cuda, (out.shape, out.dtype)
        N, Cc, H, W = out.shape
        for it in items_host:
            if it.src is not None:
                assert it.src.device == out.device and it.taps_y.idx.device == out.device and it.taps_x.idx.device == out.device
                assert it.taps_y.idx.shape[0] == H and it.taps_x.idx.shape[0] == W, (it.taps_y.idx.shape, it.taps_x.idx.shape)
        table = self.img_stack_table(items_host)
        self.img_stack_check(table, N, Cc, H, W)
        staged = torch.empty(C.sizeof(table), dtype=torch.uint8, pin_memory=True)
        staged.copy_(torch.frombuffer(table, dtype=torch.uint8))
        dev = staged.to(out.device, non_blocking=True)
        L.check(self.lib.gs_img_stack(_ptr(dev), len(table), _ptr(out), N, Cc, H, W, _stream()), "gs_img_stack")
        return table

    VOL_DTYPES = {torch.float32: 0, torch.int16: 1}

    def patch_zscore(self, volume, start, size, out, scale_to_range=(-1.0, 1.0)):
        """gs_patch_zscore: out (d, h, w) fp32 = z_score_normalize(volume[z:z+d, y:y+h, x:x+w], scale_to_range) for a dense
        (D, H, W) fp32 / int16 volume resident on the device (normalization.py:18-30); scale_to_range None: plain z-score"""
        assert volume.dim() == 3 and volume.is_contiguous() and volume.dtype in self.VOL_DTYPES, (volume.shape, volume.dtype)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == size[0] * size[1] * size[2]
        nws = getattr(self, "_patch_ws", None) or int(self.lib.gs_patch_zscore_ws_floats())
        self._patch_ws = nws
        ws = torch.empty(nws, dtype=torch.float32, device=self.device)        # per launch: stream-safe through the allocator
        st, sz = (C.c_int32 * 3)(*[int(v) for v in start]), (C.c_int32 * 3)(*[int(v) for v in size])
        lo, hi = scale_to_range if scale_to_range else (0.0, 0.0)
        L.check(self.lib.gs_patch_zscore(_ptr(volume), self.VOL_DTYPES[volume.dtype], *volume.shape, st, sz,
                                         int(bool(scale_to_range)), float(lo), float(hi), _ptr(out), _ptr(ws), _stream()),
                "gs_patch_zscore")

    # ---- multi-modal patch sampling (volsample.hip) ---------------------------------------------------------------
    @staticmethod
    def _case_volume(name, t, dtypes, shape=None):
        if not isinstance(t, torch.Tensor) or not (t.is_cuda and t.dim() == 3 and t.is_contiguous() and t.dtype in dtypes):
            got = (tuple(t.shape), t.dtype, str(t.device)) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{name}: expected a dense (D, H, W) device tensor of dtype {sorted(str(d) for d in dtypes)}; "
                             f"got {got}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(t.shape)} differs from the mask's {tuple(shape)}")

    @staticmethod
    def _point(name, t, n):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= n):
            raise ValueError(f"{name}: expected a contiguous int32 device tensor of at least {n} elements")

    def voxel_draw_range_len(self, dims, patch):
        """voxels of the valid zone's box owned by each workgroup of gs_voxel_draw's first pass (0: empty zone)"""
        return int(self.lib.gs_voxel_draw_range_len(*[int(v) for v in dims], (C.c_int32 * 3)(*[int(v) for v in patch])))

    def voxel_draw(self, mask, weight, patch, u, out, focal_A=None, dims_A=None, proportion=None):
        """gs_voxel_draw: one focal point of a resident case into out (int32[4] on the device: z, y, x, fallback_used;
        -1s when the valid zone holds no body voxel / no positive weight). mask: uint8 (D, H, W); weight: None or an fp32 /
        int16 volume of the same shape; u: the host's uniform in [0, 1). focal_A (device int32[3]) + dims_A + proportion make
        it the stochastic-focal draw of domain B. Enqueued on the current stream; nothing syncs."""
        self._case_volume("mask", mask, (torch.uint8,))
        if weight is not None:
            self._case_volume("weight", weight, tuple(self.VOL_DTYPES), mask.shape)
        self._point("out", out, 4)
        if focal_A is not None:
            self._point("focal_A", focal_A, 3)
            if dims_A is None or proportion is None:
                raise ValueError("a focal point needs dims_A and proportion")
        nws = getattr(self, "_draw_ws", None) or int(self.lib.gs_voxel_draw_ws_bytes())
        self._draw_ws = nws
        ws = torch.empty(nws // 8, dtype=torch.float64, device=mask.device)     # per launch: private to it
        da = (C.c_int32 * 3)(*[int(v) for v in dims_A]) if focal_A is not None else None
        pr = (C.c_double * 3)(*[float(v) for v in proportion]) if focal_A is not None else None
        L.check(self.lib.gs_voxel_draw(_ptr(mask), _ptr(weight), self.VOL_DTYPES[weight.dtype] if weight is not None else 0,
                                       *mask.shape, (C.c_int32 * 3)(*[int(v) for v in patch]), float(u), _ptr(focal_A), da,
                                       pr, _ptr(out), _ptr(ws), _stream()), "gs_voxel_draw")

    def _mod_table(self, who, volumes, mask, outside, divisor, lo, hi):
        """the per-modality columns of one case as gs_* arguments (csrc/volsample.hip ModTable): checks the mask, every
        volume against it and one outside / divisor / lo / hi entry per volume -> (n, pointers, dtypes, the four columns)"""
        n = len(volumes)
        if n < 1:
            raise ValueError(f"{who}: at least one volume")
        self._case_volume("mask", mask, (torch.uint8,))
        for i, v in enumerate(volumes):
            self._case_volume(f"volume {i}", v, tuple(self.VOL_DTYPES), mask.shape)
        if not all(len(t) == n for t in (outside, divisor, lo, hi)):
            raise ValueError(f"outside / divisor / lo / hi need one entry per volume ({n})")
        cols = [(C.c_float * n)(*[float(v) for v in vals]) for vals in (outside, divisor, lo, hi)]
        return (n, (C.c_void_p * n)(*[v.data_ptr() for v in volumes]),
                (C.c_int32 * n)(*[self.VOL_DTYPES[v.dtype] for v in volumes]), cols)

    @staticmethod
    def _out_f32(out, shape):
        shape = tuple(int(v) for v in shape)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                and tuple(out.shape) == shape):
            raise ValueError(f"out: expected a dense fp32 device tensor of shape {shape}")

    def patch_clip_minmax(self, volumes, mask, point, patch, outside, divisor, lo, hi, out):
        """gs_patch_clip_minmax: out [C, d, h, w] fp32 = the patch around `point` (device int32[3]) of every volume of one
        case: where(mask, v, outside) / divisor, clamped to [lo, hi], min-max normalised to [-1, 1]. volumes: C fp32 / int16
        (D, H, W) device tensors; outside / divisor / lo / hi: C host numbers each."""
        n, ptrs, dts, cols = self._mod_table("patch_clip_minmax", volumes, mask, outside, divisor, lo, hi)
        self._point("point", point, 3)
        self._out_f32(out, (n, *patch))
        L.check(self.lib.gs_patch_clip_minmax(ptrs, dts, n, _ptr(mask), *mask.shape, (C.c_int32 * 3)(*[int(v) for v in patch]),
                                              _ptr(point), *cols, _ptr(out), _stream()), "gs_patch_clip_minmax")

    @staticmethod
    def _matrix(matrix):
        m = [float(v) for row in matrix for v in (row if hasattr(row, "__len__") else [row])]
        if len(m) != 9:
            raise ValueError(f"matrix: expected 9 numbers (3 x 3, row-major); got {len(m)}")
        return (C.c_double * 9)(*m)

    @staticmethod
    def _lattice(field):
        """(grid as int32[3], device pointer) of an elastic field: a contiguous float64 device tensor [3, G0, G1, G2]"""
        if not (isinstance(field, torch.Tensor) and field.is_cuda and field.dtype == torch.float64 and field.dim() == 4
                and field.shape[0] == 3 and field.is_contiguous()):
            got = (tuple(field.shape), field.dtype, str(field.device)) if isinstance(field, torch.Tensor) else type(field).__name__
            raise ValueError(f"field: expected a contiguous float64 device tensor of shape [3, G0, G1, G2]; got {got}")
        return (C.c_int32 * 3)(*[int(v) for v in field.shape[1:]]), _ptr(field)

    def _gather_clip_minmax(self, sym, volumes, mask, point, patch, matrix, lattice, outside, divisor, lo, hi, out):
        """gs_patch_affine_clip_minmax (lattice = ()) or gs_patch_elastic_clip_minmax (lattice = (grid, field pointer))"""
        n, ptrs, dts, cols = self._mod_table(sym[3:], volumes, mask, outside, divisor, lo, hi)
        self._point("point", point, 3)
        self._out_f32(out, (n, *patch))
        L.check(getattr(self.lib, sym)(ptrs, dts, n, _ptr(mask), *mask.shape, _ptr(point),
                                       (C.c_int32 * 3)(*[int(v) for v in patch]), self._matrix(matrix), *lattice, *cols,
                                       _ptr(out), _stream()), sym)

    def _gather_raw(self, sym, volume, start, size, matrix, lattice, fill, out):
        """gs_patch_affine (lattice = ()) or gs_patch_elastic (lattice = (grid, field pointer))"""
        self._case_volume("volume", volume, tuple(self.VOL_DTYPES))
        self._out_f32(out, size)
        st, sz = (C.c_int32 * 3)(*[int(v) for v in start]), (C.c_int32 * 3)(*[int(v) for v in size])
        L.check(getattr(self.lib, sym)(_ptr(volume), self.VOL_DTYPES[volume.dtype], *volume.shape, st, sz,
                                       self._matrix(matrix), *lattice, float(fill), _ptr(out), _stream()), sym)

    def patch_affine_clip_minmax(self, volumes, mask, point, patch, matrix, outside, divisor, lo, hi, out):
        """gs_patch_affine_clip_minmax: patch_clip_minmax through a 3 x 3 matrix — the trilinear gather of
        data/utils/patch_affine.py (mask, then interpolate), then the same chain. matrix: 9 numbers, row-major, or 3 x 3."""
        self._gather_clip_minmax("gs_patch_affine_clip_minmax", volumes, mask, point, patch, matrix, (), outside, divisor, lo,
                                 hi, out)

    def patch_affine(self, volume, start, size, matrix, fill, out):
        """gs_patch_affine: out (d, h, w) fp32 = the raw trilinear gather of the window [start, start + size) of a dense
        (D, H, W) fp32 / int16 device volume through `matrix`, `fill` outside the volume; no mask, no normalisation"""
        self._gather_raw("gs_patch_affine", volume, start, size, matrix, (), fill, out)

    def patch_elastic_clip_minmax(self, volumes, mask, point, patch, matrix, field, outside, divisor, lo, hi, out):
        """gs_patch_elastic_clip_minmax: patch_affine_clip_minmax with a free-form deformation in front of the matrix.
        field: float64 device tensor [3, G0, G1, G2], control-point displacements in voxels (include/ganslate_hip.h)."""
        self._gather_clip_minmax("gs_patch_elastic_clip_minmax", volumes, mask, point, patch, matrix, self._lattice(field),
                                 outside, divisor, lo, hi, out)

    def patch_elastic(self, volume, start, size, matrix, field, fill, out):
        """gs_patch_elastic: patch_affine with a free-form deformation in front of the matrix (field as above)"""
        self._gather_raw("gs_patch_elastic", volume, start, size, matrix, self._lattice(field), fill, out)

    @staticmethod
    def _intensity(rows, n, bias_lattice):
        """(GsPatchIntensity[n], bias_grid as int32[3] or None, device pointer or None): rows of (gamma, contrast,
        brightness, noise_std, bias, key0, key1), one per modality (None: the neutral row); bias_lattice: None or a
        contiguous float64 device tensor [G0, G1, G2]"""
        if rows is None or len(rows) != n:
            raise ValueError(f"intensity: expected one row per modality ({n}); got {None if rows is None else len(rows)}")
        table = (L.PatchIntensity * n)()
        for c, r in enumerate(rows):
            r = (1.0, 1.0, 0.0, 0.0, 0.0, 0, 0) if r is None else r
            if len(r) != 7:
                raise ValueError(f"intensity row {c}: expected (gamma, contrast, brightness, noise_std, bias, key0, key1)")
            t = table[c]
            t.gamma, t.contrast, t.brightness, t.noise_std, t.bias = [float(v) for v in r[:5]]
            t.key0, t.key1 = int(r[5]) & 0xffffffff, int(r[6]) & 0xffffffff
        if bias_lattice is None:
            return table, None, None
        b = bias_lattice
        if not (isinstance(b, torch.Tensor) and b.is_cuda and b.dtype == torch.float64 and b.dim() == 3 and b.is_contiguous()):
            got = (tuple(b.shape), b.dtype, str(b.device)) if isinstance(b, torch.Tensor) else type(b).__name__
            raise ValueError(f"bias_lattice: expected a contiguous float64 device tensor of shape [G0, G1, G2]; got {got}")
        return table, (C.c_int32 * 3)(*[int(v) for v in b.shape]), _ptr(b)

    def patch_augment_clip_minmax(self, volumes, mask, point, patch, matrix, field, intensity, bias_lattice, outside, divisor,
                                  lo, hi, out):
        """gs_patch_augment_clip_minmax: patch_elastic_clip_minmax (field None: patch_affine_clip_minmax) with the intensity
        chain of data/utils/patch_intensity.py between the min-max step and 2 n - 1. intensity: one row (gamma, contrast,
        brightness, noise_std, bias, key0, key1) per volume; bias_lattice: None or a float64 device tensor [G0, G1, G2]
        in [-1, 1], shared by the volumes (include/ganslate_hip.h)."""
        sym = "gs_patch_augment_clip_minmax"
        n, ptrs, dts, cols = self._mod_table(sym[3:], volumes, mask, outside, divisor, lo, hi)
        self._point("point", point, 3)
        self._out_f32(out, (n, *patch))
        lattice = (None, None) if field is None else self._lattice(field)
        L.check(self.lib.gs_patch_augment_clip_minmax(ptrs, dts, n, _ptr(mask), *mask.shape, _ptr(point),
                                                      (C.c_int32 * 3)(*[int(v) for v in patch]), self._matrix(matrix),
                                                      *lattice, *self._intensity(intensity, n, bias_lattice), *cols,
                                                      _ptr(out), _stream()), sym)

    def patch_zscore_intensity(self, volume, start, size, out, intensity, bias_lattice=None, scale_to_range=(-1.0, 1.0)):
        """gs_patch_zscore_intensity: patch_zscore with rescale and the intensity chain on n = (t - min t) / (max t - min t);
        intensity: one row (gamma, contrast, brightness, noise_std, bias, key0, key1); bias_lattice as above"""
        assert volume.dim() == 3 and volume.is_contiguous() and volume.dtype in self.VOL_DTYPES, (volume.shape, volume.dtype)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == size[0] * size[1] * size[2]
        nws = getattr(self, "_patch_ws", None) or int(self.lib.gs_patch_zscore_ws_floats())
        self._patch_ws = nws
        ws = torch.empty(nws, dtype=torch.float32, device=self.device)        # per launch: stream-safe through the allocator
        st, sz = (C.c_int32 * 3)(*[int(v) for v in start]), (C.c_int32 * 3)(*[int(v) for v in size])
        lo, hi = scale_to_range
        L.check(self.lib.gs_patch_zscore_intensity(_ptr(volume), self.VOL_DTYPES[volume.dtype], *volume.shape, st, sz,
                                                   float(lo), float(hi), *self._intensity([intensity], 1, bias_lattice),
                                                   _ptr(out), _ptr(ws), _stream()), "gs_patch_zscore_intensity")

    def volume_prepare(self, volumes, mask, extra_masks, target, outside, divisor, lo, hi, out=None, masks_out=None):
        """gs_volume_prepare: one whole case for the val / test engines -> (out, [masks]). volumes: C fp32 / int16
        (D, H, W) device tensors; mask: the body mask (uint8, non-zero = inside); extra_masks: up to VM_MAX_LABELS further
        uint8 masks; target: (Dt, Ht, Wt) — every axis comes out as max(size, target), padded centred with the minimum of
        where(mask, v, outside) (each mask with its own minimum); then / divisor, clamp to [lo, hi], min-max to [-1, 1].
        out: fp32 [C, Do, Ho, Wo]; masks: uint8 [Do, Ho, Wo] each, the body mask first. Enqueued on the current stream;
        nothing syncs."""
        if not 1 <= len(volumes) <= L.PATCH_MAX_MODALITIES:
            raise ValueError(f"volume_prepare: between 1 and {L.PATCH_MAX_MODALITIES} volumes; got {len(volumes)}")
        extra_masks = list(extra_masks or [])
        if len(extra_masks) > L.VM_MAX_LABELS:
            raise ValueError(f"volume_prepare: at most {L.VM_MAX_LABELS} extra masks; got {len(extra_masks)}")
        n, ptrs, dts, cols = self._mod_table("volume_prepare", volumes, mask, outside, divisor, lo, hi)
        for i, m in enumerate(extra_masks):
            self._case_volume(f"extra mask {i}", m, (torch.uint8,), mask.shape)
        target = [int(v) for v in target]
        if len(target) != 3 or min(target) < 1:
            raise ValueError(f"target must be three positive sizes (D, H, W); got {target}")
        shape = tuple(max(s, t) for s, t in zip(mask.shape, target))
        masks_in = [mask] + extra_masks
        if out is None:
            out = torch.empty((n, *shape), dtype=torch.float32, device=mask.device)
        if masks_out is None:
            masks_out = [torch.empty(shape, dtype=torch.uint8, device=mask.device) for _ in masks_in]
        self._out_f32(out, (n, *shape))
        if len(masks_out) != len(masks_in):
            raise ValueError(f"masks_out: one tensor per mask ({len(masks_in)})")
        for i, m in enumerate(masks_out):
            self._case_volume(f"masks_out {i}", m, (torch.uint8,), shape)
        nws = getattr(self, "_prepare_ws", None) or int(self.lib.gs_volume_prepare_ws_bytes())
        self._prepare_ws = nws
        ws = torch.empty(nws // 4, dtype=torch.float32, device=mask.device)     # per launch: private to it
        mi = (C.c_void_p * len(masks_in))(*[m.data_ptr() for m in masks_in])
        mo = (C.c_void_p * len(masks_in))(*[m.data_ptr() for m in masks_out])
        L.check(self.lib.gs_volume_prepare(ptrs, dts, n, mi, len(masks_in), *mask.shape, (C.c_int32 * 3)(*target), *cols,
                                           _ptr(out), mo, _ptr(ws), _stream()), "gs_volume_prepare")
        return out, list(masks_out)

    def body_mask(self, volume, threshold, out=None, return_rounds=False):
        """gs_body_mask: (mask, info) of a dense (D, H, W) fp32 / int16 device volume — mask uint8 0 / 1 by the definition
        of data/utils/body_mask.py (threshold, largest 6-connected component, per-slice hole filling), info int32[2] on the
        device: voxels of the chosen component and its first voxel's flat index (0, -1: nothing reached the threshold, the
        mask is all zero). Exact and reproducible. Synchronises the current stream a few times (the labelling rounds read a
        device flag back). return_rounds: also the rounds the two labelling phases ran, as a third value."""
        self._case_volume("volume", volume, tuple(self.VOL_DTYPES))
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("body_mask: the threshold is NaN")
        if volume.numel() == 0 or volume.numel() >= 1 << 31:
            raise ValueError(f"body_mask: {tuple(volume.shape)} voxels do not fit 31-bit indices (or there are none)")
        if out is None:
            out = torch.empty(tuple(volume.shape), dtype=torch.uint8, device=volume.device)
        self._case_volume("out", out, (torch.uint8,), volume.shape)
        info = torch.empty(2, dtype=torch.int32, device=volume.device)
        ws = torch.empty(int(self.lib.gs_body_mask_ws_bytes(*volume.shape)) // 8, dtype=torch.int64, device=volume.device)
        L.check(self.lib.gs_body_mask(_ptr(volume), self.VOL_DTYPES[volume.dtype], *volume.shape, threshold, _ptr(out),
                                      _ptr(info), _ptr(ws), _stream()), "gs_body_mask")
        if return_rounds:
            return out, info, [int(v) for v in ws[:1].view(torch.int32).tolist()]
        return out, info

    ADV_MODES = {"lsgan": 0, "vanilla": 1, "wgangp": 2, "nonsaturating": 3}

    def adv_loss(self, x, mode, target_is_real, label, loss=None, grad=None, grad_scale=None):
        """gs_adv_loss: `x` is one discriminator map (B, ...), fp32; nonsaturating reduces per sample (loss: B floats)"""
        L.check(self.lib.gs_adv_loss(_ptr(x), x.numel(), x.shape[0], self.ADV_MODES[mode], int(bool(target_is_real)),
                                     float(label), _ptr(loss), _ptr(grad), _ptr(grad_scale), _stream()), "gs_adv_loss")

    def mse_const(self, x, target, loss=None, grad=None, grad_scale=None):
        L.check(self.lib.gs_mse_const(_ptr(x), x.numel(), float(target), _ptr(loss), _ptr(grad), _ptr(grad_scale),
                                      _stream()), "gs_mse_const")

    def l1(self, a, b, loss=None, grad_a=None, grad_scale=None):
        L.check(self.lib.gs_l1(_ptr(a), _ptr(b), a.numel(), _ptr(loss), _ptr(grad_a), _ptr(grad_scale), _stream()),
                "gs_l1")

    def mean(self, x, out):
        L.check(self.lib.gs_mean(_ptr(x), x.numel(), _ptr(out), _stream()), "gs_mean")

    def scalar_affine(self, xs, rows, consts=None):
        """[c_r + sum_k rows[r][k] * xs[k]] as a fresh fp32 vector [R]; xs = 0-d fp32 device tensors or None (= 0)"""
        K, R = len(xs), len(rows)
        out = torch.empty(R, dtype=torch.float32, device=self.device)
        px = (C.c_void_p * K)(*[(_ptr(x) if x is not None else None) for x in xs])
        m = (C.c_float * (R * K))(*[float(v) for row in rows for v in row])
        c = (C.c_float * R)(*[float(v) for v in consts]) if consts is not None else None
        L.check(self.lib.gs_scalar_affine(px, K, m, c, R, _ptr(out), _stream()), "gs_scalar_affine")
        return out

    # ---- feature taps (CUT) ------------------------------------------------------------------------------------
    def tap_gather(self, src, pid, c):
        """src [n, ..., cs] NHWC activations, pid int64 [P] flat pixel ids -> fp32 [n, P, c]"""
        n, cs = src.shape[0], src.shape[-1]
        pid = pid.contiguous()
        out = torch.empty((n, pid.numel(), c), dtype=torch.float32, device=self.device)
        L.check(self.lib.gs_tap_gather(_ptr(src), n, src.numel() // (n * cs), cs, _ptr(pid), pid.numel(), c, _ptr(out),
                                       _stream()), "gs_tap_gather")
        return out

    def tap_scatter_add(self, dst, pid, g, W, f0=0):
        """dst [n, Hp, Wp, cs] (a gradient on the domain padded by f0) += g [n, P, c] at the unpadded pixels pid"""
        n, cs = dst.shape[0], dst.shape[-1]
        pid, g = pid.contiguous(), g.contiguous().float()
        L.check(self.lib.gs_tap_scatter_add(_ptr(dst), n, dst.numel() // (n * cs), cs, _ptr(pid), pid.numel(), g.shape[-1], W,
                                            dst.shape[-2], f0, _ptr(g), _stream()), "gs_tap_scatter_add")

    def tap_rows_sum(self, g, db):
        g = g.contiguous().float()
        L.check(self.lib.gs_tap_rows_sum(_ptr(g), g.numel() // g.shape[-1], g.shape[-1], _ptr(db), _stream()),
                "gs_tap_rows_sum")

    def zero_fill(self, out):
        """zeroes a dense tensor in place and returns it"""
        nbytes = out.numel() * out.element_size()
        if nbytes % 16 or out.data_ptr() % 16:
            return out.zero_()
        L.check(self.lib.gs_zero_bytes(_ptr(out), nbytes, _stream()), "gs_zero_bytes")
        return out

    def zeros_like_act(self, t):
        return self.zero_fill(torch.empty_like(t))

    def image_tap_gather(self, x, pid, pad):
        N, Cc, H, W = x.shape
        pid = pid.contiguous()
        out = torch.empty((N, pid.numel(), Cc), dtype=torch.float32, device=self.device)
        L.check(self.lib.gs_image_tap_gather(_ptr(x), N, Cc, H, W, pad, _ptr(pid), pid.numel(), _ptr(out), _stream()),
                "gs_image_tap_gather")
        return out

    def image_tap_scatter(self, g, pid, shape, pad):
        N, Cc, H, W = shape
        pid, g = pid.contiguous(), g.contiguous().float()
        gx = torch.empty(shape, dtype=torch.float32, device=self.device)
        L.check(self.lib.gs_image_tap_scatter(_ptr(g), N, Cc, H, W, pad, _ptr(pid), pid.numel(), _ptr(gx), _stream()),
                "gs_image_tap_scatter")
        return gx

    def flip_w_if(self, x, flag):
        """x.flip(-1) where the int32 device flag is set, x otherwise (a copy either way)"""
        x = x.contiguous().float()
        out = torch.empty_like(x)
        L.check(self.lib.gs_flip_w_if(_ptr(x), _ptr(out), x.numel() // x.shape[-1], x.shape[-1], _ptr(flag), _stream()),
                "gs_flip_w_if")
        return out

    def sum2(self, a, b):
        out = torch.empty_like(a)
        L.check(self.lib.gs_sum2_f32(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream()), "gs_sum2_f32")
        return out

    def ssim_distance(self, x, y, out):
        NC = x.numel() // (x.shape[-1] * x.shape[-2])
        H, W = x.shape[-2], x.shape[-1]
        scratch = torch.empty(self.lib.gs_ssim_scratch_floats(NC, H, W), dtype=torch.float32, device=x.device)
        L.check(self.lib.gs_ssim_distance(_ptr(x), _ptr(y), NC, H, W, _ptr(out), _ptr(scratch), _stream()),
                "gs_ssim_distance")

    # ---- MIND structure-consistency loss for images and volumes (mind.hip, mind3d.hip) -------------------------------
    MIND_CONFIG = {"non_local_region_size": 9, "patch_size": 7, "neighbor_size": 3, "gaussian_patch_sigma": 2.0}
    MIND3D_CONFIG = {"non_local_region_size": 3, "patch_size": 5, "neighbor_size": 3, "gaussian_patch_sigma": 2.0}
    # what differs between the two ranks: the prefix of the methods and of the library's four entry points, the tensors'
    # rank, the descriptor's channels, the default config and the words of the refusals
    _MIND = {
        2: dict(name="mind", dim=4, channels=81, config=MIND_CONFIG, noun="image",
                takes="the MIND descriptor takes [N, C, H, W] images (volumes are not supported)"),
        3: dict(name="mind3d", dim=5, channels=27, config=MIND3D_CONFIG, noun="volume",
                takes="the volumetric MIND descriptor takes [N, C, D, H, W] volumes"),
    }

    @staticmethod
    def _mind_check(r, *samples):
        """ValueError before any launch: fp32 dense tensors of the rank's shape on one device, equal in batch and extent"""
        noun = r["noun"]
        for t in samples:
            if t.dim() != r["dim"]:
                raise ValueError(f"{r['takes']}; got {tuple(t.shape)}")
            if t.dtype != torch.float32:
                raise ValueError(f"the MIND kernels take fp32 {noun}s; got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError(f"the MIND kernels take dense (contiguous) {noun}s")
            if t.numel() == 0:
                raise ValueError(f"empty {noun} batch {tuple(t.shape)}")
        a = samples[0]
        for t in samples[1:]:
            if (t.shape[0], *t.shape[2:]) != (a.shape[0], *a.shape[2:]) or t.device != a.device:
                raise ValueError(f"MIND loss: {noun}s differ in batch, extent or device: {tuple(a.shape)} vs {tuple(t.shape)}")

    @staticmethod
    def _mind_args(r, cfg):
        cfg = dict(r["config"], **(cfg or {}))
        return (int(cfg["non_local_region_size"]), int(cfg["patch_size"]), int(cfg["neighbor_size"]),
                float(cfg["gaussian_patch_sigma"]))

    def _mind_descriptor(self, r, x, out, cfg):
        self._mind_check(r, x)
        N, Cc, *ext = x.shape
        shape = (N, r["channels"], *ext)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=x.device)
        self._mind_check(r, out)
        if tuple(out.shape) != shape:
            raise ValueError(f"{r['name']}_descriptor: out must be {shape}, got {tuple(out.shape)}")
        entry = f"gs_{r['name']}_descriptor"
        L.check(getattr(self.lib, entry)(_ptr(x), N, Cc, *ext, *self._mind_args(r, cfg), _ptr(out), _stream()), entry)
        return out

    def _mind_scratch(self, r, x, backward):
        nbytes = getattr(self.lib, f"gs_{r['name']}_scratch_bytes")(x.shape[0], *x.shape[2:], backward)
        return torch.empty(nbytes, dtype=torch.uint8, device=x.device)

    def _mind_l1(self, r, x, y, out, cfg):
        self._mind_check(r, x, y)
        if out.dtype != torch.float32 or out.numel() != 1:
            raise ValueError(f"{r['name']}_l1: out must hold one fp32 value")
        N, Cx, *ext = x.shape
        scratch = self._mind_scratch(r, x, 0)
        entry = f"gs_{r['name']}_l1"
        L.check(getattr(self.lib, entry)(_ptr(x), _ptr(y), N, Cx, y.shape[1], *ext, *self._mind_args(r, cfg), _ptr(out),
                                         _ptr(scratch), _stream()), entry)

    def _mind_l1_backward(self, r, x, y, grad_y, grad_scale, cfg):
        self._mind_check(r, x, y)
        self._mind_check(r, grad_y)
        if grad_y.shape != y.shape:
            raise ValueError(f"{r['name']}_l1_backward: grad_y must have y's shape {tuple(y.shape)}, got {tuple(grad_y.shape)}")
        if grad_scale is not None and (grad_scale.dtype != torch.float32 or grad_scale.numel() != 1):
            raise ValueError(f"{r['name']}_l1_backward: grad_scale must hold one fp32 value")
        N, Cx, *ext = x.shape
        scratch = self._mind_scratch(r, x, 1)
        entry = f"gs_{r['name']}_l1_backward"
        L.check(getattr(self.lib, entry)(_ptr(x), _ptr(y), N, Cx, y.shape[1], *ext, *self._mind_args(r, cfg),
                                         _ptr(grad_scale), _ptr(grad_y), _ptr(scratch), _stream()), entry)

    def mind_descriptor(self, x, out=None, cfg=None):
        """[N, C, H, W] fp32 -> [N, 81, H, W] MIND features of the channel mean (gs_mind_descriptor)"""
        return self._mind_descriptor(self._MIND[2], x, out, cfg)

    def mind_l1(self, x, y, out, cfg=None):
        """out (0-d fp32) = sum |MIND(x) - MIND(y)| / (H W 81): a sum over the batch, unweighted (gs_mind_l1)"""
        self._mind_l1(self._MIND[2], x, y, out, cfg)

    def mind_l1_backward(self, x, y, grad_y, grad_scale=None, cfg=None):
        """grad_y = grad_scale * d mind_l1(x, y) / dy; grad_scale is a device scalar (gs_mind_l1_backward)"""
        self._mind_l1_backward(self._MIND[2], x, y, grad_y, grad_scale, cfg)

    def mind3d_descriptor(self, x, out=None, cfg=None):
        """[N, C, D, H, W] fp32 -> [N, 27, D, H, W] MIND features of the channel mean (gs_mind3d_descriptor)"""
        return self._mind_descriptor(self._MIND[3], x, out, cfg)

    def mind3d_l1(self, x, y, out, cfg=None):
        """out (0-d fp32) = sum |MIND(x) - MIND(y)| / (D H W 27): a sum over the batch, unweighted (gs_mind3d_l1)"""
        self._mind_l1(self._MIND[3], x, y, out, cfg)

    def mind3d_l1_backward(self, x, y, grad_y, grad_scale=None, cfg=None):
        """grad_y = grad_scale * d mind3d_l1(x, y) / dy; grad_scale is a device scalar (gs_mind3d_l1_backward)"""
        self._mind_l1_backward(self._MIND[3], x, y, grad_y, grad_scale, cfg)

    # ---- validation / test image metrics (valmetrics.hip) --------------------------------------------------
    VALMETRIC_COLUMNS = ("mae", "mse", "nmse", "psnr", "ssim", "nmi", "histogram_chi2")

    def valmetrics(self, target, pred, ssim=True, hist=True, return_counts=False):
        """Per-sample image metrics of val_test_metrics.py on the device: a [N, 7] fp64 table in VALMETRIC_COLUMNS order
        (columns not asked for hold NaN). target / pred: [N, C, H, W] (the C channels are the SSIM planes) or
        [N, C, D, H, W] (all C*D depth slices are). With return_counts, also the raw bin counts (t [N, 100], p [N, 100],
        joint [N, 100, 100] indexed [t bin, p bin]) as int64 tensors. Enqueued on the current stream; nothing syncs."""
        return self._valmetrics(target, pred, None, ssim, hist, return_counts)

    def valmetrics_masked(self, target, pred, masks, ssim=True, hist=True, return_counts=False):
        """`valmetrics` inside region masks (validator_tester.py:78-98; what the reference's masked arrays make of each
        metric is stated at gs_valmetrics_masked in ganslate_hip.h): a [N, L, 7] fp64 table, one row per sample and mask.
        masks: a list of 1..VM_MAX_LABELS tensors (bool, uint8 or any number type; non-zero = inside) of exactly the
        batch's shape. A (sample, mask) pair with no element inside holds NaN in every column. With return_counts, also
        the raw bin counts of t*m and p*m ([N, L, 100], [N, L, 100], [N, L, 100, 100]). t*m and p*m are not built: the
        kernels apply the masks on load. Enqueued on the current stream; nothing syncs."""
        return self._valmetrics(target, pred, list(masks), ssim, hist, return_counts)

    def _valmetrics(self, target, pred, masks, ssim, hist, return_counts):
        """the body of valmetrics (masks is None: rows are [N]) and valmetrics_masked (a list: rows are [N, L])"""
        if target.shape != pred.shape:
            raise ValueError(f"target {tuple(target.shape)} and prediction {tuple(pred.shape)} differ in shape")
        if target.dim() not in (4, 5):
            raise NotImplementedError(f"image metrics for {target.dim() - 1}-D samples are not implemented")
        if masks is not None:
            if not 1 <= len(masks) <= L.VM_MAX_LABELS:
                raise ValueError(f"between 1 and {L.VM_MAX_LABELS} masks per call; got {len(masks)}")
            for i, m in enumerate(masks):
                if m.shape != target.shape:
                    raise ValueError(f"mask {i} has shape {tuple(m.shape)}; the batch has {tuple(target.shape)} "
                                     "(masks are not broadcast)")
        N, H, W = target.shape[0], target.shape[-2], target.shape[-1]
        P = target[0].numel() // (H * W)
        if ssim and (H < 7 or W < 7):
            raise ValueError(f"SSIM needs planes of at least 7 x 7 (the window size); got {H} x {W}")
        if P * H * W >= 2 ** 31:
            raise ValueError("a sample must hold fewer than 2^31 elements")
        hist = hist or return_counts
        t = target.detach().contiguous().float()
        p = pred.detach().contiguous().float()
        rows = (N,) if masks is None else (N, len(masks))
        table = torch.empty(*rows, 7, dtype=torch.float64, device=t.device)
        counts = torch.empty(*rows, 2 * L.VM_BINS + L.VM_BINS ** 2, dtype=torch.int32, device=t.device) if hist else None
        flags = (L.VM_FLAGS["ssim"] if ssim else 0) | (L.VM_FLAGS["hist"] if hist else 0)
        tail = (N, P, H, W, flags, _ptr(table), _ptr(counts))
        if masks is None:
            scratch = torch.empty(self.lib.gs_valmetric_scratch_bytes(N, P, H, W), dtype=torch.uint8, device=t.device)
            L.check(self.lib.gs_valmetrics(_ptr(t), _ptr(p), *tail, _ptr(scratch), _stream()), "gs_valmetrics")
        else:
            # one byte per element: bool and uint8 masks go as they are, every other dtype through `!= 0`
            held = [(m if m.dtype in (torch.bool, torch.uint8) else m != 0).detach().to(t.device).contiguous()
                    .view(torch.uint8) for m in masks]
            nl = len(held)
            ptrs = (C.c_void_p * nl)(*[m.data_ptr() for m in held])
            scratch = torch.empty(self.lib.gs_valmetric_masked_scratch_bytes(N, nl, P, H, W), dtype=torch.uint8,
                                  device=t.device)
            L.check(self.lib.gs_valmetrics_masked(_ptr(t), _ptr(p), ptrs, nl, *tail, _ptr(scratch), _stream()),
                    "gs_valmetrics_masked")
        if not return_counts:
            return table
        B = L.VM_BINS
        c = counts.long()
        return table, (c[..., :B], c[..., B:2 * B], c[..., 2 * B:].reshape(*rows, B, B))

    # ---- sliding-window inference (slidewin.hip) -------------------------------------------------------------
    # The stitching of utils/sliding_window_inferer.py around a predictor. Tensors are dense fp32 [N, C, D, H, W] on the
    # device (an image: D == 1); `table` is an int32 [n, 4] device tensor of (batch item, z, y, x) window starts in padded
    # coordinates. Enqueued on the current stream; nothing syncs; shape errors raise ValueError before any launch.
    @staticmethod
    def _sw_dense(name, t, dim=5, dtype=torch.float32):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected a tensor; got {type(t).__name__}")
        if not (t.is_cuda and t.dtype == dtype and t.dim() == dim and t.is_contiguous()):
            raise ValueError(f"{name}: expected a contiguous {dim}-D {dtype} device tensor; got {tuple(t.shape)} {t.dtype} "
                             f"on {t.device}{'' if t.is_contiguous() else ', not contiguous'}")
        return t

    @classmethod
    def _sw_table(cls, table):
        cls._sw_dense("table", table, 2, torch.int32)
        if table.shape[0] < 1 or table.shape[1] != 4:
            raise ValueError(f"table: expected int32 [n >= 1, 4]; got {tuple(table.shape)}")
        return table

    @staticmethod
    def _sw_triple(name, v, lowest):
        v = [int(a) for a in v]
        if len(v) != 3 or min(v) < lowest:
            raise ValueError(f"{name}: expected three integers >= {lowest}; got {v}")
        return v, (C.c_int32 * 3)(*v)

    def sw_gather(self, x, table, roi, pad_before, cval, out=None):
        """gs_sw_gather: the windows of `table`'s rows, [n, C, *roi], cut from x [B, C, D, H, W] as if it were padded with
        `cval` to max(size, roi) with pad_before[k] elements in front (the padded copy is never built)."""
        self._sw_dense("x", x)
        self._sw_table(table)
        roi, c_roi = self._sw_triple("roi", roi, 1)
        pad, c_pad = self._sw_triple("pad_before", pad_before, 0)
        B, Cc, D, H, W = x.shape
        if any(p > max(s, r) - s for p, s, r in zip(pad, (D, H, W), roi)):
            raise ValueError(f"pad_before {pad} exceeds max(size, roi) - size for size {(D, H, W)}, roi {roi}")
        n = table.shape[0]
        if out is None:
            out = torch.empty((n, Cc, *roi), dtype=torch.float32, device=x.device)
        elif self._sw_dense("out", out).shape != (n, Cc, *roi):
            raise ValueError(f"out: expected {(n, Cc, *roi)}; got {tuple(out.shape)}")
        L.check(self.lib.gs_sw_gather(_ptr(x), B, Cc, D, H, W, _ptr(table), n, c_roi, c_pad, float(cval), _ptr(out),
                                      _stream()), "gs_sw_gather")
        return out

    def sw_accumulate(self, acc, pred, imap, table, table_host):
        """gs_sw_accumulate: acc[b, :, window_i] += imap * pred[i] for the rows of one chunk in table order, with the host
        loop's roundings and no atomics. acc [B, C, Dp, Hp, Wp] at the padded size, pred [n, C, *roi], imap [*roi];
        table_host = the same rows as a CPU int32 tensor (checked against acc; sizes the launch)."""
        self._sw_dense("acc", acc)
        self._sw_dense("pred", pred)
        self._sw_dense("imap", imap, 3)
        self._sw_table(table)
        n = table.shape[0]
        if not (isinstance(table_host, torch.Tensor) and not table_host.is_cuda and table_host.dtype == torch.int32
                and table_host.is_contiguous() and table_host.shape == table.shape):
            raise ValueError(f"table_host: expected a contiguous CPU int32 tensor of shape {tuple(table.shape)}")
        roi, c_roi = self._sw_triple("roi", imap.shape, 1)
        B, Cc, Dp, Hp, Wp = acc.shape
        if pred.shape != (n, Cc, *roi):
            raise ValueError(f"pred: expected {(n, Cc, *roi)} (table rows, acc channels, imap shape); got {tuple(pred.shape)}")
        if any(r > s for r, s in zip(roi, (Dp, Hp, Wp))):
            raise ValueError(f"acc {(Dp, Hp, Wp)} is smaller than the window {roi}")
        th = table_host
        lim = torch.tensor([B - 1, Dp - roi[0], Hp - roi[1], Wp - roi[2]], dtype=torch.int32)
        if bool((th < 0).any()) or bool((th > lim).any()):
            raise ValueError("table_host: a window lies outside the accumulator")
        L.check(self.lib.gs_sw_accumulate(_ptr(acc), B, Cc, Dp, Hp, Wp, _ptr(table), C.c_void_p(th.data_ptr()), n, c_roi,
                                          _ptr(imap), _ptr(pred), _stream()), "gs_sw_accumulate")

    def sw_finalize(self, acc, imap, table, size, pad_before, out=None):
        """gs_sw_finalize: [B, C, *size] = acc[.., v + pad_before] / count(v + pad_before), count = the sum of imap over all
        windows of `table` (every row of the call) that cover the voxel, in table order; acc at the padded size
        max(size, roi)."""
        self._sw_dense("acc", acc)
        self._sw_dense("imap", imap, 3)
        self._sw_table(table)
        roi, c_roi = self._sw_triple("roi", imap.shape, 1)
        size, _ = self._sw_triple("size", size, 1)
        pad, c_pad = self._sw_triple("pad_before", pad_before, 0)
        B, Cc = acc.shape[:2]
        padded = tuple(max(s, r) for s, r in zip(size, roi))
        if tuple(acc.shape[2:]) != padded:
            raise ValueError(f"acc: expected spatial size {padded} = max(size, roi); got {tuple(acc.shape[2:])}")
        if any(p > q - s for p, q, s in zip(pad, padded, size)):
            raise ValueError(f"pad_before {pad} exceeds max(size, roi) - size for size {size}, roi {roi}")
        if out is None:
            out = torch.empty((B, Cc, *size), dtype=torch.float32, device=acc.device)
        elif self._sw_dense("out", out).shape != (B, Cc, *size):
            raise ValueError(f"out: expected {(B, Cc, *size)}; got {tuple(out.shape)}")
        L.check(self.lib.gs_sw_finalize(_ptr(acc), B, Cc, *size, _ptr(table), table.shape[0], c_roi, c_pad, _ptr(imap),
                                        _ptr(out), _stream()), "gs_sw_finalize")
        return out

    # ---- logged image grids (visgrid.hip) ---------------------------------------------------------------------
    @staticmethod
    def visuals_plan(visuals, multi_modality_split=None):
        """The host side of the reference's process_visuals_for_logging (trackers/utils.py): drops the `None` entries and
        splits multi-modality tensors channel-wise as `_split_multimodal_visuals` does (`real_A` -> `real_A1`, `real_A2`
        for a split {"A": [c1, c2]}; a `_A` / `_B` name that ends with no domain of the split is left out, as there; names
        without `_A` / `_B`, the masks, pass). Returns [(name, tensor, first channel, channels)]: a split is an offset into
        the same tensor, never a copy. Needs no GPU."""
        visuals = {k: v for k, v in visuals.items() if v is not None}
        plan = []
        for name, t in visuals.items():
            if multi_modality_split is None or not ("_A" in name or "_B" in name):
                plan.append((name, t, 0, int(t.shape[1])))
                continue
            for domain in multi_modality_split:
                if not name.endswith(domain):
                    continue
                split = multi_modality_split[domain]
                if split is None:            # a split may be given for one of the two domains only
                    plan.append((name, t, 0, int(t.shape[1])))
                    continue
                split = tuple(int(c) for c in split)
                if sum(split) != t.shape[1]:
                    raise ValueError("Please specify channel-split correctly!")
                first = 0
                for i, c in enumerate(split):
                    plan.append((f"{name}{i + 1}", t, first, c))
                    first += c
        return plan

    def visuals_grid(self, visuals, *, single_example=False, mid_slice_only=False, multi_modality_split=None, out=None):
        """gs_visuals_grid_u8: the image the reference logs for an ordered {name: tensor} of visuals ([N, C, H, W] or
        [N, C, D, H, W], dense fp32 on the device, values in [-1, 1]): the visuals side by side along the width, the slices of
        a volume stacked along the height (or the middle slice, D // 2, with `mid_slice_only`), gray replicated to RGB.
        Returns ("-".join(names), uint8 device tensor [n, Hout, K * W, 3]) with n = 1 for `single_example`, else N. One
        launch on the current stream; nothing syncs; ValueError before any launch."""
        plan = self.visuals_plan(visuals, multi_modality_split)
        if not plan:
            raise ValueError("visuals_grid: no visuals")
        if len(plan) > L.VIS_MAX_SRCS:
            raise ValueError(f"visuals_grid: at most {L.VIS_MAX_SRCS} visuals (after the modality split); got {len(plan)}")
        shape = None
        for name, t, _, c in plan:
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name}: expected a tensor; got {type(t).__name__}")
            if not (t.is_cuda and t.dtype == torch.float32 and t.dim() in (4, 5) and t.is_contiguous()):
                raise ValueError(f"{name}: expected a contiguous 4-D or 5-D torch.float32 device tensor; got {tuple(t.shape)} "
                                 f"{t.dtype} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}")
            if c not in (1, 3):
                raise ValueError(f"{name}: a visual holds 1 or 3 channels; got {c}")
            if shape is None:
                shape = (t.shape[0], *t.shape[2:])
            elif (t.shape[0], *t.shape[2:]) != shape:
                raise ValueError(f"{name}: batch and spatial shape {(t.shape[0], *t.shape[2:])} differ from {shape} of "
                                 f"`{plan[0][0]}`")
        N, (D, H, W) = shape[0], (shape[1:] if len(shape) == 4 else (1, *shape[1:]))
        if min(N, D, H, W) < 1:
            raise ValueError(f"visuals_grid: empty visuals {shape}")
        K, n = len(plan), 1 if single_example else N
        slice_ = D // 2 if (mid_slice_only and len(shape) == 4) else -1
        want = (n, H * (D if slice_ < 0 else 1), K * W, 3)
        if out is None:
            out = torch.empty(want, dtype=torch.uint8, device=plan[0][1].device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
                  and tuple(out.shape) == want):
            raise ValueError(f"out: expected a contiguous torch.uint8 device tensor of shape {want}")
        src = (C.c_void_p * K)(*[t.data_ptr() for _, t, _, _ in plan])
        ctot = (C.c_int32 * K)(*[t.shape[1] for _, t, _, _ in plan])
        c0 = (C.c_int32 * K)(*[f for _, _, f, _ in plan])
        cc = (C.c_int32 * K)(*[c for _, _, _, c in plan])
        L.check(self.lib.gs_visuals_grid_u8(src, ctot, c0, cc, K, n, N, D, H, W, slice_, _ptr(out), _stream()),
                "gs_visuals_grid_u8")
        return "-".join(name for name, _, _, _ in plan), out

    # ---- optimiser -----------------------------------------------------------------------------------------
    def adam_step(self, p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, zero_grad=True):
        bc1 = 1.0 - beta1 ** step
        bc2_sqrt = (1.0 - beta2 ** step) ** 0.5
        hyper = (C.c_float * 6)(lr, beta1, beta2, eps, bc1, bc2_sqrt)
        L.check(self.lib.gs_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), hyper, float(grad_scale),
                                      int(zero_grad), _stream()), "gs_adam_step")

    def adam_step_dev(self, p, g, m, v, hyper_dev, grad_scale=1.0, zero_grad=True, packs=None):
        """hyper_dev: device float32[6] = lr, beta1, beta2, eps, 1-beta1^t, sqrt(1-beta2^t) (see NativeAdam.prepare).
        packs = (inv_f, fpack, inv_d, dpack): the update also writes the pack groups that are 8 consecutive master elements
        (NativeNet.fused_pack_targets)"""
        if packs is not None:
            inv_f, fpack, inv_d, dpack = packs
            L.check(self.lib.gs_adam_step_dev_packs(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(hyper_dev),
                                                    float(grad_scale), int(zero_grad), _ptr(inv_f), _ptr(fpack), _ptr(inv_d),
                                                    _ptr(dpack), _stream()), "gs_adam_step_dev_packs")
            return
        L.check(self.lib.gs_adam_step_dev(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(hyper_dev),
                                          float(grad_scale), int(zero_grad), _stream()), "gs_adam_step_dev")

    def adam_step_dev_ranges(self, p, g, m, v, ranges_dev, max_len, hyper_dev, grad_scale=1.0, zero_grad=True, packs=None):
        """adam_step_dev over the ranges [start, end) (device int64 [n][2]) of the flat buffers in one launch; packs index the
        whole buffers"""
        inv_f, fpack, inv_d, dpack = packs if packs is not None else (None, None, None, None)
        L.check(self.lib.gs_adam_step_dev_packs_ranges(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ranges_dev), ranges_dev.shape[0],
                                                       int(max_len), _ptr(hyper_dev), float(grad_scale), int(zero_grad),
                                                       _ptr(inv_f), _ptr(fpack), _ptr(inv_d), _ptr(dpack), _stream()),
                "gs_adam_step_dev_packs_ranges")

    def pool_query(self, pool, images, out, code_dev):
        B = images.shape[0]
        nbytes = images[0].numel() * images.element_size()
        L.check(self.lib.gs_pool_query(_ptr(pool), _ptr(images), _ptr(out), _ptr(code_dev), B, nbytes, _stream()),
                "gs_pool_query")

    def repack(self, master, index, pack):
        L.check(self.lib.gs_repack_bf16(_ptr(master), _ptr(index), _ptr(pack), pack.numel(), _stream()),
                "gs_repack_bf16")

    def repack_groups(self, master, gindex, pack, index=None):
        """pack[8 g + j] = bf16(master[gindex[g] + j]); gindex[g] = -1: zeros, -2: the group's own entries of `index`"""
        L.check(self.lib.gs_repack_bf16_groups(_ptr(master), _ptr(gindex), _ptr(index) if index is not None else None,
                                               _ptr(pack), gindex.numel(), _stream()), "gs_repack_bf16_groups")

    def repack_tiled_groups(self, master, gindex, pack, seg, tiles):
        """all transposed segments of a pack: seg int64 [nseg, 5] = (pack offset, gindex offset, rows, kp, first tile) on the
        device; pack[off + (8 G + j) * kp + k] = bf16(master[gindex[goff + G * kp + k] + j])"""
        L.check(self.lib.gs_repack_bf16_tiled_groups(_ptr(master), _ptr(gindex), _ptr(pack), _ptr(seg), seg.shape[0],
                                                     int(tiles), _stream()), "gs_repack_bf16_tiled_groups")

    def repack_tiled(self, master, index, pack, rows, kp):
        """one [rows][kp] pack segment whose master indices run along the rows (see NativeNet._get_packs)"""
        L.check(self.lib.gs_repack_bf16_tiled(_ptr(master), _ptr(index), _ptr(pack), rows, kp, _stream()),
                "gs_repack_bf16_tiled")

    def ssim_distance_backward(self, x, y, grad_y, grad_scale=None):
        NC = x.numel() // (x.shape[-1] * x.shape[-2])
        H, W = x.shape[-2], x.shape[-1]
        scratch = torch.empty(self.lib.gs_ssim_backward_scratch_floats(NC, H, W), dtype=torch.float32, device=x.device)
        L.check(self.lib.gs_ssim_distance_backward(_ptr(x), _ptr(y), NC, H, W, _ptr(grad_scale), _ptr(grad_y),
                                                   _ptr(scratch), _stream()), "gs_ssim_distance_backward")

    # ---- SelfAttentionBlock (csrc/attn.hip) ----------------------------------------------------------------------
    ATTN_KEYS = ("gamma", "wq", "bq", "wk", "bk", "wv", "bv")

    def _attn_args(self, x, tensors):
        Cc = int(x.shape[-1])
        d = L.AttnDesc(int(x.shape[0]), int(x.numel() // (x.shape[0] * Cc)), Cc)
        p = L.AttnParams()
        for k in self.ATTN_KEYS:
            t = None if tensors is None else tensors.get(k)
            if t is not None:
                assert t.dtype == torch.float32 and t.is_contiguous() and t.device == x.device, k
            setattr(p, k, t.data_ptr() if t is not None else None)
        return d, p

    def attn_forward(self, x, params, need_backward=None):
        """x: NDHWC activation [B, ..., C]; params: {gamma [1], wq [C/8, C], bq, wk, bk, wv [C, C], bv} fp32 (torch layout)
        -> (out like x, saved state for attn_backward)"""
        assert x.is_contiguous() and x.dtype == self.act_dtype
        d, p = self._attn_args(x, params)
        # (a pass that will not run backward — inference, validation — takes the forward part of the scratch only)
        need_bwd = True if need_backward is None else bool(need_backward)     # (callers inside an autograd Function say so)
        size = self.lib.gs_attn_work_bytes(C.byref(d)) if need_bwd else self.lib.gs_attn_forward_work_bytes(C.byref(d))
        work = torch.empty(int(size), dtype=torch.uint8, device=self.device)
        out = torch.empty_like(x)
        L.check(self.lib.gs_attn_forward(C.byref(d), _ptr(x), C.byref(p), _ptr(out), _ptr(work), _stream()), "gs_attn_forward")
        return out, ((x, work) if need_bwd else None)

    def attn_backward(self, saved, dout, params, grads):
        """-> dx; parameter gradients are ADDED into the tensors of `grads` (same keys as params; None: skipped)"""
        if saved is None:
            raise RuntimeError("attn_backward: this forward pass kept no state (it ran under no_grad / need_backward=False)")
        x, work = saved
        d, p = self._attn_args(x, params)
        _, g = self._attn_args(x, grads)
        dx = torch.empty_like(x)
        L.check(self.lib.gs_attn_backward(C.byref(d), _ptr(x), _ptr(dout.contiguous()), C.byref(p),
                                          C.byref(g) if grads is not None else None, _ptr(work), _ptr(dx), _stream()),
                "gs_attn_backward")
        return dx

    # ---- PatchNCE + patch MLP (csrc/patchnce.hip) ---------------------------------------------------------------
    def _nce_desc(self, channels, batch, patches, nc, nce_T, lambda_nce):
        d = L.PatchNCEDesc()
        d.levels, d.batch, d.patches, d.nc, d.nce_T, d.lambda_nce = len(channels), batch, patches, nc, nce_T, lambda_nce
        for i, c in enumerate(channels):
            d.channels[i] = c
        return d

    def patchnce_forward(self, xq, xk, params, *, batch, nc=256, nce_T=0.07, lambda_nce=1.0):
        """xq / xk: lists of [batch, patches_l, C_l] fp32 (target / source patches per level), params: flat fp32 MLP
        parameters -> (loss per level [L] fp32, saved state for patchnce_backward).
        Levels normally share one patch count and run as ONE launch group. FeaturePatchMLP draws min(num_patches,
        pixels of the level) ids per level (cut.py:262-268), so on small inputs deep levels carry fewer patches: then every
        level runs as its own launch group with its own row count, weighted lambda / (levels * batch * patches_l) like
        the reference's per-level .mean() (cut.py:218-226)."""
        n_lv = len(xq)
        channels = [int(t.shape[-1]) for t in xq]
        for l, (q, k) in enumerate(zip(xq, xk)):
            if q.dim() != 3 or tuple(q.shape) != tuple(k.shape) or int(q.shape[0]) != batch:
                raise ValueError(f"patchnce_forward: level {l}: target {tuple(q.shape)} / source {tuple(k.shape)} patches "
                                 f"must both be [batch={batch}, patches, channels]")
        per_level = [int(t.shape[1]) for t in xq]
        if nc != 256 or max(per_level) > 256 or min(per_level) < 1 or max(channels) > 256:
            raise NotImplementedError(
                f"gs_patchnce_*: the fused PatchNCE kernels take mlp_nc == 256, 1..256 patches per image and level "
                f"and <= 256 channels per level (got mlp_nc={nc}, patches={per_level}, channels={channels}); "
                "num_patches: 0 (every pixel) and wider features have no HIP path")
        xq = [t.contiguous().float() for t in xq]
        xk = [t.contiguous().float() for t in xk]
        loss = torch.empty(n_lv, dtype=torch.float32, device=self.device)
        if len(set(per_level)) == 1:
            groups = [(list(range(n_lv)), 0, lambda_nce)]
        else:      # one group per level; its lambda carries the 1 / levels of the whole loss
            offs, off = [], 0
            for c in channels:
                offs.append(off)
                off += nc * c + nc + nc * nc + nc
            groups = [([l], offs[l], lambda_nce / n_lv) for l in range(n_lv)]
        saved = []
        for lv, poff, lam in groups:
            d = self._nce_desc([channels[l] for l in lv], batch, per_level[lv[0]], nc, nce_T, lam)
            work = torch.empty(int(self.lib.gs_patchnce_work_bytes(C.byref(d))), dtype=torch.uint8, device=self.device)
            gq, gk = [xq[l] for l in lv], [xk[l] for l in lv]
            pq = (C.c_void_p * len(lv))(*[t.data_ptr() for t in gq])
            pk = (C.c_void_p * len(lv))(*[t.data_ptr() for t in gk])
            L.check(self.lib.gs_patchnce_forward(C.byref(d), pq, pk, _ptr(params[poff:]), _ptr(work),
                                                 _ptr(loss[lv[0]:]), _stream()), "gs_patchnce_forward")
            saved.append((d, gq, work, poff))
        return loss, saved

    def patchnce_backward(self, saved, params, grads, grad_scale=None):
        """-> list of d(sum of level losses)/d xq[l] * grad_scale; parameter gradients are added into `grads`"""
        out = []
        for d, xq, work, poff in saved:
            dxq = [torch.empty_like(t) for t in xq]
            pq = (C.c_void_p * len(xq))(*[t.data_ptr() for t in xq])
            pd = (C.c_void_p * len(xq))(*[t.data_ptr() for t in dxq])
            L.check(self.lib.gs_patchnce_backward(C.byref(d), pq, pd, _ptr(params[poff:]), _ptr(grads[poff:]),
                                                  _ptr(work), _ptr(grad_scale), _stream()), "gs_patchnce_backward")
            out += dxq
        return out
