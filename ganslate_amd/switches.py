"""Every GS_* kernel-selection and A/B switch, declared once. Two tables and a small read API; nothing else in the package
reads a GS_* variable from the environment. The accessors read os.environ at the moment of the call (tests and bench.py
change the environment mid-process); nothing is cached. A name that is not declared here raises KeyError.

This module imports nothing from the package (and no torch): tools and tests may import it on its own."""
import os

# ---- library options -------------------------------------------------------------------------------------------------
# Options of libganslate_hip.so (gs_set_option; the rows of GS_OPTIONS in csrc/common.hpp, where each one's meaning and
# default live — tests/test_abi_cpu.py holds the two sets of names equal). The library reads no environment variable:
# HipOps.sync_options maps the variable named here onto the option when the backend is created, whenever a model is built
# and after every test. None: only set programmatically (HipOps.options(...)); sync_options puts it back to its default.
LIBRARY_OPTIONS = {
    "splitk": "GS_SPLITK",
    "splitk_max_blocks": "GS_SPLITK_MAXB",
    "splitk_target": "GS_SPLITK_TARGET",
    "hconv": "GS_HCONV",
    "hconv_wide": "GS_HCONV_WIDE",
    "hwgrad": "GS_HWGRAD",
    "hwgrad_wide": "GS_HWGRAD_WIDE",
    "hwgrad_planes": "GS_HWGRAD_PLANES",          # BOTH: also a row of HOST_SWITCHES (can_merge_wgrad reads it)
    "norm_bwd_ppb": "GS_BWD_PPB",
    "norm_apply_unroll": "GS_APPLY_U",
    "gconv_tile288": "GS_GCONV_TILE288",
    "gconv_multi": "GS_GCONV_MULTI",
    "hconvw_ring": "GS_HCONVW_RING",
    "hconvt": "GS_HCONVT",
    "hstrip": "GS_HSTRIP",
    "wfold_rows": "GS_WFOLD_ROWS",
    "hwgrad_ft": "GS_HWGRAD_FT",
    "gconv_big": "GS_GCONV_BIG",
    "hconv_box8": "GS_HCONV_BOX8",
    "hconvw_persist": "GS_HCONVW_PERSIST",
    "hstrip_regs": "GS_HSTRIP_REGS",
    "gconv_twin": "GS_GCONV_TWIN",
    "wgrad_twin": "GS_WGRAD_TWIN",
    "gconv_persist": "GS_GCONV_PERSIST",
    "hconvt_persist": "GS_HCONVT_PERSIST",
    "wgrad_rows": "GS_WGRAD_ROWS",
    "splitk_multi": "GS_SPLITK_MULTI",
    "splitk_ring": "GS_SPLITK_RING",
    "gconv_ring4": "GS_GCONV_RING4",
    "hconv5": "GS_HCONV5",
    "hconv5_seg": None,
    "hwgrad2": "GS_HWGRAD2",
    "hconv2": "GS_HCONV2",
    "pwise": "GS_PWISE",
    "daxis": "GS_DAXIS",
    "elastic_rows": None,
}

# ---- host switches ---------------------------------------------------------------------------------------------------
# Variables the Python side reads itself. variable: (default, kind, meaning).
ON_OFF = "on/off"       # off if and only if the value is "0"
OPT_IN = "opt-in"       # on if and only if the value is "1"
INT = "int"
STR = "str"             # free form; the meaning lists the values
HOST_SWITCHES = {
    # hip/ops.py, read per launch / per planning query
    "GS_COUT1": ("1", ON_OFF, "dot-product kernels for the one-output-channel layer: forward, data and weight gradient "
                              "(csrc/cout1.hip)"),
    "GS_TWIN_NATIVE": ("1", ON_OFF, "a twin batch runs as ONE launch where the kernel picks the weight set per image "
                                    "(0: always two launches of N / 2)"),
    "GS_TWIN_FUSED": ("1", ON_OFF, "... also the padded-domain launches with the fused norm-backward epilogue"),
    "GS_TWIN_MULTI": ("1", ON_OFF, "... also the merged output-parity classes of a stride-2 layer (hconvt.hip)"),
    "GS_TWIN_WGRAD": ("1", ON_OFF, "... also the weight gradients"),
    "GS_FUSE_NORM": ("1", ON_OFF, "the reduction pass of the consumer's InstanceNorm backward runs in the epilogue of the "
                                  "data-gradient launch"),
    "GS_FUSE_SI2": ("1", ON_OFF, "... also for the data gradients of transposed convs (input stride 2)"),
    "GS_FUSE_MULTI": ("1", ON_OFF, "... also for the merged parity classes of a stride-2 conv's data gradient. Worth 0.3 % "
                                   "once the fused instantiation stopped spilling, DESIGN.md §4.11"),
    "GS_WGRAD_PAIR": ("1", ON_OFF, "the weight gradients of two backward passes of one layer share a launch (hwgrad.hip)"),
    "GS_HWGRAD_PLANES": ("1", ON_OFF, "BOTH: the library option hwgrad_planes (3x3x3 layers as three depth planes of the "
                                      "wide halo kernel) and the host's pairing of those layers' launches"),
    "GS_WGRAD_FRESH": ("1", ON_OFF, "a layer's first weight gradient since the optimiser cleared the buffer is passed on as "
                                    "a hint (gs_wgrad_desc.dw_fresh)"),
    "GS_WGRAD_DET": ("1", ON_OFF, "deterministic weight and bias gradients: partial sums to a per-launch workspace, "
                                  "fixed-order second stage (0: atomics)"),
    # nn/native/net.py
    "GS_ADAM_PACKS": ("1", ON_OFF, "the Adam launch refreshes the bf16 weight packs of a network with one pack set itself"),
    # nn/optim.py, read when an early update is armed
    "GS_WGRAD_ADAM": ("1", ON_OFF, "layers of few pixels: weight gradient + Adam update in one launch (gs_wgrad_adam)"),
    "GS_WGRAD_ADAM_TR": ("1", ON_OFF, "... which also writes the layer's transposed pack"),
    "GS_ADAM_RANGES": ("1", ON_OFF, "what the fused launches leave (biases, small layers) is updated by ONE multi-range "
                                    "launch behind the pass"),
    "GS_EARLY_ADAM_MIN": (None, INT, "smallest chunk (elements) worth an early Adam launch; unset: NativeAdam.EARLY_MIN"),
    # nn/gans/base.py
    "GS_FORCE_DDP": ("0", OPT_IN, "the data-parallel path with a 1-rank group (tests, bench.py)"),
    "GS_SIDE_STREAM": ("1", STR, "second launch stream for the discriminators' update: 0 none, 1 all, or a comma list of "
                                 "side-work names"),
    "GS_EARLY_ADAM": ("1", ON_OFF, "the optimiser updates the layers a single backward pass is done with while the pass "
                                   "goes on (0: after the pass)"),
    "GS_STEP_GRAPH": ("1", ON_OFF, "iterations replay a captured hipGraph (0: launch by launch)"),
    "GS_DDP_GRAPH_COLLECTIVES": (None, STR, "gradient all-reduce of a captured data-parallel step: 0 between the two "
                                            "graphs, 1 captured into the first, auto builds both and checks them against "
                                            "each other; the default depends on the world size (BaseGAN._capture_step)"),
    # recipes and generators, read at model build
    "GS_CUT_BATCH": ("1", ON_OFF, "CUT: same-network passes over independent batches run as one pass (0: one pass each, as "
                                  "the reference)"),
    "GS_TWIN": ("1", STR, "CycleGAN: the two generators / discriminators run lock-step as one twin batch: 0 never, 2d not for "
                          "volumes, 1 where the executor's twin_default allows, all everywhere"),
    "GS_WFOLD": ("1", ON_OFF, "the W taps of the k7 boundary convs are folded into the channel axis (csrc/wfold.hip; 0: the "
                              "plain lowering)"),
}


def raw(name, default=None):
    """the variable as it stands in the environment now; unset: `default` where the caller supplies one, else the table's"""
    row = HOST_SWITCHES[name]
    return os.environ.get(name, row[0] if default is None else default)


def on(name):
    v = raw(name)
    return v == "1" if HOST_SWITCHES[name][1] == OPT_IN else v != "0"


def value(name, default=None):
    """on/off and opt-in switches as bool (their default is the table's alone), integers as int, free-form ones as they are"""
    kind = HOST_SWITCHES[name][1]
    if kind in (ON_OFF, OPT_IN):
        return on(name)
    v = raw(name, default)
    return int(v) if kind == INT else v


def library_value(option):
    """the integer the environment asks of a library option now; None: no variable drives it, or the variable is unset"""
    env = LIBRARY_OPTIONS[option]
    return int(os.environ[env]) if env is not None and env in os.environ else None
