"""The device input pipeline outside training, host side: `val|test|infer.dataset.device_transforms` on the two image-folder
datasets (loaders hand over RawImage lists, the pipeline on the oracle backend equals the host transform bit for bit), the
Validator / Tester / Inferer fed through it against the same engines on the host transform path, per-entry geometry with
`multi_dataset`, the volume dataset's guard, and the descriptor table of the batched kernels (GsU8BatchItem): which input
rows the horizontal pass computes, and the library's host-side validation of a table. Every comparison is exact."""
import csv
import ctypes
import random
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from ganslate_amd.data.device_transforms import DeviceImagePipeline, RawImage, batch_item, resample_tables
from ganslate_amd.nn.native import backend
from oracle.ops_ref import RefOps
from tests import imgbatch_ref as R

ROOT = Path(__file__).resolve().parent.parent
CONF = ROOT / "tests" / "configs" / "imagefolder_engines.yaml"
SIZES = [(40, 52), (37, 53), (64, 40), (33, 90), (48, 48)]          # five PNGs, five sizes (h, w)


@pytest.fixture()
def fp32_oracle_backend():
    backend.set_ops(RefOps(act_dtype=torch.float32))
    yield
    backend.set_ops(None)


def _folder(root, sizes=SIZES):
    for dom in "AB":
        (root / dom).mkdir(parents=True)
        for k, (h, w) in enumerate(sizes):
            Image.fromarray(R.image(h, w, 3, ord(dom) + k), "RGB").save(root / dom / f"{k}.png")
    return root


def _args(root, out, *extra):
    return [f"config={CONF}", "train.cuda=false", "train.seed=7", f"train.output_dir={out}", f"val.output_dir={out}",
            f"test.output_dir={out}", f"infer.output_dir={out}"] + \
        [f"{m}.dataset.root={root}" for m in ("train", "val", "test", "infer")] + list(extra)


@pytest.mark.parametrize("mode", ["val", "test", "infer"])
@pytest.mark.parametrize("target", ["UnpairedImageDataset", "PairedImageDataset"])
def test_loaders_hand_over_raw_images_and_the_oracle_pipeline_equals_the_host_transform(tmp_path, mode, target):
    from ganslate_amd.utils.builders import build_conf, build_loader
    root = _folder(tmp_path / "data")
    base = _args(root, tmp_path) + [f"{mode}.dataset._target_=ganslate.data.{target}", f"{mode}.batch_size=3"]
    batches = {}
    for flag in (True, False):
        conf = build_conf(base + [f"{mode}.dataset.device_transforms={flag}"])
        conf.mode = mode
        loader = build_loader(conf)
        assert loader.dataset.transform.raw is flag
        random.seed(11)
        got = list(loader)
        assert [len(b["A"]) for b in got] == [3, 2]
        if flag:
            assert all(isinstance(r, RawImage) and r.pixels.dtype == torch.uint8 for b in got for k in "AB" for r in b[k])
            assert len({tuple(r.pixels.shape) for b in got for r in b["A"]}) >= 3
            pipe = loader.dataset.device_pipeline(conf, "cpu")
            assert isinstance(pipe, DeviceImagePipeline) and pipe.batched       # the oracle has no batched op: per image
            pipe._ops = RefOps()
            got = [pipe(b) for b in got]
        else:
            assert loader.dataset.device_pipeline(conf, "cpu") is None
        batches[flag] = got
    for a, b in zip(batches[True], batches[False]):
        for k in "AB":
            assert a[k].dtype == torch.float32 and torch.equal(a[k], b[k]), (mode, target, k)


def test_the_trainers_pipeline_is_not_the_batched_one(tmp_path):
    from ganslate_amd.utils.builders import build_conf, build_loader
    conf = build_conf(_args(_folder(tmp_path / "data"), tmp_path, "train.dataset.device_transforms=true"))
    conf.mode = "train"
    assert build_loader(conf).dataset.device_pipeline(conf, "cpu").batched is False


_RUNS = {}


def _trained(tmp_path_factory):
    """one training iteration with validation at iteration 1, with val.dataset.device_transforms on and off: the Validator's
    per-sample rows of both, and the run directory with checkpoint 1 (the same weights in both: train.seed)"""
    if not _RUNS:
        from ganslate_amd.engines import init_engine
        root = _folder(tmp_path_factory.mktemp("data"))
        for flag in (False, True):
            out = tmp_path_factory.mktemp(f"run_{flag}")
            tr = init_engine("train", _args(root, out, f"val.dataset.device_transforms={flag}"))
            tr.run()                                  # the draws of both runs follow train.seed
            _RUNS[flag] = (tr, out)
        _RUNS["root"] = root
    return _RUNS


def test_validator_logs_the_same_rows_on_both_input_paths(fp32_oracle_backend, tmp_path_factory):
    runs = _trained(tmp_path_factory)
    rows = {}
    for flag in (True, False):
        v = runs[flag][0].validator
        loader = v.data_loaders[None]
        assert (v.input_pipeline(loader) is not None) is flag and loader.dataset.transform.raw is flag
        rows[flag] = v.samples[None]
        assert v.history[-1][0] == 1
    assert len(rows[True]) == 5 and set(rows[True][0]) == {"mae", "mse", "nmse", "psnr"}       # batches of 2 + 2 + 1
    assert rows[True] == rows[False]
    assert all(np.isfinite(x) for r in rows[True] for x in r.values())
    w = [torch.load(runs[f][1] / "checkpoints" / "1.pth", map_location="cpu")["G_AB"] for f in (True, False)]
    assert all(torch.equal(w[0][k], w[1][k]) for k in w[0])


def test_tester_writes_the_same_metrics_csv_on_both_input_paths(fp32_oracle_backend, tmp_path_factory):
    from ganslate_amd.engines import init_engine
    runs = _trained(tmp_path_factory)
    out = runs[False][1]
    text = {}
    for flag in (True, False):
        te = init_engine("test", _args(runs["root"], out, f"test.dataset.device_transforms={flag}"))
        random.seed(31)
        te.run()
        assert (te.input_pipeline(te.data_loaders[None]) is not None) is flag
        text[flag] = (out / "test" / "metrics.csv").read_text()
        rows = list(csv.DictReader(text[flag].splitlines()))
        assert [int(r["sample"]) for r in rows] == [0, 1, 2, 3, 4] and all(np.isfinite(float(r["mae"])) for r in rows)
    assert text[True] == text[False]


def test_inferer_hands_the_same_tensors_to_the_datasets_save_on_both_input_paths(fp32_oracle_backend, tmp_path_factory):
    from ganslate_amd.engines import init_engine
    runs = _trained(tmp_path_factory)
    out = runs[False][1]
    saved = {}
    for flag in (True, False):
        eng = init_engine("infer", _args(runs["root"], out, f"infer.dataset.device_transforms={flag}"))
        kept = saved.setdefault(flag, [])
        eng.data_loader.dataset.save = lambda tensor, save_dir, _k=kept: _k.append(tensor.detach().float().cpu().clone())
        random.seed(41)
        eng.run()
        assert (eng.input_pipeline(eng.data_loader) is not None) is flag
    assert len(saved[True]) == len(saved[False]) == 5 and saved[True][0].shape == (3, 32, 32)
    for a, b in zip(saved[True], saved[False]):
        assert torch.equal(a, b)


def test_every_multi_dataset_entry_gets_its_own_geometry(tmp_path):
    """build_loader deep-copies the conf per entry; the engine's own conf has `dataset: None`, so the pipeline takes the
    sizes from the dataset's transform"""
    from ganslate_amd.engines.base import BaseEngineWithInference
    from ganslate_amd.utils.builders import build_conf, build_loader
    root = _folder(tmp_path / "data")
    text = CONF.read_text()
    single = re.search(r"val:\n(?:  .*\n)*?  dataset:\n(?:    .*\n)+", text).group(0)
    entry = """      _target_: ganslate.data.PairedImageDataset
      root: "%s"
      preprocess: ["resize", "random_crop"]
      load_size: %s
      final_size: [24, 24]
      num_workers: 0
      device_transforms: true
"""
    multi = single[:single.index("  dataset:")] + "  multi_dataset:\n    small:\n" + entry % (root, "[30, 34]") + \
        "    large:\n" + entry % (root, "[50, 44]")
    path = tmp_path / "multi.yaml"
    path.write_text(text.replace(single, multi))
    conf = build_conf([f"config={path}", "train.cuda=false", f"train.output_dir={tmp_path}", f"val.output_dir={tmp_path}"])
    conf.mode = "val"
    assert conf.val.dataset is None
    loaders = build_loader(conf)
    assert set(loaders) == {"small", "large"}

    class Engine(BaseEngineWithInference):
        def _set_mode(self):
            self.conf.mode = "val"

    eng = Engine(conf)
    eng.model = type("M", (), {"device": torch.device("cpu")})()
    for name, load in (("small", (30, 34)), ("large", (50, 44))):
        pipe = eng.input_pipeline(loaders[name])
        assert pipe is eng.input_pipeline(loaders[name]) and pipe.load == load and pipe.final == (24, 24)
        far = (int(0.999999 * (load[0] - 24)), int(0.999999 * (load[1] - 24)))
        assert pipe.geometry(40, 52, (0.999999, 0.999999)) == (load[0], load[1]) + far + (24, 24)
        pipe._ops = RefOps()
        random.seed(5)
        batch = next(iter(loaders[name]))
        host = loaders[name].dataset.transform
        want = [host.__class__.__call__(_host_copy(host), Image.fromarray(r.pixels.numpy(), "RGB"),
                                        {"crop": r.crop, "flip": r.flip, "zoom": r.zoom}) for r in batch["A"]]
        assert torch.equal(pipe(batch)["A"], torch.stack(want))


def _host_copy(transform):
    t = transform.__class__.__new__(transform.__class__)
    t.pre, t.load, t.final, t.raw = transform.pre, transform.load, transform.final, False
    return t


def test_a_volume_dataset_under_val_still_raises(tmp_path):
    from ganslate_amd.data.volume_datasets import UnpairedVolumeDataset
    from ganslate_amd.engines.base import BaseEngineWithInference
    ds = UnpairedVolumeDataset.__new__(UnpairedVolumeDataset)
    ds.raw = True
    engine = type("Engine", (BaseEngineWithInference,), {"_set_mode": lambda self: None})
    eng = engine.__new__(engine)
    eng.conf = type("C", (), {"mode": "val"})()
    eng._input_pipelines = {}
    loader = type("L", (), {"dataset": ds})()
    with pytest.raises(NotImplementedError, match="the device-side pipeline batches training samples only"):
        eng.input_pipeline(loader)
    ds.raw = False
    eng.model = type("M", (), {"device": torch.device("cpu")})()
    assert eng.input_pipeline(loader) is None


def test_validator_raises_for_a_volume_folder_with_the_flag_under_val(fp32_oracle_backend, tmp_path):
    """through the engine: a training conf whose `val` section is a volume folder with device_transforms on"""
    from ganslate_amd.engines import init_engine
    for dom in "AB":
        (tmp_path / "vol" / dom).mkdir(parents=True)
        np.save(tmp_path / "vol" / dom / "0.npy", np.random.default_rng(1).normal(size=(8, 16, 16)).astype(np.float32))
    text = (ROOT / "tests" / "configs" / "cyclegan3d_val_synthetic.yaml").read_text()
    single = """  dataset:
    _target_: ganslate.data.SyntheticImageDataset
    image_channels: 1
    final_size: [16, 24, 20]
    length: 2
"""
    volumes = f"""  dataset:
    _target_: ganslate.data.UnpairedVolumeDataset
    root: "{tmp_path / 'vol'}"
    patch_size: [8, 16, 16]
    num_workers: 0
    device_transforms: true
"""
    assert text.count(single) == 1
    (tmp_path / "vol.yaml").write_text(text.replace(single, volumes))
    tr = init_engine("train", [f"config={tmp_path / 'vol.yaml'}", "train.cuda=false", f"train.output_dir={tmp_path}",
                               f"val.output_dir={tmp_path}"])
    assert tr.validator.data_loaders[None].dataset.raw is True
    with pytest.raises(NotImplementedError, match="the device-side pipeline batches training samples only"):
        tr.validator.run(current_idx=0)


# ---- descriptor geometry ------------------------------------------------------------------------------------------------
GEOMETRY = [  # (H, W, load, final, crop)
    (256, 256, (286, 286), (256, 256), (0.3, 0.6)), (256, 256, (286, 286), (256, 256), (0.999999, 0.999999)),
    (256, 256, (286, 286), (256, 256), (0.0, 0.0)), (1024, 768, (286, 286), (256, 256), (0.999999, 0.999999)),
    (1024, 768, (286, 286), (256, 256), (0.5, 0.0)), (5, 5, (48, 270), (40, 261), (0.999999, 0.999999)),
    (128, 31, (48, 270), (8, 261), (0.5, 0.5)), (48, 270, (48, 270), (40, 261), (0.999999, 0.2)),
    (300, 9, (48, 270), (40, 261), (0.0, 0.999999)), (37, 53, (64, 64), (64, 64), (0.7, 0.7)),
]


@pytest.mark.parametrize("H,W,load,final,crop", GEOMETRY)
def test_descriptor_rows_are_exactly_the_rows_under_the_crop_window(H, W, load, final, crop):
    conf = type("D", (dict,), {"__getattr__": dict.__getitem__})
    pipe = DeviceImagePipeline(conf(mode="val", val=conf(dataset=conf(preprocess=["resize", "random_crop", "random_flip"],
                                                                       load_size=list(load), final_size=list(final)))),
                               "cpu")
    assert pipe.batched
    raw = RawImage(torch.zeros((H, W, 3), dtype=torch.uint8), crop, True)
    it = pipe.describe(raw)
    rh, rw, top, left, fh, fw = pipe.geometry(H, W, crop)
    assert (it.in_h, it.in_w, it.rh, it.rw, it.top, it.left, it.flip) == (H, W, rh, rw, top, left, True)
    assert (rh, rw) == load and (fh, fw) == final and top + fh <= rh and left + fw <= rw
    assert it == batch_item(H, W, rh, rw, top, left, fh, True, it.tables_h, it.tables_v)
    bounds = resample_tables(H, rh)[0]
    windows = [(it, top)]
    if crop == (0.999999, 0.999999):                                 # the largest draw below 1, and the last row itself
        assert (top, left) == (int(0.999999 * (rh - fh)), int(0.999999 * (rw - fw))) and top >= rh - fh - 1
        windows.append((batch_item(H, W, rh, rw, rh - fh, rw - fw, fh, True), rh - fh))
    for it, top in windows:
        named = set()
        for yy in range(top, top + fh):
            named |= set(range(int(bounds[yy, 0]), int(bounds[yy, 0] + bounds[yy, 1])))
        assert set(range(it.row0, it.row0 + it.rows)) == named       # exactly: the supports of neighbours overlap or touch
        assert it.row0 == bounds[top, 0] and it.row0 + it.rows == bounds[top + fh - 1, 0] + bounds[top + fh - 1, 1]
        assert 0 <= it.row0 and it.rows >= 1 and it.row0 + it.rows <= H


def _table(items, C=3, guard=0):
    from ganslate_amd.hip.ops import HipOps
    srcs = [torch.zeros((it.in_h, it.in_w, C), dtype=torch.uint8) for it in items]
    return HipOps.u8_batch_table(items, srcs, C, guard), srcs


def _item(H, W, rh, rw, top, left, fh, flip=False):
    return batch_item(H, W, rh, rw, top, left, fh, flip, R.tables(W, rw), R.tables(H, rh))


def test_descriptor_table_mirrors_the_header_and_lays_the_arena_out():
    from ganslate_amd.hip import lib as L
    header = (ROOT / "include" / "ganslate_hip.h").read_text()
    body = re.search(r"typedef struct GsU8BatchItem \{(.*?)\} GsU8BatchItem;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].lstrip("*") for n in names]
    assert names == [f[0] for f in L.U8BatchItem._fields_]
    assert ctypes.sizeof(L.U8BatchItem) == 5 * 8 + 8 + 12 * 4 and L.U8BatchItem.tmp_off.offset == 40
    items = [_item(37, 53, 48, 270, 0, 0, 40), _item(128, 31, 48, 270, 20, 4, 8, True), _item(5, 5, 48, 270, 8, 9, 40)]
    (table, nbytes), srcs = _table(items, guard=64)
    end = 64
    for d, it, s in zip(table, items, srcs):
        assert d.src == s.data_ptr() and d.bounds_v == it.tables_v[0].data_ptr() and d.kk_h == it.tables_h[1].data_ptr()
        assert (d.in_h, d.in_w, d.rh, d.rw, d.row0, d.rows, d.top, d.left, d.flip) == tuple(int(v) for v in it[:9])
        assert (d.ksize_h, d.ksize_v) == (it.tables_h[1].shape[1], it.tables_v[1].shape[1])
        assert d.tmp_off >= end and d.tmp_off % 64 == 0              # slices do not overlap, a guard between them
        end = d.tmp_off + d.rows * d.rw * 3 + 64
    assert nbytes >= end
    assert items[1].rows < 128 and items[2].rows == 5


def test_the_library_validates_a_host_table_before_any_launch():
    """gs_u8_batch_check is host code: the checks of the per-image entry points, for a table the kernels cannot report on"""
    from ganslate_amd.hip import lib as L
    if not L.library_path().is_file():
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    good = [_item(37, 53, 48, 270, 8, 9, 40), _item(64, 64, 48, 270, 0, 0, 40, True)]
    (table, nbytes), keep = _table(good)
    assert lib.gs_u8_batch_check(table, 2, 3, 40, 261, nbytes) == 0
    for C, fh, fw, n, arena, msg in ((2, 40, 261, 2, nbytes, "C must be 1 or 3"), (3, 40, 261, 0, nbytes, "1 <= n"),
                                     (3, 41, 261, 2, nbytes, r"image 0: crop window \[8\+41, 9\+261\] outside the 48 x 270"),
                                     (3, 40, 262, 2, nbytes, "image 0: crop window"),
                                     (3, 40, 261, 2, nbytes - 4096, "image 1: tmp slice")):
        assert lib.gs_u8_batch_check(table, n, C, fh, fw, arena) == 2
        assert re.search(msg, lib.gs_last_error().decode()), lib.gs_last_error().decode()
    assert lib.gs_u8_batch_check(None, 2, 3, 40, 261, nbytes) == 2
    for field, value, msg in (("top", -1, "crop window"), ("left", 10, "crop window"), ("row0", -1, "rows"),
                              ("rows", 70, "rows"), ("src", None, "bad descriptor"), ("kk_v", None, "bad descriptor"),
                              ("ksize_h", 0, "bad descriptor")):
        (table, nbytes), keep = _table(good)
        setattr(table[1], field, value)
        with pytest.raises(L.HipError, match=f"image 1: .*{msg}"):
            L.check(lib.gs_u8_batch_check(table, 2, 3, 40, 261, nbytes), "gs_u8_batch_check")
