"""The batched device image transform on the GPU (csrc/imgproc.hip gs_u8_batch_*): one launch per pass for a batch of decoded
images of different sizes, against the per-image kernels on the same tables and against Pillow's resize (oracle/pil_ref.py)
+ crop + flip + the fp32 normalise, on a NaN-filled output with guard bytes round every tmp slice and round the output;
the row restriction of the horizontal pass; DeviceImagePipeline outside training against the host transform of the
datasets; and the Validator / Tester / Inferer fed through it against the same engines on the host path. Every comparison
is exact: integer resampling, and the same fp32 operations in the same order."""
import random
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from ganslate_amd.data.device_transforms import DeviceImagePipeline, RawImage, batch_item
from ganslate_amd.hip import lib as L
from ganslate_amd.hip.ops import HipOps
from tests import imgbatch_ref as R

pytestmark = pytest.mark.gpu

CONF = Path(__file__).resolve().parent / "configs" / "imagefolder_engines.yaml"
RH, RW, FH, FW = 48, 270, 40, 261            # RW > 256: two column blocks with a ragged tail; FW > 256 likewise
SIX = [(37, 53), (64, 64), (19, 80), (128, 31), (300, 9), (5, 5)]        # 300 -> 48: ksize 27; 5 -> 48 / 270: upscaled
WINDOWS = [(0, 0, False), (RH - FH, RW - FW, True), (4, 5, True), (0, RW - FW, False), (RH - FH, 0, True), (3, 7, False)]
# the six, and behind them two images that keep one axis (identity tables: 48 rows, 270 columns)
BATCHES = {"six": (SIX, WINDOWS), "six_and_identity": (SIX + [(48, 100), (20, 270)], WINDOWS + [(8, 9, True), (2, 0, False)])}
GUARD, FILL = 64, 0xA5


class D(dict):
    __getattr__ = dict.__getitem__


def _items(images, windows, rh, rw, fh, device):
    items, keep = [], []
    for a, (top, left, flip) in zip(images, windows):
        h, w = a.shape[:2]
        th = tuple(t.to(device) for t in R.tables(w, rw))
        tv = tuple(t.to(device) for t in R.tables(h, rh))
        items.append(batch_item(h, w, rh, rw, top, left, fh, flip, th, tv))
        keep.append(torch.from_numpy(a).to(device))
    return items, keep


def _run_guarded(ops, items, srcs, c, fh, fw):
    """the batched op on a NaN-filled output inside a guarded buffer and an arena it owns: (out, table, tmp, guards intact)"""
    dev = srcs[0].device
    n = len(items)
    _, nbytes = HipOps.u8_batch_table(items, srcs, c, GUARD)
    tmp = torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)
    big = torch.full((GUARD + n * c * fh * fw + GUARD,), 12345.0, dtype=torch.float32, device=dev)
    out = big[GUARD:GUARD + n * c * fh * fw].view(n, c, fh, fw)
    out.fill_(float("nan"))
    table, _ = ops.u8_batch_resample(items, srcs, out, c, tmp=tmp, guard=GUARD)
    untouched = torch.ones(nbytes, dtype=torch.bool)
    for d, it in zip(table, items):
        assert d.tmp_off >= GUARD
        untouched[d.tmp_off:d.tmp_off + it.rows * it.rw * c] = False
    assert int(untouched.sum()) >= (n + 1) * GUARD
    tmp_ok = bool((tmp.cpu()[untouched] == FILL).all())
    big = big.cpu()
    out_ok = bool((big[:GUARD] == 12345.0).all() and (big[-GUARD:] == 12345.0).all())
    return out.cpu(), table, tmp.cpu(), tmp_ok and out_ok


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_batched_kernels_equal_the_per_image_kernels_and_pillow(hip_ops, batch, c):
    sizes, windows = BATCHES[batch]
    dev = hip_ops.device
    images = [R.image(h, w, c, 3 + k) for k, (h, w) in enumerate(sizes)]
    items, srcs = _items(images, windows, RH, RW, FH, dev)
    assert max(it.tables_v[1].shape[1] for it in items) > 20 and {w[:2] for w in windows} >= {(0, 0), (RH - FH, RW - FW)}
    got, table, tmp, guards_intact = _run_guarded(hip_ops, items, srcs, c, FH, FW)
    assert not torch.isnan(got).any(), "every output element is written"
    assert guards_intact, "bytes outside the tmp slices or round the output changed"
    assert torch.equal(got, R.per_image_batch(hip_ops, images, RH, RW, windows, FH, FW, dev).cpu()), "per-image kernels"
    assert torch.equal(got, R.pillow_batch(images, RH, RW, windows, FH, FW)), "Pillow resize + crop + flip + normalise"
    # the tmp slice of every image: the rows [row0, row0 + rows) of Pillow's horizontal pass
    for d, it, a in zip(table, items, images):
        want = a if a.shape[1] == RW else R.pil_ref.resample_pass(a, RW, 1)
        part = tmp[d.tmp_off:d.tmp_off + it.rows * RW * c].view(it.rows, RW, c)
        assert np.array_equal(part.numpy(), want[it.row0:it.row0 + it.rows])


def test_the_horizontal_pass_computes_only_the_rows_under_the_crop_window(hip_ops):
    """8 crop rows of a 48-row resize of a 128-row image: the slice holds far fewer than 128 rows"""
    dev = hip_ops.device
    images = [R.image(128, 31, 3, 9), R.image(128, 200, 3, 10)]
    windows = [(20, 4, True), (RH - 8, 0, False)]
    items, srcs = _items(images, windows, RH, RW, 8, dev)
    assert all(8 * 128 // 48 <= it.rows <= 8 * 128 // 48 + 2 * 8 + 2 < 128 for it in items), [it.rows for it in items]
    assert items[1].row0 + items[1].rows == 128 and items[0].row0 > 0
    got, table, tmp, guards_intact = _run_guarded(hip_ops, items, srcs, 3, 8, FW)
    assert table[1].tmp_off - table[0].tmp_off < 128 * RW * 3
    assert guards_intact and not torch.isnan(got).any()
    assert torch.equal(got, R.per_image_batch(hip_ops, images, RH, RW, windows, 8, FW, dev).cpu())
    assert torch.equal(got, R.pillow_batch(images, RH, RW, windows, 8, FW))


def test_a_batch_of_one(hip_ops):
    dev = hip_ops.device
    images, windows = [R.image(37, 53, 3, 1)], [(5, 6, True)]
    items, srcs = _items(images, windows, RH, RW, FH, dev)
    got, _, _, guards_intact = _run_guarded(hip_ops, items, srcs, 3, FH, FW)
    assert guards_intact and torch.equal(got, R.pillow_batch(images, RH, RW, windows, FH, FW))
    out = torch.full((1, 3, FH, FW), float("nan"), device=dev)
    hip_ops.u8_batch_resample(items, srcs, out, 3)                      # the arena sized by the op itself
    assert torch.equal(out.cpu(), got)


def _host_and_raw(conf, sizes, c, seed):
    from ganslate_amd.data.image_datasets import _Transform
    host = _Transform(conf)
    random.seed(seed)
    raws, want = [], []
    for k, (h, w) in enumerate(sizes):
        a = R.image(h, w, c, 10 + k)
        prm = host.params()
        want.append(host(Image.fromarray(a if c == 3 else a[..., 0], "RGB" if c == 3 else "L"), prm))
        raws.append(RawImage(torch.from_numpy(a if c == 3 else a[..., 0].copy()), prm["crop"], prm["flip"], prm["zoom"]))
    return raws, torch.stack(want)


def test_images_with_chains_of_different_lengths_share_a_batch(hip_ops):
    """scale_width + random_zoom: an image whose width already is load_w skips the first resize; the others run it through
    the per-image kernels and join the batch for their last one"""
    conf = D(mode="val", val=D(dataset=D(preprocess=["scale_width", "random_zoom", "random_crop"], load_size=[72, 80],
                                         final_size=[64, 64])))
    pipe = DeviceImagePipeline(conf, hip_ops.device, ops=hip_ops)
    sizes = [(90, 100), (75, 80), (64, 64), (200, 81), (81, 80)]
    raws, want = _host_and_raw(conf, sizes, 3, 4)
    chains = [len(pipe.sizes(h, w, r.zoom)) for (h, w), r in zip(sizes, raws)]
    assert chains == [2, 1, 2, 2, 1]
    calls = []
    batch_op = hip_ops.u8_batch_resample
    pipe._ops = type("Counting", (), {"__getattr__": lambda self, k: getattr(hip_ops, k),
                                      "u8_batch_resample": lambda self, *a, **kw: (calls.append(len(a[0])), batch_op(*a, **kw))[1]})()
    got = pipe({"A": raws, "metadata": [{"id": k} for k in range(5)]})
    assert calls == [5] and got["metadata"] == [{"id": k} for k in range(5)]
    assert torch.equal(got["A"].cpu(), want)
    per_image = DeviceImagePipeline(conf, hip_ops.device, ops=hip_ops, batched=False)({"A": raws})["A"]
    assert torch.equal(got["A"], per_image)


@pytest.mark.parametrize("pre", [("resize",), ("resize", "random_crop", "random_flip"),
                                 ("scale_width", "random_zoom", "random_crop")])
@pytest.mark.parametrize("target", ["UnpairedImageDataset", "PairedImageDataset"])
def test_pipeline_in_val_mode_equals_the_host_transform_bit_for_bit(hip_ops, tmp_path, target, pre):
    """through the loaders of both datasets: the same files and draws with val.dataset.device_transforms on (decoded bytes ->
    DeviceImagePipeline on the GPU) and off (the PIL + torch transform in the workers)"""
    from ganslate_amd.utils.builders import build_conf, build_loader
    root = tmp_path / "data"
    for dom in "AB":
        (root / dom).mkdir(parents=True)
        for k, (h, w) in enumerate([(40, 52), (37, 53), (64, 40), (33, 90)]):
            Image.fromarray(R.image(h, w, 3, ord(dom) + k), "RGB").save(root / dom / f"{k}.png")
    base = [f"config={CONF}", f"val.dataset.root={root}", f"val.dataset._target_=ganslate.data.{target}",
            "val.batch_size=4", f"val.dataset.preprocess=[{','.join(pre)}]"]
    batches = {}
    for flag in (True, False):
        conf = build_conf(base + [f"val.dataset.device_transforms={flag}"])
        conf.mode = "val"
        loader = build_loader(conf)
        assert list(loader.dataset.transform.pre) == list(pre)
        random.seed(17)
        batch = next(iter(loader))
        if flag:
            pipe = loader.dataset.device_pipeline(conf, hip_ops.device)
            assert pipe.batched and pipe.ops is not None and hasattr(pipe.ops, "u8_batch_resample")
            batch = {k: v.cpu() for k, v in pipe(batch).items()}
        batches[flag] = batch
    shape = (4, 3, 32, 32) if "random_crop" in pre else (4, 3, 36, 40)
    for k in "AB":
        assert batches[True][k].shape == shape and torch.equal(batches[True][k], batches[False][k]), k


_RUN = {}


def _trained(tmp_path_factory):
    """one training iteration (and the validation after it) of the project YAML with device_transforms on under train AND
    val; leaves checkpoint 1 and the Validator's rows on both input paths"""
    if not _RUN:
        from ganslate_amd.engines import init_engine
        from ganslate_amd.engines.validator import Validator
        from ganslate_amd.utils.builders import build_conf
        root, out = tmp_path_factory.mktemp("data"), tmp_path_factory.mktemp("run")
        for dom in "AB":
            (root / dom).mkdir()
            for k, (h, w) in enumerate([(40, 52), (37, 53), (64, 40), (33, 90), (48, 48)]):
                Image.fromarray(R.image(h, w, 3, ord(dom) + k), "RGB").save(root / dom / f"{k}.png")
        args = [f"config={CONF}", "train.seed=7"] + [f"{m}.output_dir={out}" for m in ("train", "val", "test", "infer")] + \
            [f"{m}.dataset.root={root}" for m in ("train", "val", "test", "infer")]
        tr = init_engine("train", args + ["train.dataset.device_transforms=true", "val.dataset.device_transforms=true"])
        tr.run()
        assert tr.input_pipeline is not None and [h[0] for h in tr.validator.history] == [1]
        # the same model scored once more by this validator and by one on the host transform path, with the same draws
        conf = build_conf(args + ["val.dataset.device_transforms=false"])
        conf.mode = "train"
        rows = {}
        for flag, v in ((True, tr.validator), (False, Validator(conf, tr.model))):
            assert (v.input_pipeline(v.data_loaders[None]) is not None) is flag
            random.seed(23)
            v.run(current_idx=1)
            rows[flag] = v.samples[None]
        assert (out / "checkpoints" / "1.pth").is_file()
        _RUN.update(args=args, out=out, val_rows=rows)
    return _RUN


def test_validator_scores_the_same_rows_on_both_input_paths(hip_ops, tmp_path_factory):
    rows = _trained(tmp_path_factory)["val_rows"]
    assert len(rows[True]) == 5 and {"mae", "mse", "nmse", "psnr", "ssim"} <= set(rows[True][0])
    assert rows[True] == rows[False]


def test_tester_writes_the_same_metrics_csv_on_both_input_paths(hip_ops, tmp_path_factory):
    from ganslate_amd.engines import init_engine
    run = _trained(tmp_path_factory)
    text, rows = {}, {}
    for flag in (True, False):
        te = init_engine("test", run["args"] + [f"test.dataset.device_transforms={flag}"])
        random.seed(31)
        te.run()
        assert (te.input_pipeline(te.data_loaders[None]) is not None) is flag
        text[flag], rows[flag] = (run["out"] / "test" / "metrics.csv").read_text(), te.samples[None]
    assert len(rows[True]) == 5 and rows[True] == rows[False]             # exact float equality
    assert text[True] == text[False] and text[True].count("\n") == 6


def test_inferer_saves_the_same_tensors_on_both_input_paths(hip_ops, tmp_path_factory):
    from ganslate_amd.engines import init_engine
    run = _trained(tmp_path_factory)
    saved = {}
    for flag in (True, False):
        eng = init_engine("infer", run["args"] + [f"infer.dataset.device_transforms={flag}"])
        kept = saved.setdefault(flag, [])
        eng.data_loader.dataset.save = lambda tensor, save_dir, _k=kept: _k.append(tensor.detach().float().cpu().clone())
        random.seed(41)
        eng.run()
        assert (eng.input_pipeline(eng.data_loader) is not None) is flag
    assert len(saved[True]) == len(saved[False]) == 5 and saved[True][0].shape == (3, 32, 32)
    for a, b in zip(saved[True], saved[False]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    names = sorted(p.name for p in (run["out"] / "infer" / "images").iterdir())
    assert names == sorted(f"{i}_input-output.png" for i in range(1, 6))


def test_bad_arguments_come_back_as_the_librarys_error(hip_ops):
    dev = hip_ops.device
    images, windows = [R.image(37, 53, 3, 1), R.image(64, 64, 3, 2)], [(0, 0, False), (8, 9, True)]
    items, srcs = _items(images, windows, RH, RW, FH, dev)
    out = torch.zeros((2, 3, FH, FW), device=dev)
    two = [s[..., :2].contiguous() for s in srcs]
    with pytest.raises(L.HipError, match=r"gs_u8_batch_check: bad argument \(1 <= n <= 65535, C must be 1 or 3\)"):
        hip_ops.u8_batch_resample(items, two, torch.zeros((2, 2, FH, FW), device=dev), 2)
    table, nbytes = HipOps.u8_batch_table(items, srcs, 3)
    dev_table = torch.frombuffer(table, dtype=torch.uint8).to(dev)
    tmp = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    lib = hip_ops.lib
    for n, c in ((2, 2), (0, 3), (2, 4)):
        with pytest.raises(L.HipError, match="gs_u8_batch_resample_h: bad argument"):
            L.check(lib.gs_u8_batch_resample_h(dev_table.data_ptr(), n, c, tmp.data_ptr(), RW, 64, None), "h")
        with pytest.raises(L.HipError, match="gs_u8_batch_resample_v_crop_normalize: bad argument"):
            L.check(lib.gs_u8_batch_resample_v_crop_normalize(dev_table.data_ptr(), n, c, tmp.data_ptr(), FH, FW,
                                                              out.data_ptr(), None), "v")
    with pytest.raises(L.HipError, match="gs_u8_batch_resample_h: bad argument"):
        L.check(lib.gs_u8_batch_resample_h(None, 2, 3, tmp.data_ptr(), RW, 64, None), "h")
    with pytest.raises(L.HipError, match="gs_u8_batch_resample_v_crop_normalize: bad argument"):
        L.check(lib.gs_u8_batch_resample_v_crop_normalize(dev_table.data_ptr(), 2, 3, tmp.data_ptr(), FH, FW, None, None), "v")
    # a crop window outside the resized image: found on the host, before the table is uploaded
    bad = [items[0], items[1]._replace(top=RH - FH + 1)]
    with pytest.raises(L.HipError, match=r"image 1: crop window \[9\+40, 9\+261\] outside the 48 x 270 resized image"):
        hip_ops.u8_batch_resample(bad, srcs, out, 3)
    with pytest.raises(L.HipError, match="image 0: crop window"):
        hip_ops.u8_batch_resample(items, srcs, torch.zeros((2, 3, FH, RW + 1), device=dev), 3)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                                 # nothing was launched
