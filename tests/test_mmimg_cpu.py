"""The multi-modal 2-D image datasets on the host (data/multimodal_images.py) and everything of their device path that is
host code: the float64 oracle (tests/mmimg_ref.py) against torch's float64 bicubic interpolation, the Philox known answers,
the tap-table builder, the host samples against the oracle, identity `load_size`, the config errors, the index rules,
sample ids, dummy channels, `denormalize` / `save`, the descriptors DeviceMultiModalImagePipeline builds (run through a
float64 restatement of the kernel), `gs_img_stack_check`, and the YAML surface of the two new configs.

Bounds. E = sum |w_y w_x x| is the envelope of the 16-tap sum (mmimg_ref.resize), s = 2 / (hi - lo) for a rescaled
modality and 1 otherwise, eps32 = 2^-23.
- oracle against torch float64: 1e-10 * E.
- host samples against the oracle: K_t * eps32 * E * s + 2e-6. The host path is torch's own fp32 interpolation, which
  computes the source coordinate and from it the weights in fp32: its error depends on the size pair (1.8 for
  80 x 120 -> 64 x 96, over a hundred times that for 40 x 50 -> 64 x 96) and, relative to E, on the data (the weight errors of
  the taps sum to zero, so the error follows the differences of the pixels while E follows their size). K_t is therefore
  MEASURED here — torch fp32 against the oracle on 64 independent random images of exactly the size pairs the test uses
  (`measure_kt`), many more planes than a sample has — and the samples are asserted at twice that maximum. Measured per load
  size over SIZES: 27.1 (3 x 3), 54.1 (8 x 9), 19.8 (4 x 5), 54.2 (5 x 7), 207.3 (2 x 257); over all 25 pairs in one
  sequence of draws 210.1; on the engine folder's pairs (`ENGINE_SIZES` and 30 x 44 -> 64 x 96): 548.5. 2e-6 is the
  tolerance tests/test_mmvol_cpu.py gives the same clamp / min-max chain (a last-ulp difference of one division).
- identity `load_size`: bit for bit."""
import ctypes
import random
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mmimg_ref as R
from tests.test_mmvol_cpu import _D

ROOT = Path(__file__).resolve().parent.parent
CLIP = {"rgb": (0.0, 255.0), "normal": (-1.0, 1.0), "depth": (0.0, 8.0)}
RESCALE = {"rgb": True, "normal": False, "depth": True}
# stored (H, W) per sample, and the (H, W) a folder is loaded at: every pair of the two lists is checked. 1 x 1 -> 3 x 3 has
# every tap clamped, 13 x 17 -> 4 x 5 scales down, 5 x 7 -> 5 x 7 is the identity, 257 crosses a 256-wide block
SIZES = [(1, 1), (2, 3), (13, 17), (5, 7), (3, 20)]
LOADS = [(3, 3), (8, 9), (4, 5), (5, 7), (2, 257)]
ENGINE_SIZES = [(64, 96), (40, 50), (80, 120), (64, 96)]


def toy_folder(root, sizes=SIZES, seed=3, depth_sizes=None):
    """one sample per entry of `sizes`: rgb as .png (even samples) or uint8 .npy (odd), normal fp32 (H, W, 3) reaching past
    [-1, 1], depth fp32 (H, W) reaching past [0, 8] (stored at `depth_sizes` where given); names `<9 digits>-<modality>`"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    for name in ("rgb", "normal", "depth"):
        (root / name).mkdir(parents=True)
    for k, (h, w) in enumerate(sizes):
        rgb = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        if k % 2 == 0:
            Image.fromarray(rgb).save(root / "rgb" / f"{k:09d}-rgb.png")
        else:
            np.save(root / "rgb" / f"{k:09d}-rgb.npy", rgb)
        np.save(root / "normal" / f"{k:09d}-normal.npy", rng.uniform(-1.2, 1.2, size=(h, w, 3)).astype(np.float32))
        dh, dw = depth_sizes[k] if depth_sizes else (h, w)
        np.save(root / "depth" / f"{k:09d}-depth.npy", rng.uniform(-0.5, 9.0, size=(dh, dw)).astype(np.float32))
    return root


def dataset_conf(root, mode="train", load=(8, 9), **kw):
    """`load` is (H, W); the config field is (W, H)"""
    ds = _D(root=str(root), modalities=_D(A=["rgb", "normal"], B=["rgb", "depth"] if mode == "train" else ["depth"]),
            clip_range=_D({k: list(v) for k, v in CLIP.items()}), rescale=_D(normal=False), load_size=[load[1], load[0]],
            device_transforms=False)
    if mode == "train":
        ds.update(paired=True, noise_std=_D())
    else:
        ds.update(dummy_channels_B=[0, 0], denormalize_modality=None)
    ds.update(kw)
    return _D({"mode": mode, mode: _D(dataset=ds)})


def stored(root, name, k):
    from ganslate_amd.data.multimodal_images import read_image
    return read_image(sorted((Path(root) / name).iterdir())[k])


def expected(root, name, k, load, noise_std=0.0, z=None):
    """(value, tolerance per unit K) of one modality of one sample from the oracle: float64 [C, H, W] each"""
    x = R.to_chw(stored(root, name, k))
    r, E = R.resize(x, *load)
    lo, hi = CLIP[name]
    return R.chain(r, lo, hi, RESCALE[name], noise_std, z), R.EPS32 * E * R.scale(lo, hi, RESCALE[name])


def measure_kt(pairs, seed=11, planes=64):
    """max over the (stored size, load size) pairs of |torch fp32 - oracle| / (eps32 E) on `planes` random 0..255 images"""
    rng = np.random.default_rng(seed)
    worst = 0.0
    for (h, w), (H, W) in pairs:
        x = rng.uniform(0.0, 255.0, size=(planes, h, w)).astype(np.float32)
        got = F.interpolate(torch.from_numpy(x)[None], size=(H, W), mode="bicubic", align_corners=False)[0].numpy()
        r, E = R.resize(x.astype(np.float64), H, W)
        worst = max(worst, float(np.max(np.abs(got - r) / (R.EPS32 * E))))
    return worst


# ---- the oracle itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [((1, 1), (3, 3)), ((2, 3), (8, 9)), ((13, 17), (4, 5)), ((5, 7), (5, 7)),
                                     ((6, 300), (4, 257)), ((3, 20), (2, 257))])
def test_oracle_equals_torch_float64(src, dst):
    rng = np.random.default_rng(5)
    x = rng.uniform(-100.0, 255.0, size=(2, *src))
    want = F.interpolate(torch.from_numpy(x)[None], size=dst, mode="bicubic", align_corners=False)[0].numpy()
    r, E = R.resize(x, *dst)
    assert r.shape == want.shape == (2, *dst)
    assert np.all(np.abs(r - want) <= 1e-10 * E)
    if src == dst:
        assert np.array_equal(r, x)
    if src == (1, 1):                                           # every tap is the one pixel: the weights sum to 1
        assert np.allclose(r, x[:, :1, :1], rtol=1e-14)


def test_philox_known_answers():
    """the published Random123 vectors of Philox4x32-10"""
    assert R.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


NOISE_KEY = (1, 2)


def test_noise_plane_statistics():
    z = R.noise_plane(96, 128, NOISE_KEY)
    n = z.size
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.77           # sqrt(-2 ln 2^-24)
    assert abs(z.mean()) <= 5.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert not np.array_equal(z, R.noise_plane(96, 128, (2, 1)))


def test_table_builder_equals_the_oracle():
    from ganslate_amd.data.multimodal_images import bicubic_taps
    for n_in, n_out in [(1, 3), (2, 8), (3, 9), (13, 4), (17, 5), (7, 7), (20, 257), (300, 257), (40, 64)]:
        t = bicubic_taps(n_in, n_out)
        idx, w = R.taps(n_in, n_out)
        assert t.n_in == n_in and t.n_out == n_out and t.idx.dtype == np.int32 and t.w.dtype == np.float32
        assert t.idx.shape == t.w.shape == (n_out, 4)
        assert np.array_equal(t.idx, idx) and np.array_equal(t.w, w.astype(np.float32))       # one rounding, the last step
        assert t.idx.min() >= 0 and t.idx.max() <= n_in - 1
        assert np.allclose(w.sum(1), 1.0, atol=1e-15)
    same = bicubic_taps(7, 7)
    assert np.array_equal(same.w, np.tile(np.float32([0, 1, 0, 0]), (7, 1)))
    assert np.array_equal(same.idx[:, 1], np.arange(7))
    assert bicubic_taps(7, 7) is same                           # cached per (n_in, n_out)
    with pytest.raises(ValueError, match="positive"):
        bicubic_taps(0, 4)


# ---- host samples -------------------------------------------------------------------------------------------------------
def test_torch_fp32_error_is_nonzero_except_at_identity():
    """prints the K_t the module docstring records; the figure itself is torch's and the CPU's, so it is not asserted"""
    kt = measure_kt([(s, l) for s in SIZES for l in LOADS])
    print(f"K_t on SIZES x LOADS: {kt:.2f}")
    assert np.isfinite(kt) and kt > 1.0                         # torch's fp32 path is not the float64 one ...
    assert measure_kt([((5, 7), (5, 7))]) == 0.0                # ... except where the resize is a copy


@pytest.mark.parametrize("load", LOADS)
def test_host_samples_equal_the_oracle(tmp_path, load):
    from ganslate_amd.data import MultiModalImageDataset, MultiModalImageValTestDataset
    root = toy_folder(tmp_path / "data")
    kt = measure_kt([(s, load) for s in SIZES])
    print(f"load {load}: K_t = {kt:.2f}")
    train = MultiModalImageDataset(dataset_conf(root, load=load))
    val = MultiModalImageValTestDataset(dataset_conf(root, "val", load=load, dummy_channels_B=[3, 0]))
    assert len(train) == len(val) == len(SIZES) and train.collate_fn is None and train.device_pipeline(None, "cpu") is None
    assert train.channels == {"rgb": 3, "normal": 3, "depth": 1} and train.size == tuple(load)
    for k in range(len(SIZES)):
        s, v = train[k], val[k]
        assert list(s) == ["A", "B"] and list(v) == ["A", "B", "metadata"]
        assert s["A"].shape == (6, *load) and s["B"].shape == (4, *load) and s["A"].dtype == s["B"].dtype == torch.float32
        assert v["A"].shape == (6, *load) and v["B"].shape == (4, *load) and v["metadata"] == {"sample_id": f"{k:09d}"}
        assert torch.equal(v["A"], s["A"]) and torch.equal(v["B"][3:], s["B"][3:]) and not v["B"][:3].any()
        for tensor, names in ((s["A"], ("rgb", "normal")), (s["B"], ("rgb", "depth"))):
            c = 0
            for name in names:
                want, unit = expected(root, name, k, load)
                got = tensor[c:c + want.shape[0]].numpy().astype(np.float64)
                assert np.all(np.abs(got - want) <= 2.0 * kt * unit + 2e-6), (k, name, np.max(np.abs(got - want) / (unit + 1e-30)))
                c += want.shape[0]
        assert float(s["A"][:3].min()) >= -1.0 and float(s["A"][:3].max()) <= 1.0
        assert float(s["A"][3:].min()) >= -1.0 and float(s["A"][3:].max()) <= 1.0          # the normal map: clamped only
    hit = train[1]["A"][3:].abs().max()
    assert float(hit) == 1.0                                   # ... and its clamp is reached by the toy data


def test_identity_load_size_is_the_bare_clip_chain_bit_for_bit(tmp_path):
    from ganslate_amd.data import MultiModalImageDataset
    from ganslate_amd.data.utils.normalization import min_max_normalize
    root = toy_folder(tmp_path / "data", sizes=[(5, 7), (5, 7), (5, 7)])
    ds = MultiModalImageDataset(dataset_conf(root, load=(5, 7)))
    for k in range(3):
        s = ds[k]
        c = 0
        for tensor, names in ((s["A"], ("rgb", "normal")), (s["B"], ("rgb", "depth"))):
            c = 0
            for name in names:
                x = torch.from_numpy(R.to_chw(stored(root, name, k)).astype(np.float32))
                want = torch.clamp(x, *CLIP[name])
                want = min_max_normalize(want, *CLIP[name]) if RESCALE[name] else want
                assert torch.equal(tensor[c:c + x.shape[0]], want), (k, name)
                c += x.shape[0]


def test_training_noise_is_one_plane_per_modality(tmp_path):
    from ganslate_amd.data import MultiModalImageDataset
    root = toy_folder(tmp_path / "data", sizes=[(13, 17)] * 2)
    quiet = MultiModalImageDataset(dataset_conf(root, load=(16, 24)))
    noisy = MultiModalImageDataset(dataset_conf(root, load=(16, 24), noise_std=_D(B=_D(rgb=0.05))))
    assert noisy.noise_std == {"A": {}, "B": {"rgb": 0.05}}
    torch.manual_seed(7)
    a, b = quiet[0], noisy[0]
    assert torch.equal(a["A"], b["A"]) and torch.equal(a["B"][3:], b["B"][3:])
    d = (b["B"][:3] - a["B"][:3]).double()
    free = (b["B"][:3].abs() < 1.0).all(0)                     # pixels no channel of which was clamped
    assert free.float().mean() > 0.5
    assert torch.allclose(d[0][free], d[1][free], atol=3e-7) and torch.allclose(d[0][free], d[2][free], atol=3e-7)
    assert 0.03 < float(d[0][free].std()) < 0.07 and float(b["B"][:3].abs().max()) <= 1.0
    torch.manual_seed(7)
    assert torch.equal(noisy[0]["B"], b["B"])
    with pytest.raises(ValueError, match="noise_std.B"):
        MultiModalImageDataset(dataset_conf(root, noise_std=_D(B=_D(normal=0.1))))


def test_config_errors(tmp_path):
    from ganslate_amd.data import MultiModalImageDataset, MultiModalImageValTestDataset
    root = toy_folder(tmp_path / "data")
    with pytest.raises(ValueError, match=r"clip_range has no entry for \['depth'\]"):
        MultiModalImageDataset(dataset_conf(root, clip_range=_D(rgb=[0, 255], normal=[-1, 1])))
    with pytest.raises(ValueError, match="min < max"):
        MultiModalImageDataset(dataset_conf(root, clip_range=_D(rgb=[0, 255], normal=[1, 1], depth=[0, 8])))
    with pytest.raises(ValueError, match="load_size"):
        MultiModalImageDataset(dataset_conf(root, load_size=[0, 4]))
    with pytest.raises(ValueError, match="denormalize_modality"):
        MultiModalImageValTestDataset(dataset_conf(root, "val", denormalize_modality="rgb"))
    with pytest.raises(ValueError, match="dummy_channels_B"):
        MultiModalImageValTestDataset(dataset_conf(root, "val", dummy_channels_B=[-1, 0]))
    with pytest.raises(ValueError, match="no modality folder .*thermal"):
        MultiModalImageDataset(dataset_conf(root, modalities=_D(A=["rgb"], B=["thermal"]), clip_range=_D(rgb=[0, 255], thermal=[0, 1])))
    (root / "depth" / "000000004-depth.npy").unlink()
    with pytest.raises(ValueError, match=r"different numbers of files.*rgb': 5.*depth': 4"):
        MultiModalImageDataset(dataset_conf(root))
    np.save(root / "depth" / "000000004-depth.npy", np.zeros((3, 20), np.float64))
    with pytest.raises(ValueError, match="uint8 or float32"):
        MultiModalImageDataset(dataset_conf(root))[4]
    (root / "depth" / "000000009-depth.exr").write_bytes(b"")
    with pytest.raises(ValueError, match="convert them to .npy once"):
        MultiModalImageDataset(dataset_conf(root))


def test_read_image_forms(tmp_path):
    """.npy as stored; Pillow files as RGB or L, whatever their mode"""
    from PIL import Image
    from ganslate_amd.data.multimodal_images import read_image
    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, size=(6, 5, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "c.png")
    Image.fromarray(rgb[:, :, 0]).save(tmp_path / "g.png")
    Image.fromarray(np.dstack([rgb, rgb[:, :, :1]]), "RGBA").save(tmp_path / "a.png")
    Image.fromarray(rgb).save(tmp_path / "c.jpg", quality=95)
    assert np.array_equal(read_image(tmp_path / "c.png"), rgb) and np.array_equal(read_image(tmp_path / "a.png"), rgb)
    grey = read_image(tmp_path / "g.png")
    assert grey.shape == (6, 5) and grey.dtype == np.uint8 and np.array_equal(grey, rgb[:, :, 0])
    jpg = read_image(tmp_path / "c.jpg")
    assert jpg.shape == (6, 5, 3) and jpg.dtype == np.uint8
    for dtype, shape in ((np.float32, (6, 5)), (np.float32, (6, 5, 3)), (np.uint8, (6, 5, 2))):
        np.save(tmp_path / "x.npy", np.zeros(shape, dtype))
        v = read_image(tmp_path / "x.npy")
        assert v.shape == shape and v.dtype == dtype
    for dtype, shape in ((np.int16, (6, 5)), (np.float32, (6,)), (np.float32, (1, 6, 5, 3))):
        np.save(tmp_path / "x.npy", np.zeros(shape, dtype))
        with pytest.raises(ValueError, match="uint8 or float32"):
            read_image(tmp_path / "x.npy")


def test_index_rules(tmp_path):
    """index_A = index % n; index_B = index_A when paired, else random.randint(0, n - 1) — never the reference's pinned 9, 1"""
    from ganslate_amd.data import MultiModalImageDataset
    from ganslate_amd.data.multimodal_images import RawImageSample, collate_raw
    root = toy_folder(tmp_path / "data")
    n = len(SIZES)
    paired = MultiModalImageDataset(dataset_conf(root, device_transforms=True))
    assert paired.collate_fn is collate_raw
    for index in (0, 3, n, 2 * n + 1):
        s = paired[index]
        assert isinstance(s["A"], RawImageSample) and (s["A"].index, s["B"].index) == (index % n, index % n)
        assert s["A"].keys == s["B"].keys == {}
    unpaired = MultiModalImageDataset(dataset_conf(root, paired=False, device_transforms=True, noise_std=_D(B=_D(rgb=0.05))))
    random.seed(9)
    want = [random.randint(0, n - 1) for _ in range(12)]
    assert len(set(want)) > 2
    random.seed(9)
    np.random.seed(4)
    got = [unpaired[index] for index in range(12)]
    assert [s["A"].index for s in got] == [i % n for i in range(12)] and [s["B"].index for s in got] == want
    np.random.seed(4)
    keys = [tuple(int(v) for v in np.random.randint(0, 1 << 32, size=2, dtype=np.uint64)) for _ in range(12)]
    assert [s["B"].keys for s in got] == [{"rgb": k} for k in keys] and all(s["A"].keys == {} for s in got)
    assert len(set(keys)) == 12 and all(0 <= w < 1 << 32 for k in keys for w in k)
    # the host path draws index_B by the same rule
    host = MultiModalImageDataset(dataset_conf(root, paired=False, load=(5, 7)))
    single = MultiModalImageDataset(dataset_conf(root, paired=True, load=(5, 7)))
    random.seed(9)
    for index in range(4):
        assert torch.equal(host[index]["B"], single[want[index]]["B"])


def test_sample_ids_dummies_denormalize_and_save(tmp_path):
    from ganslate_amd.data import MultiModalImageValTestDataset
    from ganslate_amd.data.multimodal_images import RawImageSample
    root = toy_folder(tmp_path / "data", sizes=[(5, 7)] * 3)
    ids = MultiModalImageValTestDataset.sample_id
    assert ids("000000012-rgb.jpg") == "000000012" and ids("a-b-rgb.png") == "a-b" and ids("plain.npy") == "plain"
    ds = MultiModalImageValTestDataset(dataset_conf(root, "test", load=(5, 7), dummy_channels_B=[3, 0]))
    assert ds.sample_ids == ["000000000", "000000001", "000000002"] and ds.denormalize_modality == "depth"
    s = ds[1]
    assert s["B"].shape == (4, 5, 7) and not s["B"][:3].any() and s["metadata"] == {"sample_id": "000000001"}
    both = MultiModalImageValTestDataset(dataset_conf(root, "val", load=(5, 7), dummy_channels_B=[1, 2]))[1]["B"]
    assert both.shape == (4, 5, 7) and torch.equal(both[1], s["B"][3]) and not both[0].any() and not both[2:].any()
    depth = np.clip(np.load(root / "depth" / "000000001-depth.npy"), 0.0, 8.0)
    back = ds.denormalize(s["B"][3:].clone())
    assert np.allclose(back[0].numpy(), depth, atol=8e-6)             # a few ulp of 8
    for tensor in (s["B"], s["B"][3:]):                               # the whole domain tensor, or the translated channel
        path = ds.save(tensor, tmp_path / "saved", s["metadata"])
        assert path == tmp_path / "saved" / "000000001.npy"
        saved = np.load(path)
        assert saved.shape == (5, 7) and saved.dtype == np.float32 and np.allclose(saved, depth, atol=8e-6)
    assert s["B"].min() >= -1.0                                       # save works on a copy
    for channels in (2, 3, 5):                                        # none of the three layouts: refused, not guessed
        with pytest.raises(ValueError, match=f"a tensor of {channels} channels"):
            ds.save(torch.zeros(channels, 5, 7), tmp_path / "saved", s["metadata"])
    infer = MultiModalImageValTestDataset(dataset_conf(root, "infer", load=(5, 7)))
    assert list(infer[0]) == ["A", "metadata"]
    raw = MultiModalImageValTestDataset(dataset_conf(root, "val", load=(5, 7), device_transforms=True))[2]
    assert isinstance(raw["A"], RawImageSample) and raw["A"].index == raw["B"].index == 2 and raw["metadata"] == {"sample_id": "000000002"}
    # a colour modality in B is saved as (H, W, C), as stored
    colour = MultiModalImageValTestDataset(dataset_conf(root, "val", load=(5, 7), modalities=_D(A=["rgb"], B=["depth", "normal"]),
                                                        denormalize_modality="normal", dummy_channels_B=[0, 1]))
    t = colour[0]["B"]
    saved = np.load(colour.save(t, tmp_path / "saved2", {"sample_id": "x"}))
    assert t.shape == (5, 5, 7) and saved.shape == (5, 7, 3)
    assert np.array_equal(saved, np.clip(np.load(root / "normal" / "000000000-normal.npy"), -1.0, 1.0))


# ---- the device pipeline's descriptors, run through a float64 restatement of the kernel ---------------------------------
class OracleOps:
    """img_stack on the CPU from the same host items HipOps.img_stack takes: the table builder's checks, then the oracle"""

    def __init__(self):
        self.launches = 0

    def img_stack(self, items, out):
        from ganslate_amd.hip.ops import HipOps
        table = HipOps.img_stack_table(items)
        N, C, H, W = out.shape
        seen = np.zeros((N, C), np.int64)
        for d, it in zip(table, items):
            seen[it.item, it.c0:it.c0 + it.c] += 1
            if it.src is None:
                assert not d.src
                out[it.item, it.c0:it.c0 + it.c] = 0.0
                continue
            assert (d.in_h, d.in_w, d.c, d.hwc) == (*it.src.shape[:2], it.c, 1) and d.dtype == (0 if it.src.dtype == torch.uint8 else 1)
            assert np.array_equal(it.taps_y.idx.numpy(), R.taps(it.src.shape[0], H)[0])
            assert np.array_equal(it.taps_x.w.numpy(), R.taps(it.src.shape[1], W)[1].astype(np.float32))
            r, _ = R.resize(R.to_chw(it.src.numpy()), H, W)
            z = R.noise_plane(H, W, (d.key0, d.key1)) if d.noise_std > 0 else None
            out[it.item, it.c0:it.c0 + it.c] = torch.from_numpy(R.chain(r, d.lo, d.hi, bool(d.rescale), d.noise_std, z)).float()
        assert (seen == 1).all()
        self.launches += 1
        return table


@pytest.mark.parametrize("mode", ["train", "val", "infer"])
def test_pipeline_descriptors_on_oracle_ops_equal_the_host_path(tmp_path, mode):
    from torch.utils.data import DataLoader
    from ganslate_amd.data import MultiModalImageDataset, MultiModalImageValTestDataset
    from ganslate_amd.data.device_images import DeviceMultiModalImagePipeline
    root = toy_folder(tmp_path / "data", depth_sizes=[(2, 2), (4, 3), (13, 17), (5, 7), (6, 6)])
    load = (8, 9)
    cls = MultiModalImageDataset if mode == "train" else MultiModalImageValTestDataset
    kw = dict(paired=True) if mode == "train" else dict(dummy_channels_B=[3, 1])
    host, raw = cls(dataset_conf(root, mode, load=load, **kw)), cls(dataset_conf(root, mode, load=load, device_transforms=True, **kw))
    ops = OracleOps()
    pipe = raw.device_pipeline(None, "cpu")
    assert isinstance(pipe, DeviceMultiModalImagePipeline)
    pipe._ops = ops
    kt = measure_kt([(s, load) for s in SIZES + [(2, 2), (4, 3), (6, 6)]])
    want = next(iter(DataLoader(host, batch_size=5)))
    for _ in range(2):
        got = pipe(next(iter(DataLoader(raw, batch_size=5, collate_fn=raw.collate_fn))))
        assert set(got) == set(want)
        for key in ("A", "B") if mode != "infer" else ("A",):
            assert got[key].shape == want[key].shape and got[key].dtype == torch.float32
            # 2 K_t eps32 E s with E s <= 1.5^2 * 2 on [-1, 1]-sized outputs (the weights' absolute sum is at most 1.5 per axis)
            assert torch.allclose(got[key], want[key], atol=2.0 * kt * R.EPS32 * 4.5 + 2e-6, rtol=0), key
        if mode != "train":
            assert got["metadata"] == want["metadata"]
            if mode == "val":
                assert not got["B"][:, :3].any() and not got["B"][:, 4:].any() and got["B"][:, 3].any()
    n_files = 5 * (3 if mode != "infer" else 2)
    assert pipe.uploads == n_files == len(pipe.resident)          # rgb feeds A and B from one resident copy; nothing twice
    assert ops.launches == (4 if mode != "infer" else 2)
    assert set(pipe.tables) >= {(1, 8), (1, 9), (13, 8), (17, 9)}


def test_noise_keys_reach_the_descriptors(tmp_path):
    from ganslate_amd.data import MultiModalImageDataset
    from ganslate_amd.data.multimodal_images import collate_raw
    root = toy_folder(tmp_path / "data", sizes=[(5, 7)] * 2)
    raw = MultiModalImageDataset(dataset_conf(root, load=(5, 7), device_transforms=True, noise_std=_D(B=_D(rgb=0.05))))
    quiet = MultiModalImageDataset(dataset_conf(root, load=(5, 7)))
    pipe = raw.device_pipeline(None, "cpu")
    pipe._ops = OracleOps()
    np.random.seed(1)
    sample = raw[1]
    got = pipe(collate_raw([sample]))
    z = R.noise_plane(5, 7, sample["B"].keys["rgb"])
    want = quiet[1]
    assert torch.allclose(got["A"][0], want["A"], atol=1e-6, rtol=0) and torch.allclose(got["B"][0, 3:], want["B"][3:], atol=1e-6, rtol=0)
    noisy = np.clip(want["B"][:3].numpy().astype(np.float64) + 0.05 * z, -1.0, 1.0)
    assert np.allclose(got["B"][0, :3].numpy(), noisy, atol=1e-6) and np.abs(got["B"][0, :3].numpy() - want["B"][:3].numpy()).max() > 0.01


# ---- gs_img_stack_check: host code, no GPU ----------------------------------------------------------------------------------
def _descriptors(N=2, front=1):
    """a valid table for out [N, front + 4, 6, 9]: per batch item `front` dummy channels, rgb (3 channels), depth (1)"""
    from ganslate_amd.hip import lib as L
    table = (L.ImgStackItem * (3 * N))()
    for i in range(N):
        d = table[3 * i]
        d.item, d.c0, d.c = i, 0, front
        for j, (c0, c, dtype, lo, hi) in enumerate(((front, 3, 0, 0.0, 255.0), (front + 3, 1, 1, 0.0, 8.0))):
            d = table[3 * i + 1 + j]
            d.src, d.idx_y, d.w_y, d.idx_x, d.w_x = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000     # never dereferenced by the check
            d.dtype, d.hwc, d.in_h, d.in_w, d.c, d.item, d.c0, d.rescale = dtype, 1, 5, 7, c, i, c0, 1
            d.lo, d.hi, d.noise_std, d.key0, d.key1 = lo, hi, 0.05 if j == 0 else 0.0, 7, 0xFFFFFFFF
    return table


def test_img_stack_check_refuses_every_bad_descriptor():
    from ganslate_amd.hip import lib as L
    header = (ROOT / "include" / "ganslate_hip.h").read_text()
    import re
    body = re.search(r"typedef struct GsImgStackItem \{(.*?)\} GsImgStackItem;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].lstrip("*") for n in names]
    assert names == [f[0] for f in L.ImgStackItem._fields_]
    assert ctypes.sizeof(L.ImgStackItem) == 5 * 8 + 8 * 4 + 3 * 4 + 2 * 4 + 4 and L.ImgStackItem.lo.offset == 72
    assert int(re.search(r"GS_IMG_U8 = (\d+)", header).group(1)) == L.IMG_DTYPES["uint8"]
    assert int(re.search(r"GS_IMG_F32 = (\d+)", header).group(1)) == L.IMG_DTYPES["float32"]
    if not L.library_path().is_file():
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    args = (2, 5, 6, 9)
    assert lib.gs_img_stack_check(_descriptors(), 6, *args) == 0

    def refused(mutate, match, n=6, a=args):
        table = _descriptors()
        mutate(table)
        assert lib.gs_img_stack_check(table, n, *a) == 2
        with pytest.raises(L.HipError, match=match):
            L.check(lib.gs_img_stack_check(table, n, *a), "gs_img_stack_check")

    for name in ("idx_y", "w_y", "idx_x", "w_x"):
        refused(lambda t, name=name: setattr(t[1], name, None), "descriptor 1: null tap table")
    refused(lambda t: setattr(t[2], "in_h", 0), "descriptor 2: source size 0 x 7 x 1")
    refused(lambda t: setattr(t[2], "in_w", -3), "descriptor 2: source size 5 x -3 x 1")
    refused(lambda t: setattr(t[4], "hi", 0.0), r"descriptor 4: clip range \[0, 0\] is empty")
    refused(lambda t: setattr(t[4], "lo", 300.0), "descriptor 4: clip range")
    refused(lambda t: setattr(t[1], "dtype", 2), "descriptor 1: dtype 2")
    refused(lambda t: setattr(t[1], "noise_std", -0.1), "descriptor 1: noise_std")
    refused(lambda t: setattr(t[2], "c0", 5), r"descriptor 2: channels \[5, 5\+1\) outside \[0, 5\)")
    refused(lambda t: setattr(t[1], "c0", -1), "descriptor 1: channels")
    refused(lambda t: setattr(t[0], "c", 0), "descriptor 0: channels")
    refused(lambda t: setattr(t[3], "item", 2), r"descriptor 3: batch item 2 outside \[0, 2\)")
    refused(lambda t: setattr(t[3], "item", -1), "descriptor 3: batch item -1")
    refused(lambda t: setattr(t[2], "c0", 3), "descriptor 2: channel 3 of batch item 0 is written twice")
    refused(lambda t: setattr(t[3], "item", 0), "descriptor 3: channel 0 of batch item 0 is written twice")
    refused(lambda t: None, "channel 0 of batch item 1 is written by no descriptor", n=3)
    refused(lambda t: setattr(t[0], "c0", 0), "channel 5 of batch item 0 is written by no descriptor", a=(2, 6, 6, 9))
    refused(lambda t: None, "bad argument", n=0)
    refused(lambda t: None, "bad argument", a=(2, 5, 0, 9))
    refused(lambda t: None, "bad argument", a=(2, 5, 70000, 9))
    assert lib.gs_img_stack_check(None, 6, *args) == 2
    assert lib.gs_img_stack(None, 6, None, *args, None) == 2           # the launcher refuses null arrays before any GPU call


def test_img_stack_table_refuses_tables_of_another_size():
    from ganslate_amd.data.device_images import StackItem
    from ganslate_amd.data.multimodal_images import TapTable, bicubic_taps
    from ganslate_amd.hip.ops import HipOps
    dev = lambda n_in, n_out: TapTable(torch.from_numpy(bicubic_taps(n_in, n_out).idx), torch.from_numpy(bicubic_taps(n_in, n_out).w), n_in, n_out)
    src = torch.zeros((5, 7, 3), dtype=torch.uint8)
    table = HipOps.img_stack_table([StackItem(src, dev(5, 8), dev(7, 9), 3, 0, 0, 0.0, 255.0, True, 0.05, (3, (1 << 32) - 1)),
                                    StackItem(None, None, None, 2, 0, 3)])
    assert (table[0].in_h, table[0].in_w, table[0].c, table[0].key0, table[0].key1) == (5, 7, 3, 3, 0xFFFFFFFF)
    assert table[0].src == src.data_ptr() and not table[1].src and (table[1].c0, table[1].c) == (3, 2)
    planar = HipOps.img_stack_table([StackItem(src.permute(2, 0, 1).contiguous(), dev(5, 8), dev(7, 9), 3, 0, 0, hwc=False)])
    assert (planar[0].hwc, planar[0].in_h, planar[0].in_w, planar[0].c, table[0].hwc) == (0, 5, 7, 3, 1)
    with pytest.raises(AssertionError):
        HipOps.img_stack_table([StackItem(src, dev(5, 8), dev(7, 9), 3, 0, 0, hwc=False)])  # (5, 7, 3) read as 5 planes of 7 x 3
    with pytest.raises(AssertionError):
        HipOps.img_stack_table([StackItem(src, dev(6, 8), dev(7, 9), 3, 0, 0)])            # rows of a 6-row image
    with pytest.raises(AssertionError):
        HipOps.img_stack_table([StackItem(src, dev(5, 8), dev(7, 9), 1, 0, 0)])            # channel count
    with pytest.raises(AssertionError):
        HipOps.img_stack_table([StackItem(src.to(torch.int16), dev(5, 8), dev(7, 9), 3, 0, 0)])


# ---- YAML surface -----------------------------------------------------------------------------------------------------------
def engine_folder(root):
    """four samples around the configs' 96 x 64 load size: two stored at it, one smaller, one larger; depth of sample 1 at
    a size of its own"""
    return toy_folder(root, sizes=ENGINE_SIZES, depth_sizes=[(64, 96), (30, 44), (80, 120), (64, 96)])


def test_datasets_through_the_builders(tmp_path):
    from ganslate_amd.data import MultiModalImageDataset, MultiModalImageValTestDataset
    from ganslate_amd.utils.builders import build_conf, build_loader
    root = engine_folder(tmp_path / "data")
    for yaml, paired, cb, dummies in (("cyclegan_balanced_mmimg_val.yaml", False, 4, (3, 0)), ("pix2pix_mmimg_val.yaml", True, 1, (0, 0))):
        conf = build_conf([f"config=tests/configs/{yaml}"] + [f"{m}.dataset.root={root}" for m in ("train", "val", "test")])
        conf.mode = "train"
        loader = build_loader(conf)
        ds = loader.dataset
        assert isinstance(ds, MultiModalImageDataset) and ds.paired is paired and ds.raw is False
        assert ds.size == (64, 96) and ds.rescale == {"rgb": True, "normal": False, "depth": True}
        assert ds.noise_std == {"A": {}, "B": ({"rgb": 0.05} if not paired else {})}
        batch = next(iter(loader))
        n = conf.train.batch_size
        assert batch["A"].shape == (n, 6, 64, 96) and batch["B"].shape == (n, cb, 64, 96)
        assert float(batch["A"].min()) >= -1.0 and float(batch["A"].max()) <= 1.0
        for mode in ("val", "test"):
            conf.mode = mode
            loader = build_loader(conf)
            assert isinstance(loader.dataset, MultiModalImageValTestDataset) and loader.dataset.dummy_channels_B == dummies
            batch = next(iter(loader))
            assert batch["A"].shape[1:] == (6, 64, 96) and batch["B"].shape[1:] == (cb, 64, 96)
            assert batch["metadata"]["sample_id"][0] == "000000000"
