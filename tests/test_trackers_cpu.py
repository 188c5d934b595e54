"""The host side of the output path, without a GPU: utils.io.decollate, communication.gather outside and inside a
2-process gloo group, the file names of utils.trackers.ImageWriter for every engine (fed ready-made uint8 grids), the
`infer` engine's registration and deployment mode, and the modality-split planning of HipOps.visuals_plan."""
import os
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import visgrid_ref as R

ROOT = Path(__file__).resolve().parent.parent
CONFIGS = ROOT / "tests" / "configs"


def test_decollate_splits_a_collated_batch_into_samples():
    from ganslate_amd.utils.io import decollate
    batch = {"id": ["a", "b"], "index": torch.tensor([4, 5]), "spacing": [torch.tensor([1.0, 2.0]), torch.tensor([3.0, 4.0])],
             "origin": torch.tensor([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]), "nested": {"path": ["p0", "p1"]}, "empty": []}
    out = decollate(batch)
    assert len(out) == 2
    assert out[0]["id"] == "a" and out[1]["id"] == "b"
    assert out[0]["index"] == 4 and isinstance(out[0]["index"], int)
    assert out[1]["spacing"] == [2.0, 4.0]
    assert torch.equal(out[1]["origin"], torch.tensor([3.0, 4.0, 5.0]))
    assert out[1]["nested"] == {"path": "p1"} and out[0]["empty"] == []
    assert len(decollate({"id": ["a", "b", "c"]}, batch_size=3)) == 3
    with pytest.raises(RuntimeError):
        decollate({"id": ["a", "b"]})                  # no tensor to read the batch size from
    with pytest.raises(RuntimeError):
        decollate(["a", "b"])
    with pytest.raises(TypeError):
        decollate({"x": 3}, batch_size=1)


def test_gather_returns_the_value_itself_when_not_distributed():
    from ganslate_amd.utils import communication
    value = ("name", np.zeros((1, 2, 2, 3), np.uint8))
    assert communication.gather(value) is value


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _grid(n, h, w, start):
    return (np.arange(n * h * w * 3, dtype=np.int64).reshape(n, h, w, 3) * 7 + start).astype(np.uint8)


def _gather_worker(rank, world, port, out_dir):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank), GANSLATE_DIST_BACKEND="gloo")
    import torch.distributed as dist
    from ganslate_amd.utils import communication
    from ganslate_amd.utils.trackers import ImageWriter
    communication.init_distributed()
    mine = {"rank": rank, "grid": _grid(1, 2, 2, rank)}
    got = communication.gather(mine)
    if rank == 0:
        assert isinstance(got, list) and [g["rank"] for g in got] == list(range(world))
        assert all(np.array_equal(g["grid"], _grid(1, 2, 2, r)) for r, g in enumerate(got))
    else:
        assert got is mine
    # the writer gathers byte grids: rank 0 numbers the samples of all ranks in rank order
    writer = ImageWriter(_conf("infer", out_dir))
    paths = writer.write_infer(1 + 0 * world * 2, ("input-output", _grid(2, 4, 6, 50 * rank)))
    assert len(paths) == (4 if rank == 0 else 0)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_gather_collects_every_rank_on_rank_0_in_a_gloo_group(tmp_path):
    from PIL import Image
    world = 2
    mp.spawn(_gather_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    images = tmp_path / "infer" / "images"
    assert sorted(p.name for p in images.iterdir()) == [f"{i}_input-output.png" for i in (1, 2, 3, 4)]
    for i in range(4):          # samples 1, 2 from rank 0, 3, 4 from rank 1
        got = np.asarray(Image.open(images / f"{i + 1}_input-output.png"))
        assert np.array_equal(got, _grid(2, 4, 6, 50 * (i // 2))[i % 2])


def _conf(mode, output_dir):
    from ganslate_amd.configs.omegalite import OmegaConf
    conf = OmegaConf.create({"mode": mode, mode: {"output_dir": str(output_dir), "batch_size": 2,
                                                  "logging": {"freq": 1, "multi_modality_split": None}}})
    return conf


def _names(root):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*.png"))


def test_image_writer_file_names_follow_the_reference(tmp_path):
    from PIL import Image
    from ganslate_amd.utils.trackers import ImageWriter
    grids = _grid(3, 4, 6, 0)
    # train: the first example only
    w = ImageWriter(_conf("train", tmp_path))
    assert (tmp_path / "train" / "train_config.yaml").is_file()
    w.write_train(50, ("real_A-fake_B", grids))
    assert _names(tmp_path / "train" / "images") == ["50_real_A-fake_B.png"]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "train" / "images" / "50_real_A-fake_B.png")), grids[0])
    # val: a directory per iteration, samples numbered over the batches of a dataset, per dataset with multi_dataset
    w = ImageWriter(_conf("val", tmp_path))
    w.add_samples(("real_A-fake_B-real_B", grids[:2]))
    w.add_samples(("real_A-fake_B-real_B", grids[2:]))
    w.write_samples(100)
    w.add_samples(("real_A-fake_B-real_B-BODY", grids[:1]))
    w.write_samples(100, dataset_name="first")
    assert _names(tmp_path / "val" / "images") == ["100/0_real_A-fake_B-real_B.png", "100/1_real_A-fake_B-real_B.png",
                                                   "100/2_real_A-fake_B-real_B.png",
                                                   "first/100/0_real_A-fake_B-real_B-BODY.png"]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "val" / "images" / "100" / "2_real_A-fake_B-real_B.png")), grids[2])
    # test: no iteration
    w = ImageWriter(_conf("test", tmp_path))
    w.add_samples(("real_A-fake_B-real_B", grids))
    w.write_samples(None)
    w.add_samples(("real_A-fake_B-real_B", grids[:1]))
    w.write_samples(None, dataset_name="second")
    assert _names(tmp_path / "test" / "images") == ["0_real_A-fake_B-real_B.png", "1_real_A-fake_B-real_B.png",
                                                    "2_real_A-fake_B-real_B.png", "second/0_real_A-fake_B-real_B.png"]
    assert w.write_samples(None) == []                       # the buffer was emptied
    # infer: iter_idx + i
    w = ImageWriter(_conf("infer", tmp_path))
    w.write_infer(1, ("input-output", grids[:2]))
    w.write_infer(3, ("input-output", grids[2:]))
    assert _names(tmp_path / "infer" / "images") == ["1_input-output.png", "2_input-output.png", "3_input-output.png"]
    assert (tmp_path / "infer" / "infer_config.yaml").read_text().count("output_dir") == 1
    # a backend without the kernel composes nothing, and nothing is written for it
    w = ImageWriter(_conf("train", tmp_path / "none"), ops=types.SimpleNamespace(name="oracle"))
    assert w.compose({"real_A": torch.zeros(1, 1, 2, 2)}) is None
    assert w.write_train(1, None) is None and w.write_infer(1, None) == [] and w.add_samples(None) is None
    assert not (tmp_path / "none" / "train" / "images").exists()


def test_init_engine_builds_the_inferer_and_run_asserts_in_deployment(tmp_path):
    """`infer` is an engine now; in deployment mode it has no loader and no writer and run() refuses. Building the model
    needs the backend: the fp32 oracle stands in for the GPU here."""
    from ganslate_amd.engines import init_engine
    from ganslate_amd.engines.inferer import Inferer
    from ganslate_amd.engines.utils import ENGINES
    from ganslate_amd.nn.native import backend
    from oracle.ops_ref import RefOps
    assert ENGINES["infer"] is Inferer
    backend.set_ops(RefOps(act_dtype=torch.float32))
    try:
        eng = init_engine("infer", [f"config={CONFIGS / 'infer2d_synthetic.yaml'}", "train.cuda=false",
                                    f"train.output_dir={tmp_path}", f"infer.output_dir={tmp_path}",
                                    "infer.is_deployment=true", "infer.checkpointing.load_iter=0"])
    finally:
        backend.set_ops(None)
    assert isinstance(eng, Inferer) and eng.conf.mode == "infer" and list(eng.model.networks) == ["G_AB"]
    assert not hasattr(eng, "data_loader") and not hasattr(eng, "writer")
    assert eng.output_dir == tmp_path / "infer"
    with pytest.raises(AssertionError, match="deployment"):
        eng.run()
    out = eng.infer(torch.zeros(1, 3, 32, 32))
    assert out.shape == (1, 3, 32, 32)
    assert eng._get_input_key({"input": 0, "A": 1}) == "input" and eng._get_input_key({"A": 1}) == "A"
    with pytest.raises(ValueError):
        eng._get_input_key({"B": 1})
    with pytest.raises(NotImplementedError):
        init_engine("deploy", [])
    with pytest.raises(NotImplementedError, match="no `infer` section"):      # an engine without its section has nothing to run
        init_engine("infer", [f"config={CONFIGS / 'cyclegan_synthetic.yaml'}"])
    with pytest.raises(NotImplementedError, match="no `test` section"):
        init_engine("test", [f"config={CONFIGS / 'cyclegan_synthetic.yaml'}"])


def test_save_generated_tensor_calls_the_datasets_save_with_and_without_metadata(tmp_path):
    from ganslate_amd.data.synthetic import SyntheticSavingImageDataset
    from ganslate_amd.engines.base import BaseEngineWithInference
    calls = []

    class Plain:
        def save(self, tensor, save_dir):
            calls.append((tuple(tensor.shape), Path(save_dir)))

    eng = types.SimpleNamespace(output_dir=tmp_path / "test")
    save = BaseEngineWithInference.save_generated_tensor
    batch = torch.arange(2 * 1 * 2 * 2, dtype=torch.float32).reshape(2, 1, 2, 2)
    save(eng, batch, None, types.SimpleNamespace(dataset=Plain()), idx=7, dataset_name="first")
    assert calls == [((1, 2, 2), tmp_path / "test" / "saved" / "first" / "7")] * 2
    save(eng, batch, None, types.SimpleNamespace(dataset=object()))                    # no `save`: nothing happens
    ds = SyntheticSavingImageDataset.__new__(SyntheticSavingImageDataset)
    meta = {"id": ["sample_0000", "sample_0001"], "index": torch.tensor([0, 1])}
    save(eng, batch, meta, types.SimpleNamespace(dataset=ds))
    for i in range(2):
        assert np.array_equal(np.load(tmp_path / "test" / "saved" / f"sample_000{i}.npy"), batch[i].numpy())


def test_modality_split_names_offsets_and_error():
    from ganslate_amd.hip.ops import HipOps
    a, b, m = torch.zeros(2, 4, 3, 3), torch.zeros(2, 1, 3, 3), torch.zeros(2, 1, 3, 3)
    vis = {"real_A": a, "idt_B": None, "fake_B": b, "BODY": m}
    plan = HipOps.visuals_plan(vis)
    assert [(n, c0, c) for n, _, c0, c in plan] == [("real_A", 0, 4), ("fake_B", 0, 1), ("BODY", 0, 1)]
    plan = HipOps.visuals_plan(vis, {"A": [1, 3], "B": None})
    assert [(n, c0, c) for n, _, c0, c in plan] == [("real_A1", 0, 1), ("real_A2", 1, 3), ("fake_B", 0, 1), ("BODY", 0, 1)]
    assert plan[0][1] is a and plan[1][1] is a                                           # offsets, no copy
    assert [n for n, _, _, _ in plan] == list(R.split_visuals(vis, {"A": [1, 3], "B": None}))
    plan = HipOps.visuals_plan({"real_A": a, "rec_A": a}, {"A": [2, 1, 1]})
    assert [n for n, _, _, _ in plan] == ["real_A1", "real_A2", "real_A3", "rec_A1", "rec_A2", "rec_A3"]
    with pytest.raises(ValueError, match="channel-split"):
        HipOps.visuals_plan(vis, {"A": [1, 2], "B": None})
    with pytest.raises(ValueError, match="channel-split"):
        R.split_visuals(vis, {"A": [1, 2], "B": None})


def test_oracle_threshold_values_are_the_ones_the_issue_names():
    v = R.threshold_values()
    assert v.dtype == torch.float32 and v.numel() == 4335 + 7 + 257
    x = (2 * (np.arange(1, 256, dtype=np.float64) - 0.5) / 255 - 1).astype(np.float32)
    block = v[:4335].numpy().reshape(255, 17)
    assert np.array_equal(block[:, 8], x)
    assert np.array_equal(np.nextafter(block[:, :-1], np.float32(np.inf)), block[:, 1:])    # consecutive floats
    # every window lies on its threshold: bytes k - 1 or k only, never decreasing, k at its high end and (where 8 ulp of x
    # are not lost in the rounding of x + 1, as they are just above 0) k - 1 at its low end
    _, img = R.grid_ref({"x": torch.from_numpy(block.copy()).reshape(1, 1, 255, 17)})
    got = img[0, :, :, 0].numpy().astype(np.int64)
    k = np.arange(1, 256)[:, None]
    assert ((got == k - 1) | (got == k)).all() and (np.diff(got, axis=1) >= 0).all() and (got[:, 16] == k[:, 0]).all()
    assert (got[:, 0] == k[:, 0] - 1).sum() > 200
