"""CUT on the V-Net generators on the HIP path: the encoder-only partial pass against the oracle backend, the tap kernels
on volumes, whole iterations against the real reference's golden losses (tests/golden/cut_vnet.json), the captured step,
run-to-run reproducibility, and one iteration of the brats cut.yaml's networks at its patch size through the Trainer.
Tolerances as in tests/test_cut_gpu.py (bf16 storage)."""
import pytest
import torch

from .cut_vnet import CONF, build_product_cut_vnet, load_golden_cut_vnet, run_product_cut_vnet_steps

pytestmark = pytest.mark.gpu


def test_tap_gather_and_scatter_address_volumes_by_flat_row(hip_ops):
    """gs_tap_gather takes flat row ids over pixels = D H W; gs_tap_scatter_add with f0 = 0 and Wp = W maps an id to itself:
    both serve [n, D, H, W, cs] buffers unchanged. Shapes: a small odd one, and the brats cut.yaml's level 0 as the batched
    target pass holds it (2 x 32 x 176 x 176 x 16 — 31.7 M elements, the largest buffer a tap touches there; none reaches
    2^31 elements)."""
    from oracle.ops_ref import RefOps
    ref = RefOps(act_dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(7)
    for shape, c, P in (((2, 3, 5, 7, 24), 20, 33), ((2, 32, 176, 176, 16), 16, 256), ((1, 4, 22, 22, 128), 128, 256)):
        n, cs = shape[0], shape[-1]
        voxels = shape[1] * shape[2] * shape[3]
        src = (torch.rand(shape, generator=g) * 2 - 1).to(torch.bfloat16)
        pid = torch.randperm(voxels, generator=g)[:P]
        pid[0], pid[1] = voxels - 1, 0                 # both ends of the buffer
        got = hip_ops.tap_gather(src.to(hip_ops.device), pid.to(hip_ops.device), c)
        assert torch.equal(got.cpu(), ref.tap_gather(src, pid, c))
        assert torch.equal(got.cpu(), src.reshape(n, voxels, cs)[:, pid, :c].float())
        rows = torch.randn(n, P, c, generator=g)
        dst = (torch.rand(shape, generator=g) * 2 - 1).to(torch.bfloat16)
        want = dst.clone()
        ref.tap_scatter_add(want, pid, rows, shape[-2])
        dev = dst.to(hip_ops.device)
        hip_ops.tap_scatter_add(dev, pid.to(hip_ops.device), rows.to(hip_ops.device), shape[-2])
        torch.cuda.synchronize()
        assert torch.equal(dev.cpu(), want), shape


def test_vnet3d_feature_taps_hip_vs_oracle_backend(hip_ops):
    """encoder-only partial pass of Vnet3D in bf16: sampled features and the gradients they send into the encoder and the
    input, one batch and two batches in one pass; caps as for Resnet2D in tests/test_cut_gpu.py, measured values are printed"""
    from ganslate_amd.nn.generators import Vnet3D
    from ganslate_amd.nn.native import backend
    from oracle import torch_ref
    from oracle.ops_ref import RefOps
    arch = (16, (2, 2, 3), (3, 3, 3))
    sd = torch_ref.seeded_state_dict(torch_ref.Vnet3D(1, 1, *arch), 63)
    g = torch.Generator().manual_seed(63)
    sizes = (16, 32, 48)
    xs = [torch.rand(1, 1, *sizes, generator=g) * 2 - 1 for _ in range(2)]
    layers = [0, 1, 2, 3]
    rel = lambda a, b: ((a - b).norm() / (b.norm() + 1e-12)).item()
    for parts in (1, 2):
        res = {}
        for name, ops in (("hip", hip_ops), ("cpu", RefOps(act_dtype=torch.bfloat16))):
            backend.set_ops(ops)
            try:
                net = Vnet3D(1, 1, "instance", *arch, use_memory_saving=False, use_inverse=False)
                net.load_state_dict(sd)
                gg = torch.Generator().manual_seed(64)
                ids = [[torch.randperm(net.tap_extent(e, *sizes), generator=gg)[:64].to(ops.device) for e in layers]
                       for _ in range(parts)]
                xi = [x.clone().to(ops.device).requires_grad_() for x in xs[:parts]]
                feats = [net.extract_patch_features(xi[0], layers, ids[0])] if parts == 1 else \
                    net.extract_patch_features_parts(xi, layers, ids)
                feats = [f for per in feats for f in per]
                w = [torch.randn(f.shape, generator=gg).to(ops.device) for f in feats]
                sum((f * ww).sum() for f, ww in zip(feats, w)).backward()
                res[name] = ([f.detach().cpu() for f in feats], [x.grad.cpu() for x in xi], net.master.grad.cpu().clone())
            finally:
                backend.set_ops(hip_ops)
        worst_f = max(rel(fh, fc) for fh, fc in zip(res["hip"][0], res["cpu"][0]))
        worst_x = max(rel(a, b) for a, b in zip(res["hip"][1], res["cpu"][1]))
        worst_w = rel(res["hip"][2], res["cpu"][2])
        print(f"vnet3d taps, {parts} part(s): features {worst_f:.3e}, input gradient {worst_x:.3e}, "
              f"parameter gradients {worst_w:.3e}")
        assert worst_f <= 2e-2
        assert worst_x <= 0.30
        assert worst_w <= 0.30


@pytest.mark.parametrize("case", ["cutv_16x24x32_p256", "cutv_16x24x32_p32"])
def test_cut_vnet_step_matches_reference_golden(hip_ops, case):
    from .envelope import step_tolerance  # iteration 0: 2e-2; later: the reference's own scatter (envelope.json)
    gold = load_golden_cut_vnet()[case]
    c = gold["config"]
    model = build_product_cut_vnet(c)
    assert model.networks["G"].ops.name == "hip" and model.graph_capturable
    got = run_product_cut_vnet_steps(model, c, c["steps"])
    for s in range(c["steps"]):
        g = gold["steps"][s]
        assert got[s]["lrs"] == pytest.approx(g["lrs"], abs=1e-12)
        for k, v in g["losses"].items():
            tol = step_tolerance(k, s, {"adv": 2e-2, "cycle": 2e-2})
            print(case, s, k, got[s]["losses"][k], v, f"rel {abs(got[s]['losses'][k] / v - 1):.2e} (tol {tol:.2e})")
            assert got[s]["losses"][k] == pytest.approx(v, rel=tol), (s, k, got[s]["losses"][k], v)


def test_cut_vnet_captured_step_equals_launch_by_launch_with_the_flip_coin(hip_ops, monkeypatch):
    """the captured step holds for a V-Net generator: patch ids over (D, H, W) and the W-mirrored target ids are host
    state, the coin is device data — five iterations with a coin sequence that has both outcomes"""
    import numpy as np
    c = load_golden_cut_vnet()["cutv_16x24x32_p32"]["config"]
    runs = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("GS_STEP_GRAPH", graph)
        np.random.seed(7)
        model = build_product_cut_vnet(c, extra=("train.gan.use_equivariance_flip=true",))
        assert model.use_equivariance_flip and model.graph_capturable
        runs[graph] = run_product_cut_vnet_steps(model, c, 5)
        assert (model._graph is not None) == (graph == "1")
    coins = np.random.RandomState(7).random_sample(5) > 0.5
    assert coins.any() and not coins.all(), "pick a seed with both outcomes"
    for s, (a, b) in enumerate(zip(runs["1"], runs["0"])):
        for k in b["losses"]:
            assert a["losses"][k] == pytest.approx(b["losses"][k], rel=2e-3, abs=1e-5), (s, k)


def test_cut_vnet_step_is_reproducible_bit_for_bit(hip_ops):
    """no atomics came with the volume taps: two runs give the same losses and the same weights, bit for bit"""
    c = load_golden_cut_vnet()["cutv_16x24x32_p256"]["config"]
    runs = []
    for _ in range(2):
        model = build_product_cut_vnet(c)
        losses = run_product_cut_vnet_steps(model, c, 3)
        torch.cuda.synchronize()
        runs.append((losses, {n: net.master.detach().cpu().clone() for n, net in model.networks.items()}))
    assert runs[0][0] == runs[1][0]
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_brats_cut_yaml_runs_one_iteration_through_the_trainer(hip_ops, tmp_path):
    """the brats cut.yaml's networks and patch size (Vnet3D 16 / [2,2,3] / [3,3,3], PatchGAN3D n_layers 2, nce_layers
    [0..4], 32 x 176 x 176, batch 1) from tests/configs/cut_vnet3d_synthetic.yaml: finite losses, the reference's
    state_dict keys, and a checkpoint that loads back to the same tensors"""
    from ganslate_amd.engines import init_engine
    from ganslate_amd.utils.builders import build_conf, build_gan
    from oracle import torch_ref
    args = [f"config={CONF}", f"train.output_dir={tmp_path}", "train.n_iters=1", "train.n_iters_decay=0",
            "train.checkpointing.freq=1", "train.logging.freq=1", "train.seed=3"]
    tr = init_engine("train", args)
    model = tr.model
    assert model.networks["G"].ops.name == "hip"
    assert model.nce_layers == [0, 1, 2, 3, 4] and model.tap_layers == [0, 1, 2, 3]
    assert model.networks["mlp"].channels == [16, 32, 64, 128]
    tr.run()
    torch.cuda.synchronize()
    assert [h[0] for h in tr.history] == [1]
    losses = tr.history[0][1]
    assert set(losses) >= {"D", "G", "NCE", "NCE_idt"}
    assert all(v == v and abs(v) < 1e4 for v in losses.values()), losses
    assert tuple(model.visuals["fake_B"].shape) == (1, 1, 32, 176, 176)
    shadow = torch_ref.Vnet3D(1, 1, 16, (2, 2, 3), (3, 3, 3))
    sd = model.networks["G"].state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in shadow.state_dict().items()}
    ck = torch.load(tmp_path / "checkpoints" / "1.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"G", "D", "mlp", "optimizer_G", "optimizer_D", "optimizer_mlp"}
    assert set(ck["G"]) == set(shadow.state_dict())
    assert sorted(ck["mlp"]) == sorted(f"mlps.{i}.{m}.{p}" for i in range(4) for m in (0, 2) for p in ("weight", "bias"))
    torch.manual_seed(99)                     # NOT this run's weights: what the second model holds came from the file
    resumed = build_gan(build_conf(args + ["train.checkpointing.load_iter=1"]))
    for name, net in model.networks.items():
        mine, theirs = net.state_dict(), resumed.networks[name].state_dict()
        assert set(mine) == set(theirs)
        for k in mine:
            assert torch.equal(mine[k].cpu(), theirs[k].cpu()), (name, k)
