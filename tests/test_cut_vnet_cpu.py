"""CUT on the V-Net generators (projects/brats_mri_sequence_translation/experiments/cut.yaml) on the fp32 oracle backend:
the encoder-only partial pass of Vnet3D / Vnet2D / SelfAttentionVnet3D against the oracle's `encoder` walked module by
module (ganslate/nn/gans/unpaired/cut.py:297-312), the recipe's dimension-agnostic patch ids, the reference's handling of
an `nce_layers` index equal to the encoder's length, and whole iterations against the real reference's golden losses
(tests/golden/cut_vnet.json, tools/gen_golden_cut_vnet.py)."""
import pytest
import torch

from ganslate_amd.nn.native import backend
from oracle import torch_ref
from oracle.ops_ref import RefOps

from .cut_vnet import build_product_cut_vnet, load_golden_cut_vnet, run_product_cut_vnet_steps


@pytest.fixture()
def fp32_oracle_backend():
    backend.set_ops(RefOps(act_dtype=torch.float32))
    yield
    backend.set_ops(None)


def _rows(feat):
    """[N, C, *spatial] -> [N, pixels, C], the reference's permute + flatten (cut.py:252-257)"""
    return feat.movedim(1, -1).flatten(1, -2)


def _oracle_taps(shadow, xs, layers, ids_per_part, weights):
    """walks `shadow.encoder` over every batch, samples the listed layers, and sends sum(feature * weight) back"""
    feats = []
    for x, ids in zip(xs, ids_per_part):
        f, per = x, []
        for e, module in enumerate(shadow.encoder):
            f = module(f)
            if e in layers:
                per.append(_rows(f)[:, ids[layers.index(e)], :])
        feats.append(per)
    sum((f * w).sum() for per, ws in zip(feats, weights) for f, w in zip(per, ws)).backward()
    return feats


def _assert_gradients(native, shadow, what):
    """every parameter gradient, mapped through state_dict names, with the tolerances of tests/test_networks_cpu.py::_compare:
    1e-3 of the tensor's largest gradient (+ 1e-7); a bias in front of an InstanceNorm has an exactly-zero true gradient,
    so only its smallness relative to the layer's weight gradient is checked. Parameters the encoder walk does not reach
    (up path, OutBlock, attention) have no gradient on the oracle side and must be untouched zeros here."""
    grads = native.grads_state_dict()
    normed = {nd.name for nd in native.nodes if nd.norm}
    named = {n: p for n, p in shadow.named_parameters() if not n.startswith("encoder.")}
    seen = 0
    for n, p in named.items():
        got = grads[n].reshape(p.shape)
        if p.grad is None:
            assert got.abs().max().item() == 0.0, (what, n)
            continue
        seen += 1
        if n.endswith(".bias") and n[:-5] in normed:
            wscale = named[n[:-5] + ".weight"].grad.abs().max().item()
            assert p.grad.abs().max().item() <= 1e-3 * wscale and got.abs().max().item() <= 1e-3 * wscale, (what, n)
            continue
        scale = p.grad.abs().max().item()
        assert (p.grad - got).abs().max().item() <= 1e-3 * scale + 1e-7, (what, n, (p.grad - got).abs().max().item(), scale)
    return seen


def _tap_case(native, shadow, x_shape, layers, parts, seed, P=24):
    sd = torch_ref.seeded_state_dict(shadow, seed)
    shadow.load_state_dict(sd)
    native.load_state_dict(sd)
    g = torch.Generator().manual_seed(seed)
    sizes = x_shape[2:]
    xs = [torch.rand(x_shape, generator=g) * 2 - 1 for _ in range(parts)]
    ids = [[torch.randperm(native.tap_extent(e, *sizes), generator=g)[:P] for e in layers] for _ in range(parts)]
    xa = [x.clone().requires_grad_() for x in xs]
    xb = [x.clone().requires_grad_() for x in xs]
    if parts == 1:
        got = [native.extract_patch_features(xb[0], layers, ids[0])]
    else:
        got = native.extract_patch_features_parts(xb, layers, ids)
    weights = [[torch.randn(f.shape, generator=g) for f in per] for per in got]
    want = _oracle_taps(shadow, xa, layers, ids, weights)
    sum((f * w).sum() for per, ws in zip(got, weights) for f, w in zip(per, ws)).backward()
    for p, (gp, wp) in enumerate(zip(got, want)):
        assert len(gp) == len(wp) == len(layers)
        for e, a, b in zip(layers, gp, wp):
            assert a.shape == b.shape and a.dtype == torch.float32
            assert torch.allclose(a, b, atol=2e-5, rtol=1e-4), (p, e, (a - b).abs().max())
    for a, b in zip(xa, xb):
        gscale = a.grad.abs().max().item()
        assert (a.grad - b.grad).abs().max().item() <= 1e-3 * gscale, (a.grad - b.grad).abs().max()
    return _assert_gradients(native, shadow, (type(native).__name__, parts))


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("memory_saving", [False, True])
def test_vnet3d_encoder_taps_match_the_oracle_encoder_walk(fp32_oracle_backend, memory_saving, parts):
    """features, input gradient and every parameter gradient of the partial pass; all four tap levels, gradients injected
    at each of them. Depth, height and width differ so that a wrong axis order in the flat ids cannot pass."""
    from ganslate_amd.nn.generators import Vnet3D
    native = Vnet3D(1, 1, "instance", 8, (1, 2, 1), (1, 2, 1), use_memory_saving=memory_saving, use_inverse=False)
    shadow = torch_ref.Vnet3D(1, 1, 8, (1, 2, 1), (1, 2, 1))
    assert native.encoder_len() == len(shadow.encoder) == 4
    seen = _tap_case(native, shadow, (2, 1, 8, 16, 24), [0, 1, 2, 3], parts, 171 + parts)
    assert seen == sum(1 for n, _ in shadow.named_parameters() if n.startswith(("in_ab.", "downs.")))


def test_vnet3d_taps_of_a_subset_of_levels_and_two_input_channels(fp32_oracle_backend):
    """levels 0 and 2 only: the pass stops at DownBlock 1, level 1 receives no injected rows; in_channels 2 (x.repeat)"""
    from ganslate_amd.nn.generators import Vnet3D
    native = Vnet3D(2, 1, "instance", 8, (1, 1, 1), (1, 1, 1), use_memory_saving=False, use_inverse=False)
    _tap_case(native, torch_ref.Vnet3D(2, 1, 8, (1, 1, 1), (1, 1, 1)), (1, 2, 8, 8, 16), [0, 2], 1, 173)
    # only level 0: no DownBlock runs at all
    native = Vnet3D(1, 1, "instance", 8, (1,), (1,), use_memory_saving=False, use_inverse=False)
    _tap_case(native, torch_ref.Vnet3D(1, 1, 8, (1,), (1,)), (1, 1, 4, 6, 8), [0], 1, 174)


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("memory_saving", [False, True])
def test_vnet2d_encoder_taps_match_the_oracle_encoder_walk(fp32_oracle_backend, memory_saving, parts):
    from ganslate_amd.nn.generators import Vnet2D
    native = Vnet2D(1, 1, "instance", 8, (1, 2), (2, 1), use_memory_saving=memory_saving, use_inverse=False)
    shadow = torch_ref.Vnet2D(1, 1, 8, (1, 2), (2, 1))
    _tap_case(native, shadow, (2, 1, 16, 24), [0, 1, 2], parts, 175 + parts)


def test_encoder_pass_of_an_inverse_capable_vnet_runs_a_to_b(fp32_oracle_backend):
    """use_inverse=True adds the B -> A layers; the encoder modules are called without `inverse` (cut.py:308)"""
    from ganslate_amd.nn.generators import Vnet3D
    native = Vnet3D(1, 1, "instance", 8, (1, 1), (1, 1), use_memory_saving=True, use_inverse=True)
    _tap_case(native, torch_ref.Vnet3D(1, 1, 8, (1, 1), (1, 1), use_inverse=True), (1, 1, 8, 8, 16), [0, 1, 2], 1, 177)


def test_tap_dims_are_the_encoder_feature_shapes(fp32_oracle_backend):
    from ganslate_amd.nn.generators import Vnet2D, Vnet3D
    for native, shadow, shape in ((Vnet3D(1, 1, "instance", 8, (1, 1, 1), (1, 1, 1), False, False),
                                   torch_ref.Vnet3D(1, 1, 8, (1, 1, 1), (1, 1, 1)), (1, 1, 8, 16, 24)),
                                  (Vnet2D(1, 1, "instance", 8, (1, 1), (1, 1), False, False),
                                   torch_ref.Vnet2D(1, 1, 8, (1, 1), (1, 1)), (1, 1, 12, 20))):
        f = torch.rand(shape)
        with torch.no_grad():
            for e, module in enumerate(shadow.encoder):
                f = module(f)
                assert native.tap_dims(e, *shape[2:]) == tuple(f.shape[2:]), e
                assert native.tap_extent(e, *shape[2:]) == f[0, 0].numel()
                assert native.encoder_tap(e) == (("x", e), f.shape[1])
        with pytest.raises(AssertionError):
            native.encoder_tap(native.encoder_len())


def test_selfattention_vnet3d_encoder_taps_skip_the_attention_blocks(fp32_oracle_backend):
    """the reference's encoder walk calls the DownBlocks only (selfattention_vnet3d.py:116, cut.py:307-308) while the full
    forward feeds the attended maps on: the features equal the oracle's encoder walk, differ from the full pass's attended
    activations, and a recorded full pass over the same tensor is not read beyond the first attended block"""
    from ganslate_amd.nn.generators import SelfAttentionVnet3D
    kw = dict(first_layer_channels=8, down_blocks=(1, 1, 1), up_blocks=(1, 1, 1))
    shadow = torch_ref.SelfAttentionVnet3D(1, 1, use_inverse=False, enable_attention_block=(False, True, True), **kw)
    native = SelfAttentionVnet3D(1, 1, "instance", use_memory_saving=False, use_inverse=False,
                                 enable_attention_block=(False, True, True), **kw)
    layers = [0, 1, 2, 3]
    _tap_case(native, shadow, (1, 1, 8, 16, 16), layers, 1, 178)           # loads the seeded weights into both
    with torch.no_grad():                      # gamma is initialised to 0 (attention = identity): give the blocks a say
        for n, p in shadow.named_parameters():
            if n.endswith("gamma"):
                p.fill_(0.7)
    native.load_state_dict(shadow.state_dict())
    g = torch.Generator().manual_seed(179)
    x = torch.rand(1, 1, 8, 16, 16, generator=g) * 2 - 1
    ids = [torch.randperm(native.tap_extent(e, 8, 16, 16), generator=g)[:16] for e in layers]
    with torch.no_grad():
        walk, f = [], x
        for module in shadow.encoder:
            f = module(f)
            walk.append(f)
        attended, f = [shadow.in_ab(x)], None
        for i, (d, attn) in enumerate(zip(shadow.downs, shadow.attn_blocks)):
            attended.append(attn(d(attended[-1])))
    assert not torch.allclose(walk[2], attended[2], atol=1e-3) and not torch.allclose(walk[3], attended[3], atol=1e-3)
    xi = x.clone().requires_grad_()
    y = native(xi)                             # a recorded full pass over this very tensor, still alive
    assert native.recorded_pass(xi.contiguous().float()) is not None
    for detached in (True, False):
        feats = native.extract_patch_features(xi, layers, ids, detached=detached)
        for e, (a, pid) in enumerate(zip(feats, ids)):
            assert torch.allclose(a, _rows(walk[e])[:, pid, :], atol=2e-5, rtol=1e-4), (detached, e)
        assert not torch.allclose(feats[3], _rows(attended[3])[:, ids[3], :], atol=1e-3)
    # up to the first attended block the recorded pass IS the encoder walk, and is read instead of a second pass
    calls = []
    fwd = native._forward
    native._forward = lambda *a, **k: (calls.append(k.get("stop")), fwd(*a, **k))[1]
    native.extract_patch_features(xi, [0, 1], ids[:2], detached=True)
    assert calls == []
    native.extract_patch_features(xi, [0, 1, 2], ids[:3], detached=True)
    assert calls == [2]
    del y


def test_recorded_pass_serves_detached_source_features(fp32_oracle_backend):
    """CUT's source patches of real_A: read out of fake_B = G(real_A)'s recorded pass — also when that pass carried
    several batches (forward_parts) — and equal to an encoder pass of their own"""
    from ganslate_amd.nn.generators import Vnet3D
    native = Vnet3D(1, 1, "instance", 8, (1, 1), (1, 1), use_memory_saving=False, use_inverse=False)
    native.load_state_dict(torch_ref.seeded_state_dict(torch_ref.Vnet3D(1, 1, 8, (1, 1), (1, 1)), 181))
    g = torch.Generator().manual_seed(181)
    a, b = (torch.rand(1, 1, 8, 8, 16, generator=g) * 2 - 1 for _ in range(2))
    layers = [0, 1, 2]
    ids = [torch.randperm(native.tap_extent(e, 8, 8, 16), generator=g)[:16] for e in layers]
    alone = [native.extract_patch_features(t, layers, ids, detached=True) for t in (a, b)]
    calls = []
    fwd = native._forward
    native._forward = lambda *a_, **k: (calls.append(k.get("stop")), fwd(*a_, **k))[1]
    ya, yb = native.forward_parts((a, b))
    single = native.forward_parts((a,))[0]
    assert torch.equal(single, ya)              # per-sample InstanceNorm: batching does not change an image's output
    n_before = len(calls)
    for t, want in zip((a, b), alone):
        for f, w in zip(native.extract_patch_features(t, layers, ids, detached=True), want):
            assert torch.equal(f, w)
    assert len(calls) == n_before               # no further pass was launched
    # the full pass over two batches sends each batch's gradient back to its own input
    a2, b2 = a.clone().requires_grad_(), b.clone().requires_grad_()
    oa, ob = native.forward_parts((a2, b2))
    w = torch.randn(oa.shape, generator=g)
    native.master.grad.zero_()
    (oa * w).sum().backward()
    a3 = a.clone().requires_grad_()
    grads_two = native.master.grad.clone()
    native.master.grad.zero_()
    (native(a3) * w).sum().backward()
    assert b2.grad is None or b2.grad.abs().max() == 0
    assert torch.allclose(a2.grad, a3.grad, atol=1e-6 * a3.grad.abs().max().item(), rtol=1e-4)
    assert (grads_two - native.master.grad).abs().max() <= 1e-4 * native.master.grad.abs().max()


# ---- the recipe ---------------------------------------------------------------------------------------------------------
def _small_cut(extra=(), nce_layers="[0,1,2,3,4]", down="[1,1,1]", up="[1,1,1]"):
    from ganslate_amd.utils.builders import build_conf, build_gan
    from .cut_vnet import CONF
    conf = build_conf([f"config={CONF}", f"train.gan.nce_layers={nce_layers}", "train.gan.num_patches=16",
                       f"train.gan.generator.down_blocks={down}", f"train.gan.generator.up_blocks={up}",
                       "train.dataset.final_size=[16,24,32]", *extra])
    torch.manual_seed(9)
    return build_gan(conf)


def test_nce_layer_index_equal_to_the_encoder_length_is_dropped_and_still_divides(fp32_oracle_backend):
    """the reference asserts len(encoder) >= max(nce_layers) (cut.py:301), extracts the layers that exist (:307-310), builds
    one MLP per extracted level (:316-331), lets zip drop the surplus criterion (:219-220) and divides by len(nce_layers)
    (:226): with three DownBlocks and nce_layers [0,1,2,3,4] that is four levels and the 4-level sum divided by FIVE"""
    model = _small_cut()
    G, mlp = model.networks["G"], model.networks["mlp"]
    assert G.encoder_len() == 4 and model.tap_layers == [0, 1, 2, 3] and model.nce_layers == [0, 1, 2, 3, 4]
    assert mlp.channels == [16, 32, 64, 128]
    assert sorted({k.split(".")[1] for k in mlp.state_dict()}) == ["0", "1", "2", "3"]
    g = torch.Generator().manual_seed(3)
    src, tgt = (torch.rand(1, 1, 16, 24, 32, generator=g) * 2 - 1 for _ in range(2))
    ids = model.sample_patch_ids(16, 24, 32)
    assert len(ids) == 4
    loss = float(model._calculate_nce_loss(src, tgt, patch_ids=ids).detach())
    # the same through the oracle's restatement of FeaturePatchMLP + PatchNCELoss on the oracle V-Net's encoder walk
    shadow = torch_ref.Vnet3D(1, 1, 16, (1, 1, 1), (1, 1, 1))
    shadow.load_state_dict(G.state_dict())
    ref_mlp = torch_ref._PatchMLP(mlp.channels, 16, 256)
    ref_mlp.load_state_dict(mlp.state_dict())
    with torch.no_grad():
        def feats(x):
            out, f = [], x
            for module in shadow.encoder:
                f = module(f)
                out.append(f.flatten(2, 3))          # (_PatchMLP flattens H, W of a 4-D map: fold D into H first)
            return out
        sp, _ = ref_mlp(feats(src), ids)
        tp, _ = ref_mlp(feats(tgt), ids)
        level_sum = sum(float(torch_ref.patch_nce(t, s, 1, model.nce_T).mean() * model.lambda_nce) for t, s in zip(tp, sp))
    assert loss == pytest.approx(level_sum / 5, rel=1e-5)
    assert loss != pytest.approx(level_sum / 4, rel=1e-2)


def test_nce_layer_index_beyond_the_encoder_length_raises(fp32_oracle_backend):
    with pytest.raises(AssertionError, match="cannot extract features from layers that do not exist"):
        _small_cut(nce_layers="[0,1,2,3,5]")
    # Resnet2D keeps its own strict check and message
    from ganslate_amd.nn.generators import Resnet2D
    with pytest.raises(AssertionError, match="encoder has 13 layers"):
        Resnet2D(3, 3, "instance", 3).encoder_layers([0, 4, 13])


def test_flat_and_flipped_ids_address_a_volume_like_the_reference(fp32_oracle_backend):
    """ids are flat over (D, H, W) in row-major order — feat.permute(0, 2, 3, 4, 1).flatten(1, 3) (cut.py:254) — and the
    flip remap addresses in feat.flip(-1) (cut.py:214) what the id addresses in feat, level by level"""
    model = _small_cut()
    G = model.networks["G"]
    sizes = (16, 24, 32)
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(12)
    ids = model.sample_patch_ids(*sizes)
    flipped = model._flipped_ids(ids, *sizes)
    for e, pid, fid in zip(model.tap_layers, ids, flipped):
        d, h, w = G.tap_dims(e, *sizes)
        assert len(pid) == min(16, d * h * w) and int(pid.max()) < d * h * w
        feat = torch.rand(2, 5, d, h, w, generator=g)
        rows = feat.permute(0, 2, 3, 4, 1).flatten(1, 3)
        z, y, x = pid // (h * w), (pid // w) % h, pid % w
        assert torch.equal(rows[:, pid, :], feat[:, :, z, y, x].permute(0, 2, 1)), e
        assert torch.equal(feat.flip(-1).permute(0, 2, 3, 4, 1).flatten(1, 3)[:, fid, :], rows[:, pid, :]), e
        # ... and those rows are what the executor's channels-last buffer is gathered by
        act = feat.permute(0, 2, 3, 4, 1).contiguous()
        assert torch.equal(G.ops.tap_gather(act, pid, 5), rows[:, pid, :])
        back = torch.zeros_like(act)
        G.ops.tap_scatter_add(back, pid, rows[:, pid, :], w)
        want = torch.zeros_like(rows)
        want[:, pid, :] = rows[:, pid, :]
        assert torch.equal(back.flatten(1, 3), want)


def test_2d_patch_id_draw_order_is_unchanged(fp32_oracle_backend):
    """one torch.randperm per level in level order: with a fixed seed Resnet2D's ids are what the recipe drew before it
    learnt about volumes (length, head and sum of every level's ids, recorded from the parent commit)"""
    from pathlib import Path
    from ganslate_amd.utils.builders import build_conf, build_gan
    conf = build_conf([f"config={Path(__file__).parent / 'configs' / 'cut_synthetic.yaml'}", "train.batch_size=1"])
    torch.manual_seed(5)
    model = build_gan(conf)
    recorded = {
        (64, 64): [(256, [355, 1531, 3268, 138, 2735, 347], 600437), (256, [973, 338, 514, 534, 629, 1007], 134880),
                   (256, [67, 61, 216, 71, 42, 20], 32640), (256, [191, 35, 115, 109, 154, 206], 32640),
                   (256, [191, 47, 194, 165, 132, 18], 32640)],
        (40, 56): [(256, [1643, 1598, 1910, 2816, 1583, 1602], 332378), (256, [164, 191, 521, 54, 42, 415], 71737),
                   (140, [34, 6, 2, 45, 83, 130], 9730), (140, [15, 91, 21, 9, 134, 70], 9730),
                   (140, [127, 106, 46, 108, 25, 100], 9730)],
    }
    for hw, want in recorded.items():
        torch.manual_seed(77)
        ids = model.sample_patch_ids(*hw)
        assert [(len(i), i[:6].tolist(), int(i.sum())) for i in ids] == want, hw
        w = [model.networks["G"].tap_dims(e, *hw)[1] for e in model.nce_layers]
        for pid, fid, ww in zip(ids, model._flipped_ids(ids, *hw), w):
            assert torch.equal(fid, (pid // ww) * ww + (ww - 1 - pid % ww))


@pytest.mark.parametrize("case", ["cutv_16x24x32_p256", "cutv_16x24x32_p32"])
def test_cut_vnet_product_step_matches_reference_golden_fp32(fp32_oracle_backend, case):
    """whole iterations of the recipe (D, then G + mlp; both PatchNCE terms; four listed layers on a three-module encoder)
    against the real reference's losses, with the tolerances of the 2-D golden test
    (tests/test_cyclegan_cpu.py::test_cut_product_step_matches_reference_golden_fp32)"""
    gold = load_golden_cut_vnet()[case]
    c = gold["config"]
    model = build_product_cut_vnet(c)
    assert len(model.tap_layers) == gold["feature_levels"] == len(c["nce_layers"]) - 1
    got = run_product_cut_vnet_steps(model, c, 2)
    for s in range(2):
        g = gold["steps"][s]
        assert got[s]["lrs"] == pytest.approx(g["lrs"], abs=1e-12)
        assert set(got[s]["losses"]) == set(g["losses"])
        for k, v in g["losses"].items():
            tol = 2e-4 if s == 0 else (0.02 if k.startswith("NCE") else 0.10)
            assert got[s]["losses"][k] == pytest.approx(v, rel=tol), (s, k, got[s]["losses"][k], v)


def test_cut_vnet_unbatched_step_equals_the_batched_one(fp32_oracle_backend, monkeypatch):
    """GS_CUT_BATCH=0 runs G(real_A), G(real_B) and the two target encoder passes one by one, as the reference does"""
    gold = load_golden_cut_vnet()["cutv_16x24x32_p32"]
    c = gold["config"]
    runs = {}
    for batch in ("1", "0"):
        monkeypatch.setenv("GS_CUT_BATCH", batch)
        runs[batch] = run_product_cut_vnet_steps(build_product_cut_vnet(c), c, 2)
    for a, b in zip(runs["1"], runs["0"]):
        for k, v in b["losses"].items():
            assert a["losses"][k] == pytest.approx(v, rel=1e-4), k
