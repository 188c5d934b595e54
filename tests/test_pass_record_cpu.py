"""What belongs to ONE recorded pass lives in that pass's record (ganslate_amd/nn/native/net.py: PassForm, _PassFn, the
`need` mask and `tw` / `inverse` of the saved state), not on the network: two passes of one network recorded before either
backward, replayed in the opposite order, must leave exactly what the same two passes leave when each is recorded and
replayed on its own, in that backward order, on an identically initialised copy — the flat gradient of every network and
every input gradient, bit for bit (same ops in the same order per pass; the accumulation order into master.grad is the
backward order, which the copy reproduces). fp32 oracle backend; the stream side is in tests/test_pass_record_gpu.py."""
import pytest
import torch

from ganslate_amd.nn.native import backend
from ganslate_amd.nn.native.twin import TwinNet

from oracle.ops_ref import RefOps


@pytest.fixture()
def fp32_oracle_backend():
    backend.set_ops(RefOps(act_dtype=torch.float32))
    yield
    backend.set_ops(None)


def copy_of(make, src):
    net = make()
    with torch.no_grad():
        net.master.copy_(src.master)
    net.mark_packs_dirty()
    return net


def fresh(make, seed):
    torch.manual_seed(seed)
    net = make()
    net.init_weights("normal", 0.05)
    return net, copy_of(make, net)


class Case:
    """seeded inputs and output weights; leaf(i, grad) hands out a fresh leaf of input i, loss() weighs outputs"""

    def __init__(self, seed, *shapes):
        g = torch.Generator().manual_seed(seed)
        self.x = [torch.rand(*s, generator=g) * 2 - 1 for s in shapes]
        self.g, self.leaves = g, []
        self.w = {}

    def leaf(self, i, grad=True):
        t = self.x[i].clone().requires_grad_(grad)
        self.leaves.append(t)
        return t

    def loss(self, key, *outs):
        if key not in self.w:
            self.w[key] = [torch.randn(o.shape, generator=self.g) for o in outs]
        return sum((o * w).sum() for o, w in zip(outs, self.w[key]))


def record(case, one_pass, nets):
    """-> (loss, the leaves the pass drew)"""
    k = len(case.leaves)
    loss = one_pass(nets)
    return loss, case.leaves[k:]


def run_pair(nets, copies, case, first, second):
    """first, second: callables (networks) -> loss of one pass over fresh leaves"""
    (l1, in1), (l2, in2) = record(case, first, nets), record(case, second, nets)     # both recorded before either backward
    l2.backward()                                                                    # ... and replayed in the opposite order
    l1.backward()
    want = []
    for one_pass in (second, first):            # the copy: one pass at a time, in that backward order
        loss, leaves = record(case, one_pass, copies)
        loss.backward()
        want = leaves + want
    for net, ref in zip(nets, copies):
        net.flush_deferred_wgrads()
        ref.flush_deferred_wgrads()
        assert bool(net.master.grad.any()) and torch.equal(net.master.grad, ref.master.grad)
    got = in1 + in2
    assert len(got) == len(want) and any(t.requires_grad for t in got)
    for a, b in zip(got, want):
        assert (a.grad is None) == (b.grad is None) == (not a.requires_grad)
        if a.grad is not None:
            assert bool(a.grad.any()) and torch.equal(a.grad, b.grad)


def patchgan(cin):
    from ganslate_amd.nn.discriminators import PatchGAN2D
    return lambda: PatchGAN2D(cin, 8, 2, (4, 4), "instance")


def unet():
    from ganslate_amd.nn.generators import Unet2D
    return Unet2D(3, 3, 5, "instance", ngf=8)


def vnet(**kw):
    from ganslate_amd.nn.generators import Vnet3D
    return lambda: Vnet3D(1, 1, "instance", first_layer_channels=8, down_blocks=(1, 1), up_blocks=(1, 1),
                          use_memory_saving=False, **kw)


def test_channel_pair_pass_interleaved_with_a_plain_pass(fp32_oracle_backend):
    """forward_parts_cat with the mask (grad, no grad) recorded, then a plain forward whose input wants a gradient; the plain
    pass's backward runs first"""
    net, ref = fresh(patchgan(6), 3)
    c = Case(4, (2, 3, 16, 16), (2, 3, 16, 16), (2, 6, 16, 16))
    cat = lambda n: c.loss("cat", *n[0].forward_parts_cat([(c.leaf(0), c.leaf(1, grad=False))]))
    plain = lambda n: c.loss("plain", n[0](c.leaf(2)))
    run_pair([net], [ref], c, cat, plain)


def test_pix2pix_concatenates_for_a_discriminator_without_channel_sources(fp32_oracle_backend):
    """A discriminator whose images do not enter through the plain image conversion (a W-folded k7 stem:
    supports_channel_sources() is False) has forward_parts_cat like every NativeNet, and refuses it. The recipe's two D calls
    hand it torch.cat([real_A, fake_B], dim=1) instead: predictions, losses and parameter gradients are those of an identical
    copy fed the concatenated tensors, bit for bit, and fake_B's gradient reaches the generator."""
    from ganslate_amd.nn.generators import Resnet2D
    from .helpers import build_product_pix2pix
    c = dict(size=[32, 32], batch=1, n_iters=100, n_iters_decay=100, num_downs=5, ngf=8, use_dropout=False, n_layers=2,
             lambda_pix2pix=30.0, seed=27)
    model = build_product_pix2pix(c)
    # one-channel images: the two-channel pair is few enough channels for the stem's W taps to be folded into them
    model.networks["G"] = fresh(lambda: Resnet2D(1, 1, "instance", 1), 28)[0]
    D, ref = fresh(lambda: Resnet2D(2, 1, "instance", 1), 29)
    model.networks["D"] = D
    A, B = (torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(30 + k)) * 2 - 1 for k in range(2))
    assert D.nodes[0].spec.wfold == "in" and not D.supports_channel_sources()
    with pytest.raises(NotImplementedError):
        D.forward_parts_cat([(A, B)])
    model.set_input({"A": A, "B": B})
    model.forward()
    fake_B = model.visuals["fake_B"].detach()
    model.set_requires_grad(D, False)
    model.backward_G()
    with torch.no_grad():
        assert float(model.losses["G"]) == float(model.criterion_adv(ref(torch.cat([A, fake_B], dim=1)), target_is_real=True))
    model.networks["G"].flush_deferred_wgrads()
    assert bool(model.networks["G"].master.grad.any()) and (D.master.grad is None or not bool(D.master.grad.any()))
    model.set_requires_grad(D, True)
    model.backward_D()
    want_real, want_fake = ref.forward_parts((torch.cat([A, B], dim=1), torch.cat([A, fake_B], dim=1)))
    assert torch.equal(model.pred_real, want_real) and torch.equal(model.pred_fake, want_fake)
    (model.criterion_adv(want_real, target_is_real=True) + model.criterion_adv(want_fake, target_is_real=False)).backward()
    D.flush_deferred_wgrads()
    ref.flush_deferred_wgrads()
    assert bool(D.master.grad.any()) and torch.equal(D.master.grad, ref.master.grad)


@pytest.mark.parametrize("arch", ["native", "unet2d"])
def test_channel_source_passes_with_two_masks(fp32_oracle_backend, arch):
    net, ref = fresh(patchgan(3) if arch == "native" else unet, 5)
    hw = (16, 16) if arch == "native" else (32, 32)          # (the smallest extents every layer of each still accepts)
    c = Case(6, (2, 2, *hw), (2, 4, *hw), (2, 1, *hw))
    one = lambda n: c.loss("one", *n[0].forward_sources([[(c.leaf(0), 0, 2), (c.leaf(1, grad=False), 3, 4)]]))
    two = lambda n: c.loss("two", *n[0].forward_sources([[(c.leaf(0, grad=False), 0, 2), (c.leaf(2), 0, 1)]]))
    run_pair([net], [ref], c, one, two)


def test_vnet_pass_in_each_direction(fp32_oracle_backend):
    net, ref = fresh(vnet(use_inverse=True), 7)
    c = Case(8, (1, 1, 4, 4, 4), (1, 1, 4, 4, 4))
    ab = lambda n: c.loss("ab", n[0](c.leaf(0)))
    ba = lambda n: c.loss("ba", n[0](c.leaf(1), inverse=True))
    run_pair([net], [ref], c, ab, ba)
    for name, g in net.grads_state_dict().items():          # each direction reached its own layers
        if name in ("in_ab.conv1.weight", "in_ba.conv1.weight", "out_ab.conv2.weight", "out_ba.conv2.weight"):
            assert bool(g.any()), name


def test_vnet_alone_and_as_first_network_of_a_twin(fp32_oracle_backend):
    make = vnet(use_inverse=False)
    a, a1 = fresh(make, 9)
    b, b1 = fresh(make, 10)
    c = Case(11, (1, 1, 4, 4, 4), (1, 1, 4, 4, 4), (1, 1, 4, 4, 4))
    alone = lambda n: c.loss("alone", n[0](c.leaf(0)))
    twin = lambda n: c.loss("twin", *TwinNet(n[0], n[1])(c.leaf(1), c.leaf(2)))
    run_pair([a, b], [a1, b1], c, alone, twin)


# ---- what the node hands back to autograd -------------------------------------------------------------------------------
def node_returns(outs, case):
    """the input gradients the pass's node returns behind those of (token, form): its backward, called directly with seeded
    output gradients"""
    outs = outs if isinstance(outs, (tuple, list)) else (outs,)
    return outs[0].grad_fn.apply(*[torch.randn(o.shape, generator=case.g) for o in outs])[2:]


def test_an_input_that_wants_no_gradient_gets_none_in_every_form(fp32_oracle_backend):
    c = Case(12, (2, 3, 32, 32), (1, 3, 32, 32), (2, 1, 32, 32), (1, 1, 4, 4, 4), (1, 1, 4, 4, 4))
    x, y, z = c.leaf(0), c.leaf(1, grad=False), c.leaf(2, grad=False)
    d6, d3 = fresh(patchgan(6), 13)[0], fresh(patchgan(3), 14)[0]
    d3.master.requires_grad = False                                        # (a frozen network still passes input gradients)
    forms = {
        "forward_parts": (d3.forward_parts((y, x)), [False, True]),
        "forward_parts_cat": (d6.forward_parts_cat([(c.leaf(0, grad=False), x)]), [False, True]),
        "forward_sources": (d3.forward_sources([[(c.leaf(0, grad=False), 0, 2), (z, 0, 1)], [(x, 0, 3)]]),
                            [False, False, True]),
        "unet forward_sources": (unet().forward_sources([[(x, 0, 3)]]), [True]),
    }
    d3b = fresh(patchgan(3), 15)[0]
    d3b.master.requires_grad = False
    pa, pb = TwinNet(d3, d3b)((y, c.leaf(1, grad=False)), (c.leaf(1), y))
    forms["twin"] = (pa + pb, [False, False, True, False])
    va, vb = fresh(vnet(use_inverse=False), 16)[0], fresh(vnet(use_inverse=False), 17)[0]
    forms["vnet parts"] = (va.forward_parts((c.leaf(3, grad=False), c.leaf(4))), [False, True])
    for name, (outs, mask) in forms.items():
        grads = node_returns(outs, c)
        assert [g is not None for g in grads] == mask, name
    # a whole-batch pass of a trainable network over an input that wants none, and a tap pass
    assert node_returns(d6(c.leaf(0, grad=False).repeat(1, 2, 1, 1)), c) == (None,)
    from ganslate_amd.nn.generators import Resnet2D
    g = fresh(lambda: Resnet2D(3, 3, "instance", 2), 18)[0]
    taps = [g.encoder_tap(e)[0] for e in (4, 8)]
    ids = [[torch.randint(0, 64, (5,), generator=c.g) for _ in taps] for _ in range(2)]
    feats = g.forward_taps_parts((y, c.leaf(1)), taps, ids)
    grads = node_returns([f for part in feats for f in part], c)
    assert [t is not None for t in grads] == [False, True]


def test_an_output_left_out_of_the_loss_gives_its_input_a_zero_gradient(fp32_oracle_backend):
    c = Case(19, (2, 3, 16, 16), (1, 3, 16, 16), (1, 1, 4, 4, 4), (2, 1, 4, 4, 4))
    d3, d3b = fresh(patchgan(3), 20)[0], fresh(patchgan(3), 21)[0]
    x, y = c.leaf(0), c.leaf(1)
    used, _ = d3.forward_parts((x, y))
    c.loss("parts", used).backward()
    assert bool(x.grad.any()) and torch.equal(y.grad, torch.zeros_like(y))
    xa, ya, xb, yb = c.leaf(0), c.leaf(1), c.leaf(0), c.leaf(1)
    (pa, _), (_, pb) = TwinNet(d3, d3b)((xa, ya), (xb, yb))
    c.loss("twin", pa, pb).backward()
    assert bool(xa.grad.any()) and bool(yb.grad.any())
    assert torch.equal(ya.grad, torch.zeros_like(ya)) and torch.equal(xb.grad, torch.zeros_like(xb))
    v = fresh(vnet(use_inverse=False), 22)[0]
    p, q = c.leaf(2), c.leaf(3)
    _, used = v.forward_parts((p, q))
    c.loss("vnet", used).backward()
    assert bool(q.grad.any()) and torch.equal(p.grad, torch.zeros_like(p))


def test_recorded_pass_finds_whole_batch_and_parts_passes_only(fp32_oracle_backend):
    c = Case(23, (2, 3, 16, 16), (1, 3, 16, 16))
    d3, d6 = fresh(patchgan(3), 24)[0], fresh(patchgan(6), 25)[0]
    x, y = c.leaf(0), c.leaf(1)
    out = d3(x)
    saved, n0 = d3.recorded_pass(x)
    assert n0 == 0 and saved.N == 2 and saved is out.grad_fn.saved
    outs = d3.forward_parts((x, y))
    (sx, nx), (sy, ny) = d3.recorded_pass(x), d3.recorded_pass(y)
    assert sx is sy is outs[0].grad_fn.saved and (nx, ny) == (0, 2) and sx.N == 3
    a, b = c.leaf(0), c.leaf(0)
    pred, = d6.forward_parts_cat([(a, b)])
    assert pred.grad_fn.saved is not None and d6.recorded_pass(a) is None and d6.recorded_pass(b) is None
    # a pass that has run its backward is no longer handed out
    c.loss("w", *outs).backward()
    assert d3.recorded_pass(y) is None
