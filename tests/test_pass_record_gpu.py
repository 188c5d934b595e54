"""tests/test_pass_record_cpu.py's pairs on the HIP backend with the two passes of one network on two streams, the way the
recipes run them (cyclegan.py:120-137: a pass launched on a side stream has its backward run there by autograd;
`multi_stream_passes` orders the backward passes of one network by events): recorded before either backward, replayed in the
opposite order, they must leave bit for bit what the copy leaves that runs one pass at a time on one stream. Plus a tap pass
whose output gradients were produced on a side stream (the node notes their use on its own stream) against the same pass on
one stream.

Sizes: 2 images of 32 x 32 for the 2-D networks; one 16^3 volume for the V-Net with first_layer_channels=8 (the constructor
takes no fewer) and two levels of one coupling each, 16 -> 8 -> 4 — small extents that every layer still accepts."""
import pytest
import torch

from ganslate_amd.nn.native import backend

from .test_pass_record_cpu import copy_of, record

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dev(hip_ops):
    backend.set_ops(hip_ops)
    return hip_ops.device


def fresh(make, seed):
    torch.manual_seed(seed)
    net = make()
    net.init_weights("normal", 0.05)
    return net, copy_of(make, net)


class Case:
    """tests/test_pass_record_cpu.py's Case with everything on the device, drawn before any stream forks"""

    def __init__(self, dev, seed, shapes, out_shapes):
        g = torch.Generator().manual_seed(seed)
        self.x = [(torch.rand(*s, generator=g) * 2 - 1).to(dev) for s in shapes]
        self.w = {k: [torch.randn(*s, generator=g).to(dev) for s in ss] for k, ss in out_shapes.items()}
        self.leaves = []

    def leaf(self, i, grad=True):
        t = self.x[i].clone().requires_grad_(grad)
        self.leaves.append(t)
        return t

    def loss(self, key, *outs):
        assert [tuple(o.shape) for o in outs] == [tuple(w.shape) for w in self.w[key]]
        return sum((o * w).sum() for o, w in zip(outs, self.w[key]))


def run_pair_on_two_streams(net, ref, case, first, second):
    main = torch.cuda.current_stream()
    net.refresh_packs(case.x[0])           # the weight packs are shared by both streams: refreshed before the fork
    net.multi_stream_passes = True
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    recs = []
    for st, one_pass in zip(sides, (first, second)):
        st.wait_stream(main)
        with torch.cuda.stream(st):
            recs.append(record(case, one_pass, [net]))
    (l1, in1), (l2, in2) = recs
    l2.backward()                          # autograd runs each pass's backward on the stream its forward ran on
    l1.backward()
    for st in sides:
        main.wait_stream(st)
    want = []
    for one_pass in (second, first):       # the copy: one pass at a time on one stream, in that backward order
        loss, leaves = record(case, one_pass, [ref])
        loss.backward()
        want = leaves + want
    net.flush_deferred_wgrads()
    ref.flush_deferred_wgrads()
    torch.cuda.synchronize()
    assert bool(net.master.grad.any()) and torch.equal(net.master.grad, ref.master.grad)
    got = in1 + in2
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert (a.grad is None) == (b.grad is None) == (not a.requires_grad)
        if a.grad is not None:
            assert bool(a.grad.any()) and torch.equal(a.grad, b.grad)


def test_channel_pair_pass_and_plain_pass_on_two_streams(dev):
    from ganslate_amd.nn.discriminators import PatchGAN2D
    net, ref = fresh(lambda: PatchGAN2D(6, 64, 3, (4, 4), "instance"), 3)
    c = Case(dev, 4, [(2, 3, 32, 32), (2, 3, 32, 32), (2, 6, 32, 32)], {"cat": [(2, 1, 2, 2)], "plain": [(2, 1, 2, 2)]})
    cat = lambda n: c.loss("cat", *n[0].forward_parts_cat([(c.leaf(0), c.leaf(1, grad=False))]))
    plain = lambda n: c.loss("plain", n[0](c.leaf(2)))
    run_pair_on_two_streams(net, ref, c, cat, plain)


def test_vnet_pass_in_each_direction_on_two_streams(dev):
    from ganslate_amd.nn.generators import Vnet3D
    make = lambda: Vnet3D(1, 1, "instance", first_layer_channels=8, down_blocks=(1, 1), up_blocks=(1, 1),
                          use_memory_saving=False, use_inverse=True)
    net, ref = fresh(make, 7)
    vol = (1, 1, 16, 16, 16)
    c = Case(dev, 8, [vol, vol], {"ab": [vol], "ba": [vol]})
    ab = lambda n: c.loss("ab", n[0](c.leaf(0)))
    ba = lambda n: c.loss("ba", n[0](c.leaf(1), inverse=True))
    run_pair_on_two_streams(net, ref, c, ab, ba)


def test_tap_pass_takes_gradients_produced_on_a_side_stream(dev):
    from ganslate_amd.nn.generators import Resnet2D
    net, ref = fresh(lambda: Resnet2D(3, 3, "instance", 2), 9)
    layers = [4, 8]            # (a raw conv output and an activated one)
    taps = [net.encoder_tap(e)[0] for e in layers]
    g = torch.Generator().manual_seed(10)
    ids = [[torch.randperm(net.tap_extent(e, 32, 32), generator=g)[:16].to(dev) for e in layers] for _ in range(2)]
    chans = [net.encoder_tap(e)[1] for e in layers]
    c = Case(dev, 11, [(1, 3, 32, 32), (1, 3, 32, 32)], {"taps": [(1, 16, ch) for _ in range(2) for ch in chans]})
    res = []
    for n, side in ((net, torch.cuda.Stream()), (ref, None)):
        main = torch.cuda.current_stream()
        x, y = c.leaf(0), c.leaf(1, grad=False)
        feats = n.forward_taps_parts((x, y), taps, ids)
        flat = [f for part in feats for f in part]
        if side is None:
            c.loss("taps", *flat).backward()
        else:
            side.wait_stream(main)
            with torch.cuda.stream(side):            # the loss and (through autograd) its gradients live on the side stream
                loss = c.loss("taps", *flat)
            loss.backward()
            main.wait_stream(side)
        torch.cuda.synchronize()
        res.append(([f.detach() for f in flat], x.grad, n.master.grad))
        assert y.grad is None and bool(x.grad.any()) and bool(n.master.grad.any())
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
