"""Writes tests/golden/separable.json from the IMPORTED reference's own Vnet3D(is_separable=True) (needs the reference
checkout next to the stand-in modules of oracle/ref_stubs, like oracle/gen_golden.py):

    python tools/gen_golden_separable.py

Case: 1 -> 1 channels, first_layer_channels 8, down_blocks (1, 1), up_blocks (1, 1), input 1 x 1 x 8 x 16 x 24 (three
different extents: an axis mix-up cannot cancel), use_inverse False and True. The file holds numbers only: weights are
oracle.torch_ref.seeded_state_dict draws (entry k of the state dict ~ N(0, 1) from torch.Generator(weight_seed * 1000 + k),
times 0.01 for biases and 0.02 otherwise), recorded per state-dict key as [shape, sum] — or "=<key>" for a second name of the
same tensor — so a test regenerates them bit for bit; `param_grads` follows the keys that are not second names, null where
the run left a parameter without gradient; outputs in full as integers in units of OUTPUT_SCALE (tanh outputs: |y| < 1; the 5e-7 this
rounds by is far below the 1e-5 the comparisons allow); gradients as per-parameter norms plus a seeded sample of elements."""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle" / "ref_stubs"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, str(ROOT))

import ganslate.configs.base  # noqa: E402,F401
from ganslate.nn.generators.vnet.vnet3d import Vnet3D  # noqa: E402

SEED = 97
SHAPE = (1, 1, 8, 16, 24)
GAIN, BIAS_GAIN = 0.02, 0.01
SAMPLES = 4            # gradient elements recorded per parameter
OUTPUT_SCALE = 1e-6


def f32(t):
    return [float("%.9g" % v) for v in t.detach().flatten().tolist()]


def seeded(net, seed):
    """oracle.torch_ref.seeded_state_dict, with the recipe of every draw written down"""
    sd, rec, seen = {}, {}, {}
    for k, (name, t) in enumerate(net.state_dict().items()):
        if t.data_ptr() in seen:
            sd[name], rec[name] = sd[seen[t.data_ptr()]], "=" + seen[t.data_ptr()]
            continue
        scale = BIAS_GAIN if name.endswith("bias") else GAIN
        g = torch.Generator().manual_seed(seed * 1000 + k)
        v = torch.randn(t.shape, generator=g) * scale
        sd[name] = v
        rec[name] = [list(t.shape), float("%.9g" % v.double().sum())]
        seen[t.data_ptr()] = name
    return sd, rec


def run(net, x, inverse):
    for p in net.parameters():
        p.grad = None
    xi = x.clone().requires_grad_()
    out = net(xi, inverse=True) if inverse else net(xi)
    loss = (out * out).mean()
    loss.backward()
    grads = []
    for k, (n, p) in enumerate(net.named_parameters()):
        if p.grad is None:          # (the other direction's layers)
            grads.append(None)
            continue
        g = torch.Generator().manual_seed(SEED * 7 + k)
        idx = torch.randint(0, p.numel(), (min(SAMPLES, p.numel()),), generator=g)
        grads.append({"norm": float("%.9g" % p.grad.double().norm()), "idx": idx.tolist(), "values": f32(p.grad.flatten()[idx])})
    g = torch.Generator().manual_seed(SEED * 11)
    idx = torch.randint(0, xi.numel(), (32,), generator=g)
    gin = {"norm": float(xi.grad.double().norm()), "idx": idx.tolist(), "values": f32(xi.grad.flatten()[idx])}
    q = torch.round(out.detach().double().flatten() / OUTPUT_SCALE).long().tolist()
    return {"output_q": q, "output_scale": OUTPUT_SCALE, "loss": float(loss.detach()), "input_grad": gin, "param_grads": grads}


def case(use_inverse):
    net = Vnet3D(1, 1, "instance", first_layer_channels=8, down_blocks=(1, 1), up_blocks=(1, 1), use_memory_saving=False,
                 use_inverse=use_inverse, is_separable=True)
    sd, rec = seeded(net, SEED)
    net.load_state_dict(sd)
    g = torch.Generator().manual_seed(SEED)
    x = torch.rand(SHAPE, generator=g) * 2 - 1
    assert [n for n, _ in net.named_parameters()] == [n for n, r in rec.items() if not isinstance(r, str)]
    c = {"use_inverse": use_inverse, "weight_seed": SEED, "input_seed": SEED, "input_shape": list(SHAPE), "weights": rec, "forward": run(net, x, False)}
    if use_inverse:
        c["inverse"] = run(net, x, True)
    return c


def main():
    torch.set_num_threads(1)
    torch.manual_seed(0)
    out = {"plain": case(False), "inverse": case(True)}
    path = ROOT / "tests" / "golden" / "separable.json"
    path.write_text(json.dumps(out, separators=(",", ":")))
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
