"""ORACLE for `is_separable=True` (test infrastructure only): ganslate/nn/separable.py:5-78 restated in plain torch, and the
network-level oracle of oracle/torch_ref.py built with those layers in place of Conv3d / ConvTranspose3d
(ganslate/nn/utils.py:39-50 picks them the same way). Pinned against the imported reference by tests/golden/separable.json
(tools/gen_golden_separable.py) in tests/test_separable_cpu.py."""
import contextlib
import json
import os

import torch
from torch import nn

from oracle import torch_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "separable.json")


class SeparableConv3d(nn.Module):
    """(1,k,k) conv cin -> cout, then (k,1,1) conv cout -> cout; neither grouped, nothing in between"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        k, s, p = kernel_size, stride, padding
        self.conv_depthwise = nn.Conv3d(in_channels, out_channels, (1, k, k), (1, s, s), (0, p, p), bias=bias)
        self.conv_pointwise = nn.Conv3d(out_channels, out_channels, (k, 1, 1), (s, 1, 1), (p, 0, 0), bias=bias)

    def forward(self, x):
        return self.conv_pointwise(self.conv_depthwise(x))


class SeparableConvTranspose3d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        k, s, p = kernel_size, stride, padding
        self.conv_transp_depthwise = nn.ConvTranspose3d(in_channels, out_channels, (1, k, k), (1, s, s), (0, p, p), bias=bias)
        self.conv_transp_pointwise = nn.ConvTranspose3d(out_channels, out_channels, (k, 1, 1), (s, 1, 1), (p, 0, 0), bias=bias)

    def forward(self, x):
        return self.conv_transp_pointwise(self.conv_transp_depthwise(x))


@contextlib.contextmanager
def _separable_layers():
    """torch_ref's V-Net blocks ask _vconv for their layer classes while they are constructed"""
    plain = torch_ref._vconv

    def vconv(dims):
        assert dims == 3, "separable layers exist for volumes"
        return SeparableConv3d, SeparableConvTranspose3d, nn.InstanceNorm3d

    torch_ref._vconv = vconv
    try:
        yield
    finally:
        torch_ref._vconv = plain


def vnet3d(*args, **kwargs):
    with _separable_layers():
        return torch_ref.Vnet3D(*args, **kwargs)


def selfattention_vnet3d(*args, **kwargs):
    with _separable_layers():
        return torch_ref.SelfAttentionVnet3D(*args, **kwargs)


_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)
    return _golden


def golden_state_dict(case):
    """the golden's weights by state-dict key: entry k is the draw torch.Generator(weight_seed * 1000 + k), N(0, 1) times 0.01
    for a bias and 0.02 otherwise (oracle.torch_ref.seeded_state_dict), checked against the recorded shape's sum; "=<key>" is
    a second name of that key's tensor"""
    sd = {}
    for k, (name, v) in enumerate(case["weights"].items()):
        if isinstance(v, str):
            sd[name] = sd[v[1:]]
            continue
        shape, total = v
        g = torch.Generator().manual_seed(case["weight_seed"] * 1000 + k)
        t = torch.randn(shape, generator=g) * (0.01 if name.endswith("bias") else 0.02)
        assert abs(float(t.double().sum()) - total) <= 1e-6 * max(1.0, abs(total)), name
        sd[name] = t
    return sd


def parameter_keys(case):
    """state-dict keys that are not second names: the reference's parameters, in the order torch yields them"""
    return [k for k, v in case["weights"].items() if not isinstance(v, str)]


def weight_shapes(case):
    w = case["weights"]
    return {k: (w[v[1:]] if isinstance(v, str) else v)[0] for k, v in w.items()}


def param_grads(case, rec):
    """the recorded gradients of one run by parameter key (parameters the run left without gradient are absent)"""
    return {k: g for k, g in zip(parameter_keys(case), rec["param_grads"]) if g is not None}


def golden_output(rec):
    """the recorded output: integers in units of output_scale"""
    return torch.tensor(rec["output_q"], dtype=torch.float64).mul(rec["output_scale"]).float()


def golden_input(case):
    g = torch.Generator().manual_seed(case["input_seed"])
    return torch.rand(case["input_shape"], generator=g) * 2 - 1
