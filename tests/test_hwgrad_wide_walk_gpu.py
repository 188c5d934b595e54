"""hwgrad_wide_kernel's box walk, element by element: the weight gradient of the 3x3 residual convs on the geometries at
which the double-buffered walk takes a different path — two and three boxes per workgroup (both parities of the staging
buffer, a last box without a successor in either buffer), boxes that hang over the image edge, the second operand pair
beginning in the middle of a workgroup's walk, twin batches, and one box per workgroup (nothing staged under the MFMAs).
The two wave groups of a workgroup stage their shares of the next box at different moments of the current one; a piece
staged into the wrong buffer, too early or never shows up here as a wrong element.

Every case runs twice, for every element of dW against a float64 sum written out below (no code shared with the oracle):
  * integer-valued bf16 operands: exact equality. Products of small integers and their sums below 2^24 are exact in fp32 in
    any order, and the test checks that bound on the magnitudes before it compares;
  * random operands: rel 2e-3 of the reference's max-abs, tests/test_ops_gpu.py's tolerance for fp32 weight gradients.
The slab count of each launch is read back from the plan-only query and the boxes per workgroup are derived from it, so a
retuned grid fails the geometry assertion instead of silently leaving the branch.
"""
import ctypes as C

import pytest
import torch

from ganslate_amd.nn.native.spec import ConvSpec, lower
from ganslate_amd.nn.native.twin import Twin
from tests import exact
from tests.test_ops_gpu import close_f32

pytestmark = pytest.mark.gpu

# name: (channels, images per network, H, W, pair, twin, boxes per workgroup the case is about)
WALK = {
    "boxes-2-and-3": (256, 1, 96, 96, False, False, {2, 3}),       # 36 boxes on 16 workgroups
    "ragged-88x104": (256, 1, 88, 104, False, False, {2, 3}),      # 6 x 7 boxes, the last row / column half outside
    "pair-64x64": (256, 1, 64, 64, True, False, {2}),              # box 0 from the first pair, box 1 from the second
    "twin-64x64": (256, 1, 64, 64, False, True, {2}),              # 8 workgroups per network
    "twin-pair-64x64": (256, 1, 64, 64, True, True, {4}),
    "floor-4-boxes": (64, 1, 32, 32, False, False, {1}),           # P = Q = 64, 4 boxes: one per workgroup
}


def _border(i, n, mode):
    """source index and validity of position i on an axis of n (oracle-independent restatement of the border rules)"""
    ok = (i >= 0) & (i < n)
    if mode == "reflect":
        j = torch.where(i < 0, -i, torch.where(i >= n, 2 * (n - 1) - i, i))
        return j, torch.ones_like(ok)
    return i.clamp(0, n - 1), ok


def ref64(w, a, g):
    """dW[p][t][q] = sum over images and pixels of a[pix][p] * g[B(pix + off_t)][q] in float64; a, g channels-last [N, H, W, C]"""
    a64, g64 = a.double(), g.double()
    out = torch.zeros(w.P, w.T, w.Q, dtype=torch.float64)
    ii, jj = torch.arange(w.Ha), torch.arange(w.Wa)
    for t in range(w.T):
        ih, okh = _border(ii + w.dh[t], w.Hg, w.border)
        iw, okw = _border(jj + w.dw[t], w.Wg, w.border)
        patch = g64[:, ih][:, :, iw] * (okh[:, None] & okw[None, :]).double()[None, :, :, None]
        out[:, t, :] = torch.einsum("nijp,nijq->pq", a64, patch)
    return out


def _operands(kind, shape, gen):
    if kind == "integer":
        return exact.int_act(shape[0], shape[1:3], shape[3], shape[3], gen, 0.25, 3)
    return torch.randn(*shape, generator=gen).to(torch.bfloat16)


def _slabs(ops, w, N, C_, pair, twin):
    """slabs per network of the launch, from the plan-only query"""
    d = ops._wdesc(w, N, C_, 0, C_, 0)
    if twin:
        assert ops.lib.gs_wgrad_twin_native(C.byref(d), int(pair)), "the layer has no twin launch"
        floats = int(ops.lib.gs_wgrad_ws_floats_twin(C.byref(d), int(pair))) // 2
    else:
        floats = int(ops.lib.gs_wgrad_ws_floats(C.byref(d), int(pair)))
    assert floats > 0 and floats % (w.P * w.T * w.Q) == 0
    return floats // (w.P * w.T * w.Q)


@pytest.mark.parametrize("kind", ["integer", "random"])
@pytest.mark.parametrize("border", ["reflect", "zero"])
@pytest.mark.parametrize("name", list(WALK))
def test_wide_halo_weight_gradient_walk(hip_ops, name, border, kind):
    Cc, n_net, H, W, pair, twin, walks = WALK[name]
    dev = hip_ops.device
    spec = ConvSpec("conv", Cc, Cc, 3, 1, 1, pad_mode=border)
    w = lower(spec, H, W).wgrad
    assert w.border == border and w.T == 9 and w.si == 1 and w.P == Cc and w.Q == Cc
    nets = 2 if twin else 1
    N = nets * n_net

    # geometry: the launch is the wide kernel's (one workgroup per CU and (p, q) block), walking the boxes the case is about
    slabs = _slabs(hip_ops, w, N, Cc, pair, twin)
    boxes = n_net * ((H + 15) // 16) * ((W + 15) // 16) * (2 if pair else 1)       # per network
    assert slabs == min(256 // ((Cc // 64) ** 2 * nets), boxes), f"{slabs} slabs per network: not the wide kernel's grid"
    assert {len(range(g, boxes, slabs)) for g in range(slabs)} == walks, "the boxes per workgroup moved off this case's branch"

    gen = torch.Generator().manual_seed(sum(map(ord, name + border + kind)))
    mk = lambda: _operands(kind, (N, H, W, Cc), gen)
    a, g = mk(), mk()                                   # dense side (output gradient), gathered side (input)
    a2, g2 = (mk(), mk()) if pair else (None, None)
    half = lambda t, h: t[h * n_net:(h + 1) * n_net]
    ref = torch.stack([ref64(w, half(a, h), half(g, h)) + (ref64(w, half(a2, h), half(g2, h)) if pair else 0)
                       for h in range(nets)])
    if kind == "integer":       # every partial sum of every order is an integer below 2^24: bounded by the sum of magnitudes
        bound = max((ref64(w, half(x, h).abs(), half(y, h).abs()).max().item()
                     for h in range(nets) for x, y in ((a, g),) + (((a2, g2),) if pair else ())))
        assert (2 if pair else 1) * bound < 2 ** 24

    dw = torch.zeros(nets, w.P * w.T * w.Q, device=dev)
    pr = (a2.to(dev), g2.to(dev)) if pair else None
    hip_ops.wgrad(w, a.to(dev), g.to(dev), Twin(dw[0], dw[1]) if twin else dw[0], pair=pr)
    torch.cuda.synchronize()
    got = dw.cpu().view(nets, w.P, w.T, w.Q)
    for h in range(nets):
        what = f"{name}, {border} border, {kind} data, network {h}: dW [P][T][Q]"
        if kind == "integer":
            exact.assert_identical(got[h], ref[h].float(), what)
        else:
            close_f32(got[h], ref[h], what, rel=2e-3)
