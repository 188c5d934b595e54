"""Oracle of the logged image grid: the reference's op sequence on the CPU, step by step in fp32
(ganslate/utils/trackers/utils.py process_visuals_for_logging, then torchvision.utils.save_image):
channel repeat, `cat` along the width, `permute` + `cat` of the slices along the height, `(x + 1) / 2`,
`mul(255).add(0.5).clamp(0, 255)`, truncation to uint8, HWC with gray replicated to three channels. Shared by the grid,
tracker and engine tests; comparisons against it are bit for bit."""
import numpy as np
import torch


def split_visuals(visuals, multi_modality_split=None):
    """`_split_multimodal_visuals` with torch.split (copies), after the `None` entries are dropped"""
    visuals = {k: v for k, v in visuals.items() if v is not None}
    if multi_modality_split is None:
        return visuals
    out = {}
    for name, t in visuals.items():
        if "_A" in name or "_B" in name:
            for domain in multi_modality_split:
                if name.endswith(domain):
                    split = multi_modality_split[domain]
                    if split is None:
                        out[name] = t
                        continue
                    if sum(split) != t.shape[1]:
                        raise ValueError("Please specify channel-split correctly!")
                    for i, part in enumerate(torch.split(t, tuple(split), dim=1)):
                        out[f"{name}{i + 1}"] = part
        else:
            out[name] = t
    return out


def to_bytes(image):
    """torchvision.utils.save_image on one CxHxW image in [0, 1]: the HWC uint8 array handed to PIL. The float -> uint8
    cast of a value outside [0, 255] does not occur after the clamp; a NaN is defined as 0 here as in the kernel."""
    t = image.mul(255).add(0.5).clamp(0, 255)
    t = torch.where(torch.isnan(t), torch.zeros_like(t), t)
    t = t.permute(1, 2, 0).to(torch.uint8)
    if t.shape[2] == 1:                      # PIL writes a gray grid of make_grid as three equal channels
        t = t.expand(-1, -1, 3)
    return t.contiguous()


def grid_ref(visuals, single_example=False, mid_slice_only=False, multi_modality_split=None):
    """(name, uint8 [n, Hout, Wout, 3] CPU tensor) of {name: fp32 tensor [N, C, H, W] or [N, C, D, H, W]}"""
    visuals = {k: v.detach().float().cpu() for k, v in split_visuals(visuals, multi_modality_split).items()}
    most = max(v.shape[1] for v in visuals.values())
    tensors = []
    for v in visuals.values():                # _make_all_visuals_channels_equal
        assert v.shape[1] in (1, 3)
        tensors.append(torch.repeat_interleave(v, most // v.shape[1], dim=1) if v.shape[1] < most else v)
    three_d = tensors[0].ndim == 5
    batch = torch.cat(tuple(tensors), dim=4 if three_d else 3)
    if single_example:
        batch = batch[:1]
    images = []
    for grid in batch:
        if three_d:
            grid = grid.permute(1, 0, 2, 3)
            grid = grid[grid.shape[0] // 2] if mid_slice_only else torch.cat(tuple(grid), dim=1)
        grid = (grid + 1) / 2
        images.append(to_bytes(grid))
    return "-".join(visuals.keys()), torch.stack(images)


def threshold_values(seed=0, extra=257):
    """The fp32 values at which a byte changes: for k = 1..255, x_k = float32(2 (k - 1/2) / 255 - 1) and every fp32 value
    from 8 ulp below it to 8 ulp above it (4335 values), then -0.0, +-1, +-1.5, +-inf and a seeded randn."""
    x = (2 * (np.arange(1, 256, dtype=np.float64) - 0.5) / 255 - 1).astype(np.float32)
    bits = x.view(np.int32).astype(np.int64)
    # the sign-magnitude integer of a float orders the floats: step in that order
    order = np.where(bits < 0, -(bits & 0x7FFFFFFF), bits)
    steps = (order[:, None] + np.arange(-8, 9)[None, :]).reshape(-1)
    back = np.where(steps < 0, (-steps) | 0x80000000, steps).astype(np.uint32).view(np.float32)
    assert back.size == 4335
    special = np.array([-0.0, 1.0, -1.0, 1.5, -1.5, np.inf, -np.inf], dtype=np.float32)
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.from_numpy(back.copy()), torch.from_numpy(special), torch.randn(extra, generator=g)])


def tiled(shape, offset=0, seed=0):
    """an fp32 tensor of `shape` that walks through threshold_values from `offset` on, wrapping round"""
    v = threshold_values(seed)
    n = int(np.prod(shape))
    idx = (torch.arange(n) + offset) % v.numel()
    return v[idx].reshape(shape).clone()
