"""CPU references for the batched device image transform (csrc/imgproc.hip gs_u8_batch_*): per image, Pillow's resize as
oracle/pil_ref.py restates it, then crop, flip and torchvision's fp32 ToTensor / Normalize; and the op-level oracle
(oracle/ops_ref.RefOps) on the tables the product uploads, pass by pass. TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

from ganslate_amd.data.device_transforms import resample_tables
from oracle import pil_ref
from oracle.ops_ref import RefOps


def image(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def pillow_batch(images, rh, rw, windows, fh, fw):
    """images: (H, W, C) uint8 arrays; windows: (top, left, flip) per image -> fp32 (n, C, fh, fw)"""
    out = []
    for a, (top, left, flip) in zip(images, windows):
        r = pil_ref.resize_bicubic(a, rh, rw)[top:top + fh, left:left + fw]
        if flip:
            r = r[:, ::-1]
        x = r.astype(np.float32) / np.float32(255.0)
        x = (x - np.float32(0.5)) / np.float32(0.5)
        out.append(torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, -1, 0))))
    return torch.stack(out)


def tables(n_in, n_out):
    b, k = resample_tables(n_in, n_out)
    return torch.from_numpy(b).contiguous(), torch.from_numpy(k).contiguous()


def per_image_batch(ops, images, rh, rw, windows, fh, fw, device="cpu"):
    """the existing per-image entry points (of `ops`: RefOps on the CPU, HipOps on the device) on the product's tables"""
    n, c = len(images), images[0].shape[2]
    out = torch.empty((n, c, fh, fw), dtype=torch.float32, device=device)
    for i, (a, (top, left, flip)) in enumerate(zip(images, windows)):
        h, w = a.shape[:2]
        bh, kh = (t.to(device) for t in tables(w, rw))
        bv, kv = (t.to(device) for t in tables(h, rh))
        tmp = torch.empty((h, rw, c), dtype=torch.uint8, device=device)
        ops.u8_resample_h(torch.from_numpy(a).to(device), tmp, bh, kh)
        ops.u8_resample_v_crop_normalize(tmp, out[i], rh, bv, kv, top, left, flip)
    return out


def oracle_batch(images, rh, rw, windows, fh, fw):
    return per_image_batch(RefOps(), images, rh, rw, windows, fh, fw)


class BatchRefOps(RefOps):
    """RefOps plus a restatement of HipOps.u8_batch_resample on the CPU: the same descriptor table and arena layout
    (HipOps.u8_batch_table), the horizontal pass on the rows [row0, row0 + rows) only, the vertical pass indexed relative
    to row0. Lets the host side of the batched path (DeviceImagePipeline.batch) run without a GPU."""

    def u8_batch_resample(self, items_host, srcs, out, Cc, tmp=None, guard=0):
        from ganslate_amd.hip.ops import HipOps
        table, nbytes = HipOps.u8_batch_table(items_host, srcs, Cc, guard)
        fh, fw = out.shape[2], out.shape[3]
        if tmp is None:
            tmp = torch.empty(nbytes, dtype=torch.uint8)
        for i, (d, it, src) in enumerate(zip(table, items_host, srcs)):
            assert 0 <= it.top and it.top + fh <= it.rh and 0 <= it.left and it.left + fw <= it.rw
            assert 0 <= it.row0 and it.row0 + it.rows <= it.in_h
            (bh, kh), (bv, kv) = it.tables_h, it.tables_v
            part = tmp[d.tmp_off:d.tmp_off + it.rows * it.rw * Cc].view(it.rows, it.rw, Cc)
            self.u8_resample_h(src[it.row0:it.row0 + it.rows], part, bh, kh)
            shifted = bv.clone()
            shifted[:, 0] -= it.row0
            assert int(shifted[it.top:it.top + fh, 0].min()) >= 0
            assert int((shifted[it.top:it.top + fh, 0] + shifted[it.top:it.top + fh, 1]).max()) <= it.rows
            self.u8_resample_v_crop_normalize(part, out[i], it.rh, shifted, kv, it.top, it.left, it.flip)
        return table, tmp
