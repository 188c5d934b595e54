"""Device-side training-patch pipeline of the 3-D volume datasets: volumes resident in HBM, per
iteration only patch coordinates arrive from the loader (data/volume_datasets.py RawPatch), crop + z-score + range
scaling run as gs_patch_zscore (csrc/volproc.hip) and write straight into the fp32 [N, 1, d, h, w] batch `set_input`
takes. Reference path being replaced: projects/brats_mri_sequence_translation/datasets/train_dataset.py:83-92.
With `augmentation` a sample also carries a 3 x 3 matrix: gs_patch_affine (csrc/volsample.hip) gathers the patch through
it into a scratch patch, and gs_patch_zscore normalises that as a volume of its own. A sample that also carries an elastic
field takes gs_patch_elastic there; the fields of a batch are uploaded in one copy. A sample whose intensity row is not
neutral (data/utils/patch_intensity.py) takes gs_patch_zscore_intensity in place of gs_patch_zscore; the bias lattices of a
batch are one more copy."""
import numpy as np
import torch

from .resident_cache import ResidentCache
from .utils.patch_intensity import active


class ResidentVolumes(ResidentCache):
    """the resident volumes and masks of one dataset, as the kernels take them: a mask as uint8 0 / 1, a volume as fp32 or
    int16"""

    def __init__(self, dataset, device, ops=None, max_resident_bytes=200 << 30):
        super().__init__(device, ops, max_resident_bytes)
        self.dataset = dataset

    def _host(self, name, index):
        return torch.from_numpy(np.array(self.dataset.load(name, index)))           # a copy out of the memory map

    def volume(self, name, index, mask=False):
        def upload():
            host = self._host(name, index)
            if mask:
                host = (host != 0).to(torch.uint8)
            elif host.dtype not in (torch.float32, torch.int16):
                host = host.float()
            return host.to(self.device)

        return self._get((name, index), upload)


def upload_fields(items, device):
    """{id(field): float64 device tensor [3, G0, G1, G2]} of every elastic field the raw samples carry: one host array, one
    copy. A field shared by two samples (a paired one) travels once."""
    fields = {}
    for r in items:
        if getattr(r, "field", None) is not None:
            fields.setdefault(id(r.field), r.field)
    if not fields:
        return {}
    dev = torch.from_numpy(np.stack([np.asarray(f, dtype=np.float64) for f in fields.values()])).to(device)
    return {key: dev[n] for n, key in enumerate(fields)}


def upload_bias(items, device):
    """{id(lattice): float64 device tensor [G0, G1, G2]} of the bias lattices of the samples whose intensity block is
    active (data/utils/patch_intensity.py): like the elastic fields, one host array and one copy per batch"""
    lattices = {}
    for r in items:
        block = active(getattr(r, "intensity", None))
        if block is not None and block[1] is not None:
            lattices.setdefault(id(block[1]), block[1])
    if not lattices:
        return {}
    dev = torch.from_numpy(np.stack([np.asarray(b, dtype=np.float64) for b in lattices.values()])).to(device)
    return {key: dev[n] for n, key in enumerate(lattices)}


class DeviceVolumePipeline(ResidentVolumes):
    """callable(raw batch) -> {"A": fp32 [N, 1, *patch] on the device, "B": ...}"""

    def __init__(self, dataset, device, ops=None, max_resident_bytes=200 << 30):
        super().__init__(dataset, device, ops, max_resident_bytes)
        self.size = [int(v) for v in dataset.patch_sampler.patch_size]       # (d, h, w); d = 1 for 2-D patch sizes
        self.squeeze = dataset.patch_sampler.dims == 2

    def _host(self, domain, index):
        return self.dataset.load(domain, index)              # torch tensors, keyed by domain

    def __call__(self, batch):
        from .volume_datasets import RawPatch
        out = {}
        raws = [r for items in batch.values() if items and isinstance(items[0], RawPatch) for r in items]
        fields, lattices = upload_fields(raws, self.device), upload_bias(raws, self.device)
        for key, items in batch.items():
            if not items or not isinstance(items[0], RawPatch):
                out[key] = items
                continue
            dst = torch.empty((len(items), 1, *self.size), dtype=torch.float32, device=self.device)
            for n, r in enumerate(items):
                if r.matrix is None:
                    self.ops.patch_zscore(self.volume(r.domain, r.index), r.start, self.size, dst[n, 0], (-1.0, 1.0))
                    continue
                # augmented: the raw gather into a dense patch, which patch_zscore then takes as a volume of its own
                raw = torch.empty(tuple(self.size), dtype=torch.float32, device=self.device)
                if r.field is not None:
                    self.ops.patch_elastic(self.volume(r.domain, r.index), r.start, self.size, r.matrix, fields[id(r.field)],
                                           self.dataset.augmentation.fill, raw)
                else:
                    self.ops.patch_affine(self.volume(r.domain, r.index), r.start, self.size, r.matrix,
                                          self.dataset.augmentation.fill, raw)
                block = active(r.intensity)
                if block is None:           # none, or its one row came out neutral: the plain z-score
                    self.ops.patch_zscore(raw, (0, 0, 0), self.size, dst[n, 0], (-1.0, 1.0))
                else:
                    self.ops.patch_zscore_intensity(raw, (0, 0, 0), self.size, dst[n, 0], block[0][0],
                                                    None if block[1] is None else lattices[id(block[1])], (-1.0, 1.0))
            out[key] = dst.squeeze(2) if self.squeeze else dst
        return out


class DeviceMultiModalPipeline(ResidentVolumes):
    """callable(raw batch) -> {"A": fp32 [N, C_A, *patch] on the device, "B": fp32 [N, C_B, *patch]} for
    MultiModalVolumeDataset (data/multimodal_volumes.py): volumes and body masks resident in HBM, per iteration only case
    indices and uniforms arrive. Per sample: one gs_voxel_draw per domain when unpaired (B's reads A's point from device
    memory), one in total when paired, and one gs_patch_clip_minmax per domain writing all of its modalities straight into
    the batch (csrc/volsample.hip). Nothing synchronises per iteration; the empty-zone check of a case runs once, when its
    mask is first uploaded. A sample that carries an augmentation matrix takes gs_patch_affine_clip_minmax instead: the
    same crop as one trilinear gather through the matrix (data/utils/patch_affine.py), and one that also carries an elastic
    field gs_patch_elastic_clip_minmax (the fields of a batch are uploaded in one copy); a domain whose intensity block is
    not neutral takes gs_patch_augment_clip_minmax, the same gather with the intensity chain inside. Reference path being replaced: projects/maastro_hx4_pet_translation/datasets/
    train_dataset.py:106-188 with datasets/utils/patch_samplers.py."""

    def __init__(self, dataset, device, ops=None, max_resident_bytes=200 << 30):
        super().__init__(dataset, device, ops, max_resident_bytes)
        self.size = [int(v) for v in dataset.patch_size]
        self.checked = set()
        self.points = None          # int32 [N, 2, 4] of the last batch: (z, y, x, fallback_used) per sample and domain

    def case(self, domain, index):
        """(mask, weight or None, [volumes]) of one case of a domain; on first use the count of the kernel's own draw tells
        whether the case can be sampled at all — one .item() per case, never per iteration"""
        ds = self.dataset
        mask = self.volume(ds.body_mask[domain], index, mask=True)
        weight = self.volume(ds.weight_modality, index) if domain == "A" and ds.weight_modality else None
        if (domain, index) not in self.checked and (domain == "A" or not ds.paired):
            probe = torch.empty(4, dtype=torch.int32, device=self.device)
            self.ops.voxel_draw(mask, weight, self.size, 0.0, probe)
            if int(probe[0].item()) < 0:
                raise ds.empty_zone_error(domain, index)
            self.checked.add((domain, index))
        return mask, weight, [self.volume(n, index) for n in ds.modalities[domain]]

    def _patch(self, domain, index, vols, mask, point, dst, matrix=None, field=None, intensity=None, lattice=None):
        ds = self.dataset
        names = ds.modalities[domain]
        cols = ([ds.outside_value[n] for n in names], [ds.divisor(n, index) for n in names],
                [ds.clip_range[n][0] for n in names], [ds.clip_range[n][1] for n in names])
        if intensity is not None:           # (rows, _) of an active block; lattice: its bias lattice on the device
            self.ops.patch_augment_clip_minmax(vols, mask, point, self.size, matrix, field, intensity[0], lattice, *cols, dst)
        elif matrix is None:
            self.ops.patch_clip_minmax(vols, mask, point, self.size, *cols, dst)
        elif field is not None:
            self.ops.patch_elastic_clip_minmax(vols, mask, point, self.size, matrix, field, *cols, dst)
        else:
            self.ops.patch_affine_clip_minmax(vols, mask, point, self.size, matrix, *cols, dst)

    def __call__(self, batch):
        from .multimodal_volumes import RawCase
        items_A, items_B = batch.get("A"), batch.get("B")
        if not items_A or not isinstance(items_A[0], RawCase):
            return batch
        ds, n = self.dataset, len(items_A)
        out = {k: v for k, v in batch.items() if k not in ("A", "B")}
        dst = {k: torch.empty((n, len(ds.modalities[k]), *self.size), dtype=torch.float32, device=self.device) for k in "AB"}
        points = torch.empty((n, 2, 4), dtype=torch.int32, device=self.device)
        fields = upload_fields(list(items_A) + list(items_B), self.device)
        lattices = upload_bias(list(items_A) + list(items_B), self.device)
        field_of = lambda r: None if r.field is None else fields[id(r.field)]

        def aug_of(r):
            block = active(r.intensity)
            lattice = None if block is None or block[1] is None else lattices[id(block[1])]
            return r.matrix, field_of(r), block, lattice
        for i, (a, b) in enumerate(zip(items_A, items_B)):
            mask_A, weight, vols_A = self.case("A", a.index)
            self.ops.voxel_draw(mask_A, weight, self.size, a.u, points[i, 0])
            self._patch("A", a.index, vols_A, mask_A, points[i, 0], dst["A"][i], *aug_of(a))
            if ds.paired:                                   # the same point, A's mask and A's case
                points[i, 1].copy_(points[i, 0])
                self._patch("B", a.index, [self.volume(m, a.index) for m in ds.modalities["B"]], mask_A, points[i, 0],
                            dst["B"][i], *aug_of(b))
            else:
                mask_B, _, vols_B = self.case("B", b.index)
                self.ops.voxel_draw(mask_B, None, self.size, b.u, points[i, 1], focal_A=points[i, 0],
                                    dims_A=tuple(mask_A.shape), proportion=ds.focal_region_proportion)
                self._patch("B", b.index, vols_B, mask_B, points[i, 1], dst["B"][i], *aug_of(b))
        self.points = points
        out.update(dst)
        return out


class DeviceWholeVolumePipeline(ResidentVolumes):
    """callable(raw batch) -> {"A": fp32 [N, C_A, Do, Ho, Wo] on the device, "B": fp32 [N, before + C_B + after, ...],
    "masks": {label: uint8 [N, 1, Do, Ho, Wo] on the device}, "metadata": as it came} for MultiModalVolumeValTestDataset
    (data/multimodal_valtest.py): raw volumes and masks resident in HBM under the same `max_resident_bytes` rule as the
    training pipelines, per batch only case indices arrive. A case whose body mask is generated gets it from gs_body_mask
    (csrc/bodymask.hip) once — the mask stays resident, and that one call reads the component's voxel count back, so a CT
    without a body raises for the case by name. Per case and use one gs_volume_prepare call (csrc/volsample.hip) masks,
    pads and normalises all modalities of both domains and pads every mask; one strided copy then splits its channels into
    A's and B's batch tensors. Reference path being replaced: projects/maastro_hx4_pet_translation/datasets/
    val_test_dataset.py:86-187 with ganslate/data/utils/body_mask.py."""

    def __init__(self, dataset, device, ops=None, max_resident_bytes=200 << 30):
        super().__init__(dataset, device, ops, max_resident_bytes)

    def body(self, index):
        ds = self.dataset
        if not ds.generates(index):
            return self.volume(ds.body_mask, index, mask=True)

        def generate():
            v, info = self.ops.body_mask(self.volume(ds.body_mask_from, index), ds.body_mask_threshold)
            if int(info[0].item()) == 0:
                raise ds.empty_body_error(index)
            return v

        return self._get((None, index), generate)            # no file has this name

    def __call__(self, batch):
        from .multimodal_valtest import RawWholeCase
        items = batch.get("A")
        if not items or not isinstance(items[0], RawWholeCase):
            return batch
        ds = self.dataset
        domains = ds.domains()
        names = [n for k in domains for n in ds.modalities[k]]
        labels = ds.mask_labels()
        out = {k: v for k, v in batch.items() if k not in ("A", "B")}
        both, masks = None, None
        for i, item in enumerate(items):
            index = item.index
            body = self.body(index)
            extra = [body if ds.masks[label] == ds.body_mask else self.volume(ds.masks[label], index, mask=True)
                     for label in labels]
            shape = tuple(max(s, t) for s, t in zip(body.shape, ds.pad_to or body.shape))
            if both is None:
                both = torch.empty((len(items), len(names), *shape), dtype=torch.float32, device=self.device)
                masks = torch.empty((1 + len(labels), len(items), 1, *shape), dtype=torch.uint8, device=self.device)
            elif tuple(both.shape[2:]) != shape:
                raise ValueError(f"the cases of one batch come out in different shapes ({tuple(both.shape[2:])} and {shape} "
                                 f"for {ds.cases[index]!r}): set `pad_to` to a common shape or use `batch_size: 1`")
            self.ops.volume_prepare([self.volume(n, index) for n in names], body, extra, shape,
                                    [ds.outside_value[n] for n in names], [ds.divisor(n, index) for n in names],
                                    [ds.clip_range[n][0] for n in names], [ds.clip_range[n][1] for n in names],
                                    out=both[i], masks_out=[masks[m, i, 0] for m in range(1 + len(labels))])
        n_A = len(ds.modalities["A"])
        out["A"] = both[:, :n_A].contiguous() if len(names) > n_A else both
        if "B" in domains:
            before, after = ds.dummy_channels_B
            B = torch.zeros((len(items), before + len(names) - n_A + after, *both.shape[2:]), dtype=torch.float32,
                            device=self.device) if before or after else None
            if B is None:
                B = both[:, n_A:].contiguous()
            else:
                B[:, before:before + len(names) - n_A].copy_(both[:, n_A:])
            out["B"] = B
        if labels:
            out["masks"] = {label: masks[1 + m] for m, label in enumerate(labels)}
        return out
