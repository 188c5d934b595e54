"""The image side of the reference's trackers (ganslate/utils/trackers/{base,training,validation_testing,inference}.py):
`<[mode].output_dir>/<mode>/images/*.png` and `<mode>_config.yaml`. The grid of a set of visuals is composed on the GPU
by one kernel (HipOps.visuals_grid, visgrid.hip) as finished HWC bytes; one device -> host copy of those bytes follows, and
`PIL.Image.fromarray(grid).save(path)` on rank 0, which is where torchvision.utils.save_image ends as well. Under DDP the
byte grids are gathered to rank 0 (communication.gather), never fp32 tensors.

File names, relative to `images/` (trackers/base.py:57-62, training.py:62, validation_testing.py:88-100, inference.py:43):
    train   {iter}_{name}.png                       first example of the batch, a volume as all slices stacked
    val     [{dataset}/]{iter}/{idx}_{name}.png     every sample, mid slice
    test    [{dataset}/]{idx}_{name}.png            every sample, mid slice
    infer   {iter_idx + i}_{name}.png               every sample, all slices stacked
W&B, TensorBoard and `image_window` (which only feeds those two) are not part of this build.

A backend without `visuals_grid` (the CPU oracle of the test-suite) composes nothing: `compose` says so once in the log and
returns None, which every `write_*` / `add_samples` accepts."""
import logging
from pathlib import Path

import numpy as np

from . import communication, io
from ..configs.omegalite import OmegaConf


class ImageWriter:

    def __init__(self, conf, ops=None):
        self.conf = conf
        self.mode = conf.mode
        self.output_dir = Path(conf[conf.mode].output_dir) / conf.mode
        self.logger = logging.getLogger("ganslate_amd")
        self._ops = ops
        self._skipped = False
        self._samples = []          # val / test: (name, grid [H, W, 3]) of every sample since the last write_samples
        self._save_config()

    def _save_config(self):
        if communication.get_rank() == 0:
            path = self.output_dir / f"{self.mode}_config.yaml"
            io.mkdirs(path.parent)
            path.write_text(OmegaConf.to_yaml(self.conf))

    # ---- device side ---------------------------------------------------------------------------------------------
    def compose(self, visuals, single_example=False, mid_slice_only=False):
        """(name, uint8 array [n, Hout, Wout, 3]) of an ordered {name: tensor}: one kernel launch on the current stream and
        one copy of the bytes to the host (which waits for the stream). None on a backend without the kernel."""
        if self._ops is None:
            from ..nn.native.backend import get_ops
            self._ops = get_ops()
        if not hasattr(self._ops, "visuals_grid"):
            if not self._skipped:
                self.logger.info(f"backend `{getattr(self._ops, 'name', self._ops)}` has no image-grid kernel; "
                                 f"no {self.mode} images are written")
                self._skipped = True
            return None
        logging_conf = self.conf[self.mode].logging
        split = getattr(logging_conf, "multi_modality_split", None) if logging_conf is not None else None
        # the kernel reads dense fp32: a visual kept in another type or layout is converted first (a no-op otherwise)
        visuals = {k: v.detach().float().contiguous() for k, v in visuals.items() if v is not None}
        name, grid = self._ops.visuals_grid(visuals, single_example=single_example, mid_slice_only=mid_slice_only,
                                            multi_modality_split=split)
        return name, grid.cpu().numpy()

    # ---- host side: ready-made (name, uint8 [n, H, W, 3]) pairs ---------------------------------------------------
    def _save(self, stem, name, image):
        path = self.output_dir / "images" / f"{stem}_{name}.png"
        io.mkdirs(path.parent)
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(image)).save(path)
        return path

    @staticmethod
    def _gathered(named):
        """the (name, grids) pairs of all ranks as one pair on rank 0, samples in rank order; None on the other ranks"""
        if communication.get_world_size() < 2:
            return named
        everyone = communication.gather(named)
        if communication.get_rank() != 0:
            return None
        everyone = [e for e in everyone if e is not None]
        if not everyone:
            return None
        return everyone[0][0], np.concatenate([grids for _, grids in everyone], axis=0)

    def write_train(self, iter_idx, named):
        """`{iter}_{name}.png`: the first example; no gather, each rank's batch would do (training.py:28-33)"""
        if named is None or communication.get_rank() != 0:
            return None
        name, grids = named
        return self._save(f"{iter_idx}", name, grids[0])

    def write_infer(self, iter_idx, named):
        """`{iter_idx + i}_{name}.png` for every sample i of the (gathered) batch (inference.py:40-43)"""
        named = self._gathered(named)
        if named is None or communication.get_rank() != 0:
            return []
        name, grids = named
        return [self._save(f"{iter_idx + i}", name, grid) for i, grid in enumerate(grids)]

    def add_samples(self, named):
        """val / test: keep the (gathered) samples of a batch until write_samples (validation_testing.py:40-50)"""
        named = self._gathered(named)
        if named is None or communication.get_rank() != 0:
            return
        name, grids = named
        self._samples.extend((name, grid) for grid in grids)

    def write_samples(self, iter_idx=None, dataset_name=None):
        """`[{dataset}/][{iter}/ in val, {iter}_ in test]{idx}_{name}.png` for the samples kept since the last call
        (validation_testing.py:88-100), then forgets them"""
        paths = []
        for idx, (name, grid) in enumerate(self._samples):
            stem = f"{dataset_name}/" if dataset_name is not None else ""
            if iter_idx is not None:
                stem += f"{iter_idx}" + ("/" if self.mode == "val" else "_")
            paths.append(self._save(stem + f"{idx}", name, grid))
        self._samples = []
        return paths
