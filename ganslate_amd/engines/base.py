"""Engine bases (ganslate/engines/base.py:11-50): `BaseEngineWithInference.infer` sends a batch through the model's
generator — patch-wise through the MONAI-free sliding-window inferer when `<mode>.sliding_window` is configured
(window_size / batch_size / overlap / mode, padding value -1 like the reference, base.py:41-50).
`save_generated_tensor` hands every generated sample to the dataset's own `save()` where it has one (base.py:52-87).
`input_pipeline` is this backend's device-side input path (`<mode>.dataset.device_transforms`, data/device_transforms.py) for
the engines that only run a forward pass: one pipeline per loader, applied to every batch in front of everything that
reads it."""
import copy
import logging
from abc import ABC, abstractmethod
from pathlib import Path

from ..utils import sliding_window_inferer
from ..utils.io import decollate


class BaseEngine(ABC):

    def __init__(self, conf):
        self.conf = copy.deepcopy(conf)          # isolates this engine's conf.mode from the caller's
        self._set_mode()
        self.output_dir = Path(conf[conf.mode].output_dir) / self.conf.mode
        self.model = None
        self.logger = logging.getLogger("ganslate_amd")

    @abstractmethod
    def _set_mode(self):
        """sets self.conf.mode ('train', 'val', ...)"""


class BaseEngineWithInference(BaseEngine):

    def __init__(self, conf):
        super().__init__(conf)
        self.sliding_window_inferer = self._init_sliding_window_inferer()
        self._input_pipelines = {}

    def infer(self, data, *args, **kwargs):
        data = data.to(self.model.device)
        if self.sliding_window_inferer:
            return self.sliding_window_inferer(data, self.model.infer, *args, **kwargs)
        return self.model.infer(data, *args, **kwargs)

    def input_pipeline(self, loader):
        """callable(raw batch) -> batch of device tensors for a loader whose dataset hands over undecoded work
        (`device_transforms: true`), built once per loader from the dataset's own `device_pipeline`; None for a dataset on
        the host path. Entries that are not raw images (`masks`, `metadata`) pass through the pipeline untouched."""
        if loader not in self._input_pipelines:
            self._input_pipelines[loader] = self._make_input_pipeline(loader.dataset)
        return self._input_pipelines[loader]

    def _make_input_pipeline(self, dataset):
        from ..data.multimodal_volumes import MultiModalVolumeDataset
        from ..data.volume_datasets import UnpairedVolumeDataset
        # where each dataset keeps the switch: the image folders in their transform, the volume folder on itself
        places = ((getattr(dataset, "transform", None), "raw"), (dataset, "raw"), (getattr(dataset, "conf", None), "device_transforms"),
                  (dataset, "device_transforms"))
        flag = any(getattr(owner, name, False) is True for owner, name in places)
        make = getattr(dataset, "device_pipeline", None)
        if flag and (make is None or isinstance(dataset, (UnpairedVolumeDataset, MultiModalVolumeDataset))):
            # the volume datasets' device paths hold training patches, not whole volumes
            raise NotImplementedError(f"{self.conf.mode} datasets run the host transform path: set "
                                      f"`{self.conf.mode}.dataset.device_transforms: false` (the device-side "
                                      "pipeline batches training samples only)")
        return make(self.conf, self.model.device) if make else None

    def _init_sliding_window_inferer(self):
        sw = self.conf[self.conf.mode].sliding_window
        if not sw:
            return None
        return sliding_window_inferer.SlidingWindowInferer(roi_size=list(sw.window_size), sw_batch_size=sw.batch_size,
                                                           overlap=sw.overlap, mode=sw.mode, cval=-1)

    def save_generated_tensor(self, generated_tensor, metadata, data_loader, idx=None, dataset_name=None):
        """A dataset that wants the outputs stored in its own way or format defines `save(tensor, save_dir[, metadata])`;
        it is called once per sample of the batch with `save_dir = <output_dir>/saved/[{dataset_name}/][{idx}/]` and that
        sample's share of the collated `metadata` (left out when the batch carries none)."""
        save_fn = getattr(data_loader.dataset, "save", None)
        if not save_fn:
            return
        save_dir = self.output_dir / "saved"
        if dataset_name is not None:
            save_dir = save_dir / f"{dataset_name}"
        if idx is not None:
            save_dir = save_dir / f"{idx}"
        if metadata:
            metadata = decollate(metadata, batch_size=len(generated_tensor))
        for i in range(len(generated_tensor)):
            if metadata:
                save_fn(tensor=generated_tensor[i], save_dir=save_dir, metadata=metadata[i])
            else:
                save_fn(tensor=generated_tensor[i], save_dir=save_dir)
