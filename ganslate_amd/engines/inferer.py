"""Inferer (ganslate/engines/inferer.py:10-79): the generator of checkpoint `infer.checkpointing.load_iter` (BaseGAN.setup)
over the `infer` dataset, patch-wise when `infer.sliding_window` is set. Per batch: `infer` -> the dataset's `save()` for
every output (BaseEngineWithInference.save_generated_tensor, `<infer.output_dir>/infer/saved/`) -> one
`images/{iter_idx + i}_input-output.png` per sample, input and output side by side with a volume's slices stacked
(utils/trackers.py). With `infer.is_deployment` there is no loader and no writer: the owner calls `infer()` itself and
`run()` asserts. Timers are rank-local like the Trainer's; the reference reduces three of them per batch
(trackers/base.py:56,61, inference.py:60)."""
import time
from pathlib import Path

import torch

from ..utils import communication, environment
from ..utils.builders import build_gan, build_loader
from ..utils.trackers import ImageWriter
from .base import BaseEngineWithInference


class Inferer(BaseEngineWithInference):

    def __init__(self, conf):
        super().__init__(conf)
        # under this engine's own `infer.output_dir`; BaseEngine's directory follows the caller's conf, whose mode is "train"
        self.output_dir = Path(self.conf.infer.output_dir) / "infer"
        if not self.conf.infer.is_deployment:
            assert self.conf.infer.dataset, "Please specify the dataset for inference."
            environment.setup_logging()
            self.writer = ImageWriter(self.conf)
            self.data_loader = build_loader(self.conf)
        self.model = build_gan(self.conf)

    def _set_mode(self):
        self.conf.mode = "infer"

    def run(self):
        assert not self.conf.infer.is_deployment, \
            "`Inferer.run()` cannot be used in deployment, please use `Inferer.infer()`."
        self.logger.info("Inference started.")
        batch_size = self.conf.infer.batch_size
        n_samples = len(self.data_loader.dataset)
        input_key = None
        pipeline = self.input_pipeline(self.data_loader)      # `infer.dataset.device_transforms` (data/device_transforms.py)
        t_start = time.perf_counter()
        for i, data in enumerate(self.data_loader):
            if pipeline is not None:
                data = pipeline(data)
            # every process does an iteration of batch_size samples; numbering starts at 1 (inferer.py:39-43)
            iter_idx = i * communication.get_world_size() * batch_size + 1
            if i == 0:
                input_key = self._get_input_key(data)
                if not hasattr(self.data_loader.dataset, "save"):
                    self.logger.warning("The dataset class used does not have a 'save' method. It is not necessary, however, "
                                        "it may be useful in cases where the outputs should be stored individually ('images/' "
                                        "folder saves input and output in a single image), or in a specific format.")
            t_loaded = time.perf_counter()
            out = self.infer(data[input_key])
            if out.is_cuda:
                torch.cuda.synchronize(out.device)
            t_inferred = time.perf_counter()
            self.save_generated_tensor(generated_tensor=out, metadata=data.get("metadata"), data_loader=self.data_loader)
            t_saved = time.perf_counter()
            visuals = {"input": data[input_key].to(out.device), "output": out}
            self.writer.write_infer(iter_idx, self.writer.compose(visuals))
            per = [(b - a) / batch_size for a, b in ((t_start, t_loaded), (t_loaded, t_inferred), (t_inferred, t_saved))]
            self.logger.info(f"{min(iter_idx, n_samples)}/{n_samples} - loading: {per[0]:.2f}s | inference: {per[1]:.2f}s"
                             f" | saving: {per[2]:.2f}s")
            t_start = time.perf_counter()

    def _get_input_key(self, data):
        """the dataset hands the input over under the key 'input' or 'A'"""
        if "input" in data:
            return "input"
        if "A" in data:
            return "A"
        raise ValueError("An inference dataset needs to provide the input data under the dict key 'input' or 'A'.")
