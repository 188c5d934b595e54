"""Validator and Tester (ganslate/engines/validator_tester.py:9-135 + trainer.py:95-108). The Validator shares the
Trainer's model; the Tester builds the generator itself and loads `test.checkpointing.load_iter` (BaseGAN.setup). Both
run `infer` (sliding-window when configured) over their loader(s) and score every sample with the metrics of
utils/metrics/val_test_metrics.py that `<mode>.metrics` enables.

- Model on the GPU: all seven metrics (mae, mse, nmse, psnr, ssim, nmi, histogram_chi2) on the device
  (utils/val_metrics.py, valmetrics.hip), plus `cycle_SSIM` = ssim(real_A, infer(fake_B, direction="BA")) in validation
  when `val.metrics.cycle_metrics` is set. A model whose `infer` takes no `direction` (Pix2Pix, CUT) gets a log line and
  no cycle metric; the reference raises a RuntimeError there, which with the default `cycle_metrics: true` stops every
  Pix2Pix / CUT validation. The per-sample tables stay on the device until the end of each dataset.
- Model on the CPU (the oracle backend of the test-suite): the host path of mae, mse, nmse and psnr below; ssim, nmi and
  histogram_chi2 are skipped there with a log line.

Batches that carry `masks` ({label: tensor of the batch's shape}, as the medical datasets return BODY, GTV, ...) get every
enabled metric once more per label on the device path, as `<metric>_<label>` (and `Original_<metric>_<label>` with
`compute_over_input`), between the standard keys and `cycle_SSIM` as validator_tester.py:78-98 orders them. The masks are
not denormalised; all labels of a batch go through one masked call. The host path ignores masks. The Tester writes
`<test.output_dir>/test/metrics.csv` when `test.metrics.save_to_csv` is set: one row per sample, one column per metric,
plus a `dataset` column with `multi_dataset`.

With `<mode>.dataset.device_transforms: true` the image-folder datasets hand over decoded bytes and every batch goes through
the device-side input pipeline first (BaseEngineWithInference.input_pipeline); what follows sees the same tensors, already
on the device.

Every batch's `fake_B` goes to the dataset's `save()` where it has one (BaseEngineWithInference.save_generated_tensor,
`saved/[{dataset}/][{iter}/]`), and every sample is logged as one PNG of `real_A, fake_B, real_B` and then each mask label as
`2 * mask - 1` side by side, a volume as its middle slice: `images/[{dataset}/]{iter}/{idx}_{name}.png` in validation,
`images/[{dataset}/]{idx}_{name}.png` in test (utils/trackers.py; the grid is one kernel, HipOps.visuals_grid, so images are
written on the device path only). The W&B / TensorBoard trackers stay out of scope."""
import csv
import inspect
from pathlib import Path

import numpy as np
import torch

from ..utils import environment
from ..utils.builders import build_gan, build_loader
from ..utils.trackers import ImageWriter
from .base import BaseEngineWithInference


def _mae(gt, pred):
    return float(np.mean(np.abs(gt - pred)))


def _mse(gt, pred):
    return float(np.mean((gt - pred) ** 2))


def _nmse(gt, pred):
    return float(np.linalg.norm(gt - pred) ** 2 / np.linalg.norm(gt) ** 2)


def _psnr(gt, pred):
    # skimage.metrics.peak_signal_noise_ratio(gt, pred, data_range=gt.max()) (val_test_metrics.py:56-59)
    err = np.mean((gt.astype(np.float64) - pred.astype(np.float64)) ** 2)
    return float(10 * np.log10((float(gt.max()) ** 2) / err))


METRICS = {"mae": _mae, "mse": _mse, "nmse": _nmse, "psnr": _psnr}


def _takes_direction(fn):
    try:
        params = inspect.signature(fn).parameters.values()
    except (TypeError, ValueError):
        return False
    return any(p.name == "direction" or p.kind == p.VAR_KEYWORD for p in params)


class BaseValTestEngine(BaseEngineWithInference):
    """The metric loop shared by the Validator and the Tester; subclasses set `self.model` and call `_init_metrics`."""

    def __init__(self, conf):
        super().__init__(conf)
        self.data_loaders = build_loader(self.conf)
        if not isinstance(self.data_loaders, dict):
            self.data_loaders = {None: self.data_loaders}
        self.history = []          # (iteration, dataset name, {metric: mean over the samples})
        self.samples = {}          # dataset name -> per-sample rows of the last run
        self.metricizer = None
        self._masks_logged = False
        self.writer = ImageWriter(self.conf)

    def _init_metrics(self):
        wanted = self.conf[self.conf.mode].metrics
        self.on_device = self.model.device.type == "cuda"
        self.cycle = False
        if self.on_device:
            from ..utils.val_metrics import DeviceValTestMetrics
            self.metricizer = DeviceValTestMetrics(self.conf)
            if getattr(wanted, "cycle_metrics", False):
                self.cycle = _takes_direction(self.model.infer)
                if not self.cycle:
                    self.logger.info(f"{self.conf.mode}.metrics.cycle_metrics: `{type(self.model).__name__}.infer` has no "
                                     "`direction`; cycle_SSIM skipped")
        else:
            self.metric_names = [k for k in METRICS if getattr(wanted, k, False)]
            skipped = [k for k in ("ssim", "nmi", "histogram_chi2") if getattr(wanted, k, False)]
            if skipped:
                self.logger.info(f"{self.conf.mode} metrics {skipped} need scikit-image / scipy in the reference; "
                                 "skipped here")

    def run(self, current_idx=None):
        self.logger.info(f'{"Validation" if self.conf.mode == "val" else "Testing"} started.')
        was_training = [getattr(net, "training", True) for net in self.model.networks.values()]
        self.model.eval()
        try:
            for name, loader in self.data_loaders.items():
                dataset = loader.dataset
                self.input_pipeline(loader)        # raises for a dataset whose device path cannot feed this engine
                # Denormalize the data if the dataset defines `denormalize` (validator_tester.py:72-77)
                denormalize = getattr(dataset, "denormalize", None)
                over_input = bool(getattr(self.conf[self.conf.mode].metrics, "compute_over_input", False))
                score = self._device_rows if self.on_device else self._host_rows
                rows = score(loader, denormalize, over_input, name, current_idx)
                self.writer.write_samples(current_idx, dataset_name=name)
                self.samples[name] = rows
                mean = {k: float(np.mean([r[k] for r in rows])) for k in rows[0]} if rows else {}
                self.history.append((current_idx, name, mean))
                self.logger.info(f"{self.conf.mode} @ {current_idx} [{name}] {mean}")
        finally:
            for net, flag in zip(self.model.networks.values(), was_training):
                net.train(flag)

    def _log_masks(self, data):
        if "masks" in data and not self._masks_logged:
            self.logger.info("batches carry `masks`: masked metrics are computed on the device path only; the host "
                             "path ignores the masks")
            self._masks_logged = True

    def _save_and_log(self, data, loader, visuals, dataset_name, current_idx):
        """the output side of a batch (validator_tester.py:70-78,117 + ValTestTracker.add_sample)"""
        self.save_generated_tensor(generated_tensor=visuals["fake_B"], metadata=data.get("metadata"), data_loader=loader,
                                   idx=current_idx, dataset_name=dataset_name)
        visuals = dict(visuals)
        for label, mask in data.get("masks", {}).items():
            visuals[label] = mask.to(self.model.device).float() * 2 - 1
        self.writer.add_samples(self.writer.compose(visuals, mid_slice_only=True))

    def _batches(self, loader):
        """the loader's batches, through the device-side input pipeline where the dataset has one"""
        pipeline = self.input_pipeline(loader)
        return loader if pipeline is None else map(pipeline, loader)

    def _host_rows(self, loader, denormalize, over_input, dataset_name=None, current_idx=None):
        rows = []
        for data in self._batches(loader):
            self._log_masks(data)
            real_A = data["A"].to(self.model.device)
            with torch.no_grad():
                fake_B = self.infer(real_A)
            self._save_and_log(data, loader, {"real_A": real_A, "fake_B": fake_B, "real_B": data["B"]}, dataset_name,
                               current_idx)
            pred, target, original = fake_B.detach().float().cpu(), data["B"].float(), data["A"].float()
            if denormalize:
                pred, target = denormalize(pred.clone()), denormalize(target.clone())
                if over_input:
                    original = denormalize(original.clone())
            pred, target, original = pred.numpy(), target.numpy(), original.numpy()
            # one score per SAMPLE of the batch (ValTestMetrics.get_metrics iterates zip(inputs, targets),
            # val_test_metrics.py:152-153): psnr's data range and nmse's norm are per sample
            for i in range(pred.shape[0]):
                row = {k: METRICS[k](target[i], pred[i]) for k in self.metric_names}
                if over_input:
                    row.update({f"Original_{k}": METRICS[k](target[i], original[i]) for k in self.metric_names})
                rows.append(row)
        return rows

    def _device_rows(self, loader, denormalize, over_input, dataset_name=None, current_idx=None):
        """per-batch device tables, one host copy per dataset (validator_tester.py:62-112)"""
        m = self.metricizer
        tables, originals, cycles = [], [], []
        labels, masked, masked_originals = None, [], []
        for data in self._batches(loader):
            real_A = data["A"].to(self.model.device)
            with torch.no_grad():
                fake_B = self.infer(real_A)
                target = data["B"].to(self.model.device)
                self._save_and_log(data, loader, {"real_A": real_A, "fake_B": fake_B, "real_B": target}, dataset_name,
                                   current_idx)
                pred, target, original = fake_B.detach().float(), target.float(), real_A.float()
                if denormalize:
                    pred, target = denormalize(pred.clone()), denormalize(target.clone())
                    if over_input:
                        original = denormalize(original.clone())
                tables.append(m.table(pred, target))
                if over_input:
                    originals.append(m.table(original, target))
                if "masks" in data:
                    if labels is None:
                        labels = list(data["masks"])
                    if list(data["masks"]) != labels or len(masked) != len(tables) - 1:
                        raise ValueError(f"every batch of a dataset must carry the same mask labels; got "
                                         f"{list(data['masks'])} after {labels}")
                    masks = [data["masks"][k].to(self.model.device) for k in labels]
                    masked.append(m.masked_table(pred, target, masks))
                    if over_input:
                        masked_originals.append(m.masked_table(original, target, masks))
                elif labels is not None:
                    raise ValueError(f"every batch of a dataset must carry the same mask labels; got none after {labels}")
                if self.cycle:
                    rec_A = self.infer(fake_B, direction="BA")
                    cycles.append(m.cycle_table(rec_A, real_A))
        if not tables:
            return []
        cols = m.to_lists(torch.cat(tables))
        if over_input:
            cols.update(m.to_lists(torch.cat(originals), prefix="Original_"))
        if labels:
            # one copy of the [samples, L, 7] table(s); per label the masked keys, then the Original_ ones (:84-95)
            by_label = torch.cat(masked).cpu().transpose(0, 1)
            by_label_original = torch.cat(masked_originals).cpu().transpose(0, 1) if over_input else None
            for i, label in enumerate(labels):
                cols.update({f"{k}_{label}": v for k, v in m.to_lists(by_label[i]).items()})
                if over_input:
                    cols.update({f"Original_{k}_{label}": v for k, v in m.to_lists(by_label_original[i]).items()})
        if self.cycle:
            cols["cycle_SSIM"] = torch.cat(cycles).cpu().tolist()
        n = len(next(iter(cols.values()))) if cols else 0
        return [{k: v[i] for k, v in cols.items()} for i in range(n)]


class Validator(BaseValTestEngine):

    def __init__(self, conf, model):
        super().__init__(conf)
        self.model = model
        self._init_metrics()

    def _set_mode(self):
        self.conf.mode = "val"


class Tester(BaseValTestEngine):
    """Scores the generator of checkpoint `test.checkpointing.load_iter` on the test set(s) (validator_tester.py:127-135)
    and writes the per-sample metrics.csv. There is no cycle metric in test mode (TestMetricsConfig has no such flag, and
    a CycleGAN built outside training holds only G_AB)."""

    def __init__(self, conf):
        super().__init__(conf)
        # under this engine's own `test.output_dir`, as the reference's tracker does (trackers/base.py:18);
        # BaseEngine's directory follows the caller's conf, whose mode is still "train"
        self.output_dir = Path(self.conf.test.output_dir) / "test"
        environment.setup_logging()
        self.model = build_gan(self.conf)
        self._init_metrics()

    def _set_mode(self):
        self.conf.mode = "test"

    def run(self, current_idx=None):
        super().run(current_idx)
        if self.conf.test.metrics.save_to_csv:
            self.write_csv()

    def write_csv(self):
        multi = self.conf.test.multi_dataset is not None
        names = []
        for rows in self.samples.values():
            for r in rows:
                names += [k for k in r if k not in names]
        fields = (["dataset"] if multi else []) + ["sample"] + names
        self.output_dir.mkdir(parents=True, exist_ok=True)
        path = self.output_dir / "metrics.csv"
        with open(path, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=fields)
            w.writeheader()
            for name, rows in self.samples.items():
                for i, r in enumerate(rows):
                    w.writerow({**({"dataset": name} if multi else {}), "sample": i, **r})
        self.logger.info(f"Per-sample test metrics written to `{path}`")
        return path
