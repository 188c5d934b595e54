"""Validation / test image metrics on the device (ganslate/utils/metrics/val_test_metrics.py:134-166, ValTestMetrics):
every enabled metric of `conf[mode].metrics` for every sample of a batch, computed by valmetrics.hip
(HipOps.valmetrics) into a [N, 7] fp64 device table. `table` / `cycle_table` enqueue and return device tensors; the
engines collect them and copy them to the host once per dataset (`to_lists`). `get_metrics` / `get_cycle_metrics`
mirror the reference's interface and sync.

Only what the flags ask for is launched: the moments pass always (mae, mse, nmse, psnr come from it), the SSIM pass for
`ssim` (and cycle_SSIM), the histogram pass for `nmi` or `histogram_chi2`.

Masked metrics (validator_tester.py:78-98, get_metrics(..., mask=...) at val_test_metrics.py:141-149): `masked_table`
scores a batch inside every mask of a list with one HipOps.valmetrics_masked call into a [N, L, 7] table; what the
reference's masked arrays make of each metric is stated at gs_valmetrics_masked in include/ganslate_hip.h."""
from ..nn.native.backend import get_ops

COLUMNS = ("mae", "mse", "nmse", "psnr", "ssim", "nmi", "histogram_chi2")      # layout of a table row (valmetrics.hip)
ORDER = ("ssim", "mse", "nmse", "psnr", "mae", "nmi", "histogram_chi2")        # key order of the reference's METRIC_DICT


class DeviceValTestMetrics:

    def __init__(self, conf, ops=None):
        self.conf = conf
        wanted = conf[conf.mode].metrics
        self.names = [k for k in ORDER if getattr(wanted, k, False)]
        self.ops = ops if ops is not None else get_ops()
        if not hasattr(self.ops, "valmetrics"):
            raise RuntimeError(f"backend `{getattr(self.ops, 'name', self.ops)}` has no device image metrics")
        self._ssim = "ssim" in self.names
        self._hist = "nmi" in self.names or "histogram_chi2" in self.names

    def table(self, pred, target):
        """[N, 7] fp64 device table of metric_fn(target[i], pred[i]) (NaN in the columns not enabled)"""
        return self.ops.valmetrics(target, pred, ssim=self._ssim, hist=self._hist)

    def cycle_table(self, rec, real):
        """[N] fp64 device column: ssim(real[i], rec[i]) (get_cycle_metrics, no denormalisation)"""
        return self.ops.valmetrics(real, rec, ssim=True, hist=False)[:, COLUMNS.index("ssim")]

    def masked_table(self, pred, target, masks):
        """[N, L, 7] fp64 device table of metric_fn on the masked arrays of target[i], pred[i] for each of the L masks
        (tensors of the batch's shape, non-zero = inside); a (sample, mask) pair with an empty mask holds NaN"""
        if not hasattr(self.ops, "valmetrics_masked"):
            raise RuntimeError(f"backend `{getattr(self.ops, 'name', self.ops)}` has no masked device image metrics")
        return self.ops.valmetrics_masked(target, pred, list(masks), ssim=self._ssim, hist=self._hist)

    def to_lists(self, table, prefix=""):
        """{prefix + name: [per-sample values]} for the enabled metrics of a (possibly concatenated) table: one copy"""
        host = table.detach().cpu().tolist()
        return {prefix + k: [row[COLUMNS.index(k)] for row in host] for k in self.names}

    def get_metrics(self, pred, target, mask=None):
        if mask is not None:
            return self.to_lists(self.masked_table(pred, target, [mask])[:, 0])
        return self.to_lists(self.table(pred, target))

    def get_cycle_metrics(self, rec, real):
        return {"cycle_SSIM": self.cycle_table(rec, real).cpu().tolist()}
