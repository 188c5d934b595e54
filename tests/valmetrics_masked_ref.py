"""Float64 numpy restatement of the per-sample MASKED validation / test metrics: what
ganslate/utils/metrics/val_test_metrics.py computes when get_metrics(..., mask=...) (:141-149) hands its metric functions
np.ma.masked_array(x * m, mask=~m) with m = mask.astype(bool) (create_masked_array, :19-29), built on the unmasked
restatement (tests/valmetrics_ref.py). Some of the calls behind the metrics honour the mask, others strip it:

- mae, mse, nmse: np.mean / np.linalg.norm run over the elements inside the mask (n of them)
- psnr: skimage converts both arrays with np.asarray, so the error is averaged over all S elements of the sample, while
  data_range = target.max() is the masked maximum Rm (the largest target value INSIDE the mask, not max(t * m))
- ssim: scipy.ndimage.uniform_filter sees t * m and p * m; the data range is Rm again
- nmi, histogram_chi2: np.histogramdd / np.histogram see t * m and p * m (masked-out elements count as zeros)

The mae / mse / nmse / masked-max / histogram rows are checked against numpy's masked arrays by
tests/test_valmetrics_masked_cpu.py. The psnr and ssim rows are read from scikit-image's source (_as_floats,
mean_squared_error, structural_similarity); scikit-image is not available to the tests, so they are not pinned against
it, as the unmasked ssim is not. A mask with nothing inside gives NaN in every column (the reference yields numpy's
masked constant there)."""
import numpy as np

from tests import valmetrics_ref as ref

COLUMNS = ref.COLUMNS


def _inside(mask):
    return np.asarray(mask).astype(bool)


def products(t, p, mask):
    """(t * m, p * m) in the arrays' own dtype: what np.asarray makes of the reference's masked arrays"""
    m = _inside(mask)
    return t * m, p * m


def masked_max(t, mask):
    """Rm: the largest target value inside the mask"""
    return float(t[_inside(mask)].max())


def mae(t, p, mask):
    m = _inside(mask)
    return ref.mae(t[m], p[m])


def mse(t, p, mask):
    m = _inside(mask)
    return float(ref.mse(t[m], p[m]))


def nmse(t, p, mask):
    m = _inside(mask)
    return ref.nmse(t[m], p[m])


def psnr(t, p, mask):
    tm, pm = products(t, p, mask)
    with np.errstate(divide="ignore"):
        return float(10 * np.log10(np.float64(masked_max(t, mask)) ** 2 / ref.mse(tm, pm)))


def ssim(t, p, mask):
    if t.ndim not in (3, 4):
        raise NotImplementedError(f"SSIM for {t.ndim} images not implemented")
    if t.shape[-1] < 7 or t.shape[-2] < 7:
        raise ValueError("win_size exceeds image extent")
    tm, pm = products(t, p, mask)
    planes = ref.ssim_map_interior(tm, pm, masked_max(t, mask)).reshape(-1, t.shape[-2] - 6, t.shape[-1] - 6)
    return float(np.mean(planes.mean(axis=(1, 2))))


def nmi(t, p, mask):
    return ref.nmi(*products(t, p, mask))


def histogram_chi2(t, p, mask):
    return ref.histogram_chi2(*products(t, p, mask))


def bin_counts(t, p, mask):
    return ref.bin_counts(*products(t, p, mask))


FNS = {"mae": mae, "mse": mse, "nmse": nmse, "psnr": psnr, "ssim": ssim, "nmi": nmi, "histogram_chi2": histogram_chi2}


def metrics(t, p, mask, names=COLUMNS):
    """{name: value} for one sample (target t, prediction p) inside `mask` (same shape; non-zero = inside)"""
    if not _inside(mask).any():
        return {k: float("nan") for k in names}
    return {k: FNS[k](t, p, mask) for k in names}
