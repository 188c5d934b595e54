"""Float64 numpy restatement of the per-sample validation / test metrics of ganslate/utils/metrics/val_test_metrics.py
(metric_fn(target, pred) for one sample of C x H x W or C x D x H x W), without scikit-image or scipy:

- ssim: skimage.metrics.structural_similarity with defaults (7 x 7 uniform window, sample covariance 49/48, K1 0.01,
  K2 0.03) and data_range = max(target) of the sample, in float64, averaged over the crop(S, 3) interior of each plane
  (box sums by cumulative sums) and then over the planes (every channel, or every depth slice of every channel)
- nmi: (H0 + H1) / H01 of np.histogramdd([t, p], bins=100, density=True) with scipy.stats.entropy's definition
- histogram_chi2: np.histogram(x, bins=100) of each, normalised to sum 1, sum (p - g)^2 / (p + g) without 0/0 bins
"""
import numpy as np

COLUMNS = ("mae", "mse", "nmse", "psnr", "ssim", "nmi", "histogram_chi2")
BINS = 100


def _d(t, p):
    return t.astype(np.float64) - p.astype(np.float64)


def mae(t, p):
    return float(np.mean(np.abs(_d(t, p))))


def mse(t, p):
    return np.mean(_d(t, p) ** 2)


def nmse(t, p):
    return float(np.sum(_d(t, p) ** 2) / np.sum(t.astype(np.float64) ** 2))


def psnr(t, p):
    with np.errstate(divide="ignore"):
        return float(10 * np.log10(np.float64(t.max()) ** 2 / mse(t, p)))     # mse == 0 -> inf


def _box7(x):
    """sum over every 7 x 7 window of the last two axes (the valid part only: (H-6) x (W-6))"""
    c = np.zeros(x.shape[:-2] + (x.shape[-2] + 1, x.shape[-1] + 1))
    c[..., 1:, 1:] = np.cumsum(np.cumsum(x, axis=-2), axis=-1)
    return c[..., 7:, 7:] - c[..., :-7, 7:] - c[..., 7:, :-7] + c[..., :-7, :-7]


def ssim_map_interior(t, p, data_range):
    """S of skimage structural_similarity over the interior of each H x W plane of t, p (float64)"""
    x, y = t.astype(np.float64), p.astype(np.float64)
    n = 49.0
    ux, uy = _box7(x) / n, _box7(y) / n
    uxx, uyy, uxy = _box7(x * x) / n, _box7(y * y) / n, _box7(x * y) / n
    cov = n / (n - 1)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))


def ssim(t, p):
    if t.ndim not in (3, 4):
        raise NotImplementedError(f"SSIM for {t.ndim} images not implemented")
    if t.shape[-1] < 7 or t.shape[-2] < 7:
        raise ValueError("win_size exceeds image extent")
    planes = ssim_map_interior(t, p, float(t.max())).reshape(-1, t.shape[-2] - 6, t.shape[-1] - 6)
    return float(np.mean(planes.mean(axis=(1, 2))))


def _entropy(pk):
    pk = np.asarray(pk, dtype=np.float64).ravel()
    pk = pk / pk.sum()
    nz = pk[pk > 0]
    return float(-np.sum(nz * np.log(nz)))


def joint_histogram(t, p):
    return np.histogramdd([np.reshape(t, -1), np.reshape(p, -1)], bins=BINS, density=True)


def nmi(t, p):
    hist, _ = joint_histogram(t, p)
    return (_entropy(hist.sum(axis=0)) + _entropy(hist.sum(axis=1))) / _entropy(hist)


def histogram_chi2(t, p):
    g, _ = np.histogram(t, bins=BINS)
    q, _ = np.histogram(p, bins=BINS)
    g, q = g / g.sum(), q / q.sum()
    keep = (g + q) != 0
    return float(np.sum((q[keep] - g[keep]) ** 2 / (q[keep] + g[keep])))


def bin_counts(t, p):
    """raw counts: np.histogram of t, of p, and the unnormalised joint np.histogramdd([t, p])"""
    ht, _ = np.histogram(t, bins=BINS)
    hp, _ = np.histogram(p, bins=BINS)
    hj, _ = np.histogramdd([np.reshape(t, -1), np.reshape(p, -1)], bins=BINS)
    return ht.astype(np.int64), hp.astype(np.int64), hj.astype(np.int64)


FNS = {"mae": mae, "mse": lambda t, p: float(mse(t, p)), "nmse": nmse, "psnr": psnr, "ssim": ssim, "nmi": nmi,
       "histogram_chi2": histogram_chi2}


def metrics(t, p, names=COLUMNS):
    """{name: value} for one sample (target t, prediction p)"""
    return {k: FNS[k](t, p) for k in names}
