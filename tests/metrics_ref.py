"""Float64 numpy restatement of the device image metrics (csrc/metrics.hip), for
the tests: from one float32 image [3,H,W] (and an optional ground truth) the
same raw sums, histogram and metrics upr_image_metrics returns.  Box windows
are direct sums of shifted slices; SSIM pads with zeros, NIQE with numpy's
`symmetric` mode (scipy.ndimage's `reflect`: d c b a | a b c d).  No scipy.
Test infrastructure, not product code."""
import os

import numpy as np

NAMES = ("mean_brightness", "contrast", "entropy", "niqe", "saturation", "naturalness", "mse", "psnr", "ssim")
UNPAIRED = ("mean_brightness", "contrast", "entropy", "niqe", "saturation", "naturalness")
PAIRED = ("mean_brightness", "contrast", "entropy", "niqe", "psnr", "ssim", "mse", "saturation", "naturalness")
NSUMS = 14
# the metrics the reference accumulates in float32, and the two it forms in float64 / from integers
F32_ACCUMULATED = ("mean_brightness", "contrast", "niqe", "saturation", "naturalness", "mse", "psnr")
EXACT = ("ssim", "entropy")
TOL_F32 = 2e-6
TOL_EXACT = 1e-10

SHAPES = ((8, 8), (13, 70), (37, 53), (64, 64), (96, 160))
KINDS = ("enh", "low", "q8")


def load_fixture(golden_dir):
    """tests/golden/g10_metrics.npz (make_golden_metrics.py) -> list of cases:
    dict(shape, kind, x [3,H,W] f32, gt [3,H,W] f32, unpaired {name: float}, paired {name: float})."""
    z = np.load(os.path.join(golden_dir, "g10_metrics.npz"))
    cases = []
    for h, w in SHAPES:
        for kind in KINDS:
            k = f"{h}x{w}_{kind}"
            cases.append({"shape": (h, w), "kind": kind, "x": z[f"{k}_x"], "gt": z[f"{h}x{w}_gt"],
                          "unpaired": dict(zip(UNPAIRED, z[f"{k}_unpaired"].tolist())),
                          "paired": dict(zip(PAIRED, z[f"{k}_paired"].tolist()))})
    return cases


def hist_rule(x):
    """np.histogram(x, bins=256, range=(0, 1)) restated: a float32 value with
    0 <= x <= 1 goes to bin min(int(x * 256), 255) (x * 256 is exact in float32);
    anything else, NaN included, is dropped."""
    v = np.asarray(x, np.float32).ravel()
    keep = (v >= 0) & (v <= 1)
    b = np.minimum((v[keep] * np.float32(256)).astype(np.int64), 255)
    return np.bincount(b, minlength=256).astype(np.int64)


def box_sum(padded, k):
    """k x k window sums of an array padded by k // 2 on every side (rows, then columns)."""
    H, W = padded.shape[0] - (k - 1), padded.shape[1] - (k - 1)
    rows = np.zeros((padded.shape[0], W))
    for i in range(k):
        rows += padded[:, i:i + W]
    out = np.zeros((H, W))
    for i in range(k):
        out += rows[i:i + H]
    return out


def sums_hist(x, gt=None):
    """x, gt float32 [3,H,W] -> (sums float64 [14], hist int64 [256]); sums 10-13 NaN without gt."""
    x = np.asarray(x, np.float32)
    s = np.full(NSUMS, np.nan)
    xd = x.astype(np.float64)
    s[0:3] = xd.sum(axis=(1, 2))
    s[3:6] = (xd * xd).sum(axis=(1, 2))
    mx, mn = x.max(axis=0), x.min(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        sat = np.where(mx > np.float32(1e-8), (mx - mn) / mx, np.float32(0)).astype(np.float32)
    s[6] = sat.astype(np.float64).sum()
    gray = (np.float32(0.299) * x[0] + np.float32(0.587) * x[1]) + np.float32(0.114) * x[2]
    g2 = gray * gray  # float32
    mu = box_sum(np.pad(gray.astype(np.float64), 3, mode="symmetric"), 7) / 49.0
    e2 = box_sum(np.pad(g2.astype(np.float64), 3, mode="symmetric"), 7) / 49.0
    s[7] = np.sqrt(np.maximum(e2 - mu * mu, 0.0)).sum()
    s[8] = mu.sum()
    s[9] = (mu * mu).sum()
    if gt is not None:
        yd = np.asarray(gt, np.float32).astype(np.float64)
        s[10] = ((xd - yd) ** 2).sum()
        C1, C2 = 0.01 ** 2, 0.03 ** 2
        for c in range(3):
            a, b = np.pad(xd[c], 5), np.pad(yd[c], 5)
            mu1, mu2 = box_sum(a, 11) / 121.0, box_sum(b, 11) / 121.0
            s1 = box_sum(a * a, 11) / 121.0 - mu1 * mu1
            s2 = box_sum(b * b, 11) / 121.0 - mu2 * mu2
            s12 = box_sum(a * b, 11) / 121.0 - mu1 * mu2
            s[11 + c] = (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).sum()
    return s, hist_rule(x)


def finish(s, hist, H, W):
    """The nine metrics (order NAMES) from the raw sums and the histogram, as metrics_fin_kernel forms them."""
    hw, n = float(H * W), 3.0 * H * W
    m = np.full(len(NAMES), np.nan)
    mean = s[0:3].sum() / n
    contrast = np.sqrt(max(s[3:6].sum() / n - mean * mean, 0.0))
    p = hist[hist > 0] / hist.sum()
    cm = s[0:3] / hw
    cstd = np.sqrt(((cm - cm.mean()) ** 2).mean())
    cscore = min(max(1.0 - abs(contrast - 0.15) / 0.15, 0.0), 1.0)
    bscore = min(max(1.0 - abs(mean - 0.5) / 0.5, 0.0), 1.0)
    mmu = s[8] / hw
    m[0] = mean
    m[1] = contrast
    m[2] = -(p * np.log2(p)).sum()
    m[3] = (s[7] / hw) / (np.sqrt(max(s[9] / hw - mmu * mmu, 0.0)) + 1e-8)
    m[4] = s[6] / hw
    m[5] = 0.3 * (1.0 - cstd) + 0.4 * cscore + 0.3 * bscore
    if not np.isnan(s[10]):
        mse = s[10] / n
        m[6] = mse
        m[7] = 100.0 if mse < 1e-10 else 20.0 * np.log10(1.0 / np.sqrt(mse))
        m[8] = (s[11:14] / hw).sum() / 3.0
    return m


def metrics(x, gt=None):
    """x (, gt) float32 [3,H,W] -> (metrics float64 [9] in NAMES order, sums [14], hist [256])."""
    s, h = sums_hist(x, gt)
    return finish(s, h, x.shape[1], x.shape[2]), s, h


def metrics_dict(x, gt=None):
    """calculate_metrics' dict (keys and order included) from the restatement."""
    m = dict(zip(NAMES, metrics(x, gt)[0].tolist()))
    return {k: m[k] for k in (PAIRED if gt is not None else UNPAIRED)}


def tolerance(name):
    return TOL_EXACT if name in EXACT else TOL_F32


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)
