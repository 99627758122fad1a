"""Numpy restatement of the blind noise estimate and the denoiser driven by it
(include/upr.h upr_noise_sigma_u8 / upr_denoise_lut_dev /
upr_denoise_nlm_u8_luts), the checker of csrc/noise.hip and upr.denoise's
estimate_sigma / nlm_auto: integer counts, then Python floats one operation at
a time, so the device's sigma agrees with it bit for bit and its pixels byte
for byte.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

import denoise_ref

BINS = 2041
Q = 4.0469385011764905  # 6 x the standard normal's 0.75 quantile


def histogram(img_u8, content=None):
    """img_u8: u8 [H,W,3]; content (top, left, nh, nw) or None -> int64 [2041]: the counts of
    |r| over the interior content pixels of the three channels, clipped samples skipped."""
    H, W = img_u8.shape[:2]
    top, left, nh, nw = content if content is not None else (0, 0, H, W)
    hist = np.zeros(BINS, np.int64)
    if nh < 3 or nw < 3:
        return hist
    I = img_u8[top:top + nh, left:left + nw].astype(np.int64)
    c, u, d = I[1:-1], I[:-2], I[2:]
    r = (u[:, :-2] + u[:, 2:] + d[:, :-2] + d[:, 2:]
         - 2 * (u[:, 1:-1] + d[:, 1:-1] + c[:, :-2] + c[:, 2:]) + 4 * c[:, 1:-1])
    clip = (I == 0) | (I == 255)
    bad = np.zeros(r.shape, bool)
    for dy in range(3):
        for dx in range(3):
            bad |= clip[dy:dy + nh - 2, dx:dx + nw - 2]
    return np.bincount(np.abs(r[~bad]), minlength=BINS).astype(np.int64)


def sigma_of_histogram(hist):
    n = int(hist.sum())
    if n == 0:
        return 0.0
    cum = np.cumsum(hist)
    b = int(np.argmax(2 * cum >= n))
    below = int(cum[b - 1]) if b else 0
    lo, wd = (b - 0.5, 1.0) if b else (0.0, 0.5)
    frac = float(n - 2 * below) / float(2 * int(hist[b]))
    med = lo + wd * frac
    return med / Q


def sigma(img_u8, content=None):
    """The noise std of one u8 [H,W,3] image in u8 levels, a Python float."""
    return sigma_of_histogram(histogram(img_u8, content))


def nlm_auto(src_u8, low_u8, illu_u8=None, content=None, scale=1.0, floor=denoise_ref.FLOOR,
             search=denoise_ref.SEARCH, patch=denoise_ref.PATCH):
    """denoise_ref.nlm of src_u8 with strength = scale * sigma(low_u8, content)."""
    return denoise_ref.nlm(src_u8, illu_u8, content, float(scale) * sigma(low_u8, content), floor, search, patch)
