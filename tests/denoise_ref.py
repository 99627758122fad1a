"""Numpy restatement of the illumination-weighted non-local means (include/upr.h
upr_denoise_lut / upr_denoise_nlm_u8), the checker of csrc/denoise.hip and
upr.denoise: the same integers in the same order of rounding, so the device's
pixels agree with it byte for byte.

TEST INFRASTRUCTURE ONLY.
"""
import math

import numpy as np

STRENGTH = 1.0
FLOOR = 16
SEARCH = 5
PATCH = 2

# floor(4095 exp(-i / 32) + 0.5), i = 0..255, as the kernel's table holds it
EXPW = np.array([
    4095, 3969, 3847, 3729, 3614, 3503, 3395, 3290, 3189, 3091, 2996, 2904, 2814, 2728, 2644, 2563,
    2484, 2407, 2333, 2261, 2192, 2124, 2059, 1996, 1934, 1875, 1817, 1761, 1707, 1655, 1604, 1554,
    1506, 1460, 1415, 1372, 1329, 1289, 1249, 1210, 1173, 1137, 1102, 1068, 1035, 1004, 973, 943,
    914, 886, 858, 832, 806, 782, 757, 734, 712, 690, 668, 648, 628, 609, 590, 572,
    554, 537, 521, 505, 489, 474, 459, 445, 432, 418, 405, 393, 381, 369, 358, 347,
    336, 326, 316, 306, 297, 288, 279, 270, 262, 254, 246, 238, 231, 224, 217, 210,
    204, 198, 192, 186, 180, 174, 169, 164, 159, 154, 149, 145, 140, 136, 132, 128,
    124, 120, 116, 113, 109, 106, 103, 99, 96, 93, 90, 88, 85, 82, 80, 77,
    75, 73, 70, 68, 66, 64, 62, 60, 58, 57, 55, 53, 52, 50, 48, 47,
    45, 44, 43, 41, 40, 39, 38, 37, 35, 34, 33, 32, 31, 30, 29, 28,
    28, 27, 26, 25, 24, 24, 23, 22, 21, 21, 20, 20, 19, 18, 18, 17,
    17, 16, 16, 15, 15, 14, 14, 13, 13, 13, 12, 12, 12, 11, 11, 10,
    10, 10, 10, 9, 9, 9, 8, 8, 8, 8, 7, 7, 7, 7, 7, 6,
    6, 6, 6, 6, 5, 5, 5, 5, 5, 5, 5, 4, 4, 4, 4, 4,
    4, 4, 4, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2,
    2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1,
], dtype=np.int64)
assert EXPW.tolist() == [int(math.floor(4095.0 * math.exp(-i / 32.0) + 0.5)) for i in range(256)]


def lut(strength=STRENGTH, floor=FLOOR, patch=PATCH):
    """upr_denoise_lut: uint32 [256], fp64 one operation at a time."""
    n = float(3 * (2 * patch + 1) ** 2)
    L = np.maximum(np.arange(256), int(floor)).astype(np.float64)
    h = float(strength) * 255.0 / L
    h2 = h * h
    with np.errstate(divide="ignore", over="ignore"):
        v = np.minimum(np.floor(1048576.0 * 32.0 / (n * h2) + 0.5), 4294967295.0)
    v = np.where(h2 == 0.0, 4294967295.0, v)
    return v.astype(np.uint64).astype(np.uint32)


def _box(a, r):
    """Exact sums of an int64 [h + 2r, w + 2r] array over every (2r+1)^2 window -> [h, w]."""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(a, axis=0), axis=1)
    k = 2 * r + 1
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def nlm(src_u8, illu_u8=None, content=None, strength=STRENGTH, floor=FLOOR, search=SEARCH, patch=PATCH):
    """One image: src_u8 u8 [H,W,3]; illu_u8 u8 [H,W] or [H,W,3] (channel 0 is read) or None;
    content (top, left, nh, nw) or None for the whole image -> u8 [H,W,3]."""
    H, W = src_u8.shape[:2]
    top, left, nh, nw = content if content is not None else (0, 0, H, W)
    S, P = int(search), int(patch)
    R = S + P
    table = lut(strength, floor, P).astype(np.uint64)
    if illu_u8 is None:
        Lp = np.full((nh, nw), 255, np.int64)
    else:
        m = illu_u8 if illu_u8.ndim == 2 else illu_u8[..., 0]
        Lp = m[top:top + nh, left:left + nw].astype(np.int64)
    scale = table[Lp]
    I = src_u8[top:top + nh, left:left + nw].astype(np.int64)
    pad = np.pad(I, ((R, R), (R, R), (0, 0)), mode="edge")  # I~ on [-R, nh + R) x [-R, nw + R)
    # the p + o side: I~ on [-P, nh + P) x [-P, nw + P)
    a = pad[S:S + nh + 2 * P, S:S + nw + 2 * P]
    yy, xx = np.mgrid[:nh, :nw]
    sw = np.zeros((nh, nw), np.int64)
    swi = np.zeros((nh, nw, 3), np.int64)
    for sy in range(-S, S + 1):
        for sx in range(-S, S + 1):
            b = pad[S + sy:S + sy + nh + 2 * P, S + sx:S + sx + nw + 2 * P]
            d = _box(((a - b) ** 2).sum(axis=2), P)
            assert d.max() < 1 << 24
            t = (d.astype(np.uint64) * scale) >> np.uint64(20)
            w = np.where(t < 256, EXPW[np.minimum(t, 255).astype(np.int64)], 0)
            inside = (yy + sy >= 0) & (yy + sy < nh) & (xx + sx >= 0) & (xx + sx < nw)
            w = np.where(inside, w, 0)
            sw += w
            swi += w[..., None] * pad[R + sy:R + sy + nh, R + sx:R + sx + nw]
    assert sw.min() >= 4095 and swi.max() < 1 << 30
    out = src_u8.copy()
    out[top:top + nh, left:left + nw] = ((2 * swi + sw[..., None]) // (2 * sw[..., None])).astype(np.uint8)
    return out


def nlm_float64(src_u8, illu_u8=None, content=None, strength=STRENGTH, floor=FLOOR, search=SEARCH, patch=PATCH):
    """The same filter in plain float64, independently formulated: direct patch sums per
    candidate, weights exp(-mean squared difference / h^2), no tables -> float64 [H,W,3]."""
    H, W = src_u8.shape[:2]
    top, left, nh, nw = content if content is not None else (0, 0, H, W)
    S, P = int(search), int(patch)
    n = 3.0 * (2 * P + 1) ** 2
    I = src_u8[top:top + nh, left:left + nw].astype(np.float64)
    if illu_u8 is None:
        Lp = np.full((nh, nw), 255.0)
    else:
        m = illu_u8 if illu_u8.ndim == 2 else illu_u8[..., 0]
        Lp = np.maximum(m[top:top + nh, left:left + nw].astype(np.float64), float(floor))
    h2 = (strength * 255.0 / Lp) ** 2
    ys, xs = np.arange(nh), np.arange(nw)

    def at(y, x):  # I~: coordinates clamped to the rectangle
        return I[np.clip(y, 0, nh - 1)[:, None], np.clip(x, 0, nw - 1)[None, :]]

    num = np.zeros((nh, nw, 3))
    den = np.zeros((nh, nw))
    for sy in range(-S, S + 1):
        for sx in range(-S, S + 1):
            d = np.zeros((nh, nw))
            for oy in range(-P, P + 1):
                for ox in range(-P, P + 1):
                    d += ((at(ys + oy, xs + ox) - at(ys + sy + oy, xs + sx + ox)) ** 2).sum(axis=2)
            with np.errstate(divide="ignore", invalid="ignore"):
                w = np.where(d == 0, 1.0, np.exp(-(d / n) / h2))
            inside = ((ys + sy >= 0) & (ys + sy < nh))[:, None] & ((xs + sx >= 0) & (xs + sx < nw))[None, :]
            w = np.where(inside, w, 0.0)
            den += w
            num += w[..., None] * at(ys + sy, xs + sx)
    out = src_u8.astype(np.float64)
    out[top:top + nh, left:left + nw] = num / den[..., None]
    return out


def psnr_u8(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)
