"""Numpy restatement of the lightness order error (include/upr.h upr_image_loe;
Wang et al. 2013): the u8 cast, the lightness map, the integer sample grid and
the count D of order-reversed ordered pairs, in two forms -- pair by pair (in
row chunks) and from the 256 x 256 joint histogram and its 2-D prefix."""
import numpy as np


def u8(x):
    """The project's float -> u8 cast: float32 clip(v, 0, 1) * 255, truncated."""
    return (np.clip(np.asarray(x, np.float32), 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)


def grid(H, W, sample):
    """-> (source rows [h], source columns [w]) of the sample grid."""
    m = min(H, W)
    if sample <= 0 or m <= sample:
        return np.arange(H), np.arange(W)
    h = max(1, (H * sample + m // 2) // m)
    w = max(1, (W * sample + m // 2) // m)
    return ((2 * np.arange(h) + 1) * H) // (2 * h), ((2 * np.arange(w) + 1) * W) // (2 * w)


def lightness(x, sample):
    """x [3,H,W] float -> int64 [N]: max over the channels of the cast, on the sample grid."""
    L = u8(x).max(0)
    r, c = grid(L.shape[0], L.shape[1], sample)
    return L[np.ix_(r, c)].ravel().astype(np.int64)


def count_pairs(a, b, chunk=256):
    """D pair by pair: ordered (x, y) with (a_x >= a_y) != (b_x >= b_y)."""
    D = 0
    for i in range(0, len(a), chunk):
        D += int(((a[i:i + chunk, None] >= a[None, :]) != (b[i:i + chunk, None] >= b[None, :])).sum())
    return D


def count_hist(a, b):
    """D from the joint histogram J and its inclusive 2-D prefix C:
    sum J[a][b] (C[a][255] + C[255][b] - 2 C[a][b]) (python integers: no overflow)."""
    J = np.zeros((256, 256), np.int64)
    np.add.at(J, (a, b), 1)
    C = J.cumsum(0).cumsum(1)
    T = C[:, 255:256] + C[255:256, :] - 2 * C
    return sum(int(j) * int(t) for j, t in zip(J.ravel(), T.ravel()) if j)


def loe(low, enh, sample=50, pairs=False):
    """low, enh [3,H,W] -> (D, N, D / N)."""
    a, b = lightness(low, sample), lightness(enh, sample)
    D = count_pairs(a, b) if pairs else count_hist(a, b)
    return D, len(a), D / len(a)


def pair(H, W, seed):
    """A dark noise image and a brightened, unevenly lit, noisy version of it, float32 [3,H,W]."""
    rng = np.random.default_rng(seed)
    x = rng.random((3, H, W), dtype=np.float32) * np.float32(0.3)
    ramp = np.linspace(0.5, 2.5, W, dtype=np.float32)[None, None, :]
    e = np.clip(x * ramp * 2 + np.float32(0.02) * rng.standard_normal((3, H, W)).astype(np.float32), 0, 1)
    return x, e.astype(np.float32)


# (H, W, sample) of the small cases both forms and the device are checked on
SMALL = [(8, 8, 50), (37, 53, 50), (64, 96, 50), (120, 200, 50), (96, 64, 16), (64, 64, 0)]
