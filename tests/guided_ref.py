"""Numpy restatement of the guided-filter restore (include/upr.h upr_guided_fit /
upr_guided_apply), the checker of csrc/guided.hip and upr.guided: the same
integer sums and the same fp64 operations in the same order, so the device's
coefficients agree with it bit for bit and its pixels byte for byte.

TEST INFRASTRUCTURE ONLY.  The low-resolution side of a case comes from
oracle.letterbox (lowres()).
"""
import numpy as np

from oracle import letterbox as olb

RADIUS = 4
EPS = 1e-4


def content_rect(shape, max_size):
    """(top, left, nh, nw) of load_image's letterbox (auto=True, scaleup=False) for an (H, W) image; max_size None:
    the image's own size."""
    H, W = shape
    new = (max_size, max_size) if max_size is not None else (H, W)
    r = min(min(new[0] / H, new[1] / W), 1.0)
    nw, nh = int(round(W * r)), int(round(H * r))
    dw, dh = np.mod(new[1] - nw, 32) / 2, np.mod(new[0] - nh, 32) / 2
    return int(round(dh - 0.1)), int(round(dw - 0.1)), nh, nw


def lowres(src_u8, max_size):
    """The letterboxed u8 image of the harness and its content rectangle."""
    H, W = src_u8.shape[:2]
    lb, _, _ = olb.letterbox(src_u8, new_shape=max_size if max_size is not None else (H, W), auto=True,
                             scaleup=False)
    rect = content_rect((H, W), max_size)
    assert lb.shape[0] >= rect[0] + rect[2] and lb.shape[1] >= rect[1] + rect[3]
    return lb, rect


def _window_sums(v, r):
    """Exact int64 sums of v [h, w] over the (2r+1)^2 window clipped to the array."""
    h, w = v.shape
    c = np.zeros((h + 1, w + 1), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(v.astype(np.int64), axis=0), axis=1)
    y0, y1 = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r, h - 1) + 1
    x0, x1 = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r, w - 1) + 1
    return c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]


def _ordered_sum_last(a, r):
    """Sum over the clipped window along the last axis: the in-range taps in increasing index,
    starting from the first one."""
    n = a.shape[-1]
    idx = np.arange(n)
    acc = np.zeros_like(a)
    started = np.zeros(n, bool)
    for d in range(-r, r + 1):
        t = idx + d
        ok = (t >= 0) & (t < n)
        tv = a[..., np.clip(t, 0, n - 1)]
        acc = np.where(ok & ~started, tv, np.where(ok & started, acc + tv, acc))
        started |= ok
    return acc


def _count(h, w, r):
    ny = np.minimum(np.arange(h) + r, h - 1) - np.maximum(np.arange(h) - r, 0) + 1
    nx = np.minimum(np.arange(w) + r, w - 1) - np.maximum(np.arange(w) - r, 0) + 1
    return ny[:, None].astype(np.int64) * nx[None, :].astype(np.int64)


def fit_ab(guide_u8, target_u8, content, radius=RADIUS, eps=EPS):
    """The per-pixel a, b before the window mean: float64 [2,3,nh,nw]."""
    top, left, nh, nw = content
    N = _count(nh, nw, radius)
    out = np.empty((2, 3, nh, nw), np.float64)
    for c in range(3):
        I = guide_u8[top:top + nh, left:left + nw, c].astype(np.int64)
        p = target_u8[top:top + nh, left:left + nw, c].astype(np.int64)
        S_I, S_p = _window_sums(I, radius), _window_sums(p, radius)
        S_II, S_Ip = _window_sums(I * I, radius), _window_sums(I * p, radius)
        num = (N * S_Ip - S_I * S_p).astype(np.float64)
        den = (N * S_II - S_I * S_I).astype(np.float64) + (eps * 65025.0) * (N * N).astype(np.float64)
        a = num / den
        out[0, c] = a
        out[1, c] = (S_p.astype(np.float64) - a * S_I.astype(np.float64)) / N.astype(np.float64)
    return out


def fit(guide_u8, target_u8, content, radius=RADIUS, eps=EPS):
    """One image: guide_u8 / target_u8 u8 [Hl,Wl,3] -> ab float64 [2,3,nh,nw]."""
    _, _, nh, nw = content
    ab = fit_ab(guide_u8, target_u8, content, radius, eps)
    N = _count(nh, nw, radius).astype(np.float64)
    rows = _ordered_sum_last(ab, radius)
    cols = np.swapaxes(_ordered_sum_last(np.swapaxes(rows, -1, -2), radius), -1, -2)
    return cols / N


def _taps(n_full, n):
    f = (np.arange(n_full, dtype=np.float64) + 0.5) * (float(n) / float(n_full)) - 0.5
    f = np.minimum(np.maximum(f, 0.0), float(n - 1))
    i0 = np.floor(f).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), f - i0.astype(np.float64)


def _sample(M, H, W):
    """v(M) of every full-resolution pixel: M float64 [..., nh, nw] -> [..., H, W]."""
    y0, y1, wy = _taps(H, M.shape[-2])
    x0, x1, wx = _taps(W, M.shape[-1])
    wy = wy[:, None]
    r0, r1 = M[..., y0, :], M[..., y1, :]
    h0 = (1.0 - wx) * r0[..., x0] + wx * r0[..., x1]
    h1 = (1.0 - wx) * r1[..., x0] + wx * r1[..., x1]
    return (1.0 - wy) * h0 + wy * h1


def apply(src_u8, ab, illu_u8=None, content=None, comparison=None):
    """One image: src_u8 u8 [H,W,3], ab [2,3,nh,nw], illu_u8 the letterboxed map u8 [Hl,Wl,3] or None
    -> (enh [H,W,3], illu [H,W,3] or None, cmp [H,comparison*W,3] or None)."""
    H, W = src_u8.shape[:2]
    v = _sample(ab, H, W)  # [2,3,H,W]
    e = v[0] * np.moveaxis(src_u8, 2, 0).astype(np.float64) + v[1]
    enh = np.floor(np.minimum(np.maximum(e, 0.0), 255.0) + 0.5).astype(np.uint8)
    enh = np.ascontiguousarray(np.moveaxis(enh, 0, 2))
    illu = None
    if illu_u8 is not None:
        top, left, nh, nw = content
        m = illu_u8[top:top + nh, left:left + nw, 0].astype(np.float64)
        illu = np.repeat(np.floor(_sample(m, H, W) + 0.5).astype(np.uint8)[:, :, None], 3, axis=2)
    cmp = None
    if comparison:
        cmp = np.concatenate([src_u8, enh] + ([illu] if comparison == 3 else []), axis=1)
    return enh, illu, cmp


def restore(src_u8, guide_u8, target_u8, illu_u8=None, content=None, radius=RADIUS, eps=EPS, comparison=None):
    """One image; the crop when the letterbox resized nothing."""
    top, left, nh, nw = content
    if (nh, nw) == src_u8.shape[:2]:
        def crop(a):
            return np.ascontiguousarray(a[top:top + nh, left:left + nw])
        enh = crop(target_u8)
        illu = crop(illu_u8) if illu_u8 is not None else None
        cmp = None
        if comparison:
            cmp = np.concatenate([crop(guide_u8), enh] + ([illu] if comparison == 3 else []), axis=1)
        return enh, illu, cmp
    return apply(src_u8, fit(guide_u8, target_u8, content, radius, eps), illu_u8, content, comparison)


def psnr_u8(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)
