"""Guided-filter restore: the letterboxed result carried to the source's size.

The fast guided filter (He & Sun 2015), per channel: fit() fits the local
affine model target ~ a * guide + b between the letterboxed input and the
letterboxed result (u8 pixels as the output files hold them, content rectangle
only) and returns the window means of a and b; apply() samples them bilinearly
at every full-resolution pixel and applies them to the source's bytes
(upr_guided_fit / upr_guided_apply, csrc/guided.hip; the arithmetic is stated
in include/upr.h and restated in numpy in tests/guided_ref.py, byte for byte).
restore() does both, or crops the content rectangle when nothing was resized.
Device only, like every other op of this package.
"""
import ctypes

import torch

from . import _lib as L
from .runtime import _WS, _ptr, _require_device, _stream

DEFAULT_RADIUS = 4
DEFAULT_EPS = 1e-4


def check_params(radius, eps):
    if not 1 <= int(radius) <= 32:
        raise ValueError(f"guided radius must be in 1..32, got {radius!r}")
    if not float(eps) > 0.0:
        raise ValueError(f"guided eps must be > 0, got {eps!r}")


def _content(content, Hl, Wl):
    top, left, nh, nw = (int(v) for v in content)
    if nh < 1 or nw < 1 or top < 0 or left < 0 or top + nh > Hl or left + nw > Wl:
        raise ValueError(f"content rectangle {(top, left, nh, nw)} lies outside {Hl} x {Wl}")
    return top, left, nh, nw


def _u8_batch(t, name):
    _require_device(t, name)
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
        raise ValueError(f"{name} must be a uint8 [B, H, W, 3] tensor, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def fit(guide_u8, target_u8, content, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS):
    """guide_u8, target_u8: u8 [B,Hl,Wl,3] on the device; content: (top, left, nh, nw)
    -> ab float64 [B,2,3,nh,nw] (the coefficient maps A, then B)."""
    check_params(radius, eps)
    guide_u8, target_u8 = _u8_batch(guide_u8, "guide_u8"), _u8_batch(target_u8, "target_u8")
    if guide_u8.shape != target_u8.shape or guide_u8.device != target_u8.device:
        raise ValueError(f"guide {tuple(guide_u8.shape)} and target {tuple(target_u8.shape)} differ")
    B, Hl, Wl, _ = guide_u8.shape
    top, left, nh, nw = _content(content, Hl, Wl)
    dev = guide_u8.device
    lib = L.lib()
    with torch.cuda.device(dev):
        ab = torch.empty((B, 2, 3, nh, nw), dtype=torch.float64, device=dev)
        ws = _WS.get(dev, lib.upr_guided_fit_workspace(B, nh, nw))
        rc = lib.upr_guided_fit(_ptr(guide_u8), _ptr(target_u8), B, Hl, Wl, top, left, nh, nw, int(radius),
                                float(eps), _ptr(ab), _ptr(ws), ctypes.c_size_t(ws.numel()), _stream(dev))
    L.check(rc, "upr_guided_fit")
    return ab


def _sources(src_u8):
    """(tensor to keep alive, base address, byte stride, B, H, W) of a u8 [B,H,W,3] tensor or of
    the staged sources letterbox_u8_batch(return_sources=True) hands back."""
    if hasattr(src_u8, "buf"):
        H, W = src_u8.shape
        _require_device(src_u8.buf, "src_u8")
        if src_u8.stride < H * W * 3 or src_u8.buf.numel() < (src_u8.count - 1) * src_u8.stride + H * W * 3:
            raise ValueError("staged sources: the buffer does not hold count images at that stride")
        return src_u8.buf, src_u8.buf.data_ptr(), int(src_u8.stride), int(src_u8.count), int(H), int(W)
    t = _u8_batch(src_u8, "src_u8")
    B, H, W, _ = t.shape
    return t, t.data_ptr(), H * W * 3, B, H, W


def apply(src_u8, ab, illu_u8=None, content=None, comparison=None):
    """src_u8: u8 [B,H,W,3] on the device (or staged sources); ab from fit(); illu_u8: the
    letterboxed illumination pixels u8 [B,Hl,Wl,3] or None; content: the (top, left, nh, nw)
    fit() was given -> (enh_u8 [B,H,W,3], illu_u8 [B,H,W,3] or None, cmp_u8
    [B,H,comparison*W,3] or None): [src | enh] (comparison=2) or [src | enh | illu] (3)."""
    if comparison not in (None, 2, 3):
        raise ValueError(f"comparison must be None, 2 or 3, got {comparison!r}")
    if comparison == 3 and illu_u8 is None:
        raise ValueError("comparison=3 needs the illumination map")
    keep, base, stride, B, H, W = _sources(src_u8)
    _require_device(ab, "ab")
    if ab.dtype != torch.float64 or ab.dim() != 5 or tuple(ab.shape[:3]) != (B, 2, 3):
        raise ValueError(f"ab must be float64 [{B}, 2, 3, nh, nw], got {ab.dtype} {tuple(ab.shape)}")
    ab = ab.contiguous()
    nh, nw = int(ab.shape[3]), int(ab.shape[4])
    if illu_u8 is not None:
        illu_u8 = _u8_batch(illu_u8, "illu_u8")
        if illu_u8.shape[0] != B:
            raise ValueError(f"illu_u8 holds {illu_u8.shape[0]} images, the sources {B}")
        Hl, Wl = int(illu_u8.shape[1]), int(illu_u8.shape[2])
        if content is None:
            raise ValueError("content is required with illu_u8")
        top, left, ch, cw = _content(content, Hl, Wl)
        if (ch, cw) != (nh, nw):
            raise ValueError(f"content {(ch, cw)} is not ab's {(nh, nw)}")
    else:
        top, left, Hl, Wl = 0, 0, nh, nw
    if nh > H or nw > W:
        raise ValueError(f"coefficients {nh} x {nw} are larger than the source {H} x {W}")
    dev = ab.device
    with torch.cuda.device(dev):
        enh = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        illu = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) if illu_u8 is not None else None
        cmp = torch.empty((B, H, comparison * W, 3), dtype=torch.uint8, device=dev) if comparison else None
        rc = L.lib().upr_guided_apply(ctypes.c_void_p(base), ctypes.c_size_t(stride), B, H, W, _ptr(ab),
                                      _ptr(illu_u8), Hl, Wl, top, left, nh, nw, _ptr(enh), _ptr(illu), _ptr(cmp),
                                      comparison or 0, _stream(dev))
    L.check(rc, "upr_guided_apply")
    del keep
    return enh, illu, cmp


def restore(src_u8, guide_u8, target_u8, illu_u8=None, content=None, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS,
            comparison=None):
    """The three output images at the source's size: src_u8 as for apply(); guide_u8 /
    target_u8 / illu_u8 the letterboxed input / result / illumination pixels u8 [B,Hl,Wl,3];
    content from utils.letterbox.letterbox_content.  When the letterbox resized nothing
    ((nh, nw) == (H, W)) there is no filter: the outputs are the content rectangle of the
    letterboxed pixels, byte for byte."""
    check_params(radius, eps)
    if comparison not in (None, 2, 3):
        raise ValueError(f"comparison must be None, 2 or 3, got {comparison!r}")
    if comparison == 3 and illu_u8 is None:
        raise ValueError("comparison=3 needs the illumination map")
    guide_u8 = _u8_batch(guide_u8, "guide_u8")
    top, left, nh, nw = _content(content, guide_u8.shape[1], guide_u8.shape[2])
    _, _, _, B, H, W = _sources(src_u8)
    if (nh, nw) == (H, W):
        def crop(t):
            return t[:, top:top + nh, left:left + nw]
        enh = crop(_u8_batch(target_u8, "target_u8")).contiguous()
        illu = crop(_u8_batch(illu_u8, "illu_u8")).contiguous() if illu_u8 is not None else None
        cmp = None
        if comparison:
            cmp = torch.cat([crop(guide_u8), enh] + ([illu] if comparison == 3 else []), dim=2).contiguous()
        return enh, illu, cmp
    ab = fit(guide_u8, target_u8, (top, left, nh, nw), radius, eps)
    return apply(src_u8, ab, illu_u8, (top, left, nh, nw), comparison)
