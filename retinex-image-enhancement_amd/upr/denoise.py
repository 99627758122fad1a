"""Illumination-weighted non-local means on the u8 pixels of an output file.

The Retinex split brightens a pixel by roughly 1 / illumination and the sensor
noise with it, so nlm() filters every pixel with a strength of its own:
h = strength * 255 / max(illumination, floor) u8 levels (upr_denoise_lut /
upr_denoise_nlm_u8, csrc/denoise.hip; the integer arithmetic is stated in
include/upr.h and restated in numpy in tests/denoise_ref.py, byte for byte).
Device only, like every other op of this package.
"""
import ctypes

import torch

from . import _lib as L
from .guided import _content, _u8_batch
from .runtime import _ptr, _require_device, _stream

DEFAULT_STRENGTH = 1.0
DEFAULT_FLOOR = 16
DEFAULT_SEARCH = 5
DEFAULT_PATCH = 2


def check_params(strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR, search=DEFAULT_SEARCH, patch=DEFAULT_PATCH):
    s = float(strength)
    if not (s >= 0.0 and s != float("inf")):
        raise ValueError(f"denoise strength must be a finite number >= 0, got {strength!r}")
    if not 1 <= int(floor) <= 255:
        raise ValueError(f"denoise floor must be in 1..255, got {floor!r}")
    if not 1 <= int(search) <= 10:
        raise ValueError(f"denoise search radius must be in 1..10, got {search!r}")
    if not 1 <= int(patch) <= 3:
        raise ValueError(f"denoise patch radius must be in 1..3, got {patch!r}")


def lut(strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR, patch=DEFAULT_PATCH):
    """The strength table of upr_denoise_lut: a ctypes array of 256 uint32 (host; no device call)."""
    check_params(strength, floor, DEFAULT_SEARCH, patch)
    table = (ctypes.c_uint32 * 256)()
    L.check(L.lib().upr_denoise_lut(float(strength), int(floor), int(patch), table), "upr_denoise_lut")
    return table


def nlm(src_u8, illu_u8=None, content=None, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR, search=DEFAULT_SEARCH,
        patch=DEFAULT_PATCH, out=None):
    """src_u8: u8 [B,H,W,3] on the device; illu_u8: the illumination pixels u8 [B,H,W,3]
    (channel 0 is read) or [B,H,W], or None (no map: 255 everywhere); content: (top, left, nh,
    nw) from utils.letterbox.letterbox_content, None: the whole image -> a new u8 [B,H,W,3]
    tensor: the content rectangle filtered, the pixels outside it copied.  out: a u8 [B,H,W,3]
    tensor to write instead; it must not share memory with src_u8."""
    check_params(strength, floor, search, patch)
    src_u8 = _u8_batch(src_u8, "src_u8")
    B, H, W, _ = src_u8.shape
    top, left, nh, nw = _content(content if content is not None else (0, 0, H, W), H, W)
    dev = src_u8.device
    stride = 0
    if illu_u8 is not None:
        _require_device(illu_u8, "illu_u8")
        shape = tuple(illu_u8.shape)
        if illu_u8.dtype != torch.uint8 or illu_u8.device != dev or shape not in ((B, H, W), (B, H, W, 3)):
            raise ValueError(f"illu_u8 must be a uint8 [{B}, {H}, {W}] or [{B}, {H}, {W}, 3] tensor on {dev}, got "
                             f"{illu_u8.dtype} {shape} on {illu_u8.device}")
        illu_u8 = illu_u8.contiguous()
        stride = 3 if illu_u8.dim() == 4 else 1
    table = lut(strength, floor, patch)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty_like(src_u8)
        else:
            _require_device(out, "out")
            if out.dtype != torch.uint8 or out.shape != src_u8.shape or out.device != dev or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous uint8 {tuple(src_u8.shape)} tensor on {dev}")
        rc = L.lib().upr_denoise_nlm_u8(_ptr(src_u8), _ptr(illu_u8), stride, B, H, W, top, left, nh, nw, int(search),
                                        int(patch), table, _ptr(out), _stream(dev))
    L.check(rc, "upr_denoise_nlm_u8")
    return out
