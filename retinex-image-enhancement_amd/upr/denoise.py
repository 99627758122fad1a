"""Illumination-weighted non-local means on the u8 pixels of an output file.

The Retinex split brightens a pixel by roughly 1 / illumination and the sensor
noise with it, so nlm() filters every pixel with a strength of its own:
h = strength * 255 / max(illumination, floor) u8 levels (upr_denoise_lut /
upr_denoise_nlm_u8, csrc/denoise.hip; the integer arithmetic is stated in
include/upr.h and restated in numpy in tests/denoise_ref.py, byte for byte).
estimate_sigma() measures every image's noise level on the device (the median
Laplacian-difference estimator upr_noise_sigma_u8, csrc/noise.hip); nlm() takes
such a per-image tensor as its strength, and nlm_auto() chains the estimate,
the per-image tables (upr_denoise_lut_dev) and the filter
(upr_denoise_nlm_u8_luts) with no host copy (tests/noise_ref.py restates the
three, bit for bit).
Device only, like every other op of this package.
"""
import ctypes

import torch

from . import _lib as L
from .guided import _content, _u8_batch
from .runtime import _WS, _ptr, _require_device, _stream

DEFAULT_STRENGTH = 1.0
DEFAULT_FLOOR = 16
DEFAULT_SEARCH = 5
DEFAULT_PATCH = 2
AUTO = "auto"  # a strength: the image's own estimate_sigma() times auto_scale
DEFAULT_AUTO_SCALE = 1.0


def check_params(strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR, search=DEFAULT_SEARCH, patch=DEFAULT_PATCH,
                 auto_scale=DEFAULT_AUTO_SCALE):
    if isinstance(strength, str):
        if strength != AUTO:
            raise ValueError(f"denoise strength must be a finite number >= 0 or {AUTO!r}, got {strength!r}")
    else:
        s = float(strength)
        if not (s >= 0.0 and s != float("inf")):
            raise ValueError(f"denoise strength must be a finite number >= 0, got {strength!r}")
    g = float(auto_scale)
    if not (g >= 0.0 and g != float("inf")):
        raise ValueError(f"denoise auto scale must be a finite number >= 0, got {auto_scale!r}")
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


def _sigma_tensor(sigma, name):
    _require_device(sigma, name)
    if sigma.dtype != torch.float64 or sigma.dim() != 1 or sigma.shape[0] < 1:
        raise ValueError(f"{name} must be a float64 [B] tensor, got {sigma.dtype} {tuple(sigma.shape)}")
    return sigma.contiguous()


def lut_device(sigma, scale=DEFAULT_AUTO_SCALE, floor=DEFAULT_FLOOR, patch=DEFAULT_PATCH):
    """sigma: float64 [B] on the device -> the tables of upr_denoise_lut_dev, [B,256] on the
    device: row b is lut(scale * sigma[b], floor, patch), built there.  The uint32 entries are
    held in a torch.int32 tensor (the same bits)."""
    check_params(DEFAULT_STRENGTH, floor, DEFAULT_SEARCH, patch, scale)
    sigma = _sigma_tensor(sigma, "sigma")
    dev = sigma.device
    with torch.cuda.device(dev):
        tables = torch.empty((sigma.shape[0], 256), dtype=torch.int32, device=dev)
        rc = L.lib().upr_denoise_lut_dev(_ptr(sigma), sigma.shape[0], float(scale), int(floor), int(patch),
                                         _ptr(tables), _stream(dev))
    L.check(rc, "upr_denoise_lut_dev")
    return tables


def estimate_sigma(low_u8, content=None):
    """The noise std, in u8 levels, of every image of low_u8 (u8 [B,H,W,3] on the device: the
    low-light input's pixels, not the enhanced ones), measured inside the content rectangle
    -> float64 [B] on the device.  Nothing comes to the host."""
    low_u8 = _u8_batch(low_u8, "low_u8")
    B, H, W, _ = low_u8.shape
    top, left, nh, nw = _content(content if content is not None else (0, 0, H, W), H, W)
    dev = low_u8.device
    lib = L.lib()
    with torch.cuda.device(dev):
        sigma = torch.empty((B,), dtype=torch.float64, device=dev)
        ws = _WS.get(dev, lib.upr_noise_sigma_workspace(B))
        rc = lib.upr_noise_sigma_u8(_ptr(low_u8), B, H, W, top, left, nh, nw, _ptr(sigma), _ptr(ws),
                                    ctypes.c_size_t(ws.numel()), _stream(dev))
    L.check(rc, "upr_noise_sigma_u8")
    return sigma


def _nlm(src_u8, illu_u8, content, table, search, patch, out):
    """table: the ctypes array of lut() (one strength for the batch) or the [B,256] device
    tensor of lut_device() (a strength per image)."""
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
    per_image = isinstance(table, torch.Tensor)
    if per_image and (table.shape[0] != B or table.device != dev):
        raise ValueError(f"per-image strengths must be {B} values on {dev}, got {table.shape[0]} on {table.device}")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty_like(src_u8)
        else:
            _require_device(out, "out")
            if out.dtype != torch.uint8 or out.shape != src_u8.shape or out.device != dev or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous uint8 {tuple(src_u8.shape)} tensor on {dev}")
        if per_image:
            rc = L.lib().upr_denoise_nlm_u8_luts(_ptr(src_u8), _ptr(illu_u8), stride, B, H, W, top, left, nh, nw,
                                                 int(search), int(patch), _ptr(table), _ptr(out), _stream(dev))
        else:
            rc = L.lib().upr_denoise_nlm_u8(_ptr(src_u8), _ptr(illu_u8), stride, B, H, W, top, left, nh, nw,
                                            int(search), int(patch), table, _ptr(out), _stream(dev))
    L.check(rc, "upr_denoise_nlm_u8_luts" if per_image else "upr_denoise_nlm_u8")
    return out


def nlm(src_u8, illu_u8=None, content=None, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR, search=DEFAULT_SEARCH,
        patch=DEFAULT_PATCH, out=None):
    """src_u8: u8 [B,H,W,3] on the device; illu_u8: the illumination pixels u8 [B,H,W,3]
    (channel 0 is read) or [B,H,W], or None (no map: 255 everywhere); content: (top, left, nh,
    nw) from utils.letterbox.letterbox_content, None: the whole image -> a new u8 [B,H,W,3]
    tensor: the content rectangle filtered, the pixels outside it copied.  out: a u8 [B,H,W,3]
    tensor to write instead; it must not share memory with src_u8.  strength: one number for
    the batch, or a float64 [B] device tensor of per-image strengths (estimate_sigma's): the
    tables are then built on the device and nothing comes to the host."""
    if isinstance(strength, torch.Tensor):
        check_params(DEFAULT_STRENGTH, floor, search, patch)
        return _nlm(src_u8, illu_u8, content, lut_device(strength, 1.0, floor, patch), search, patch, out)
    if isinstance(strength, str):
        raise ValueError(f"nlm() takes a number or a per-image tensor as strength, got {strength!r}; "
                         "nlm_auto() measures it")
    check_params(strength, floor, search, patch)
    return _nlm(src_u8, illu_u8, content, lut(strength, floor, patch), search, patch, out)


def nlm_auto(src_u8, low_u8, illu_u8=None, content=None, scale=DEFAULT_AUTO_SCALE, floor=DEFAULT_FLOOR,
             search=DEFAULT_SEARCH, patch=DEFAULT_PATCH, out=None):
    """nlm() with the strength of image b measured: scale * estimate_sigma(low_u8, content)[b].
    src_u8: the enhanced pixels to filter; low_u8: the low-light input's pixels, the same
    [B,H,W,3].  Three launches on the current stream (the estimate, the tables, the filter);
    nothing comes to the host."""
    check_params(AUTO, floor, search, patch, scale)
    if tuple(low_u8.shape) != tuple(src_u8.shape) or low_u8.device != src_u8.device:
        raise ValueError(f"low_u8 must be like src_u8, {tuple(src_u8.shape)} on {src_u8.device}, got "
                         f"{tuple(low_u8.shape)} on {low_u8.device}")
    tables = lut_device(estimate_sigma(low_u8, content), scale, floor, patch)
    return _nlm(src_u8, illu_u8, content, tables, search, patch, out)
