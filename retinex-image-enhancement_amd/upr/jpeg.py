"""Device-side JPEG encoder (include/upr.h upr_jpeg_encode): u8 RGB images that are already
on the device become complete baseline JPEG files there -- colour conversion, forward DCT,
quantisation, Huffman coding with the Annex K tables, byte stuffing and restart markers -- and
the host only copies `size` bytes per image and writes them.

Files are 8-bit Y/Cb/Cr 4:4:4 (no chroma subsampling), `quality` means what PIL's `quality`
means, and one restart interval covers `restart_rows` rows of 8x8 blocks.  Not built: 4:2:0,
Huffman tables optimised per image, grayscale files (see DESIGN.md "Device JPEG encoder" for
the exact arithmetic, measured sizes and times).
"""
import ctypes

import torch

from . import _lib as L
from .runtime import _Workspace, _ptr, _require_device, _stream

DEFAULT_RESTART_ROWS = 1

_ws = _Workspace()


def _restart_rows(restart_rows):
    rr = DEFAULT_RESTART_ROWS if restart_rows is None else int(restart_rows)
    if rr < 1:
        raise ValueError(f"restart_rows must be >= 1, got {restart_rows}")
    return rr


def _quality(quality):
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality must be in 1..100, got {quality}")
    return q


def _check(rc, what, H, W, rr):
    if rc == L.UPR_ERR_SHAPE:
        raise ValueError(f"{what}: a {H}x{W} image in restart intervals of {rr} block rows is over the encoder's "
                         f"limits (H, W <= 65535, ceil(W / 8) * restart_rows <= 65535, file bound <= 2^31 bytes; "
                         f"status {rc})")
    L.check(rc, what)


def bound(H, W, restart_rows=None):
    """(largest file of one H x W image, scratch bytes per image); ValueError for a shape the
    encoder refuses (H or W above 65535, ceil(W / 8) * restart_rows above 65535, or a file bound
    above 2^31 bytes)."""
    rr = _restart_rows(restart_rows)
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    rc = L.lib().upr_jpeg_bound(int(H), int(W), rr, ctypes.byref(nb), ctypes.byref(ns))
    _check(rc, "upr_jpeg_bound", H, W, rr)
    return nb.value, ns.value


def encode_device(x, quality=95, restart_rows=None):
    """x: u8 [H,W,3] or [B,H,W,3] on the device -> (buf u8 [B, stride], sizes int64 [B]), both on
    the device: image b's file is buf[b, :sizes[b]].  Queued on the current stream; no
    synchronisation."""
    q = _quality(quality)
    rr = _restart_rows(restart_rows)
    _require_device(x)
    if x.dtype != torch.uint8 or x.dim() not in (3, 4) or x.shape[-1] != 3:
        raise TypeError(f"JPEG input must be uint8 [H,W,3] or [B,H,W,3], got {x.dtype} {tuple(x.shape)}")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    B, H, W, _ = x.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"empty image batch {tuple(x.shape)}")
    per_image, scratch_image = bound(H, W, rr)
    x = x.contiguous()
    stride = (per_image + 15) // 16 * 16
    buf = torch.empty((B, stride), dtype=torch.uint8, device=x.device)
    sizes = torch.empty((B,), dtype=torch.int64, device=x.device)
    scratch = _ws.get(x.device, B * scratch_image)
    with torch.cuda.device(x.device):
        rc = L.lib().upr_jpeg_encode(_ptr(x), B, H, W, q, rr, _ptr(buf), stride, _ptr(sizes), _ptr(scratch),
                                     B * scratch_image, _stream(x.device))
    _check(rc, "upr_jpeg_encode", H, W, rr)
    return buf, sizes


def encode(x, quality=95, restart_rows=None):
    """JPEG file bytes of each image of x (u8 [H,W,3] or [B,H,W,3] on the device) -> list[bytes].
    One copy of `sizes`, then only sizes[b] bytes per image."""
    buf, sizes = encode_device(x, quality, restart_rows)
    return [buf[b, :n].cpu().numpy().tobytes() for b, n in enumerate(sizes.tolist())]
