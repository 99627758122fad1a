"""Device-side PNG encoder (include/upr.h upr_png_encode): u8 RGB images that are
already on the device become complete PNG files there -- filters, deflate in
independent strips, CRC-32 and Adler-32 -- and the host only copies `size`
bytes per image and writes them.

Files are lossless and decode anywhere.  matches="none" (the default) is
Huffman-only deflate, so the files are larger than PIL's; matches="lz" adds
greedy LZ77 matching inside each strip and writes every strip in the smallest
of the matched, the Huffman-only and the stored form, so no file grows (see
DESIGN.md "Device PNG encoder" for measured sizes and times).
"""
import ctypes

import torch

from . import _lib as L
from .runtime import _Workspace, _ptr, _require_device, _stream

FILTERS = tuple(L.PNG_FILTERS)
MATCHES = tuple(L.PNG_MATCHES)
DEFAULT_ROWS_PER_STRIP = 16

_ws = _Workspace()


def bound(H, W, rows_per_strip=None, matches="none"):
    """(largest file of one H x W image, scratch bytes per image); ValueError for a shape the
    encoder refuses (rows_per_strip * (3W + 1) > 2^24, or a file bound above 2^31 bytes)."""
    match = _match(matches)
    rps = _rows_per_strip(H, rows_per_strip)
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    rc = L.lib().upr_png_bound_ex(int(H), int(W), rps, match, ctypes.byref(nb), ctypes.byref(ns))
    _check(rc, "upr_png_bound_ex", H, W, rps)
    return nb.value, ns.value


def _match(matches):
    if matches not in L.PNG_MATCHES:
        raise ValueError(f"matches must be one of {MATCHES}, got {matches!r}")
    return L.PNG_MATCHES[matches]


def _rows_per_strip(H, rows_per_strip):
    rps = DEFAULT_ROWS_PER_STRIP if rows_per_strip is None else int(rows_per_strip)
    if rps < 1:
        raise ValueError(f"rows_per_strip must be >= 1, got {rows_per_strip}")
    return min(rps, max(int(H), 1))


def _check(rc, what, H, W, rps):
    if rc == L.UPR_ERR_SHAPE:
        raise ValueError(f"{what}: a {H}x{W} image in strips of {rps} rows is over the encoder's limits "
                         f"(rows_per_strip * (3W + 1) <= {L.UPR_PNG_MAX_STRIP_BYTES}, file bound <= 2^31 bytes; "
                         f"status {rc})")
    L.check(rc, what)


def encode_device(x, filter="adaptive", rows_per_strip=None, matches="none"):
    """x: u8 [H,W,3] or [B,H,W,3] on the device -> (buf u8 [B, stride], sizes int64 [B]), both on
    the device: image b's file is buf[b, :sizes[b]].  Queued on the current stream; no
    synchronisation."""
    match = _match(matches)
    _require_device(x)
    if x.dtype != torch.uint8 or x.dim() not in (3, 4) or x.shape[-1] != 3:
        raise TypeError(f"PNG input must be uint8 [H,W,3] or [B,H,W,3], got {x.dtype} {tuple(x.shape)}")
    if filter not in L.PNG_FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, got {filter!r}")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    B, H, W, _ = x.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"empty image batch {tuple(x.shape)}")
    rps = _rows_per_strip(H, rows_per_strip)
    per_image, scratch_image = bound(H, W, rps, matches)
    x = x.contiguous()
    stride = (per_image + 15) // 16 * 16
    buf = torch.empty((B, stride), dtype=torch.uint8, device=x.device)
    sizes = torch.empty((B,), dtype=torch.int64, device=x.device)
    scratch = _ws.get(x.device, B * scratch_image)
    with torch.cuda.device(x.device):
        rc = L.lib().upr_png_encode_ex(_ptr(x), B, H, W, L.PNG_FILTERS[filter], match, rps, _ptr(buf), stride,
                                       _ptr(sizes), _ptr(scratch), B * scratch_image, _stream(x.device))
    _check(rc, "upr_png_encode_ex", H, W, rps)
    return buf, sizes


def encode(x, filter="adaptive", rows_per_strip=None, matches="none"):
    """PNG file bytes of each image of x (u8 [H,W,3] or [B,H,W,3] on the device) -> list[bytes].
    One copy of `sizes`, then only sizes[b] bytes per image."""
    buf, sizes = encode_device(x, filter, rows_per_strip, matches)
    return [buf[b, :n].cpu().numpy().tobytes() for b, n in enumerate(sizes.tolist())]
