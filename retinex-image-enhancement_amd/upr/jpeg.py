"""Device-side JPEG encoder (include/upr.h upr_jpeg_encode_ex): u8 RGB images that are already
on the device become complete baseline JPEG files there -- colour conversion, forward DCT,
quantisation, Huffman coding, byte stuffing and restart markers -- and the host only copies
`size` bytes per image and writes them.

Files are 8-bit; `quality` means what PIL's `quality` means, and one restart interval covers
`restart_rows` rows of MCUs.  `subsampling` is "444" (Y/Cb/Cr, no chroma subsampling: the
default, PIL's subsampling=0), "420" (chroma halved both ways with a 2x2 box, 16x16-pixel MCUs:
PIL's subsampling=2) or "gray" (a one-component file of the input's luma: PIL's mode "L").
`optimize=True` builds the Huffman tables from each image's own symbol counts on the device
(PIL's optimize=True) in place of the Annex K tables; the pixels a decoder gets are the same.
huffman_build() runs the table routine alone on given counts.  Not built: 4:2:2, progressive
scans, arithmetic coding (see DESIGN.md "Device JPEG encoder" for the exact arithmetic,
measured sizes and times).
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


def _modes(subsampling, optimize):
    if subsampling not in L.JPEG_SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {sorted(L.JPEG_SUBSAMPLINGS)}, got {subsampling!r}")
    return L.JPEG_SUBSAMPLINGS[subsampling], L.JPEG_HUFFMAN["optimized" if optimize else "standard"]


def _check(rc, what, H, W, rr):
    if rc == L.UPR_ERR_SHAPE:
        raise ValueError(f"{what}: a {H}x{W} image in restart intervals of {rr} MCU rows is over the encoder's "
                         f"limits (H, W <= 65535, MCUs per row * restart_rows <= 65535, file bound <= 2^31 bytes; "
                         f"status {rc})")
    L.check(rc, what)


def bound(H, W, restart_rows=None, subsampling="444", optimize=False):
    """(largest file of one H x W image, scratch bytes per image); ValueError for a shape the
    encoder refuses (H or W above 65535, MCUs per row * restart_rows above 65535, or a file bound
    above 2^31 bytes)."""
    rr = _restart_rows(restart_rows)
    sub, huff = _modes(subsampling, optimize)
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    rc = L.lib().upr_jpeg_bound_ex(int(H), int(W), rr, sub, huff, ctypes.byref(nb), ctypes.byref(ns))
    _check(rc, "upr_jpeg_bound_ex", H, W, rr)
    return nb.value, ns.value


def encode_device(x, quality=95, restart_rows=None, subsampling="444", optimize=False):
    """x: u8 [H,W,3] or [B,H,W,3] on the device -> (buf u8 [B, stride], sizes int64 [B]), both on
    the device: image b's file is buf[b, :sizes[b]].  Queued on the current stream; no
    synchronisation."""
    q = _quality(quality)
    rr = _restart_rows(restart_rows)
    sub, huff = _modes(subsampling, optimize)
    _require_device(x)
    if x.dtype != torch.uint8 or x.dim() not in (3, 4) or x.shape[-1] != 3:
        raise TypeError(f"JPEG input must be uint8 [H,W,3] or [B,H,W,3], got {x.dtype} {tuple(x.shape)}")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    B, H, W, _ = x.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"empty image batch {tuple(x.shape)}")
    per_image, scratch_image = bound(H, W, rr, subsampling, optimize)
    x = x.contiguous()
    stride = (per_image + 15) // 16 * 16
    buf = torch.empty((B, stride), dtype=torch.uint8, device=x.device)
    sizes = torch.empty((B,), dtype=torch.int64, device=x.device)
    scratch = _ws.get(x.device, B * scratch_image)
    with torch.cuda.device(x.device):
        rc = L.lib().upr_jpeg_encode_ex(_ptr(x), B, H, W, q, rr, sub, huff, _ptr(buf), stride, _ptr(sizes),
                                        _ptr(scratch), B * scratch_image, _stream(x.device))
    _check(rc, "upr_jpeg_encode_ex", H, W, rr)
    return buf, sizes


def encode(x, quality=95, restart_rows=None, subsampling="444", optimize=False):
    """JPEG file bytes of each image of x (u8 [H,W,3] or [B,H,W,3] on the device) -> list[bytes].
    One copy of `sizes`, then only sizes[b] bytes per image."""
    buf, sizes = encode_device(x, quality, restart_rows, subsampling, optimize)
    return [buf[b, :n].cpu().numpy().tobytes() for b, n in enumerate(sizes.tolist())]


def huffman_build(freq):
    """Huffman tables of symbol counts, by the routine the encoder's optimize=True runs.
    freq: integer counts [256], [257], [n,256] or [n,257] (entry 256 is ignored), any device;
    counts must fit 32 bits.  -> list of (bits: tuple of 16, vals: tuple of the coded symbols)
    per table, or the one pair for a 1-D freq."""
    f = torch.as_tensor(freq)
    single = f.dim() == 1
    if single:
        f = f.unsqueeze(0)
    if f.dim() != 2 or f.shape[0] < 1 or f.shape[1] not in (256, 257) or f.is_floating_point():
        raise TypeError(f"freq must be integer counts [256 or 257] or [n, 256 or 257], got {f.dtype} {tuple(f.shape)}")
    f = f.to(torch.int64)
    if int(f.min()) < 0 or int(f.max()) >= 1 << 32:
        raise ValueError("counts must be in 0 .. 2^32 - 1")
    dev = f.device if f.is_cuda else torch.device("cuda", torch.cuda.current_device())
    n = f.shape[0]
    f32 = torch.zeros((n, 257), dtype=torch.int64, device=dev)
    f32[:, :f.shape[1]] = f.to(dev)
    # the u32 counts as the low words of little-endian int64
    f32 = f32.view(torch.int32)[:, 0::2].contiguous()
    out = torch.empty((n, 16 + 256), dtype=torch.uint8, device=dev)
    nvals = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().upr_jpeg_huffman_build(_ptr(f32), n, _ptr(out), _ptr(nvals), _stream(dev)),
                "upr_jpeg_huffman_build")
    out, nvals = out.cpu().numpy(), nvals.tolist()
    tables = [(tuple(int(v) for v in out[t, :16]), tuple(int(v) for v in out[t, 16:16 + nvals[t]])) for t in range(n)]
    return tables[0] if single else tables
