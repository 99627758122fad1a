"""Tensor-level wrappers over libupr.so.

PyTorch is used only for device memory and streams: every compute call goes
through the C ABI with raw device pointers and the caller's current HIP stream.
Non-ROCm tensors are rejected (no CPU fallback).
"""
import ctypes

import torch

from . import _lib as L

_DT = {torch.float32: L.UPR_F32, torch.float16: L.UPR_F16}


def dtype_code(dt):
    if dt not in _DT:
        raise TypeError(f"UP-Retinex HIP path supports float32 and float16 tensors, got {dt}")
    return _DT[dt]


def _require_device(t, name="input"):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise RuntimeError(
            f"{name} is on '{t.device}': the UP-Retinex framework executes on ROCm devices only "
            f"(MI355X HIP kernels); move the model and the tensor to a 'cuda' (ROCm) device")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _Workspace:
    """Grow-only scratch buffer per (device, HIP stream), torch-allocated.

    Keyed by the caller's current stream: work issued on two streams never
    shares scratch, and a buffer is allocated on (and, when it grows, released
    to torch's caching allocator from) the stream that uses it, so the
    allocator's stream ordering keeps a replaced buffer alive until the work
    queued on that stream has drained (include/upr.h: thread-safe across
    distinct handles or streams).  At most MAX_STREAMS buffers are kept (least
    recently used evicted), so code that makes a new stream per request does
    not pin a buffer per stream; an evicted buffer returns to torch's caching
    allocator, which reuses it on its own stream only (stream-ordered safe)."""

    MAX_STREAMS = 8

    def __init__(self):
        from collections import OrderedDict
        self.buf = OrderedDict()

    def get(self, dev, nbytes):
        stream = torch.cuda.current_stream(dev)
        key = (dev.type, dev.index, stream.cuda_stream)
        b = self.buf.pop(key, None)
        if b is None or b.numel() < nbytes:
            with torch.cuda.stream(stream):
                b = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
        self.buf[key] = b  # most recently used last
        while len(self.buf) > self.MAX_STREAMS:
            self.buf.popitem(last=False)
        return b


_WS = _Workspace()


class ModelHandle:
    """Owns one UprModel* (packed device weights) built from a state_dict."""

    def __init__(self, state_dict, use_preact, use_aspp, dtype, device, ienet_only=False, prefix="", head_only=False):
        lib = L.lib()
        self.dtype = dtype
        self.device = device
        self.ienet_only = ienet_only
        self.head_only = head_only
        names, descs, keep = [], [], []
        for k, v in state_dict.items():
            if not torch.is_floating_point(v):
                continue  # num_batches_tracked
            t = v.detach().to("cpu", torch.float32).contiguous()
            keep.append(t)
            nm = (prefix + k).encode()
            names.append(nm)
            d = L.UprTensorDesc()
            d.name = nm
            d.data = ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))
            d.ndim = t.dim()
            for i, s in enumerate(t.shape):
                d.shape[i] = s
            descs.append(d)
        arr = (L.UprTensorDesc * len(descs))(*descs)
        out = ctypes.c_void_p()
        flags = (L.UPR_MODEL_IENET_ONLY if ienet_only else 0) | (L.UPR_MODEL_HEAD_ONLY if head_only else 0)
        with torch.cuda.device(device):
            rc = lib.upr_model_create(arr, len(descs), int(bool(use_preact)), int(bool(use_aspp)),
                                      dtype_code(dtype), flags, ctypes.byref(out))
        L.check(rc, "upr_model_create")
        self._h = out
        self._lib = lib

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and h.value:
            try:
                self._lib.upr_model_destroy(h)
            except Exception:
                pass
            self._h = None

    def profile(self, enable=True):
        """Record a HIP event pair around every op of later forwards."""
        L.check(self._lib.upr_model_profile(self._h, int(bool(enable))), "upr_model_profile")

    def forks(self):
        """Forwards so far that ran the two-stream (multi-scale side stream) schedule."""
        return int(self._lib.upr_model_forks(self._h))

    def split_state(self):
        """Split-fp16 region of an fp32 model: 0 off, 1 active, 2 disabled after a range overflow."""
        return int(self._lib.upr_model_split_state(self._h))

    def op_forms(self):
        """(name, form) per op of the most recent forward, in launch order: 0 the
        model dtype's own kernels, 1 split-fp16 tensors, 2 split in registers, 3
        weights split once."""
        n = int(self._lib.upr_model_op_forms(self._h, None, 0))
        arr = (L.UprOpForm * max(n, 1))()
        n = int(self._lib.upr_model_op_forms(self._h, arr, n))
        return [(a.name.decode(), int(a.form)) for a in arr[:n]]

    def profile_read(self):
        """Per-op stats (launch order): list of dicts name/kind/calls/ms/flops/bytes."""
        n = ctypes.c_int(0)
        L.check(self._lib.upr_model_profile_read(self._h, None, 0, ctypes.byref(n)), "upr_model_profile_read")
        arr = (L.UprOpStat * max(n.value, 1))()
        L.check(self._lib.upr_model_profile_read(self._h, arr, n.value, ctypes.byref(n)), "upr_model_profile_read")
        return [{"name": a.name.decode(), "kind": "conv_igemm" if a.kind == L.UPR_OP_CONV_IGEMM else "other",
                 "calls": a.calls, "ms": a.ms, "flops": a.flops, "bytes": a.bytes} for a in arr[:n.value]]

    def enhance(self, x, refl):
        """HEAD_ONLY handle: multi_scale_enhance(x, refl) -> enhanced [B,3,H,W]."""
        _require_device(x)
        _require_device(refl, "reflectance")
        if x.dim() != 4 or x.shape[1] != 3 or refl.shape != x.shape:
            raise RuntimeError(f"expected x and reflectance of one shape [B, 3, H, W], got {tuple(x.shape)} and "
                               f"{tuple(refl.shape)}")
        if x.dtype != self.dtype or refl.dtype != self.dtype:
            raise RuntimeError(f"input dtypes {x.dtype}/{refl.dtype} do not match model dtype {self.dtype}")
        x, refl = x.contiguous(), refl.contiguous()
        B, _, H, W = x.shape
        dev = x.device
        with torch.cuda.device(dev):
            enh = torch.empty_like(x)
            nbytes = self._lib.upr_model_workspace(self._h, B, H, W)
            ws = _WS.get(dev, nbytes)
            rc = self._lib.upr_model_forward(self._h, _ptr(x), B, H, W, _ptr(enh), _ptr(refl), None,
                                             _ptr(ws), ctypes.c_size_t(ws.numel()), _stream(dev))
        L.check(rc, "upr_model_forward(head only)")
        return enh

    def forward(self, x):
        _require_device(x)
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"expected input of shape [B, 3, H, W], got {tuple(x.shape)}")
        if x.dtype != self.dtype:
            raise RuntimeError(f"input dtype {x.dtype} does not match model dtype {self.dtype}")
        x = x.contiguous()
        B, _, H, W = x.shape
        dev = x.device
        with torch.cuda.device(dev):
            illu = torch.empty((B, 1, H, W), dtype=x.dtype, device=dev)
            if self.ienet_only:
                enh = refl = None
            else:
                enh = torch.empty((B, 3, H, W), dtype=x.dtype, device=dev)
                refl = torch.empty_like(enh)
            nbytes = self._lib.upr_model_workspace(self._h, B, H, W)
            ws = _WS.get(dev, nbytes)
            rc = self._lib.upr_model_forward(self._h, _ptr(x), B, H, W, _ptr(enh), _ptr(refl), _ptr(illu),
                                             _ptr(ws), ctypes.c_size_t(ws.numel()), _stream(dev))
        L.check(rc, "upr_model_forward")
        return enh, refl, illu


# ---------------------------------------------------------------------------
# enhancer / op wrappers
# ---------------------------------------------------------------------------
def clahe_enhance(enh, clip=2.0, tiles=(8, 8)):
    """Batched apply_clahe_enhancement: [B,3,H,W] float -> [B,3,H,W] float."""
    _require_device(enh)
    enh = enh.contiguous()
    B, C, H, W = enh.shape
    if C != 3:
        raise RuntimeError("clahe_enhance expects 3 channels")
    lib = L.lib()
    out = torch.empty_like(enh)
    with torch.cuda.device(enh.device):
        ws = _WS.get(enh.device, lib.upr_clahe_enhance_workspace(B, H, W, tiles[0], tiles[1]))
        rc = lib.upr_clahe_enhance(_ptr(enh), _ptr(out), _ptr(ws), B, H, W, float(clip), int(tiles[0]),
                                   int(tiles[1]), dtype_code(enh.dtype), _stream(enh.device))
    L.check(rc, "upr_clahe_enhance")
    return out


def gray_hist(x):
    _require_device(x)
    x = x.contiguous()
    B, C, H, W = x.shape
    hist = torch.empty((B, 256), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.lib().upr_gray_hist(_ptr(x), _ptr(hist), B, H, W, dtype_code(x.dtype), _stream(x.device))
    L.check(rc, "upr_gray_hist")
    return hist


def multiscale(x, enh=None):
    """Returns (out or None, factor[B] float64, sums[B,3] float64)."""
    _require_device(x)
    x = x.contiguous()
    B, C, H, W = x.shape
    sums = torch.empty((B, 3), dtype=torch.float64, device=x.device)
    factor = torch.empty((B,), dtype=torch.float64, device=x.device)
    out = None
    if enh is not None:
        enh = enh.contiguous()
        if enh.shape != x.shape or enh.dtype != x.dtype:
            raise RuntimeError("multiscale: enhanced image must match the input's shape and dtype")
        out = torch.empty_like(enh)
    with torch.cuda.device(x.device):
        rc = L.lib().upr_multiscale(_ptr(x), _ptr(enh), _ptr(out), _ptr(sums), _ptr(factor), B, H, W,
                                    dtype_code(x.dtype), _stream(x.device))
    L.check(rc, "upr_multiscale")
    return out, factor, sums


def quantize_u8(x):
    _require_device(x)
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.lib().upr_quantize_u8(_ptr(x), _ptr(out), x.numel(), dtype_code(x.dtype), _stream(x.device))
    L.check(rc, "upr_quantize_u8")
    return out


def to_u8_hwc(x):
    """save_image pixels: one [C,H,W] image (C 1 or 3) -> u8 [H,W,3] on the device."""
    _require_device(x)
    x = x.contiguous()
    C, H, W = x.shape
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.lib().upr_to_u8_hwc(_ptr(x), C, H, W, dtype_code(x.dtype), _ptr(out), _stream(x.device))
    L.check(rc, "upr_to_u8_hwc")
    return out


def panels_u8(x, enh, illu=None, comparison=2):
    """The harness's output pixels for a batch in one launch: x, enh [B,3,H,W] and illu
    [B,1,H,W] (or None) -> (enh_u8 [B,H,W,3], illu_u8 [B,H,W,3] or None, cmp_u8
    [B,H,comparison*W,3] or None), u8 on the device.  Image b of each is to_u8_hwc's bytes;
    the comparison is [x | enh] (comparison=2), [x | enh | illu] (3) or absent (None)."""
    _require_device(x)
    _require_device(enh, "enhanced")
    if comparison not in (None, 2, 3):
        raise ValueError(f"comparison must be None, 2 or 3, got {comparison!r}")
    if comparison == 3 and illu is None:
        raise ValueError("comparison=3 needs the illumination map")
    if x.dim() != 4 or x.shape[1] != 3 or enh.shape != x.shape or enh.dtype != x.dtype or enh.device != x.device:
        raise RuntimeError(f"expected x and enh of one shape [B, 3, H, W], dtype and device, got {tuple(x.shape)} "
                           f"{x.dtype} and {tuple(enh.shape)} {enh.dtype}")
    B, _, H, W = x.shape
    if illu is not None:
        _require_device(illu, "illumination")
        if tuple(illu.shape) != (B, 1, H, W) or illu.dtype != x.dtype or illu.device != x.device:
            raise RuntimeError(f"expected illu [{B}, 1, {H}, {W}] {x.dtype}, got {tuple(illu.shape)} {illu.dtype}")
        illu = illu.contiguous()
    x, enh = x.contiguous(), enh.contiguous()
    dev = x.device
    with torch.cuda.device(dev):
        enh_u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        illu_u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) if illu is not None else None
        cmp_u8 = torch.empty((B, H, comparison * W, 3), dtype=torch.uint8, device=dev) if comparison else None
        rc = L.lib().upr_panels_u8(_ptr(x), _ptr(enh), _ptr(illu), B, H, W, dtype_code(x.dtype), _ptr(enh_u8),
                                   _ptr(illu_u8), _ptr(cmp_u8), comparison or 0, _stream(dev))
    L.check(rc, "upr_panels_u8")
    return enh_u8, illu_u8, cmp_u8


def rgb2lab_u8(rgb):
    """rgb: [..., 3] uint8 interleaved."""
    _require_device(rgb)
    rgb = rgb.contiguous()
    lab = torch.empty_like(rgb)
    with torch.cuda.device(rgb.device):
        rc = L.lib().upr_rgb2lab_u8(_ptr(rgb), _ptr(lab), rgb.numel() // 3, _stream(rgb.device))
    L.check(rc, "upr_rgb2lab_u8")
    return lab


def lab2rgb_u8(lab):
    _require_device(lab)
    lab = lab.contiguous()
    rgb = torch.empty_like(lab)
    with torch.cuda.device(lab.device):
        rc = L.lib().upr_lab2rgb_u8(_ptr(lab), _ptr(rgb), lab.numel() // 3, _stream(lab.device))
    L.check(rc, "upr_lab2rgb_u8")
    return rgb


def clahe_u8(src, clip=2.0, tiles=(8, 8)):
    """src: [B,H,W] or [H,W] uint8 -> same shape."""
    _require_device(src)
    squeeze = src.dim() == 2
    s = (src.unsqueeze(0) if squeeze else src).contiguous()
    B, H, W = s.shape
    dst = torch.empty_like(s)
    lut = torch.empty(B * tiles[0] * tiles[1] * 256, dtype=torch.uint8, device=s.device)
    with torch.cuda.device(s.device):
        rc = L.lib().upr_clahe_u8(_ptr(s), _ptr(dst), _ptr(lut), B, H, W, float(clip), int(tiles[0]),
                                  int(tiles[1]), _stream(s.device))
    L.check(rc, "upr_clahe_u8")
    return dst[0] if squeeze else dst


def pack_conv_weight(w):
    """torch conv weight [Cout, Cin, kh, kw] -> packed [Cout, kh*kw*Cin] (tap-major)."""
    co, ci, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(co, kh * kw * ci).contiguous()


def _conv_io(x, residual, ychan, kh, kw, stride, pad, dil, f32_only=None, ydtype=None):
    """What the conv wrappers share: x on a device (float32 for the wrapper that
    f32_only names), x and residual contiguous, an empty NHWC output of ychan
    channels -> (x, residual, y)."""
    _require_device(x)
    if f32_only and x.dtype != torch.float32:
        raise ValueError(f"{f32_only} expects float32 tensors")
    x = x.contiguous()
    B, H, W, _ = x.shape
    Ho = (H + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    y = torch.empty((B, Ho, Wo, ychan), dtype=ydtype or x.dtype, device=x.device)
    return x, None if residual is None else residual.contiguous(), y


def conv2d_nhwc(x, w_packed, bias, kh, kw, stride=1, pad=0, dil=1, residual=None, relu=False):
    """x [B,H,W,Cin] -> y [B,Ho,Wo,Cout] through the implicit-GEMM MFMA kernel."""
    Cout = w_packed.shape[0]
    x, residual, y = _conv_io(x, residual, Cout, kh, kw, stride, pad, dil)
    B, H, W, Cin = x.shape
    with torch.cuda.device(x.device):
        rc = L.lib().upr_conv2d_nhwc(_ptr(x), B, H, W, Cin, _ptr(w_packed.contiguous()), _ptr(bias), Cout, kh, kw,
                                     stride, pad, dil, _ptr(residual), int(bool(relu)), _ptr(y),
                                     dtype_code(x.dtype), _stream(x.device))
    L.check(rc, "upr_conv2d_nhwc")
    return y


def conv2d_nhwc_regs(x, w_packed, bias, kh, kw, stride=1, pad=0, dil=1, residual=None, relu=False, overflow=None):
    """conv2d_nhwc for fp32 tensors in the split-in-registers form (fp16 MFMAs on
    fragments split after the LDS read), and in no other: shapes its kernels do
    not take raise UprError (UPR_ERR_UNSUPPORTED).

    overflow: optional int32 device tensor of one element, set to 1 when an
    input was outside the fp16 range (the output is then void)."""
    Cout = w_packed.shape[0]
    x, residual, y = _conv_io(x, residual, Cout, kh, kw, stride, pad, dil, f32_only="conv2d_nhwc_regs")
    B, H, W, Cin = x.shape
    with torch.cuda.device(x.device):
        rc = L.lib().upr_conv2d_nhwc_regs(_ptr(x), B, H, W, Cin, _ptr(w_packed.contiguous()), _ptr(bias), Cout, kh, kw,
                                          stride, pad, dil, _ptr(residual), int(bool(relu)), _ptr(y), _ptr(overflow),
                                          _stream(x.device))
    L.check(rc, "upr_conv2d_nhwc_regs")
    return y


def pack_split_w(w_packed, kh, kw, w2=None):
    """Packed fp32 conv weight [Cout, kh*kw*Cin] (pack_conv_weight), optionally with
    a second 1x1 K-segment w2 [Cout, C2] (a projecting shortcut) -> the uint8
    host blob conv2d_nhwc_wsplit takes: per output channel the fp16 planes W_hi
    = fp16(w s_n), W_lo = fp16(w s_n - W_hi) in MFMA k-slot order, then float
    1/s_n [Cout] at the next multiple of 256 bytes (include/upr.h)."""
    wc = w_packed.detach().to("cpu", torch.float32).contiguous()
    co, k = wc.shape
    w2c = None if w2 is None else w2.detach().to("cpu", torch.float32).reshape(co, -1).contiguous()
    c2 = 0 if w2c is None else w2c.shape[1]
    p2 = ctypes.c_void_p(w2c.data_ptr()) if w2c is not None else None
    lib = L.lib()
    cin = k // (kh * kw) if k % (kh * kw) == 0 else 0
    need = lib.upr_pack_split_w_f32(ctypes.c_void_p(wc.data_ptr()), co, cin, kh, kw, p2, c2, None, 0)
    if need == 0:
        raise ValueError(f"pack_split_w: unsupported weight shape {tuple(wc.shape)} + {c2} (Cout % 64, Cin % 32)")
    blob = torch.empty(need, dtype=torch.uint8)
    lib.upr_pack_split_w_f32(ctypes.c_void_p(wc.data_ptr()), co, cin, kh, kw, p2, c2, ctypes.c_void_p(blob.data_ptr()), need)
    return blob


def conv2d_nhwc_wsplit(x, w_blob, cout, bias, kh, kw, stride=1, pad=0, dil=1, residual=None, relu=False, x2=None,
                       stride2=1, overflow=None):
    """fp32 conv2d_nhwc on the fp16 MFMA unit with weights split once (w_blob:
    pack_split_w, on the device), and in no other form: shapes its kernel does
    not take raise UprError (UPR_ERR_UNSUPPORTED).  y = relu?(conv(x) +
    conv1x1(x2 at stride2) + bias) + residual (added after the ReLU).

    overflow: optional int32 device tensor of one element, set to 1 when an
    input was outside the fp16 range (the output is then void)."""
    x, residual, y = _conv_io(x, residual, cout, kh, kw, stride, pad, dil, f32_only="conv2d_nhwc_wsplit")
    B, H, W, Cin = x.shape
    H2 = W2 = C2 = 0
    if x2 is not None:
        x2 = x2.contiguous()
        _, H2, W2, C2 = x2.shape
    with torch.cuda.device(x.device):
        rc = L.lib().upr_conv2d_nhwc_wsplit(_ptr(x), B, H, W, Cin, _ptr(w_blob), w_blob.numel(), _ptr(bias), cout, kh,
                                            kw, stride, pad, dil, _ptr(residual), int(bool(relu)), _ptr(y), _ptr(x2),
                                            H2, W2, C2, stride2, _ptr(overflow), _stream(x.device))
    L.check(rc, "upr_conv2d_nhwc_wsplit")
    return y


def last_wsplit_kernel():
    """The kernel this thread's latest conv2d_nhwc_wsplit ran: "ring" (the row
    ring: 64 -> 64 stride-1 3x3 ops, unless UPR_W64_RING=0 at the call), "tile"
    (the gathered 256 x 64 tile) or None (the call was refused)."""
    return {1: "tile", 2: "ring"}.get(L.lib().upr_conv_wsplit_ran())


def split_f32(x, overflow=None):
    """fp32 NHWC [..., C] -> split fp16 [..., 2C] = [hi | lo] (hi + lo * 2^-11 = x to ~2^-22).

    overflow: optional int32 device tensor of one element, set to 1 when a
    value is outside the fp16 range."""
    _require_device(x)
    if x.dtype != torch.float32 or x.shape[-1] % 8:
        raise ValueError("split_f32 expects float32 with a channel count that is a multiple of 8")
    x = x.contiguous()
    C = x.shape[-1]
    y = torch.empty(x.shape[:-1] + (2 * C,), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.lib().upr_split_f32(_ptr(x), _ptr(y), x.numel() // C, C, _ptr(overflow), _stream(x.device))
    L.check(rc, "upr_split_f32")
    return y


def unsplit_f32(y):
    """Inverse of split_f32: split fp16 [..., 2C] -> fp32 [..., C]."""
    _require_device(y)
    if y.dtype != torch.float16 or y.shape[-1] % 16:
        raise ValueError("unsplit_f32 expects a float16 split tensor")
    y = y.contiguous()
    C = y.shape[-1] // 2
    x = torch.empty(y.shape[:-1] + (C,), dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        rc = L.lib().upr_unsplit_f32(_ptr(y), _ptr(x), y.numel() // (2 * C), C, _stream(y.device))
    L.check(rc, "upr_unsplit_f32")
    return x


def pack_split_weight(w):
    """torch conv weight [Cout, Cin, kh, kw] (fp32, host packing) -> the uint8 blob
    conv2d_split takes: split-fp16 K-segments [W_hi | W_hi 2^-11], W_lo and the per-channel scale."""
    wc = w.detach().to("cpu", torch.float32).contiguous()
    co, ci, kh, kw = wc.shape
    lib = L.lib()
    need = lib.upr_pack_split_f32(ctypes.c_void_p(wc.data_ptr()), co, ci, kh, kw, None, 0)
    if need == 0:
        raise ValueError(f"pack_split_weight: unsupported weight shape {tuple(wc.shape)} (Cin % 64 == 0)")
    blob = torch.empty(need, dtype=torch.uint8)
    lib.upr_pack_split_f32(ctypes.c_void_p(wc.data_ptr()), co, ci, kh, kw, ctypes.c_void_p(blob.data_ptr()), need)
    return blob


def conv2d_split(x, w_blob, cout, bias, kh, kw, stride=1, pad=0, dil=1, residual=None, relu=False):
    """conv2d_nhwc on split tensors: x [B,H,W,2Cin] and residual [B,Ho,Wo,2Cout] fp16
    split, w_blob from pack_split_weight (on the device) -> y [B,Ho,Wo,2Cout] split."""
    x, residual, y = _conv_io(x, residual, 2 * cout, kh, kw, stride, pad, dil, ydtype=torch.float16)
    B, H, W, C2 = x.shape
    with torch.cuda.device(x.device):
        rc = L.lib().upr_conv2d_nhwc(_ptr(x), B, H, W, C2 // 2, _ptr(w_blob), _ptr(bias), cout, kh, kw, stride, pad,
                                     dil, _ptr(residual), int(bool(relu)), _ptr(y), L.UPR_F32_SPLIT,
                                     _stream(x.device))
    L.check(rc, "upr_conv2d_nhwc(split)")
    return y


def lab_tables():
    """Host copies of the 8-bit Lab tables (no device needed)."""
    import numpy as np
    g = np.zeros(256, np.uint16)
    c = np.zeros(3072, np.uint16)
    yf = np.zeros(512, np.uint16)
    ig = np.zeros(4096, np.uint16)
    m1 = np.zeros(9, np.int32)
    m2 = np.zeros(9, np.int32)
    L.lib().upr_lab_tables(g.ctypes.data, c.ctypes.data, yf.ctypes.data, ig.ctypes.data, m1.ctypes.data,
                           m2.ctypes.data)
    return {"gamma": g, "cbrt": c, "yf": yf, "invgamma": ig, "rgb2xyz": m1, "xyz2rgb": m2}


def multiscale_features(x, scale_idx):
    """[B,3,H,W] -> [B,7,hs,ws] feature maps of scale 0 (x1), 1 (x0.5) or 2 (x0.25)."""
    _require_device(x)
    x = x.contiguous()
    B, C, H, W = x.shape
    s = (1.0, 0.5, 0.25)[scale_idx]
    hs, ws = (H, W) if scale_idx == 0 else (int(H * s), int(W * s))
    out = torch.empty((B, 7, hs, ws), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.lib().upr_multiscale_features(_ptr(x), _ptr(out), B, H, W, int(scale_idx), dtype_code(x.dtype),
                                             _stream(x.device))
    L.check(rc, "upr_multiscale_features")
    return out


def content_aware(x, enh=None, saliency=False, attention=False):
    """Returns (out or None, saliency [B,H,W] f32 or None, attention [B,H,W] f32 or None)."""
    _require_device(x)
    x = x.contiguous()
    B, C, H, W = x.shape
    dev = x.device
    out = None
    if enh is not None:
        enh = enh.contiguous()
        if enh.shape != x.shape or enh.dtype != x.dtype:
            raise RuntimeError("content_aware: enhanced image must match the input's shape and dtype")
        out = torch.empty_like(enh)
    sal = torch.empty((B, H, W), dtype=torch.float32, device=dev) if saliency else None
    att = torch.empty((B, H, W), dtype=torch.float32, device=dev) if attention else None
    lib = L.lib()
    with torch.cuda.device(dev):
        nbytes = lib.upr_content_aware_workspace(B, H, W)
        ws = _WS.get(dev, nbytes)
        rc = lib.upr_content_aware(_ptr(x), _ptr(enh), _ptr(out), _ptr(sal), _ptr(att), _ptr(ws),
                                   ctypes.c_size_t(ws.numel()), B, H, W, dtype_code(x.dtype), _stream(dev))
    L.check(rc, "upr_content_aware")
    return out, sal, att


def image_metrics(enh, ref=None, sums=False, hist=False):
    """calculate_metrics (utils/utils.py:95-333) of every image of enh [B,3,H,W]
    against ref (same shape and dtype, optional).  Returns (metrics [B,9] f64 in
    the order of _lib.METRIC_NAMES, the last three NaN without ref; sums [B,14]
    f64 or None; hist [B,256] int32 or None), all on the device, no synchronisation."""
    _require_device(enh)
    if enh.dim() != 4 or enh.shape[1] != 3:
        raise RuntimeError(f"expected an image batch of shape [B, 3, H, W], got {tuple(enh.shape)}")
    if ref is not None:
        _require_device(ref, "reference")
        if ref.shape != enh.shape or ref.dtype != enh.dtype or ref.device != enh.device:
            raise RuntimeError("image_metrics: the reference must match the image's shape, dtype and device")
        ref = ref.contiguous()
    enh = enh.contiguous()
    B, _, H, W = enh.shape
    dev = enh.device
    lib = L.lib()
    with torch.cuda.device(dev):
        m = torch.empty((B, L.UPR_METRICS_N), dtype=torch.float64, device=dev)
        s = torch.empty((B, L.UPR_METRICS_NSUMS), dtype=torch.float64, device=dev) if sums else None
        h = torch.empty((B, 256), dtype=torch.int32, device=dev) if hist else None
        ws = _WS.get(dev, lib.upr_image_metrics_workspace(B, H, W))
        rc = lib.upr_image_metrics(_ptr(enh), _ptr(ref), _ptr(m), _ptr(s), _ptr(h), _ptr(ws),
                                   ctypes.c_size_t(ws.numel()), B, H, W, dtype_code(enh.dtype), _stream(dev))
    L.check(rc, "upr_image_metrics")
    return m, s, h


def image_loe(low, enh, size=50, counts=False):
    """Lightness order error (Wang et al. 2013; include/upr.h upr_image_loe) of
    every image of enh [B,3,H,W] against its low-light input low (same shape,
    dtype and device) on the size-pixel sample grid (0: every pixel).  Returns
    loe [B] f64, or (loe, counts [B,2] int64 = (D, N)) with counts=True, on the
    device, no synchronisation."""
    _require_device(low, "low")
    _require_device(enh, "enhanced")
    if low.dim() != 4 or low.shape[1] != 3:
        raise RuntimeError(f"expected an image batch of shape [B, 3, H, W], got {tuple(low.shape)}")
    if enh.shape != low.shape or enh.dtype != low.dtype or enh.device != low.device:
        raise RuntimeError("image_loe: the enhanced image must match the input's shape, dtype and device")
    if int(size) != size or size < 0:
        raise ValueError(f"image_loe: size must be an integer >= 0, got {size!r}")
    low, enh = low.contiguous(), enh.contiguous()
    B, _, H, W = low.shape
    dev = low.device
    lib = L.lib()
    with torch.cuda.device(dev):
        out = torch.empty((B,), dtype=torch.float64, device=dev)
        c = torch.empty((B, 2), dtype=torch.int64, device=dev) if counts else None
        ws = _WS.get(dev, lib.upr_image_loe_workspace(B))
        rc = lib.upr_image_loe(_ptr(low), _ptr(enh), _ptr(out), _ptr(c), _ptr(ws), ctypes.c_size_t(ws.numel()), B, H,
                               W, int(size), dtype_code(low.dtype), _stream(dev))
    L.check(rc, "upr_image_loe")
    return (out, c) if counts else out


class _Decompose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, illu):
        B, C, H, W = x.shape
        refl = torch.empty_like(x)
        with torch.cuda.device(x.device):
            rc = L.lib().upr_retinex_decompose(_ptr(x), _ptr(illu), _ptr(refl), B, C, H, W, illu.shape[1],
                                               dtype_code(x.dtype), _stream(x.device))
        L.check(rc, "upr_retinex_decompose")
        ctx.save_for_backward(x, illu)
        return refl

    @staticmethod
    def backward(ctx, g):
        x, illu = ctx.saved_tensors
        B, C, H, W = x.shape
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gi = torch.empty_like(illu) if ctx.needs_input_grad[1] else None
        g = g.contiguous().to(x.dtype)
        with torch.cuda.device(x.device):
            rc = L.lib().upr_retinex_decompose_bwd(_ptr(x), _ptr(illu), _ptr(g), _ptr(gx), _ptr(gi), B, C, H, W,
                                                   illu.shape[1], dtype_code(x.dtype), _stream(x.device))
        L.check(rc, "upr_retinex_decompose_bwd")
        return gx, gi


def retinex_decompose(x, illu):
    """x / (illu + 1e-6) (models/model.py:405-413) on the device, illu [B,1,H,W]
    broadcast over the channels (or [B,C,H,W]); differentiable in x and illu."""
    _require_device(x)
    _require_device(illu, "illumination")
    if x.dim() != 4 or illu.dim() != 4 or illu.shape[0] != x.shape[0] or illu.shape[2:] != x.shape[2:] or \
            illu.shape[1] not in (1, x.shape[1]):
        raise RuntimeError(f"retinex_decompose: shapes {tuple(x.shape)} and {tuple(illu.shape)} do not broadcast "
                           f"as [B,C,H,W] / [B,1 or C,H,W]")
    if x.dtype != illu.dtype:
        raise RuntimeError(f"retinex_decompose: dtype mismatch {x.dtype} vs {illu.dtype}")
    dtype_code(x.dtype)
    return _Decompose.apply(x.contiguous(), illu.contiguous())
