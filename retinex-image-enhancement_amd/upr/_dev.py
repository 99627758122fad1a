"""Device plumbing of the training engine, loss engine, optimiser and scaler: torch's
stream and tensor addresses as the C ABI's void*, device tensors, status helpers."""
import ctypes

import torch

from . import _lib as L

F32 = torch.float32


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_dev = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The current HIP stream of the current device (torch's), as the C ABI's
    void*.  Read through torch's raw accessors when present: the ~600 launches
    of a training step each ask, and torch.cuda.current_stream() builds a
    Stream object per call (~1 ms of host time per step)."""
    if _raw_stream is not None and _cur_dev is not None:
        return ctypes.c_void_p(_raw_stream(_cur_dev()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_chk = L.check


def took(rc, what):
    """True when the call ran, False on UPR_ERR_UNSUPPORTED (nothing launched: the
    caller takes its fallback); any other status raises."""
    if rc == 0:
        return True
    if rc != L.UPR_ERR_UNSUPPORTED:
        L.check(rc, what)
    return False


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _fp(t, off=0):
    """Pointer to element `off` of a fp32 tensor."""
    return ctypes.c_void_p(t.data_ptr() + 4 * off) if t is not None else None


def empty(shape, dev):
    return torch.empty(shape, dtype=F32, device=dev)


def _h16(n, dev):
    return torch.empty((n,), dtype=torch.float16, device=dev)


def zero(t):
    _chk(L.lib().upr_t_zero(_p(t), t.numel() * t.element_size(), _stream()), "zero")
