"""Pointwise / resampling operations (csrc/train_pointwise.hip, train_resample.hip)."""
import ctypes

from .. import _lib as L
from .._dev import _chk, _fp, _h16, _p, _stream, took
from .state import _AMP


def relu_mask(g, y, want16=False, only16=False):
    """g *= (y > 0) in place.  want16: also write the masked gradient's fp16 copy
    (the next autocast dgrad's operand) in the same pass; only16: the fp32
    g is left unmasked (fp16-only) -- for a gradient whose only reader is a frozen
    conv's fp16 dgrad."""
    g.drop16()  # masked in place: any fp16 copy is stale
    if want16 and g.whole:
        g16 = _h16(g.M * g.C, g.t.device)
        if y.only16:  # y exists in fp16 only (frozen VGG activations under autocast)
            rc = L.lib().upr_t_relu_mask16h(_fp(g.t), g.cs, g.coff, _p(y.compact16()), y.C, g.M, g.C, _p(g16),
                                            int(not only16), _stream())
        else:
            rc = L.lib().upr_t_relu_mask16(_fp(g.t), g.cs, g.coff, _fp(y.t), y.cs, y.coff, g.M, g.C, _p(g16),
                                           int(not only16), _stream())
        if took(rc, "relu_mask16"):
            g.attach16(g16, grad=True, only=only16)
            return
    y.need32("the ReLU backward (its mask)")
    _chk(L.lib().upr_t_relu_mask(_fp(g.t), g.cs, g.coff, _fp(y.t), y.cs, y.coff, g.M, g.C, _stream()), "relu_mask")


def maxpool_into(x, y, k, s, p, code=None, only16=False):
    """nn.MaxPool2d(k, s, p) of Act x into Act y (argmax codes for the backward
    when `code`); under autocast also y's fp16 copy in the same pass.
    only16 (under autocast, from an fp16 input): y is written as its fp16 copy
    only (y.only16; the max of fp16 values is an fp16 value, so nothing is
    rounded) -- the frozen VGG's pools, whose every reader takes fp16."""
    lib, st = L.lib(), _stream()
    if _AMP[0] and y.whole:
        y16 = _h16(y.M * y.C, y.t.device)
        x16 = x.compact16()
        if x16 is not None:
            # the activation's fp16 copy (its only value when x.only16)
            yv = y.view()
            if only16:
                yv.data = None
            rc = lib.upr_t_maxpool16_code(_p(x16), x.B, x.H, x.W, x.C, k, s, p, ctypes.byref(yv), y.H, y.W,
                                          _p(code), _p(y16), st)
            if took(rc, "maxpool16"):
                y.attach16(y16, only=only16)
                return
        x.need32("the max-pool")
        rc = lib.upr_t_maxpool_code(ctypes.byref(x.view()), x.B, x.H, x.W, x.C, k, s, p, ctypes.byref(y.view()), y.H,
                                    y.W, _p(code), _p(y16), st)
        if took(rc, "maxpool"):
            y.attach16(y16)
            return
    _chk(lib.upr_t_maxpool_code(ctypes.byref(x.view()), x.B, x.H, x.W, x.C, k, s, p, ctypes.byref(y.view()), y.H, y.W,
                                _p(code), None, st), "maxpool")
    y.drop16()


def add_into(dst, src):
    """dst (+)= src (Acts of equal shape)."""
    acc = dst.consume_fresh()
    _chk(L.lib().upr_t_copy(ctypes.byref(src.view()), ctypes.byref(dst.view()), src.B, src.H, src.W, src.C, acc,
                            _stream()), "copy")


def pointwise(a, b, out, n, op, mask_in=None, mask_out=None, p=0.0, seed=0):
    _chk(L.lib().upr_t_pointwise(_p(a), _p(b), _p(out), n, op, _p(mask_in), _p(mask_out), ctypes.c_float(p),
                                 ctypes.c_uint64(seed), _stream()), "pointwise")
