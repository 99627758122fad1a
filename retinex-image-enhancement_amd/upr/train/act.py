"""Activations / gradients (`Act`), the fp16 copy one may carry under autocast
(`Half`) and concat assembly (`Concat`).  Only this module assigns the copy's
bookkeeping; everything else attaches, drops and asks through Act's methods."""
import ctypes

from .. import _lib as L
from .._dev import F32, _chk, _fp, _h16, _p, _stream, empty
from .state import _AMP


class Half:
    """An fp16 copy here: pixel m, channel c at t[m * cs + coff + c] of a flat fp16 tensor."""
    __slots__ = ("t", "cs", "coff")

    def __init__(self, t, cs, coff=0):
        self.t, self.cs, self.coff = t, cs, coff

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + 2 * self.coff)

    def slice(self, coff, C):
        return Half(self.t, self.cs, self.coff + coff)


class Act:
    """NHWC activation: channels [coff, coff+C) of a [B,H,W,cs] fp32 tensor.

    `fresh` marks a gradient buffer nothing has written yet: the first
    producer overwrites (or zeroes it when it scatters with atomics), later
    producers accumulate.

    Under autocast an Act may carry an fp16 copy of its values (attach16; whoever
    changes the fp32 values drops or replaces it)."""

    def __init__(self, t, C=None, coff=0):
        assert t.dim() == 4 and t.dtype == F32 and t.is_contiguous()
        self.t = t
        self.B, self.H, self.W, self.cs = t.shape
        self.C = self.cs if C is None else C
        self.coff = coff
        self.fresh = False
        # the fp16 copy (Half) or None: compact (this whole tensor's, C wide), or a slice of a concat's
        # (_h); _grad: a gradient's copy, which the gradient convs trust as their fp16 operand; _only: the
        # fp32 values were deliberately not written, need32() refuses their readers; _shared: a whole concat's
        # copy that channel slices taken afterwards read in place (a slice's copy then has a stride wider
        # than its C): EnhancedFAM's fusion input gradient
        self.drop16()

    @staticmethod
    def new(B, H, W, C, dev, fresh=True):
        a = Act(empty((B, H, W, C), dev))
        a.fresh = fresh
        return a

    def slice(self, coff, C):
        """Channels [coff, coff+C): a shared copy and its marks go along, a compact copy never does."""
        s = Act(self.t, C, self.coff + coff)
        s.fresh = self.fresh
        if self._shared and self._h is not None:
            s._h, s._grad, s._only, s._shared = self._h.slice(coff, C), self._grad, self._only, True
        return s

    # ---- the fp16 copy: state changes ----
    def attach16(self, h, grad=False, only=False, shared=False):
        """This Act's values are (also) at `h`: a Half, or a whole Act's flat fp16 tensor (compact)."""
        if not isinstance(h, Half):
            assert self.whole, "a compact fp16 copy belongs to a whole tensor"
            h = Half(h, self.C)
        self._h, self._grad, self._only, self._shared = h, bool(grad), bool(only), bool(shared)

    def drop16(self):
        """The fp32 values are (about to be) the only ones: forget the copy and its marks."""
        self._h, self._grad, self._only, self._shared = None, False, False, False

    def consume_fresh(self):
        """Returns 1 (accumulate) or 0 (overwrite) for the next producer; the fp16 copy goes."""
        acc = 0 if self.fresh else 1
        self.fresh = False
        self.drop16()
        return acc

    # ---- the fp16 copy: queries ----
    @property
    def whole(self):
        """This Act is a whole compact tensor (not a channel slice of a wider one)."""
        return self.coff == 0 and self.cs == self.C

    @property
    def only16(self):
        return self._only

    def compact16(self, C=None, grad=False):
        """The compact copy (flat fp16 tensor) or None; C: only if exactly C wide; grad: only a gradient's."""
        if self._h is None or not self.whole or (C is not None and C != self.C) or (grad and not self._grad):
            return None
        return self._h.t

    def any16(self, grad=False):
        """The copy as a Half (.ptr(), .cs), compact or a slice of a shared one, or None."""
        return self._h if self._h is not None and (self._grad or not grad) else None

    def need32(self, reader):
        """`reader` is about to read the fp32 values."""
        if self._only:
            raise RuntimeError(f"upr: {reader} reads the fp32 values of an fp16-only activation / gradient")

    @property
    def M(self):
        return self.B * self.H * self.W

    def ptr(self):
        return _fp(self.t, self.coff)

    def view(self):
        return L.UprView(self.t.data_ptr() + 4 * self.coff, self.H * self.W * self.cs, self.W * self.cs, self.cs, 1)

    def zero_if_fresh(self):
        if self.fresh:
            _chk(L.lib().upr_t_zero(_p(self.t), self.t.numel() * 4, _stream()), "zero")
            self.fresh = False


class Concat:
    """A concat [B,H,W,C] whose producers write their channel slices in place and,
    under autocast, the same slices of its fp16 copy.  `only`: no fp32 slices at
    all (every reader takes the copy); holds only with a copy.  Each producer
    gets part() and reports wrote(); finish() attaches the copy if every slice
    of it was written, and refuses fp16-only slices left without one."""

    def __init__(self, B, H, W, C, dev, only=False):
        self.act = Act.new(B, H, W, C, dev, fresh=False)
        self.h = Half(_h16(self.act.M * C, dev), C) if _AMP[0] else None
        self.ok16 = self.h is not None
        self.only = bool(only) and self.ok16

    def part(self, coff, C):
        return self.act.slice(coff, C), (self.h.slice(coff, C) if self.h is not None else None)

    def wrote(self, ok):
        self.ok16 = self.ok16 and bool(ok)

    def finish(self, all32=False):
        """all32: every fp32 slice was written whatever `only` asked (a fallback re-did them)."""
        if all32:
            self.only = False
        if self.ok16:
            self.act.attach16(self.h, only=self.only)
        elif self.only:
            raise RuntimeError("upr: fp16-only concat slices without the concat's fp16 copy")
        return self.act


def nchw_view(t, coff=0):
    B, C, H, W = t.shape
    return L.UprView(t.data_ptr() + 4 * coff * H * W, C * H * W, W, 1, H * W)
