"""nn.Conv2d / nn.ConvTranspose2d layers and the per-step weight re-pack
(csrc/train_conv.hip, train_wgrad.hip, train_small.hip)."""
import ctypes
import sys

import torch

from .. import _lib as L
from .._dev import _chk, _fp, _h16, _p, _stream, empty, took, zero
from .act import Act, Half
from .bn import chan_sum
from .ops import relu_mask
from .state import _AMP, _TRACE_CAST, _timed


def mfma16(x, B, H, W, C, cs, coff, w16, bias, N, kh, kw, s, p, d, res, relu, out, store=0, x16=None,
           keep16=False, out16=None, only16=False, grad16=False, shared16=False):
    """fp16 MFMA conv with fp32 in / out (upr_t_conv_mfma16); res: Act or None.  x16 (Half): the
    input's fp16 copy when its producer wrote it -- compact, or the shared copy of the concat it
    is a slice of (stride wider than C: read in place).  out16 (Half): where the (half)out copy
    goes when `out` is a slice of a concat whose copy the caller assembles; otherwise a whole
    `out` keeps its own (keep16, no residual).  Returns the input's flat fp16 tensor."""
    Ho = (H + 2 * p - d * (kh - 1) - 1) // s + 1
    Wo = (W + 2 * p - d * (kw - 1) - 1) // s + 1
    dev = out.t.device
    ready = x16 is not None
    if not ready:
        x16 = Half(_h16(B * H * W * C, dev), C)
        if _TRACE_CAST:  # UPR_TRACE_CAST=1: name the convs whose fp16 operand is cast here
            import traceback
            where = " < ".join(f"{f.name}:{f.lineno}" for f in traceback.extract_stack()[-5:-1][::-1])
            print(f"upr_cast conv {C}->{N} k{kh} s{s} {H}x{W} B{B} at {where}", file=sys.stderr)
    if x16.cs != C:
        store |= L.UPR_T_STORE_X16_STRIDED
    if out16 is not None:
        y16p, y16cs = out16.ptr(), out16.cs
    else:
        y16 = _h16(B * Ho * Wo * N, dev)
        y16p, y16cs = _p(y16), 0
    keep = keep16 and res is None
    _chk(L.lib().upr_t_conv_mfma16(_fp(x, 0), B, H, W, C, cs, coff, _p(w16), _p(bias), N, kh, kw, s, p, d,
                                   res.ptr() if res is not None else None, res.cs if res is not None else 0,
                                   int(relu), _fp(out.t), out.cs, out.coff,
                                   store | (L.UPR_T_STORE_KEEP16 if keep else 0) |
                                   (L.UPR_T_STORE_ONLY16 if only16 and keep else 0),
                                   x16.ptr(), int(ready), y16p, y16cs, _stream()), "conv_mfma16")
    # forward activations (keep16): without a residual y16 is (half)out exactly, and the next
    # autocast conv reading out takes it; forward activations are not modified in place
    if out16 is None and keep and out.whole and out.C == (N // 4 if store & L.UPR_T_STORE_CONVT2X2 else N):
        out.attach16(y16, grad=grad16, only=only16, shared=shared16)
    else:
        out.drop16()
    return x16.t


# ---------------------------------------------------------------------------
# layers
# ---------------------------------------------------------------------------
class Conv:
    """nn.Conv2d (model.py / VGG) forward, input-gradient and weight-gradient.

    Cin, Cout multiples of 32 run on the MFMA implicit-GEMM kernels (weights
    re-packed every step: [Cout][(ky,kx,ci)] forward, flipped [Cin][(ky,kx,co)]
    for the input gradient); other shapes on the direct kernels."""

    def __init__(self, m, frozen=False):
        self.m = m
        self.Cout, self.Cin, self.kh, self.kw = m.weight.shape
        self.s = m.stride[0]
        self.p = m.padding[0]
        self.d = m.dilation[0]
        self.bias = m.bias
        self.mfma = self.Cin % 32 == 0 and self.Cout % 32 == 0
        self.frozen = frozen
        self.wp = self.wt = self.wp16 = self.wt16 = None
        self.amp = False  # fp16 arithmetic of the last forward (its backward follows it)
        self.dgrad16_c3 = False
        self.only16 = False

    def out_hw(self, H, W):
        return ((H + 2 * self.p - self.d * (self.kh - 1) - 1) // self.s + 1,
                (W + 2 * self.p - self.d * (self.kw - 1) - 1) // self.s + 1)

    def pack_jobs(self):
        """This conv's re-packs as UprPackJob tuples (pack_convs): the forward
        and flipped dgrad layouts, fp16 only under autocast, else fp32."""
        if not self.mfma:
            return []
        w, amp = self.m.weight, _AMP[0]
        if self.wp is None:
            self.wp = torch.empty_like(w).view(-1)
            self.wt = torch.empty_like(w).view(-1)
        if amp and self.wp16 is None:
            self.wp16, self.wt16 = _h16(w.numel(), w.device), _h16(w.numel(), w.device)
        n = w.numel()
        return [(w.data_ptr(), 0 if amp else self.wp.data_ptr(), self.wp16.data_ptr() if amp else 0, self.Cout,
                 self.Cin, self.kh, self.kw, 0, n),
                (w.data_ptr(), 0 if amp else self.wt.data_ptr(), self.wt16.data_ptr() if amp else 0, self.Cout,
                 self.Cin, self.kh, self.kw, 1, n)]

    def pack(self):
        pack_convs([self], self)

    def fwd(self, x, relu=False, out=None, res=None, x_view=None, out16=None, only16=False):
        """x: Act (or x_view: (UprView, B, H, W) for an NCHW network input); out16: see mfma16
        (autocast MFMA convs only; self.wrote16 tells whether the copy was written).
        only16: under autocast every reader of the output takes its fp16 copy (the
        frozen VGG's activations): the fp32 output is not written (out.only16)."""
        if x_view is not None:
            xv, B, H, W = x_view
        else:
            B, H, W = x.B, x.H, x.W
        Ho, Wo = self.out_hw(H, W)
        if out is None:
            out = Act.new(B, Ho, Wo, self.Cout, x.t.device, fresh=False)
        out.fresh = False
        out.drop16()  # any fp16 copy of an earlier content is stale now
        # (a channel slice of a concat qualifies when its fp16 copy goes to the concat's copy, out16)
        self.only16 = bool(only16 and _AMP[0] and res is None and (out.whole or out16 is not None))
        self.amp = _AMP[0] and self.mfma and x_view is None
        # autocast 3 -> 32 / 64 3x3 convs: input gradient on MFMA from an fp16 dy (upr_t_conv_dgrad_c3_16)
        self.dgrad16_c3 = _AMP[0] and self.Cin == 3 and self.Cout in (32, 64) and \
            (self.kh, self.kw, self.s, self.p, self.d) == (3, 3, 1, 1, 1)
        self.out_wo = Wo
        kind = "mfma16" if self.amp else ("mfma32" if self.mfma and x_view is None else "direct")
        with _timed(kind, "fwd", self.flops(B, Ho, Wo), (self.Cin, self.Cout, self.kh, self.s, H, W)):
            self._fwd(x, B, H, W, Ho, Wo, relu, out, res, x_view, out16 if self.amp else None)
        self.wrote16 = self.amp and out16 is not None and res is None
        return out

    def flops(self, B, Ho, Wo):
        return 2.0 * B * Ho * Wo * self.Cout * self.Cin * self.kh * self.kw

    def wgrad16_ok(self, W):
        """Under autocast, this conv's weight gradient on an input of width W runs on
        the fp16-operand GEMM (it reads the input's fp16 copy only)."""
        if not (_AMP[0] and self.mfma):
            return False
        if self.frozen:
            return True
        return ((W + 2 * self.p - self.d * (self.kw - 1) - 1) // self.s + 1) % 64 == 0

    def takes16_grad(self):
        """True when every reader of this conv's output gradient in its backward can
        take the gradient's fp16 copy alone (autocast: input gradient on the fp16
        MFMA, weight gradient on the fp16-operand GEMM, bias sum from fp16), so its
        producer (the BatchNorm backward) may skip the fp32 store."""
        if not (self.amp and self.mfma) or self.s not in (1, 2) or self.Cout % 8:
            return False
        if self.frozen:
            return True
        return getattr(self, "out_wo", 0) % 64 == 0 and getattr(self, "x16", None) is not None

    def _fwd(self, x, B, H, W, Ho, Wo, relu, out, res, x_view, out16=None):
        lib, st = L.lib(), _stream()
        if x_view is not None:
            xv = x_view[0]
        if self.amp:
            # the fp16 copy of x is the weight gradient's B operand (upr_t_conv_wgrad16)
            t16 = x.compact16(self.Cin)
            x16 = mfma16(x.t, B, H, W, self.Cin, x.cs, x.coff, self.wp16, self.bias, self.Cout, self.kh,
                         self.kw, self.s, self.p, self.d, res, relu, out, x16=x.any16() if t16 is not None else None,
                         keep16=True, out16=out16, only16=self.only16)
            if t16 is None and x.whole and x.C == self.Cin:
                x.attach16(x16)  # the next autocast conv reading x (EnhancedFAM: three of them) reuses the copy
            self.x16 = None if self.frozen else x16
        elif self.mfma and x_view is None:
            _chk(lib.upr_t_conv_mfma(_fp(x.t), B, H, W, self.Cin, x.cs, x.coff, _p(self.wp),
                                     _p(self.bias), self.Cout, self.kh, self.kw, self.s, self.p, self.d,
                                     res.ptr() if res is not None else None, res.cs if res is not None else 0,
                                     int(relu), _fp(out.t), out.cs, out.coff, 0, st), "conv_mfma")
        else:
            assert res is None
            v = x.view() if x_view is None else xv
            if _AMP[0] and self.Cin == 3 and self.Cout in (32, 64) and out.whole:
                # autocast: the 3-channel input convs also write their output's fp16 copy (the
                # next conv's operand) instead of a separate cast pass
                y16 = _h16(B * Ho * Wo * self.Cout, out.t.device)
                rc = lib.upr_t_conv_direct16(ctypes.byref(v), B, H, W, self.Cin, _p(self.m.weight), _p(self.bias),
                                             self.Cout, self.kh, self.kw, self.s, self.p, self.d,
                                             ctypes.byref(out.view()), Ho, Wo, int(relu), 0, _p(y16),
                                             int(self.only16), st)
                if took(rc, "conv_direct16"):
                    out.attach16(y16, only=self.only16)
                    return
            _chk(lib.upr_t_conv_direct(ctypes.byref(v), B, H, W, self.Cin, _p(self.m.weight), _p(self.bias),
                                       self.Cout, self.kh, self.kw, self.s, self.p, self.d,
                                       ctypes.byref(out.view()), Ho, Wo, int(relu), 0, st), "conv_direct")

    def _dgrad_s2(self, k, gy, src16, B, Ho, Wo, gx, acc, o16):
        """Input gradient of a stride-2 conv straight from dy, no zero-upsampled operand
        (upr_t_conv_mfma16).  k = 1, the projecting shortcut (model.py:119-122), store S2_1X1:
        dx(2i, 2j) += W^T dy(i, j), accumulated into gx.  k = 3, pad 1 (enc1.conv1,
        model.py:100-178), store S2_3X3_DGRAD: the four output phases as small convs over dy;
        o16: a fresh gx gets its fp16 copy only.  False when the kernel does not take the
        shape (the caller then zero-upsamples)."""
        if gy.only16 and src16 is None:
            return False
        dev, ready = gy.t.device, src16 is not None
        x16 = src16 if ready else _h16(B * Ho * Wo * self.Cout, dev)
        keep = k == 3 and bool(o16) and not acc
        y16 = _h16(B * 4 * Ho * Wo * self.Cin if keep else 16, dev)  # written only with keep
        rc = L.lib().upr_t_conv_mfma16(None if ready else _fp(gy.t, 0), B, Ho, Wo, self.Cout, gy.cs, gy.coff,
                                       _p(self.wt16), None, self.Cin, k, k, 1, k // 2, 1, gx.ptr() if acc else None,
                                       gx.cs if acc else 0, 0, _fp(gx.t), gx.cs, gx.coff,
                                       (L.UPR_T_STORE_S2_1X1 if k == 1 else L.UPR_T_STORE_S2_3X3_DGRAD) |
                                       (L.UPR_T_STORE_KEEP16 | L.UPR_T_STORE_ONLY16 if keep else 0),
                                       _p(x16), int(ready), _p(y16), 0, _stream())
        if not took(rc, "conv_dgrad_s2"):
            return False
        if keep:
            gx.attach16(y16, grad=True, only=True)
        else:
            gx.drop16()  # gx changed: any fp16 copy of it is stale
        return True

    def bwd_relu_stem(self, x, gy, y, x_view=None):
        """relu_mask(gy, y) then bwd(x, gy, None, x_view): the weight gradient of a
        conv whose input needs no gradient (the image stems), the ReLU backward of
        its output y fused into the small-channel weight-gradient kernel (gy is
        left unmasked: this is its only reader)."""
        # (y.only16 -- the stem output stored fp16-only -- still takes the stem kernel,
        # whose mask reads y's fp16 copy; the generic direct kernel reads y in fp32)
        if not self.frozen and not (self.mfma and x_view is None) and not gy.only16:
            lib, st = L.lib(), _stream()
            if x_view is not None:
                xv, B, H, W = x_view
            else:
                xv, B, H, W = x.view(), x.B, x.H, x.W
            y16 = y.compact16()
            stem = (self.Cin, self.Cout, self.kh, self.kw, self.s, self.p, self.d) == (3, 32, 3, 3, 1, 1, 1) and \
                self.bias is not None and gy.whole and gy.C == 32 and y16 is not None and \
                (gy.H, gy.W) == (H, W)
            if stem:  # the LDS-staged 3 -> 32 kernel, mask from y's fp16 copy
                with _timed("direct", "wgrad", self.flops(B, H, W), (3, 32, 3, 1, H, W)):
                    rc = lib.upr_t_conv_stem_wgrad_relu16(ctypes.byref(xv), gy.ptr(), _p(y16), B, H, W,
                                                          _p(self.m.weight.grad), _p(self.bias.grad), st)
                if took(rc, "conv_stem_wgrad_relu16"):
                    return
            if not y.only16:
                with _timed("direct", "wgrad", self.flops(B, gy.H, gy.W),
                            (self.Cin, self.Cout, self.kh, self.s, H, W)):
                    rc = lib.upr_t_conv_direct_wgrad_relu(ctypes.byref(xv), ctypes.byref(gy.view()),
                                                          ctypes.byref(y.view()), B, H, W, self.Cin, gy.H, gy.W,
                                                          self.Cout, self.kh, self.kw, self.s, self.p, self.d,
                                                          _p(self.m.weight.grad),
                                                          _p(self.bias.grad) if self.bias is not None else None, st)
                if took(rc, "conv_direct_wgrad_relu"):
                    return
        relu_mask(gy, y)
        self.bwd(x, gy, None, x_view=x_view)

    def bwd(self, x, gy, gx=None, x_view=None, mask=None, gx_only16=False, gx_keep16=False):
        """gy: Act gradient of this conv's output (pre-activation).
        Accumulates the weight / bias gradients; gx (Act, nullable) receives
        the input gradient (overwrite when fresh, else accumulate).
        mask = (a16, only16): the ReLU backward of the activation gx flows
        into, fused into the input-gradient epilogue (a16 = that activation's
        fp16 copy, a Half); gx's fp16 copy then holds the masked gradient and
        its fp32 values are not written when only16.  Returns True when the mask was applied.
        gx_only16: the input gradient's reader (a BatchNorm backward) takes its fp16
        copy: under autocast gx gets that copy and no fp32 store when fresh.
        gx_keep16: gx also gets its fp16 copy (fp32 kept), shared by gx's channel slices."""
        lib, st = L.lib(), _stream()
        if x_view is not None:
            xv, B, H, W = x_view
        else:
            B, H, W = x.B, x.H, x.W
        Ho, Wo = gy.H, gy.W
        F = self.flops(B, Ho, Wo)
        mf = self.mfma and x_view is None
        # autocast: gy's own fp16 copy (Half), compact or a channel slice of a shared concat copy
        h16 = gy.any16(grad=True) if self.amp and gy.C == self.Cout else None
        kw_ = ("mfma16" if self.amp and getattr(self, "x16", None) is not None else "mfma32") if mf else "direct"
        with _timed(None if self.frozen else kw_, "wgrad", F, (self.Cin, self.Cout, self.kh, self.s, H, W)):
            if not self.frozen:
                gw = self.m.weight.grad
                if self.mfma and x_view is None:
                    x16 = getattr(self, "x16", None)
                    # autocast: fp16 operands, fp32 accumulation (trainers/train.py:72); added
                    # straight into weight.grad's layout
                    # gy's fp16 copy (the fused BN backward's dx16) is the AMP A operand as is
                    # (in gy's own layout: the C ABI indexes dy16 like dy, so a slice of a shared concat
                    # copy passes the concat's base)
                    dy16 = h16.t if h16 is not None else None
                    if dy16 is None:
                        gy.need32("the weight gradient (its output gradient)")
                    if x16 is None:
                        x.need32("the weight gradient (its input)")
                    _chk(lib.upr_t_conv_wgrad_into(_fp(x.t), _p(x16) if self.amp else None, B, H, W, self.Cin, x.cs,
                                                   x.coff, _fp(gy.t), _p(dy16), Ho, Wo, self.Cout, gy.cs, gy.coff,
                                                   self.kh, self.kw, self.s, self.p, self.d, _p(gw), st),
                         "conv_wgrad")
                    self.x16 = None
                    if self.bias is not None:
                        chan_sum(gy, self.Cout, self.bias.grad, st)
                else:
                    v = x.view() if x_view is None else xv
                    _chk(lib.upr_t_conv_direct_wgrad(ctypes.byref(v), ctypes.byref(gy.view()), B, H, W, self.Cin, Ho, Wo,
                                                     self.Cout, self.kh, self.kw, self.s, self.p, self.d, _p(gw),
                                                     _p(self.bias.grad) if self.bias is not None else None, st),
                         "conv_direct_wgrad")
        if gx is None:
            return
        with _timed("mfma16" if self.amp else ("mfma32" if self.mfma else "direct"), "dgrad", F,
                    (self.Cin, self.Cout, self.kh, self.s, H, W)):
            if self.mfma:
                acc = gx.consume_fresh()
                src, sH, sW, scs, scoff = gy.t, Ho, Wo, gy.cs, gy.coff
                whole_gx = gx.whole and gx.C == self.Cin
                if mask is not None and self.amp and self.s == 1 and not acc and h16 is not None and whole_gx:
                    a16, only16 = mask
                    y16 = _h16(B * H * W * self.Cin, gx.t.device)
                    rc = lib.upr_t_conv_mfma16_relu_bwd_cs(h16.ptr(), h16.cs, B, Ho, Wo,
                                                           self.Cout, _p(self.wt16), self.Cin, self.kh, self.kw,
                                                           self.d * (self.kh - 1) - self.p, self.d, _fp(gx.t), gx.cs,
                                                           0, _p(y16), self.Cin, a16.ptr(), a16.cs, int(only16), st)
                    if took(rc, "conv_mfma16_relu_bwd"):
                        gx.attach16(y16, grad=True, only=only16)
                        return True
                # autocast: the fp16 operand comes from gy's producer (its compact copy; a channel
                # slice of a shared concat copy is read in place by the stride-1 convs only) or,
                # for stride 2, straight from an fp16 zero-upsample (no fp32 pass + cast)
                src16 = gy.compact16(self.Cout, grad=True) if self.amp else None
                x16 = h16 if src16 is not None or self.s == 1 else None
                if self.s == 2 and self.amp and H == 2 * Ho and W == 2 * Wo and \
                        ((self.kh, self.kw, self.p, self.d) == (3, 3, 1, 1) or
                         (acc and (self.kh, self.kw, self.p, self.d) == (1, 1, 0, 1))) and \
                        self._dgrad_s2(self.kh, gy, src16, B, Ho, Wo, gx, acc, bool(gx_only16) and whole_gx):
                    return
                if self.s != 1:
                    assert self.s == 2 and H == 2 * Ho and W == 2 * Wo, "stride-2 dgrad needs even sizes"
                    if self.amp and self.Cout % 8 == 0:
                        z16 = _h16(B * H * W * self.Cout, gy.t.device)
                        if gy.only16:
                            _chk(lib.upr_t_zero_upsample16h(_p(gy.compact16()), B, Ho, Wo, self.Cout, _p(z16), st),
                                 "zero_upsample16h")
                        else:
                            _chk(lib.upr_t_zero_upsample16(_fp(gy.t), B, Ho, Wo, self.Cout, gy.cs, gy.coff, _p(z16),
                                                           st), "zero_upsample16")
                        x16, src = Half(z16, self.Cout), None
                    else:
                        x16 = None
                        gy.need32("the stride-2 input gradient's zero-upsample")
                        z = empty((B, H, W, self.Cout), gy.t.device)
                        _chk(lib.upr_t_zero_upsample(_fp(gy.t), B, Ho, Wo, self.Cout, gy.cs, gy.coff,
                                                     _p(z), st), "zero_upsample")
                        src = z
                    sH, sW, scs, scoff = H, W, self.Cout, 0
                pad_t = self.d * (self.kh - 1) - self.p
                if x16 is None:
                    gy.need32("the input gradient conv")
                if self.amp:
                    o16 = bool(gx_only16) and whole_gx and not acc
                    k16 = o16 or (bool(gx_keep16) and whole_gx and not acc)
                    mfma16(src, B, sH, sW, self.Cout, scs, scoff, self.wt16, None, self.Cin, self.kh, self.kw, 1,
                           pad_t, self.d, gx if acc else None, False, gx, x16=x16, keep16=k16, only16=o16,
                           grad16=True, shared16=bool(gx_keep16))
                else:
                    _chk(lib.upr_t_conv_mfma(_fp(src), B, sH, sW, self.Cout, scs, scoff, _p(self.wt), None, self.Cin,
                                             self.kh, self.kw, 1, pad_t, self.d, gx.ptr() if acc else None,
                                             gx.cs if acc else 0, 0, _fp(gx.t), gx.cs, gx.coff, 0, st), "conv_dgrad")
            else:
                acc = gx.consume_fresh()
                g16 = gy.compact16(grad=True) if self.dgrad16_c3 else None
                if g16 is not None:
                    # autocast (VGG conv1_1): fp16 dy from the fused ReLU mask, MFMA
                    rc = lib.upr_t_conv_dgrad_c3_16(_p(g16), B, H, W, _p(self.m.weight), self.Cout,
                                                    ctypes.byref(gx.view()), int(acc), st)
                    if took(rc, "conv_dgrad_c3_16"):
                        return
                gy.need32("the direct input gradient")
                _chk(lib.upr_t_conv_direct_dgrad(ctypes.byref(gy.view()), Ho, Wo, _p(self.m.weight), B, H, W, self.Cin,
                                                 self.Cout, self.kh, self.kw, self.s, self.p, self.d,
                                                 ctypes.byref(gx.view()), acc, st), "conv_direct_dgrad")


class ConvT:
    """nn.ConvTranspose2d(k=2, s=2) (UpBlock.up, model.py:261): a GEMM with
    N = 4*Cout and a pixel-shuffle store; dgrad = k2 s2 conv over dy; wgrad =
    the same GEMM over pixels with dy as the 'input'."""

    def __init__(self, m):
        self.m = m
        self.Cin, self.Cout = m.weight.shape[0], m.weight.shape[1]
        self.wp = self.wp16 = self.wd16 = None
        self.amp = False

    def pack_jobs(self):
        w, amp = self.m.weight, _AMP[0]
        if self.wp is None:
            self.wp = torch.empty_like(w).view(-1)
            self.wd = torch.empty_like(w).view(-1)
            self.gp = torch.empty_like(w).view(-1)
            self.b4 = empty((4 * self.Cout,), w.device)
        if amp and self.wp16 is None:
            self.wp16, self.wd16 = _h16(w.numel(), w.device), _h16(w.numel(), w.device)
        n = w.numel()
        return [(w.data_ptr(), 0 if amp else self.wp.data_ptr(), self.wp16.data_ptr() if amp else 0, self.Cout,
                 self.Cin, 2, 2, 2, n),
                (w.data_ptr(), 0 if amp else self.wd.data_ptr(), self.wd16.data_ptr() if amp else 0, self.Cout,
                 self.Cin, 2, 2, 3, n),
                (self.m.bias.data_ptr(), self.b4.data_ptr(), 0, self.Cout, 1, 1, 1, 4, self.Cout)]

    def pack(self):
        pack_convs([self], self)

    def fwd(self, x):
        out = Act.new(x.B, 2 * x.H, 2 * x.W, self.Cout, x.t.device, fresh=False)
        self.amp = _AMP[0]
        with _timed("mfma16" if self.amp else "mfma32", "fwd", self.flops(x)):
            if self.amp:
                mfma16(x.t, x.B, x.H, x.W, self.Cin, x.cs, x.coff, self.wp16, self.b4, 4 * self.Cout, 1, 1,
                       1, 0, 1, None, False, out, store=L.UPR_T_STORE_CONVT2X2,
                       x16=x.any16() if x.compact16(self.Cin) is not None else None, keep16=True)
            else:
                _chk(L.lib().upr_t_conv_mfma(x.ptr(), x.B, x.H, x.W, self.Cin, x.cs, 0, _p(self.wp), _p(self.b4),
                                             4 * self.Cout, 1, 1, 1, 0, 1, None, 0, 0, _fp(out.t), out.cs, 0,
                                             L.UPR_T_STORE_CONVT2X2, _stream()), "convT")
        return out

    def flops(self, x):
        return 2.0 * x.B * x.H * x.W * self.Cin * 4 * self.Cout

    def bwd(self, x, gy, gx):
        lib, st = L.lib(), _stream()
        F = self.flops(x)
        kind = "mfma16" if self.amp else "mfma32"
        # gy's fp16 copy from its producer (UpBlockT: the following conv's input gradient,
        # gx_keep16) is both GEMMs' fp16 operand as is -- no internal cast passes
        gy16 = gy.compact16(grad=True) if self.amp else None
        with _timed(kind, "wgrad", F):
            zero(self.gp)
            # dwp[ci][(a,b,co)] = sum_p x[p][ci] * gy[2y+a][2x+b][co]: a k2 s2 "conv" of gy producing x
            if self.amp:
                _chk(lib.upr_t_conv_wgrad16(gy.ptr(), _p(gy16), gy.B, gy.H, gy.W, self.Cout, gy.cs, 0, x.ptr(), x.H, x.W,
                                            self.Cin, x.cs, 0, 2, 2, 2, 0, 1, _p(self.gp), st), "convT_wgrad16")
            else:
                _chk(lib.upr_t_conv_wgrad(gy.ptr(), gy.B, gy.H, gy.W, self.Cout, gy.cs, 0, x.ptr(), x.H, x.W, self.Cin,
                                          x.cs, 0, 2, 2, 2, 0, 1, _p(self.gp), st), "convT_wgrad")
            _chk(lib.upr_t_unpack_grad(_p(self.gp), _p(self.m.weight.grad), self.Cout, self.Cin, 2, 2, 3, 1, st),
                 "unpack")
            chan_sum(gy, self.Cout, self.m.bias.grad, st)
        with _timed(kind, "dgrad", F):
            acc = gx.consume_fresh()
            if self.amp:
                mfma16(gy.t, gy.B, gy.H, gy.W, self.Cout, gy.cs, gy.coff, self.wd16, None, self.Cin, 2, 2, 2,
                       0, 1, gx if acc else None, False, gx, x16=gy.any16() if gy16 is not None else None)
            else:
                _chk(lib.upr_t_conv_mfma(gy.ptr(), gy.B, gy.H, gy.W, self.Cout, gy.cs, 0, _p(self.wd), None, self.Cin, 2,
                                         2, 2, 0, 1, gx.ptr() if acc else None, gx.cs if acc else 0, 0, _fp(gx.t),
                                         gx.cs, gx.coff, 0, st), "convT_dgrad")


def pack_convs(convs, owner):
    """Re-pack every conv's weights for this step in ONE launch
    (upr_t_pack_weights); the device job table is rebuilt only when a pointer,
    shape or the autocast mode changed, and is kept alive on `owner`."""
    jobs = []
    for c in convs:
        jobs += c.pack_jobs()
    if not jobs:
        return
    key = tuple(jobs)
    tab = getattr(owner, "_pack_tab", None)
    if tab is None or tab[0] != key:
        arr = (L.UprPackJob * len(jobs))(*[L.UprPackJob(*j) for j in jobs])
        host = torch.frombuffer(bytearray(arr), dtype=torch.uint8)
        dev = convs[0].m.weight.device
        owner._pack_tab = (key, host.to(dev), len(jobs), max(j[-1] for j in jobs))
    _, t, nj, mx = owner._pack_tab
    _chk(L.lib().upr_t_pack_weights(_p(t), nj, mx, _stream()), "pack_weights")

