"""nn.BatchNorm2d forward / backward and the per-channel sum (csrc/train_bn.hip)."""
import ctypes

import torch

from .. import _lib as L
from .._dev import _chk, _fp, _h16, _p, _stream, empty, took, zero
from .act import Act
from .ops import relu_mask
from .state import _AMP


class BN:
    """nn.BatchNorm2d: training mode (batch statistics, running-stat update) or,
    when the module is in eval mode, the running statistics (a standalone
    submodule forward, upr/modules.py)."""

    def __init__(self, m):
        self.m = m
        self.C = m.num_features
        dev = m.weight.device
        self.mean = empty((self.C,), dev)
        self.invstd = empty((self.C,), dev)
        # per-channel sums + the two-stage reduction's partial slots (upr_t_reduce_acc_doubles)
        self.acc = torch.empty((L.lib().upr_t_reduce_acc_doubles(self.C),), dtype=torch.float64, device=dev)

    def fwd(self, x, relu=False, out=None, res=None, res_post=False, only16=False, out16=None):
        """only16: under autocast every reader of the output takes its fp16 copy (convs
        whose weight gradients run on the fp16-operand GEMM): the fp32 output is not
        written (out.only16).  out16 (Half): `out` is a channel slice of a concat whose
        fp16 copy the caller assembles; the slice's fp16 values go there (and with only16
        its fp32 values are not written); self.wrote16 tells whether they did."""
        self.wrote16 = False
        lib, st = L.lib(), _stream()
        m = self.m
        # under autocast x is an fp16 conv's output: its fp16 copy holds the same values
        x16 = x.compact16(self.C) if _AMP[0] else None
        self.x16 = x16
        if m.training:
            # fp16 input: statistics and finalise in two launches (upr_t_bn_stats16_fin)
            if x16 is None or not took(
                    lib.upr_t_bn_stats16_fin(_p(x16), x.M, self.C, _p(self.acc), ctypes.c_float(m.momentum),
                                             ctypes.c_float(m.eps), _p(m.running_mean), _p(m.running_var),
                                             _p(m.num_batches_tracked), _p(self.mean), _p(self.invstd), st),
                    "bn_stats16_fin"):
                x.need32("the BatchNorm statistics")
                _chk(lib.upr_t_bn_stats(x.ptr(), x.M, self.C, x.cs, 0, _p(self.acc), st), "bn_stats")
                _chk(lib.upr_t_bn_finalize(_p(self.acc), x.M, self.C, ctypes.c_float(m.momentum),
                                           ctypes.c_float(m.eps), _p(m.running_mean), _p(m.running_var),
                                           _p(m.num_batches_tracked), _p(self.mean), _p(self.invstd), st),
                     "bn_finalize")
        else:
            _chk(lib.upr_t_bn_eval_stats(_p(m.running_mean), _p(m.running_var), self.C, ctypes.c_float(m.eps),
                                         _p(self.mean), _p(self.invstd), st), "bn_eval_stats")
        if out is None:
            out = Act.new(x.B, x.H, x.W, self.C, x.t.device, fresh=False)
        if out16 is not None and _AMP[0] and x16 is not None and res is None:
            # a concat slice: fp16 values into the caller's copy (no fallback: the fp16
            # input path always exists here, and a half-written copy must not be claimed)
            skip32 = int(bool(only16))
            _chk(lib.upr_t_bn_apply16h_cs(_p(x16), x.M, self.C, _p(self.mean), _p(self.invstd), _p(m.weight),
                                          _p(m.bias), None, 0, 0, 0, int(relu), _fp(out.t), out.cs, out.coff,
                                          out16.ptr(), out16.cs, skip32, st),
                 "bn_apply16h_cs")
            self.wrote16 = True
            # (the slice object; the caller marks the concat.  An unfused backward that
            # would mask with this output refuses an fp16-only one, below in bwd)
            if skip32:
                out.attach16(out16, only=True)
            else:
                out.drop16()
            return self._keep(x, out, relu, None, False)
        # under autocast the consumer is an fp16 conv: write its fp16 input copy here
        y16 = _h16(out.M * self.C, out.t.device) if _AMP[0] and out.whole and out.C == self.C else None
        skip32 = int(bool(only16) and y16 is not None)
        done = False
        if x16 is not None:
            rc = lib.upr_t_bn_apply16h(_p(x16), x.M, self.C, _p(self.mean), _p(self.invstd), _p(m.weight),
                                       _p(m.bias), res.ptr() if res is not None else None,
                                       res.cs if res is not None else 0, 0, int(res_post), int(relu), _fp(out.t),
                                       out.cs, out.coff, _p(y16), skip32, st)
            done = took(rc, "bn_apply")
        if not done:
            skip32 = 0
            x.need32("the BatchNorm apply")
            rc = lib.upr_t_bn_apply16(x.ptr(), x.M, self.C, x.cs, 0, _p(self.mean), _p(self.invstd), _p(m.weight),
                                      _p(m.bias), res.ptr() if res is not None else None,
                                      res.cs if res is not None else 0, 0, int(res_post), int(relu), _fp(out.t),
                                      out.cs, out.coff, _p(y16), st)
            _chk(rc, "bn_apply")
        if y16 is not None:
            out.attach16(y16, only=skip32)
        else:
            out.drop16()
        return self._keep(x, out, relu, res, res_post)

    def _keep(self, x, out, relu, res, res_post):
        self.x = x
        self.out_act = out
        self.batch_stats = bool(self.m.training)  # the backward follows the statistics this forward used
        # y = relu(bn(x)) (+ a residual added after the ReLU): the backward may fold the mask in
        self.relu_only = bool(relu) and (res is None or bool(res_post))
        self.has_res = res is not None
        return out

    def bwd(self, g, gx, relu=False, only16=False):
        """g: Act gradient of the BN output; relu=True: g is the gradient of
        relu(bn(x)) (+ a residual added after the ReLU, res_post: this
        forward's relu=True), the ReLU mask is folded into the BN backward
        (recomputed from x, no separate pass; the residual does not enter it).
        Under autocast the input gradient also gets its compact fp16 copy
        (marked a gradient's) for the input-gradient conv that consumes it; only16 (the
        consumer's Conv.takes16_grad()): the fp32 gx is not written at all."""
        lib, st = L.lib(), _stream()
        m, x = self.m, self.x
        assert not relu or self.relu_only, "ReLU fold needs a relu(bn(x)) forward"
        if g.coff % 4 == 0 and gx.coff % 4 == 0:
            dx16 = _h16(gx.M * self.C, gx.t.device) if _AMP[0] and gx.whole and gx.C == self.C else None
            acc = 0 if gx.fresh else 1
            skip32 = int(bool(only16) and dx16 is not None and acc == 0)
            # g's fp16 copy (the input-gradient conv's fp16 output) when it has one
            g16 = g.compact16(self.C, grad=True)
            done = False
            if self.x16 is not None:
                rc = lib.upr_t_bn_bwd_fused16(_fp(g.t), _p(g16), g.cs, g.coff, _p(self.x16), _p(self.mean),
                                              _p(self.invstd), _p(m.weight), _p(m.bias), int(relu), x.M, self.C,
                                              _p(self.acc), _p(m.weight.grad), _p(m.bias.grad), _fp(gx.t), gx.cs,
                                              gx.coff, acc, int(self.batch_stats), _p(dx16), skip32, st)
                done = took(rc, "bn_bwd_fused")
            if not done:
                skip32 = 0
                x.need32("the BatchNorm backward (its input)")
                g.need32("the BatchNorm backward (its output gradient)")
                rc = lib.upr_t_bn_bwd_fused(_fp(g.t), g.cs, g.coff, x.ptr(), x.cs, _p(self.mean), _p(self.invstd),
                                            _p(m.weight), _p(m.bias), int(relu), x.M, self.C, _p(self.acc),
                                            _p(m.weight.grad), _p(m.bias.grad), _fp(gx.t), gx.cs, gx.coff, acc,
                                            int(self.batch_stats), _p(dx16), st)
                done = took(rc, "bn_bwd_fused")
            if done:
                gx.consume_fresh()
                if dx16 is not None:
                    gx.attach16(dx16, grad=True, only=skip32)
                return
        if relu:
            # the mask comes from the stored output here: with a post-ReLU
            # residual that output is relu(bn(x)) + skip, not the ReLU's own
            # output, and the mask would be wrong wherever skip > 0 >= bn(x)
            if self.has_res:
                raise NotImplementedError("unfused ReLU backward of relu(bn(x)) + skip: the mask needs the "
                                          "pre-residual value (the fused BatchNorm backward takes this layer)")
            self.out_act.need32("the unfused ReLU backward of a BatchNorm output (its mask)")
            relu_mask(g, self.out_act)
        zero(self.acc[:2 * self.C])
        _chk(lib.upr_t_bn_bwd_reduce(_fp(g.t), g.cs, g.coff, x.ptr(), x.cs, 0, _p(self.mean), _p(self.invstd), x.M,
                                     self.C, _p(self.acc), st), "bn_bwd_reduce")
        acc = gx.consume_fresh()
        _chk(lib.upr_t_bn_bwd_apply(_fp(g.t), g.cs, g.coff, x.ptr(), x.cs, 0, _p(self.mean), _p(self.invstd),
                                    _p(m.weight), _p(self.acc), x.M, self.C, _p(m.weight.grad), _p(m.bias.grad),
                                    _fp(gx.t), gx.cs, gx.coff, acc, int(self.batch_stats), st), "bn_bwd_apply")


def chan_sum(g, C, out, st):
    """out[C] += per-channel sum of the Act g (conv bias gradients; two-stage, deterministic);
    of its fp16 copy when that is its only value."""
    lib = L.lib()
    ws = torch.empty((lib.upr_t_reduce_acc_doubles(C),), dtype=torch.float64, device=g.t.device)
    if not g.only16:
        _chk(lib.upr_t_chan_sum_ws(g.ptr(), g.M, C, g.cs, 0, _p(out), 1, _p(ws), st), "dbias")
    elif g.whole:
        _chk(lib.upr_t_chan_sum16(_p(g.compact16()), g.M, C, _p(out), 1, _p(ws), st), "dbias16")
    else:  # a slice of a shared concat copy
        _chk(lib.upr_t_chan_sum16s(g.any16().ptr(), g.M, C, g.cs, _p(out), 1, _p(ws), st), "dbias16s")

