"""The whole network's training step graph: MultiScaleUP_Retinex forward and backward."""
import ctypes

from .. import _lib as L
from .._dev import _chk, _fp, _p, _stream, empty, took, zero
from .act import Act, Concat, nchw_view
from .blocks import FAMT, IENetT
from .conv import Conv, pack_convs
from .state import autocast_active, set_amp


class UPRetinexTrainGraph:
    """MultiScaleUP_Retinex.forward (model.py:415-455) in training mode and its
    backward.  Built once per model; buffers are reallocated per step by the
    caching allocator (torch.empty), weights re-packed per step."""

    def __init__(self, model, head_only=False):
        """head_only: the multi-scale enhancement head alone (multi_scale_enhance
        with a caller-given reflectance, model.py:415-443), no IENet."""
        self.model = model
        self.ie = None if head_only else IENetT(model.ie_net)
        self.s1c, self.s1f = Conv(model.scale1[0]), FAMT(model.scale1[2])
        self.s2c, self.s2f = Conv(model.scale2[1]), FAMT(model.scale2[3])
        self.s3c, self.s3f = Conv(model.scale3[1]), FAMT(model.scale3[3])
        self.fusion, self.outc = Conv(model.fusion), Conv(model.output_layer)
        self._convs = (self.ie.convs() if self.ie is not None else []) + \
            [self.s1c, self.s2c, self.s3c, self.fusion, self.outc] + \
            self.s1f.convs() + self.s2f.convs() + self.s3f.convs()

    def pack(self):
        pack_convs(self._convs, self)

    def forward(self, x):
        """x [B,3,H,W] fp32 NCHW (H, W multiples of 16) -> (enh, refl, illu)."""
        lib, st = L.lib(), _stream()
        B, _, H, W = x.shape
        dev = x.device
        self.x = x
        set_amp(autocast_active())
        self.pack()
        illu = self.ie.fwd(x)
        self.illu = illu
        o = self._head_fwd(x)
        self.e = empty((B, H, W, 3), dev)
        refl = empty((B, 3, H, W), dev)
        enh = empty((B, 3, H, W), dev)
        _chk(lib.upr_t_retinex_fwd(_p(x), _p(illu), _fp(o.t), _p(self.e), _p(refl), _p(enh), B, H, W, st),
             "retinex")
        self.refl, self.enh = refl, enh
        return enh, refl, illu

    def enhance_forward(self, x, refl):
        """Head only: x, refl [B,3,H,W] fp32 NCHW (H, W multiples of 16) -> enh."""
        lib, st = L.lib(), _stream()
        B, _, H, W = x.shape
        self.x = x
        set_amp(autocast_active())
        self.pack()
        o = self._head_fwd(x)
        self.e = empty((B, H, W, 3), x.device)
        enh = empty((B, 3, H, W), x.device)
        _chk(lib.upr_t_enhance_fwd(_p(refl), _fp(o.t), _p(self.e), _p(enh), B, H, W, st), "enhance")
        self.refl, self.enh = refl, enh
        return enh

    def enhance_backward(self, g_enh, want_refl):
        """Head only: parameter gradients into the .grad views; returns dL/drefl
        (None unless want_refl)."""
        lib, st = L.lib(), _stream()
        B, _, H, W = self.x.shape
        g_o = Act.new(B, H, W, 3, self.x.device, fresh=False)
        g_refl = empty((B, 3, H, W), self.x.device) if want_refl else None
        _chk(lib.upr_t_enhance_bwd(_p(self.e), _p(self.refl), _p(g_enh), _fp(g_o.t), _p(g_refl), B, H, W, st),
             "enhance_bwd")
        self._head_bwd(g_o)
        return g_refl

    def _head_fwd(self, x):
        """scale1/2/3 -> concat -> fusion -> output_layer (model.py:415-440): the
        pre-sigmoid output [B,H,W,3] (Act)."""
        lib, st = L.lib(), _stream()
        B, _, H, W = x.shape
        dev = x.device
        # pyramid (model.py:415-432): bilinear 0.5 / 0.25, max-pool 2 / 4
        xv = nchw_view(x)
        pyr = []
        for f, k in ((2, 2), (4, 4)):
            xs = Act.new(B, H // f, W // f, 3, dev, fresh=False)
            _chk(lib.upr_t_bilinear(ctypes.byref(xv), B, H, W, 3, ctypes.byref(xs.view()), H // f, W // f, 0, st),
                 "bilinear")
            xp = Act.new(B, H // f // k, W // f // k, 3, dev, fresh=False)
            _chk(lib.upr_t_maxpool(ctypes.byref(xs.view()), B, H // f, W // f, 3, k, k, 0, ctypes.byref(xp.view()),
                                   H // f // k, W // f // k, st), "maxpool")
            pyr.append(xp)
        self.pyr = pyr
        # the scale stems' outputs fp16-only where every reader takes fp16 (FAMT.takes16_input;
        # the stems' own ReLU backward masks with the fp16 copy)
        self.s1 = self.s1c.fwd(None, relu=True, x_view=(xv, B, H, W),
                               out=Act.new(B, H, W, 32, dev, fresh=False), only16=self.s1f.takes16_input(W))
        f1 = self.s1f.fwd(self.s1)
        self.s2 = self.s2c.fwd(pyr[0], relu=True, only16=self.s2f.takes16_input(pyr[0].W))
        f2 = self.s2f.fwd(self.s2)
        self.s3 = self.s3c.fwd(pyr[1], relu=True)
        f3 = self.s3f.fwd(self.s3)
        # under autocast the concat's fp16 copy (the fusion conv's operand) is written alongside;
        # only that copy when the fusion conv's weight gradient also reads it (wm = 2)
        cat = Concat(B, H, W, 96, dev, only=self.fusion.wgrad16_ok(W))
        wm = 2 if cat.only else 0
        for i, f in enumerate((f1, f2, f3)):
            if not cat.ok16:  # no fp16 copy, or an earlier slice's kernel did not take the shape
                break
            o, o16 = cat.part(32 * i, 32)
            if i == 0:
                rc = lib.upr_t_copy16(ctypes.byref(f.view()), ctypes.byref(o.view()), B, H, W, 32, wm, o16.ptr(),
                                      o16.cs, st)
            else:
                rc = lib.upr_t_bilinear16(ctypes.byref(f.view()), B, f.H, f.W, 32, ctypes.byref(o.view()), H, W, wm,
                                          o16.ptr(), o16.cs, st)
            cat.wrote(took(rc, "cat16"))
        if not cat.ok16:  # every slice in fp32 (whatever the fp16 attempt left behind)
            _chk(lib.upr_t_copy(ctypes.byref(f1.view()), ctypes.byref(cat.act.slice(0, 32).view()), B, H, W, 32, 0, st),
                 "cat")
            for i, f in enumerate((f2, f3)):
                _chk(lib.upr_t_bilinear(ctypes.byref(f.view()), B, f.H, f.W, 32,
                                        ctypes.byref(cat.act.slice(32 * (i + 1), 32).view()), H, W, 0, st), "upsample")
        self.fused = cat.finish(all32=not cat.ok16)
        self.fz = self.fusion.fwd(self.fused)
        self.f_hw = [(f2.H, f2.W), (f3.H, f3.W)]
        return self.outc.fwd(self.fz)

    def backward(self, g_enh, g_refl=None, g_illu=None):
        """Accumulates every parameter gradient into the model's .grad views
        (zeroed first by the caller)."""
        lib, st = L.lib(), _stream()
        x = self.x
        B, _, H, W = x.shape
        dev = x.device
        g_o = Act.new(B, H, W, 3, dev, fresh=False)
        g_r = Act.new(B, H, W, 1, dev, fresh=False)
        _chk(lib.upr_t_retinex_bwd(_p(x), _p(self.illu), _p(self.e), _p(self.refl), _p(g_enh), _p(g_refl),
                                   _p(g_illu), _fp(g_o.t), _fp(g_r.t), B, H, W, st), "retinex_bwd")
        self._head_bwd(g_o)
        self.ie.bwd(g_r)

    def _head_bwd(self, g_o):
        """Backward of _head_fwd from dL/d(output_layer output) (Act [B,H,W,3])."""
        lib, st = L.lib(), _stream()
        x = self.x
        B, _, H, W = x.shape
        dev = x.device
        g_fz = Act.new(B, H, W, 32, dev)
        self.outc.bwd(self.fz, g_o, g_fz)
        g_fused = Act.new(B, H, W, 96, dev)
        self.fusion.bwd(self.fused, g_fz, g_fused)
        for (sc, sf, s_act, xin), i in zip(((self.s1c, self.s1f, self.s1, None),
                                            (self.s2c, self.s2f, self.s2, self.pyr[0]),
                                            (self.s3c, self.s3f, self.s3, self.pyr[1])), range(3)):
            if i == 0:
                g_f = g_fused.slice(0, 32)  # read in place by the FAM backward (no split copy)
            else:
                g_f = Act.new(s_act.B, s_act.H, s_act.W, 32, dev, fresh=False)
                zero(g_f.t)
                _chk(lib.upr_t_bilinear_bwd(ctypes.byref(g_fused.slice(32 * i, 32).view()), B, g_f.H, g_f.W, 32, H, W,
                                            ctypes.byref(g_f.view()), st), "upsample_bwd")
            g_s = Act.new(s_act.B, s_act.H, s_act.W, 32, dev)
            sf.bwd(g_f, g_s)
            if i == 0:
                sc.bwd_relu_stem(None, g_s, s_act, x_view=(nchw_view(x), B, H, W))
            else:
                sc.bwd_relu_stem(xin, g_s, s_act)
