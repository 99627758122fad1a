"""The reference's modules (models/model.py) as layer objects (csrc/train_fam.hip: the FAM attention)."""
import ctypes

import torch

from .. import _lib as L
from .._dev import _chk, _fp, _h16, _p, _stream, empty
from .act import Act, Concat, nchw_view
from .bn import BN
from .conv import Conv, ConvT
from .ops import add_into, maxpool_into, pointwise, relu_mask
from .state import FP16_ONLY_STORES


class ResBlockT:
    """ResBlock (model.py:100-135)."""

    def __init__(self, m):
        self.conv1, self.bn1 = Conv(m.conv1), BN(m.bn1)
        self.conv2, self.bn2 = Conv(m.conv2), BN(m.bn2)
        self.proj = len(m.shortcut) > 0
        if self.proj:
            self.sconv, self.sbn = Conv(m.shortcut[0]), BN(m.shortcut[1])

    def convs(self):
        return [self.conv1, self.conv2] + ([self.sconv] if self.proj else [])

    def fwd(self, x):
        self.x = x
        # a conv whose only reader is a BatchNorm keeps its output in fp16 only under
        # autocast (the BN reads the fp16 copy: the same values)
        c1 = self.conv1.fwd(x, only16=True)
        self.a1 = self.bn1.fwd(c1, relu=True, only16=self.conv2.wgrad16_ok(c1.W))
        c2 = self.conv2.fwd(self.a1, only16=True)
        sc = self.sbn.fwd(self.sconv.fwd(x, only16=True)) if self.proj else x
        self.out = self.bn2.fwd(c2, relu=True, res=sc)
        return self.out

    def bwd(self, g, gx):
        relu_mask(g, self.out)
        g_c2 = Act.new(g.B, g.H, g.W, self.conv2.Cout, g.t.device)
        self.bn2.bwd(g, g_c2, only16=self.conv2.takes16_grad())
        if self.proj:
            g_cs = Act.new(g.B, g.H, g.W, self.sconv.Cout, g.t.device)
            self.sbn.bwd(g, g_cs, only16=self.sconv.takes16_grad())
        else:
            add_into(gx, g)
        g_a1 = Act.new(self.a1.B, self.a1.H, self.a1.W, self.a1.C, g.t.device)
        self.conv2.bwd(self.a1, g_c2, g_a1, gx_only16=True)
        g_c1 = Act.new(g_a1.B, g_a1.H, g_a1.W, g_a1.C, g.t.device)
        self.bn1.bwd(g_a1, g_c1, relu=True, only16=self.conv1.takes16_grad())
        self.conv1.bwd(self.x, g_c1, gx)
        if self.proj:
            # after conv1's: the shortcut's input gradient accumulates (the 1x1
            # stride-2 one then adds at the even pixels only, _dgrad_s2_1x1);
            # fp32 addition commutes, so the sum is the same bits either order
            self.sconv.bwd(self.x, g_cs, gx)


class PreActResBlockT:
    """PreActResBlock (model.py:138-178)."""

    def __init__(self, m):
        self.bn1, self.conv1 = BN(m.bn1), Conv(m.conv1)
        self.bn2, self.conv2 = BN(m.bn2), Conv(m.conv2)
        self.proj = len(m.shortcut) > 0
        if self.proj:
            self.sconv, self.sbn = Conv(m.shortcut[0]), BN(m.shortcut[1])

    def convs(self):
        return [self.conv1, self.conv2] + ([self.sconv] if self.proj else [])

    def fwd(self, x):
        self.x = x
        self.o = self.bn1.fwd(x, relu=True)
        sc = self.sbn.fwd(self.sconv.fwd(self.o, only16=True)) if self.proj else x
        c1 = self.conv1.fwd(self.o, only16=True)
        self.a2 = self.bn2.fwd(c1, relu=True, only16=self.conv2.wgrad16_ok(c1.W))
        return self.conv2.fwd(self.a2, res=sc)

    def bwd(self, g, gx):
        dev = g.t.device
        g_a2 = Act.new(self.a2.B, self.a2.H, self.a2.W, self.a2.C, dev)
        self.conv2.bwd(self.a2, g, g_a2, gx_only16=True)
        g_c1 = Act.new(g_a2.B, g_a2.H, g_a2.W, g_a2.C, dev)
        self.bn2.bwd(g_a2, g_c1, relu=True, only16=self.conv1.takes16_grad())
        g_o = Act.new(self.o.B, self.o.H, self.o.W, self.o.C, dev)
        self.conv1.bwd(self.o, g_c1, g_o)
        if self.proj:
            g_cs = Act.new(g.B, g.H, g.W, self.sconv.Cout, dev)
            self.sbn.bwd(g, g_cs, only16=self.sconv.takes16_grad())
            self.sconv.bwd(self.o, g_cs, g_o)
        else:
            add_into(gx, g)
        self.bn1.bwd(g_o, gx, relu=True)


class ASPPT:
    """ASPPModule (model.py:181-251); Dropout(0.1) mask from a counter hash
    whose seed is drawn from torch's default generator (so, as with the
    reference's nn.Dropout, torch.manual_seed makes the masks reproducible)."""

    def __init__(self, m, dropout_mask_fn=None):
        self.c1, self.b1 = Conv(m.conv1x1[0]), BN(m.conv1x1[1])
        self.br = [(Conv(s[0]), BN(s[1])) for s in m.aspp_branches]
        self.gc, self.gb = Conv(m.global_pool[1]), BN(m.global_pool[2])
        self.fc, self.fb = Conv(m.fusion[0]), BN(m.fusion[1])
        self.p = m.fusion[3].p
        self.C = self.c1.Cout
        self.seed = 0
        self.mod = m

    def convs(self):
        return [self.c1, self.gc, self.fc] + [c for c, _ in self.br]

    def fwd(self, x):
        dev = x.t.device
        C, nb = self.C, len(self.br) + 2
        self.x = x
        # under autocast the branch BatchNorms and the global broadcast also write the
        # concat's fp16 copy (the fusion conv's operand); only that copy when the fusion
        # conv's weight gradient reads it too (the branch BatchNorm backwards recompute
        # their ReLU masks from their inputs: nothing else reads the concat)
        cat = Concat(x.B, x.H, x.W, C * nb, dev, only=FP16_ONLY_STORES[0] and self.fc.wgrad16_ok(x.W))
        for i, (cv, bn) in enumerate([(self.c1, self.b1)] + self.br):
            o, o16 = cat.part(C * i, C)
            bn.fwd(cv.fwd(x, only16=True), relu=True, out=o, out16=o16, only16=cat.only)
            cat.wrote(bn.wrote16)
        # global branch: mean -> 1x1 -> BN (over the batch) -> ReLU -> broadcast
        self.gm = Act.new(x.B, 1, 1, x.C, dev, fresh=False)
        _chk(L.lib().upr_t_pixel_sum(x.ptr(), x.B, x.H * x.W, x.C, x.cs, 0, ctypes.c_float(1.0 / (x.H * x.W)),
                                     _fp(self.gm.t), 0, _stream()), "gap")
        self.gp = self.gb.fwd(self.gc.fwd(self.gm), relu=True)
        if not cat.only:
            _chk(L.lib().upr_t_broadcast(_fp(self.gp.t), x.B, x.H * x.W, C, ctypes.c_float(1.0), _fp(cat.act.t),
                                         C * nb, C * (nb - 1), 0, _stream()), "broadcast")
        if cat.ok16:
            _chk(L.lib().upr_t_broadcast16(_fp(self.gp.t), x.B, x.H * x.W, C, ctypes.c_float(1.0), _p(cat.h.t),
                                           C * nb, C * (nb - 1), _stream()), "broadcast16")
        self.cat = cat.finish()
        self.a = self.fb.fwd(self.fc.fwd(self.cat, only16=True), relu=True)
        self.dropped = self.mod.training  # the backward applies the mask only when this forward drew one
        if not self.dropped:
            self.mask = None
            return self.a  # nn.Dropout in eval mode is the identity
        out = Act.new(x.B, x.H, x.W, C, dev, fresh=False)
        self.mask = torch.empty((out.t.numel(),), dtype=torch.uint8, device=dev)
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        pointwise(self.a.t, None, out.t, out.t.numel(), 2, mask_out=self.mask, p=self.p, seed=self.seed)
        return out

    def bwd(self, g, gx):
        dev = g.t.device
        C, nb, x = self.C, len(self.br) + 2, self.x
        g_a = Act.new(g.B, g.H, g.W, C, dev)
        if self.dropped:
            pointwise(g.t, None, g_a.t, g.t.numel(), 3, mask_in=self.mask, p=self.p)
            g_a.fresh = False
        else:
            add_into(g_a, g)
        g_cf = Act.new(g.B, g.H, g.W, C, dev)
        self.fb.bwd(g_a, g_cf, relu=True)
        g_cat = Act.new(g.B, g.H, g.W, C * nb, dev)
        self.fc.bwd(self.cat, g_cf, g_cat)
        # global branch
        g_gp = Act.new(x.B, 1, 1, C, dev, fresh=False)
        _chk(L.lib().upr_t_pixel_sum(_fp(g_cat.t), x.B, x.H * x.W, C, g_cat.cs, C * (nb - 1), ctypes.c_float(1.0),
                                     _fp(g_gp.t), 0, _stream()), "gsum")
        relu_mask(g_gp, self.gp)
        g_gc = Act.new(x.B, 1, 1, C, dev)
        self.gb.bwd(g_gp, g_gc)
        g_gm = Act.new(x.B, 1, 1, x.C, dev)
        self.gc.bwd(self.gm, g_gc, g_gm)
        # conv branches (the first one initialises gx)
        for i, (cv, bn) in enumerate([(self.c1, self.b1)] + self.br):
            gs = g_cat.slice(C * i, C)
            g_c = Act.new(g.B, g.H, g.W, C, dev)
            bn.bwd(gs, g_c, relu=True)
            cv.bwd(x, g_c, gx)
        acc = gx.consume_fresh()
        _chk(L.lib().upr_t_broadcast(_fp(g_gm.t), x.B, x.H * x.W, x.C, ctypes.c_float(1.0 / (x.H * x.W)), gx.ptr(),
                                     gx.cs, 0, acc, _stream()), "broadcast_bwd")


class UpBlockT:
    """UpBlock (model.py:254-274) + the caller's skip add (model.py:346-348)."""

    def __init__(self, m):
        self.up = ConvT(m.up)
        self.c1, self.b1 = Conv(m.conv[0]), BN(m.conv[1])
        self.c2, self.b2 = Conv(m.conv[3]), BN(m.conv[4])

    def convs(self):
        return [self.up, self.c1, self.c2]

    def fwd(self, x, skip=None):
        """skip=None: UpBlock.forward alone (model.py:271-274, no skip add)."""
        self.x = x
        self.u = self.up.fwd(x)
        c1 = self.c1.fwd(self.u, only16=True)
        self.a1 = self.b1.fwd(c1, relu=True, only16=self.c2.wgrad16_ok(c1.W))
        # the skip add (model.py:346-348) in the BatchNorm apply's epilogue: relu(bn(c2)) + skip,
        # the same fp32 operations as the separate add
        return self.b2.fwd(self.c2.fwd(self.a1, only16=True), relu=True, res=skip, res_post=skip is not None)

    def bwd(self, g, gx, g_skip=None):
        dev = g.t.device
        if g_skip is not None:
            add_into(g_skip, g)
        g_c2 = Act.new(g.B, g.H, g.W, g.C, dev)
        self.b2.bwd(g, g_c2, relu=True, only16=self.c2.takes16_grad())
        g_a1 = Act.new(g.B, g.H, g.W, g.C, dev)
        self.c2.bwd(self.a1, g_c2, g_a1, gx_only16=True)
        g_c1 = Act.new(g.B, g.H, g.W, g.C, dev)
        self.b1.bwd(g_a1, g_c1, relu=True, only16=self.c1.takes16_grad())
        g_u = Act.new(g.B, g.H, g.W, g.C, dev)
        self.c1.bwd(self.u, g_c1, g_u, gx_keep16=True)  # + the fp16 copy ConvT's backward reads
        self.up.bwd(self.x, g_u, gx)


class FAMT:
    """EnhancedFAM (model.py:11-97)."""

    def __init__(self, m):
        self.b1 = Conv(m.branch1)
        self.b2 = Conv(m.branch2_conv)
        self.b3a, self.b3b = Conv(m.branch3_conv1), Conv(m.branch3_conv2)
        self.b4a, self.b4b = Conv(m.branch4_conv1), Conv(m.branch4_conv2)
        self.fu = Conv(m.fusion)
        self.ca1, self.ca2 = Conv(m.channel_attention[1]), Conv(m.channel_attention[3])
        self.sa = Conv(m.spatial_attention[0])

    def convs(self):
        return [self.b1, self.b2, self.b3a, self.b3b, self.b4a, self.b4b, self.fu, self.ca1, self.ca2, self.sa]

    def takes16_input(self, W):
        """Under autocast, every reader of this module's input x of width W takes its
        fp16 copy: branch1 / branch3 / branch4's first convs (forward on that copy, weight
        gradients on the fp16 GEMM) and the 3x3 max-pool (fp16 path); the input may
        then be stored fp16-only."""
        return FP16_ONLY_STORES[0] and all(c.wgrad16_ok(W) for c in (self.b1, self.b3a, self.b4a))

    def fwd(self, x):
        dev = x.t.device
        lib, st = L.lib(), _stream()
        C = self.fu.Cout
        B, H, W = x.B, x.H, x.W
        HW = H * W
        self.x = x
        # under autocast the four branch convs also write the concat's fp16 copy (the fusion conv's operand).
        # fp16-only stores: the concat's fp32 slices are read by nothing when the fusion
        # conv's weight gradient runs on the fp16 GEMM (it reads the copy), and t3 / t4 by
        # nothing when branch3 / branch4's second conv's weight gradient does (the ReLU
        # backward masks with their fp16 copies); Act.need32 refuses any fp32 read
        # of an fp16-only activation
        cat = Concat(B, H, W, 4 * C, dev, only=FP16_ONLY_STORES[0] and self.fu.wgrad16_ok(W))

        def branch(conv, inp, k):
            o, o16 = cat.part(k * C, C)
            conv.fwd(inp, out=o, out16=o16, only16=cat.only)
            cat.wrote(conv.wrote16)
        branch(self.b1, x, 0)
        self.mp = Act.new(B, H, W, x.C, dev, fresh=False)
        self.mp_code = torch.empty(B * H * W * x.C, dtype=torch.uint8, device=dev)  # argmax codes for the backward
        # mp's readers: branch2's conv (forward: its fp16 copy; weight gradient: the fp16
        # GEMM when wgrad16_ok) -- the backward of the pool itself takes the argmax codes
        maxpool_into(x, self.mp, 3, 1, 1, self.mp_code, only16=FP16_ONLY_STORES[0] and self.b2.wgrad16_ok(W))
        branch(self.b2, self.mp, 1)
        self.t3 = self.b3a.fwd(x, relu=True, only16=FP16_ONLY_STORES[0] and self.b3b.wgrad16_ok(W))
        branch(self.b3b, self.t3, 2)
        self.t4 = self.b4a.fwd(x, relu=True, only16=FP16_ONLY_STORES[0] and self.b4b.wgrad16_ok(W))
        branch(self.b4b, self.t4, 3)
        self.cat = cat.finish()
        self.o = self.fu.fwd(self.cat, relu=True)
        self.pool = Act.new(B, 1, 1, C, dev, fresh=False)
        _chk(lib.upr_t_pixel_sum(_fp(self.o.t), B, HW, C, C, 0, ctypes.c_float(1.0 / HW), _fp(self.pool.t), 0, st),
             "gap")
        self.h1 = self.ca1.fwd(self.pool, relu=True)
        z = self.ca2.fwd(self.h1)
        self.ca = empty((B, C), dev)
        pointwise(z.t, None, self.ca, B * C, 0)
        self.o2 = empty((B, H, W, C), dev)
        self.m = Act.new(B, H, W, 2, dev, fresh=False)
        _chk(lib.upr_t_fam_ca_apply(_p(self.o.t), _p(self.ca), B, HW, C, _p(self.o2), _fp(self.m.t), st), "ca_apply")
        s_pre = self.sa.fwd(self.m)
        self.sav = empty((B, H, W), dev)
        out = Act.new(B, H, W, C, dev, fresh=False)
        _chk(lib.upr_t_fam_sa_apply(_p(self.o2), _fp(s_pre.t), B, HW, C, _p(self.sav), _fp(out.t), st), "sa_apply")
        return out

    def bwd(self, g, gx):
        """g: Act [B,H,W,32] (a channel slice of a wider tensor allowed); gx receives the input gradient."""
        dev = g.t.device
        lib, st = L.lib(), _stream()
        B, H, W, C = g.B, g.H, g.W, self.fu.Cout
        HW = H * W
        g_o2 = empty((B, H, W, C), dev)
        g_s = Act.new(B, H, W, 1, dev, fresh=False)
        g.need32("the EnhancedFAM backward")
        _chk(lib.upr_t_fam_sa_bwd_cs(g.ptr(), g.cs, _p(self.o2), _p(self.sav), B, HW, C, _p(g_o2), _fp(g_s.t), st),
             "sa_bwd")
        g_m = Act.new(B, H, W, 2, dev)
        self.sa.bwd(self.m, g_s, g_m)
        g_o = Act.new(B, H, W, C, dev, fresh=False)
        g_ca = empty((B, C), dev)
        _chk(lib.upr_t_fam_ca_bwd(_p(g_o2), _fp(g_m.t), _fp(self.o.t), _p(self.o2), _p(self.ca), B, HW, C, _fp(g_o.t),
                                  _p(g_ca), st), "ca_bwd")
        g_z = Act.new(B, 1, 1, C, dev, fresh=False)
        pointwise(g_ca, self.ca, g_z.t, B * C, 1)
        g_h1 = Act.new(B, 1, 1, self.h1.C, dev)
        self.ca2.bwd(self.h1, g_z, g_h1)
        relu_mask(g_h1, self.h1)
        g_pool = Act.new(B, 1, 1, C, dev)
        self.ca1.bwd(self.pool, g_h1, g_pool)
        # under autocast the fusion conv's gradient operand (its fp16 copy) comes out of the same pass
        g16 = _h16(g_o.M * C, dev) if self.fu.amp and self.fu.mfma else None
        _chk(lib.upr_t_fam_pool_bwd16(_fp(g_o.t), _fp(g_pool.t), _fp(self.o.t), B, HW, C, _p(g16), st), "pool_bwd")
        if g16 is not None:
            g_o.attach16(g16, grad=True)
        g_cat = Act.new(B, H, W, 4 * C, dev)
        # the four branch convs read slices of its fp16 copy; no fp32 store when every one of
        # them takes an fp16 gradient (their weight gradients on the fp16 GEMM: Wo % 64)
        only16 = all(c.takes16_grad() for c in (self.b1, self.b2, self.b3b, self.b4b))
        self.fu.bwd(self.cat, g_o, g_cat, gx_only16=only16, gx_keep16=True)
        self.b1.bwd(self.x, g_cat.slice(0, C), gx)
        g_mp = Act.new(B, H, W, self.x.C, dev)
        self.b2.bwd(self.mp, g_cat.slice(C, C), g_mp)
        gx.zero_if_fresh()
        _chk(lib.upr_t_maxpool_bwd_code(_p(self.mp_code), ctypes.byref(g_mp.view()), B, H, W, self.x.C, 3, 1, 1,
                                        H, W, ctypes.byref(gx.view()), 1, st), "maxpool_bwd")
        self.mp_code = None
        for (ca_, cb_, t) in ((self.b3a, self.b3b, self.t3), (self.b4a, self.b4b, self.t4)):
            k = 2 if cb_ is self.b3b else 3
            g_t = Act.new(B, H, W, t.C, dev)
            # the ReLU backward of t fused into this input gradient's epilogue (t's fp16 copy as
            # the mask); fp32 g_t skipped when the consuming conv takes the fp16 gradient only
            mask = (t.any16(), ca_.takes16_grad()) if t.compact16() is not None else None
            if not cb_.bwd(t, g_cat.slice(k * C, C), g_t, mask=mask):
                relu_mask(g_t, t, want16=ca_.amp and ca_.mfma)
            ca_.bwd(self.x, g_t, gx)


class IENetT:
    """ResidualIENet (model.py:277-360)."""

    def __init__(self, m):
        Blk = PreActResBlockT if m._use_preact else ResBlockT
        self.inp = Conv(m.input_layer)
        self.enc = [Blk(m.enc1), Blk(m.enc2), Blk(m.enc3)]
        self.mid = []
        for sub in m.bottleneck:
            self.mid.append(ASPPT(sub) if type(sub).__name__ == "ASPPModule" else Blk(sub))
        self.dec = [UpBlockT(m.dec3), UpBlockT(m.dec2), UpBlockT(m.dec1)]
        self.h0, self.h2 = Conv(m.residual_head[0]), Conv(m.residual_head[2])

    def convs(self):
        out = [self.inp, self.h0, self.h2]
        for b in self.enc + self.mid + self.dec:
            out += b.convs()
        return out

    def fwd(self, x):
        B, _, H, W = x.shape
        self.x = x  # keeps the input alive: the backward reads it through the raw view below
        self.xin = (nchw_view(x), B, H, W)
        self.x1 = self.inp.fwd(None, relu=True, x_view=self.xin, out=Act.new(B, H, W, 32, x.device, fresh=False))
        self.x2 = self.enc[0].fwd(self.x1)
        self.x3 = self.enc[1].fwd(self.x2)
        self.x4 = self.enc[2].fwd(self.x3)
        t = self.x4
        self.mids = []
        for b in self.mid:
            self.mids.append(t)
            t = b.fwd(t)
        self.x5 = t
        d3 = self.dec[0].fwd(self.x5, self.x3)
        d2 = self.dec[1].fwd(d3, self.x2)
        self.d1 = self.dec[2].fwd(d2, self.x1)
        self.d3, self.d2 = d3, d2
        self.h = self.h0.fwd(self.d1, relu=True)
        r = self.h2.fwd(self.h)
        illu = empty((B, 1, H, W), x.device)
        _chk(L.lib().upr_t_head_fwd(_p(x), _fp(r.t), _p(illu), B, H, W, _stream()), "head")
        return illu

    def bwd(self, g_r):
        """g_r: Act [B,H,W,1], gradient of the residual-head output."""
        dev = g_r.t.device
        B, H, W = g_r.B, g_r.H, g_r.W

        def like(a):
            return Act.new(a.B, a.H, a.W, a.C, dev)
        g_h = like(self.h)
        self.h2.bwd(self.h, g_r, g_h)
        # under autocast the masked gradient's fp16 copy (h0's input-gradient / weight-
        # gradient operand) comes out of the mask pass, not a separate cast
        relu_mask(g_h, self.h, want16=self.h0.amp and self.h0.mfma)
        g_d1 = like(self.d1)
        self.h0.bwd(self.d1, g_h, g_d1)
        g_x1, g_x2, g_x3 = like(self.x1), like(self.x2), like(self.x3)
        g_d2, g_d3 = like(self.d2), like(self.d3)
        self.dec[2].bwd(g_d1, g_d2, g_x1)
        self.dec[1].bwd(g_d2, g_d3, g_x2)
        g_t = like(self.x5)
        self.dec[0].bwd(g_d3, g_t, g_x3)
        for b, xin in zip(reversed(self.mid), reversed(self.mids)):
            g_in = like(xin)
            b.bwd(g_t, g_in)
            g_t = g_in
        self.enc[2].bwd(g_t, g_x3)
        self.enc[1].bwd(g_x3, g_x2)
        self.enc[0].bwd(g_x2, g_x1)
        self.inp.bwd_relu_stem(None, g_x1, self.x1, x_view=self.xin)

