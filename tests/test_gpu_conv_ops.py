"""Op-level parity of the direct (small-channel) training convolutions
(csrc/train_small.hip and the generic kernels of csrc/train_conv.hip) and of
the conv helpers (upr_t_pack_weight / _pack_weights / _unpack_grad /
_zero_upsample* / _cast_f16) against the float64 reference oracle/conv_ops.py
(run with `-m gpu`).  Every entry is called through ctypes (upr._lib.lib()) on
inputs made on the CPU with a fixed seed, one op at a time: an op's operands
are never another kernel's output.  Outputs a call overwrites start as the
sentinel, outputs it adds to (accumulate = 1, every dw / dbias) start random.

Views (class View): "nhwc" contiguous, "nchw", "slice4" / "slice8" a channel
slice of a 12-channels-wider NHWC buffer (op_parity.LAYOUTS; the other
channels are checked bit for bit), "off1" a slice one float past alignment of
a 3-wider buffer (forces the scalar / generic forms), (extra, coff) any other
width.

Shapes: which kernel and branch each case reaches (MI355X: 256 CUs).

  forward, upr_t_conv_direct / upr_t_conv_direct16                  FWD_MFMA
    3 -> 32 / 64, 3x3, stride 1, y channel-contiguous and 16-byte aligned:
    c3k3_mfma_kernel<32 / 64>, 16-pixel groups, 4 a block, grid min(groups / 4, 8 CUs)
      (1, 3, 5)      P = 15: less than one group
      (2, 13, 7)     P = 182: 11 full groups and one of 6 pixels; pad 0 / 1 / 2
      (1, 40, 72)    180 groups, one pass
      (1, 364, 364)  8281 groups > 4 * 8 * 256: the pre-loaded next group is
                     used and 89 waves make a second pass (grown if more CUs)
    the same with y off1 / NCHW, or Cout 16 / 48: conv_direct_c3k3_kernel   FWD_C3K3
      (upr_t_conv_direct16 on that view answers UPR_ERR_UNSUPPORTED)
    1x1, Cin 16 / 32 / 64 aligned, Cout 1..4: head1x1_kernel<Cout, Cin / 4>  HEAD_P
      P = 1, 63 (one partial wave), 261 = 64 * 4 + 5 (a second block of 5)
      x off1: small_fwd_kernel<Cout> without xvec (scalar loop only)
    Cin 6 in an 8-wide buffer: small_fwd_kernel<2>, xvec quad, then 2 scalar    FWD_SMALL
    7x7 2 -> 1 pad 3; 3x3 stride 2 pad 1 at odd H, W; dilation 2: small_fwd_kernel
    Cout 5; Cout 4 with Cin 64, 7x7 (50176 bytes of LDS > 48 KiB):
    conv_direct_kernel                                                         FWD_GENERIC

  input gradient, upr_t_conv_direct_dgrad                           DGRAD
    Cin 3, Cout 64, dy aligned NHWC: small_dgrad_kernel<3, 64> compile-time loop
      P = 255 / 256 / 257 pixels: one block less a thread, one block, two
      dy off1: the same kernel's scalar loop over all 64
    Cin 3, Cout 32: <3, 0> dvec quads (dy nhwc, slice4), dilation 2, pad 0 (Ho = H - 2)
    Cin 2, 7x7, Cout 1: <2, 0>;  Cin 1: <1, 0>
    Cin 32, Cout 3, dy [.., 3]: <32, 0> scalar loop; dy in a 4- or 8-wide
      buffer: dvec with no full quad; Cout 6 in 8-wide: one quad + 2 scalar
      dx NCHW: scalar stores; dx aligned NHWC: 16-byte stores; accumulate both
    stride 2 (even and odd H, W), Cin 4, Cin 16: conv_direct_dgrad_kernel

  weight gradient, upr_t_conv_direct_wgrad / _wgrad_relu             WGRAD_MFMA
    columns Cin kh kw (+ 1 with dbias) <= 128, Cout <= 32:
    small_wgrad_mfma_kernel<1..4> (8 pixel pairs a batch, 16 at two tiles)
      27 + 1 one tile; 36 + 1 two; 72 + 1 three; 98 (dbias NULL) and 98 + 1
      (wgrad_relu) four; 32 + 1 two and 32 exactly one; 127 + 1 exactly 128
      P = 1; P odd (the last pair has one pixel); P = 66 = 2 * 8 * 4 + 2 (a
      second block of one pair); stride 2; dilation 2; x NCHW; dy a slice
    128 + 1 columns; 3 -> 64; 16 -> 4 3x3 (145 columns):
    conv_direct_wgrad_kernel (LDS chunks of 64 pixels, a partial row a block) WGRAD_GENERIC
      (1, 260, 260): 1057 chunks > 1024 blocks, so 33 blocks take two
    7x7 2 -> 1 pad 3 with dbias: sa_wgrad_kernel, 8 x 64 tiles              SA_SHAPES
      (1, 5, 9) one partial tile; (2, 13, 70) tails both ways, two images;
      (1, 8, 64) exactly one tile; (1, 16, 128) 2 x 2 full tiles
      dbias NULL: small_wgrad_mfma_kernel<4> on the same shapes
    1x1 32 -> 1 / 3, x aligned: pw_wgrad_kernel<32, 1 / 3>, 4 rows a block  PW_SHAPES
      (3, 5, 17) 15 rows: a block straddles two images, the last has 3 rows
      (1, 4, 300) a second pass of the pixel loop (44 pixels); (2, 2, 40)
      x off1: small_wgrad_mfma_kernel<2>

Tolerances (tests/op_parity.py, as test_gpu_fam_ops.py): the kernel's error
against float64 within 4x the error of plain fp32 torch on the CPU (F.conv2d
and its autograd), at least half an ulp of the largest |reference|, and under
1e-4 * max|ref| + 1e-6; per output tensor, and for dw also per output channel.
One rounding or none (fp16 copies, layout helpers, untouched channels, refused
calls, run-to-run determinism of the forms built without atomics): torch.equal.

Measured on the MI355X: max |error| against float64 in ulp of the case's
largest |reference|, the worst case of each group; "used" is the worst kernel
error / allowed error over all cases (1 would fail).  The slowest test takes
0.9 s (the first input-gradient case, which also loads the kernels), the
364 x 364 forward cases 0.3-0.4 s, every other under 0.2 s; the file 4 s.

  group (calls)                                              restatement   kernel   used
  fwd c3k3_mfma<32> (6)                                          2.22       3.05    0.44
  fwd c3k3_mfma<64> (6)                                          4.30       4.17    0.43
  fwd direct16 y (6)                                             4.34       3.27    0.35
  fwd conv_direct_c3k3 (7)                                       4.28       3.13    0.35
  fwd head1x1 (72)                                               6.19       6.19    0.36
  fwd small_fwd scalar (1x1, off1 x) (36)                       24.78       3.57    0.64
  fwd small_fwd (8)                                              4.36       2.43    0.36
  fwd conv_direct (generic) (5)                                 17.30      13.44    0.38
  dgrad small_dgrad<3,64> (3)                                    2.24       5.36    0.69
  dgrad small_dgrad<3,64> scalar dy (1)                          1.72       3.83    0.56
  dgrad small_dgrad<3,0> (3)                                     7.21       3.00    0.27
  dgrad small_dgrad<3,0> scalar dy (1)                           7.26       3.13    0.11
  dgrad small_dgrad<2,0> (2)                                     2.62       3.46    0.36
  dgrad small_dgrad<1,0> (2)                                     1.89       1.74    0.23
  dgrad small_dgrad<32,0> scalar dy (2)                          0.77       0.77    0.25
  dgrad small_dgrad<32,0> dvec (4)                               1.75       4.39    0.63
  dgrad conv_direct_dgrad (generic) (5)                          2.57       3.72    0.73
  wgrad small_wgrad_mfma<1> dw (8)                               9.43       2.22    0.25
  wgrad small_wgrad_mfma<1> dw per channel (8)                   9.43       2.22    0.55
  wgrad small_wgrad_mfma<1> dbias (6)                            1.19       1.19    0.25
  wgrad small_wgrad_mfma<2> dw (3)                               5.11       2.10    0.17
  wgrad small_wgrad_mfma<2> dw per channel (3)                   5.11       2.10    0.25
  wgrad small_wgrad_mfma<2> dbias (3)                            2.06       0.97    0.30
  wgrad small_wgrad_mfma<3> dw (2)                               3.74       1.45    0.19
  wgrad small_wgrad_mfma<3> dw per channel (2)                   3.74       1.45    0.33
  wgrad small_wgrad_mfma<3> dbias (2)                            0.60       1.48    0.72
  wgrad small_wgrad_mfma<4> dw (4)                               6.26       1.41    0.18
  wgrad small_wgrad_mfma<4> dw per channel (4)                   6.26       1.41    0.28
  wgrad small_wgrad_mfma<4> dbias (3)                            2.40       2.40    0.25
  wgrad_relu small_wgrad_mfma<4> dw (1)                          3.92       1.25    0.08
  wgrad_relu small_wgrad_mfma<4> dw per channel (1)              3.92       1.25    0.08
  wgrad_relu small_wgrad_mfma<4> dbias (1)                       8.66       6.66    0.19
  wgrad_relu small_wgrad_mfma<1> dw (2)                          1.64       0.98    0.22
  wgrad_relu small_wgrad_mfma<1> dw per channel (2)              1.64       0.98    0.53
  wgrad_relu small_wgrad_mfma<1> dbias (1)                       0.57       0.70    0.30
  wgrad_relu small_wgrad_mfma<2> dw (1)                          2.01       1.56    0.19
  wgrad_relu small_wgrad_mfma<2> dw per channel (1)              2.01       1.56    0.35
  wgrad_relu small_wgrad_mfma<2> dbias (1)                       0.74       0.74    0.25
  wgrad sa_wgrad (tiled 7x7) dw (8)                              6.83       1.15    0.10
  wgrad sa_wgrad (tiled 7x7) dw per channel (8)                  6.83       1.15    0.10
  wgrad sa_wgrad (tiled 7x7) dbias (8)                          27.20      31.20    0.29
  wgrad small_wgrad_mfma<4> (7x7, no dbias) dw (4)               6.83       1.58    0.12
  wgrad small_wgrad_mfma<4> (7x7, no dbias) dw per channel (4)     6.83       1.58    0.12
  wgrad pw_wgrad<32,1> dw (6)                                    6.16       2.28    0.19
  wgrad pw_wgrad<32,1> dw per channel (6)                        6.16       2.28    0.19
  wgrad pw_wgrad<32,1> dbias (3)                                 4.82      11.18    0.58
  wgrad small_wgrad_mfma<2> (1x1, off1 x) dw (6)                 6.16       2.46    0.30
  wgrad small_wgrad_mfma<2> (1x1, off1 x) dw per channel (6)     6.16       2.46    0.34
  wgrad small_wgrad_mfma<2> (1x1, off1 x) dbias (6)              4.82      11.18    0.58
  wgrad pw_wgrad<32,3> dw (6)                                    3.34       1.43    0.17
  wgrad pw_wgrad<32,3> dw per channel (6)                        3.34       1.43    0.36
  wgrad pw_wgrad<32,3> dbias (3)                                 1.36       3.64    0.67
  wgrad conv_direct_wgrad (generic) dw (5)                      66.26       3.00    0.45
  wgrad conv_direct_wgrad (generic) dw per channel (5)          66.26       3.00    0.50
  wgrad conv_direct_wgrad (generic) dbias (4)                    1.69       2.81    0.43

  torch.equal groups (y16, skip32, refused calls, untouched channels, 16-byte
  vs scalar loads, run-to-run determinism of every weight-gradient form, the
  layout helpers, zero_upsample*, cast_f16): no difference.

Five cases missed the bound as first written, each a long sequential chain of
fp32 additions; the kernels now add in shorter chains.
  * sa_wgrad_kernel, dbias at (1, 16, 128): 14.84 ulp against the restatement's
    0.16 (7.4x the allowed error): a thread added 4 rows x 64 columns in one
    chain.  Now 8 interleaved sums a row, a tree over them and over the rows.
  * small_wgrad_mfma_kernel<2>, dbias at (3, 5, 17), off1 x: 36.8 ulp of a
    cancelling sum against 4.8 (1.9x): two tiles run 16 pixel pairs a batch, a
    chain of 32 an accumulator; the pairs now alternate between two.
  * conv_direct_wgrad_kernel, dbias at (1, 260, 260): 7.02 ulp against 1.69
    (1.04x): 1024 blocks' fp32 atomics in arrival order.  Now a partial row a
    block, added in block order by small_wgrad_fin_kernel (2.8 ulp, and the
    same bits run to run).
  * small_dgrad_kernel<3, 64> at (1, 16, 16): 7.98 ulp against 1.93 (1.04x): one
    chain of 9 x 64 terms.  Now two partial sums (four in the run-time-Cout
    forms).
  * small_fwd_kernel's scalar loop, 1x1 over 32 / 64 channels: 3.18 ulp against
    0.79 and 2.42 against 0.58 (1.01x, 1.05x).  Now four partial sums; the
    16-byte and the scalar loads add in the same order (bit-equal).
The four direct-conv entries beside upr_t_conv_direct now make its argument
checks (and all five also refuse H, W, kh, kw <= 0 and pad < 0).
"""
import collections
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import has_gpu
from op_parity import DEV, LAYOUTS, P, SENT, _np, _within_restated
from oracle import conv_ops as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]


def _lib():
    from upr import _lib as L
    return L, L.lib(), torch.cuda.current_stream().cuda_stream


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _is_sent(t):
    return torch.equal(t, torch.full_like(t, SENT))


def _eq(a, b, what):
    assert torch.equal(a.cpu(), b.cpu()), f"{what}: not bit-equal"


class View:
    """A logical [B, H, W, C] CPU tensor placed on the device in `layout`,
    with the UprView that describes it."""

    def __init__(self, t, layout="nhwc"):
        from upr._lib import UprView
        B, H, W, C = t.shape
        self.shape, self.layout = (B, H, W, C), layout
        if layout == "nchw":
            host, self.coff = _nchw(t).contiguous(), 0
            strides = (C * H * W, W, 1, H * W)
        else:
            extra, self.coff = (0, 0) if layout == "nhwc" else LAYOUTS.get(layout, layout)
            cs = C + extra
            host = torch.full((B, H, W, cs), SENT, dtype=t.dtype)
            host[..., self.coff:self.coff + C] = t
            strides = (H * W * cs, W * cs, cs, 1)
        self.buf = host.to(DEV)
        self.v = UprView(self.buf.data_ptr() + 4 * self.coff, *strides)
        self.ref = ctypes.byref(self.v)

    def get(self):
        if self.layout == "nchw":
            return self.buf.permute(0, 2, 3, 1).cpu()
        return self.buf[..., self.coff:self.coff + self.shape[3]].cpu()

    def untouched(self, what):
        """Channels of the wider buffer outside the slice still hold the sentinel."""
        if self.layout == "nchw":
            return
        C = self.shape[3]
        for part in (self.buf[..., :self.coff], self.buf[..., self.coff + C:]):
            assert _is_sent(part), f"{what}: wrote outside its channel slice"


def _sent_view(shape, layout="nhwc"):
    return View(torch.full(shape, SENT), layout)


Conv = collections.namedtuple("Conv", "B H W Cin Cout k s p d xl yl bias relu acc",
                              defaults=(1, 0, 1, "nhwc", "nhwc", 1, 0, 0))


def _osz(c):
    return O.out_size(c.H, c.k, c.s, c.p, c.d), O.out_size(c.W, c.k, c.s, c.p, c.d)


@functools.lru_cache(maxsize=2)
def _inputs(B, H, W, Cin, Cout, k, s, p, d):
    """Seeded CPU operands of one conv geometry, N(0, 1): x, w, bias, dy, the
    accumulate operands y0 / dx0 and the gradients' starting values dw0 / db0."""
    g = _gen(B, H, W, Cin, Cout, k, s, p, d)
    Ho, Wo = O.out_size(H, k, s, p, d), O.out_size(W, k, s, p, d)
    shapes = {"x": (B, H, W, Cin), "w": (Cout, Cin, k, k), "bias": (Cout,), "dy": (B, Ho, Wo, Cout),
              "y0": (B, Ho, Wo, Cout), "dx0": (B, H, W, Cin), "dw0": (Cout, Cin, k, k), "db0": (Cout,)}
    return {n: torch.randn(sh, generator=g) for n, sh in shapes.items()}


def _in(c):
    return _inputs(c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.s, c.p, c.d)


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
def _fwd_call(c, y16=None, skip32=0, entry16=False):
    """One upr_t_conv_direct (or _direct16) call; returns (rc, the y view)."""
    _, lib, st = _lib()
    d = _in(c)
    Ho, Wo = _osz(c)
    xv = View(d["x"], c.xl)
    yv = View(d["y0"], c.yl) if c.acc else _sent_view((c.B, Ho, Wo, c.Cout), c.yl)
    w, bias = d["w"].to(DEV), (d["bias"].to(DEV) if c.bias else None)
    args = (xv.ref, c.B, c.H, c.W, c.Cin, P(w), P(bias), c.Cout, c.k, c.k, c.s, c.p, c.d, yv.ref, Ho, Wo, c.relu, c.acc)
    rc = lib.upr_t_conv_direct16(*args, y16, skip32, st) if entry16 else lib.upr_t_conv_direct(*args, st)
    torch.cuda.synchronize()
    return rc, yv


def _fwd_refs(c):
    d = _in(c)
    x, w, b = d["x"], d["w"], (d["bias"] if c.bias else None)
    ref = O.conv_fwd(_np(x), _np(w), None if b is None else _np(b), c.s, c.p, c.d, bool(c.relu),
                     _np(d["y0"]) if c.acc else None)
    rst = F.conv2d(_nchw(x), w, b, c.s, c.p, c.d).permute(0, 2, 3, 1)
    if c.acc:
        rst = rst + d["y0"]
    if c.relu:
        rst = torch.relu(rst)
    return ref, rst


def _fwd(c, group):
    rc, yv = _fwd_call(c)
    assert rc == 0, (group, c, rc)
    ref, rst = _fwd_refs(c)
    tag = f"{group} | {tuple(c)}"
    _within_restated(tag, yv.get(), ref, rst)
    yv.untouched(tag)
    return yv


def _big_side():
    """The side of the square image with more 16-pixel groups than one pass of
    c3k3_mfma_kernel's grid takes (4 * 8 * CUs): 364 at 256 CUs."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 364
    while (n * n + 15) // 16 <= 4 * 8 * cus:
        n += 4
    return n


# (B, H, W, pad, x layout, y layout, bias, relu, accumulate); H = 0: the second-pass image
FWD_MFMA = [
    (1, 3, 5, 1, "nchw", "nhwc", 1, 0, 0),
    (2, 13, 7, 1, "nchw", "nhwc", 1, 1, 0),
    (2, 13, 7, 0, "slice4", "nhwc", 0, 0, 1),
    (2, 13, 7, 2, "nhwc", "slice4", 1, 1, 1),
    (1, 40, 72, 1, "nchw", "slice8", 0, 1, 0),
    (1, 0, 0, 1, "nchw", "nhwc", 1, 1, 0),
]


@pytest.mark.parametrize("Cout", [32, 64])
@pytest.mark.parametrize("case", FWD_MFMA, ids=lambda t: "-".join(map(str, t)))
def test_fwd_c3k3_mfma(case, Cout):
    B, H, W, p, xl, yl, bias, relu, acc = case
    if H == 0:
        H = W = _big_side()
    _fwd(Conv(B, H, W, 3, Cout, 3, 1, p, 1, xl, yl, bias, relu, acc), f"fwd c3k3_mfma<{Cout}>")


@pytest.mark.parametrize("Cout", [32, 64])
@pytest.mark.parametrize("B,H,W,p,relu", [(2, 13, 7, 1, 1), (1, 40, 72, 1, 0), (2, 13, 7, 2, 0)])
def test_fwd_direct16(B, H, W, p, relu, Cout):
    """upr_t_conv_direct16: y16 is (half)y bit for bit; with skip32 y keeps the
    sentinel and y16 is the same."""
    c = Conv(B, H, W, 3, Cout, 3, 1, p, 1, "nchw", "nhwc", 1, relu, 0)
    Ho, Wo = _osz(c)
    y16 = torch.full((B * Ho * Wo, Cout), SENT, dtype=torch.float16, device=DEV)
    rc, yv = _fwd_call(c, P(y16), 0, entry16=True)
    assert rc == 0
    ref, rst = _fwd_refs(c)
    _within_restated(f"fwd direct16 y | {tuple(c)}", yv.get(), ref, rst)
    _eq(y16.view(B, Ho, Wo, Cout), yv.get().half(), "y16 vs (half)y")
    y16s = torch.full_like(y16, SENT)
    rc, ys = _fwd_call(c, P(y16s), 1, entry16=True)
    assert rc == 0
    assert _is_sent(ys.buf), "skip32 wrote y"
    _eq(y16s, y16, "y16 with skip32")


def test_fwd_direct16_refusals():
    """skip32 with accumulate and a NULL y16: UPR_ERR_ARG; Cout <= 4 and a y16
    off 8-byte alignment: UPR_ERR_UNSUPPORTED; nothing written."""
    L, _, _ = _lib()
    c = Conv(2, 13, 7, 3, 32, 3, 1, 1, 1, "nchw", "nhwc", 1, 0, 0)
    Ho, Wo = _osz(c)
    y16 = torch.full((c.B * Ho * Wo * c.Cout + 4,), SENT, dtype=torch.float16, device=DEV)
    for cc, ptr, skip, want in [(c._replace(acc=1), P(y16), 1, L.UPR_ERR_ARG), (c, None, 0, L.UPR_ERR_ARG),
                                (c, P(y16, 1), 0, L.UPR_ERR_UNSUPPORTED),
                                (c._replace(Cout=4), P(y16), 0, L.UPR_ERR_UNSUPPORTED)]:
        rc, yv = _fwd_call(cc, ptr, skip, entry16=True)
        assert rc == want, (cc, rc, want)
        assert _is_sent(y16)
        if cc.acc:
            _eq(yv.get(), _in(cc)["y0"], "a refused call changed y")
        else:
            assert _is_sent(yv.buf)


# (B, H, W, Cout, pad, x layout, y layout, bias, relu, accumulate)
FWD_C3K3 = [
    (1, 3, 5, 32, 1, "nchw", "off1", 1, 0, 0),
    (2, 13, 7, 32, 1, "nchw", "nchw", 1, 1, 1),
    (2, 13, 7, 32, 0, "slice4", "off1", 0, 1, 0),
    (1, 40, 72, 32, 1, "nchw", "off1", 1, 0, 1),
    (2, 13, 7, 64, 2, "nhwc", "nchw", 1, 0, 0),
    (2, 13, 7, 16, 1, "nchw", "nhwc", 1, 1, 0),
    (2, 13, 7, 48, 2, "nhwc", "slice4", 0, 0, 1),
]


@pytest.mark.parametrize("case", FWD_C3K3, ids=lambda t: "-".join(map(str, t)))
def test_fwd_c3k3_generic(case):
    """The 3-channel 3x3 shapes off the MFMA form's y layout or channel
    counts: conv_direct_c3k3_kernel; upr_t_conv_direct16 refuses the view."""
    L, _, _ = _lib()
    B, H, W, Cout, p, xl, yl, bias, relu, acc = case
    c = Conv(B, H, W, 3, Cout, 3, 1, p, 1, xl, yl, bias, relu, acc)
    _fwd(c, "fwd conv_direct_c3k3")
    Ho, Wo = _osz(c)
    y16 = torch.full((B * Ho * Wo, Cout), SENT, dtype=torch.float16, device=DEV)
    rc, yv = _fwd_call(c._replace(acc=0), P(y16), 0, entry16=True)
    assert rc == L.UPR_ERR_UNSUPPORTED and _is_sent(y16) and _is_sent(yv.buf)


HEAD_P = [(1, 1, 1), (1, 7, 9), (1, 9, 29)]  # P = 1, 63, 261 = 64 * 4 + 5


@pytest.mark.parametrize("Cout", [1, 2, 3, 4])
@pytest.mark.parametrize("Cin", [16, 32, 64])
def test_fwd_head1x1(Cin, Cout):
    """head1x1_kernel<Cout, Cin / 4> on aligned x (contiguous and a slice),
    y NHWC and NCHW, bias / relu / accumulate varied over the cases; the same
    on off1 x: small_fwd_kernel<Cout>'s scalar loop."""
    n = 0
    for B, H, W in HEAD_P:
        for xl in ("nhwc", "slice4", "off1"):
            yl = ("nchw", "nhwc", "slice8")[n % 3]
            bias, relu, acc = (n + 1) % 4 != 0, (n // 2) % 2, (n // 3) % 2
            group = "fwd small_fwd scalar (1x1, off1 x)" if xl == "off1" else "fwd head1x1"
            _fwd(Conv(B, H, W, Cin, Cout, 1, 1, 0, 1, xl, yl, int(bias), relu, acc), group)
            n += 1


# (B, H, W, Cin, Cout, k, s, p, d, x layout, y layout, bias, relu, accumulate)
FWD_SMALL = [
    Conv(1, 9, 29, 6, 2, 1, 1, 0, 1, (2, 0), "nhwc", 1, 0, 0),   # xvec: one quad, then 2 scalar channels
    Conv(1, 9, 29, 6, 2, 1, 1, 0, 1, "off1", "nchw", 1, 1, 1),   # scalar loop
    Conv(2, 13, 70, 2, 1, 7, 1, 3, 1, "nhwc", "nhwc", 1, 0, 0),  # the spatial attention conv
    Conv(2, 13, 70, 2, 1, 7, 1, 3, 1, "nchw", "slice4", 0, 1, 1),
    Conv(1, 13, 9, 8, 4, 3, 2, 1, 1, "nhwc", "nhwc", 1, 1, 0),   # stride 2, odd H and W; xvec quads only
    Conv(1, 13, 9, 3, 3, 3, 2, 1, 1, "nchw", "nchw", 0, 0, 1),
    Conv(2, 11, 10, 4, 2, 3, 1, 2, 2, "slice4", "nhwc", 1, 0, 0),  # dilation 2
    Conv(2, 11, 10, 5, 3, 3, 1, 0, 2, "nhwc", "off1", 1, 1, 0),   # dilation 2, pad 0: Ho = H - 4
]


@pytest.mark.parametrize("c", FWD_SMALL, ids=lambda c: "-".join(map(str, c)))
def test_fwd_small(c):
    _fwd(c, "fwd small_fwd")


def test_vector_and_scalar_loads_agree():
    """small_fwd_kernel and small_dgrad_kernel add in the same order whether
    they load 16 bytes or scalars: an aligned and an off1 operand give the
    same bits."""
    for c in (Conv(1, 13, 9, 8, 4, 3, 2, 1, 1, "nhwc", "nhwc", 1, 1, 0), Conv(1, 9, 29, 6, 2, 1, 1, 0, 1, (2, 0), "nhwc")):
        (rc, a), (rc1, b) = _fwd_call(c), _fwd_call(c._replace(xl="off1"))
        assert rc == 0 and rc1 == 0
        _eq(a.get(), b.get(), f"small_fwd 16-byte vs scalar x {tuple(c)}")
    for c in (Conv(1, 15, 17, 3, 64, 3, 1, 1, 1, "nchw", "nhwc"), Conv(2, 13, 7, 3, 32, 3, 1, 1, 1, "nchw", "slice4"),
              Conv(1, 15, 17, 32, 6, 3, 1, 1, 1, "nhwc", (2, 0))):
        (rc, a), (rc1, b) = _dgrad_call(c), _dgrad_call(c._replace(yl="off1"))
        assert rc == 0 and rc1 == 0
        _eq(a.get(), b.get(), f"small_dgrad 16-byte vs scalar dy {tuple(c)}")


FWD_GENERIC = [
    Conv(2, 13, 7, 7, 5, 3, 1, 1, 1, "nhwc", "nhwc", 1, 0, 0),
    Conv(1, 13, 9, 7, 5, 3, 2, 1, 1, "nchw", "slice4", 0, 1, 1),
    Conv(1, 11, 10, 4, 5, 3, 1, 2, 2, "slice4", "nchw", 1, 1, 0),
    Conv(1, 5, 6, 64, 4, 7, 1, 3, 1, "nhwc", "nhwc", 1, 0, 0),    # 50176 bytes of weights: over the LDS limit
    Conv(1, 5, 6, 64, 4, 7, 1, 3, 1, "slice4", "off1", 1, 1, 1),
]


@pytest.mark.parametrize("c", FWD_GENERIC, ids=lambda c: "-".join(map(str, c)))
def test_fwd_generic(c):
    _fwd(c, "fwd conv_direct (generic)")


# ---------------------------------------------------------------------------
# input gradient
# ---------------------------------------------------------------------------
def _autograd32(c, dy=None):
    """Plain fp32 torch on the CPU: (dx, dw, dbias) of F.conv2d by autograd."""
    d = _in(c)
    x, w = _nchw(d["x"]).clone().requires_grad_(True), d["w"].clone().requires_grad_(True)
    dy = d["dy"] if dy is None else dy
    F.conv2d(x, w, None, c.s, c.p, c.d).backward(_nchw(dy))
    return x.grad.permute(0, 2, 3, 1), w.grad, dy.sum((0, 1, 2))


def _dgrad_call(c, Ho=None, Wo=None, **over):
    _, lib, st = _lib()
    d = _in(c)
    ho, wo = _osz(c)
    dyv = View(d["dy"], c.yl)
    dxv = View(d["dx0"], c.xl) if c.acc else _sent_view((c.B, c.H, c.W, c.Cin), c.xl)
    w = d["w"].to(DEV)
    a = dict(dy=dyv.ref, Ho=ho if Ho is None else Ho, Wo=wo if Wo is None else Wo, w=P(w), B=c.B, H=c.H, W=c.W,
             Cin=c.Cin, Cout=c.Cout, kh=c.k, kw=c.k, s=c.s, p=c.p, d=c.d, dx=dxv.ref, acc=c.acc)
    a.update(over)
    rc = lib.upr_t_conv_direct_dgrad(*a.values(), st)
    torch.cuda.synchronize()
    return rc, dxv


def _dgrad(c, group):
    rc, dxv = _dgrad_call(c)
    assert rc == 0, (group, c, rc)
    d = _in(c)
    ref = O.conv_dgrad(_np(d["dy"]), _np(d["w"]), c.H, c.W, c.s, c.p, c.d)
    rst = _autograd32(c)[0]
    if c.acc:
        ref, rst = ref + _np(d["dx0"]), rst + d["dx0"]
    tag = f"{group} | {tuple(c)}"
    _within_restated(tag, dxv.get(), ref, rst)
    dxv.untouched(tag)


# Conv(.., xl = dx layout, yl = dy layout, bias unused, relu unused, acc)
DGRAD = [
    ("small_dgrad<3,64>", Conv(1, 15, 17, 3, 64, 3, 1, 1, 1, "nchw", "nhwc", 0, 0, 0)),   # P = 255
    ("small_dgrad<3,64>", Conv(1, 16, 16, 3, 64, 3, 1, 1, 1, "nhwc", "slice4", 0, 0, 1)),  # P = 256
    ("small_dgrad<3,64>", Conv(1, 1, 257, 3, 64, 3, 1, 1, 1, "nchw", "nhwc", 0, 0, 1)),   # P = 257
    ("small_dgrad<3,64> scalar dy", Conv(1, 15, 17, 3, 64, 3, 1, 1, 1, "nchw", "off1", 0, 0, 0)),
    ("small_dgrad<3,0>", Conv(2, 13, 7, 3, 32, 3, 1, 1, 1, "nchw", "nhwc", 0, 0, 0)),
    ("small_dgrad<3,0>", Conv(2, 13, 7, 3, 32, 3, 1, 0, 1, "slice4", "slice4", 0, 0, 1)),  # pad 0: Ho = H - 2
    ("small_dgrad<3,0>", Conv(2, 11, 10, 3, 32, 3, 1, 2, 2, "nchw", "nhwc", 0, 0, 0)),    # dilation 2
    ("small_dgrad<3,0> scalar dy", Conv(2, 13, 7, 3, 32, 3, 1, 1, 1, "off1", "nchw", 0, 0, 1)),
    ("small_dgrad<2,0>", Conv(2, 13, 70, 2, 1, 7, 1, 3, 1, "nhwc", "nhwc", 0, 0, 0)),     # dy [.., 1]: scalar loads
    ("small_dgrad<2,0>", Conv(2, 13, 70, 2, 1, 7, 1, 3, 1, "nchw", "off1", 0, 0, 1)),
    ("small_dgrad<1,0>", Conv(1, 16, 16, 1, 4, 3, 1, 1, 1, "nhwc", "nhwc", 0, 0, 0)),
    ("small_dgrad<1,0>", Conv(1, 15, 17, 1, 5, 3, 1, 2, 2, "nchw", (3, 0), 0, 0, 1)),     # one quad + 1 scalar
    ("small_dgrad<32,0> scalar dy", Conv(1, 1, 257, 32, 3, 1, 1, 0, 1, "nchw", "nhwc", 0, 0, 0)),
    ("small_dgrad<32,0> scalar dy", Conv(1, 15, 17, 32, 3, 1, 1, 0, 1, "nhwc", "nhwc", 0, 0, 1)),
    ("small_dgrad<32,0> dvec", Conv(1, 15, 17, 32, 3, 1, 1, 0, 1, "nhwc", (1, 0), 0, 0, 0)),   # 4-wide: no full quad
    ("small_dgrad<32,0> dvec", Conv(1, 16, 16, 32, 3, 1, 1, 0, 1, "nchw", (5, 0), 0, 0, 1)),   # 8-wide
    ("small_dgrad<32,0> dvec", Conv(1, 15, 17, 32, 6, 1, 1, 0, 1, "slice4", (2, 0), 0, 0, 1)),  # one quad + 2 scalar
    ("small_dgrad<32,0> dvec", Conv(1, 15, 17, 32, 6, 3, 1, 1, 1, "off1", (2, 0), 0, 0, 0)),   # scalar stores
    ("conv_direct_dgrad (generic)", Conv(1, 12, 14, 3, 32, 3, 2, 1, 1, "nchw", "nhwc", 0, 0, 0)),  # stride 2, even
    ("conv_direct_dgrad (generic)", Conv(1, 13, 9, 3, 32, 3, 2, 1, 1, "nhwc", "slice4", 0, 0, 1)),  # stride 2, odd
    ("conv_direct_dgrad (generic)", Conv(2, 13, 9, 32, 3, 1, 2, 0, 1, "nhwc", "nhwc", 0, 0, 0)),    # 1x1 stride 2
    ("conv_direct_dgrad (generic)", Conv(2, 13, 7, 4, 5, 3, 1, 1, 1, "nhwc", "nhwc", 0, 0, 0)),
    ("conv_direct_dgrad (generic)", Conv(2, 11, 10, 16, 4, 3, 1, 2, 2, "slice4", "nchw", 0, 0, 1)),
]


@pytest.mark.parametrize("group,c", DGRAD, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_dgrad(group, c):
    _dgrad(c, "dgrad " + group)


# ---------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------
def _mask_of(c):
    """The masking ReLU output: N(0, 1) with 0.0, -0.0 and NaN planted."""
    Ho, Wo = _osz(c)
    m = torch.randn((c.B, Ho, Wo, c.Cout), generator=_gen("mask", *c[:9]))
    flat = m.view(-1)
    flat[0::5], flat[1::5], flat[2::5] = 0.0, -0.0, float("nan")
    return m


def _wgrad_call(c, mask=None, x_layout=None, **over):
    """One upr_t_conv_direct_wgrad (or _wgrad_relu with mask) call from the
    random dw0 / db0; returns (rc, dw, dbias, the sentinel bias buffer a
    dbias = NULL call must leave alone)."""
    _, lib, st = _lib()
    d = _in(c)
    Ho, Wo = _osz(c)
    xv, dyv = View(d["x"], x_layout or c.xl), View(d["dy"], c.yl)
    dw, db = d["dw0"].to(DEV), d["db0"].to(DEV)
    spare = torch.full((c.Cout,), SENT, device=DEV)
    a = dict(x=xv.ref, dy=dyv.ref)
    if mask is not None:
        mv = View(mask, "nhwc")
        a["y"] = mv.ref
    a.update(B=c.B, H=c.H, W=c.W, Cin=c.Cin, Ho=Ho, Wo=Wo, Cout=c.Cout, kh=c.k, kw=c.k, s=c.s, p=c.p, d=c.d, dw=P(dw),
             dbias=P(db) if c.bias else None)
    a.update(over)
    fn = lib.upr_t_conv_direct_wgrad if mask is None else lib.upr_t_conv_direct_wgrad_relu
    rc = fn(*a.values(), st)
    torch.cuda.synchronize()
    return rc, dw, db, spare


def _wgrad_check(c, dw, db, group, mask=None):
    d = _in(c)
    dy = d["dy"] if mask is None else torch.where(mask > 0, d["dy"], torch.zeros(()))
    dw64, db64 = O.conv_wgrad(_np(d["x"]), _np(d["dy"]), c.k, c.k, c.s, c.p, c.d,
                              None if mask is None else mask.numpy())
    _, dw32, db32 = _autograd32(c, dy)
    tag = f"{group} | {tuple(c)}"
    ref, rst = _np(d["dw0"]) + dw64, d["dw0"] + dw32
    _within_restated(tag + " dw", dw, ref, rst)
    co = c.Cout
    _within_restated(tag + " dw per channel", dw.reshape(co, -1).T, ref.reshape(co, -1).T, rst.reshape(co, -1).T,
                     per_channel=True)
    if c.bias:
        _within_restated(tag + " dbias", db, _np(d["db0"]) + db64, d["db0"] + db32)
    else:
        _eq(db, d["db0"], "dbias = NULL: the bias gradient")


def _wgrad(c, group, mask=None, twice=False, x_layout=None):
    rc, dw, db, spare = _wgrad_call(c, mask, x_layout)
    assert rc == 0, (group, c, rc)
    assert _is_sent(spare)
    _wgrad_check(c, dw, db, group, mask)
    if twice:
        rc, dw2, db2, _ = _wgrad_call(c, mask, x_layout)
        assert rc == 0
        _eq(dw2, dw, f"{group}: dw run to run")
        _eq(db2, db, f"{group}: dbias run to run")
    return dw, db


# Conv(.., xl = x layout, yl = dy layout, bias = dbias given, relu unused, acc unused)
WGRAD_MFMA = [
    ("<1> 27+1", Conv(1, 1, 1, 3, 32, 3, 1, 1, 1, "nchw", "nhwc", 1)),       # P = 1
    ("<1> 27+1", Conv(1, 5, 7, 3, 32, 3, 1, 1, 1, "nchw", "slice4", 1)),     # P = 35: the last pair has one pixel
    ("<1> 27+1", Conv(1, 6, 11, 3, 5, 3, 1, 1, 1, "nhwc", "nhwc", 1)),       # P = 66: a second block of one pair
    ("<1> 27+1", Conv(2, 24, 24, 3, 32, 3, 1, 1, 1, "nchw", "nhwc", 1)),
    ("<1> 27", Conv(2, 24, 24, 3, 32, 3, 1, 1, 1, "nchw", "nhwc", 0)),
    ("<1> 27+1", Conv(2, 13, 9, 3, 1, 3, 2, 1, 1, "nchw", "off1", 1)),       # stride 2, odd H and W
    ("<1> 27+1", Conv(2, 11, 10, 3, 5, 3, 1, 2, 2, "slice4", "nchw", 1)),    # dilation 2
    ("<2> 36+1", Conv(2, 13, 7, 4, 5, 3, 1, 1, 1, "nhwc", "nhwc", 1)),
    ("<2> 36+1", Conv(1, 6, 11, 4, 32, 3, 1, 1, 1, "nchw", "slice8", 1)),
    ("<3> 72+1", Conv(2, 13, 7, 8, 1, 3, 1, 1, 1, "nhwc", "nhwc", 1)),
    ("<3> 72+1", Conv(1, 13, 9, 8, 5, 3, 2, 1, 1, "slice4", "nhwc", 1)),
    ("<4> 98", Conv(2, 13, 70, 2, 1, 7, 1, 3, 1, "nhwc", "nhwc", 0)),
    ("<4> 98+1", Conv(1, 5, 7, 2, 5, 7, 1, 3, 1, "nchw", "nhwc", 1)),
    ("<2> 32+1", Conv(1, 9, 29, 32, 2, 1, 1, 0, 1, "nhwc", "nhwc", 1)),
    ("<1> 32", Conv(1, 9, 29, 32, 2, 1, 1, 0, 1, "slice4", "nhwc", 0)),      # exactly one tile
    ("<4> 127+1", Conv(1, 5, 7, 127, 5, 1, 1, 0, 1, "nhwc", "nhwc", 1)),     # exactly 128 columns
    ("<4> 127+1", Conv(1, 6, 11, 127, 32, 1, 1, 0, 1, "nhwc", "nhwc", 1)),
]


@pytest.mark.parametrize("group,c", WGRAD_MFMA, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_wgrad_small_mfma(group, c):
    """small_wgrad_mfma_kernel at its four tile counts + small_wgrad_fin_kernel:
    from random dw / dbias, before + oracle; the same bits run to run."""
    _wgrad(c, "wgrad small_wgrad_mfma" + group, twice=True)


def test_wgrad_no_dbias_same_dw():
    """27 columns with and without the bias column take the same single tile:
    dw is the same bits, and no bias buffer is written."""
    c = Conv(2, 24, 24, 3, 32, 3, 1, 1, 1, "nchw", "nhwc", 1)
    rc, dw, _, _ = _wgrad_call(c)
    rc0, dw0, db0, spare = _wgrad_call(c._replace(bias=0))
    assert rc == 0 and rc0 == 0
    _eq(dw0, dw, "dw with dbias = NULL")
    _eq(db0, _in(c)["db0"], "dbias buffer of a dbias = NULL call")
    assert _is_sent(spare)


WGRAD_RELU = [
    ("<4> 98+1", Conv(2, 13, 70, 2, 1, 7, 1, 3, 1, "nhwc", "nhwc", 1)),     # the plain call goes to sa_wgrad_kernel
    ("<1> 27+1", Conv(2, 13, 7, 3, 32, 3, 1, 1, 1, "nchw", "nhwc", 1)),
    ("<1> 27", Conv(1, 5, 7, 3, 5, 3, 1, 1, 1, "nchw", "slice4", 0)),
    ("<2> 32+1", Conv(3, 5, 17, 32, 3, 1, 1, 0, 1, "nhwc", "nhwc", 1)),     # the plain call goes to pw_wgrad_kernel
]


@pytest.mark.parametrize("group,c", WGRAD_RELU, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_wgrad_relu(group, c):
    """upr_t_conv_direct_wgrad_relu: dy counts where y > 0; y holds positive
    and negative values, 0.0, -0.0 and NaN."""
    _wgrad(c, "wgrad_relu small_wgrad_mfma" + group, mask=_mask_of(c), twice=True)


def test_wgrad_relu_unsupported():
    """Cout = 33, and more than 128 columns, have no masked form:
    UPR_ERR_UNSUPPORTED, dw and dbias untouched."""
    L, _, _ = _lib()
    for c in (Conv(1, 5, 7, 3, 33, 3, 1, 1, 1, "nchw", "nhwc", 1), Conv(1, 5, 7, 16, 4, 3, 1, 1, 1, "nhwc", "nhwc", 1)):
        rc, dw, db, _ = _wgrad_call(c, _mask_of(c))
        assert rc == L.UPR_ERR_UNSUPPORTED
        _eq(dw, _in(c)["dw0"], "refused: dw")
        _eq(db, _in(c)["db0"], "refused: dbias")


SA_SHAPES = [(1, 5, 9), (2, 13, 70), (1, 8, 64), (1, 16, 128)]


@pytest.mark.parametrize("B,H,W", SA_SHAPES)
def test_wgrad_sa_tiled(B, H, W):
    """sa_wgrad_kernel (dbias given) and, with dbias NULL, the MFMA form on
    the same operands: both within the bound of the same oracle dw."""
    c = Conv(B, H, W, 2, 1, 7, 1, 3, 1, "nhwc", "nhwc", 1)
    _wgrad(c, "wgrad sa_wgrad (tiled 7x7)", twice=True)
    _wgrad(c._replace(xl="nchw"), "wgrad sa_wgrad (tiled 7x7)")
    _wgrad(c._replace(bias=0), "wgrad small_wgrad_mfma<4> 98 (7x7, no dbias)", twice=True)


PW_SHAPES = [(3, 5, 17), (1, 4, 300), (2, 2, 40)]


@pytest.mark.parametrize("Cout", [1, 3])
@pytest.mark.parametrize("B,H,W", PW_SHAPES)
def test_wgrad_pw(B, H, W, Cout):
    """pw_wgrad_kernel<32, Cout> on aligned x (contiguous and a slice; with
    and without dbias); off1 x runs the MFMA form: the same bound."""
    c = Conv(B, H, W, 32, Cout, 1, 1, 0, 1, "nhwc", "nhwc", 1)
    _wgrad(c, f"wgrad pw_wgrad<32,{Cout}>", twice=True)
    _wgrad(c._replace(xl="slice4", yl="slice4", bias=0), f"wgrad pw_wgrad<32,{Cout}>")
    _wgrad(c._replace(xl="off1"), "wgrad small_wgrad_mfma<2> 32+1 (1x1, off1 x)", twice=True)


WGRAD_GENERIC = [
    Conv(1, 20, 24, 3, 64, 3, 1, 1, 1, "nchw", "nhwc", 1),
    Conv(1, 260, 260, 3, 64, 3, 1, 1, 1, "nchw", "nhwc", 1),    # 1057 chunks on 1024 blocks
    Conv(2, 13, 7, 16, 4, 3, 1, 1, 1, "nhwc", "slice4", 1),      # 145 columns
    Conv(1, 13, 9, 16, 4, 3, 2, 1, 1, "slice4", "nhwc", 0),
    Conv(1, 6, 11, 128, 5, 1, 1, 0, 1, "nhwc", "nhwc", 1),       # 129 columns
]


@pytest.mark.parametrize("c", WGRAD_GENERIC, ids=lambda c: "-".join(map(str, c)))
def test_wgrad_generic(c):
    """conv_direct_wgrad_kernel: LDS chunks of 64 pixels, one partial row a
    block, added in block order: the same bits run to run."""
    _wgrad(c, "wgrad conv_direct_wgrad (generic)", twice=True)


def test_wgrad_generic_too_large():
    """More than 4096 entries: UPR_ERR_UNSUPPORTED, nothing written."""
    L, _, _ = _lib()
    c = Conv(1, 5, 7, 16, 64, 3, 1, 1, 1, "nhwc", "nhwc", 1)
    rc, dw, db, _ = _wgrad_call(c)
    assert rc == L.UPR_ERR_UNSUPPORTED
    _eq(dw, _in(c)["dw0"], "refused: dw")
    _eq(db, _in(c)["db0"], "refused: dbias")


# ---------------------------------------------------------------------------
# refusals of the four direct-conv entries
# ---------------------------------------------------------------------------
def _null_data(view):
    from upr._lib import UprView
    return ctypes.byref(UprView(None, view.v.sb, view.v.sh, view.v.sw, view.v.sc))


BAD_GEOMETRY = [dict(B=0), dict(Cin=0), dict(Cout=0), dict(s=0), dict(d=0), dict(H=0), dict(W=0), dict(kh=0),
                dict(kw=0), dict(p=-1)]


def test_refusals_fwd():
    L, lib, st = _lib()
    c = Conv(2, 13, 7, 3, 32, 3, 1, 1, 1, "nchw", "nhwc", 1)
    d = _in(c)
    Ho, Wo = _osz(c)
    xv, yv, w, b = View(d["x"], c.xl), _sent_view((c.B, Ho, Wo, c.Cout)), d["w"].to(DEV), d["bias"].to(DEV)
    good = dict(x=xv.ref, B=c.B, H=c.H, W=c.W, Cin=c.Cin, w=P(w), bias=P(b), Cout=c.Cout, kh=3, kw=3, s=1, p=1, d=1,
                y=yv.ref, Ho=Ho, Wo=Wo, relu=0, acc=0)
    bad = [dict(x=None), dict(y=None), dict(w=None), dict(x=_null_data(xv)), dict(y=_null_data(yv))] + BAD_GEOMETRY
    for over in bad + [dict(Ho=Ho + 1), dict(Wo=Wo - 1)]:
        want = L.UPR_ERR_SHAPE if ("Ho" in over or "Wo" in over) else L.UPR_ERR_ARG
        a = dict(good, **over)
        assert lib.upr_t_conv_direct(*a.values(), st) == want, over
        y16 = torch.full((c.B * Ho * Wo, c.Cout), SENT, dtype=torch.float16, device=DEV)
        assert lib.upr_t_conv_direct16(*a.values(), P(y16), 0, st) == want, over
        torch.cuda.synchronize()
        assert _is_sent(yv.buf) and _is_sent(y16), over


def test_refusals_dgrad():
    L, _, _ = _lib()
    c = Conv(2, 13, 7, 3, 32, 3, 1, 1, 1, "nchw", "nhwc", 0)
    Ho, Wo = _osz(c)
    dyv = View(_in(c)["dy"], c.yl)
    dxv = _sent_view((c.B, c.H, c.W, c.Cin))
    bad = [dict(dy=None), dict(dx=None), dict(w=None), dict(dy=_null_data(dyv)), dict(dx=_null_data(dxv))]
    for over in bad + BAD_GEOMETRY + [dict(Ho=Ho + 1), dict(Wo=Wo - 1), dict(Ho=c.H - 2, Wo=c.W - 2)]:
        want = L.UPR_ERR_SHAPE if ("Ho" in over or "Wo" in over) else L.UPR_ERR_ARG
        rc, dx = _dgrad_call(c, **over)
        assert rc == want, (over, rc)
        assert _is_sent(dx.buf), over


@pytest.mark.parametrize("masked", [0, 1])
def test_refusals_wgrad(masked):
    L, _, _ = _lib()
    c = Conv(2, 13, 7, 3, 32, 3, 1, 1, 1, "nchw", "nhwc", 1)
    d = _in(c)
    Ho, Wo = _osz(c)
    mask = _mask_of(c) if masked else None
    xv, dyv = View(d["x"], c.xl), View(d["dy"], c.yl)
    bad = [dict(x=None), dict(dy=None), dict(dw=None), dict(x=_null_data(xv)), dict(dy=_null_data(dyv))]
    if masked:
        bad += [dict(y=None), dict(y=_null_data(dyv))]
    for over in bad + BAD_GEOMETRY + [dict(Ho=Ho + 1), dict(Wo=Wo - 1)]:
        want = L.UPR_ERR_SHAPE if ("Ho" in over or "Wo" in over) else L.UPR_ERR_ARG
        rc, dw, db, _ = _wgrad_call(c, mask, **over)
        assert rc == want, (over, rc)
        _eq(dw, d["dw0"], f"refused {over}: dw")
        _eq(db, d["db0"], f"refused {over}: dbias")


# ---------------------------------------------------------------------------
# helpers: bit-exact against the oracle's index restatements
# ---------------------------------------------------------------------------
PACK_SHAPES = [(64, 32, 3), (3, 32, 1), (1, 2, 7), (32, 64, 2)]


def _pack_w(Co, Ci, k, mode):
    """A weight in the layout the mode reads: [Co][Ci][k][k], or the ConvTranspose [Ci][Co][2][2]."""
    shape = (Co, Ci, k, k) if mode < 2 else (Ci, Co, k, k)
    return torch.randn(shape, generator=_gen("pack", Co, Ci, k, mode))


@pytest.mark.parametrize("Co,Ci,k", PACK_SHAPES)
def test_pack_weight_unpack_grad(Co, Ci, k):
    """upr_t_pack_weight modes 0-3 against the index restatement (modes 2 / 3
    off k = 2: UPR_ERR_SHAPE); upr_t_unpack_grad inverts modes 0 and 3, adds
    with accumulate, and refuses the other modes."""
    L, lib, st = _lib()
    for mode in range(4):
        w = _pack_w(Co, Ci, k, mode)
        out = torch.full((w.numel(),), SENT, device=DEV)
        rc = lib.upr_t_pack_weight(P(w.to(DEV)), P(out), Co, Ci, k, k, mode, st)
        torch.cuda.synchronize()
        if mode >= 2 and k != 2:
            assert rc == L.UPR_ERR_SHAPE and _is_sent(out)
            continue
        assert rc == 0
        _eq(out, torch.from_numpy(np.ascontiguousarray(O.pack_weight(w.numpy(), mode))), f"pack mode {mode}")
        g0 = torch.randn(w.shape, generator=_gen("g0", Co, Ci, k))
        for acc in (0, 1):
            g = g0.to(DEV)
            rc = lib.upr_t_unpack_grad(P(out), P(g), Co, Ci, k, k, mode, acc, st)
            torch.cuda.synchronize()
            if mode in (1, 2):
                assert rc == L.UPR_ERR_ARG
                _eq(g, g0, "refused unpack")
                continue
            assert rc == 0
            back = torch.from_numpy(np.ascontiguousarray(O.unpack_grad(out.cpu().numpy(), Co, Ci, k, k, mode)))
            _eq(back, w, "oracle round trip")
            _eq(g, g0 + w if acc else w, f"unpack mode {mode} accumulate {acc}")


@pytest.mark.parametrize("which", ["both", "out32", "out16"])
def test_pack_weights_batch(which):
    """upr_t_pack_weights: one launch with a job of every mode 0-4 and
    differing n; max_n = 18432 > 64 * 256, so gridDim.x is capped and the
    stride loop runs.  fp32 equals upr_t_pack_weight's bits, fp16 is that
    rounded once; a NULL output is skipped."""
    L, lib, st = _lib()
    jobs_spec = [(64, 32, 3, 0), (3, 32, 1, 1), (32, 64, 2, 2), (5, 3, 2, 3), (64, 32, 3, 1), (1, 2, 7, 0)]
    keep, Jobs = [], (L.UprPackJob * (len(jobs_spec) + 1))()
    for i, (Co, Ci, k, mode) in enumerate(jobs_spec):
        w = _pack_w(Co, Ci, k, mode)
        wd = w.to(DEV)
        o32 = torch.full((w.numel(),), SENT, device=DEV)
        o16 = torch.full((w.numel(),), SENT, dtype=torch.float16, device=DEV)
        single = torch.full((w.numel(),), SENT, device=DEV)
        assert lib.upr_t_pack_weight(P(wd), P(single), Co, Ci, k, k, mode, st) == 0
        keep.append((w, wd, o32, o16, single, mode))
        Jobs[i] = L.UprPackJob(P(wd), P(o32) if which != "out16" else None, P(o16) if which != "out32" else None, Co,
                               Ci, k, k, mode, w.numel())
    bias = torch.randn(64, generator=_gen("packbias"))
    bd = bias.to(DEV)
    b32, b16 = torch.full((256,), SENT, device=DEV), torch.full((256,), SENT, dtype=torch.float16, device=DEV)
    Jobs[len(jobs_spec)] = L.UprPackJob(P(bd), P(b32) if which != "out16" else None,
                                        P(b16) if which != "out32" else None, 64, 0, 0, 0, 4, 64)
    raw = torch.frombuffer(bytearray(bytes(Jobs)), dtype=torch.uint8).to(DEV)
    max_n = max(t[0].numel() for t in keep)
    assert max_n > 64 * 256
    assert lib.upr_t_pack_weights(P(raw), 0, max_n, st) == 0 and lib.upr_t_pack_weights(P(raw), len(Jobs), 0, st) == 0
    torch.cuda.synchronize()
    assert all(_is_sent(t[2]) and _is_sent(t[3]) for t in keep), "njobs = 0 / max_n = 0 wrote"
    assert lib.upr_t_pack_weights(P(raw), len(Jobs), max_n, st) == 0
    torch.cuda.synchronize()
    for w, _, o32, o16, single, mode in keep:
        _eq(single, torch.from_numpy(np.ascontiguousarray(O.pack_weight(w.numpy(), mode))), f"single mode {mode}")
        if which != "out16":
            _eq(o32, single, f"batched mode {mode} fp32")
        else:
            assert _is_sent(o32)
        if which != "out32":
            _eq(o16, single.half(), f"batched mode {mode} fp16")
        else:
            assert _is_sent(o16)
    rep = torch.from_numpy(O.pack_weight(bias.numpy(), 4))
    if which != "out16":
        _eq(b32, rep, "mode 4 fp32")
    if which != "out32":
        _eq(b16, rep.half(), "mode 4 fp16")


def test_zero_upsample():
    """upr_t_zero_upsample / 16 / 16h on dy a channel slice, B = 2, Ho != Wo:
    the even phase is dy, the three odd phases exactly zero; the fp16 forms are
    the fp32 form rounded once; the documented refusals write nothing."""
    L, lib, st = _lib()
    B, Ho, Wo, C = 2, 3, 5, 16
    dy = torch.randn((B, Ho, Wo, C), generator=_gen("zup"))
    for layout in ("nhwc", "slice4", "slice8"):
        v = View(dy, layout)
        cs = v.v.sw
        z = torch.full((B, 2 * Ho, 2 * Wo, C), SENT, device=DEV)
        assert lib.upr_t_zero_upsample(P(v.buf), B, Ho, Wo, C, cs, v.coff, P(z), st) == 0
        want = torch.from_numpy(O.zero_upsample(dy.numpy()))
        _eq(z, want, f"zero_upsample {layout}")
        for ph in ((1, 0), (0, 1), (1, 1)):
            assert not z[:, ph[0]::2, ph[1]::2].any()
        z16 = torch.full(z.shape, SENT, dtype=torch.float16, device=DEV)
        assert lib.upr_t_zero_upsample16(P(v.buf), B, Ho, Wo, C, cs, v.coff, P(z16), st) == 0
        _eq(z16, want.half(), f"zero_upsample16 {layout}")
    d16 = dy.half().to(DEV)
    z16h = torch.full((B, 2 * Ho, 2 * Wo, C), SENT, dtype=torch.float16, device=DEV)
    assert lib.upr_t_zero_upsample16h(P(d16), B, Ho, Wo, C, P(z16h), st) == 0
    _eq(z16h, want.half(), "zero_upsample16h")
    # refusals: C % 8, an unaligned pointer, cs / coff not multiples of 4
    big = torch.full((B * Ho * Wo * 32 + 8,), SENT, device=DEV)
    z16 = torch.full((B * 4 * Ho * Wo * C + 8,), SENT, dtype=torch.float16, device=DEV)
    for a in [(P(big), B, Ho, Wo, 12, 16, 0, P(z16)), (P(big, 1), B, Ho, Wo, C, 16, 0, P(z16)),
              (P(big), B, Ho, Wo, C, 16, 0, P(z16, 1)), (P(big), B, Ho, Wo, C, 18, 0, P(z16)),
              (P(big), B, Ho, Wo, C, 20, 2, P(z16)), (None, B, Ho, Wo, C, 16, 0, P(z16))]:
        assert lib.upr_t_zero_upsample16(*a, st) == L.UPR_ERR_ARG, a
    h = torch.full((B * Ho * Wo * C + 8,), SENT, dtype=torch.float16, device=DEV)
    for a in [(P(h), B, Ho, Wo, 12, P(z16)), (P(h, 1), B, Ho, Wo, C, P(z16)), (P(h), B, Ho, Wo, C, P(z16, 1)),
              (P(h), B, Ho, Wo, C, None)]:
        assert lib.upr_t_zero_upsample16h(*a, st) == L.UPR_ERR_ARG, a
    torch.cuda.synchronize()
    assert _is_sent(z16)


@pytest.mark.parametrize("n", [1, 255, 4097])
def test_cast_f16(n):
    """upr_t_cast_f16 against x.half(): subnormal results, ties to even,
    overflow to +-inf, +-0 and NaN among random values."""
    _, lib, st = _lib()
    x = torch.randn(n, generator=_gen("cast", n)) * 100
    special = torch.tensor([float("nan"), 0.0, -0.0, 65504.0, 65519.9, 65520.0, -65520.0, 1e6, -1e6, 2.0 ** -24,
                            2.0 ** -25, 2.0 ** -25 * 1.0001, 3 * 2.0 ** -25, 6e-6, -6.1e-5, 1.0 + 2.0 ** -11,
                            1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 2049.0, 2051.0, 1e-9])
    k = min(n, special.numel())
    x[n - k:] = special[:k]
    y = torch.full((n,), SENT, dtype=torch.float16, device=DEV)
    assert lib.upr_t_cast_f16(P(x.to(DEV)), P(y), n, st) == 0
    want = x.half()
    got = y.cpu()
    assert torch.equal(got.view(torch.int16)[~want.isnan()], want.view(torch.int16)[~want.isnan()])
    assert torch.equal(got.isnan(), want.isnan())


def conv_configs():
    """Every (Cin, Cout, k, stride, pad, dil) of this file's conv cases (the
    grid tests/test_cpu_conv_ops_oracle.py holds the oracle to)."""
    cs = [Conv(1, 1, 1, 3, co, 3, 1, t[3], 1) for t in FWD_MFMA for co in (32, 64)]
    cs += [Conv(1, 1, 1, 3, t[3], 3, 1, t[4], 1) for t in FWD_C3K3]
    cs += [Conv(1, 1, 1, ci, co, 1) for ci in (16, 32, 64) for co in (1, 2, 3, 4)]
    cs += FWD_SMALL + FWD_GENERIC + [c for _, c in DGRAD + WGRAD_MFMA + WGRAD_RELU] + WGRAD_GENERIC
    cs += [Conv(1, 1, 1, 2, 1, 7, 1, 3, 1), Conv(1, 1, 1, 32, 1, 1), Conv(1, 1, 1, 32, 3, 1),
           Conv(1, 1, 1, 3, 33, 3, 1, 1, 1), Conv(1, 1, 1, 16, 64, 3, 1, 1, 1)]
    return sorted({(c.Cin, c.Cout, c.k, c.s, c.p, c.d) for c in cs})
