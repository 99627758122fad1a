"""Op-level parity of the MFMA-path weight gradients (csrc/train_wgrad.hip and
the per-tap kernel of csrc/train_conv.hip) against the float64 reference
oracle.conv_ops.conv_wgrad (run with `-m gpu`).  The three entries
upr_t_conv_wgrad, upr_t_conv_wgrad16 and upr_t_conv_wgrad_into are called
through ctypes on operands made on the CPU with a fixed seed, one op a call;
dw / dwp starts random (the contract is +=).  Channel slices live in
sentinel-filled wider buffers (wgrad_cases.LAYOUTS), the packed dwp and the
torch-layout dw of _wgrad_into sit inside a flat buffer with sentinel floats
before and after (dw one float in, so off 16-byte alignment), and every
operand buffer is compared bit for bit with its host copy after the call.
Every case first asserts that upr_t_conv_wgrad_ran names the kernel, tile,
split count and dy operand of its table row (tests/wgrad_cases.py; the split
counts come from the restated launcher arithmetic, checked on the CPU by
tests/test_cpu_wgrad_cases.py).

Shapes: which kernel and branch each case reaches ((B, H, W, Cin, Cout, k, s,
p, d); the notes of wgrad_cases.py say the same per row).

  fp32 split-K GEMM, wgrad_gemm_kernel<BM, BN>                        GEMM32_ROWS
    <32,256> Cout 32 / 96, <64,128> Cout 64, <128,64> Cout 128 / 256; through
    upr_t_conv_wgrad and upr_t_conv_wgrad_into (x16 NULL), bit-equal
      (1,3,5,32,32,1,1,0,1)       P 15: less than one 32-pixel step; KT 32 of a 256-wide tile
      (1,5,7,32,32,3,1,1,1)       P 35: one split, the second step has 3 pixels ("pixels past
                                  the range read a zero line"); KT 288: 32 valid columns in n-tile 2
      (2,5,7,32,64,3,1,1,1)       P 70: the image boundary inside a step; 3 n-tiles, the last partial
      (2,9,11,64,128,3,2,1,1)     stride 2 at odd H, W (5 x 6 out); nine full n-tiles of 64
      (1,13,21,32,32,3,1,2,2)     dilation 2; P 273: splits of 96, 96, 81 (a last step of 17)
      (1,12,12,32,32,3,1,0,1)     pad 0
      (2,8,8,32,96,1,2,0,1)       the projecting shortcut; three m-tiles
      (1,6,10,256,256,3,1,1,1)    two m-tiles by 36 n-tiles
      (1,8,12,32,64,2,2,0,1)      the ConvTranspose form (k 2, s 2)
      (1,4,16,128,32,1,1,0,1), (1,4,16,96,32,1,1,0,1)   the fusion convs: one partial n-tile
      (1,240,256,256,256,3,1,1,1) 15 splits of 4096 pixels, the longest chain of the bs 8
                                  512^2 step; 35 MB of slabs
    x and dy as slice4 / slice8 of wider buffers on the second, fourth and fifth
  fp32 per-tap kernel, conv_wgrad_kernel (fp32 atomics)                 TAP32_ROWS
    x off1, dy off1 (also through _wgrad_into: scratch + upr_t_unpack_grad), dwp off1
      the second and fourth GEMM shapes; (1,32,32,..) P 1024: one block, the
      bits repeat; (1,25,41,..) P 1025: a second block of one pixel, bound only
  fp16 im2col, wgrad16_kernel<BM, NR> (Wo % 64 == 0)                 IM2COL16_ROWS
    upr_t_conv_wgrad16 with x16, and with x16 NULL (the cast; x contiguous and
    slice8x), upr_t_conv_wgrad_into with x16 (x given and NULL) and dy / dy16;
    all bit-equal.  <32,9> 3 units one split / declined by the halo form (H 12,
    H 3, dilation 3, pad 0 with Ho != H) / 27 runs in three n-tiles; <64,9> 10
    units in splits of 4, 4, 2 with the image boundary inside one, and two
    n-tiles; <128,2> stride 2; <32,8>, <128,4>, <128,1>, <64,1>, <64,2> the
    1x1 forms; <64,4> the ConvTranspose form.  dy (and dy16) slice4 / slice8
    on (2,5,64,32,64,..) and (2,8,64,64,64,..).
  fp16 halo, wgrad16h_kernel<CIN, 32, NTAP, RPW, D, A16>                HALO16_ROWS
    <32,9,1> TR 8: (1,8,64) one step, every halo zero; (1,8,128) a halo column
    is the neighbour segment's pixel; (2,24,128) row blocks of 2 and 1 steps,
    two images.  <32,9,2> TR 4: (1,4,64), (2,12,128).  <96,1,0>, <128,1,0>:
    (1,4,64), (2,12,128).  Each reading dy and reading dy16 (two kernels,
    bit-equal); dy slice4 / slice8 on the two (2,..,128) 3x3 shapes.
  routing: (1,8,24,32,32,3,1,1,1) through the fp16 entries runs the fp32 GEMM
    on the unrounded x (x NULL: UPR_ERR_ARG); upr_t_conv_wgrad16's cast takes
    x only at x_cs % 8 == 0, so op_parity's slice8 (12 wider) runs the fp32
    GEMM too; a dy16 off 8-byte alignment is ignored; every argument check
    returns its code with dw untouched and the query reporting no kernel.

Tolerances (tests/op_parity.py _within_restated, as test_gpu_conv_ops.py): the
kernel's error against float64 within 4x the error of plain fp32 torch on the
CPU (torch.nn.grad.conv2d_weight on the operands the kernel is specified to
use: x16 and (half)dy for the fp16 forms), at least half an ulp of the largest
|reference|, and under 1e-4 * max|ref| + 1e-6; per tensor and per output
channel.  Every form built without atomics: the same bits from a second call.

Measured on the MI355X: max |error| against float64 in ulp of the case's
largest |reference|, the worst case of each group; "used" is the worst kernel
error / allowed error over all cases (1 would fail).  The slowest tests are
the two long chains, CPU references and operand copies included: im2col 1.4 s
(243 MB of fp32 operands), fp32 GEMM 0.8 s (126 MB); every other takes under
0.2 s; the file 5.0 s (profiles/wgrad_ops_gpu_tests_v1.log).

  group (calls)                                   restatement   kernel   used
  wgrad_gemm<32,256> (46)                              5.37       2.66   0.31
  wgrad_gemm<32,256> per channel (46)                  5.37       2.66   0.63
  wgrad_gemm<64,128> (4)                               2.00       2.69   0.38
  wgrad_gemm<64,128> per channel (4)                   2.00       2.69   0.72
  wgrad_gemm<128,64> (22)                             22.00       9.24   0.18
  wgrad_gemm<128,64> per channel (22)                 22.00       9.24   0.37
  conv_wgrad per tap (12)                              5.00       6.70   0.51
  conv_wgrad per tap per channel (12)                  5.00       6.70   0.83
  conv_wgrad per tap, scratch + unpack (8)             5.00       7.70   0.58
  conv_wgrad per tap, scratch + unpack per channel (8)  5.00      7.70   0.83
  wgrad16<32,9> (30)                                   7.68       3.37   0.25
  wgrad16<32,9> per channel (30)                       7.68       3.37   0.38
  wgrad16<64,9> (24)                                   2.30       2.21   0.28
  wgrad16<64,9> per channel (24)                       2.30       2.21   0.52
  wgrad16<128,2> (6)                                   8.56       2.63   0.08
  wgrad16<128,2> per channel (6)                       8.56       2.63   0.21
  wgrad16<32,8> (6)                                    1.69       1.48   0.22
  wgrad16<32,8> per channel (6)                        1.69       1.48   0.38
  wgrad16<128,4> (6)                                   4.90       1.72   0.09
  wgrad16<128,4> per channel (6)                       4.90       1.72   0.21
  wgrad16<128,1> (6)                                   4.12       1.87   0.11
  wgrad16<128,1> per channel (6)                       4.12       1.87   0.28
  wgrad16<64,1> (6)                                    3.45       1.53   0.11
  wgrad16<64,1> per channel (6)                        3.45       1.53   0.25
  wgrad16<64,2> (6)                                    4.08       1.74   0.11
  wgrad16<64,2> per channel (6)                        4.08       1.74   0.24
  wgrad16<64,4> (6)                                    4.92       1.52   0.08
  wgrad16<64,4> per channel (6)                        4.92       1.52   0.23
  wgrad16<128,4> long chain (1)                       32.59       6.09   0.05
  wgrad16<128,4> long chain per channel (1)           32.59       6.09   0.08
  wgrad16h<32,9,1> dy (11) / dy16 (5)                  4.06       1.88   0.13
  wgrad16h<32,9,1> per channel                         4.06       1.88   0.23
  wgrad16h<32,9,2> dy (8) / dy16 (4)                  14.56       1.78   0.10
  wgrad16h<32,9,2> per channel                        14.56       1.78   0.15
  wgrad16h<96,1,0> dy (6) / dy16 (2)                   7.11       1.44   0.06
  wgrad16h<96,1,0> per channel                         7.11       1.44   0.13
  wgrad16h<128,1,0> dy (6) / dy16 (2)                 10.50       1.81   0.08
  wgrad16h<128,1,0> per channel                       10.50       1.81   0.11

  torch.equal groups (run to run; packed against torch layout; slices against
  contiguous; the cast against x16; dy against dy16; a misaligned dy16; refused
  calls; sentinels and operand buffers): no difference.  The per-tap kernel's
  two blocks at P 1025 give 6.70 or 7.70 ulp by the order of their atomics;
  both orders are at 0.83 of the bound.

One case missed the bound as first written: wgrad_gemm_kernel<64,128> at
(2,5,7,32,64,3,1,1,1), per channel 4.52 ulp against the restatement's 1.79
(1.195x the allowed error; (2,8,8,32,96,1,2,0,1) was at 0.93).  A split's
pixels were added in one chain, a rounding a pixel (restated on the CPU: the
same 4.52 ulp).  The kernel now keeps two accumulators a tile, which take the
pixel pairs of a step in turn and are added once at the end: 2.69 ulp, 0.72
of the bound, and the 4096-pixel chain went from 13.21 to 9.24 ulp.  bench.py
--train in alternating runs against the parent build: 70.0-70.1 against
71.1-71.4 ms a step in fp32, 21.24-21.26 against 21.27-21.32 ms with --amp
(profiles/wgrad_gemm_two_chains_bench.txt).

The im2col table was drawn up without a long-chain case, on the claim that a
split has at most about 18 units at bs 8 512^2.  The restated launcher says 64
units where the shape has two n-tiles (64 -> 64, 64 -> 32) and 32 with one:
128 MFMA accumulations an accumulator (tests/test_cpu_wgrad_cases.py pins the
figures).  test_im2col16_long_chain runs that length at the cheapest shape
that reaches it, (1,29,4096,256,256,3,1,1,1): 29 splits of 64 units.
"""
import collections
import ctypes

import numpy as np
import pytest
import torch

import wgrad_cases as C
from conftest import has_gpu
from op_parity import DEV, P, SENT, _within_restated

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]


def _lib():
    from upr import _lib as L
    return L, L.lib(), torch.cuda.current_stream().cuda_stream


def _ran():
    """(kernel, t0, t1, t2, splits, dy16) of the calling thread's latest weight-gradient call."""
    L, lib, _ = _lib()
    r = L.UprWgradRan()
    assert lib.upr_t_conv_wgrad_ran(ctypes.byref(r)) == 0
    return (r.kernel, r.t0, r.t1, r.t2, r.splits, r.dy16)


def _wide(t, layout):
    """t [M, C] as the channel slice of a sentinel-filled [M, C + extra] buffer:
    (host copy, device buffer, channel stride, channel offset)."""
    extra, coff = C.LAYOUTS[layout]
    M, Ch = t.shape
    host = torch.full((M, Ch + extra), SENT, dtype=t.dtype)
    host[:, coff:coff + Ch] = t
    return host, host.to(DEV), Ch + extra, coff


def _ids(v):
    return "-".join(map(str, v.case)) if isinstance(v, C.Row) else str(v)


Out = collections.namedtuple("Out", "rc dw ran")
PAD = 4  # sentinel floats in front of a packed dwp (keeps it 16-byte aligned)


def _call(c, entry, xl="contig", dyl="contig", x16=False, dy16=False, x_null=False, dwp_shift=0, dy16_decoy=False,
          **over):
    """One call of `entry` ("wgrad", "wgrad16", "into") from the random dw0.
    x16: pass (half)x compact; dy16: pass (half)dy in dy's layout (dy16_decoy:
    a buffer of zeros one fp16 past 8-byte alignment instead); x_null: x = NULL;
    dwp_shift: the packed dwp that many floats past alignment; over: arguments
    replaced by name.  Returns Out(rc, dw [Cout, Cin, k, k] on the CPU, the
    query's answer) after checking every sentinel and operand buffer."""
    _, lib, st = _lib()
    d = C.operands(c)
    Ho, Wo = C.out_hw(c)
    n = c.Cout * c.Cin * c.k * c.k
    xh, xb, x_cs, x_coff = _wide(d["x"].reshape(-1, c.Cin), xl)
    dyh, dyb, dy_cs, dy_coff = _wide(d["dy"].reshape(-1, c.Cout), dyl)
    x16h = d["x"].half()
    x16b = x16h.to(DEV) if x16 else None
    if dy16_decoy:
        d16h = torch.zeros(dyh.numel() + 4, dtype=torch.float16)
        d16b = d16h.to(DEV)
        dy16p = P(d16b, 1)
    elif dy16:
        d16h, d16b, _, _ = _wide(d["dy"].half().reshape(-1, c.Cout), dyl)
        dy16p = P(d16b)
    else:
        d16h = d16b = dy16p = None
    packed = entry != "into"
    lead = PAD + dwp_shift if packed else 1
    start = d["dw0"].permute(0, 2, 3, 1).reshape(-1) if packed else d["dw0"].reshape(-1)
    flat_h = torch.full((lead + n + PAD,), SENT)
    flat_h[lead:lead + n] = start
    flat = flat_h.to(DEV)
    a = dict(x=None if x_null else P(xb), x16=P(x16b), B=c.B, H=c.H, W=c.W, Cin=c.Cin, x_cs=x_cs, x_coff=x_coff,
             dy=P(dyb), dy16=dy16p, Ho=Ho, Wo=Wo, Cout=c.Cout, dy_cs=dy_cs, dy_coff=dy_coff, kh=c.k, kw=c.k, s=c.s,
             p=c.p, d=c.d, dw=P(flat, lead))
    assert set(over) <= set(a), over
    a.update(over)
    if entry != "into":
        del a["dy16"]
    if entry == "wgrad":
        del a["x16"]
    fn = {"wgrad": lib.upr_t_conv_wgrad, "wgrad16": lib.upr_t_conv_wgrad16, "into": lib.upr_t_conv_wgrad_into}[entry]
    rc = fn(*a.values(), st)
    ran = _ran()
    torch.cuda.synchronize()
    got = flat.cpu()
    what = f"{entry} {tuple(c)} x {xl} dy {dyl}"
    assert torch.equal(got[:lead], flat_h[:lead]) and torch.equal(got[lead + n:], flat_h[lead + n:]), \
        f"{what}: wrote outside dw"
    assert torch.equal(xb.cpu(), xh) and torch.equal(dyb.cpu(), dyh), f"{what}: an operand buffer changed"
    if x16b is not None:
        assert torch.equal(x16b.cpu(), x16h), f"{what}: x16 changed"
    if d16b is not None:
        assert torch.equal(d16b.cpu(), d16h), f"{what}: dy16 changed"
    dw = got[lead:lead + n]
    dw = dw.view(c.Cout, c.k, c.k, c.Cin).permute(0, 3, 1, 2).contiguous() if packed else dw.view(c.Cout, c.Cin, c.k, c.k)
    return Out(rc, dw, ran)


def _bound(c, dw, fp16, tag):
    ref, rst = C.references(c, fp16)
    _within_restated(tag + " dw", dw, ref, rst)
    _within_restated(tag + " dw per channel", C.as_kc(dw, c.Cout), C.as_kc(ref, c.Cout), C.as_kc(rst, c.Cout),
                     per_channel=True)


def _run(row, entry, group, fp16, dy16=False, twice=True, family=None, **kw):
    """A call that must succeed on the kernel of its row: the route, the bound,
    and (forms without atomics) the same bits from a second call."""
    c = row.case
    want = C.route(row, family) + (int(dy16),)
    o = _call(c, entry, dy16=dy16, **kw)
    tag = f"{group} | {tuple(c)} | {entry} " + " ".join(f"{k}={v}" for k, v in kw.items())
    assert o.rc == 0, (tag, o.rc)
    assert o.ran == want, (tag, o.ran, want)
    _bound(c, o.dw, fp16, tag)
    if twice:
        o2 = _call(c, entry, dy16=dy16, **kw)
        assert o2.rc == 0 and o2.ran == want
        assert torch.equal(o2.dw, o.dw), f"{tag}: not the same bits run to run"
    return o


def _name(row):
    t = row.tile
    return {C.GEMM32: f"wgrad_gemm<{t[0]},{t[1]}>", C.TAP32: "conv_wgrad per tap", C.IM2COL16: f"wgrad16<{t[0]},{t[1]}>",
            C.HALO16: f"wgrad16h<{t[0]},{t[1]},{t[2]}>"}[row.family]


# ---------------------------------------------------------------------------
# fp32 split-K GEMM
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("row", C.GEMM32_ROWS, ids=_ids)
def test_gemm32(row):
    """wgrad_gemm_kernel through upr_t_conv_wgrad (packed dwp) and through
    upr_t_conv_wgrad_into with x16 NULL (PyTorch's layout, off alignment)."""
    a = _run(row, "wgrad", _name(row), False)
    b = _run(row, "into", _name(row), False)
    assert torch.equal(a.dw, b.dw), "packed and torch-layout results differ"
    if C.GEMM32_ROWS.index(row) in C.GEMM32_LAYOUT_ROWS:
        for xl, dyl in C.GEMM32_LAYOUTS:
            for entry in ("wgrad", "into"):
                o = _run(row, entry, _name(row) + " slices", False, twice=False, xl=xl, dyl=dyl)
                assert torch.equal(o.dw, a.dw), f"x {xl} dy {dyl}: a slice changes the bits"


# ---------------------------------------------------------------------------
# fp32 per-tap kernel (atomics)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("way", C.TAP32_WAYS)
@pytest.mark.parametrize("row", C.TAP32_ROWS, ids=_ids)
def test_tap32(row, way):
    """conv_wgrad_kernel, reached by x or dy one float past alignment or by a
    packed dwp one float past it.  One pixel block: every weight gets a single
    atomic add, so the bits repeat; two blocks: the bound only."""
    one_block = C.tap32_plan(row.case)["splits"] == 1
    kw = {"x_off1": dict(xl="off1"), "dy_off1": dict(dyl="off1"), "dwp_off1": dict(dwp_shift=1)}[way]
    _run(row, "wgrad", _name(row) + " " + way, False, twice=one_block, **kw)
    if way != "dwp_off1":
        # upr_t_conv_wgrad_into: the GEMM declines the operand, so the packed form goes to scratch and
        # upr_t_unpack_grad adds it to dw; the query names the inner call's kernel
        _run(row, "into", _name(row) + " scratch + unpack " + way, False, twice=one_block, **kw)


# ---------------------------------------------------------------------------
# fp16 im2col
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("row", C.IM2COL16_ROWS, ids=_ids)
def test_im2col16(row):
    """wgrad16_kernel<BM, NR> through upr_t_conv_wgrad16 (x16 given; x16 NULL:
    the internal cast of a contiguous x and of a slice) and through
    upr_t_conv_wgrad_into with x16 and with / without dy16."""
    g = _name(row)
    a = _run(row, "wgrad16", g, True, x16=True)
    for xl in ("contig", "slice8x"):
        o = _run(row, "wgrad16", g + " cast", True, twice=False, xl=xl)
        assert torch.equal(o.dw, a.dw), f"x {xl}: the internal cast changes the bits"
    b = _run(row, "into", g, True, x16=True)
    b16 = _run(row, "into", g + " dy16", True, dy16=True, x16=True)
    assert torch.equal(a.dw, b.dw) and torch.equal(b.dw, b16.dw), "dwp / dw / dy16 forms differ"
    o = _run(row, "into", g + " x NULL", True, dy16=True, twice=False, x16=True, x_null=True)
    assert torch.equal(o.dw, b.dw)
    if C.IM2COL16_ROWS.index(row) in C.IM2COL16_LAYOUT_ROWS:
        for dyl in ("slice4", "slice8"):
            for entry, dy16 in (("wgrad16", False), ("into", False), ("into", True)):
                o = _run(row, entry, g + " dy slice" + (" dy16" if dy16 else ""), True, dy16=dy16, twice=False,
                         x16=True, dyl=dyl)
                assert torch.equal(o.dw, a.dw), f"dy {dyl} dy16 {dy16}: a slice changes the bits"


def test_im2col16_long_chain():
    """29 splits of 64 units: the chain length the 64-channel convs of the bs 8
    512^2 step reach (the table's own cases stop at 4 units a split)."""
    row = C.IM2COL16_LONG
    _run(row, "wgrad16", _name(row) + " long chain", True, x16=True)


# ---------------------------------------------------------------------------
# fp16 halo
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dy16", [False, True], ids=["dy", "dy16"])
@pytest.mark.parametrize("row", C.HALO16_ROWS, ids=_ids)
def test_halo16(row, dy16):
    """wgrad16h_kernel<CIN, 32, NTAP, RPW, D, A16>: reading fp32 dy and reading
    its fp16 copy are two kernels."""
    g = _name(row) + (" dy16" if dy16 else " dy")
    a = _run(row, "into", g, True, dy16=dy16, x16=True)
    if not dy16:
        b = _run(row, "wgrad16", g, True, x16=True)
        assert torch.equal(a.dw, b.dw), "dwp and dw forms differ"
        o = _run(row, "wgrad16", g + " cast", True, twice=False)
        assert torch.equal(o.dw, a.dw), "the internal cast changes the bits"
    if C.HALO16_ROWS.index(row) in C.HALO16_LAYOUT_ROWS:
        for dyl in ("slice4", "slice8"):
            o = _run(row, "into", g + " dy slice", True, dy16=dy16, twice=False, x16=True, dyl=dyl)
            assert torch.equal(o.dw, a.dw), f"dy {dyl}: a slice changes the bits"


def test_halo16_dy_and_dy16_agree():
    """The two halo kernels multiply the same fp16 values in the same order."""
    for row in C.HALO16_ROWS:
        a = _call(row.case, "into", x16=True)
        b = _call(row.case, "into", x16=True, dy16=True)
        assert a.rc == 0 and b.rc == 0 and torch.equal(a.dw, b.dw), row.case


# ---------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["wgrad16", "into"])
def test_fp16_entry_off_the_fp16_shapes(entry):
    """Wo = 24: with x16 given the fp32 GEMM runs on the unrounded x and dy;
    with x NULL the call is UPR_ERR_ARG, dw untouched, nothing ran."""
    L, _, _ = _lib()
    row = C.ROUTING_ROW
    dy16 = entry == "into"
    o = _call(row.case, entry, x16=True, dy16=dy16)
    assert o.rc == 0 and o.ran == C.route(row) + (0,), o.ran
    _bound(row.case, o.dw, False, f"{_name(row)} from {entry} with x16 | {tuple(row.case)}")
    plain = _call(row.case, "wgrad" if entry == "wgrad16" else "into")
    assert torch.equal(o.dw, plain.dw), "x16 given changes the fp32 result"
    r = _call(row.case, entry, x16=True, dy16=dy16, x_null=True)
    assert r.rc == L.UPR_ERR_ARG and r.ran == (C.NONE, 0, 0, 0, 0, 0), (r.rc, r.ran)
    assert torch.equal(r.dw, C.operands(row.case)["dw0"]), "a refused call changed dw"


def test_cast_refuses_a_stride_off_8():
    """upr_t_conv_wgrad16 with x16 NULL casts x only at x_cs % 8 == 0 and
    x_coff % 8 == 0: op_parity's slice8 (12 wider) and slice4 run the fp32
    GEMM on the unrounded operands."""
    row = C.IM2COL16_ROWS[0]
    for xl in ("slice8", "slice4"):
        o = _call(row.case, "wgrad16", xl=xl)
        assert o.rc == 0 and o.ran == C.route(row, C.GEMM32) + (0,), (xl, o.ran)
        _bound(row.case, o.dw, False, f"wgrad_gemm<32,256> from wgrad16, x {xl} | {tuple(row.case)}")


def test_misaligned_dy16_is_ignored():
    """A dy16 off 8-byte alignment: dy is read (the query says so) and the
    result is the no-dy16 call's bit for bit, for both fp16 kernels.  The decoy
    holds zeros, so reading it would change the result."""
    for row in (C.IM2COL16_ROWS[2], C.HALO16_ROWS[1]):
        a = _call(row.case, "into", x16=True)
        b = _call(row.case, "into", x16=True, dy16_decoy=True)
        assert a.rc == 0 and b.rc == 0
        assert a.ran == b.ran == C.route(row) + (0,), (a.ran, b.ran)
        assert torch.equal(a.dw, b.dw)


# ---------------------------------------------------------------------------
# refusals: every check returns before anything is queued
# ---------------------------------------------------------------------------
BAD_ARG = [dict(kh=0), dict(kw=0), dict(s=0), dict(d=0), dict(p=-1), dict(H=0), dict(W=0), dict(Ho=0), dict(Wo=0),
           dict(B=0), dict(Cin=0), dict(Cout=0), dict(Cin=31), dict(Cout=48), dict(dy=None), dict(dw=None),
           dict(x_coff=-4), dict(dy_coff=-4)]


@pytest.mark.parametrize("entry", ["wgrad", "wgrad16", "into"])
@pytest.mark.parametrize("row", [C.GEMM32_ROWS[1], C.HALO16_ROWS[0]], ids=_ids)
def test_refusals(row, entry):
    L, _, _ = _lib()
    c = row.case
    Ho, Wo = C.out_hw(c)
    x16 = entry != "wgrad"
    bad = [(o, L.UPR_ERR_ARG) for o in BAD_ARG]
    bad += [(dict(Ho=Ho + 1), L.UPR_ERR_SHAPE), (dict(Wo=Wo - 1), L.UPR_ERR_SHAPE), (dict(p=c.p + 1), L.UPR_ERR_SHAPE),
            (dict(d=c.d + 1), L.UPR_ERR_SHAPE), (dict(kh=c.H + 2 * c.p + 1, Ho=1), L.UPR_ERR_SHAPE)]
    for layout, what in (("contig", "x"), ("slice4", "x"), ("contig", "dy"), ("slice8", "dy")):
        extra, coff = C.LAYOUTS[layout]
        ch = c.Cin if what == "x" else c.Cout
        lay = {("xl" if what == "x" else "dyl"): layout}
        bad.append((dict(lay, **{what + "_cs": coff + ch - 4}), L.UPR_ERR_ARG))   # the slice ends past the buffer's width
        bad.append((dict(lay, **{what + "_coff": coff + extra + 4}), L.UPR_ERR_ARG))
    dw0 = C.operands(c)["dw0"]
    for over, want in bad:
        over = dict(over)
        lay = {k: over.pop(k) for k in ("xl", "dyl") if k in over}
        o = _call(c, entry, x16=x16, dy16=entry == "into", **lay, **over)
        assert o.rc == want, (over, o.rc, want)
        assert o.ran == (C.NONE, 0, 0, 0, 0, 0), (over, o.ran)
        if "dw" not in over:
            assert torch.equal(o.dw, dw0), (over, "a refused call changed dw")
    # x NULL: refused unless x16 stands in for it on a shape the fp16 kernel takes
    o = _call(c, entry, x16=x16, x_null=True)
    if x16 and row.family == C.HALO16:
        assert o.rc == 0 and o.ran[0] == C.HALO16
    else:
        assert o.rc == L.UPR_ERR_ARG and o.ran[0] == C.NONE and torch.equal(o.dw, dw0)


def test_query_refuses_null_and_is_cleared_by_a_refused_call():
    L, lib, _ = _lib()
    assert lib.upr_t_conv_wgrad_ran(None) == L.UPR_ERR_ARG
    row = C.GEMM32_ROWS[0]
    assert _call(row.case, "wgrad").ran == C.route(row) + (0,)
    assert _call(row.case, "wgrad", kh=0).ran == (C.NONE, 0, 0, 0, 0, 0)
