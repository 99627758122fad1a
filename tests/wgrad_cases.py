"""Case tables of the MFMA-path weight-gradient tests (test_gpu_wgrad_ops.py on
the device, test_cpu_wgrad_cases.py without one): the shapes, the kernel each
is expected to reach, a pure-Python restatement of the three launchers' split
arithmetic (csrc/train_wgrad.hip launch_wgrad_gemm / launch_wgrad16 /
launch_wgrad16h and the dispatch in front of them), the seeded operands and
the two references (float64 oracle, plain fp32 torch on the CPU).

A row is Row(case, family, tile, note): case = (B, H, W, Cin, Cout, k, s, p, d),
family one of GEMM32 / TAP32 / IM2COL16 / HALO16 (UPR_WGRAD_* of
include/upr_train.h), tile the kernel's template arguments as
upr_t_conv_wgrad_ran reports them -- (BM, BN, 0), (BM, NR, 0) or
(CIN, NTAP, D).  The tile is typed in here and checked against the restated
dispatch; the split count always comes from the restatement."""
import collections
import functools
import zlib

import numpy as np
import torch

import op_parity
from oracle import conv_ops as O

NONE, GEMM32, TAP32, IM2COL16, HALO16 = 0, 1, 2, 3, 4
FAMILY = {NONE: "none", GEMM32: "wgrad_gemm", TAP32: "conv_wgrad (per tap)", IM2COL16: "wgrad16", HALO16: "wgrad16h"}

# op_parity's layouts and one more: slice8 is 12 channels wider, so its channel
# stride is no multiple of 8 and upr_t_conv_wgrad16's internal cast (x_cs % 8,
# x_coff % 8) does not take it; slice8x (16 wider, offset 8) is the slice it takes
LAYOUTS = dict(op_parity.LAYOUTS, slice8x=(16, 8))

Case = collections.namedtuple("Case", "B H W Cin Cout k s p d")
Row = collections.namedtuple("Row", "case family tile note")


def _row(case, family, tile, note=""):
    return Row(Case(*case), family, tuple(tile), note)


def out_hw(c):
    return O.out_size(c.H, c.k, c.s, c.p, c.d), O.out_size(c.W, c.k, c.s, c.p, c.d)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------
# the launchers' arithmetic, restated
# ---------------------------------------------------------------------------
WG_KP, W16_KP, WG_PPB = 32, 64, 1024  # pixels a K step (fp32, fp16); pixels a block of the per-tap kernel


def gemm32_tile(Cout):
    """wgrad_gemm's dispatch: (BM, BN)."""
    return (128, 64) if Cout % 128 == 0 else (64, 128) if Cout % 64 == 0 else (32, 256)


def gemm32_plan(c):
    """launch_wgrad_gemm: dict(tile, mtiles, ntiles, splits, pps, sizes = pixels of each split)."""
    Ho, Wo = out_hw(c)
    P, KT = c.B * Ho * Wo, c.k * c.k * c.Cin
    BM, BN = gemm32_tile(c.Cout)
    mtiles, ntiles = c.Cout // BM, cdiv(KT, BN)
    tiles = mtiles * ntiles
    splits = max(1, min(cdiv(1024, tiles), cdiv(P, 4 * WG_KP)))
    pps = cdiv(cdiv(P, splits), WG_KP) * WG_KP
    splits = cdiv(P, pps)
    sizes = [min(P, (i + 1) * pps) - i * pps for i in range(splits)]
    return dict(tile=(BM, BN, 0), mtiles=mtiles, ntiles=ntiles, splits=splits, pps=pps, sizes=sizes, P=P, KT=KT,
                slab_bytes=4 * splits * c.Cout * ntiles * BN)


def tap32_plan(c):
    """upr_t_conv_wgrad's fallback: blocks of 1024 pixels, added with atomics."""
    Ho, Wo = out_hw(c)
    P = c.B * Ho * Wo
    return dict(tile=(32, 32, 0), splits=cdiv(P, WG_PPB), P=P)


def im2col16_tile(c):
    """wgrad16_gemm + wgrad16_nr: (BM, NR)."""
    BM = 128 if c.Cout % 128 == 0 else 64 if c.Cout % 64 == 0 else 32
    nr = c.k * c.k * c.Cin // 32
    if BM <= 64 and nr % 9 == 0:
        return BM, 9
    if BM <= 64 and nr % 8 == 0:
        return BM, 8
    return BM, 4 if nr % 4 == 0 else 2 if nr % 2 == 0 else 1


def im2col16_plan(c):
    """launch_wgrad16: a unit is 64 consecutive pixels of one output row."""
    Ho, Wo = out_hw(c)
    assert Wo % W16_KP == 0, c
    units, nruns = c.B * Ho * (Wo // W16_KP), c.k * c.k * c.Cin // 32
    BM, NR = im2col16_tile(c)
    mtiles, ntiles = c.Cout // BM, cdiv(nruns, NR)
    tiles = mtiles * ntiles
    splits = max(1, min(cdiv(1024, tiles), cdiv(units, 4)))
    ups = cdiv(units, splits)
    splits = cdiv(units, ups)
    sizes = [min(units, (i + 1) * ups) - i * ups for i in range(splits)]
    return dict(tile=(BM, NR, 0), mtiles=mtiles, ntiles=ntiles, splits=splits, ups=ups, sizes=sizes, units=units)


def halo16_cfg(c):
    """wgrad16_gemm's halo gate + wgrad16h's dispatch: (CIN, NTAP, D, TR) or None
    when the halo form declines (then the im2col kernel runs)."""
    Ho, Wo = out_hw(c)
    if not (c.s == 1 and Ho == c.H and Wo == c.W and c.W % 64 == 0):
        return None
    if c.k == 1 and c.p == 0:
        cfg = (c.Cin, 1, 0, 4) if (c.Cin in (96, 128) and c.Cout == 32) else None
    elif c.k == 3 and c.p == c.d and c.d in (1, 2) and c.Cin == 32 and c.Cout == 32:
        cfg = (32, 9, c.d, 8 if c.d == 1 else 4)
    else:
        cfg = None
    if cfg is None or c.H % cfg[3]:
        return None
    return cfg


def halo16_plan(c):
    """launch_wgrad16h: a step is TR output rows of one 64-pixel column segment;
    a split = (image, row block, segment); row blocks of spb steps, the last shorter."""
    CIN, NTAP, D, TR = halo16_cfg(c)
    ntg, segs, spc = 1, c.W // 64, c.H // TR
    cols = c.B * segs * ntg
    nrb = max(1, min(cdiv(512, cols), (spc + 1) // 2))
    spb = cdiv(spc, nrb)
    nrb = cdiv(spc, spb)
    blocks = [min(spc, (i + 1) * spb) - i * spb for i in range(nrb)]
    return dict(tile=(CIN, NTAP, D), TR=TR, segs=segs, spc=spc, spb=spb, nrb=nrb, row_blocks=blocks,
                splits=c.B * nrb * segs)


def fp16_family(c):
    """The kernel an fp16 call (x16 given or cast) reaches: HALO16, IM2COL16, or
    GEMM32 when Wo % 64 != 0 (the fp32 arithmetic)."""
    if out_hw(c)[1] % W16_KP:
        return GEMM32
    return HALO16 if halo16_cfg(c) else IM2COL16


PLAN = {GEMM32: gemm32_plan, TAP32: tap32_plan, IM2COL16: im2col16_plan, HALO16: halo16_plan}


def route(row, family=None):
    """(family, t0, t1, t2, splits) as upr_t_conv_wgrad_ran reports it."""
    family = row.family if family is None else family
    plan = PLAN[family](row.case)
    return (family,) + tuple(plan["tile"]) + (plan["splits"],)


# ---------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------
LONG = Case(1, 240, 256, 256, 256, 3, 1, 1, 1)

GEMM32_ROWS = [
    _row((1, 3, 5, 32, 32, 1, 1, 0, 1), GEMM32, (32, 256, 0), "P 15: less than one step; KT 32 of a 256-wide tile"),
    _row((1, 5, 7, 32, 32, 3, 1, 1, 1), GEMM32, (32, 256, 0), "P 35: one split, the second step has 3 pixels; KT 288"),
    _row((2, 5, 7, 32, 64, 3, 1, 1, 1), GEMM32, (64, 128, 0), "P 70: the image boundary inside a step; 3 n-tiles"),
    _row((2, 9, 11, 64, 128, 3, 2, 1, 1), GEMM32, (128, 64, 0), "stride 2 at odd H, W (5 x 6 out); 9 full n-tiles"),
    _row((1, 13, 21, 32, 32, 3, 1, 2, 2), GEMM32, (32, 256, 0), "dilation 2; P 273: splits of 96, 96, 81"),
    _row((1, 12, 12, 32, 32, 3, 1, 0, 1), GEMM32, (32, 256, 0), "pad 0"),
    _row((2, 8, 8, 32, 96, 1, 2, 0, 1), GEMM32, (32, 256, 0), "the projecting shortcut; three m-tiles"),
    _row((1, 6, 10, 256, 256, 3, 1, 1, 1), GEMM32, (128, 64, 0), "two m-tiles by 36 n-tiles"),
    _row((1, 8, 12, 32, 64, 2, 2, 0, 1), GEMM32, (64, 128, 0), "the ConvTranspose form"),
    _row((1, 4, 16, 128, 32, 1, 1, 0, 1), GEMM32, (32, 256, 0), "EnhancedFAM fusion; a single partial n-tile"),
    _row((1, 4, 16, 96, 32, 1, 1, 0, 1), GEMM32, (32, 256, 0), "head fusion; a single partial n-tile"),
    _row(LONG, GEMM32, (128, 64, 0), "the long chain: 15 splits of 4096 pixels"),
]
# x / dy layouts run on the second, fourth and fifth row besides contiguous
GEMM32_LAYOUT_ROWS = (1, 3, 4)
GEMM32_LAYOUTS = [(xl, dyl) for xl in ("contig", "slice4", "slice8") for dyl in ("contig", "slice4", "slice8")
                  if (xl, dyl) != ("contig", "contig")]

# the per-tap kernel: the second and fourth rows above, and two shapes of its own
TAP32_ROWS = [
    GEMM32_ROWS[1]._replace(family=TAP32, tile=(32, 32, 0), note="P 35: one partial block"),
    GEMM32_ROWS[3]._replace(family=TAP32, tile=(32, 32, 0), note="stride 2, 64 -> 128: 4 x 18 tiles of one block"),
    _row((1, 32, 32, 32, 32, 3, 1, 1, 1), TAP32, (32, 32, 0), "P 1024: exactly one block (deterministic)"),
    _row((1, 25, 41, 32, 32, 3, 1, 1, 1), TAP32, (32, 32, 0), "P 1025: a second block of one pixel"),
]
# how a call is pushed off the GEMM: x or dy one float past alignment, or a packed dwp one float past
TAP32_WAYS = ("x_off1", "dy_off1", "dwp_off1")

IM2COL16_ROWS = [
    _row((1, 3, 64, 32, 32, 3, 1, 1, 1), IM2COL16, (32, 9, 0), "H % 8 != 0: not the halo form; 3 units, one split"),
    _row((1, 12, 64, 32, 32, 3, 1, 1, 1), IM2COL16, (32, 9, 0), "the halo form declines 12 % 8"),
    _row((2, 5, 64, 32, 64, 3, 1, 1, 1), IM2COL16, (64, 9, 0), "10 units: splits of 4, 4, 2; image boundary in a split"),
    _row((1, 6, 128, 64, 128, 3, 2, 1, 1), IM2COL16, (128, 2, 0), "stride 2; nine n-tiles"),
    _row((1, 4, 64, 256, 32, 1, 1, 0, 1), IM2COL16, (32, 8, 0), ""),
    _row((1, 4, 64, 128, 128, 1, 1, 0, 1), IM2COL16, (128, 4, 0), ""),
    _row((1, 2, 64, 32, 128, 1, 1, 0, 1), IM2COL16, (128, 1, 0), ""),
    _row((1, 2, 64, 32, 64, 1, 1, 0, 1), IM2COL16, (64, 1, 0), ""),
    _row((1, 2, 64, 64, 64, 1, 1, 0, 1), IM2COL16, (64, 2, 0), ""),
    _row((1, 4, 128, 32, 64, 2, 2, 0, 1), IM2COL16, (64, 4, 0), "ConvTranspose"),
    _row((1, 8, 64, 32, 32, 3, 1, 3, 3), IM2COL16, (32, 9, 0), "dilation 3: the halo form takes at most 2"),
    _row((1, 6, 66, 32, 32, 3, 1, 0, 1), IM2COL16, (32, 9, 0), "pad 0, Wo 64, Ho != H"),
    _row((2, 8, 64, 64, 64, 3, 1, 1, 1), IM2COL16, (64, 9, 0), "two n-tiles"),
    _row((1, 8, 64, 96, 32, 3, 1, 1, 1), IM2COL16, (32, 9, 0), "27 runs, three n-tiles"),
]
# dy contig / slice4 / slice8 (and dy16 in the same layout) on the third and the last-but-one row
IM2COL16_LAYOUT_ROWS = (2, 12)
# the longest im2col chain of the bs 8 512^2 step, 64 units a split (128 MFMA accumulations an
# accumulator), at the cheapest shape that reaches it: 36 tiles, so 29 splits of 64 units
IM2COL16_LONG = _row((1, 29, 4096, 256, 256, 3, 1, 1, 1), IM2COL16, (128, 4, 0), "the long chain: 29 splits of 64 units")

HALO16_ROWS = [
    _row((1, 8, 64, 32, 32, 3, 1, 1, 1), HALO16, (32, 9, 1), "one step, one segment, every halo zero"),
    _row((1, 8, 128, 32, 32, 3, 1, 1, 1), HALO16, (32, 9, 1), "a halo column is the neighbour segment's pixel"),
    _row((2, 24, 128, 32, 32, 3, 1, 1, 1), HALO16, (32, 9, 1), "3 steps a column: row blocks of 2 and 1; two images"),
    _row((1, 4, 64, 32, 32, 3, 1, 2, 2), HALO16, (32, 9, 2), "TR 4, one step"),
    _row((2, 12, 128, 32, 32, 3, 1, 2, 2), HALO16, (32, 9, 2), "the two-image case at TR 4"),
    _row((1, 4, 64, 96, 32, 1, 1, 0, 1), HALO16, (96, 1, 0), ""),
    _row((2, 12, 128, 96, 32, 1, 1, 0, 1), HALO16, (96, 1, 0), ""),
    _row((1, 4, 64, 128, 32, 1, 1, 0, 1), HALO16, (128, 1, 0), ""),
    _row((2, 12, 128, 128, 32, 1, 1, 0, 1), HALO16, (128, 1, 0), ""),
]
# dy slice4 / slice8 (+ dy16) on the two (2, .., 128) 3x3 rows
HALO16_LAYOUT_ROWS = (2, 4)

# Wo % 64 != 0: an fp16 call computes in fp32, on the unrounded x
ROUTING_ROW = _row((1, 8, 24, 32, 32, 3, 1, 1, 1), GEMM32, (32, 256, 0), "Wo 24: the fp16 entries run the fp32 GEMM")

ALL_ROWS = GEMM32_ROWS + TAP32_ROWS + IM2COL16_ROWS + [IM2COL16_LONG] + HALO16_ROWS + [ROUTING_ROW]


def wgrad_configs():
    """The distinct (Cin, Cout, k, s, p, d) of every table."""
    return sorted({tuple(r.case[3:]) for r in ALL_ROWS})


# ---------------------------------------------------------------------------
# operands and references (made once a case, never modified)
# ---------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(("wgrad",) + key).encode()))


@functools.lru_cache(maxsize=4)
def operands(c):
    """Seeded N(0, 1) CPU operands: x [B, H, W, Cin], dy [B, Ho, Wo, Cout], and
    dw0 [Cout, Cin, k, k], the gradient's starting value (the contract is +=)."""
    g = _gen(*c)
    Ho, Wo = out_hw(c)
    return {"x": torch.randn((c.B, c.H, c.W, c.Cin), generator=g), "dy": torch.randn((c.B, Ho, Wo, c.Cout), generator=g),
            "dw0": torch.randn((c.Cout, c.Cin, c.k, c.k), generator=g)}


def kernel_operands(c, fp16):
    """The operand values the kernel is specified to use, as fp32 tensors: the
    fp16 forms read x16 = (half)x and round dy to nearest-even (or read dy16)."""
    d = operands(c)
    if fp16:
        return d["x"].half().float(), d["dy"].half().float()
    return d["x"], d["dy"]


def dw64(c, x, dy):
    """The float64 weight gradient of (x, dy) at c's k, s, p, d: [Cout, Cin, k, k] numpy."""
    return O.conv_wgrad(x.double().numpy(), dy.double().numpy(), c.k, c.k, c.s, c.p, c.d)[0]


def wgrad64(c, x, dy):
    """dw0 + the float64 weight gradient."""
    return operands(c)["dw0"].double().numpy() + dw64(c, x, dy)


def wgrad32(c, x, dy):
    """dw0 + plain fp32 torch on the CPU (torch.nn.grad.conv2d_weight)."""
    dw = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (c.Cout, c.Cin, c.k, c.k), dy.permute(0, 3, 1, 2),
                                     stride=c.s, padding=c.p, dilation=c.d)
    return operands(c)["dw0"] + dw


@functools.lru_cache(maxsize=None)
def references(c, fp16):
    """(float64 reference, fp32 restatement) of dw0 + dw on the kernel's operands."""
    x, dy = kernel_operands(c, fp16)
    return wgrad64(c, x, dy), wgrad32(c, x, dy)


def as_kc(dw, Cout):
    """[Cout, Cin, k, k] -> [K, Cout]: the per-output-channel form of _within_restated."""
    return dw.reshape(Cout, -1).T
