"""Op-level parity of the EnhancedFAM attention kernels and the network tail
(csrc/train_fam.hip), of upr_t_pixel_sum / upr_t_broadcast / upr_t_broadcast16
(csrc/train_resample.hip) and of upr_t_pointwise (csrc/train_pointwise.hip)
against the float64 reference oracle/fam_ops.py (run with `-m gpu`).  Every
entry is called through ctypes (upr._lib.lib()) on inputs made on the CPU, one
op at a time: an op's operands are never another kernel's output.

Shapes.  The C == 32 attention kernels run 8 lanes a pixel on 16-byte aligned
buffers; fam_ca_bwd32_kernel splits HW into clamp(HW / 1024, 1, 256) chunks,
pixel_sum4_kernel into clamp(HW / (32 R), 1, 256) (R = 1024 / C row groups a
block; the same at C = 32).  ATT_SHAPES and PIXEL_SUM_CASES name what each
shape reaches.  Every other C, and C == 32 on a pointer one float past
alignment, takes the one-thread-per-pixel forms (fam_ca_bwd_kernel: LDS partials and
atomics, clamp(HW / 4096, 1, 256) chunks).

Tolerances (tests/op_parity.py, as test_gpu_bn_ops.py).
  * one or two IEEE operations with no choice of order (o2, g_o2, the channel
    maximum, broadcast, broadcast16, pointwise add / scale / dropout, the fp16
    copy of pool_bwd16), the generic forms against the 32-channel forms on
    elementwise outputs, and run-to-run determinism of the forms built
    without atomics: torch.equal;
  * the channel argmax on ties and NaN: g_o with ca = 1 is additions only, so
    it is compared bit for bit with the restatement that puts g_m[..., 1] on
    np.argmax's channel (the first maximum, or the first NaN);
  * everything else: the kernel's error against float64 within 4x the error
    of the same formula restated in plain fp32 torch ops on the CPU (sigmoid
    as 1 / (1 + exp(-x))), at least half an ulp of the largest |reference|,
    and under 1e-4 * max|ref| + 1e-6.

Measured on the MI355X: max |error| against float64 in ulp of the case's
largest |reference|, the worst case of each group; "used" is the worst kernel
error / allowed error over all cases (1 would fail):

  group (calls)                          restatement   kernel   used
  m mean_c, 32-channel (5)                   2.07        1.25    0.25
  m mean_c, generic (8)                      1.82        2.38    0.44
  sa, 32-channel / generic (5 / 8)           1.47        1.47    0.25
  out, 32-channel (5)                        1.16        1.16    0.25
  out, generic (8)                           1.35        1.35    0.31
  g_spre, 32-channel and sa_bwd_cs (10)      1.92        1.67    0.54
  g_spre, generic (8)                        1.84        2.73    0.54
  g_o, 32-channel / generic (5 / 7)          1.21        1.21    0.25
  g_ca, 32-channel (5)                       3.59        2.87    0.43
  g_ca, generic: fp32 atomics (7)            1.96        3.36    0.43
  pool_bwd, 4-channel / scalar (9 / 8)       0.50        0.50    0.25
  head illu (3)                              1.25        1.25    0.25
  retinex e / refl (3)                       1.26        1.26    0.25
  retinex enh (3)                            2.62        1.62    0.26
  retinex_bwd g_o (12)                       1.31        0.97    0.25
  retinex_bwd g_r (12)                      10.27       10.27    0.47
  saturated refl / enh / g_o                 5.23        5.02    0.25
  enhance e / enh (6)                        2.31        1.38    0.25
  enhance_bwd g_o / g_refl (6 / 3)           1.31        0.97    0.25
  pixel_sum, vector form (28)                4.50        6.74    0.61
  pixel_sum, scalar form: atomics (20)       1.89        4.36    0.67
  pointwise sigmoid / its backward (2)       1.32        1.32    0.25

  torch.equal groups (o2, max_c, g_o2, the argmax rule, generic vs 32-channel,
  g16, broadcast / broadcast16, pointwise add / scale / dropout and its mask,
  run-to-run determinism): no difference.  The two 263168-pixel cases take
  0.84 s (attention, all five ops) and 0.08 s (pixel_sum).

Two cases missed the bound as first written, both a long sequential chain of
fp32 additions where the restatement (torch's pairwise sum) has none; both
kernels now add in shorter chains.
  * upr_t_pixel_sum at C = 1024, HW = 300: 8.08 ulp against the restatement's
    1.91 (1.06x the allowed error).  The chunk count was HW / 1024 whatever C,
    right for C = 32 (R = 32 row groups, 32 rows a lane) but one block and 300
    rows a lane at R = 1 (256 rows a lane on the ASPP pool's C = 256).  It is
    now HW / (32 R): about 32 rows a lane at every C, the same at C = 32.
  * the generic upr_t_fam_ca_bwd at HW = 515: 6.92 ulp against 1.96 (0.99x,
    inside by 1%): one thread a channel added the block's 256 LDS partials in
    a row.  It now adds 8 groups of 32, then the 8 group sums (3.36 ulp).
upr_t_broadcast took any y_cs; y_cs < y_coff + C (overlapping rows) is now
UPR_ERR_ARG as in upr_t_broadcast16.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu
from op_parity import DEV, P, SENT, _np, _untouched, _within_restated
from oracle import fam_ops as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

# (B, HW) at C = 32: what fam_ca_bwd32_kernel does with it
ATT_SHAPES = [
    (1, 1),        # one pixel: 8 lanes of one wave
    (3, 37),       # a partial wave; the 32-pixel loop's second pass is 5 pixels
    (2, 2053),     # 2 chunks of 1027 / 1026 pixels
    (1, 5123),     # 5 chunks of 1025, the last 1023
    (1, 263168),   # HW / 1024 = 257 > 256: the chunk cap (1028 pixels a chunk)
]


def _lib():
    from upr import _lib as L
    return L, L.lib(), torch.cuda.current_stream().cuda_stream


def _sig32(x):
    """The kernels' sigmoid in fp32 torch ops: 1 / (1 + exp(-x))."""
    return 1.0 / (1.0 + torch.exp(-x))


def _dev(t, off1=False):
    """t on the device; off1: one element past an aligned address (the generic forms)."""
    if t is None:
        return None
    if not off1:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


def _out(shape, off1=False, dtype=torch.float32):
    """A sentinel-filled output: an entry that accumulated instead of overwriting would show."""
    return _dev(torch.full(shape, SENT, dtype=dtype), off1)


def _is_sent(t):
    return torch.equal(t, torch.full_like(t, SENT))


def _eq(a, b, what):
    assert torch.equal(a.cpu(), b.cpu()), f"{what}: not bit-equal"


# ---------------------------------------------------------------------------
# EnhancedFAM attention
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _att_inputs(B, HW, C):
    """Seeded CPU inputs: o = relu(randn) (the fusion conv's ReLU output, about
    half exact zeros), ca in (0.05, 0.95) with channel 1 exactly 0 and channel
    2 negative, s_pre ~ N(0, 4), gradients ~ N(0, 1); o2 = o * ca and sa =
    sigmoid(s_pre) in fp32, the operands of the later ops."""
    gen = torch.Generator().manual_seed(7919 * C + 31 * HW + B)
    d = {"o": torch.relu(torch.randn(B, HW, C, generator=gen))}
    ca = 0.05 + 0.9 * torch.rand(B, C, generator=gen)
    if C > 1:
        ca[:, 1] = 0.0
    if C > 2:
        ca[:, 2] = -0.3
    d["ca"] = ca
    d["s_pre"] = 2 * torch.randn(B, HW, generator=gen)
    for k, shape in (("g", (B, HW, C)), ("g_m", (B, HW, 2)), ("g_o2", (B, HW, C)), ("g_pool", (B, C)),
                     ("g_o0", (B, HW, C))):
        d[k] = torch.randn(shape, generator=gen)
    d["o2"] = d["o"] * ca[:, None, :]
    d["sa"] = _sig32(d["s_pre"])
    return d


def _ca_bwd32(g_o2, g_m, o, o2, ca):
    """The kernels' order in fp32: (g_o2 + g_m0 / C) + g_m1 at the argmax, then * ca / * o."""
    C = o2.shape[-1]
    am = torch.from_numpy(np.argmax(o2.numpy(), axis=-1))
    hit = torch.arange(C) == am[..., None]
    gt = (g_o2 + g_m[..., :1] / C) + torch.where(hit, g_m[..., 1:], torch.zeros(()))
    return gt * ca[:, None, :], (gt * o).sum(1)


def _run_attention(d, B, HW, C, off1=False):
    """ca_apply, sa_apply, sa_bwd, ca_bwd (C <= 32; twice) and pool_bwd on the
    CPU-made operands of d, every output sentinel-filled before the call."""
    _, lib, st = _lib()
    o, ca, o2_in, g, g_o2_in, g_pool = (_dev(d[k], off1) for k in ("o", "ca", "o2", "g", "g_o2", "g_pool"))
    s_pre, sa_in, g_m = _dev(d["s_pre"]), _dev(d["sa"]), _dev(d["g_m"])
    r = {"o2": _out((B, HW, C), off1), "m": _out((B, HW, 2)), "sa": _out((B, HW)), "out": _out((B, HW, C), off1),
         "g_o2": _out((B, HW, C), off1), "g_spre": _out((B, HW)), "pool": _dev(d["g_o0"], off1)}
    assert lib.upr_t_fam_ca_apply(P(o), P(ca), B, HW, C, P(r["o2"]), P(r["m"]), st) == 0
    assert lib.upr_t_fam_sa_apply(P(o2_in), P(s_pre), B, HW, C, P(r["sa"]), P(r["out"]), st) == 0
    assert lib.upr_t_fam_sa_bwd(P(g), P(o2_in), P(sa_in), B, HW, C, P(r["g_o2"]), P(r["g_spre"]), st) == 0
    if C <= 32:
        for k in ("", "_again"):
            r["g_o" + k], r["g_ca" + k] = _out((B, HW, C), off1), _out((B, C))
            assert lib.upr_t_fam_ca_bwd(P(g_o2_in), P(g_m), P(o), P(o2_in), P(ca), B, HW, C, P(r["g_o" + k]),
                                        P(r["g_ca" + k]), st) == 0
    assert lib.upr_t_fam_pool_bwd(P(r["pool"]), P(g_pool), P(o), B, HW, C, st) == 0
    torch.cuda.synchronize()
    return r


def _check_attention(r, d, B, HW, C, tag):
    n = {k: _np(v) for k, v in d.items()}
    o2_64, m64 = O.ca_apply(n["o"], n["ca"])
    assert np.array_equal(o2_64.astype(np.float32), d["o2"].numpy())  # one multiply: fp32 = float64 rounded once
    _eq(r["o2"], d["o2"], f"o2 {tag}")
    _eq(r["m"][..., 1], d["o2"].max(-1).values, f"max_c {tag}")
    _within_restated(f"m_mean {tag}", r["m"][..., 0], m64[..., 0], d["o2"].sum(-1) / C)
    sa64, out64 = O.sa_apply(n["o2"], n["s_pre"])
    _within_restated(f"sa {tag}", r["sa"], sa64, d["sa"])
    _within_restated(f"out {tag}", r["out"], out64, d["o2"] * d["sa"][..., None])
    g_o2_64, g_spre64 = O.sa_bwd(n["g"], n["o2"], n["sa"])
    _eq(r["g_o2"], d["g"] * d["sa"][..., None], f"g_o2 {tag}")
    _within_restated(f"g_spre {tag}", r["g_spre"], g_spre64, (d["g"] * d["o2"]).sum(-1) * d["sa"] * (1.0 - d["sa"]))
    if C <= 32:
        g_o64, g_ca64 = O.ca_bwd(n["g_o2"], n["g_m"], n["o"], n["o2"], n["ca"])
        g_o32, g_ca32 = _ca_bwd32(d["g_o2"], d["g_m"], d["o"], d["o2"], d["ca"])
        _within_restated(f"g_o {tag}", r["g_o"], g_o64, g_o32)
        _within_restated(f"g_ca {tag}", r["g_ca"], g_ca64, g_ca32)  # from a sentinel: overwritten, not added to
        _eq(r["g_o_again"], r["g_o"], f"g_o twice {tag}")
    pool64 = O.pool_bwd(n["g_o0"], n["g_pool"], n["o"])
    pool32 = torch.where(d["o"] > 0, d["g_o0"] + d["g_pool"][:, None, :] / HW, torch.zeros(()))
    _within_restated(f"pool_bwd {tag}", r["pool"], pool64, pool32)


@pytest.mark.parametrize("B,HW", ATT_SHAPES)
def test_fam_attention_c32(B, HW):
    """The 8-lanes-a-pixel forms of upr_t_fam_ca_apply / _sa_apply / _sa_bwd /
    _ca_bwd and the 4-channel upr_t_fam_pool_bwd against float64; g_ca (from a
    sentinel-filled buffer: overwritten) is the same bits run to run."""
    d = _att_inputs(B, HW, 32)
    r = _run_attention(d, B, HW, 32)
    _check_attention(r, d, B, HW, 32, f"c32 B{B} HW{HW}")
    _eq(r["g_ca_again"], r["g_ca"], "g_ca of the 32-channel form, run to run")


@pytest.mark.parametrize("C", [1, 3, 8, 31, 48])
def test_fam_attention_generic(C):
    """The one-thread-per-pixel forms at C != 32 (B = 2, HW = 515: three
    blocks of pixels, the last partial).  C = 48: upr_t_fam_ca_bwd returns
    UPR_ERR_ARG and writes nothing."""
    L, lib, st = _lib()
    B, HW = 2, 515
    d = _att_inputs(B, HW, C)
    r = _run_attention(d, B, HW, C)
    _check_attention(r, d, B, HW, C, f"generic C{C} B{B} HW{HW}")
    if C > 32:
        t = [_dev(d[k]) for k in ("g_o2", "g_m", "o", "o2", "ca")]
        g_o, g_ca = _out((B, HW, C)), _out((B, C))
        assert lib.upr_t_fam_ca_bwd(*map(P, t), B, HW, C, P(g_o), P(g_ca), st) == L.UPR_ERR_ARG
        torch.cuda.synchronize()
        assert _is_sent(g_o) and _is_sent(g_ca)


@pytest.mark.parametrize("B,HW", [(2, 515), (1, 5123), (1, 8200)])
def test_fam_attention_generic_matches_c32(B, HW):
    """C = 32 with every [.., C] buffer one float past alignment takes the
    generic forms: elementwise outputs equal the 32-channel forms' bit for
    bit, sums (another order) hold the float64 bound.  HW = 8200: the generic
    ca_bwd's 2 chunks add into g_ca atomically."""
    d = _att_inputs(B, HW, 32)
    a = _run_attention(d, B, HW, 32)
    g = _run_attention(d, B, HW, 32, off1=True)
    _check_attention(g, d, B, HW, 32, f"generic C32 off1 B{B} HW{HW}")
    for k in ("o2", "sa", "out", "g_o2", "g_o", "pool"):
        _eq(g[k], a[k], f"{k}: generic form vs 32-channel form")
    _eq(g["m"][..., 1], a["m"][..., 1], "max_c: generic form vs 32-channel form")


@pytest.mark.parametrize("layout", ["compact", "slice0", "slice32", "slice64", "cs33"])
def test_fam_sa_bwd_cs(layout):
    """upr_t_fam_sa_bwd_cs with g the compact tensor, a 32-channel slice of a
    [M, 96] buffer holding 3e4 elsewhere, and a [M, 33] buffer (g_cs % 4 != 0:
    the generic form): the same g_o2 bits and g_spre within the float64 bound;
    g_cs < C is UPR_ERR_ARG with nothing written."""
    L, lib, st = _lib()
    B, HW, C = 2, 515, 32
    d = _att_inputs(B, HW, C)
    cs, coff = {"compact": (32, 0), "slice0": (96, 0), "slice32": (96, 32), "slice64": (96, 64), "cs33": (33, 0)}[layout]
    gw = torch.full((B * HW, cs), 3e4)
    gw[:, coff:coff + C] = d["g"].view(-1, C)
    gw, o2, sa = gw.to(DEV), _dev(d["o2"]), _dev(d["sa"])
    g_o2, g_spre = _out((B, HW, C)), _out((B, HW))
    assert lib.upr_t_fam_sa_bwd_cs(P(gw, coff), cs, P(o2), P(sa), B, HW, C, P(g_o2), P(g_spre), st) == 0
    torch.cuda.synchronize()
    n = {k: _np(d[k]) for k in ("g", "o2", "sa")}
    _eq(g_o2, d["g"] * d["sa"][..., None], f"g_o2 {layout}")
    _within_restated(f"g_spre cs {layout}", g_spre, O.sa_bwd(n["g"], n["o2"], n["sa"])[1],
                     (d["g"] * d["o2"]).sum(-1) * d["sa"] * (1.0 - d["sa"]))
    g_o2, g_spre = _out((B, HW, C)), _out((B, HW))
    assert lib.upr_t_fam_sa_bwd_cs(P(gw), 16, P(o2), P(sa), B, HW, C, P(g_o2), P(g_spre), st) == L.UPR_ERR_ARG
    torch.cuda.synchronize()
    assert _is_sent(g_o2) and _is_sent(g_spre)


def _argmax_tensor():
    """o2 [1, 64, 32]: eight crafted pixels, then 56 pixels of small integers
    (most of them with their maximum on several channels and lanes)."""
    gen = torch.Generator().manual_seed(41)
    o2 = torch.randint(0, 4, (1, 64, 32), generator=gen).float()
    nan, inf = float("nan"), float("inf")
    base = -torch.rand(8, 32, generator=gen) - 1.0  # distinct values in (-2, -1)
    base[0] = 0.0                                   # all zeros
    base[1] = -1.5                                  # all equal and negative
    base[2, [2, 3]] = 7.0                           # the maximum twice in one lane
    base[3, [5, 21]] = 7.0                          # in lanes 1 and 5
    base[4, [31, 0]] = 7.0                          # in the last and the first channel
    base[5] = -inf                                  # all -inf
    base[6, 4], base[6, 9], base[6, 30] = 9.0, nan, nan  # the first NaN wins over a larger finite value
    base[7, 0] = nan                                # NaN at channel 0 only
    o2[0, :8] = base
    want = [0, 0, 2, 5, 0, 0, 9, 0]
    return o2, want


@pytest.mark.parametrize("off1", [False, True], ids=["c32", "generic"])
def test_fam_argmax_rule(off1):
    """The channel argmax of upr_t_fam_ca_bwd on ties, infinities and NaN is
    torch.max(dim)'s (first maximum, or first NaN), in the 8-lane shuffle
    reduction and in the generic scan: with ca = 1, g_o = (g_o2 + g_m0 / 32) +
    g_m1 at that channel is additions only, compared bit for bit; and
    upr_t_fam_ca_apply's maximum on the same tensor is the maximum, NaN where
    a NaN is present."""
    _, lib, st = _lib()
    B, HW, C = 1, 64, 32
    o2, want = _argmax_tensor()
    assert np.argmax(o2.numpy(), -1)[0, :8].tolist() == want
    gen = torch.Generator().manual_seed(42)
    g_o2, g_m = torch.randn(B, HW, C, generator=gen), torch.randn(B, HW, 2, generator=gen)
    g_m[..., 1] = 1000.0 + torch.arange(HW)  # far from everything else: a misplaced route shows
    ca = torch.ones(B, C)
    g_o32, _ = _ca_bwd32(g_o2, g_m, o2, o2, ca)
    t = [_dev(x, off1) for x in (g_o2,)] + [_dev(g_m)] + [_dev(x, off1) for x in (o2, o2, ca)]
    g_o, g_ca = _out((B, HW, C), off1), _out((B, C))
    assert lib.upr_t_fam_ca_bwd(*map(P, t), B, HW, C, P(g_o), P(g_ca), st) == 0
    o2_out, m = _out((B, HW, C), off1), _out((B, HW, 2))
    assert lib.upr_t_fam_ca_apply(P(t[2]), P(t[4]), B, HW, C, P(o2_out), P(m), st) == 0
    torch.cuda.synchronize()
    got = g_o.cpu()
    routed = (got - (g_o2 + g_m[..., :1] / C)) > 500.0
    assert routed.sum(-1).eq(1).all(), "the max route must land on exactly one channel a pixel"
    assert routed[0, :8].float().argmax(-1).tolist() == want
    _eq(got, g_o32, "g_o on ties / NaN")
    mx = o2.max(-1).values
    assert torch.equal(torch.nan_to_num(m[..., 1].cpu(), nan=12345.0), torch.nan_to_num(mx, nan=12345.0))
    assert torch.isnan(m[0, 6, 1]) and torch.isnan(m[0, 7, 1]) and m[0, 5, 1] == -float("inf")


POOL_CASES = [(3, 37, 32), (2, 2053, 32), (2, 515, 12), (2, 515, 6)]


@pytest.mark.parametrize("B,HW,C", POOL_CASES)
def test_fam_pool_bwd(B, HW, C):
    """upr_t_fam_pool_bwd and upr_t_fam_pool_bwd16 in place on g_o: C = 32
    runs 4 channels a thread (the scalar kernel on an unaligned g_o gives the
    same bits), g16 == g_o.half(); C = 12 (C / 4 = 3 does not divide 256) and
    C = 6 take the scalar kernel, and refuse the fp16 copy with
    UPR_ERR_UNSUPPORTED leaving g_o alone; so does a g16 address 2 mod 8."""
    L, lib, st = _lib()
    d = _att_inputs(B, HW, C)
    o, g_pool = _dev(d["o"]), _dev(d["g_pool"])
    ref = O.pool_bwd(_np(d["g_o0"]), _np(d["g_pool"]), _np(d["o"]))
    rs = torch.where(d["o"] > 0, d["g_o0"] + d["g_pool"][:, None, :] / HW, torch.zeros(()))
    g_o = _dev(d["g_o0"])
    assert lib.upr_t_fam_pool_bwd(P(g_o), P(g_pool), P(o), B, HW, C, st) == 0
    torch.cuda.synchronize()
    _within_restated(f"pool_bwd B{B} HW{HW} C{C}", g_o, ref, rs)
    vec = C % 4 == 0 and 256 % (C // 4) == 0
    g_o_b, g16 = _dev(d["g_o0"]), _out((B, HW, C), dtype=torch.float16)
    rc = lib.upr_t_fam_pool_bwd16(P(g_o_b), P(g_pool), P(o), B, HW, C, P(g16), st)
    torch.cuda.synchronize()
    if vec:
        assert rc == 0
        _eq(g_o_b, g_o, "pool_bwd16's g_o vs pool_bwd's")
        _eq(g16, g_o.half(), "g16 vs g_o.half()")
        g_o_u = _dev(d["g_o0"], off1=True)
        assert lib.upr_t_fam_pool_bwd(P(g_o_u), P(g_pool), P(o), B, HW, C, st) == 0
        torch.cuda.synchronize()
        _eq(g_o_u, g_o, "pool_bwd: scalar kernel vs 4-channel kernel")
    else:
        assert rc == L.UPR_ERR_UNSUPPORTED
        _eq(g_o_b, d["g_o0"], "a refused pool_bwd16 wrote g_o")
        assert _is_sent(g16)
    g_o_c, g16 = _dev(d["g_o0"]), _out((B, HW, C), off1=True, dtype=torch.float16)
    assert P(g16) % 8 == 2
    assert lib.upr_t_fam_pool_bwd16(P(g_o_c), P(g_pool), P(o), B, HW, C, P(g16), st) == L.UPR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    _eq(g_o_c, d["g_o0"], "a refused pool_bwd16 wrote g_o")
    assert _is_sent(g16)


# ---------------------------------------------------------------------------
# network tail
# ---------------------------------------------------------------------------
TAIL_SHAPES = [(1, 1, 1), (3, 5, 7), (2, 16, 24)]  # H != W and B > 1: an NCHW / NHWC index slip shows


@functools.lru_cache(maxsize=4)
def _tail_inputs(B, H, W, saturated=False):
    """x in [0, 1], r ~ N(0, 1) (saturated: -200), o ~ N(0, 2), illu in [0.05,
    1] (saturated: the head's own 0), gradients ~ N(0, 1); e = sigmoid(o) and
    refl = x / (illu + 1e-6) in fp32, the backward's saved operands."""
    gen = torch.Generator().manual_seed(1009 * H + 13 * W + B + (5 if saturated else 0))
    d = {"x": torch.rand(B, 3, H, W, generator=gen), "r": torch.randn(B, H, W, generator=gen),
         "o": 2 ** 0.5 * torch.randn(B, H, W, 3, generator=gen),
         "illu": 0.05 + 0.95 * torch.rand(B, H, W, generator=gen)}
    if saturated:
        d["r"] = torch.full((B, H, W), -200.0)
        d["illu"] = torch.zeros(B, H, W)
    for k, shape in (("g_enh", (B, 3, H, W)), ("g_refl", (B, 3, H, W)), ("g_illu", (B, H, W))):
        d[k] = torch.randn(shape, generator=gen)
    d["e"] = _sig32(d["o"])
    d["refl"] = d["x"] / (d["illu"] + 1e-6)[:, None]
    return d


def _combine32(rv, ec):
    return rv * ec + (1.0 - rv) * (ec * ec)


def _retinex_bwd32(d, with_refl, with_illu):
    """retinex_bwd_kernel's order in fp32 torch ops."""
    x, il, rv, ge = d["x"], d["illu"], d["refl"], d["g_enh"]
    ec = d["e"].permute(0, 3, 1, 2)
    den = il + 1e-6
    gev = ge * (rv + 2.0 * ec * (1.0 - rv))
    grv = ge * (ec - ec * ec)
    if with_refl:
        grv = grv + d["g_refl"]
    gi = d["g_illu"] if with_illu else torch.zeros_like(il)
    for c in range(3):
        gi = gi - grv[:, c] * x[:, c] / (den * den)
    return (gev * ec * (1.0 - ec)).permute(0, 2, 3, 1), gi * il * (1.0 - il)


@pytest.mark.parametrize("B,H,W", TAIL_SHAPES)
def test_head_and_retinex_forward(B, H, W):
    """upr_t_head_fwd (x NCHW, r and illu one channel) and upr_t_retinex_fwd
    (o and e NHWC; refl and enh NCHW) against float64."""
    _, lib, st = _lib()
    d = _tail_inputs(B, H, W)
    n = {k: _np(v) for k, v in d.items()}
    tag = f"B{B} H{H} W{W}"
    x, r, il, o = (_dev(d[k]) for k in ("x", "r", "illu", "o"))
    illu = _out((B, H, W))
    assert lib.upr_t_head_fwd(P(x), P(r), P(illu), B, H, W, st) == 0
    e, refl, enh = _out((B, H, W, 3)), _out((B, 3, H, W)), _out((B, 3, H, W))
    assert lib.upr_t_retinex_fwd(P(x), P(il), P(o), P(e), P(refl), P(enh), B, H, W, st) == 0
    torch.cuda.synchronize()
    xs = d["x"]
    _within_restated(f"head illu {tag}", illu, O.head_fwd(n["x"], n["r"]),
                     _sig32((xs[:, 0] + xs[:, 1] + xs[:, 2]) / 3.0 + d["r"]))
    e64, refl64, enh64 = O.retinex_fwd(n["x"], n["illu"], n["o"])
    _within_restated(f"retinex e {tag}", e, e64, d["e"])
    _within_restated(f"retinex refl {tag}", refl, refl64, d["refl"])
    _within_restated(f"retinex enh {tag}", enh, enh64, _combine32(d["refl"], d["e"].permute(0, 3, 1, 2)))


@pytest.mark.parametrize("with_refl,with_illu", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("B,H,W", TAIL_SHAPES)
def test_retinex_backward(B, H, W, with_refl, with_illu):
    """upr_t_retinex_bwd from the saved x, illu, e and refl, with all of, each
    of and none of g_refl / g_illu."""
    _, lib, st = _lib()
    d = _tail_inputs(B, H, W)
    n = {k: _np(v) for k, v in d.items()}
    t = [_dev(d[k]) for k in ("x", "illu", "e", "refl", "g_enh")]
    g_refl, g_illu = _dev(d["g_refl"]) if with_refl else None, _dev(d["g_illu"]) if with_illu else None
    g_o, g_r = _out((B, H, W, 3)), _out((B, H, W))
    assert lib.upr_t_retinex_bwd(*map(P, t), P(g_refl), P(g_illu), P(g_o), P(g_r), B, H, W, st) == 0
    torch.cuda.synchronize()
    g_o64, g_r64 = O.retinex_bwd(n["x"], n["illu"], n["e"], n["refl"], n["g_enh"], n["g_refl"] if with_refl else None,
                                 n["g_illu"] if with_illu else None)
    g_o32, g_r32 = _retinex_bwd32(d, with_refl, with_illu)
    tag = f"B{B} H{H} W{W} g_refl={with_refl} g_illu={with_illu}"
    _within_restated(f"retinex_bwd g_o {tag}", g_o, g_o64, g_o32)
    _within_restated(f"retinex_bwd g_r {tag}", g_r, g_r64, g_r32)


def test_retinex_saturated():
    """r = -200: exp(200 - mean x) overflows fp32, illu == 0 exactly, the
    denominator is 1e-6 and refl = x * 1e6.  Forward and backward stay finite
    and inside the same bound; g_r = gi * 0 * (1 - 0) is exactly 0."""
    _, lib, st = _lib()
    B, H, W = 2, 5, 7
    d = _tail_inputs(B, H, W, True)
    n = {k: _np(v) for k, v in d.items()}
    x, r, o = (_dev(d[k]) for k in ("x", "r", "o"))
    illu = _out((B, H, W))
    assert lib.upr_t_head_fwd(P(x), P(r), P(illu), B, H, W, st) == 0
    e, refl, enh = _out((B, H, W, 3)), _out((B, 3, H, W)), _out((B, 3, H, W))
    assert lib.upr_t_retinex_fwd(P(x), P(illu), P(o), P(e), P(refl), P(enh), B, H, W, st) == 0
    t = [_dev(d[k]) for k in ("x", "illu", "e", "refl", "g_enh", "g_refl", "g_illu")]
    g_o, g_r = _out((B, H, W, 3)), _out((B, H, W))
    assert lib.upr_t_retinex_bwd(*map(P, t), P(g_o), P(g_r), B, H, W, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(illu, torch.zeros_like(illu)), "sigmoid(-200 + mean x) must be exactly 0 in fp32"
    e64, refl64, enh64 = O.retinex_fwd(n["x"], n["illu"], n["o"])
    assert refl64.max() > 9e5
    _within_restated("saturated refl", refl, refl64, d["refl"])
    _within_restated("saturated enh", enh, enh64, _combine32(d["refl"], d["e"].permute(0, 3, 1, 2)))
    g_o64, g_r64 = O.retinex_bwd(n["x"], n["illu"], n["e"], n["refl"], n["g_enh"], n["g_refl"], n["g_illu"])
    _within_restated("saturated g_o", g_o, g_o64, _retinex_bwd32(d, 1, 1)[0])
    assert not g_r64.any() and torch.equal(g_r, torch.zeros_like(g_r)), "g_r must be exactly 0"


@pytest.mark.parametrize("with_refl", [1, 0])
@pytest.mark.parametrize("B,H,W", TAIL_SHAPES)
def test_enhance(B, H, W, with_refl):
    """upr_t_enhance_fwd and upr_t_enhance_bwd (g_refl nullable) against float64."""
    _, lib, st = _lib()
    d = _tail_inputs(B, H, W)
    n = {k: _np(v) for k, v in d.items()}
    tag = f"B{B} H{H} W{W} g_refl={with_refl}"
    rf, o, ein, ge = (_dev(d[k]) for k in ("refl", "o", "e", "g_enh"))
    e, enh = _out((B, H, W, 3)), _out((B, 3, H, W))
    assert lib.upr_t_enhance_fwd(P(rf), P(o), P(e), P(enh), B, H, W, st) == 0
    g_o, g_refl = _out((B, H, W, 3)), _out((B, 3, H, W))
    assert lib.upr_t_enhance_bwd(P(ein), P(rf), P(ge), P(g_o), P(g_refl) if with_refl else None, B, H, W, st) == 0
    torch.cuda.synchronize()
    ec, rv = d["e"].permute(0, 3, 1, 2), d["refl"]
    e64, enh64 = O.enhance_fwd(n["refl"], n["o"])
    _within_restated(f"enhance e {tag}", e, e64, d["e"])
    _within_restated(f"enhance enh {tag}", enh, enh64, _combine32(rv, ec))
    g_o64, g_rf64 = O.enhance_bwd(n["e"], n["refl"], n["g_enh"])
    g_o32 = (d["g_enh"] * (rv + 2.0 * ec * (1.0 - rv)) * ec * (1.0 - ec)).permute(0, 2, 3, 1)
    _within_restated(f"enhance_bwd g_o {tag}", g_o, g_o64, g_o32)
    if with_refl:
        _within_restated(f"enhance_bwd g_refl {tag}", g_refl, g_rf64, d["g_enh"] * (ec - ec * ec))
    else:
        assert _is_sent(g_refl)


# ---------------------------------------------------------------------------
# pixel sums and their broadcast
# ---------------------------------------------------------------------------
PIXEL_SUM_CASES = [
    # B, HW, C, cs, coff: pixel_sum4_kernel (R = 256 / (C / 4) row groups, clamp(HW / (32 R), 1, 256) chunks)
    (2, 1, 32, 32, 0),          # one pixel: 31 of 32 row groups idle
    (3, 37, 32, 32, 0),         # R = 32: the 4R loop never runs, the R tail twice
    (2, 2053, 32, 128, 96),     # 2 chunks; the last 32 channels of a 128-wide buffer
    (1, 5123, 12, 12, 0),       # C / 4 = 3: R = 85, one idle lane; one chunk, 61 rows a lane
    (2, 700, 256, 1280, 1024),  # the ASPP backward's slice: R = 4, 5 chunks of 140 rows
    (1, 300, 1024, 1024, 0),    # R = 1: one row group; 9 chunks of 34 rows, the last 28
    (1, 263168, 32, 32, 0),     # HW / 1024 = 257: the 256-chunk cap
    # pixel_sum_kernel (scalar, atomics; clamp(HW / 2048, 1, 256) chunks, cb passes of 256 channels)
    (2, 515, 3, 3, 0),
    (2, 4100, 6, 8, 1),         # 2 chunks
    (1, 50, 1028, 1028, 0),     # C > 1024: 5 cb passes, the last 4 wide
    (1, 90, 259, 259, 0),       # 2 cb passes, the last 3 wide (R = 85)
    (2, 515, 32, 33, 1),        # C = 32 off the vector layout
]


@pytest.mark.parametrize("B,HW,C,cs,coff", PIXEL_SUM_CASES)
def test_pixel_sum(B, HW, C, cs, coff):
    """upr_t_pixel_sum over a channel slice of a wider buffer holding 3e4
    elsewhere, scale 1 and 1 / HW, fresh into a sentinel-filled out and added
    to a non-zero out; the vector form (no atomics) gives the same bits twice."""
    _, lib, st = _lib()
    gen = torch.Generator().manual_seed(HW + C)
    x = torch.randn(B, HW, C, generator=gen)
    out0 = torch.linspace(-3, 3, B * C).view(B, C)
    xw = torch.full((B * HW, cs), 3e4)
    xw[:, coff:coff + C] = x.view(-1, C)
    xw = xw.to(DEV)
    x64, s32 = _np(x), x.sum(1)
    vector = C % 4 == 0 and C <= 1024 and cs % 4 == 0 and coff % 4 == 0
    for scale in (1.0, 1.0 / HW):
        sc = torch.tensor(scale, dtype=torch.float32)  # the fp32 value the entry is given
        for accumulate in (0, 1):
            ref = O.pixel_sum(x64, float(sc), _np(out0) if accumulate else None)
            rs = out0 + s32 * sc if accumulate else s32 * sc
            outs = []
            for _ in range(2):
                out = out0.to(DEV) if accumulate else _out((B, C))
                assert lib.upr_t_pixel_sum(P(xw), B, HW, C, cs, coff, float(sc), P(out), accumulate, st) == 0
                torch.cuda.synchronize()
                outs.append(out)
            form = "vec" if vector else "scalar"
            _within_restated(f"pixel_sum {form} B{B} HW{HW} C{C} cs{cs}+{coff} scale={scale:.3g} acc={accumulate}",
                             outs[0], ref, rs)
            if vector:
                _eq(outs[1], outs[0], "pixel_sum (vector form), run to run")


def _bcast_ref(v, scale, B, HW, C):
    return (v * torch.tensor(scale, dtype=torch.float32))[:, None, :].expand(B, HW, C)


@pytest.mark.parametrize("B,HW,C,cs,coff", [(2, 37, 32, 32, 0), (2, 37, 32, 128, 96), (3, 5, 6, 6, 0)])
def test_broadcast(B, HW, C, cs, coff):
    """upr_t_broadcast (fresh, and added to a random y) and upr_t_broadcast16
    into a compact buffer or a channel slice whose other channels keep the
    sentinel: v * scale, then one add, bit for bit; (v * scale).half().  C = 6
    is UPR_ERR_UNSUPPORTED for the fp16 form."""
    L, lib, st = _lib()
    gen = torch.Generator().manual_seed(B + C + cs)
    v, scale = torch.randn(B, C, generator=gen), 0.37
    want = _bcast_ref(v, scale, B, HW, C)
    assert np.array_equal(O.broadcast(_np(v), np.float32(scale), HW).astype(np.float32), want.numpy())
    vd = v.to(DEV)
    y = _out((B * HW, cs))
    assert lib.upr_t_broadcast(P(vd), B, HW, C, scale, P(y), cs, coff, 0, st) == 0
    torch.cuda.synchronize()
    _eq(y[:, coff:coff + C], want.reshape(-1, C), "broadcast")
    _untouched(y, coff, C, "broadcast")
    y0 = torch.randn(B * HW, C, generator=gen)
    y[:, coff:coff + C] = y0.to(DEV)
    assert lib.upr_t_broadcast(P(vd), B, HW, C, scale, P(y), cs, coff, 1, st) == 0
    torch.cuda.synchronize()
    _eq(y[:, coff:coff + C], y0 + want.reshape(-1, C), "broadcast, accumulated")
    _untouched(y, coff, C, "broadcast, accumulated")
    y16 = _out((B * HW, cs), dtype=torch.float16)
    rc = lib.upr_t_broadcast16(P(vd), B, HW, C, scale, P(y16), cs, coff, st)
    torch.cuda.synchronize()
    if C % 4:
        assert rc == L.UPR_ERR_UNSUPPORTED and _is_sent(y16)
    else:
        assert rc == 0
        _eq(y16[:, coff:coff + C], want.reshape(-1, C).half(), "broadcast16")
        _untouched(y16, coff, C, "broadcast16")


def test_broadcast_refusals():
    """y_cs < y_coff + C: UPR_ERR_ARG from both entries; y_cs % 4 != 0 or a
    y16 address 2 mod 8: UPR_ERR_UNSUPPORTED from the fp16 form.  Nothing is
    written."""
    L, lib, st = _lib()
    B, HW, C = 2, 37, 32
    vd = torch.randn(B, C).to(DEV)
    y, y16 = _out((B * HW, 128)), _out((B * HW, 128), dtype=torch.float16)
    y16u = _out((B * HW, 128), off1=True, dtype=torch.float16)
    assert lib.upr_t_broadcast(P(vd), B, HW, C, 1.0, P(y), 120, 96, 0, st) == L.UPR_ERR_ARG
    assert lib.upr_t_broadcast(P(vd), B, HW, C, 1.0, P(y), 16, 0, 1, st) == L.UPR_ERR_ARG
    assert lib.upr_t_broadcast16(P(vd), B, HW, C, 1.0, P(y16), 120, 96, st) == L.UPR_ERR_ARG
    assert lib.upr_t_broadcast16(P(vd), B, HW, C, 1.0, P(y16), 34, 0, st) == L.UPR_ERR_UNSUPPORTED
    assert lib.upr_t_broadcast16(P(vd), B, HW, C, 1.0, P(y16u), 32, 0, st) == L.UPR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert _is_sent(y) and _is_sent(y16) and _is_sent(y16u)


# ---------------------------------------------------------------------------
# upr_t_pointwise
# ---------------------------------------------------------------------------
N_PW = 10007  # not a multiple of 256; several blocks


def _pointwise(lib, st, a, b, op, inplace, mask_in=None, mask_out=None, p=0.0, seed=0):
    ad = a.to(DEV)
    out = ad if inplace else _out(tuple(a.shape))
    rc = lib.upr_t_pointwise(P(ad), P(b), P(out), a.numel(), op, P(mask_in), P(mask_out), p, seed, st)
    torch.cuda.synchronize()
    assert rc == 0
    if not inplace:
        _eq(ad, a, "pointwise wrote its operand")
    return out


@pytest.mark.parametrize("inplace", [False, True])
def test_pointwise_sigmoid_add_scale(inplace):
    """Ops 0 (sigmoid; the inputs include +-100, +-88, 0 and -0.0), 1 (its
    backward), 4 (add) and 5 (scale by a device scalar), out of place and with
    out == a."""
    _, lib, st = _lib()
    gen = torch.Generator().manual_seed(3)
    a, g = 3 * torch.randn(N_PW, generator=gen), torch.randn(N_PW, generator=gen)
    a[:6] = torch.tensor([100.0, -100.0, 0.0, -0.0, 88.0, -88.0])
    s32 = _sig32(a)
    tag = "in place" if inplace else "out of place"
    _within_restated(f"pointwise sigmoid {tag}", _pointwise(lib, st, a, None, 0, inplace), O.sigmoid(_np(a)), s32)
    _within_restated(f"pointwise sigmoid_bwd {tag}", _pointwise(lib, st, g, s32.to(DEV), 1, inplace),
                     O.sigmoid_bwd(_np(g), _np(s32)), g * s32 * (1.0 - s32))
    _eq(_pointwise(lib, st, a, g.to(DEV), 4, inplace), a + g, "pointwise add")
    k = torch.tensor([-1.7320508, 5.0])
    _eq(_pointwise(lib, st, a, k.to(DEV), 5, inplace), a * k[0], "pointwise scale")
    assert np.array_equal(O.add(_np(a), _np(g)).astype(np.float32), (a + g).numpy())
    assert np.array_equal(O.scale(_np(a), float(k[0])).astype(np.float32), (a * k[0]).numpy())


@pytest.mark.parametrize("seed", [1234567, 2 ** 63 + 5])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_pointwise_dropout(p, seed):
    """Op 2: the keep-mask is splitmix64 of (seed, index) >= p bit for bit,
    the same for the same seed and another for another; the kept count is
    within 4 standard deviations sqrt(n p (1 - p)) of n (1 - p) (p = 0 keeps
    everything); out = a * (1 / (1 - p)) on kept elements and 0 elsewhere;
    op 3 with that mask gives the same output."""
    _, lib, st = _lib()
    n = N_PW
    a = torch.randn(n, generator=torch.Generator().manual_seed(4))
    mask = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    out = _pointwise(lib, st, a, None, 2, False, mask_out=mask, p=p, seed=seed)
    want_mask = torch.from_numpy(O.dropout_mask(n, p, seed))
    _eq(mask, want_mask, "dropout mask")
    kept = int(want_mask.sum())
    assert abs(kept - n * (1 - p)) <= 4 * (n * p * (1 - p)) ** 0.5
    if p == 0.0:
        assert kept == n
    inv = 1.0 / (1.0 - torch.tensor(p, dtype=torch.float32))
    want = torch.where(want_mask.bool(), a * inv, torch.zeros(()))
    _eq(out, want, "dropout output")
    # (the float64 statement of the same: 1 / (1 - p) and the product round once each, 2^-24 relative)
    assert np.abs(O.dropout(_np(a), want_mask.numpy(), p) - _np(want)).max() <= 2.0 ** -22 * np.abs(_np(want)).max()
    mask2 = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    _pointwise(lib, st, a, None, 2, True, mask_out=mask2, p=p, seed=seed)
    _eq(mask2, mask, "the same seed, the same mask")
    if p > 0:
        _pointwise(lib, st, a, None, 2, False, mask_out=mask2, p=p, seed=seed + 1)
        assert not torch.equal(mask2, mask), "another seed gave the same mask"
    g = torch.randn(n, generator=torch.Generator().manual_seed(5))
    _eq(_pointwise(lib, st, g, None, 3, False, mask_in=mask, p=p),
        _pointwise(lib, st, g, None, 2, False, mask_out=mask2, p=p, seed=seed), "op 3 with op 2's mask")


def test_pointwise_refusals():
    """op outside 0..5, op 2 without mask_out, op 3 without mask_in and ops 1 /
    4 / 5 without b: UPR_ERR_ARG, nothing written."""
    L, lib, st = _lib()
    a, out = torch.randn(64).to(DEV), _out((64,))
    mask = torch.full((64,), 7, dtype=torch.uint8, device=DEV)
    for op, b, mi, mo in ((-1, a, mask, mask), (6, a, mask, mask), (2, None, None, None), (3, None, None, None),
                          (1, None, None, None), (4, None, None, None), (5, None, None, None)):
        assert lib.upr_t_pointwise(P(a), P(b), P(out), 64, op, P(mi), P(mo), 0.5, 1, st) == L.UPR_ERR_ARG
    torch.cuda.synchronize()
    assert _is_sent(out) and bool((mask == 7).all())
