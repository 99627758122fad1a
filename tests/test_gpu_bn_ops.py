"""Op-level parity of the BatchNorm training kernels (csrc/train_bn.hip) and of
clip + Adam / GradScaler's unscale (csrc/train_optim.hip) against the float64
reference oracle/bn_ops.py (run with `-m gpu`).  Every entry of the BatchNorm
and optimiser sections of include/upr_train.h is called through ctypes
(upr._lib.lib()); one test goes through upr.train.BN and one through
upr.optim.

Shapes.  chan_reduce2 runs slots = clamp(M / (16 R), 1, 256) blocks of R =
1024 / (C / 4) row groups; a block's rows go through an 8R loop (one-operand
modes), a 4R loop and an R loop.  SHAPES below names what each pair reaches.

Tolerances.
  * identities the header states as bit-identical (fp16-operand entries vs the
    fp32 entries on the widened operands, y16 == y.half(), the fused ReLU fold
    vs relu_mask + the plain call, run-to-run determinism): torch.equal;
  * statistics (mean, invstd, running statistics, the returned gradient norm;
    fp64 accumulation rounded once): 2 ulp of float32(reference); for the
    mean = 100, sigma = 0.05 inputs invstd adds M * 2^-53 * mean^2 / var
    relative, the worst-case rounding of the fp64 sum of squares, computed
    from the inputs;
  * elementwise fp32 results (y, dx, dgamma, dbeta, sums, Adam's p / m / v):
    the same formula restated in plain fp32 torch ops on the CPU is measured
    against the float64 reference on the same inputs (per channel for y and
    dx); the kernel must be within 4x that error (FMA contraction and another
    equally valid operation order cost about 2x each).  The restatement can
    land exactly on a short channel (M = 2), and the final rounding alone
    costs the kernel half an ulp, so its error counts as at least half an ulp
    of the channel's largest |reference|.  The project's op-level bound
    1e-4 * max|ref| + 1e-6 is also asserted, as a ceiling.

Measured on the MI355X: max |error| against float64 in ulp of the case's
largest |reference|, the worst case of each group; "used" is the worst kernel
error / allowed error over all channels and cases (1 would fail):

  group (cases)                      restatement   kernel   used
  y, bn_apply (21)                       1.65        1.65    0.60
  dx, reduce + apply (22)                2.26        1.99    0.51
  dx, fused (16)                         2.26        1.99    0.51
  dx, fused16 on x16 (10)                3.42        3.47    0.61
  dgamma, reduce + apply / fused         4.33        1.25    0.25
  dgamma, fused16                        2.71        1.05    0.20
  dbeta, all three                       2.15        0.95    0.25
  chan_sum, fp32 atomics (22)            2.43        3.69    0.51   (67003 x 256; varies run to run)
  chan_sum_ws (22)                       2.43        0.99    0.25
  chan_sum16 / chan_sum16s (18)          2.61        0.84    0.25
  BN class y / dx / dgamma / dbeta (8)   2.21        1.28    0.56
  Adam p, 6 steps x 3 runs               2.15        2.15    0.25
  Adam m                                 1.79        1.97    0.42
  Adam v                                 3.98        3.12    0.25

  statistics, in ulp of float32(reference), bound 2: mean 0, invstd 1,
  running_mean 1, running_var 1, eval invstd 0, clip norm 0.

Adam v is the case that found a fault: with 1 - beta2 and the bias
corrections formed in fp32 from (float)0.999, v was 1.3e-5 relative off
torch's at every step (12.6x the allowed error at step 1 with clipping, 26x
without; betas (0.8, 0.95) stayed inside).  upr_t_adam now takes the betas as
doubles and rounds 1 - beta and the corrections once.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu
from op_parity import DEV, LAYOUTS, P, SENT, _np, _slice, _untouched, _wide, _within_restated, _within_ulp
from oracle import bn_ops as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

EPS, MOM = 1e-5, 0.1

# (M, C): what chan_reduce2 / the apply4 kernels do with it
SHAPES = [
    (17, 32),      # R = 128 > M: slots == 1, most row groups idle; 256 % (C/4) == 0
    (2, 64),       # M = 2 (the unbiased variance's M / (M - 1) = 2)
    (301, 4),      # C/4 = 1: R = 1024 > M, slots == 1; shared memory R * 2C doubles = 64 KiB
    (1923, 64),    # 2*40*24 + 3 rows, R = 64, slots == 1, 30.05 rows a thread: 8R, 4R and R loops + tail
    (1991, 128),   # R = 32, slots = 3, 664 / 664 / 663 rows a block = 20.7 a thread: 8R, 8R, 4R, R tail
    (5003, 128),   # slots = 9, M % 9 == 8: the last block is short; 8R, 8R, R tail
    (4099, 1024),  # C/4 = 256, R = 4, slots = 64, 65 rows a block (the last 4)
    (67003, 256),  # R = 16, M / (16 R) = 261 > 256: the kRedSlots cap (262 rows a block, the last 193)
    (2003, 12),    # C/4 = 3: 256 % 3 != 0 (generic apply4 branch), R = 341 leaves thread 1023 idle; 4R + R loops
    (1537, 96),    # C/4 = 24: generic branch, R = 42 leaves 16 threads idle, slots = 2
    (811, 160),    # C/4 = 40: generic branch, R = 25 leaves 24 threads idle, slots = 2
    (1001, 3),     # C % 4 != 0: scalar apply / atomic reduction fallback, 2 blocks of rows
    (515, 6),      # C % 4 != 0 with C > 4
]
SHAPES4 = [s for s in SHAPES if s[1] % 4 == 0]  # the float4 / fp16 entries
BIG = (67003, 256)


def _lib():
    from upr import _lib as L
    return L, L.lib(), torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=2)
def _inputs(M, C, hard=False):
    """Seeded CPU inputs: x = randn * sigma_c + mu_c (hard: mu = 100, sigma =
    0.05, which only fp64 accumulation survives), gamma in [0.5, 1.5] with a
    few negative entries, beta in [-0.2, 0.2], g and res ~ N(0, 1), and the
    float64 batch statistics of x."""
    gen = torch.Generator().manual_seed(100003 * C + M + (7 if hard else 0))
    if hard:
        sig, mu = torch.full((C,), 0.05), torch.full((C,), 100.0)
    else:
        sig = 0.5 + 1.5 * torch.rand(C, generator=gen)
        mu = 2 * torch.rand(C, generator=gen) - 1
    d = {"x": torch.randn(M, C, generator=gen) * sig + mu}
    d["gamma"] = 0.5 + torch.rand(C, generator=gen)
    d["gamma"][1::5] *= -1
    d["beta"] = -0.2 + 0.4 * torch.rand(C, generator=gen)
    d["g"] = torch.randn(M, C, generator=gen)
    d["res"] = torch.randn(M, C, generator=gen)
    d["dx0"] = torch.randn(M, C, generator=gen)
    d["mean64"], d["var64"], d["invstd64"] = O.bn_stats(_np(d["x"]), EPS)
    # the statistics the apply / backward entries are given: the reference's, rounded to fp32
    d["mean"] = torch.from_numpy(d["mean64"]).float()
    d["invstd"] = torch.from_numpy(d["invstd64"]).float()
    return d


# ---------------------------------------------------------------------------
# plain fp32 restatements (torch CPU ops, no FMA, torch's own summation)
# ---------------------------------------------------------------------------
def _apply32(x, mean, invstd, gamma, beta, res, res_post, relu):
    v = ((x - mean) * invstd) * gamma + beta
    if res is not None and not res_post:
        v = v + res
    if relu:
        v = torch.relu(v)
    if res is not None and res_post:
        v = v + res
    return v


def _bwd32(g, x, mean, invstd, gamma, batch_stats, mask, dx0, dg0, db0):
    if mask is not None:
        g = g * mask
    M = x.shape[0]
    xh = (x - mean) * invstd
    sg, sgx = g.sum(0), (g * xh).sum(0)
    dx = gamma * invstd * (g - sg / M - xh * (sgx / M)) if batch_stats else gamma * invstd * g
    if dx0 is not None:
        dx = dx + dx0
    return dx, dg0 + sgx, db0 + sg


# ---------------------------------------------------------------------------
# forward statistics
# ---------------------------------------------------------------------------
def _run_stats(lib, st, xw, M, C, cs, coff, rm0, rv0):
    """bn_stats (into a garbage-filled acc: it overwrites on every path) +
    bn_finalize; returns acc[:2C], mean, invstd, rm, rv, nbt."""
    acc = torch.full((lib.upr_t_reduce_acc_doubles(C),), 1e300, dtype=torch.float64, device=DEV)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    nbt = torch.tensor(41, dtype=torch.int64, device=DEV)
    mean, inv = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    assert lib.upr_t_bn_stats(P(xw), M, C, cs, coff, P(acc), st) == 0
    assert lib.upr_t_bn_finalize(P(acc), M, C, MOM, EPS, P(rm), P(rv), P(nbt), P(mean), P(inv), st) == 0
    torch.cuda.synchronize()
    return acc[:2 * C].clone(), mean, inv, rm, rv, nbt


def _running0(d, C):
    """Running statistics before the update: the running mean has the batch
    mean's sign, so the update adds two terms of one sign and the 2 ulp bound
    is not asked of a cancelling sum; the running variance is in [0.5, 2]."""
    return torch.from_numpy(0.7 * d["mean64"]).float(), torch.linspace(0.5, 2, C)


STATS_CASES = [(M, C, "contig", False) for M, C in SHAPES] + [
    (1991, 128, "slice4", False), (1537, 96, "slice8", False), (17, 32, "off1", False), (1923, 64, "off1", False),
    (515, 6, "slice4", False), (5003, 128, "contig", True), (4099, 1024, "contig", True), (1001, 3, "contig", True)]


@pytest.mark.parametrize("M,C,layout,hard", STATS_CASES)
def test_bn_stats_finalize(M, C, layout, hard):
    """upr_t_bn_stats + upr_t_bn_finalize: the fp64 sums, mean, invstd, the
    running statistics (unbiased variance, momentum), num_batches_tracked + 1;
    the same input twice gives the same bits."""
    _, lib, st = _lib()
    d = _inputs(M, C, hard)
    xw, cs, coff = _wide(d["x"], layout, fill=3e4)  # a leak from a neighbouring channel would show
    rm0, rv0 = _running0(d, C)
    acc, mean, inv, rm, rv, nbt = _run_stats(lib, st, xw, M, C, cs, coff, rm0, rv0)
    x64 = _np(d["x"])
    # any order of fp64 additions is within M * 2^-53 * sum|terms| of the exact sum
    for k, terms in ((0, x64), (1, x64 * x64)):
        err = np.abs(_np(acc[k * C:(k + 1) * C]) - terms.sum(axis=0))
        assert (err <= M * 2.0 ** -53 * np.abs(terms).sum(axis=0)).all(), f"acc[{k}]"
    cancel = M * 2.0 ** -53 * float(np.max(d["mean64"] ** 2 / d["var64"])) if hard else 0.0
    rm64, rv64 = O.bn_running(_np(rm0), _np(rv0), d["mean64"], d["var64"], M, MOM)
    tag = f"M{M} C{C} {layout}{' hard' if hard else ''}"
    _within_ulp(f"mean {tag}", mean, d["mean64"])
    _within_ulp(f"invstd {tag}", inv, d["invstd64"], extra_rel=cancel)
    _within_ulp(f"running_mean {tag}", rm, rm64)
    _within_ulp(f"running_var {tag}", rv, rv64)
    assert int(nbt) == 42
    if reduce_is_two_stage(C, cs, coff):
        again = _run_stats(lib, st, xw, M, C, cs, coff, rm0, rv0)
        for a, b in zip((acc, mean, inv, rm, rv), again):
            assert torch.equal(a, b), "bn_stats is not deterministic run to run"


def reduce_is_two_stage(C, cs, coff):
    """The slotted two-stage reduction (deterministic) takes C % 4 == 0, C <=
    1024 and 16-byte aligned rows; the atomic single-stage form takes the rest."""
    return C % 4 == 0 and C <= 1024 and cs % 4 == 0 and coff % 4 == 0


@pytest.mark.parametrize("C", [3, 64, 1028])
def test_bn_eval_stats(C):
    _, lib, st = _lib()
    gen = torch.Generator().manual_seed(C)
    rm, rv = torch.randn(C, generator=gen), 0.01 + 3 * torch.rand(C, generator=gen)
    mean, inv = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    assert lib.upr_t_bn_eval_stats(P(rm.to(DEV)), P(rv.to(DEV)), C, EPS, P(mean), P(inv), st) == 0
    torch.cuda.synchronize()
    m64, i64 = O.bn_eval_stats(_np(rm), _np(rv), EPS)
    assert torch.equal(mean.cpu(), rm) and np.array_equal(m64, _np(rm))
    _within_ulp(f"eval invstd C{C}", inv, i64)


# ---------------------------------------------------------------------------
# forward apply, fp32
# ---------------------------------------------------------------------------
APPLY_CASES = [
    # M, C, layout of x / y / res, residual, relu, hard
    (17, 32, "contig", "none", 0, False),
    (2, 64, "contig", "pre", 1, False),
    (301, 4, "contig", "post", 1, False),
    (301, 4, "slice4", "none", 1, False),
    (1923, 64, "contig", "post", 0, False),
    (1923, 64, "slice8", "pre", 1, False),
    (1991, 128, "slice4", "post", 1, False),
    (1991, 128, "off1", "pre", 0, False),
    (5003, 128, "contig", "none", 1, True),
    (4099, 1024, "contig", "pre", 1, False),
    (2003, 12, "contig", "none", 0, False),
    (2003, 12, "slice4", "post", 1, False),
    (1537, 96, "slice8", "pre", 0, False),
    (1537, 96, "contig", "post", 1, True),
    (811, 160, "contig", "pre", 1, False),
    (811, 160, "off1", "post", 1, False),
    (1001, 3, "contig", "post", 1, False),
    (1001, 3, "slice4", "none", 0, False),
    (515, 6, "contig", "pre", 1, False),
    (515, 6, "off1", "none", 1, True),
    (40, 1028, "contig", "post", 1, False),  # C > 1024: only the reductions refuse it
]


@pytest.mark.parametrize("M,C,layout,resmode,relu,hard", APPLY_CASES)
def test_bn_apply(M, C, layout, resmode, relu, hard):
    """upr_t_bn_apply and upr_t_bn_apply16: y = [relu](bn(x) + res_pre) +
    res_post, x / y / res contiguous or channel slices of wider buffers whose
    other channels must stay untouched; y16 == y.half() where the vector layout
    allows the fp16 copy, UPR_ERR_ARG where it does not."""
    L, lib, st = _lib()
    d = _inputs(M, C, hard)
    xw, cs, coff = _wide(d["x"], layout, fill=3e4)
    res = None if resmode == "none" else d["res"]
    rw = _wide(res, layout, fill=3e4)[0] if res is not None else None
    par = [d[k].to(DEV) for k in ("mean", "invstd", "gamma", "beta")]
    ref = O.bn_apply(_np(d["x"]), *[_np(d[k]) for k in ("mean", "invstd", "gamma", "beta")],
                     None if res is None else _np(res), resmode == "post", bool(relu))
    rs = _apply32(d["x"], d["mean"], d["invstd"], d["gamma"], d["beta"], res, resmode == "post", bool(relu))
    yw = torch.full((M, cs), SENT, device=DEV)
    assert lib.upr_t_bn_apply(P(xw), M, C, cs, coff, *map(P, par), P(rw), cs, coff, int(resmode == "post"), relu,
                              P(yw), cs, coff, st) == 0
    torch.cuda.synchronize()
    tag = f"M{M} C{C} {layout} res={resmode} relu={relu}{' hard' if hard else ''}"
    _untouched(yw, coff, C, "bn_apply")
    _within_restated(f"y {tag}", _slice(yw, coff, C), ref, rs, per_channel=True)
    # the fp16 copy
    yw2 = torch.full((M, cs), SENT, device=DEV)
    y16 = torch.full((M, C), SENT, dtype=torch.float16, device=DEV)
    rc = lib.upr_t_bn_apply16(P(xw), M, C, cs, coff, *map(P, par), P(rw), cs, coff, int(resmode == "post"), relu,
                              P(yw2), cs, coff, P(y16), st)
    torch.cuda.synchronize()
    if C % 4 == 0 and cs % 4 == 0 and coff % 4 == 0:
        assert rc == 0
        assert torch.equal(yw2, yw), "bn_apply16's y differs from bn_apply's"
        assert torch.equal(y16, _slice(yw, coff, C).half()), "y16 != y.half()"
    else:
        assert rc == L.UPR_ERR_ARG  # the fp16 copy needs the vectorised layout
        assert torch.equal(y16, torch.full_like(y16, SENT)) and torch.equal(yw2, torch.full_like(yw2, SENT))


# ---------------------------------------------------------------------------
# forward, fp16 operand
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,C,hard", [(M, C, False) for M, C in SHAPES4] + [(5003, 128, True)])
def test_bn_stats_fp16_bitwise(M, C, hard):
    """upr_t_bn_stats16 and upr_t_bn_stats16_fin on x16 equal upr_t_bn_stats +
    upr_t_bn_finalize fed x16.float() bit for bit: acc, mean, invstd, the
    running statistics, num_batches_tracked."""
    _, lib, st = _lib()
    d = _inputs(M, C, hard)
    x16 = d["x"].half().to(DEV)
    rm0, rv0 = _running0(d, C)
    want = _run_stats(lib, st, x16.float(), M, C, C, 0, rm0, rv0)
    acc = torch.full((lib.upr_t_reduce_acc_doubles(C),), 1e300, dtype=torch.float64, device=DEV)
    assert lib.upr_t_bn_stats16(P(x16), M, C, P(acc), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(acc[:2 * C], want[0]), "bn_stats16 acc"
    acc.fill_(1e300)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    nbt = torch.tensor(41, dtype=torch.int64, device=DEV)
    mean, inv = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    assert lib.upr_t_bn_stats16_fin(P(x16), M, C, P(acc), MOM, EPS, P(rm), P(rv), P(nbt), P(mean), P(inv), st) == 0
    torch.cuda.synchronize()
    for name, a, b in zip(("acc", "mean", "invstd", "running_mean", "running_var", "nbt"),
                          (acc[:2 * C], mean, inv, rm, rv, nbt), want):
        assert torch.equal(a, b), f"bn_stats16_fin {name}"


APPLY16_CASES = [
    # M, C, layout of y / res, residual, relu
    (17, 32, "contig", "none", 1),
    (2, 64, "slice4", "post", 1),
    (301, 4, "contig", "pre", 0),
    (1923, 64, "slice8", "none", 1),
    (1991, 128, "contig", "post", 1),
    (4099, 1024, "contig", "none", 0),
    (2003, 12, "slice4", "pre", 1),
    (1537, 96, "contig", "post", 0),
    (811, 160, "slice8", "none", 1),
    (40, 1028, "contig", "pre", 1),
]
APPLY16_CASES = [c + (False,) for c in APPLY16_CASES] + [(5003, 128, "contig", "post", 1, True)]


@pytest.mark.parametrize("M,C,layout,resmode,relu,hard", APPLY16_CASES)
def test_bn_apply_fp16_bitwise(M, C, layout, resmode, relu, hard):
    """upr_t_bn_apply16h / _apply16h_cs on x16 equal upr_t_bn_apply16 fed
    x16.float() bit for bit (y and y16 == y.half()); skip32 gives the same y16
    and leaves the fp32 buffer alone; a y16 channel slice (y16_cs > C) leaves
    the wide fp16 copy's other channels alone."""
    _, lib, st = _lib()
    d = _inputs(M, C, hard)
    x16 = d["x"].half().to(DEV)
    xf = x16.float()
    res = None if resmode == "none" else d["res"]
    rw = _wide(res, layout, fill=3e4)[0] if res is not None else None
    extra, coff = LAYOUTS[layout]
    cs = C + extra
    dev = [d[k].to(DEV) for k in ("mean", "invstd", "gamma", "beta")]
    par = [P(t) for t in dev]
    tail = (P(rw), cs, coff, int(resmode == "post"), relu)
    y_ref = torch.full((M, cs), SENT, device=DEV)
    assert lib.upr_t_bn_apply16(P(xf), M, C, C, 0, *par, *tail, P(y_ref), cs, coff, None, st) == 0
    y = torch.full((M, cs), SENT, device=DEV)
    y16 = torch.full((M, C), SENT, dtype=torch.float16, device=DEV)
    assert lib.upr_t_bn_apply16h(P(x16), M, C, *par, *tail, P(y), cs, coff, P(y16), 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, y_ref), "bn_apply16h y != bn_apply16(x16.float())"
    _untouched(y, coff, C, "bn_apply16h")
    assert torch.equal(y16, _slice(y, coff, C).half()), "y16 != y.half()"
    # skip32: the same y16, the fp32 buffer untouched
    y_s = torch.full((M, cs), SENT, device=DEV)
    y16_s = torch.full((M, C), SENT, dtype=torch.float16, device=DEV)
    assert lib.upr_t_bn_apply16h(P(x16), M, C, *par, *tail, P(y_s), cs, coff, P(y16_s), 1, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(y16_s, y16), "skip32 changed y16"
    assert torch.equal(y_s, torch.full_like(y_s, SENT)), "skip32 wrote the fp32 output"
    # y16 as a channel slice of a wider fp16 copy
    for c16 in (4, 8):
        wide16 = torch.full((M, C + 12), SENT, dtype=torch.float16, device=DEV)
        y_c = torch.full((M, cs), SENT, device=DEV)
        assert lib.upr_t_bn_apply16h_cs(P(x16), M, C, *par, *tail, P(y_c), cs, coff, P(wide16, c16), C + 12, 0,
                                        st) == 0
        torch.cuda.synchronize()
        assert torch.equal(y_c, y_ref)
        assert torch.equal(_slice(wide16, c16, C), y16), "y16 slice"
        _untouched(wide16, c16, C, "bn_apply16h_cs y16")


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------
def _device_mask(lib, st, d, M, C, x_dev=None):
    """y > 0 from the device forward's own fp32 relu(bn(x)) (contiguous)."""
    x = d["x"].to(DEV) if x_dev is None else x_dev
    par = [d[k].to(DEV) for k in ("mean", "invstd", "gamma", "beta")]
    y = torch.empty((M, C), device=DEV)
    assert lib.upr_t_bn_apply(P(x), M, C, C, 0, *map(P, par), None, 0, 0, 0, 1, P(y), C, 0, st) == 0
    torch.cuda.synchronize()
    return y


def _grads0(C):
    """dgamma / dbeta before the call: non-zero, they are always accumulated."""
    return torch.linspace(1, 2, C), torch.linspace(-2, -1, C)


BWD_CASES = [
    # M, C, layout of g / x / dx, batch_stats, accumulate, relu, hard
    (17, 32, "contig", 1, 0, 0, False),
    (17, 32, "slice4", 0, 1, 1, False),
    (2, 64, "contig", 1, 1, 1, False),
    (301, 4, "contig", 1, 0, 1, False),
    (1923, 64, "contig", 1, 1, 0, False),
    (1923, 64, "slice8", 1, 0, 1, False),
    (1923, 64, "off1", 1, 1, 1, False),
    (1991, 128, "slice4", 1, 1, 1, False),
    (1991, 128, "contig", 0, 0, 0, False),
    (5003, 128, "contig", 1, 0, 1, True),
    (4099, 1024, "contig", 1, 0, 1, False),
    (67003, 256, "contig", 1, 0, 1, False),
    (2003, 12, "contig", 1, 1, 1, False),
    (2003, 12, "slice4", 0, 0, 1, False),
    (1537, 96, "slice8", 1, 0, 0, False),
    (1537, 96, "contig", 1, 1, 1, True),
    (811, 160, "contig", 1, 0, 1, False),
    (811, 160, "off1", 0, 1, 0, False),
    (1001, 3, "contig", 1, 0, 1, False),
    (1001, 3, "slice4", 1, 1, 0, False),
    (515, 6, "contig", 0, 1, 1, False),
    (515, 6, "off1", 1, 0, 1, True),
]


@pytest.mark.parametrize("M,C,layout,batch_stats,accumulate,relu,hard", BWD_CASES)
def test_bn_backward(M, C, layout, batch_stats, accumulate, relu, hard):
    """upr_t_bn_bwd_reduce + upr_t_bn_bwd_apply (after upr_t_relu_mask when
    relu) and upr_t_bn_bwd_fused against the float64 backward: dx (fresh or
    added to a random dx), dgamma / dbeta added to non-zero values; g / x / dx
    contiguous or channel slices.  The fused ReLU fold equals relu_mask + the
    relu = 0 call bit for bit; the fused call is deterministic run to run and,
    where it takes the layout, equals the two separate calls bit for bit.  Off
    the vector layout it returns UPR_ERR_UNSUPPORTED and writes nothing."""
    L, lib, st = _lib()
    d = _inputs(M, C, hard)
    extra, coff = LAYOUTS[layout]
    cs = C + extra
    dg0, db0 = _grads0(C)
    dx0 = d["dx0"] if accumulate else None
    y_dev = _device_mask(lib, st, d, M, C) if relu else None
    mask = (y_dev > 0).cpu() if relu else None
    p64 = [_np(d[k]) for k in ("mean", "invstd", "gamma")]
    dx64, dg64, db64, _ = O.bn_bwd(_np(d["g"]), _np(d["x"]), *p64, bool(batch_stats),
                                   None if mask is None else mask.numpy(),
                                   None if dx0 is None else _np(dx0), _np(dg0), _np(db0))
    rs = _bwd32(d["g"], d["x"], d["mean"], d["invstd"], d["gamma"], bool(batch_stats),
                None if mask is None else mask.float(), dx0, dg0, db0)
    mean, inv, gamma, beta = [d[k].to(DEV) for k in ("mean", "invstd", "gamma", "beta")]
    xw = _wide(d["x"], layout, fill=3e4)[0]
    nacc = lib.upr_t_reduce_acc_doubles(C)
    tag = f"M{M} C{C} {layout} bs={batch_stats} acc={accumulate} relu={relu}{' hard' if hard else ''}"

    def new_out():
        dxw = _wide(dx0 if accumulate else torch.full((M, C), SENT), layout)[0]
        return dxw, dg0.to(DEV), db0.to(DEV)

    def check(name, out):
        dxw, dg, db = out
        _untouched(dxw, coff, C, name)
        _within_restated(f"dx {name} {tag}", _slice(dxw, coff, C), dx64, rs[0], per_channel=True)
        _within_restated(f"dgamma {name} {tag}", dg, dg64, rs[1])
        _within_restated(f"dbeta {name} {tag}", db, db64, rs[2])

    # the two separate kernels (the ReLU as its own mask pass over g)
    gw = _wide(d["g"], layout, fill=3e4)[0]
    if relu:
        assert lib.upr_t_relu_mask(P(gw), cs, coff, P(y_dev), C, 0, M, C, st) == 0
    acc = torch.zeros(nacc, dtype=torch.float64, device=DEV)  # zeroed: the atomic form adds
    sep = new_out()
    assert lib.upr_t_bn_bwd_reduce(P(gw), cs, coff, P(xw), cs, coff, P(mean), P(inv), M, C, P(acc), st) == 0
    assert lib.upr_t_bn_bwd_apply(P(gw), cs, coff, P(xw), cs, coff, P(mean), P(inv), P(gamma), P(acc), M, C,
                                  P(sep[1]), P(sep[2]), P(sep[0]), cs, coff, accumulate, batch_stats, st) == 0
    torch.cuda.synchronize()
    _untouched(gw, coff, C, "relu_mask", fill=3e4)
    check("reduce+apply", sep)
    if (M, C) != BIG:
        # the fp64 sums themselves: any summation order is within M * 2^-53 * sum|terms| of
        # the exact sum; x-hat is the kernels' fp32 (x - mean) * invstd, the products are exact in fp64
        gm = _np(d["g"]) * (mask.numpy() if relu else 1.0)
        xh32 = _np((d["x"] - d["mean"]) * d["invstd"])
        for k, terms in ((0, gm), (1, gm * xh32)):
            err = np.abs(_np(acc[k * C:(k + 1) * C]) - terms.sum(axis=0))
            assert (err <= M * 2.0 ** -53 * np.abs(terms).sum(axis=0)).all(), f"bn_bwd_reduce acc[{k}]"

    # the fused entry (x has no offset argument: the pointer carries it)
    def fused(g_buf, relu_flag):
        out = new_out()
        a = torch.full((nacc,), 1e300, dtype=torch.float64, device=DEV)  # scratch: zeroed by the entry
        rc = lib.upr_t_bn_bwd_fused(P(g_buf), cs, coff, P(xw, coff), cs, P(mean), P(inv), P(gamma), P(beta),
                                    relu_flag, M, C, P(a), P(out[1]), P(out[2]), P(out[0]), cs, coff, accumulate,
                                    batch_stats, None, st)
        torch.cuda.synchronize()
        return rc, out

    g_plain = _wide(d["g"], layout, fill=3e4)[0]
    rc, fu = fused(g_plain, relu)
    if not reduce_is_two_stage(C, cs, coff):
        assert rc == L.UPR_ERR_UNSUPPORTED
        first = new_out()
        for a, b in zip(fu, first):
            assert torch.equal(a, b), "a refused call wrote"
        return
    assert rc == 0
    check("fused", fu)
    for a, b in zip(fu, sep):
        assert torch.equal(a, b), "bn_bwd_fused differs from bn_bwd_reduce + bn_bwd_apply"
    rc, fu2 = fused(g_plain, relu)
    assert rc == 0
    for a, b in zip(fu, fu2):
        assert torch.equal(a, b), "bn_bwd_fused is not deterministic run to run"
    if relu:
        rc, fm = fused(gw, 0)  # gw: g masked by relu_mask above
        assert rc == 0
        for a, b in zip(fu, fm):
            assert torch.equal(a, b), "fused ReLU fold differs from relu_mask + the relu = 0 call"


BWD16_CASES = [
    # M, C, layout of g (fp32 form) / dx, batch_stats, accumulate, relu
    (17, 32, "contig", 1, 0, 1),
    (2, 64, "slice4", 1, 1, 0),
    (301, 4, "contig", 0, 0, 1),
    (1923, 64, "slice8", 1, 1, 1),
    (1991, 128, "contig", 1, 0, 1),
    (4099, 1024, "contig", 1, 0, 0),
    (67003, 256, "contig", 1, 0, 1),
    (2003, 12, "slice4", 1, 0, 1),
    (1537, 96, "contig", 1, 1, 1),
    (811, 160, "contig", 0, 0, 0),
]
BWD16_CASES = [c + (False,) for c in BWD16_CASES] + [(5003, 128, "contig", 1, 0, 1, True)]


@pytest.mark.parametrize("M,C,layout,batch_stats,accumulate,relu,hard", BWD16_CASES)
def test_bn_backward_fp16_bitwise(M, C, layout, batch_stats, accumulate, relu, hard):
    """upr_t_bn_bwd_fused16 (x16, g fp32 or g16) equals upr_t_bn_bwd_fused on
    the widened operands bit for bit (dx, dgamma, dbeta), itself within the
    float64 bound; dx16 == dx.half() from both entries; skip32 gives the same
    dx16 and parameter gradients and leaves the fp32 dx alone."""
    _, lib, st = _lib()
    d = _inputs(M, C, hard)
    extra, coff = LAYOUTS[layout]
    cs = C + extra
    x16 = d["x"].half().to(DEV)
    xf = x16.float()
    g16 = d["g"].half().to(DEV)
    dg0, db0 = _grads0(C)
    dx0 = d["dx0"] if accumulate else None
    mean, inv, gamma, beta = [d[k].to(DEV) for k in ("mean", "invstd", "gamma", "beta")]
    nacc = lib.upr_t_reduce_acc_doubles(C)

    def new_out():
        dxw = _wide(dx0 if accumulate else torch.full((M, C), SENT), layout)[0]
        return [dxw, dg0.to(DEV), db0.to(DEV), torch.full((M, C), SENT, dtype=torch.float16, device=DEV)]

    def run(entry, g_cpu, use_g16=False, skip32=0):
        out = new_out()
        a = torch.full((nacc,), 1e300, dtype=torch.float64, device=DEV)
        if use_g16:
            g_args, gw = (None, P(g16), 0, 0), None
        else:
            gw = _wide(g_cpu, layout, fill=3e4)[0]
            g_args = (P(gw), None, cs, coff)
        common = (P(mean), P(inv), P(gamma), P(beta), relu, M, C, P(a), P(out[1]), P(out[2]), P(out[0]), cs, coff,
                  accumulate, batch_stats, P(out[3]))
        if entry == "fused":
            rc = lib.upr_t_bn_bwd_fused(g_args[0], cs, coff, P(xf), C, *common, st)
        else:
            rc = lib.upr_t_bn_bwd_fused16(*g_args, P(x16), *common, skip32, st)
        torch.cuda.synchronize()
        assert rc == 0, (entry, rc)
        return out

    for use_g16 in (False, True):
        g_cpu = g16.float().cpu() if use_g16 else d["g"]
        want = run("fused", g_cpu)
        got = run("fused16", g_cpu, use_g16)
        for name, a, b in zip(("dx", "dgamma", "dbeta", "dx16"), got, want):
            assert torch.equal(a, b), f"bn_bwd_fused16 {name} != bn_bwd_fused on the widened operands (g16={use_g16})"
        assert torch.equal(got[3], _slice(got[0], coff, C).half()), "dx16 != dx.half()"
        _untouched(got[0], coff, C, "bn_bwd_fused16")
        if not accumulate:
            sk = run("fused16", g_cpu, use_g16, skip32=1)
            assert torch.equal(sk[3], got[3]), "skip32 changed dx16"
            assert torch.equal(sk[1], got[1]) and torch.equal(sk[2], got[2]), "skip32 changed dgamma / dbeta"
            assert torch.equal(sk[0], torch.full_like(sk[0], SENT)), "skip32 wrote the fp32 dx"
    if (M, C) == BIG:
        return  # (the fp32 entry it equals is measured on this shape in test_bn_backward)
    # the widened-operand result itself against float64 (g fp32, x = x16.float())
    y_dev = _device_mask(lib, st, d, M, C, xf) if relu else None
    mask = (y_dev > 0).cpu() if relu else None
    x_cpu = xf.cpu()
    dx64, dg64, db64, _ = O.bn_bwd(_np(d["g"]), _np(x_cpu), *[_np(d[k]) for k in ("mean", "invstd", "gamma")],
                                   bool(batch_stats), None if mask is None else mask.numpy(),
                                   None if dx0 is None else _np(dx0), _np(dg0), _np(db0))
    rs = _bwd32(d["g"], x_cpu, d["mean"], d["invstd"], d["gamma"], bool(batch_stats),
                None if mask is None else mask.float(), dx0, dg0, db0)
    got = run("fused16", d["g"])
    tag = f"M{M} C{C} {layout} bs={batch_stats} acc={accumulate} relu={relu}{' hard' if hard else ''}"
    _within_restated(f"dx fused16 {tag}", _slice(got[0], coff, C), dx64, rs[0], per_channel=True)
    _within_restated(f"dgamma fused16 {tag}", got[1], dg64, rs[1])
    _within_restated(f"dbeta fused16 {tag}", got[2], db64, rs[2])


# ---------------------------------------------------------------------------
# per-channel sums
# ---------------------------------------------------------------------------
SUM_CASES = [(M, C, "contig", k % 2) for k, (M, C) in enumerate(SHAPES)] + [
    (1991, 128, "slice4", 0), (1537, 96, "slice8", 1), (1923, 64, "off1", 1), (17, 32, "off1", 0), (515, 6, "slice4", 1),
    (5003, 128, "contig", 0), (17, 32, "contig", 1)]
SUM_CASES = [c + (False,) for c in SUM_CASES] + [(5003, 128, "contig", 0, True), (1001, 3, "contig", 1, True)]


@pytest.mark.parametrize("M,C,layout,accumulate,hard", SUM_CASES)
def test_chan_sums(M, C, layout, accumulate, hard):
    """upr_t_chan_sum, upr_t_chan_sum_ws (twice: deterministic), and on the
    fp16 copy upr_t_chan_sum16 / upr_t_chan_sum16s (a slice of a wider fp16
    buffer) against the float64 sum over rows, fresh or added to out; hard:
    the summed tensor is the mean = 100, sigma = 0.05 one."""
    L, lib, st = _lib()
    d = _inputs(M, C, hard)
    g = d["x"] if hard else d["g"]
    extra, coff = LAYOUTS[layout]
    cs = C + extra
    gw = _wide(g, layout, fill=3e4)[0]
    out0 = torch.linspace(-3, 3, C)
    ref = O.chan_sum(_np(g), _np(out0) if accumulate else None)
    rs = g.sum(0) + out0 if accumulate else g.sum(0)
    ws = torch.full((lib.upr_t_reduce_acc_doubles(C),), 1e300, dtype=torch.float64, device=DEV)
    tag = f"M{M} C{C} {layout} acc={accumulate}{' hard' if hard else ''}"

    def fresh():
        return out0.to(DEV) if accumulate else torch.full((C,), SENT, device=DEV)

    out = fresh()
    assert lib.upr_t_chan_sum(P(gw), M, C, cs, coff, P(out), accumulate, st) == 0
    torch.cuda.synchronize()
    _within_restated(f"chan_sum {tag}", out, ref, rs)
    outs = []
    for _ in range(2):
        out = fresh()
        assert lib.upr_t_chan_sum_ws(P(gw), M, C, cs, coff, P(out), accumulate, P(ws), st) == 0
        torch.cuda.synchronize()
        outs.append(out)
    _within_restated(f"chan_sum_ws {tag}", outs[0], ref, rs)
    if reduce_is_two_stage(C, cs, coff):
        assert torch.equal(outs[0], outs[1]), "chan_sum_ws is not deterministic run to run"
    # the fp16 copy: compact, and as the first channels of a wider fp16 buffer
    g16 = g.half()
    ref16 = O.chan_sum(_np(g16), _np(out0) if accumulate else None)
    rs16 = g16.float().sum(0) + out0 if accumulate else g16.float().sum(0)
    g16w = torch.full((M, C + 8), 3e4, dtype=torch.float16)
    g16w[:, 4:4 + C] = g16
    g16w, g16 = g16w.to(DEV), g16.to(DEV)
    out_a, out_b = fresh(), fresh()
    rc_a = lib.upr_t_chan_sum16(P(g16), M, C, P(out_a), accumulate, P(ws), st)
    rc_b = lib.upr_t_chan_sum16s(P(g16w, 4), M, C, C + 8, P(out_b), accumulate, P(ws), st)
    torch.cuda.synchronize()
    if C % 4:
        assert rc_a == rc_b == L.UPR_ERR_UNSUPPORTED
        assert torch.equal(out_a, fresh()) and torch.equal(out_b, fresh())
        return
    assert rc_a == 0 and rc_b == 0
    _within_restated(f"chan_sum16 {tag}", out_a, ref16, rs16)
    assert torch.equal(out_b, out_a), "chan_sum16s over a slice differs from chan_sum16 over the same values"


# ---------------------------------------------------------------------------
# documented refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1028, 6])
def test_bn_refusals(C):
    """C = 1028 (> 1024) and C % 4 != 0: the fused backward and every fp16
    reduction return UPR_ERR_UNSUPPORTED; skip32 without the fp16 copy, and
    skip32 with accumulate, return UPR_ERR_ARG.  Nothing is written."""
    L, lib, st = _lib()
    M = 8
    x = torch.full((M, C), SENT, device=DEV)
    x16 = torch.full((M, C + 8), SENT, dtype=torch.float16, device=DEV)
    out = torch.full((M, C), SENT, device=DEV)
    o16 = torch.full((M, C), SENT, dtype=torch.float16, device=DEV)
    vec = [torch.full((C,), SENT, device=DEV) for _ in range(8)]
    mean, inv, gamma, beta, dg, db, rm, rv = vec
    acc = torch.full((lib.upr_t_reduce_acc_doubles(C),), 1e300, dtype=torch.float64, device=DEV)
    nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
    U, A = L.UPR_ERR_UNSUPPORTED, L.UPR_ERR_ARG
    par = (P(mean), P(inv), P(gamma), P(beta))
    assert lib.upr_t_bn_bwd_fused(P(x), C, 0, P(x), C, *par, 1, M, C, P(acc), P(dg), P(db), P(out), C, 0, 0, 1,
                                  None, st) == U
    assert lib.upr_t_bn_bwd_fused16(P(x), None, C, 0, P(x16), *par, 1, M, C, P(acc), P(dg), P(db), P(out), C, 0, 0, 1,
                                    P(o16), 0, st) == U
    assert lib.upr_t_bn_bwd_fused16(None, P(x16), 0, 0, P(x16), *par, 0, M, C, P(acc), P(dg), P(db), P(out), C, 0, 0,
                                    1, P(o16), 0, st) == U
    assert lib.upr_t_bn_stats16(P(x16), M, C, P(acc), st) == U
    assert lib.upr_t_bn_stats16_fin(P(x16), M, C, P(acc), MOM, EPS, P(rm), P(rv), P(nbt), P(mean), P(inv), st) == U
    assert lib.upr_t_chan_sum16(P(x16), M, C, P(dg), 0, P(acc), st) == U
    assert lib.upr_t_chan_sum16s(P(x16), M, C, C + 8, P(dg), 0, P(acc), st) == U
    # argument errors come first, whatever C
    assert lib.upr_t_bn_apply16h(P(x16), M, C, *par, None, 0, 0, 0, 1, P(out), C, 0, None, 1, st) == A
    assert lib.upr_t_bn_apply16h_cs(P(x16), M, C, *par, None, 0, 0, 0, 1, P(out), C, 0, None, 0, 1, st) == A
    assert lib.upr_t_bn_apply16h_cs(P(x16), M, C, *par, None, 0, 0, 0, 1, P(out), C, 0, P(o16), C - 4, 0, st) == A
    assert lib.upr_t_bn_bwd_fused16(P(x), None, C, 0, P(x16), *par, 1, M, C, P(acc), P(dg), P(db), P(out), C, 0, 0, 1,
                                    None, 1, st) == A
    assert lib.upr_t_bn_bwd_fused16(P(x), None, C, 0, P(x16), *par, 1, M, C, P(acc), P(dg), P(db), P(out), C, 0, 1, 1,
                                    P(o16), 1, st) == A
    assert lib.upr_t_chan_sum16s(P(x16), M, C, C - 4, P(dg), 0, P(acc), st) == A
    torch.cuda.synchronize()
    for t in [x, out, *vec]:
        assert torch.equal(t, torch.full_like(t, SENT))
    assert torch.equal(o16, torch.full_like(o16, SENT)) and int(nbt) == 5
    assert torch.equal(acc, torch.full_like(acc, 1e300))


# ---------------------------------------------------------------------------
# through upr.train.BN (dispatch and fallbacks)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("amp", [False, True])
def test_bn_class_res_post_relu_accumulate(amp):
    """upr.train.BN.fwd(res, res_post=True, relu=True) then bwd(relu=True)
    into a non-fresh gx, in fp32 and under autocast with an input that
    carries its fp16 copy: y, dx (added to gx), dgamma / dbeta (added to
    non-zero grads), running statistics; under autocast also y16 == y.half()
    and dx16 == dx.half()."""
    from upr import train as T
    _, lib, st = _lib()
    B, H, W, C = 2, 13, 9, 64
    M = B * H * W
    d = _inputs(M, C)
    x = d["x"].half().float() if amp else d["x"]  # under autocast x is an fp16 conv's output
    m = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOM)
    rm0, rv0 = _running0(d, C)
    dg0, db0 = _grads0(C)
    with torch.no_grad():
        m.weight.copy_(d["gamma"])
        m.bias.copy_(d["beta"])
        m.running_mean.copy_(rm0)
        m.running_var.copy_(rv0)
    m = m.to(DEV).train()
    m.weight.grad, m.bias.grad = dg0.to(DEV), db0.to(DEV)
    # float64 reference and the fp32 restatement, statistics included
    x64 = _np(x)
    mean64, var64, inv64 = O.bn_stats(x64, EPS)
    rm64, rv64 = O.bn_running(_np(rm0), _np(rv0), mean64, var64, M, MOM)
    y64 = O.bn_apply(x64, mean64, inv64, _np(d["gamma"]), _np(d["beta"]), _np(d["res"]), True, True)
    mean32 = x.mean(0)
    inv32 = 1.0 / torch.sqrt(((x - mean32) ** 2).mean(0) + EPS)
    y32 = _apply32(x, mean32, inv32, d["gamma"], d["beta"], d["res"], True, True)
    T.set_amp(amp)
    try:
        bn = T.BN(m)
        xa = T.Act(x.view(B, H, W, C).to(DEV))
        if amp:
            xa.attach16(x.half().to(DEV).view(-1))
        ra = T.Act(d["res"].view(B, H, W, C).to(DEV))
        ya = bn.fwd(xa, relu=True, res=ra, res_post=True)
        torch.cuda.synchronize()
        _within_ulp(f"BN class mean amp={amp}", bn.mean, mean64)
        _within_ulp(f"BN class invstd amp={amp}", bn.invstd, inv64)
        _within_ulp(f"BN class running_mean amp={amp}", m.running_mean, rm64)
        _within_ulp(f"BN class running_var amp={amp}", m.running_var, rv64)
        assert int(m.num_batches_tracked) == 1
        _within_restated(f"BN class y amp={amp}", ya.t.view(M, C), y64, y32, per_channel=True)
        # the ReLU's mask: the device's own relu(bn(x)) from the statistics this forward made
        yr = torch.empty((M, C), device=DEV)
        assert lib.upr_t_bn_apply(xa.ptr().value, M, C, C, 0, P(bn.mean), P(bn.invstd), P(m.weight), P(m.bias), None,
                                  0, 0, 0, 1, P(yr), C, 0, st) == 0
        torch.cuda.synchronize()
        mask = (yr > 0).cpu()
        dx64, dg64, db64, _ = O.bn_bwd(_np(d["g"]), x64, mean64, inv64, _np(d["gamma"]), True, mask.numpy(),
                                       _np(d["dx0"]), _np(dg0), _np(db0))
        rs = _bwd32(d["g"], x, mean32, inv32, d["gamma"], True, mask.float(), d["dx0"], dg0, db0)
        ga = T.Act(d["g"].view(B, H, W, C).to(DEV))
        gx = T.Act(d["dx0"].view(B, H, W, C).to(DEV))  # not fresh: the backward adds
        bn.bwd(ga, gx, relu=True)
        torch.cuda.synchronize()
        _within_restated(f"BN class dx amp={amp}", gx.t.view(M, C), dx64, rs[0], per_channel=True)
        _within_restated(f"BN class dgamma amp={amp}", m.weight.grad, dg64, rs[1])
        _within_restated(f"BN class dbeta amp={amp}", m.bias.grad, db64, rs[2])
        if amp:
            ya16, gx16 = ya.compact16(), gx.compact16(grad=True)  # (the latter: only a copy marked as a gradient's)
            assert ya16 is not None and torch.equal(ya16.view(M, C), ya.t.view(M, C).half())
            assert gx16 is not None and torch.equal(gx16.view(M, C), gx.t.view(M, C).half())
            assert not ya.only16 and not gx.only16
    finally:
        T.set_amp(False)


# ---------------------------------------------------------------------------
# optimiser
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("betas,clip", [((0.9, 0.999), True), ((0.8, 0.95), True), ((0.9, 0.999), False)])
def test_adam_six_steps(betas, clip):
    """upr.optim.clip_grad_norm_ + Adam.step over 6 steps on 10 007 parameters
    (not a multiple of 256; several blocks), weight_decay 1e-2, fresh seeded
    gradients whose norm is above max_norm = 1 on odd steps and below it on
    even ones; clip = False: Adam.step with no preceding clip_grad_norm_.
    After every step p, m, v and the returned norm against the float64
    reference carried forward from the same fp32 start; the restatement is
    torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in fp32 on the CPU,
    carried forward the same way."""
    from upr import optim as UO
    n, lr, eps, wd, max_norm = 10007, 1e-3, 1e-8, 1e-2, 1.0
    gen = torch.Generator().manual_seed(77)
    p0 = torch.randn(n, generator=gen)
    pd = torch.nn.Parameter(p0.clone().to(DEV))
    opt = UO.Adam([pd], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    opt.zero_grad()
    pc = torch.nn.Parameter(p0.clone())
    ref_opt = torch.optim.Adam([pc], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    p, m, v = _np(p0), np.zeros(n), np.zeros(n)
    over = []
    for step in range(1, 7):
        g = torch.randn(n, generator=gen) * (0.02 if step % 2 else 0.002)  # |g| ~ 100 * the scale
        pd.grad.copy_(g)
        pc.grad = g.clone()
        norm_d = UO.clip_grad_norm_([pd], max_norm) if clip else None
        if clip:
            torch.nn.utils.clip_grad_norm_([pc], max_norm, foreach=False)
        opt.step()
        ref_opt.step()
        torch.cuda.synchronize()
        p, m, v, norm = O.adam_step(p, _np(g), m, v, step, lr, betas, eps, wd, max_norm if clip else None)
        tag = f"betas={betas} clip={clip} step {step}"
        if clip:
            over.append(norm > max_norm)
            _within_ulp(f"adam norm {tag}", norm_d.reshape(1), np.array([norm]))
        st = ref_opt.state[pc]
        _within_restated(f"adam p {tag}", pd.data, p, pc.data)
        _within_restated(f"adam m {tag}", opt.m[:n], m, st["exp_avg"])
        _within_restated(f"adam v {tag}", opt.v[:n], v, st["exp_avg_sq"])
        for t in (opt.flat.flat[n:], opt.m[n:], opt.v[n:]):  # the flat buffer's padding
            assert not t.any()
    if clip:
        assert over == [True, False] * 3


@pytest.mark.parametrize("scale", [65536.0, 1024.0, 0.5])
def test_unscale_exact_and_found_inf(scale):
    """upr_t_unscale over 10 007 values: g / scale exactly (the kernel
    multiplies by 1 / scale as GradScaler does; GradScaler's scales are
    powers of two -- 2^16 grown by 2, backed off by 0.5 -- for which that is
    fp32 division bit for bit); found_inf stays 0 on finite values and is set
    by one inf, by one nan, and by a finite value that overflows when
    unscaled."""
    _, lib, st = _lib()
    n = 10007
    gen = torch.Generator().manual_seed(5)
    base = torch.randn(n, generator=gen) * scale
    sc = torch.tensor([scale])
    cases = {"finite": (None, 0.0), "inf": (float("inf"), 1.0), "nan": (float("nan"), 1.0)}
    if scale < 1:
        cases["overflow"] = (3e38, 1.0)  # finite, 6e38 after the division is not
    for name, (special, want) in cases.items():
        g = base.clone()
        if special is not None:
            g[n - 3] = special
        want_g = g / sc
        assert want == float(not torch.isfinite(want_g).all())
        gd, found = g.to(DEV), torch.zeros(1, device=DEV)
        assert lib.upr_t_unscale(P(gd), n, P(sc.to(DEV)), P(found), st) == 0
        torch.cuda.synchronize()
        assert float(found) == want, name
        assert torch.equal(torch.nan_to_num(gd.cpu(), nan=12345.0), torch.nan_to_num(want_g, nan=12345.0)), name
