"""What tests/test_gpu_wgrad_ops.py relies on, checked without a device:

  * oracle.conv_ops.conv_wgrad against torch autograd in double (1e-12) at
    every (Cin, Cout, k, s, p, d) of wgrad_cases.wgrad_configs(), small H != W;
  * the split restatement of wgrad_cases.py against what the tables' notes
    claim (partial tails, 96 / 96 / 81, 4 / 4 / 2, row blocks 2 + 1, the long
    chain), and the typed tiles against the restated dispatch;
  * that the bound discriminates: _within_restated accepts the fp32
    restatement and rejects five wrong results built in float64 -> fp32,
      (a) zero padding applied per 64-column segment (halo cases, W 128),
      (b) two images treated as one image of height 2H,
      (c) the trailing P % 32 pixels dropped (fp32 cases with a tail),
      (d) the first pixel / unit / step of the second split counted twice,
      (e) dy left unrounded (fp16 cases).
The long-chain case takes part in (d) only (P % 32 == 0, one image)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as C
from op_parity import _within_restated
from oracle import conv_ops as O

REL = 1e-12


@pytest.mark.parametrize("Cin,Cout,k,s,p,d", C.wgrad_configs())
@pytest.mark.parametrize("B,H,W", [(2, 9, 12), (1, 14, 11)])
def test_oracle_wgrad_matches_autograd_double(Cin, Cout, k, s, p, d, B, H, W):
    rng = np.random.default_rng(1000 * Cin + 10 * Cout + k + s + p + d)
    Ho, Wo = O.out_size(H, k, s, p, d), O.out_size(W, k, s, p, d)
    assert Ho > 0 and Wo > 0
    x, dy = rng.standard_normal((B, H, W, Cin)), rng.standard_normal((B, Ho, Wo, Cout))
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))
    wt = torch.zeros((Cout, Cin, k, k), dtype=torch.float64, requires_grad=True)
    F.conv2d(xt, wt, None, s, p, d).backward(torch.from_numpy(np.ascontiguousarray(dy.transpose(0, 3, 1, 2))))
    dw, _ = O.conv_wgrad(x, dy, k, k, s, p, d)
    ref = wt.grad.numpy()
    assert dw.shape == ref.shape
    assert np.abs(dw - ref).max() <= REL * np.abs(ref).max()


def test_configs_cover_every_table():
    cfgs = set(C.wgrad_configs())
    assert len(cfgs) == 19
    for r in C.ALL_ROWS:
        assert tuple(r.case[3:]) in cfgs


# ---------------------------------------------------------------------------
# the restated split arithmetic against the tables' claims
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("r", C.ALL_ROWS, ids=lambda r: C.FAMILY[r.family] + "-" + "-".join(map(str, r.case)))
def test_typed_tile_is_the_restated_dispatch(r):
    plan = C.PLAN[r.family](r.case)
    assert tuple(plan["tile"]) == r.tile
    if r.family in (C.IM2COL16, C.HALO16):
        assert C.fp16_family(r.case) == r.family
    fam, t0, t1, t2, splits = C.route(r)
    assert (fam, t0, t1, t2) == (r.family,) + r.tile and splits >= 1


def _g(i):
    return C.gemm32_plan(C.GEMM32_ROWS[i].case)


def test_gemm32_claims():
    p = _g(0)
    assert (p["P"], p["KT"], p["splits"], p["ntiles"]) == (15, 32, 1, 1) and p["P"] < C.WG_KP
    p = _g(1)
    assert (p["P"], p["splits"], p["KT"], p["ntiles"]) == (35, 1, 288, 2) and p["P"] % C.WG_KP == 3
    assert p["KT"] - 256 == 32                       # the second n-tile has 32 valid columns
    p = _g(2)
    assert (p["P"], p["splits"], p["ntiles"], p["KT"] % 128) == (70, 1, 3, 32)
    assert 32 < 35 < 64                              # image 1 starts inside the second step
    p = _g(3)
    assert C.out_hw(C.GEMM32_ROWS[3].case) == (5, 6) and (p["ntiles"], p["KT"] % 64, p["mtiles"]) == (9, 0, 1)
    p = _g(4)
    assert (p["P"], p["sizes"]) == (273, [96, 96, 81]) and 81 % C.WG_KP == 17
    assert C.out_hw(C.GEMM32_ROWS[5].case) == (10, 10)
    assert _g(6)["mtiles"] == 3
    p = _g(7)
    assert (p["mtiles"], p["ntiles"]) == (2, 36)
    assert C.out_hw(C.GEMM32_ROWS[8].case) == (4, 6)
    for i in (9, 10):
        p = _g(i)
        assert p["ntiles"] == 1 and p["KT"] < 256
    p = C.gemm32_plan(C.LONG)
    assert p["sizes"] == [4096] * 15 and 34e6 < p["slab_bytes"] < 36e6
    # 4096 pixels a split is the longest chain of the bs 8 512^2 step (32 -> 32 at 512^2)
    assert C.gemm32_plan(C.Case(8, 512, 512, 32, 32, 3, 1, 1, 1))["pps"] == 4096
    # the layout rows are the second, fourth and fifth
    assert [C.GEMM32_ROWS[i].case[:3] for i in C.GEMM32_LAYOUT_ROWS] == [(1, 5, 7), (2, 9, 11), (1, 13, 21)]
    q = C.gemm32_plan(C.ROUTING_ROW.case)
    assert q["P"] == 192 and C.fp16_family(C.ROUTING_ROW.case) == C.GEMM32


def test_tap32_claims():
    assert [C.tap32_plan(r.case)["splits"] for r in C.TAP32_ROWS] == [1, 1, 1, 2]
    assert [C.tap32_plan(r.case)["P"] for r in C.TAP32_ROWS[2:]] == [1024, 1025]
    assert C.TAP32_ROWS[0].case == C.GEMM32_ROWS[1].case and C.TAP32_ROWS[1].case == C.GEMM32_ROWS[3].case


def test_im2col16_claims():
    plans = [C.im2col16_plan(r.case) for r in C.IM2COL16_ROWS]
    assert (plans[0]["units"], plans[0]["splits"]) == (3, 1)
    assert C.IM2COL16_ROWS[1].case.H % 8 == 4 and C.halo16_cfg(C.IM2COL16_ROWS[1].case) is None
    assert plans[2]["sizes"] == [4, 4, 2] and 4 < 5 < 8    # image 1 starts at unit 5, inside the second split
    assert C.out_hw(C.IM2COL16_ROWS[3].case) == (3, 64) and plans[3]["ntiles"] == 9
    assert C.out_hw(C.IM2COL16_ROWS[9].case) == (2, 64)
    assert C.out_hw(C.IM2COL16_ROWS[11].case) == (4, 64)
    assert plans[12]["ntiles"] == 2 and plans[13]["ntiles"] == 3
    assert [C.IM2COL16_ROWS[i].case[:5] for i in C.IM2COL16_LAYOUT_ROWS] == [(2, 5, 64, 32, 64), (2, 8, 64, 64, 64)]
    # the longest chain of the bs 8 512^2 step: 64 units a split where the shape has two n-tiles (32 with
    # one), so 128 MFMA accumulations an accumulator -- not the "about 18 units" the table was first
    # written with; against 2048 for the fp32 GEMM's 4096 pixels.  The table's own cases stop at 4 units;
    # IM2COL16_LONG is the cheapest shape with splits of 64.
    ups = [C.im2col16_plan(C.Case(8, 512, 512, cin, cout, 3, 1, 1, 1))["ups"] for cin, cout in ((64, 64), (32, 64), (64, 32))]
    assert ups == [64, 32, 64]
    assert max(max(p["sizes"]) for p in plans) == 4
    long = C.im2col16_plan(C.IM2COL16_LONG.case)
    assert long["sizes"] == [64] * 29 and long["tile"] == (128, 4, 0) and C.halo16_cfg(C.IM2COL16_LONG.case) is None
    assert {p["tile"][:2] for p in plans} == {(32, 9), (64, 9), (128, 2), (32, 8), (128, 4), (128, 1), (64, 1), (64, 2),
                                              (64, 4)}


def test_halo16_claims():
    plans = [C.halo16_plan(r.case) for r in C.HALO16_ROWS]
    assert [p["TR"] for p in plans] == [8, 8, 8, 4, 4, 4, 4, 4, 4]
    assert (plans[0]["spc"], plans[0]["segs"], plans[0]["splits"]) == (1, 1, 1)
    assert (plans[1]["segs"], plans[1]["splits"]) == (2, 2)
    for i in (2, 4, 6, 8):
        assert plans[i]["row_blocks"] == [2, 1] and plans[i]["splits"] == 8, i
    assert [C.HALO16_ROWS[i].case[:3] for i in C.HALO16_LAYOUT_ROWS] == [(2, 24, 128), (2, 12, 128)]
    assert {p["tile"] for p in plans} == {(32, 9, 1), (32, 9, 2), (96, 1, 0), (128, 1, 0)}
    # what the halo form declines: dilation 3, 64 channels, pad 0, a height off the row tile
    for i in (0, 1, 10, 11, 12):
        assert C.halo16_cfg(C.IM2COL16_ROWS[i].case) is None, i


def test_argument_checks_come_before_the_device():
    """The three entries refuse bad geometry and slices that leave their buffer
    without a device call (host pointers stand in; nothing reads them), and
    the query then reports that nothing ran."""
    import ctypes

    from upr import _lib as L
    lib = L.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    good = dict(B=1, H=5, W=7, Cin=32, x_cs=32, x_coff=0, dy=p, Ho=5, Wo=7, Cout=32, dy_cs=32, dy_coff=0, kh=3, kw=3,
                s=1, p=1, d=1)
    bad = [(dict(kh=0), L.UPR_ERR_ARG), (dict(s=0), L.UPR_ERR_ARG), (dict(d=0), L.UPR_ERR_ARG), (dict(p=-1), L.UPR_ERR_ARG),
           (dict(H=0), L.UPR_ERR_ARG), (dict(Wo=0), L.UPR_ERR_ARG), (dict(Cin=48), L.UPR_ERR_ARG),
           (dict(x_cs=28), L.UPR_ERR_ARG), (dict(x_coff=4), L.UPR_ERR_ARG), (dict(dy_cs=44, dy_coff=16), L.UPR_ERR_ARG),
           (dict(dy_coff=-4), L.UPR_ERR_ARG), (dict(Ho=6), L.UPR_ERR_SHAPE), (dict(Wo=6), L.UPR_ERR_SHAPE),
           (dict(kh=8, Ho=1), L.UPR_ERR_SHAPE)]
    ran = L.UprWgradRan()
    for over, want in bad:
        a = dict(good, **over)
        v = list(a.values())
        assert lib.upr_t_conv_wgrad(p, *v, p, None) == want, over
        assert lib.upr_t_conv_wgrad16(p, p, *v, p, None) == want, over
        i = list(a).index("Ho")
        assert lib.upr_t_conv_wgrad_into(p, p, *v[:i], p, *v[i:], p, None) == want, over
        assert lib.upr_t_conv_wgrad_ran(ctypes.byref(ran)) == 0
        assert (ran.kernel, ran.t0, ran.t1, ran.t2, ran.splits, ran.dy16) == (0, 0, 0, 0, 0, 0), over
    assert lib.upr_t_conv_wgrad_ran(None) == L.UPR_ERR_ARG


# ---------------------------------------------------------------------------
# the bound discriminates
# ---------------------------------------------------------------------------
def _pix_scale(c, dy, pixels, factor):
    """dy with the listed flat output pixels scaled (0: dropped, 2: counted twice)."""
    dy = dy.clone()
    dy.view(-1, c.Cout)[pixels] *= factor
    return dy


def _second_split_first(r):
    """Flat output pixels of the first pixel / unit / step of the second split, or None."""
    c = r.case
    Ho, Wo = C.out_hw(c)
    plan = C.PLAN[r.family](c)
    if plan["splits"] < 2:
        return None
    if r.family == C.GEMM32:
        return [plan["pps"]]
    if r.family == C.TAP32:
        return [C.WG_PPB]
    if r.family == C.IM2COL16:
        return list(range(plan["ups"] * 64, plan["ups"] * 64 + 64))
    # halo: splits are (image, row block, segment), segment fastest: the second split is segment 1 of
    # image 0 / row block 0 when there are two segments, else row block 1
    TR = plan["TR"]
    row0, col0 = (0, 64) if plan["segs"] > 1 else (plan["spb"] * TR, 0)
    return [(row0 + r_) * Wo + col0 + x_ for r_ in range(TR) for x_ in range(64)]


def _wrong_results(r, fp16):
    """name -> float64 dw0 + a wrongly computed gradient, on the kernel's operands."""
    c = r.case
    x, dy = C.kernel_operands(c, fp16)
    Ho, Wo = C.out_hw(c)
    P = c.B * Ho * Wo
    dw0 = C.operands(c)["dw0"].double().numpy()
    out = {}
    if r.family == C.HALO16 and c.W == 128 and c.k == 3:
        out["(a) padding per 64-column segment"] = dw0 + sum(
            C.dw64(c, x[:, :, s0:s0 + 64].contiguous(), dy[:, :, s0:s0 + 64].contiguous()) for s0 in (0, 64))
    if c.B == 2 and c.k > 1 and (Ho, Wo) == (c.H, c.W):
        out["(b) two images as one of height 2H"] = dw0 + C.dw64(c, x.reshape(1, 2 * c.H, c.W, c.Cin),
                                                                 dy.reshape(1, 2 * Ho, Wo, c.Cout))
    if r.family == C.GEMM32 and P % 32:
        out["(c) the trailing P % 32 pixels dropped"] = C.wgrad64(c, x, _pix_scale(c, dy, range(P - P % 32, P), 0.0))
    first = _second_split_first(r)
    if first is not None:
        out["(d) the second split's first unit twice"] = C.wgrad64(c, x, _pix_scale(c, dy, first, 2.0))
    if fp16:
        out["(e) dy left unrounded"] = C.wgrad64(c, x, C.operands(c)["dy"])
    return out


GROUPS = [(C.GEMM32_ROWS + [C.ROUTING_ROW], False), (C.TAP32_ROWS[2:], False), (C.IM2COL16_ROWS, True),
          (C.HALO16_ROWS, True)]
DISCRIMINATE = [(r, fp16) for rows, fp16 in GROUPS for r in rows]


@pytest.mark.parametrize("r,fp16", DISCRIMINATE,
                         ids=lambda v: C.FAMILY[v.family] + "-" + "-".join(map(str, v.case)) if isinstance(v, C.Row) else "")
def test_bound_discriminates(r, fp16):
    c = r.case
    ref, rst = C.references(c, fp16)
    tag = f"{C.FAMILY[r.family]} | {tuple(c)}"
    _within_restated(tag, rst, ref, rst)
    _within_restated(tag + " per channel", C.as_kc(rst, c.Cout), C.as_kc(ref, c.Cout), C.as_kc(rst, c.Cout),
                     per_channel=True)
    wrong = _wrong_results(r, fp16)
    for name, w64 in wrong.items():
        w32 = torch.from_numpy(w64.astype(np.float32))
        assert not torch.equal(w32, torch.from_numpy(ref.astype(np.float32))), name
        with pytest.raises(AssertionError):
            _within_restated(f"{tag} {name}", w32, ref, rst)
        with pytest.raises(AssertionError):
            _within_restated(f"{tag} {name} per channel", C.as_kc(w32, c.Cout), C.as_kc(ref, c.Cout),
                             C.as_kc(rst, c.Cout), per_channel=True)


def test_every_wrong_result_is_built_somewhere():
    """Each of (a)-(e) applies to at least one case of the group it is named for."""
    seen = {}
    for r, fp16 in DISCRIMINATE:
        if r.case == C.LONG:
            continue
        c = r.case
        Ho, Wo = C.out_hw(c)
        P = c.B * Ho * Wo
        seen.setdefault("a", []).append(r.family == C.HALO16 and c.W == 128 and c.k == 3)
        if r.family != C.TAP32:  # its two shapes of its own are single images
            seen.setdefault("b" + str(r.family), []).append(c.B == 2 and c.k > 1 and (Ho, Wo) == (c.H, c.W))
        seen.setdefault("c", []).append(r.family == C.GEMM32 and P % 32 != 0)
        seen.setdefault("d" + str(r.family), []).append(_second_split_first(r) is not None)
    for k, v in seen.items():
        assert any(v), k
    assert _second_split_first(C.GEMM32_ROWS[-1]) == [4096]
