"""fp32 convs of 64-wide output tiles on the fp16 MFMA unit with the weights
split once on the host (UPR_FP32_SPLIT_W64, include/upr.h upr_pack_split_w_f32 /
upr_conv2d_nhwc_wsplit, form 3 of upr_model_op_forms) on the MI355X.

Tensors stay fp32.  The 256-pixel x 64-channel gathered tile reads W_hi =
fp16(w s_n) and W_lo = fp16(w s_n - W_hi) ready-made, splits only its
activation fragments (hi = fp16(v), lo = fp16((v - hi) 2^11)) and accumulates
hi W_hi + hi W_lo + lo (W_hi 2^-11) in fp32.  As in test_gpu_split_regs.py the
checks compare against float64 references and bound the new form's error by 4x
the exact fp32 path's error on the same inputs (a correct split measures <=
1.5x; a broken one is off by 2^-11 relative, thousands of times; flushed fp16
subnormals show at scale 2^-12).
"""
import pytest
import torch

from conftest import has_gpu
from split_cases import DEV, REGION, WsplitCases, fwd, make_handle, make_sd, oracle_f64, regs_ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

# ---------------------------------------------------------------------------
# op level: each shape is the smallest that reaches one hazard of a 256-pixel x
# 64-channel tile with 32-deep K steps (3x3, pad 1)
# ---------------------------------------------------------------------------
CASES = {
    # B, H, W, Cin, Cout, stride, relu, residual (after the ReLU), second segment (H2, W2, C2, stride2)
    "one_partial_tile": (1, 8, 16, 32, 64, 1, False, False, None),
    "two_tiles_image_boundary": (2, 10, 24, 64, 64, 1, True, True, None),       # dec2.conv.3's flags
    "stride2": (2, 16, 24, 32, 64, 2, True, False, None),                       # enc1.conv1's form
    "shortcut_segment": (2, 9, 20, 64, 64, 1, True, False, (18, 40, 32, 2)),    # enc1.conv2: C = 64 then C = 32
    "two_n_tiles": (1, 8, 16, 64, 128, 1, False, False, None),
}

_W = WsplitCases(CASES, lambda B, H, W, Cin, Cout: 977 + 3 * H + 5 * W + Cin + 7 * Cout, "wsplit conv")
errors = _W.errors


def run_wsplit(name, scale, ovf=None, poke=None):
    return _W.run_wsplit(name, scale, ovf, poke)[0]


@pytest.mark.parametrize("name", list(CASES))
def test_wsplit_vs_f64(name):
    e16, e32 = errors(name, 1.0)
    assert e16 <= 4 * e32, f"weights split once {e16:.3e} vs fp32 path {e32:.3e}"


@pytest.mark.parametrize("scale", [2.0 ** -12, 300.0])
def test_wsplit_scaled_activations(scale):
    e16, e32 = errors("two_tiles_image_boundary", scale)
    assert e16 <= 4 * e32, f"weights split once {e16:.3e} vs fp32 path {e32:.3e} at scale {scale}"


def test_wsplit_overflow_word():
    """One input element outside the fp16 range sets the word; the plain input leaves it 0."""
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    run_wsplit("two_tiles_image_boundary", 1.0, ovf)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    run_wsplit("two_tiles_image_boundary", 1.0, ovf, poke=(1, 3, 17, 5))
    torch.cuda.synchronize()
    assert int(ovf.item()) == 1


def test_wsplit_refuses_what_its_kernel_does_not_take():
    """No silent other kernel: 16 input channels, 32 output channels and a blob
    packed for another shape are UPR_ERR_UNSUPPORTED."""
    from upr import _lib as L
    from upr import runtime
    lib = L.lib()
    x = torch.zeros(1, 8, 16, 64, device=DEV)
    y = torch.zeros(1, 8, 16, 64, device=DEV)
    blob = runtime.pack_split_w(torch.zeros(64, 9 * 64), 3, 3).to(DEV)     # 64 -> 64, 3x3
    blob32 = runtime.pack_split_w(torch.zeros(64, 9 * 32), 3, 3).to(DEV)   # 32 -> 64, 3x3

    def call(cin, cout, bl):
        return lib.upr_conv2d_nhwc_wsplit(x.data_ptr(), 1, 8, 16, cin, bl.data_ptr(), bl.numel(), None, cout, 3, 3, 1, 1,
                                          1, None, 0, y.data_ptr(), None, 0, 0, 0, 1, None, None)

    assert call(16, 64, blob) == L.UPR_ERR_UNSUPPORTED
    assert call(64, 32, blob) == L.UPR_ERR_UNSUPPORTED
    assert call(64, 64, blob32) == L.UPR_ERR_UNSUPPORTED
    assert call(32, 64, blob) == L.UPR_ERR_UNSUPPORTED
    assert call(64, 64, blob) == L.UPR_OK
    assert call(32, 64, blob32) == L.UPR_OK
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
W64 = ["ie_net." + n for n in ("enc1.conv1", "enc1.conv2", "dec2.conv.0", "dec2.conv.3")]


@pytest.mark.parametrize("shape", [(3, 48, 80), (2, 64, 64)])
def test_model_w64_vs_exact(shape, monkeypatch):
    B, H, W = shape
    sd = make_sd(False, False)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(11))
    ref = oracle_f64(sd, x, False, False, shape)
    xd = x.to(DEV)
    h_on = make_handle(sd, False, False, monkeypatch, split=True, regs=True, w64=True)
    h_now64 = make_handle(sd, False, False, monkeypatch, split=True, regs=True, w64=False)
    h_noregs = make_handle(sd, False, False, monkeypatch, split=True, regs=False, w64=True)
    h_off = make_handle(sd, False, False, monkeypatch, split=False, regs=True, w64=True)
    on, now64, noregs, off = fwd(h_on, xd), fwd(h_now64, xd), fwd(h_noregs, xd), fwd(h_off, xd)
    assert h_on.split_state() == 1
    for name, a, b, r in zip(("enhanced", "reflectance", "illumination"), on, off, ref):
        e_on = (a.double().cpu() - r).abs().max().item()
        e_off = (b.double().cpu() - r).abs().max().item()
        ulp16 = 16 * 2.0 ** -23 * r.abs().max().item()
        print(f"model {shape} {name}: err w64 {e_on:.3e}  err exact {e_off:.3e}  16 ulp {ulp16:.3e}")
        assert e_on <= max(4 * e_off, ulp16), f"{name}: weights split once {e_on:.3e}, exact {e_off:.3e}"
    # which form every op ran in
    f_on, f_now64, f_noregs, f_off = (dict(h.op_forms()) for h in (h_on, h_now64, h_noregs, h_off))
    assert sorted(n for n, f in f_on.items() if f == 3) == sorted(W64)
    assert sorted(n for n, f in f_on.items() if f == 2) == regs_ops(H, W)
    assert sorted(n for n, f in f_on.items() if f == 1 and not n.endswith(".split_in")) == sorted(REGION)
    # the switch keeps the four exact and leaves the rest of the plan alone; REGS=0 is the plan before both
    assert all(f_now64[n] == 0 for n in W64) and 3 not in f_now64.values()
    assert {n: f for n, f in f_now64.items() if n not in W64} == {n: f for n, f in f_on.items() if n not in W64}
    assert all(f_noregs[n] == 0 for n in W64) and not {2, 3} & set(f_noregs.values())
    assert len(f_off) > 30 and set(f_off.values()) == {0}
    assert not all(torch.equal(a, b) for a, b in zip(on, now64))
    # bit-equal over two forwards, and between the forked and the profiled (one-stream) forward
    again = fwd(h_on, xd)
    h_on.profile(True)
    serial = fwd(h_on, xd)
    h_on.profile_read()
    h_on.profile(False)
    for a, b, c in zip(on, again, serial):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert dict(h_on.op_forms()) == f_on
    assert h_on.split_state() == 1


def test_overflow_in_a_w64_op_switches_to_exact_plan(monkeypatch):
    """An activation above 65504 read by one weights-split-once conv only (dec2's
    first BatchNorm scaled up feeds dec2.conv.3, whose own BatchNorm, scaled down,
    brings the values back before dec1 reads them): that forward raises
    the flag, the next one runs the exact plan for good, bit-equal to UPR_FP32_SPLIT=0."""
    sd = make_sd(False, False, seed=4)
    sd["ie_net.dec2.conv.1.weight"] = sd["ie_net.dec2.conv.1.weight"] * 1.0e7
    sd["ie_net.dec2.conv.4.weight"] = sd["ie_net.dec2.conv.4.weight"] * 1.0e-7
    xd = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(13)).to(DEV)
    # only dec2.conv.3 reads the large values: with the four kept exact nothing overflows
    h_now64 = make_handle(sd, False, False, monkeypatch, split=True, regs=True, w64=False)
    fwd(h_now64, xd)
    fwd(h_now64, xd)
    assert h_now64.split_state() == 1
    h_on = make_handle(sd, False, False, monkeypatch, split=True, regs=True, w64=True)
    h_off = make_handle(sd, False, False, monkeypatch, split=False, regs=True, w64=True)
    assert h_on.split_state() == 1
    fwd(h_on, xd)
    assert dict(h_on.op_forms())["ie_net.dec2.conv.3"] == 3
    second = fwd(h_on, xd)
    assert h_on.split_state() == 2
    assert set(dict(h_on.op_forms()).values()) == {0}
    for a, b in zip(second, fwd(h_off, xd)):
        assert torch.equal(a, b)
