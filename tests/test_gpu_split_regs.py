"""fp32 convs split into fp16 (hi, lo) pairs in registers (UPR_FP32_SPLIT_REGS,
include/upr.h upr_conv2d_nhwc_regs / upr_model_op_forms) on the MI355X.

Tensors stay fp32; the row-ring kernel splits every 8-channel fragment after
its LDS read (hi = fp16(v), lo = fp16((v - hi) * 2^11)) and runs hi W_hi + hi
W_lo + (lo W_hi) 2^-11 on the fp16 MFMA unit with fp32 accumulation.  As in
test_gpu_split_conv.py the checks compare against float64 references and bound
the new form's error by 4x the fp32 MFMA path's error on the same inputs (a
CPU proxy of the arithmetic gives <= 1.4x; a broken split is off by 2^-11
relative, thousands of times; flushed fp16 subnormals show at scale 2^-12).
"""
import pytest
import torch

from conftest import has_gpu
from split_cases import DEV, REGION, RING_CASES, fwd, make_handle, make_sd, oracle_f64, regs_ops, ring_inputs

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]


# ---------------------------------------------------------------------------
# op level: the row ring (3x3, stride 1, pad 1, Cin 32)
# ---------------------------------------------------------------------------
SCALED = [(RING_CASES[1], 2.0 ** -12), (RING_CASES[1], 300.0)]  # (the table: split_cases.RING_CASES)


def run_ring_case(case, scale):
    from upr import runtime
    relu = case[4]
    x, w, b, r, refn = ring_inputs(case, scale)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    rd = r.permute(0, 2, 3, 1).contiguous().to(DEV) if r is not None else None
    wd, bd = runtime.pack_conv_weight(w).to(DEV), b.to(DEV)
    y32 = runtime.conv2d_nhwc(xd, wd, bd, 3, 3, 1, 1, 1, residual=rd, relu=relu)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    y16 = runtime.conv2d_nhwc_regs(xd, wd, bd, 3, 3, 1, 1, 1, residual=rd, relu=relu, overflow=ovf)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    e32 = (y32.double().cpu() - refn).abs().max().item()
    e16 = (y16.double().cpu() - refn).abs().max().item()
    print(f"split-regs conv {case} x{scale:g}: max|y| {refn.abs().max().item():.4g}  fp32 err {e32:.3e}  "
          f"regs err {e16:.3e}  ratio {e16 / max(e32, 1e-300):.2f}")
    return e16, e32


@pytest.mark.parametrize("case", RING_CASES)
def test_ring_regs_vs_f64(case):
    e16, e32 = run_ring_case(case, 1.0)
    assert e16 <= 4 * e32, f"split in registers {e16:.3e} vs fp32 path {e32:.3e}"


@pytest.mark.parametrize("case,scale", SCALED)
def test_ring_regs_scaled_activations(case, scale):
    e16, e32 = run_ring_case(case, scale)
    assert e16 <= 4 * e32, f"split in registers {e16:.3e} vs fp32 path {e32:.3e} at scale {scale}"


def test_regs_dtype_code_runs_the_same_kernel():
    """upr_conv2d_nhwc with dtype UPR_F32_SPLIT_REGS is the same launch (no overflow word)."""
    from upr import _lib as L
    from upr import runtime
    x, w, b, _, _ = ring_inputs(RING_CASES[1], 1.0)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd, bd = runtime.pack_conv_weight(w).to(DEV), b.to(DEV)
    y = runtime.conv2d_nhwc_regs(xd, wd, bd, 3, 3, 1, 1, 1, relu=True)
    y2 = torch.empty_like(y)
    B, H, W, Cin = xd.shape
    rc = L.lib().upr_conv2d_nhwc(xd.data_ptr(), B, H, W, Cin, wd.data_ptr(), bd.data_ptr(), 32, 3, 3, 1, 1, 1, None, 1,
                                 y2.data_ptr(), L.UPR_F32_SPLIT_REGS, None)
    torch.cuda.synchronize()
    assert rc == L.UPR_OK
    assert torch.equal(y, y2)


def test_regs_refuses_what_its_kernels_do_not_take():
    """No silent other kernel: 32 -> 64 with a residual (filter not register
    resident), a 1x1, and 64 input channels are UPR_ERR_UNSUPPORTED."""
    from upr import _lib as L
    lib = L.lib()
    x = torch.zeros(1, 8, 16, 64, device=DEV)
    w = torch.zeros(64 * 9 * 64, device=DEV)
    y = torch.zeros(1, 8, 16, 64, device=DEV)
    r = torch.zeros(1, 8, 16, 64, device=DEV)

    def call(cin, cout, k, pad, res):
        return lib.upr_conv2d_nhwc_regs(x.data_ptr(), 1, 8, 16, cin, w.data_ptr(), None, cout, k, k, 1, pad, 1,
                                        r.data_ptr() if res else None, 0, y.data_ptr(), None, None)

    assert call(32, 64, 3, 1, True) == L.UPR_ERR_UNSUPPORTED
    assert call(32, 32, 1, 0, False) == L.UPR_ERR_UNSUPPORTED
    assert call(64, 64, 3, 1, False) == L.UPR_ERR_UNSUPPORTED
    assert call(32, 64, 3, 1, False) == L.UPR_OK
    torch.cuda.synchronize()


def test_regs_overflow_word():
    """One input element outside the fp16 range sets the word; the plain input leaves it 0."""
    from upr import runtime
    x, w, b, _, _ = ring_inputs(RING_CASES[1], 1.0)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd, bd = runtime.pack_conv_weight(w).to(DEV), b.to(DEV)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    runtime.conv2d_nhwc_regs(xd, wd, bd, 3, 3, 1, 1, 1, relu=True, overflow=ovf)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    x2 = xd.clone()
    x2[1, 3, 17, 5] = 70000.0
    runtime.conv2d_nhwc_regs(x2, wd, bd, 3, 3, 1, 1, 1, relu=True, overflow=ovf)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 1


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 48, 80), (2, 64, 64)])
def test_model_regs_vs_exact(shape, monkeypatch):
    B, H, W = shape
    sd = make_sd(False, False)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(11))
    ref = oracle_f64(sd, x, False, False, shape)
    xd = x.to(DEV)
    h_on = make_handle(sd, False, False, monkeypatch, split=True, regs=True)
    h_noregs = make_handle(sd, False, False, monkeypatch, split=True, regs=False)
    h_off = make_handle(sd, False, False, monkeypatch, split=False, regs=True)
    assert h_on.split_state() == 1 and h_noregs.split_state() == 1 and h_off.split_state() == 0
    assert h_on.op_forms() == []
    on = fwd(h_on, xd)
    noregs = fwd(h_noregs, xd)
    off = fwd(h_off, xd)
    assert h_on.split_state() == 1
    for name, a, b, r in zip(("enhanced", "reflectance", "illumination"), on, off, ref):
        e_on = (a.double().cpu() - r).abs().max().item()
        e_off = (b.double().cpu() - r).abs().max().item()
        ulp16 = 16 * 2.0 ** -23 * r.abs().max().item()
        print(f"model {shape} {name}: err regs {e_on:.3e}  err exact {e_off:.3e}  16 ulp {ulp16:.3e}")
        assert e_on <= max(4 * e_off, ulp16), f"{name}: split in registers {e_on:.3e}, exact {e_off:.3e}"
    # which form every op ran in
    f_on, f_noregs, f_off = dict(h_on.op_forms()), dict(h_noregs.op_forms()), dict(h_off.op_forms())
    assert sorted(n for n, f in f_on.items() if f == 2) == regs_ops(H, W)
    assert sorted(n for n, f in f_on.items() if f == 1 and not n.endswith(".split_in")) == sorted(REGION)
    assert sorted(n for n, f in f_noregs.items() if f == 1 and not n.endswith(".split_in")) == sorted(REGION)
    assert 2 not in f_noregs.values()
    assert len(f_off) > 30 and set(f_off.values()) == {0}
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
    # the switch alone decides: REGS=0 is the previous split plan, not the exact one
    assert not all(torch.equal(a, b) for a, b in zip(noregs, off))


def test_overflow_in_a_regs_op_switches_to_exact_plan(monkeypatch):
    """An activation above 65504 read by a split-in-registers conv only (dec1's
    first BatchNorm scaled up feeds dec1.conv.3): that forward raises the flag,
    the next one runs the exact plan for good, bit-equal to UPR_FP32_SPLIT=0."""
    sd = make_sd(False, False, seed=4)
    sd["ie_net.dec1.conv.1.weight"] = sd["ie_net.dec1.conv.1.weight"] * 1.0e7
    xd = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(13)).to(DEV)
    h_on = make_handle(sd, False, False, monkeypatch, split=True, regs=True)
    h_off = make_handle(sd, False, False, monkeypatch, split=False, regs=True)
    assert h_on.split_state() == 1
    fwd(h_on, xd)
    second = fwd(h_on, xd)
    assert h_on.split_state() == 2
    assert set(dict(h_on.op_forms()).values()) == {0}
    for a, b in zip(second, fwd(h_off, xd)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("pre,dtype", [(True, torch.float32), (False, torch.float16)])
def test_other_models_untouched(pre, dtype, monkeypatch):
    """PreAct and fp16 models are bit-equal with the switch on and off and run every op in form 0."""
    sd = make_sd(pre, False, seed=3)
    xd = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(12)).to(DEV).to(dtype)
    h_on = make_handle(sd, pre, False, monkeypatch, dtype, split=True, regs=True)
    h_off = make_handle(sd, pre, False, monkeypatch, dtype, split=True, regs=False)
    for a, b in zip(fwd(h_on, xd), fwd(h_off, xd)):
        assert torch.equal(a, b)
    assert set(dict(h_on.op_forms()).values()) == {0}
    assert h_on.split_state() == 0
