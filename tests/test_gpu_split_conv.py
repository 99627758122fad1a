"""fp32 convs computed from split-fp16 operands (UPR_FP32_SPLIT, include/upr.h
upr_model_split_state / upr_split_f32) on the MI355X.

A split tensor stores v as hi = fp16(v), lo = fp16((v - hi) * 2^11).  The checks
here compare against float64 references and bound the split path's error by a
multiple of the fp32 MFMA path's error on the same inputs (4x: a CPU proxy of
the arithmetic gives <= 1.7x, and 2-3x if fp16 subnormal operands were flushed;
a broken split is off by 2^-11 relative, i.e. thousands of times).
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import has_gpu
from split_cases import DEV, fwd, make_handle, make_sd, oracle_f64

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]


# ---------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------
CONV_CASES = [
    # B, H, W, Cin, Cout, k, stride, pad, relu, residual
    (2, 12, 20, 128, 128, 3, 1, 1, True, True),    # M = 480: a partial tile, a tile spanning two images
    (1, 8, 16, 256, 256, 3, 1, 1, False, False),   # M = 128: less than one tile
    (3, 20, 28, 64, 128, 3, 2, 1, True, True),     # stride 2, M = 420
    (2, 8, 24, 256, 128, 3, 1, 1, False, True),    # residual without ReLU
]
# the first shape again at small and large activations (x, bias and residual all at that magnitude)
SCALED = [(CONV_CASES[0], 2.0 ** -12), (CONV_CASES[0], 300.0)]


def run_conv_case(case, scale):
    from upr import runtime
    B, H, W, Cin, Cout, k, s, p, relu, res = case
    g = torch.Generator().manual_seed(1234 + Cin + 7 * Cout + H)
    # ReLU'd normal activations, as the region's inputs are
    x = F.relu(torch.randn(B, Cin, H, W, generator=g)) * scale
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) * scale
    r = None
    ref = F.conv2d(x.double(), w.double(), b.double(), s, p)
    if res:
        r = torch.randn(ref.shape, generator=g) * scale
        ref = ref + r.double()
    if relu:
        ref = F.relu(ref)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    rd = r.permute(0, 2, 3, 1).contiguous().to(DEV) if res else None
    bd = b.to(DEV)
    y32 = runtime.conv2d_nhwc(xd, runtime.pack_conv_weight(w).to(DEV), bd, k, k, s, p, 1, residual=rd, relu=relu)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    ys = runtime.conv2d_split(runtime.split_f32(xd, ovf), runtime.pack_split_weight(w).to(DEV), Cout, bd, k, k, s, p, 1,
                              residual=runtime.split_f32(rd, ovf) if res else None, relu=relu)
    ysp = runtime.unsplit_f32(ys)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    refn = ref.permute(0, 2, 3, 1)
    e32 = (y32.double().cpu() - refn).abs().max().item()
    esp = (ysp.double().cpu() - refn).abs().max().item()
    print(f"split conv {case} x{scale:g}: max|y| {refn.abs().max().item():.4g}  fp32 err {e32:.3e}  "
          f"split err {esp:.3e}  ratio {esp / max(e32, 1e-300):.2f}")
    return esp, e32


@pytest.mark.parametrize("case", CONV_CASES)
def test_split_conv_vs_f64(case):
    esp, e32 = run_conv_case(case, 1.0)
    assert esp <= 4 * e32, f"split {esp:.3e} vs fp32 path {e32:.3e}"


@pytest.mark.parametrize("case,scale", SCALED)
def test_split_conv_scaled_activations(case, scale):
    esp, e32 = run_conv_case(case, scale)
    assert esp <= 4 * e32, f"split {esp:.3e} vs fp32 path {e32:.3e} at scale {scale}"


def test_split_round_trip_and_overflow_word():
    """unsplit(split(x)) == x to 2^-22 relative over the normal fp16 range of hi
    (|x| in [2^-14, 65504]); a value above 65504 sets the overflow word."""
    from upr import runtime
    g = torch.Generator().manual_seed(5)
    mag = torch.exp2(torch.rand(5, 9, 7, 64, generator=g, dtype=torch.float64) * 29.99 - 14.0).float()
    mag = mag.clamp(2.0 ** -14, 65504.0)
    x = (mag * torch.where(torch.rand(mag.shape, generator=g) < 0.5, -1.0, 1.0)).to(DEV)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    y = runtime.split_f32(x, ovf)
    back = runtime.unsplit_f32(y)
    torch.cuda.synchronize()
    assert y.shape == (5, 9, 7, 128) and y.dtype == torch.float16
    rel = ((back.double() - x.double()).abs() / x.double().abs()).max().item()
    print(f"split round trip: max relative error {rel:.3e} (bound {2.0 ** -22:.3e})")
    assert rel <= 2.0 ** -22
    assert int(ovf.item()) == 0
    x2 = x.clone()
    x2[3, 4, 5, 6] = 70000.0
    runtime.split_f32(x2, ovf)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 1


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 48, 80), (2, 64, 64)])
def test_model_split_vs_exact(shape, monkeypatch):
    B, H, W = shape
    sd = make_sd(False, False)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(11))
    ref = oracle_f64(sd, x, False, False, shape)
    xd = x.to(DEV)
    h_on = make_handle(sd, False, False, monkeypatch, split=True)
    h_off = make_handle(sd, False, False, monkeypatch, split=False)
    assert h_on.split_state() == 1 and h_off.split_state() == 0
    on = fwd(h_on, xd)
    off = fwd(h_off, xd)
    assert h_on.split_state() == 1
    for name, a, b, r in zip(("enhanced", "reflectance", "illumination"), on, off, ref):
        e_on = (a.double().cpu() - r).abs().max().item()
        e_off = (b.double().cpu() - r).abs().max().item()
        ulp16 = 16 * 2.0 ** -23 * r.abs().max().item()
        print(f"model {shape} {name}: err split {e_on:.3e}  err exact {e_off:.3e}  16 ulp {ulp16:.3e}")
        assert e_on <= max(4 * e_off, ulp16), f"{name}: split {e_on:.3e}, exact {e_off:.3e}"
    # bit-equal over two forwards, and between the forked and the profiled (one-stream) forward
    again = fwd(h_on, xd)
    assert h_on.forks() >= 1
    h_on.profile(True)
    serial = fwd(h_on, xd)
    h_on.profile_read()
    h_on.profile(False)
    for a, b, c in zip(on, again, serial):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert h_on.split_state() == 1


def test_preact_model_keeps_exact_path(monkeypatch):
    sd = make_sd(True, False, seed=3)
    xd = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(12)).to(DEV)
    h_on = make_handle(sd, True, False, monkeypatch, split=True)
    h_off = make_handle(sd, True, False, monkeypatch, split=False)
    assert h_on.split_state() == 0 and h_off.split_state() == 0
    for a, b in zip(fwd(h_on, xd), fwd(h_off, xd)):
        assert torch.equal(a, b)
    assert h_on.split_state() == 0


def test_overflow_switches_to_exact_plan(monkeypatch):
    """A region activation above 65504 (enc2's first BatchNorm scaled up): the
    forward that meets it raises the flag, the next one runs the exact plan for
    good and equals the UPR_FP32_SPLIT=0 model bit for bit."""
    sd = make_sd(False, False, seed=4)
    sd["ie_net.enc2.bn1.weight"] = sd["ie_net.enc2.bn1.weight"] * 1.0e7
    xd = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(13)).to(DEV)
    h_on = make_handle(sd, False, False, monkeypatch, split=True)
    h_off = make_handle(sd, False, False, monkeypatch, split=False)
    assert h_on.split_state() == 1
    fwd(h_on, xd)
    second = fwd(h_on, xd)
    assert h_on.split_state() == 2
    exact = fwd(h_off, xd)
    for a, b in zip(second, exact):
        assert torch.equal(a, b)
    third = fwd(h_on, xd)
    assert h_on.split_state() == 2
    for a, b in zip(third, exact):
        assert torch.equal(a, b)
