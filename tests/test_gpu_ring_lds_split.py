"""The fp32 row ring's split-in-registers programs convert each ring element to
fp16 (hi, lo) once, in LDS, instead of once per tap (UPR_RING_SPLIT_LDS,
include/upr.h).

The conversion is the same function on the same values and the MFMA order is
kept, so no program reorders a sum: every check here is bit-equality
(torch.equal) between the per-tap program (UPR_RING_SPLIT_LDS=0) and the LDS
forms (1, the default: each program in the form it ships in; 2: every program
converts at the top of the step, in the 4-group ring; 3: every program
converts one step ahead, in a 5-group ring), in one process.  The error
against float64 stays pinned by test_gpu_split_regs.py.
"""
import pytest
import torch

from conftest import has_gpu
from split_cases import DEV, RING_CASES, fwd, make_handle, make_sd, ring_inputs

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]
LDS_FORMS = ["1", "2", "3"]  # UPR_RING_SPLIT_LDS: the shipped choice, and each LDS form for every program


def many_units_case():
    """8 rows x 512 columns: 16 strips per image, one band; B images give 16 B
    units, more than the blocks of a launch (one per CU), so some blocks walk
    two units and cross a unit boundary with converted groups in the ring."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (17 if cus == 256 else cus // 16 + 1, 8, 512, 32, True, False)


CASES = RING_CASES + [
    (1, 45, 33, 32, True, False),   # 12 steps: a 5-group ring wraps twice; 1-pixel second strip
    "many_units",
]
SCALED = [(RING_CASES[1], 2.0 ** -12), (RING_CASES[1], 300.0)]


def run_regs(case, scale, mode, monkeypatch, poke=None):
    """One upr_conv2d_nhwc_regs call with UPR_RING_SPLIT_LDS = mode (read at the call)."""
    from upr import runtime
    relu = case[4]
    x, w, b, r, _ = ring_inputs(case, scale)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    if poke is not None:
        xd[poke] = 70000.0
    rd = r.permute(0, 2, 3, 1).contiguous().to(DEV) if r is not None else None
    wd, bd = runtime.pack_conv_weight(w).to(DEV), b.to(DEV)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    monkeypatch.setenv("UPR_RING_SPLIT_LDS", mode)
    y = runtime.conv2d_nhwc_regs(xd, wd, bd, 3, 3, 1, 1, 1, residual=rd, relu=relu, overflow=ovf)
    torch.cuda.synchronize()
    return y, int(ovf.item())


def check_case(case, scale, monkeypatch):
    tap, ovf_tap = run_regs(case, scale, "0", monkeypatch)
    assert ovf_tap == 0
    assert tap.abs().max().item() > 0
    for mode in LDS_FORMS:
        lds, ovf = run_regs(case, scale, mode, monkeypatch)
        ne = (lds != tap).sum().item()
        print(f"ring LDS split {case} x{scale:g} form {mode}: {ne} of {tap.numel()} outputs differ")
        assert ovf == 0
        assert torch.equal(lds, tap), f"form {mode}: {ne} outputs differ from the per-tap program"


@pytest.mark.parametrize("case", CASES, ids=str)
def test_ring_lds_bit_equal_to_per_tap(case, monkeypatch):
    check_case(many_units_case() if case == "many_units" else case, 1.0, monkeypatch)


@pytest.mark.parametrize("case,scale", SCALED)
def test_ring_lds_scaled_activations(case, scale, monkeypatch):
    check_case(case, scale, monkeypatch)


def test_unset_switch_is_the_lds_form(monkeypatch):
    """The default (variable unset) runs and equals both explicit settings."""
    from upr import runtime
    x, w, b, _, _ = ring_inputs(RING_CASES[1], 1.0)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd, bd = runtime.pack_conv_weight(w).to(DEV), b.to(DEV)
    monkeypatch.delenv("UPR_RING_SPLIT_LDS", raising=False)
    y = runtime.conv2d_nhwc_regs(xd, wd, bd, 3, 3, 1, 1, 1, relu=True)
    torch.cuda.synchronize()
    assert torch.equal(y, run_regs(RING_CASES[1], 1.0, "0", monkeypatch)[0])


@pytest.mark.parametrize("mode", ["0"] + LDS_FORMS)
def test_overflow_word_in_every_form(mode, monkeypatch):
    """One input element of 70000 (hi = +inf in the ring) sets the word."""
    _, ovf = run_regs(RING_CASES[1], 1.0, mode, monkeypatch, poke=(1, 3, 17, 5))
    assert ovf == 1


# ---------------------------------------------------------------------------
# model level: the dilation-2, x / maxpool, pool-sum and head programs
# ---------------------------------------------------------------------------
def make(sd, mode, monkeypatch):
    """UPR_RING_SPLIT_LDS is read when the handle is created."""
    monkeypatch.setenv("UPR_RING_SPLIT_LDS", mode)
    return make_handle(sd, False, False, monkeypatch, split=True, regs=True)


@pytest.mark.parametrize("shape", [(3, 48, 80), (1, 96, 64)])
def test_model_lds_bit_equal_to_per_tap(shape, monkeypatch):
    B, H, W = shape
    sd = make_sd(False, False)
    xd = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(11)).to(DEV)
    h_tap = make(sd, "0", monkeypatch)
    off = fwd(h_tap, xd)
    assert h_tap.split_state() == 1
    f_tap = h_tap.op_forms()
    assert 2 in dict(f_tap).values()
    for mode in LDS_FORMS:
        h = make(sd, mode, monkeypatch)
        on = fwd(h, xd)
        assert h.split_state() == 1
        for name, a, b in zip(("enhanced", "reflectance", "illumination"), on, off):
            ne = (a != b).sum().item()
            print(f"model {shape} form {mode} {name}: {ne} of {a.numel()} outputs differ")
            assert torch.equal(a, b), f"form {mode} {name}: {ne} outputs differ from the per-tap programs"
        assert h.op_forms() == f_tap
        # bit-equal over two forwards, and between the forked and the profiled (one-stream) forward
        again = fwd(h, xd)
        h.profile(True)
        serial = fwd(h, xd)
        h.profile_read()
        h.profile(False)
        for a, b, c in zip(on, again, serial):
            assert torch.equal(a, b) and torch.equal(a, c)
        assert h.op_forms() == f_tap
        assert h.split_state() == 1
