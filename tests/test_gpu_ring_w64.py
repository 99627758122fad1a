"""The weights-split-once 64 -> 64 stride-1 3x3 convs on the fp32 row ring
(csrc/conv_ring64.hip: dec2.conv.0, dec2.conv.3, enc1.conv2 with its shortcut
segment; UPR_W64_RING, include/upr.h upr_conv2d_nhwc_wsplit /
upr_conv_wsplit_ran) on the MI355X.

The ring stages every input row once (2 output rows x 32 pixels per step, a
34-pixel strip, row bands per image), splits it once in LDS and reads the
weight planes as they are packed; the arithmetic is that of the gathered-tile
kernel it replaces for these ops.  As in test_gpu_split_w64.py every check
compares against a float64 reference and bounds the ring's error by 4x the
exact fp32 kernels' error on the same inputs (a correct split measures <=
1.5x, a broken one is off by thousands), and every case asserts through
upr_conv_wsplit_ran that the ring -- or, for what it refuses, the tile
-- ran.  Both ring schedules (UPR_RING_SPLIT_LDS = 2 top of the step, 3 one
step ahead) must give the same bits.

Not reachable from here: a misaligned channel offset (the C entry point takes
whole tensors; the gate's `coff % 4` line refuses it for model graphs).
"""
import pytest
import torch

from conftest import has_gpu
from split_cases import DEV, WsplitCases, fwd, make_handle, make_sd, oracle_f64

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

# B, H, W, Cin, Cout, stride, pad, dil, relu, residual (after the ReLU), second segment (H2, W2, C2, stride2)
RING = {
    # the minimum rows and width the launcher takes: one partial strip, one band of four steps
    "one_partial_strip": (1, 8, 16, 64, 64, 1, 1, 1, False, False, None),
    # a full strip + a partial one, 10 rows = five 2-row steps of a 10-row band, two images: image-boundary
    # zero rows, sink stores of the partial strip, the residual landing zone (dec2.conv.3's flags)
    "strip_and_partial_two_images": (2, 10, 40, 64, 64, 1, 1, 1, True, True, None),
    # eight 8-row bands in one image: band edges read their neighbours' rows, not zeros (dec2.conv.0's flags)
    "row_bands": (1, 64, 32, 64, 64, 1, 1, 1, True, False, None),
    # odd row count (the last step's second row is out of range) and the register-fed shortcut segment (enc1.conv2)
    "shortcut_segment": (2, 9, 20, 64, 64, 1, 1, 1, True, False, (18, 40, 32, 2)),
    # 5 x 52 = 260 units of one band on 256 blocks: a block walks two units, the second starts with its
    # DMA-only step while the first one's last rows are still being computed
    "more_units_than_blocks": (5, 8, 1664, 64, 64, 1, 1, 1, True, False, None),
}
# what the ring refuses and the gathered tile takes
TILE = {
    "cin32": (1, 8, 16, 32, 64, 1, 1, 1, True, False, None),
    "n128": (1, 8, 16, 64, 128, 1, 1, 1, True, False, None),
    "stride2": (1, 16, 32, 64, 64, 2, 1, 1, True, False, None),
    "dilation2": (1, 8, 16, 64, 64, 1, 2, 2, True, False, None),
    "wo_below_16": (1, 8, 8, 64, 64, 1, 1, 1, True, False, None),
    "ho_below_4": (2, 3, 16, 64, 64, 1, 1, 1, True, False, None),
}
CASES = {**RING, **TILE}

_W = WsplitCases(CASES, lambda B, H, W, Cin, Cout: 4099 + 3 * H + 5 * W + Cin + 7 * Cout + 11 * B, "w64")
inputs, run_wsplit, run_exact, errors = _W.inputs, _W.run_wsplit, _W.run_exact, _W.errors


@pytest.mark.parametrize("name", list(RING))
def test_ring_vs_f64(name, monkeypatch):
    monkeypatch.delenv("UPR_W64_RING", raising=False)
    monkeypatch.delenv("UPR_RING_SPLIT_LDS", raising=False)
    e16, e32 = errors(name, 1.0, "ring")
    assert e16 <= 4 * e32, f"row ring {e16:.3e} vs fp32 path {e32:.3e}"


@pytest.mark.parametrize("name", ["strip_and_partial_two_images", "row_bands", "shortcut_segment"])
def test_ring_schedules_give_the_same_bits(name, monkeypatch):
    """Top of the step (4-group ring) and one step ahead (5 groups): the same
    function of the same values in the same MFMA order."""
    monkeypatch.delenv("UPR_W64_RING", raising=False)
    outs = []
    for mode in ("2", "3"):
        monkeypatch.setenv("UPR_RING_SPLIT_LDS", mode)
        y, ran = run_wsplit(name)
        torch.cuda.synchronize()
        assert ran == "ring"
        outs.append(y)
    refn = inputs(name)[-1]
    e32 = (run_exact(name).double().cpu() - refn).abs().max().item()
    for mode, y in zip(("2", "3"), outs):
        e16 = (y.double().cpu() - refn).abs().max().item()
        print(f"w64 ring {name} schedule {mode}: err {e16:.3e}  fp32 err {e32:.3e}")
        assert e16 <= 4 * e32, f"schedule {mode}: {e16:.3e} vs fp32 path {e32:.3e}"
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("scale", [2.0 ** -12, 300.0])
def test_ring_scaled_activations(scale, monkeypatch):
    """2^-12: the lo halves are fp16 subnormals (kept, not flushed); 300: large magnitudes."""
    monkeypatch.delenv("UPR_W64_RING", raising=False)
    monkeypatch.delenv("UPR_RING_SPLIT_LDS", raising=False)
    e16, e32 = errors("strip_and_partial_two_images", scale, "ring")
    assert e16 <= 4 * e32, f"row ring {e16:.3e} vs fp32 path {e32:.3e} at scale {scale}"


def test_ring_overflow_word(monkeypatch):
    """One input element outside the fp16 range sets the word; the plain input leaves it 0."""
    monkeypatch.delenv("UPR_W64_RING", raising=False)
    monkeypatch.delenv("UPR_RING_SPLIT_LDS", raising=False)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    _, ran = run_wsplit("strip_and_partial_two_images", 1.0, ovf)
    torch.cuda.synchronize()
    assert ran == "ring" and int(ovf.item()) == 0
    _, ran = run_wsplit("strip_and_partial_two_images", 1.0, ovf, poke=(1, 3, 17, 5))
    torch.cuda.synchronize()
    assert ran == "ring" and int(ovf.item()) == 1


@pytest.mark.parametrize("name", list(TILE))
def test_what_the_ring_refuses_runs_on_the_tile(name, monkeypatch):
    """No silent wrong kernel and no failure: the gathered tile, the same error bound."""
    monkeypatch.delenv("UPR_W64_RING", raising=False)
    e16, e32 = errors(name, 1.0, "tile")
    assert e16 <= 4 * e32, f"tile {e16:.3e} vs fp32 path {e32:.3e}"


def test_n32_is_refused_by_both_kernels():
    from upr import _lib as L
    from upr import runtime
    x = torch.zeros(1, 8, 16, 64, device=DEV)
    y = torch.zeros(1, 8, 16, 32, device=DEV)
    blob = runtime.pack_split_w(torch.zeros(64, 9 * 64), 3, 3).to(DEV)
    rc = L.lib().upr_conv2d_nhwc_wsplit(x.data_ptr(), 1, 8, 16, 64, blob.data_ptr(), blob.numel(), None, 32, 3, 3, 1, 1,
                                        1, None, 0, y.data_ptr(), None, 0, 0, 0, 1, None, None)
    assert rc == L.UPR_ERR_UNSUPPORTED
    assert runtime.last_wsplit_kernel() is None


def test_switch_keeps_the_tile_kernel(monkeypatch):
    monkeypatch.setenv("UPR_W64_RING", "0")
    e16, e32 = errors("strip_and_partial_two_images", 1.0, "tile")
    assert e16 <= 4 * e32
    monkeypatch.setenv("UPR_W64_RING", "1")
    assert run_wsplit("strip_and_partial_two_images")[1] == "ring"
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 48, 80)])
def test_model_ring_on_and_off(shape, monkeypatch):
    """UPR_W64_RING is read when the handle is created."""
    B, H, W = shape
    sd = make_sd(False, False)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(11))
    ref = oracle_f64(sd, x, False, False, shape)
    xd = x.to(DEV)
    monkeypatch.delenv("UPR_RING_SPLIT_LDS", raising=False)
    monkeypatch.setenv("UPR_W64_RING", "1")
    h_on = make_handle(sd, False, False, monkeypatch, split=True, regs=True, w64=True)
    monkeypatch.setenv("UPR_W64_RING", "0")
    h_tile = make_handle(sd, False, False, monkeypatch, split=True, regs=True, w64=True)
    monkeypatch.delenv("UPR_W64_RING")
    h_exact = make_handle(sd, False, False, monkeypatch, split=False, regs=True, w64=True)
    on, tile, exact = fwd(h_on, xd), fwd(h_tile, xd), fwd(h_exact, xd)
    for name, a, t, e, r in zip(("enhanced", "reflectance", "illumination"), on, tile, exact, ref):
        e_on = (a.double().cpu() - r).abs().max().item()
        e_tile = (t.double().cpu() - r).abs().max().item()
        e_exact = (e.double().cpu() - r).abs().max().item()
        ulp16 = 16 * 2.0 ** -23 * r.abs().max().item()
        print(f"model {shape} {name}: err ring {e_on:.3e}  err tile {e_tile:.3e}  err exact {e_exact:.3e}  16 ulp {ulp16:.3e}")
        assert e_on <= max(4 * e_exact, ulp16), f"{name}: ring {e_on:.3e}, exact {e_exact:.3e}"
        assert e_tile <= max(4 * e_exact, ulp16), f"{name}: tile {e_tile:.3e}, exact {e_exact:.3e}"
    # the same plan either way; the ring ran where it is expected to: some bit differs
    assert dict(h_on.op_forms()) == dict(h_tile.op_forms())
    assert sorted(n for n, f in h_on.op_forms() if f == 3) == sorted(
        "ie_net." + n for n in ("enc1.conv1", "enc1.conv2", "dec2.conv.0", "dec2.conv.3"))
    assert not all(torch.equal(a, b) for a, b in zip(on, tile))
    # bit-equal over two forwards, and between the forked and the profiled (one-stream) forward
    again = fwd(h_on, xd)
    h_on.profile(True)
    serial = fwd(h_on, xd)
    h_on.profile_read()
    h_on.profile(False)
    for a, b, c in zip(on, again, serial):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert h_on.split_state() == 1
