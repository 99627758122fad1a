"""Op-level parity of upr_t_loss_paired (csrc/train_paired.hip) against the
float64 restatement tests/paired_ref.py (run with `-m gpu`).  The entry is
called through ctypes on inputs made on the CPU, every buffer inside a frame of
sentinels.

Shapes (paired_ref.SHAPES): 2x3x7x9 (the window is larger than the image),
1x3x11x64, 1x3x16x16, 2x3x37x53 (ragged tiles, W % 4 != 0, two images), the
kernel's 16 x 32 tile and 17 x 33, a pixel more each way.  Inputs
(paired_ref.KINDS): uniform noise pairs, a 7 x 7-blurred image against 0.9 x +
0.05 + noise, the near-constant pair 0.5 + 1e-3 rand against 0.5, and a dark
pair 0.02 rand against rand.

Tolerances.  out2 and the gradient: op_parity._within_restated (the kernel's
error against float64 within 4x the error of the same definition in plain fp32
torch ops on the CPU, gradients by autograd; under 1e-4 max|ref| + 1e-6), each
scalar on its own.  Bit-equal: reruns, the unaligned call, pattern + gradient,
*total, every sentinel.  One fp32 ulp: out2[1] against the device metrics'
SSIM.

Measured on the MI355X (profiles/paired_ops_gpu_tests_v1.log): worst error
against float64 over the six shapes, in ulp of the case's largest |reference|;
"used" is the worst kernel error / allowed error (1 would fail).

  input, quantity                 restatement   kernel   used
  noise          reconstruction        0.40       0.40    0.20
                 ssim_loss             2.53       0.47    0.22
                 g_enh                22.56       0.50    0.03
  smooth         reconstruction        0.92       0.50    0.25
                 ssim_loss          2277.07       0.48    0.002
                 g_enh              1513.04       0.85    0.07
  near-constant  reconstruction        1.60       0.43    0.19
                 ssim_loss          2.6e+06       0.49    < 0.001
                 g_enh              8256.40       0.50    0.003
  dark           reconstruction        1.21       0.48    0.23
                 ssim_loss             0.50       0.50    0.25
                 g_enh                10.98       0.76    0.08

The kernel's error is the final rounding to fp32 everywhere.  The fp32
restatement's ssim_loss on the near-constant pair is up to 4.8e-6 off, beyond the
ceiling of about 1e-6: the reason the kernel is fp64.  41 tests in 2.6 s."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import paired_ref as R
from conftest import has_gpu
from op_parity import DEV, SENT, _within_restated, _within_ulp

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

PAD = 64        # sentinel elements on either side of a buffer (256 bytes: the inner part stays aligned)
WS_TAIL = 4096  # sentinel bytes after the workspace
WS_FILL = 0xA5
EPS = R.f32_eps()
IDS = lambda s: "x".join(map(str, s))  # noqa: E731


class Framed:
    """n floats on the device inside a buffer of sentinels; off shifts the inner part by `off` floats."""

    def __init__(self, shape, off=0, fill=SENT):
        self.shape, self.n, self.off, self.fill = tuple(shape), int(np.prod(shape)), off, fill
        self.buf = torch.full((self.n + 2 * PAD + off,), fill, dtype=torch.float32, device=DEV)
        self.ptr = self.buf.data_ptr() + 4 * (PAD + off)

    def set(self, t):
        self.buf[PAD + self.off:PAD + self.off + self.n] = torch.as_tensor(t, dtype=torch.float32).reshape(-1).to(DEV)
        return self

    def get(self, what="output"):
        b = self.buf.cpu()
        lo = PAD + self.off
        for part in (b[:lo], b[lo + self.n:]):
            assert torch.equal(part, torch.full_like(part, self.fill)), f"{what}: wrote outside its buffer"
        return b[lo:lo + self.n].view(self.shape).clone()


def _call(x, y, w_rec=1.0, w_ssim=1.0, eps=EPS, g0=None, want_g=True, total0=None, off=0):
    """One device call on numpy x, y [B,3,H,W] -> (out2 [2], g or None, total or None) as CPU tensors.
    g0: the gradient buffer's contents before the call (default zeros)."""
    from upr import _lib as L
    lib = L.lib()
    B, _, H, W = x.shape
    fx, fy = Framed(x.shape, off).set(x), Framed(y.shape, off).set(y)
    out2 = Framed((2,))
    fg = Framed(x.shape, off).set(np.zeros_like(x) if g0 is None else g0) if want_g else None
    ft = Framed((1,)).set([total0]) if total0 is not None else None
    nws = lib.upr_t_loss_paired_workspace(B, H, W)
    assert nws == B * 3 * -(-H // L.UPR_PAIRED_TILE[0]) * -(-W // L.UPR_PAIRED_TILE[1]) * 16
    ws = torch.full((nws + WS_TAIL,), WS_FILL, dtype=torch.uint8, device=DEV)
    rc = lib.upr_t_loss_paired(fx.ptr, fy.ptr, B, H, W, ctypes.c_float(eps), ctypes.c_float(w_rec),
                               ctypes.c_float(w_ssim), ws.data_ptr(), nws, out2.ptr, ft.ptr if ft else None,
                               fg.ptr if fg else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((ws[nws:] == WS_FILL).all()), "wrote past the workspace"
    assert np.array_equal(fx.get("enh").numpy(), x) and np.array_equal(fy.get("target").numpy(), y)
    return out2.get("out2"), fg.get("g_enh") if fg else None, ft.get("total") if ft else None


@functools.lru_cache(maxsize=None)
def _case(kind, shape, w_rec=1.0, w_ssim=1.0):
    """(x, y, float64 terms [2], float64 gradient, fp32 restated terms [2], fp32 restated gradient): computed once."""
    x, y = R.make_pair(kind, shape)
    ref = np.array(R.terms(x, y, EPS))
    g = R.grad(x, y, w_rec, w_ssim, EPS)
    xt = torch.from_numpy(x).requires_grad_(True)
    rec, sl = R.torch_terms(xt, torch.from_numpy(y), EPS)
    (float(w_rec) * rec + float(w_ssim) * sl).backward()
    return x, y, ref, g, torch.stack([rec.detach(), sl.detach()]), xt.grad


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_terms_and_gradient(kind, shape):
    x, y, ref, g, rs, rs_g = _case(kind, shape)
    out2, dg, _ = _call(x, y)
    tag = f"paired {kind} {IDS(shape)}"
    for i, name in enumerate(("reconstruction", "ssim_loss")):
        _within_restated(f"{tag} {name}", out2[i:i + 1], ref[i:i + 1], rs[i:i + 1])
    _within_restated(f"{tag} g_enh", dg, g, rs_g)


@pytest.mark.parametrize("weights", ((1.0, 0.0), (0.0, 1.0), (0.7, 1.3)), ids=("rec", "ssim", "mixed"))
def test_weights(weights):
    """Each term's gradient alone (bounded by its own size) and a mixed pair; out2 stays unweighted."""
    shape = (2, 37, 53)
    for kind in ("smooth", "dark"):
        x, y, ref, g, rs, rs_g = _case(kind, shape, *weights)
        out2, dg, _ = _call(x, y, *weights)
        assert torch.equal(out2, _call(x, y)[0]), "out2 depends on the weights"
        _within_restated(f"paired {kind} {weights} g_enh", dg, g, rs_g)


def test_accumulates_into_the_gradient():
    """g_enh pre-filled with a pattern comes back as pattern + gradient (one fp32 add per element)."""
    x, y = R.make_pair("smooth", (2, 37, 53))
    _, g, _ = _call(x, y)
    pattern = (np.arange(x.size, dtype=np.float32).reshape(x.shape) % 17 - 8) * np.float32(1e-3)
    _, gp, _ = _call(x, y, g0=pattern)
    assert torch.equal(gp, torch.from_numpy(pattern) + g)
    assert g.abs().max() > 0


def test_null_gradient_writes_only_the_scalars():
    x, y = R.make_pair("noise", (2, 37, 53))
    out2, g, _ = _call(x, y, want_g=False)  # (_call checks the frames, the inputs and the workspace tail)
    assert g is None and torch.equal(out2, _call(x, y)[0])


@pytest.mark.parametrize("shape", ((2, 37, 53), (1, 16, 32), (1, 11, 64)), ids=IDS)
def test_unaligned_pointers_give_the_same_bits(shape):
    x, y = R.make_pair("smooth", shape)
    a, b = _call(x, y, total0=1.5), _call(x, y, total0=1.5, off=1)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_reruns_are_bit_identical():
    x, y = R.make_pair("noise", (2, 37, 53))
    a, b = _call(x, y), _call(x, y)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("weights", ((1.0, 1.0), (0.3, 2.5), (0.0, 0.0)))
def test_total_rises_by_the_weighted_sum(weights):
    x, y = R.make_pair("dark", (2, 7, 9))
    out2, _, total = _call(x, y, *weights, total0=3.25)
    o = out2.numpy()
    w = np.float32(weights[0]) * o[0] + np.float32(weights[1]) * o[1]  # fp32, product by product
    assert total.numpy()[0] == np.float32(3.25) + w
    assert torch.equal(out2, _call(x, y)[0])


@pytest.mark.parametrize("shape", ((2, 37, 53), (1, 17, 33), (2, 8, 9)), ids=IDS)
def test_ssim_loss_is_the_device_metric(shape):
    """out2[1] against 1 - mean of batch_metrics' per-image SSIM (csrc/metrics.hip), to one fp32 ulp
    (upr_image_metrics takes H, W >= 8: 8 x 9 is its smallest image with the window larger than it)."""
    from utils.utils import batch_metrics
    for kind in ("smooth", "near_constant"):
        x, y = R.make_pair(kind, shape)
        out2, _, _ = _call(x, y, want_g=False)
        m = batch_metrics(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))["ssim"]
        _within_ulp(f"paired {kind} {IDS(shape)} ssim_loss vs metrics", out2[1:2], [1.0 - m.mean().item()], ulps=1.0)


def test_empty_batch_and_refused_shapes():
    from upr import _lib as L
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    out2 = Framed((2,))
    assert lib.upr_t_loss_paired(None, None, 0, 8, 8, ctypes.c_float(EPS), ctypes.c_float(1), ctypes.c_float(1),
                                 None, 0, out2.ptr, None, None, st) == L.UPR_OK
    torch.cuda.synchronize()
    assert torch.equal(out2.get(), torch.full((2,), SENT))
    for B, H, W in ((1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, 65536, 32768)):
        assert lib.upr_t_loss_paired_workspace(B, H, W) == 0
    x = Framed((1, 3, 8, 8)).set(np.zeros((1, 3, 8, 8), np.float32))
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    assert lib.upr_t_loss_paired(x.ptr, x.ptr, 1, 0, 8, ctypes.c_float(EPS), ctypes.c_float(1), ctypes.c_float(1),
                                 ws.data_ptr(), 64, out2.ptr, None, None, st) == L.UPR_ERR_SHAPE
    assert lib.upr_t_loss_paired(x.ptr, x.ptr, 1, 8, 8, ctypes.c_float(EPS), ctypes.c_float(1), ctypes.c_float(1),
                                 ws.data_ptr(), 8, out2.ptr, None, None, st) == L.UPR_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(out2.get(), torch.full((2,), SENT))


def test_single_term_modules():
    """ReconstructionLoss / SSIMLoss: the op's values, and its gradient scaled by the incoming one."""
    from losses.loss import ReconstructionLoss, SSIMLoss
    x, y = R.make_pair("smooth", (2, 37, 53))
    for i, mod in enumerate((ReconstructionLoss(), SSIMLoss())):
        out2, g, _ = _call(x, y, 1.0 - i, float(i))
        xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
        v = mod(xt, torch.from_numpy(y).to(DEV))
        (3.0 * v).backward()
        assert v.item() == out2[i].item()
        assert torch.equal(xt.grad.cpu(), g * 3.0)
        with torch.no_grad():
            assert mod(xt, torch.from_numpy(y).to(DEV)).item() == out2[i].item()
    with pytest.raises(NotImplementedError, match="target"):
        SSIMLoss()(xt, torch.from_numpy(y).to(DEV).requires_grad_(True))
    assert ReconstructionLoss(eps=1e-2)(xt, xt.detach()).item() == pytest.approx(1e-2, rel=1e-6)
