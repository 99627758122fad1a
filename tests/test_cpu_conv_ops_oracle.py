"""Self-check of the float64 op reference oracle/conv_ops.py (numpy) against
torch.nn.functional.conv2d and its autograd in double: both sides are
float64, so they agree to 1e-12 relative (of the largest reference
magnitude).  The grid holds every (Cin, Cout, k, stride, pad, dil) that
tests/test_gpu_conv_ops.py runs (conv_configs() there), at H != W, with pads
that make Ho != H and stride 2 at sizes the stride does not divide."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_ops as O
from test_gpu_conv_ops import conv_configs

REL = 1e-12

# besides the GPU file's combinations: pad > (k - 1) / 2, a stride that leaves a remainder with dilation
EXTRA = [(3, 5, 3, 2, 2, 1), (2, 3, 3, 2, 2, 2), (4, 2, 5, 3, 1, 1)]
CONFIGS = sorted(set(conv_configs()) | set(EXTRA))


def _agree(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), b.detach().double().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max()
    tol = REL * max(np.abs(b).max(), 1e-300)
    assert err <= tol, f"{what}: max|d| {err:.3e} > {tol:.3e}"


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).requires_grad_(grad)


def _nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


@pytest.mark.parametrize("Cin,Cout,k,s,p,d", CONFIGS)
@pytest.mark.parametrize("B,H,W", [(2, 9, 12), (1, 14, 11)])
def test_conv_matches_autograd_double(Cin, Cout, k, s, p, d, B, H, W):
    """forward (plain, and accumulate + ReLU), input and weight gradients,
    and the ReLU-masked weight gradient against relu's autograd; stride 2
    meets an even and an odd size in each shape."""
    if H + 2 * p < d * (k - 1) + 1 or W + 2 * p < d * (k - 1) + 1:
        H, W = H + d * (k - 1), W + d * (k - 1)
    rng = np.random.default_rng(1000 * Cin + 10 * Cout + k + s + p + d)
    Ho, Wo = O.out_size(H, k, s, p, d), O.out_size(W, k, s, p, d)
    x, w, bias = rng.standard_normal((B, H, W, Cin)), rng.standard_normal((Cout, Cin, k, k)), rng.standard_normal(Cout)
    dy, y_prev = rng.standard_normal((B, Ho, Wo, Cout)), rng.standard_normal((B, Ho, Wo, Cout))
    xt, wt, bt = _t(_nchw(x), True), _t(w, True), _t(bias, True)
    yt = F.conv2d(xt, wt, bt, s, p, d)
    assert yt.shape == (B, Cout, Ho, Wo)
    _agree(_nchw(O.conv_fwd(x, w, bias, s, p, d)), yt, "y")
    _agree(_nchw(O.conv_fwd(x, w, None, s, p, d)), F.conv2d(xt, wt, None, s, p, d), "y without bias")
    _agree(_nchw(O.conv_fwd(x, w, bias, s, p, d, relu=True, y_prev=y_prev)), torch.relu(yt + _t(_nchw(y_prev))),
           "relu(y + y_prev)")
    yt.backward(_t(_nchw(dy)))
    _agree(_nchw(O.conv_dgrad(dy, w, H, W, s, p, d)), xt.grad, "dx")
    dw, db = O.conv_wgrad(x, dy, k, k, s, p, d)
    _agree(dw, wt.grad, "dw")
    _agree(db, bt.grad, "dbias")
    # the masked weight gradient: y's own ReLU, exact zeros planted (relu'(0) = 0)
    xt.grad = wt.grad = bt.grad = None
    y0 = F.conv2d(xt, wt, bt, s, p, d)
    hole = _t(_nchw((rng.random((B, Ho, Wo, Cout)) < 0.2).astype(np.float64)))
    y1 = y0 - hole * y0.detach()  # exactly 0 where hole
    yr = torch.relu(y1)
    yr.backward(_t(_nchw(dy)))
    mask = np.transpose(yr.detach().numpy(), (0, 2, 3, 1))
    dwm, dbm = O.conv_wgrad(x, dy, k, k, s, p, d, y_mask=mask)
    _agree(dwm, wt.grad, "masked dw")
    _agree(dbm, bt.grad, "masked dbias")


def test_mask_rule():
    """y_mask > 0 is false for 0.0, -0.0, negatives and NaN."""
    x, dy = np.ones((1, 1, 5, 1)), np.arange(1.0, 6.0).reshape(1, 1, 5, 1)
    m = np.array([2.0, 0.0, -0.0, -1.0, np.nan]).reshape(1, 1, 5, 1)
    dw, db = O.conv_wgrad(x, dy, 1, 1, 1, 0, 1, y_mask=m)
    assert dw.item() == 1.0 and db.item() == 1.0


@pytest.mark.parametrize("Co,Ci,k", [(64, 32, 3), (3, 32, 1), (1, 2, 7), (5, 6, 2)])
def test_pack_layouts(Co, Ci, k):
    """modes 0 / 1 spelled out with indices; unpack_grad inverts mode 0."""
    w = np.random.default_rng(Co + Ci + k).standard_normal((Co, Ci, k, k)).astype(np.float32)
    p0, p1 = O.pack_weight(w, 0).reshape(Co, k, k, Ci), O.pack_weight(w, 1).reshape(Ci, k, k, Co)
    for co, ci, ky, kx in np.ndindex(min(Co, 4), min(Ci, 4), k, k):
        assert p0[co, ky, kx, ci] == w[co, ci, ky, kx]
        assert p1[ci, ky, kx, co] == w[co, ci, k - 1 - ky, k - 1 - kx]
    assert np.array_equal(p1, torch.from_numpy(w).flip(2, 3).permute(1, 2, 3, 0).numpy())
    assert np.array_equal(O.unpack_grad(O.pack_weight(w, 0), Co, Ci, k, k, 0), w)
    assert np.array_equal(O.pack_weight(w[:, 0, 0, 0], 4).reshape(4, Co), np.broadcast_to(w[:, 0, 0, 0], (4, Co)))


@pytest.mark.parametrize("Co,Ci", [(32, 64), (3, 5)])
def test_pack_convtranspose_layouts(Co, Ci):
    """modes 2 / 3 on a ConvTranspose2d weight [Ci][Co][2][2]: mode 2 is the
    GEMM B operand of y[b, 2i + a, 2j + c, co] = sum_ci x[b, i, j, ci] w[ci][co][a][c],
    checked against F.conv_transpose2d in double; unpack_grad inverts mode 3."""
    rng = np.random.default_rng(Co * Ci)
    w = rng.standard_normal((Ci, Co, 2, 2))
    p2, p3 = O.pack_weight(w, 2).reshape(2, 2, Co, Ci), O.pack_weight(w, 3).reshape(Ci, 2, 2, Co)
    for ci, co, a, c in np.ndindex(min(Ci, 4), min(Co, 4), 2, 2):
        assert p2[a, c, co, ci] == w[ci, co, a, c]
        assert p3[ci, a, c, co] == w[ci, co, a, c]
    assert np.array_equal(O.unpack_grad(O.pack_weight(w, 3), Co, Ci, 2, 2, 3), w)
    x = rng.standard_normal((2, 3, 4, Ci))
    g = x.reshape(-1, Ci) @ O.pack_weight(w, 2).reshape(4 * Co, Ci).T  # [pixel][(a, c, co)]
    y = g.reshape(2, 3, 4, 2, 2, Co).transpose(0, 1, 3, 2, 4, 5).reshape(2, 6, 8, Co)
    _agree(_nchw(y), F.conv_transpose2d(_t(_nchw(x)), _t(w), None, 2), "ConvTranspose as a GEMM over mode 2")


def test_zero_upsample():
    """z is the operand whose stride-1 conv gives a stride-2 conv's input
    gradient: conv_dgrad at stride 2 equals conv_dgrad at stride 1 over z."""
    rng = np.random.default_rng(5)
    dy, w = rng.standard_normal((2, 3, 5, 4)), rng.standard_normal((4, 3, 3, 3))
    z = O.zero_upsample(dy)
    assert z.shape == (2, 6, 10, 4) and np.array_equal(z[:, ::2, ::2], dy)
    assert not z[:, 1::2].any() and not z[:, :, 1::2].any()
    a = O.conv_dgrad(dy, w, 6, 10, 2, 1, 1)  # Ho = (6 + 2 - 3) // 2 + 1 = 3, Wo = 5
    b = O.conv_dgrad(z, w, 6, 10, 1, 1, 1)
    assert np.abs(a - b).max() <= REL * np.abs(a).max()
