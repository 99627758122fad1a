"""float64 restatement of the direct (small-channel) training convolutions and
the conv helpers next to them, as include/upr_train.h states them.

Plain numpy, no torch in the arithmetic: the op-level GPU tests
(tests/test_gpu_conv_ops.py) measure the kernels against this, and
tests/test_cpu_conv_ops_oracle.py checks it against torch autograd in double.

Layouts.  Activations x [B, H, W, Cin], y, dy, y_mask [B, Ho, Wo, Cout]
(logical NHWC; the tests handle the memory layout); weights in PyTorch's
[Cout][Cin][kh][kw]; Ho = (H + 2 pad - dil (kh - 1) - 1) // stride + 1.
"""
import numpy as np

F64 = np.float64


def _f64(a):
    return None if a is None else np.asarray(a, dtype=F64)


def out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _padded(x, kh, kw, stride, pad, dil, Ho, Wo):
    """x zero-padded by `pad` before and by enough after that every tap's
    strided slice [k*dil : k*dil + (Ho-1)*stride + 1 : stride] is in range."""
    B, H, W, C = x.shape
    Hp = max(H + 2 * pad, (kh - 1) * dil + (Ho - 1) * stride + 1)
    Wp = max(W + 2 * pad, (kw - 1) * dil + (Wo - 1) * stride + 1)
    xp = np.zeros((B, Hp, Wp, C), dtype=F64)
    xp[:, pad:pad + H, pad:pad + W] = x
    return xp


def _tap(xp, ky, kx, stride, dil, Ho, Wo):
    y0, x0 = ky * dil, kx * dil
    return xp[:, y0:y0 + (Ho - 1) * stride + 1:stride, x0:x0 + (Wo - 1) * stride + 1:stride]


def conv_fwd(x, w, bias, stride, pad, dil, relu=False, y_prev=None):
    """y = conv(x, w) + bias (+ y_prev, the accumulate operand), then ReLU."""
    x, w = _f64(x), _f64(w)
    B, H, W, Cin = x.shape
    Cout, _, kh, kw = w.shape
    Ho, Wo = out_size(H, kh, stride, pad, dil), out_size(W, kw, stride, pad, dil)
    xp = _padded(x, kh, kw, stride, pad, dil, Ho, Wo)
    y = np.zeros((B, Ho, Wo, Cout), dtype=F64)
    for ky in range(kh):
        for kx in range(kw):
            y += _tap(xp, ky, kx, stride, dil, Ho, Wo) @ w[:, :, ky, kx].T
    if bias is not None:
        y += _f64(bias)
    if y_prev is not None:
        y += _f64(y_prev)
    return np.maximum(y, 0.0) if relu else y


def conv_dgrad(dy, w, H, W, stride, pad, dil):
    """dx[b, oy s - pad + ky dil, ox s - pad + kx dil, ci] += dy[b, oy, ox, co] w[co][ci][ky][kx]."""
    dy, w = _f64(dy), _f64(w)
    B, Ho, Wo, Cout = dy.shape
    _, Cin, kh, kw = w.shape
    dxp = _padded(np.zeros((B, H, W, Cin)), kh, kw, stride, pad, dil, Ho, Wo)
    for ky in range(kh):
        for kx in range(kw):
            _tap(dxp, ky, kx, stride, dil, Ho, Wo)[...] += dy @ w[:, :, ky, kx]
    return np.ascontiguousarray(dxp[:, pad:pad + H, pad:pad + W])


def conv_wgrad(x, dy, kh, kw, stride, pad, dil, y_mask=None):
    """(dw [Cout][Cin][kh][kw], dbias [Cout]); with y_mask, dy counts only
    where y_mask > 0 (false for 0, -0.0 and NaN)."""
    x, dy = _f64(x), _f64(dy)
    if y_mask is not None:
        with np.errstate(invalid="ignore"):
            dy = np.where(np.asarray(y_mask) > 0, dy, 0.0)
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    xp = _padded(x, kh, kw, stride, pad, dil, Ho, Wo)
    dw = np.zeros((Cout, Cin, kh, kw), dtype=F64)
    g = dy.reshape(-1, Cout)
    for ky in range(kh):
        for kx in range(kw):
            dw[:, :, ky, kx] = g.T @ _tap(xp, ky, kx, stride, dil, Ho, Wo).reshape(-1, Cin)
    return dw, g.sum(axis=0)


# ---------------------------------------------------------------------------
# index restatements (no arithmetic; the caller rounds)
# ---------------------------------------------------------------------------
def pack_weight(w, mode):
    """upr_t_pack_weight modes 0-3 and mode 4 of upr_t_pack_weights, flat.
    0: [Co][Ci][kh][kw] -> [Co][(ky, kx, ci)];
    1: -> [Ci][(ky, kx, co)] spatially flipped;
    2: ConvTranspose [Ci][Co][2][2] -> [(a, b, co)][ci];
    3: ConvTranspose [Ci][Co][2][2] -> [ci][(a, b, co)];
    4: a bias [Co] -> four copies [q][co]."""
    w = np.asarray(w)
    if mode == 4:
        return np.tile(w.reshape(-1), 4)
    if mode == 0:
        return w.transpose(0, 2, 3, 1).reshape(-1)
    if mode == 1:
        return w[:, :, ::-1, ::-1].transpose(1, 2, 3, 0).reshape(-1)
    assert w.shape[2:] == (2, 2), w.shape
    if mode == 2:
        return w.transpose(2, 3, 1, 0).reshape(-1)
    if mode == 3:
        return w.transpose(0, 2, 3, 1).reshape(-1)
    raise ValueError(mode)


def unpack_grad(gp, Co, Ci, kh, kw, mode):
    """The inverse of pack_weight modes 0 ([Co][Ci][kh][kw]) and 3 ([Ci][Co][2][2])."""
    gp = np.asarray(gp)
    if mode == 0:
        return gp.reshape(Co, kh, kw, Ci).transpose(0, 3, 1, 2)
    if mode == 3:
        return gp.reshape(Ci, kh, kw, Co).transpose(0, 3, 1, 2)
    raise ValueError(mode)


def zero_upsample(dy):
    """z [B, 2Ho, 2Wo, C]: dy at the even positions, zeros elsewhere."""
    dy = np.asarray(dy)
    B, Ho, Wo, C = dy.shape
    z = np.zeros((B, 2 * Ho, 2 * Wo, C), dtype=dy.dtype)
    z[:, ::2, ::2] = dy
    return z
