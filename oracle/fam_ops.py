"""float64 restatement of the EnhancedFAM attention ops, the network tail
(head, retinex, enhance) and the small reductions / pointwise ops they are
wired to, as include/upr_train.h states them.

Plain numpy, no torch in the arithmetic: the op-level GPU tests
(tests/test_gpu_fam_ops.py) measure the kernels against this, and
tests/test_cpu_fam_ops_oracle.py checks it against torch autograd in double.

Layouts.  Attention: o, o2, out, g [B, HW, C]; ca, g_ca, g_pool [B, C];
m, g_m [B, HW, 2] = (mean_c, max_c); s_pre, sa, g_spre [B, HW].  Tail: x,
refl, enh and their gradients NCHW [B, 3, H, W]; o, e, g_o NHWC [B, H, W, 3];
r, illu, g_illu, g_r [B, H, W].
"""
import numpy as np

F64 = np.float64
U64 = np.uint64


def _f64(a):
    return None if a is None else np.asarray(a, dtype=F64)


def sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-_f64(x)))


# ---------------------------------------------------------------------------
# EnhancedFAM attention
# ---------------------------------------------------------------------------
def ca_apply(o, ca):
    """o2 = o * ca[b][c]; m = (mean_c o2, max_c o2) (the max is NaN where a
    channel is NaN, as torch.max)."""
    o2 = _f64(o) * _f64(ca)[:, None, :]
    return o2, np.stack([o2.mean(axis=-1), o2.max(axis=-1)], axis=-1)


def sa_apply(o2, s_pre):
    """sa = sigmoid(s_pre); out = o2 * sa."""
    sa = sigmoid(s_pre)
    return sa, _f64(o2) * sa[..., None]


def sa_bwd(g, o2, sa):
    """g_o2 = g * sa; g_spre = sum_c(g * o2) * sa * (1 - sa)."""
    g, sa = _f64(g), _f64(sa)
    return g * sa[..., None], (g * _f64(o2)).sum(axis=-1) * sa * (1.0 - sa)


def ca_bwd(g_o2, g_m, o, o2, ca):
    """g_t = g_o2 + g_m[..., 0] / C on every channel + g_m[..., 1] on the
    channel torch.max(o2, dim) picks (the first maximum, or the first NaN:
    np.argmax's rule); g_o = g_t * ca; g_ca[b][c] = sum_p g_t * o."""
    g_m, o2 = _f64(g_m), np.asarray(o2)
    C = o2.shape[-1]
    gt = _f64(g_o2) + g_m[..., :1] / C
    am = np.argmax(o2, axis=-1)
    gt = gt + np.where(np.arange(C) == am[..., None], g_m[..., 1:], 0.0)
    return gt * _f64(ca)[:, None, :], (gt * _f64(o)).sum(axis=1)


def pool_bwd(g_o, g_pool, o):
    """(g_o + g_pool[b][c] / HW) * (o > 0): the average pool's gradient joins
    and the fusion conv's ReLU masks."""
    g_o = _f64(g_o)
    return np.where(np.asarray(o) > 0, g_o + _f64(g_pool)[:, None, :] / g_o.shape[1], 0.0)


# ---------------------------------------------------------------------------
# network tail
# ---------------------------------------------------------------------------
def _nhwc(a):
    return np.transpose(a, (0, 2, 3, 1))


def _nchw(a):
    return np.transpose(a, (0, 3, 1, 2))


def head_fwd(x, r):
    """illu = sigmoid(mean_c x + r)."""
    return sigmoid(_f64(x).mean(axis=1) + _f64(r))


def _combine(refl, e):
    return refl * e + (1.0 - refl) * e * e


def retinex_fwd(x, illu, o):
    """e = sigmoid(o) (NHWC); refl = x / (illu + 1e-6); enh = refl*e + (1-refl)*e^2 (NCHW)."""
    e = sigmoid(o)
    refl = _f64(x) / (_f64(illu)[:, None] + 1e-6)
    return e, refl, _combine(refl, _nchw(e))


def retinex_bwd(x, illu, e, refl, g_enh, g_refl=None, g_illu=None):
    """Backward of head_fwd + retinex_fwd from (g_enh, g_refl, g_illu) with
    the saved illu, e and refl: g_o (NHWC, through e's sigmoid) and g_r
    (through refl = x / (illu + 1e-6), plus g_illu, through illu's sigmoid)."""
    x, illu, refl, g_enh = _f64(x), _f64(illu), _f64(refl), _f64(g_enh)
    ec = _nchw(_f64(e))
    g_e = g_enh * (refl + 2.0 * ec * (1.0 - refl))
    g_rf = g_enh * (ec - ec * ec)
    if g_refl is not None:
        g_rf = g_rf + _f64(g_refl)
    den = illu + 1e-6
    g_il = -(g_rf * x).sum(axis=1) / (den * den)
    if g_illu is not None:
        g_il = g_il + _f64(g_illu)
    return _nhwc(g_e * ec * (1.0 - ec)), g_il * illu * (1.0 - illu)


def enhance_fwd(refl, o):
    """e = sigmoid(o) (NHWC); enh = refl*e + (1-refl)*e^2 (NCHW)."""
    e = sigmoid(o)
    return e, _combine(_f64(refl), _nchw(e))


def enhance_bwd(e, refl, g_enh):
    """g_o (NHWC, through the sigmoid) and g_refl (NCHW) from g_enh."""
    refl, g_enh = _f64(refl), _f64(g_enh)
    ec = _nchw(_f64(e))
    return _nhwc(g_enh * (refl + 2.0 * ec * (1.0 - refl)) * ec * (1.0 - ec)), g_enh * (ec - ec * ec)


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def pixel_sum(x, scale, out0=None):
    """out[b][c] = (out0 +) scale * sum over the pixels of x[B, HW, C]."""
    s = F64(scale) * _f64(x).sum(axis=1)
    return s if out0 is None else s + _f64(out0)


def broadcast(v, scale, HW, y0=None):
    """y[b][p][c] = (y0 +) v[b][c] * scale."""
    v = _f64(v) * F64(scale)
    y = np.broadcast_to(v[:, None, :], (v.shape[0], HW, v.shape[1]))
    return y.copy() if y0 is None else y + _f64(y0)


def sigmoid_bwd(a, s):
    """Pointwise op 1: a * s * (1 - s), s = the sigmoid's output."""
    a, s = _f64(a), _f64(s)
    return a * s * (1.0 - s)


def hash_uniform(seed, n):
    """splitmix64 of (seed, index) for index 0 .. n-1 -> [0, 1): the top 24
    bits / 2^24 (exact in fp32 and fp64 alike)."""
    with np.errstate(over="ignore"):
        z = U64(seed) + U64(0x9E3779B97F4A7C15) * (np.arange(n, dtype=U64) + U64(1))
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    z = z ^ (z >> U64(31))
    return (z >> U64(40)).astype(F64) / 16777216.0


def dropout_mask(n, p, seed):
    """nn.Dropout(p)'s keep-mask as the kernel draws it: keep where
    hash_uniform >= p (p as the fp32 value the entry is given)."""
    return (hash_uniform(seed, n) >= F64(np.float32(p))).astype(np.uint8)


def dropout(a, mask, p):
    """Pointwise ops 2 / 3: a * mask / (1 - p)."""
    return np.where(np.asarray(mask) != 0, _f64(a) * (1.0 / (1.0 - F64(np.float32(p)))), 0.0)


def add(a, b):
    return _f64(a) + _f64(b)


def scale(a, s):
    return _f64(a) * F64(s)
