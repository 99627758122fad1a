"""float64 restatement of the loss and gradient-norm ops of csrc/train_loss.hip
and upr_t_sqsum, as include/upr_train.h states them.

The pixel terms (exposure, smoothness, colour, spatial, decoupling, texture
complexity, the dynamic smooth weight) are oracle/train.py's, which the G6
goldens pin to the reference: pixel_terms() evaluates them at a dtype and takes
the weighted gradient by torch autograd.  float64 is the reference of the
op-level GPU tests (tests/test_gpu_loss_ops.py); float32 is the plain-fp32
restatement their error bound is measured in.  The other ops are plain numpy,
no torch in the arithmetic; tests/test_cpu_loss_ops_oracle.py checks them
against torch in double.

Layouts.  low, enh, refl and their gradients NCHW [B, 3, H, W]; illu, g_illu
[B, CI, H, W] (CI 1 or 3); spectra complex [BC, H, W]; vgg_norm's y NHWC
[B, H, W, 3].  Every fp32 argument of an entry (weights, scales, module
parameters) enters at the fp32 value the entry is given.
"""
import numpy as np
import torch

from . import train as T

F64 = np.float64

# UprLossParams' reference defaults (upr_t_loss_pixel)
DEFAULT_PARAMS = {"patch": 16, "base_exposure": 0.6, "smooth_lambda": 10.0, "smooth_alpha": 1.0,
                  "decouple_lambda": 0.1, "dynamic_smooth": 1}
TEXTURE_METHODS = ("tv", "edge_density")
# the kernels' fp32 constants
VGG_MEAN32 = np.asarray(T.VGG_MEAN, dtype=np.float32).astype(F64)
VGG_STD32 = np.asarray(T.VGG_STD, dtype=np.float32).astype(F64)


def _f64(a):
    return np.asarray(a, dtype=F64)


def f32(v):
    """The fp32 value an entry receives for the python number v, as a python float."""
    return float(np.float32(v))


# ---------------------------------------------------------------------------
# pixel terms
# ---------------------------------------------------------------------------
def pixel_terms(low, enh, illu, refl, weights, params, w_smooth, texture, dtype=torch.float64):
    """upr_t_loss_pixel_p at `dtype`.  weights = (w_exp, w_col, w_spa, w_dec);
    params: UprLossParams' fields by name (DEFAULT_PARAMS); texture 0 'tv', 1
    'edge_density' (read with dynamic_smooth only).

    Returns (terms, wsm, g_enh, g_illu, g_refl): terms = float64 array
    [exposure, smoothness, colour, spatial, decouple] (terms[0..4] of the
    entry), wsm = the smooth weight (terms[8]), and the gradient of
    w_exp exposure + wsm.detach() smoothness + w_col colour + w_spa spatial +
    w_dec decouple with respect to enh, illu and refl (float64 arrays)."""
    p = dict(DEFAULT_PARAMS)
    p.update(params)
    w_exp, w_col, w_spa, w_dec = (f32(w) for w in weights)
    lo = torch.as_tensor(np.asarray(low)).to(dtype)
    e, i, r = (torch.as_tensor(np.asarray(a)).to(dtype).requires_grad_(True) for a in (enh, illu, refl))
    terms = [T.exposure_loss(e, lo, int(p["patch"]), f32(p["base_exposure"])),
             T.smoothness_loss(i, lo, f32(p["smooth_lambda"]), f32(p["smooth_alpha"])),
             T.color_loss(e),
             T.spatial_loss(e, lo),
             T.decouple_loss(i, r, f32(p["decouple_lambda"]))]
    if p["dynamic_smooth"]:
        # (the edge-density share is a .float() of booleans whatever lo's dtype)
        tc = T.texture_complexity(lo, TEXTURE_METHODS[texture]).to(dtype).mean()
        wsm = torch.clamp(f32(w_smooth) * (1.0 - tc * 0.8), 0.1, 5.0)
    else:
        wsm = torch.tensor(f32(w_smooth), dtype=dtype)
    total = (w_exp * terms[0] + wsm.detach() * terms[1] + w_col * terms[2] + w_spa * terms[3] + w_dec * terms[4])
    total.backward()

    def g(t):
        return np.zeros(tuple(t.shape)) if t.grad is None else t.grad.double().numpy()
    return (np.array([float(t.detach().double()) for t in terms]), float(wsm.detach().double()), g(e), g(i), g(r))


def exposure_patches(low, enh, patch, base):
    """The exposure term's patch means P [B, H // patch, W // patch] and its
    adaptive target T = base + (0.8 - base) (1 - mean gray(low)), in float64."""
    low, enh, base = _f64(low), _f64(enh), f32(base)
    B, _, H, W = enh.shape
    ph, pw = H // patch, W // patch
    gray = enh.mean(axis=1)[:, :ph * patch, :pw * patch]
    P = gray.reshape(B, ph, patch, pw, patch).mean(axis=(2, 4))
    return P, base + (0.8 - base) * (1.0 - low.mean(axis=1).mean())


def sobel_magnitude(img):
    """Reflect-padded Sobel magnitude [B, H, W] of the channel-mean gray of img
    [B, C, H, W] (oracle/train.py::edge_map), each tap subtracted from its
    mirror tap first.  On an axis of two samples the reflect pad makes every
    such pair equal, so that direction's derivative is exactly 0 here, as it
    is mathematically; a convolution that adds the taps in another order
    (edge_map's conv2d) leaves rounding noise in its place, and on a 2 x 2
    image, where both derivatives vanish, the 'edge_density' count of e > 1.5
    mean e would be a count of that noise."""
    img = _f64(img)
    p = np.pad(img.mean(axis=1) if img.shape[1] > 1 else img[:, 0], ((0, 0), (1, 1), (1, 1)), mode="reflect")
    t, m, b = p[:, :-2], p[:, 1:-1], p[:, 2:]
    gx = (t[:, :, 2:] - t[:, :, :-2]) + 2.0 * (m[:, :, 2:] - m[:, :, :-2]) + (b[:, :, 2:] - b[:, :, :-2])
    gy = (b[:, :, :-2] - t[:, :, :-2]) + 2.0 * (b[:, :, 1:-1] - t[:, :, 1:-1]) + (b[:, :, 2:] - t[:, :, 2:])
    return np.sqrt(gx * gx + gy * gy)


def edge_margin(img):
    """min over pixels of |e - 1.5 mean e| / (1.5 mean e), e = sobel_magnitude
    with its per-image mean: how far the 'edge_density' count is from
    changing (nan where an image's e is all 0)."""
    e = sobel_magnitude(img)
    thr = 1.5 * e.mean(axis=(1, 2), keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float((np.abs(e - thr) / thr).min())


def texture_complexity(img, method):
    """calculate_texture_complexity per image [B] in float64: method 0 'tv'
    (oracle/train.py's), 1 'edge_density' (the share of pixels with
    sobel_magnitude > 1.5 x its image mean)."""
    if method == 0:
        return T.texture_complexity(torch.as_tensor(_f64(img)), "tv").numpy()
    e = sobel_magnitude(img)
    return (e > 1.5 * e.mean(axis=(1, 2), keepdims=True)).mean(axis=(1, 2))


# ---------------------------------------------------------------------------
# frequency, MSE, VGG normalisation, scalar helpers
# ---------------------------------------------------------------------------
def freq_low_mask(H, W):
    """True where dist((y, x), (H // 2, W // 2)) <= min(H, W) // 4 (no
    fftshift, as the reference has it): the weight_low region."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dist = np.sqrt(((x - W // 2) ** 2 + (y - H // 2) ** 2).astype(F64))  # exact on lattice points of the circle
    return dist <= min(H, W) // 4


def freq(Ze, Zl, H, W, scale, w_high, w_low):
    """(sum w (|Ze| - |Zl|)^2, G = scale 2 w (|Ze| - |Zl|) Ze / |Ze|), w =
    w_low inside the mask and w_high outside; G = 0 where |Ze| = 0."""
    Ze, Zl = np.asarray(Ze, dtype=np.complex128), np.asarray(Zl, dtype=np.complex128)
    w = np.where(freq_low_mask(H, W), f32(w_low), f32(w_high))[None]
    me, ml = np.abs(Ze), np.abs(Zl)
    d = me - ml
    k = np.divide(f32(scale) * 2.0 * w * d, me, out=np.zeros_like(me), where=me > 0)
    return float((w * d * d).sum()), k * Ze


def mse(a, b, scale):
    """(mean (a - b)^2, g = scale 2 (a - b))."""
    d = _f64(a) - _f64(b)
    return float((d * d).mean()), f32(scale) * 2.0 * d


def vgg_norm(x):
    """(x NCHW - mean) / std -> NHWC, mean / std the kernel's fp32 constants."""
    return np.transpose((_f64(x) - VGG_MEAN32[None, :, None, None]) / VGG_STD32[None, :, None, None], (0, 2, 3, 1))


def vgg_norm_bwd(g_y, g_x0):
    """g_x (NCHW) = g_x0 + g_y (NHWC) / std."""
    return _f64(g_x0) + np.transpose(_f64(g_y) / VGG_STD32, (0, 3, 1, 2))


def add_real(z, g0, scale):
    """g = g0 + scale Re(z)."""
    return _f64(g0) + f32(scale) * np.asarray(z).real.astype(F64)


def scale_acc(acc, scale):
    """out[i] = scale acc[i]."""
    return f32(scale) * _f64(acc)


def loss_total(terms, w_exp, w_col, w_spa, w_dec, w_per, w_freq):
    """terms[7] of [exposure, smoothness, colour, spatial, decouple,
    perceptual, frequency, total, smooth_weight]: the weighted sum, terms[8]
    the smoothness weight."""
    t = _f64(terms)
    w = [f32(w_exp), t[8], f32(w_col), f32(w_spa), f32(w_dec), f32(w_per), f32(w_freq)]
    return float(sum(wk * tk for wk, tk in zip(w, t[:7])))


def sqsum(g, acc0=0.0):
    """acc0 + sum g^2."""
    g = _f64(g).ravel()
    return float(acc0) + float(np.dot(g, g))
