"""Float64 numpy restatement of the paired training terms (csrc/train_paired.hip,
upr_t_loss_paired), for the tests: the Charbonnier reconstruction term, 1 - mean
SSIM (the SSIM of metrics_ref.sums_hist: 11 x 11 box / 121 over a zero border,
C1 = 0.01^2, C2 = 0.03^2) and their closed-form gradient w.r.t. the enhanced
image.  Box windows are direct sums of shifted slices (metrics_ref.box_sum).
No scipy.  `torch_terms` is the same definition in torch, for autograd (float64:
the check of the closed form; float32: the plain-fp32 restatement the device
error is measured against).  Test infrastructure, not product code."""
import numpy as np

from metrics_ref import box_sum

C1, C2 = 0.01 ** 2, 0.03 ** 2
WIN, RAD, NWIN = 11, 5, 121.0
EPS = 1e-3
# the shapes of the op-level tests: the window larger than the image; one window row; one tile row;
# several ragged tiles with W % 4 != 0 and two images; the kernel's 16 x 32 tile and a pixel more each way
SHAPES = ((2, 7, 9), (1, 11, 64), (1, 16, 16), (2, 37, 53), (1, 16, 32), (1, 17, 33))
KINDS = ("noise", "smooth", "near_constant", "dark")


def f32_eps(eps=EPS):
    """The eps the C ABI receives (a float argument), as a python float."""
    return float(np.float32(eps))


def _box(a):
    return box_sum(np.pad(a, RAD), WIN)


def _moments(x, y):
    mx, my = _box(x) / NWIN, _box(y) / NWIN
    return mx, my, _box(x * x) / NWIN, _box(y * y) / NWIN, _box(x * y) / NWIN


def ssim_map(x, y):
    """x, y float64 [H,W] -> the SSIM map [H,W]."""
    mx, my, exx, eyy, exy = _moments(x, y)
    A1, A2 = 2 * mx * my + C1, 2 * (exy - mx * my) + C2
    B1, B2 = mx * mx + my * my + C1, (exx - mx * mx) + (eyy - my * my) + C2
    return (A1 * A2) / (B1 * B2)


def terms(enh, target, eps=EPS):
    """enh, target [B,3,H,W] -> (reconstruction, ssim_loss) python floats, float64 arithmetic."""
    x, y = np.asarray(enh, np.float64), np.asarray(target, np.float64)
    rec = np.sqrt((x - y) ** 2 + eps * eps).mean()
    s = 0.0
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            s += ssim_map(x[b, c], y[b, c]).sum()
    return float(rec), float(1.0 - s / x.size)


def grad(enh, target, w_rec=1.0, w_ssim=1.0, eps=EPS):
    """d(w_rec * reconstruction + w_ssim * ssim_loss) / d enh, float64 [B,3,H,W], closed form."""
    x, y = np.asarray(enh, np.float64), np.asarray(target, np.float64)
    n = float(x.size)
    d = x - y
    g = w_rec * d / np.sqrt(d * d + eps * eps) / n
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            xc, yc = x[b, c], y[b, c]
            mx, my, exx, eyy, exy = _moments(xc, yc)
            A1, A2 = 2 * mx * my + C1, 2 * (exy - mx * my) + C2
            B1, B2 = mx * mx + my * my + C1, (exx - mx * mx) + (eyy - my * my) + C2
            S = A1 * A2 / (B1 * B2)
            a = 2 * my * (A2 - A1) / (B1 * B2) - 2 * mx * S / B1 + 2 * mx * S / B2
            bq = -S / B2
            cq = 2 * A1 / (B1 * B2)
            g[b, c] -= w_ssim * (_box(a) + 2 * xc * _box(bq) + yc * _box(cq)) / (NWIN * n)
    return g


def torch_terms(enh, target, eps=EPS):
    """The same definition on torch tensors of any float dtype (avg_pool2d with
    zero padding counted in the divisor is the box / 121) -> (reconstruction, ssim_loss) tensors."""
    import torch
    import torch.nn.functional as F

    def box(t):
        return F.avg_pool2d(t, WIN, stride=1, padding=RAD, count_include_pad=True)

    x, y = enh, target
    rec = torch.sqrt((x - y) ** 2 + eps * eps).mean()
    mx, my = box(x), box(y)
    exx, eyy, exy = box(x * x), box(y * y), box(x * y)
    A1, A2 = 2 * mx * my + C1, 2 * (exy - mx * my) + C2
    B1, B2 = mx * mx + my * my + C1, (exx - mx * mx) + (eyy - my * my) + C2
    return rec, 1.0 - ((A1 * A2) / (B1 * B2)).mean()


def make_pair(kind, shape, seed=0):
    """(enh, target) float32 numpy [B,3,H,W] of one of KINDS."""
    B, H, W = shape
    r = np.random.default_rng(1000 * KINDS.index(kind) + seed + 7 * H + W)
    u = r.random((B, 3, H, W))
    if kind == "noise":
        x, y = u, r.random((B, 3, H, W))
    elif kind == "smooth":
        p = np.pad(u, ((0, 0), (0, 0), (3, 3), (3, 3)), mode="edge")
        x = np.zeros_like(u)
        for i in range(7):
            for j in range(7):
                x += p[:, :, i:i + H, j:j + W]
        x /= 49.0
        y = 0.9 * x + 0.05 + 0.01 * r.standard_normal((B, 3, H, W))
    elif kind == "near_constant":
        x, y = 0.5 + 1e-3 * u, np.full((B, 3, H, W), 0.5)
    elif kind == "dark":
        x, y = 0.02 * u, r.random((B, 3, H, W))
    else:
        raise ValueError(kind)
    return x.astype(np.float32), y.astype(np.float32)
