"""Self-check of the float64 op reference oracle/loss_ops.py and of the inputs
tests/test_gpu_loss_ops.py gives the kernels (tests/loss_ops_cases.py).

The numpy ops against torch in double: both sides are float64, so they agree
to 1e-12 relative (of the largest reference magnitude).  The frequency
composition (G of freq on fft2(enh), brought back by H W Re(ifft2(G)), is
autograd's gradient of oracle/train.py::frequency_loss) holds to 1e-10: the
FFT round trip costs a few 1e-13.  The input conditions are conditions on the
reference, asserted here and again at the top of the GPU tests."""
import numpy as np
import pytest
import torch

import loss_ops_cases as K
from oracle import loss_ops as O
from oracle import train as T

REL = 1e-12


def _agree(a, b, what, rel=REL):
    a = np.asarray(a)
    b = b.detach().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max()
    tol = rel * max(np.abs(b).max(), 1e-300)
    assert err <= tol, f"{what}: max|d| {err:.3e} > {tol:.3e}"


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).requires_grad_(grad)


@pytest.mark.parametrize("H,W", K.FREQ_SHAPES)
def test_freq_matches_autograd_double(H, W):
    ze, zl = (torch.view_as_complex(z.double()) for z in K.freq_inputs(H, W))
    w_high, w_low, scale = K.FREQ_W[0], K.FREQ_W[1], 0.125
    zt = ze.clone().requires_grad_(True)
    hm, lm = (m.double() for m in T.freq_masks(H, W))
    w = O.f32(w_high) * hm + O.f32(w_low) * lm
    s = (w * (zt.abs() - zl.abs()) ** 2).sum()
    (O.f32(scale) * s).backward()
    val, G = O.freq(ze.numpy(), zl.numpy(), H, W, scale, w_high, w_low)
    _agree(np.float64(val), s, "freq sum")
    _agree(G, zt.grad, "freq G")
    zero = ze.numpy() == 0
    assert zero.sum() == 3 and not G[zero].any() and np.isfinite(G).all()
    assert np.array_equal(O.freq_low_mask(H, W), lm.numpy().astype(bool))


def test_freq_lattice_points_on_the_circle():
    assert K.check_freq_lattice(20, 20) == 12  # 4 on the axes, 8 of (3, 4, 5)
    # a '<' mask differs from '<=' exactly there, and w_high != w_low makes it show
    assert K.FREQ_W[0] != K.FREQ_W[1]


@pytest.mark.parametrize("B,H,W", [(1, 4, 4), (2, 20, 20), (2, 17, 23)])
def test_freq_composes_to_frequency_loss_gradient(B, H, W):
    rng = np.random.default_rng(21)
    enh, low = rng.uniform(0, 1, (B, 3, H, W)), rng.uniform(0, 0.4, (B, 3, H, W))
    w_high, w_low = 1.0, 0.5
    et = _t(enh, True)
    loss = T.frequency_loss(et, _t(low), w_high, w_low)
    loss.backward()
    n = B * 3 * H * W
    Ze, Zl = np.fft.fft2(enh.reshape(B * 3, H, W)), np.fft.fft2(low.reshape(B * 3, H, W))
    # scale = 1 / n is not an fp32 number: give freq scale 1 and divide after
    val, G = O.freq(Ze, Zl, H, W, 1.0, w_high, w_low)
    _agree(np.float64(val / n), loss, "frequency loss", 1e-10)
    _agree((H * W * np.fft.ifft2(G).real / n).reshape(B, 3, H, W), et.grad, "frequency gradient", 1e-10)


def test_mse_vgg_and_scalar_helpers_match_torch_double():
    rng = np.random.default_rng(22)
    a, b = rng.standard_normal(1001), rng.standard_normal(1001)
    at = _t(a, True)
    m = torch.nn.functional.mse_loss(at, _t(b))
    (m * 1001 * O.f32(0.37)).backward()
    val, g = O.mse(a, b, 0.37)
    _agree(np.float64(val), m, "mse")
    _agree(g, at.grad, "mse g")

    x, gy, gx0 = rng.uniform(0, 1, (2, 3, 5, 7)), rng.standard_normal((2, 5, 7, 3)), rng.standard_normal((2, 3, 5, 7))
    xt = _t(x, True)
    mean = torch.from_numpy(O.VGG_MEAN32).view(1, 3, 1, 1)
    std = torch.from_numpy(O.VGG_STD32).view(1, 3, 1, 1)
    yt = ((xt - mean) / std).permute(0, 2, 3, 1)
    (yt * _t(gy)).sum().backward()
    _agree(O.vgg_norm(x), yt, "vgg_norm")
    _agree(O.vgg_norm_bwd(gy, gx0), xt.grad + _t(gx0), "vgg_norm_bwd")
    # the kernel's constants are the reference's, rounded to fp32
    assert np.abs(O.VGG_MEAN32 - T.VGG_MEAN).max() < 2e-8 and np.abs(O.VGG_STD32 - T.VGG_STD).max() < 1e-8

    z = rng.standard_normal(50) + 1j * rng.standard_normal(50)
    g0 = rng.standard_normal(50)
    _agree(O.add_real(z, g0, 0.3), _t(g0) + O.f32(0.3) * torch.from_numpy(z).real, "add_real")
    acc = rng.standard_normal(9) * 100
    _agree(O.scale_acc(acc, 1 / 3), _t(acc) * O.f32(1 / 3), "scale_acc")
    terms = rng.uniform(0.1, 2, 9)
    w = [O.f32(v) for v in (10.0, 0.5, 1.0, 0.1, 1.0, 0.5)]
    t = _t(terms)
    want = w[0] * t[0] + t[8] * t[1] + w[1] * t[2] + w[2] * t[3] + w[3] * t[4] + w[4] * t[5] + w[5] * t[6]
    _agree(np.float64(O.loss_total(terms, 10.0, 0.5, 1.0, 0.1, 1.0, 0.5)), want, "loss_total")
    assert O.loss_total(terms, 10.0, 0.5, 1.0, 0.1, 1.0, 0.0) == pytest.approx(float(want) - w[5] * terms[6], rel=REL)
    gv = rng.standard_normal(777) * 10
    _agree(np.float64(O.sqsum(gv, 2.5)), (_t(gv) ** 2).sum() + 2.5, "sqsum")


@pytest.mark.parametrize("C,H,W", K.TEXTURE_CASES + [(3, 2, 9), (1, 9, 2)])
def test_sobel_magnitude_matches_edge_map(C, H, W):
    """The paired-tap Sobel is oracle/train.py's edge_map to rounding; on the
    non-degenerate cases the edge-density share is texture_complexity's; on a
    2-sample axis that direction's derivative, on 2 x 2 the magnitude, is
    exactly 0."""
    img = (K.texture_inputs(C, H, W) if (C, H, W) in K.TEXTURE_SEEDS else
           torch.rand(2, C, H, W, generator=torch.Generator().manual_seed(5))).double()
    e = O.sobel_magnitude(img.numpy())
    ref = T.edge_map(img)[:, 0]
    assert np.abs(e - ref.numpy()).max() <= REL * max(float(ref.max()), 1.0)
    _agree(O.texture_complexity(img.numpy(), 0), T.texture_complexity(img, "tv"), "tv")
    if H == 2 and W == 2:
        assert not e.any() and not O.texture_complexity(img.numpy(), 1).any()
    else:
        assert not e[:, [0, 0, -1, -1], [0, -1, 0, -1]].any()  # the four corners: both derivatives mirror away
        if (C, H, W) in K.TEXTURE_SEEDS:
            K.check_edge_margin(img.numpy())
            # (texture_complexity's share is a float32 mean of booleans: the same count)
            assert np.array_equal(O.texture_complexity(img.numpy(), 1).astype(np.float32),
                                  T.texture_complexity(img, "edge_density").numpy())


@pytest.mark.parametrize("B,H,W,patch,CI", K.PIXEL_SHAPES)
def test_pixel_input_conditions(B, H, W, patch, CI):
    """Exposure patches on both sides of the target and clear of it, no Sobel
    magnitude near the edge-density threshold; exposure_patches is the
    exposure term's own decomposition."""
    d = K.check_pixel_inputs(B, H, W, patch, CI)
    weights, w_smooth, prm = K.WEIGHTINGS["mixed"]
    prm = dict(prm, patch=patch, dynamic_smooth=0)
    terms, wsm, g_enh, g_illu, g_refl = O.pixel_terms(d["low"], d["enh"], d["illu"], d["refl"], weights, prm, w_smooth, 0)
    P, Tg = O.exposure_patches(d["low"].numpy(), d["enh"].numpy(), patch, prm["base_exposure"])
    assert abs(np.abs(P - Tg).mean() - terms[0]) <= REL * terms[0]
    assert wsm == O.f32(w_smooth) and g_enh.shape == (B, 3, H, W) and g_illu.shape == (B, CI, H, W)
    # the exposure gradient's sign really goes both ways, and is 0 on the remainder
    ge = O.pixel_terms(d["low"], d["enh"], d["illu"], d["refl"], (1, 0, 0, 0), {"patch": patch, "dynamic_smooth": 0},
                       0.0, 0)[2]
    if P.size > 1:
        assert (ge > 0).any() and (ge < 0).any()
    assert not ge[:, :, (H // patch) * patch:].any() and not ge[:, :, :, (W // patch) * patch:].any()


@pytest.mark.parametrize("B,H,W,patch,CI", K.DYNAMIC_SHAPES)
def test_dynamic_weight_reaches_both_clamps(B, H, W, patch, CI):
    d = K.pixel_inputs(B, H, W, patch, CI)
    K.check_dynamic_weights(d["low"])
    for texture in (0, 1):
        got = [O.pixel_terms(d["low"], d["enh"], d["illu"], d["refl"], (1, 1, 1, 1), {"patch": patch}, w, texture)[1]
               for w in K.DYNAMIC_W_SMOOTH]
        assert got[0] == 0.1 and 0.1 < got[1] < 5.0 and got[2] == 5.0


def test_pixel_terms_fp32_restatement_is_close():
    """dtype = float32 is the same computation in fp32: close to, and not
    identical with, the float64 one."""
    s = (2, 37, 53, 12, 1)
    d = K.pixel_inputs(*s)
    weights, w_smooth, prm = K.WEIGHTINGS["mixed"]
    prm = dict(prm, patch=12, dynamic_smooth=0)
    a = O.pixel_terms(d["low"], d["enh"], d["illu"], d["refl"], weights, prm, w_smooth, 0)
    b = O.pixel_terms(d["low"], d["enh"], d["illu"], d["refl"], weights, prm, w_smooth, 0, torch.float32)
    assert np.abs(a[0] - b[0]).max() <= 1e-5 * np.abs(a[0]).max() and not np.array_equal(a[0], b[0])
    for x, y in zip(a[2:], b[2:]):
        assert np.abs(x - y).max() <= 1e-4 * np.abs(x).max()
