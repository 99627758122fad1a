"""Case tables and seeded CPU input builders of the loss op tests
(test_cpu_loss_ops_oracle.py, test_gpu_loss_ops.py): both import this module, so
the CPU test checks the input conditions on exactly the inputs the GPU test
gives the kernels.  The conditions are on the float64 reference, never on a
kernel's output; the seeds below were picked on the CPU so that they hold
(most seeds do), and check_*() assert them: no case is filtered."""
import functools

import numpy as np
import torch

from oracle import loss_ops as O

# (B, H, W, patch, CI) of upr_t_loss_pixel_p.  Banded: loss_pass1_band_kernel
# (patch a power of two <= 64 dividing H and W; 256 columns an x-block);
# generic: loss_pass1_kernel.  Chunks: clamp(HW / 4096, 1, 128) of the generic
# pass 1, pass 2 and the edge-density passes.
PIXEL_SHAPES = [
    (1, 2, 2, 2, 1),        # smallest legal image, reflect pad of a 2-sample axis, HW - 1 = 3
    (2, 16, 16, 16, 1),     # banded, one patch an image, W < one wave
    (1, 8, 24, 2, 1),       # banded, 2-lane patches
    (1, 8, 24, 1, 3),       # banded, patch = pixel, empty shuffle loop
    (1, 32, 272, 16, 1),    # banded, second x-block holds 16 columns
    (2, 64, 64, 64, 3),     # banded at the patch limit (rowred[64][4] full, whole-wave shuffle), CI = 3
    (2, 37, 53, 12, 1),     # generic, remainders on both axes (1 row, 5 columns), one chunk
    (1, 71, 123, 12, 3),    # generic, 2 chunks of 4367 pixels, boundary inside row 35, CI = 3
    (1, 128, 136, 128, 1),  # patch > 64 -> generic, 4 chunks, 8 remainder columns
]
# the two shapes that also run dynamic_smooth = 1 (texture 0 and 1): per-image
# thresholds at B = 2, and the edge-density passes over 2 chunks
DYNAMIC_SHAPES = [(2, 37, 53, 12, 1), (1, 71, 123, 12, 3)]
DYNAMIC_W_SMOOTH = (0.05, 1.0, 10.0)  # the 0.1 clamp, the unclamped branch, the 5.0 clamp

MIXED_PARAMS = {"base_exposure": 0.5, "smooth_lambda": 5.0, "smooth_alpha": 0.5, "decouple_lambda": 0.3}
# name -> ((w_exp, w_col, w_spa, w_dec), w_smooth, UprLossParams overrides); dynamic_smooth = 0
WEIGHTINGS = {
    "exp": ((1.0, 0.0, 0.0, 0.0), 0.0, {}),
    "col": ((0.0, 1.0, 0.0, 0.0), 0.0, {}),
    "spa": ((0.0, 0.0, 1.0, 0.0), 0.0, {}),
    "dec": ((0.0, 0.0, 0.0, 1.0), 0.0, {}),
    "smooth": ((0.0, 0.0, 0.0, 0.0), 1.0, {}),
    # distinct non-default weights and module arguments: a swapped argument shows
    "mixed": ((7.0, 0.3, 1.7, 0.45), 2.5, MIXED_PARAMS),
}
BASES = (O.DEFAULT_PARAMS["base_exposure"], MIXED_PARAMS["base_exposure"])

PIXEL_SEEDS = {s: 1 for s in PIXEL_SHAPES}

# upr_t_texture_complexity: (C, H, W), B = 2
TEXTURE_CASES = [(C, H, W) for C in (1, 3, 4) for (H, W) in ((2, 2), (37, 53), (71, 123))]
TEXTURE_SEEDS = {c: 1 for c in TEXTURE_CASES}
TEXTURE_SEEDS.update({(1, 71, 123): 2, (4, 37, 53): 2})  # seed 1 leaves a pixel within EDGE_MARGIN of the threshold

EDGE_MARGIN = 1e-5   # about 80 fp32 ulp: far above the error of the eleven fp32 operations of a Sobel magnitude
PATCH_MARGIN = 1e-3  # |P - T| of every exposure patch


def _patch_levels(gen, B, H, W, patch):
    """[B, 1, H, W] of per-patch levels 0.76 +- (0.04 .. 0.16), as many above
    as below (a permutation of alternating signs); the remainder rows and
    columns beyond floor(H / patch) x floor(W / patch) get levels of their own."""
    ph, pw = -(-H // patch), -(-W // patch)
    n = B * ph * pw
    sign = (torch.arange(n) % 2).float() * 2 - 1
    sign = sign[torch.randperm(n, generator=gen)]
    lev = (0.76 + sign * (0.04 + 0.12 * torch.rand(n, generator=gen))).view(B, 1, ph, pw)
    return lev.repeat_interleave(patch, 2).repeat_interleave(patch, 3)[:, :, :H, :W]


@functools.lru_cache(maxsize=None)
def pixel_inputs(B, H, W, patch, CI):
    """fp32 CPU inputs of one pixel-loss shape: low = rand 0.4, illu = rand 0.8
    + 0.1, refl = rand, enh = per-patch level + a channel tint + small noise.
    Uniform random enh would put nearly every patch on one side of the
    exposure target (about 0.76); the tint keeps the colour term's channel
    means apart."""
    gen = torch.Generator().manual_seed(PIXEL_SEEDS[(B, H, W, patch, CI)])
    low = torch.rand(B, 3, H, W, generator=gen) * 0.4
    illu = torch.rand(B, CI, H, W, generator=gen) * 0.8 + 0.1
    refl = torch.rand(B, 3, H, W, generator=gen)
    tint = torch.tensor([-0.05, 0.0, 0.04]).view(1, 3, 1, 1)
    enh = _patch_levels(gen, B, H, W, patch) + tint + (torch.rand(B, 3, H, W, generator=gen) - 0.5) * 0.04
    return {"low": low, "enh": enh, "illu": illu, "refl": refl}


@functools.lru_cache(maxsize=None)
def texture_inputs(C, H, W):
    gen = torch.Generator().manual_seed(TEXTURE_SEEDS[(C, H, W)])
    return torch.rand(2, C, H, W, generator=gen)


def check_exposure(d, B, H, W, patch):
    """At both exposure bases the tests use: every patch mean is at least
    PATCH_MARGIN from the float64 target, and (more than one patch) at least a
    quarter of the patches lie above it and a quarter below."""
    for base in BASES:
        P, T = O.exposure_patches(d["low"].numpy(), d["enh"].numpy(), patch, base)
        assert np.abs(P - T).min() >= PATCH_MARGIN, (B, H, W, patch, base, np.abs(P - T).min())
        if P.size > 1:
            above, below = (P > T).sum(), (P < T).sum()
            assert 4 * above >= P.size and 4 * below >= P.size, (B, H, W, patch, base, above, below, P.size)


def check_edge_margin(img):
    """No pixel's float64 Sobel magnitude is within EDGE_MARGIN (relative) of
    1.5 x its image's mean.  An image with two samples on both axes is the
    degenerate case: the reflect pad makes every Sobel tap equal to its mirror
    tap, magnitude and threshold are 0 and 0 > 0 counts nothing (see
    oracle/loss_ops.py::sobel_magnitude); no margin exists, and the condition
    there is that the reference magnitude is exactly 0."""
    img = np.asarray(img, dtype=np.float64)
    if img.shape[2] == 2 and img.shape[3] == 2:
        assert not O.sobel_magnitude(img).any(), "the 2 x 2 Sobel magnitude must be exactly 0"
        return
    m = O.edge_margin(img)
    assert m >= EDGE_MARGIN, (img.shape, m)


def check_pixel_inputs(B, H, W, patch, CI):
    d = pixel_inputs(B, H, W, patch, CI)
    check_exposure(d, B, H, W, patch)
    check_edge_margin(d["low"].numpy())
    return d


def check_dynamic_weights(low):
    """DYNAMIC_W_SMOOTH reaches the lower clamp, the unclamped branch and the
    upper clamp of w_smooth (1 - 0.8 complexity) with both texture methods,
    none of them within 1e-3 of a clamp's edge."""
    for method in (0, 1):
        tc = float(O.texture_complexity(low.numpy(), method).mean())
        raw = [O.f32(w) * (1.0 - 0.8 * tc) for w in DYNAMIC_W_SMOOTH]
        assert raw[0] < 0.1 - 1e-3 and 0.1 + 1e-3 < raw[1] < 5.0 - 1e-3 and raw[2] > 5.0 + 1e-3, (method, tc, raw)


# frequency: (H, W); radius min(H, W) // 4 around (H // 2, W // 2)
FREQ_SHAPES = [
    (20, 20),  # radius 5: the 3-4-5 lattice points (and the four axis points) exactly on the circle
    (17, 23),  # odd sizes, radius 4
    (4, 4),    # the smallest: radius 1
]
FREQ_BC = 6
FREQ_W = (0.7, 0.2)  # w_high != w_low and neither a default: a wrong mask shows on the circle


@functools.lru_cache(maxsize=None)
def freq_inputs(H, W):
    """Interleaved complex fp32 spectra [BC, H, W, 2] ~ N(0, 1) with a few Ze
    entries exactly 0 (one of them on the circle)."""
    gen = torch.Generator().manual_seed(100 * H + W)
    ze, zl = torch.randn(FREQ_BC, H, W, 2, generator=gen), torch.randn(FREQ_BC, H, W, 2, generator=gen)
    ze[0, 0, 0] = 0.0
    ze[1, H // 2, W // 2 + min(H, W) // 4] = 0.0
    ze[FREQ_BC - 1, H - 1, W - 1] = 0.0
    return ze, zl


def check_freq_lattice(H, W):
    """(20, 20) really has lattice points on the circle, off the axes too."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d2 = (x - W // 2) ** 2 + (y - H // 2) ** 2
    on = d2 == (min(H, W) // 4) ** 2
    assert on.sum() >= 4 and O.freq_low_mask(H, W)[on].all()
    return int(on.sum())
