"""Host packer of the split-fp16 conv weights (upr_pack_split_f32, no device):
layout of the two K-segments, the exact power-of-two channel scale and the
reconstruction (W_hi + W_lo) / s = w to 2^-21 of the channel's largest weight."""
import numpy as np
import torch


def test_pack_split_weight_layout_and_reconstruction():
    from upr import runtime
    g = torch.Generator().manual_seed(0)
    Co, Ci, k = 8, 64, 3
    w = torch.randn(Co, Ci, k, k, generator=g) * torch.logspace(-6, 3, Co).view(Co, 1, 1, 1)
    w[3] = 0.0  # an all-zero channel keeps scale 1
    blob = runtime.pack_split_weight(w).numpy()
    taps = k * k
    Kpad = 3 * taps * Ci
    W = blob[:Co * Kpad * 2].view(np.float16).reshape(Co, Kpad).astype(np.float64)
    off = (Co * Kpad * 2 + 255) // 256 * 256
    scale = blob[off:off + 4 * Co].view(np.float32).astype(np.float64)
    assert blob.size == off + 4 * Co
    A = W[:, :taps * 2 * Ci].reshape(Co, taps, 2, Ci)      # per tap [W_hi | W_hi 2^-11]
    Bseg = W[:, taps * 2 * Ci:].reshape(Co, taps, Ci)      # W_lo
    hi, hi_s, lo = A[:, :, 0], A[:, :, 1], Bseg
    wd = w.double().numpy().transpose(0, 2, 3, 1).reshape(Co, taps, Ci)
    for n in range(Co):
        mant, ex = np.frexp(scale[n])
        assert mant == 0.5, "scale is a power of two"
        mx = np.abs(wd[n]).max()
        if mx == 0:
            assert scale[n] == 1.0 and not W[n].any()
            continue
        assert 2.0 ** 14 <= mx / scale[n] < 2.0 ** 15
        rec = (hi[n] + lo[n]) * scale[n]
        assert np.abs(rec - wd[n]).max() <= 2.0 ** -21 * mx
        # the lo-activation operand: W_hi 2^-11, exact wherever it stays a normal fp16 value
        normal = np.abs(hi[n]) >= 2.0 ** -3
        assert np.array_equal(hi_s[n][normal], hi[n][normal] / 2048.0)


def test_pack_split_weight_rejects_unsupported_channels():
    import pytest
    from upr import runtime
    with pytest.raises(ValueError):
        runtime.pack_split_weight(torch.zeros(8, 32, 3, 3))
