"""Host packer of the weights-split-once form (upr_pack_split_w_f32, no device):
the fp16 planes W_hi = fp16(w s_n), W_lo = fp16(w s_n - W_hi) in MFMA k-slot
order, the exact power-of-two channel scale over both K-segments, and the
reconstruction (W_hi + W_lo) / s_n = w to 2^-21 of the row's largest weight
(W_hi carries 11 bits, W_lo 11 more of the remainder: 2^-22 of the element,
doubled for the fp16 subnormals of the smallest remainders)."""
import ctypes

import numpy as np
import pytest
import torch


def kslot(c):
    """Position of channel c (0..31) of a 32-deep K step within a 32-half plane:
    lane group g = (c % 16) // 4 holds channels 4g..4g+3 and 16+4g..16+4g+3."""
    return ((c % 16) // 4) * 8 + (c // 16) * 4 + c % 4


PERM = np.array([kslot(c) for c in range(32)])


def unpack(blob, Co, K):
    """blob -> (W_hi, W_lo) as float64 [Co][K] in plain k order, 1/s_n [Co]."""
    planes = blob[:Co * K * 4].view(np.float16).reshape(Co, K // 32, 2, 32).astype(np.float64)
    off = (Co * K * 4 + 255) // 256 * 256
    assert blob.size == off + 4 * Co
    inv_s = blob[off:off + 4 * Co].view(np.float32).astype(np.float64)
    hi = planes[:, :, 0, :][:, :, PERM].reshape(Co, K)
    lo = planes[:, :, 1, :][:, :, PERM].reshape(Co, K)
    return hi, lo, inv_s


def test_kslot_permutation_inverts():
    assert sorted(PERM.tolist()) == list(range(32))
    inv = np.argsort(PERM)
    assert np.array_equal(PERM[inv], np.arange(32)) and np.array_equal(inv[PERM], np.arange(32))
    # a lane group's 8 slots are the two 4-channel chunks g and 4 + g of the row
    for g in range(4):
        assert inv[8 * g:8 * g + 8].tolist() == list(range(4 * g, 4 * g + 4)) + list(range(16 + 4 * g, 20 + 4 * g))


def check_rows(w_all, hi, lo, inv_s):
    for n in range(w_all.shape[0]):
        mant, _ = np.frexp(inv_s[n])
        assert mant == 0.5, "scale is a power of two"
        mx = np.abs(w_all[n]).max()
        if mx == 0:
            assert inv_s[n] == 1.0 and not hi[n].any() and not lo[n].any()
            continue
        assert 2.0 ** 14 <= mx / inv_s[n] < 2.0 ** 15
        rec = (hi[n] + lo[n]) * inv_s[n]
        assert np.abs(rec - w_all[n]).max() <= 2.0 ** -21 * mx
        # W_hi is the fp16 rounding of the scaled weight itself
        assert np.array_equal(hi[n], (w_all[n] / inv_s[n]).astype(np.float16).astype(np.float64))


@pytest.mark.parametrize("Co,Ci,k", [(64, 32, 3), (128, 64, 3), (64, 64, 1)])
def test_pack_split_w_one_segment(Co, Ci, k):
    from upr import runtime
    g = torch.Generator().manual_seed(5 + Co + Ci)
    w = torch.randn(Co, Ci, k, k, generator=g) * torch.logspace(-6, 3, Co).view(Co, 1, 1, 1)
    w[3] = 0.0  # an all-zero channel keeps scale 1
    wp = runtime.pack_conv_weight(w)
    hi, lo, inv_s = unpack(runtime.pack_split_w(wp, k, k).numpy(), Co, k * k * Ci)
    check_rows(wp.double().numpy(), hi, lo, inv_s)


def test_pack_split_w_two_segments_share_one_scale():
    """64 -> 64 3x3 plus a 1x1 over 32 channels (a projecting shortcut): K = 576 +
    32, one s_n per row from the larger of the two segments' maxima."""
    from upr import runtime
    g = torch.Generator().manual_seed(9)
    Co = 64
    w = torch.randn(Co, 64, 3, 3, generator=g) * 0.05
    w2 = torch.randn(Co, 32, generator=g) * 0.05
    w2[:32] *= 40.0   # rows whose largest weight is in the shortcut
    w2[32:] *= 0.25   # and rows whose largest weight is in the 3x3
    w[7] = 0.0
    w2[7] = 0.0
    wp = runtime.pack_conv_weight(w)
    hi, lo, inv_s = unpack(runtime.pack_split_w(wp, 3, 3, w2).numpy(), Co, 576 + 32)
    w_all = torch.cat([wp, w2], 1).double().numpy()
    assert (np.abs(w_all[:7, 576:]).max(1) > np.abs(w_all[:7, :576]).max(1)).all()
    assert (np.abs(w_all[32:, 576:]).max(1) < np.abs(w_all[32:, :576]).max(1)).all()
    check_rows(w_all, hi, lo, inv_s)


def test_pack_split_w_bad_arguments_return_zero():
    from upr import _lib as L
    lib = L.lib()
    w = np.zeros(128 * 9 * 64, np.float32)
    p = ctypes.c_void_p(w.ctypes.data)
    ok = lib.upr_pack_split_w_f32(p, 64, 64, 3, 3, None, 0, None, 0)
    assert ok == 64 * 576 * 4 + 64 * 4
    assert lib.upr_pack_split_w_f32(p, 64, 64, 3, 3, p, 32, None, 0) == (64 * 608 * 4 + 255) // 256 * 256 + 64 * 4
    assert lib.upr_pack_split_w_f32(None, 64, 64, 3, 3, None, 0, None, 0) == 0
    assert lib.upr_pack_split_w_f32(p, 32, 64, 3, 3, None, 0, None, 0) == 0     # Cout % 64
    assert lib.upr_pack_split_w_f32(p, 64, 16, 3, 3, None, 0, None, 0) == 0     # Cin % 32
    assert lib.upr_pack_split_w_f32(p, 64, 64, 0, 3, None, 0, None, 0) == 0
    assert lib.upr_pack_split_w_f32(p, 64, 64, 3, 3, p, 16, None, 0) == 0       # C2 % 32
    assert lib.upr_pack_split_w_f32(p, 64, 64, 3, 3, None, 32, None, 0) == 0    # C2 without w2
    assert lib.upr_pack_split_w_f32(p, 64, 64, 3, 3, p, 0, None, 0) == 0        # w2 without C2
    # a buffer that is too small is left alone
    out = np.full(16, 7, np.uint8)
    assert lib.upr_pack_split_w_f32(p, 64, 64, 3, 3, None, 0, ctypes.c_void_p(out.ctypes.data), 16) == ok
    assert (out == 7).all()
