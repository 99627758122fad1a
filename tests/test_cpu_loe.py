"""The LOE restatement (tests/loe_ref.py) that the device tests trust: its two
forms agree, the known answers hold, and the sample grid is the stated one."""
import numpy as np
import pytest

import loe_ref as R


@pytest.mark.parametrize("H,W,sample", R.SMALL)
def test_pairwise_and_histogram_forms_agree(H, W, sample):
    x, e = R.pair(H, W, seed=3)
    d1, n1, _ = R.loe(x, e, sample, pairs=True)
    d2, n2, v = R.loe(x, e, sample)
    assert n1 == n2 and d1 == d2 and d1 > 0
    assert v == d2 / n2


def test_identical_and_monotone_maps_give_zero():
    x, _ = R.pair(37, 53, seed=4)
    assert R.loe(x, x.copy())[0] == 0
    a = R.lightness(x, 0)
    assert a.max() < 128
    b = 2 * a + 1  # strictly increasing in L
    assert R.count_hist(a, b) == 0 and R.count_pairs(a, b) == 0


def test_reversed_permutation():
    """16 x 16, the 256 lightness values a permutation of 0..255 and enh = 1 - low
    (k / 255 values: exact): every ordered pair of distinct pixels is reversed."""
    perm = np.random.default_rng(5).permutation(256).reshape(16, 16)
    low = np.repeat((perm.astype(np.float32) / np.float32(255))[None], 3, axis=0)
    enh = np.repeat(((255 - perm).astype(np.float32) / np.float32(255))[None], 3, axis=0)
    assert np.array_equal(R.u8(low)[0], perm) and np.array_equal(R.u8(enh)[0], 255 - perm)
    for pairs in (False, True):
        D, N, v = R.loe(low, enh, 50, pairs=pairs)
        assert (D, N, v) == (256 * 255, 256, 255.0)


def test_constant_images_give_zero():
    low = np.full((3, 20, 30), 0.25, np.float32)
    enh = np.full((3, 20, 30), 0.75, np.float32)
    for pairs in (False, True):
        assert R.loe(low, enh, 50, pairs=pairs) == (0, 600, 0.0)


def test_grid():
    r, c = R.grid(120, 200, 50)
    assert (len(r), len(c)) == (50, 83)
    assert r[0] == 1 and r[-1] == (99 * 120) // 100 and c[-1] == (165 * 200) // 166 and c.max() < 200
    r, c = R.grid(96, 64, 16)
    assert (len(r), len(c)) == (24, 16) and r[0] == 2 and c[0] == 2
    for H, W, s in ((8, 8, 50), (50, 70, 50), (37, 53, 0), (300, 200, 0)):
        r, c = R.grid(H, W, s)
        assert np.array_equal(r, np.arange(H)) and np.array_equal(c, np.arange(W))
    r, c = R.grid(51, 5000, 50)  # a long strip: h stays >= 1 and every index is inside
    assert len(r) == 50 and len(c) == (5000 * 50 + 25) // 51 and c.max() < 5000 and (np.diff(c) >= 0).all()


def test_cast_truncates_and_clamps():
    v = np.array([-0.5, 0.0, 0.999 / 255, 1.0 / 255, 0.5, 1.0, 1.5], np.float32)
    assert R.u8(v).tolist() == [0, 0, 0, 1, 127, 255, 255]
