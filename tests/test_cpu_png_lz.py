"""Device PNG encoder, match mode "lz": what can be checked without a device -- the CLI choice,
the harness's encoder check, the `matches` argument, upr_png_bound_ex against upr_png_bound,
the argument checks of upr_png_encode_ex."""
import ctypes

import pytest
import torch

from upr import _lib as L

SHAPES = [(64, 200, 16), (64, 200, 1), (64, 100, 64), (1, 1, 1), (1, 4099, 1), (300, 1, 7), (512, 512, 16),
          (37, 53, 3), (16, 30000, 16)]


def _bound(fn, *args):
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    rc = getattr(L.lib(), fn)(*args, ctypes.byref(nb), ctypes.byref(ns))
    return rc, nb.value, ns.value


def test_match_constants():
    assert L.PNG_MATCHES == {"none": 0, "lz": 1}


def test_png_encoder_flag_takes_device_lz():
    import main as cli
    p = cli.build_parser()
    assert p.parse_args(["--mode", "enhance", "--png_encoder", "device_lz"]).png_encoder == "device_lz"
    assert p.parse_args(["--mode", "predict", "--png_encoder", "device_lz"]).png_encoder == "device_lz"
    assert p.parse_args([]).png_encoder == "host"


def test_harness_accepts_device_lz():
    """save_image gets past the encoder check: what stops a CPU tensor is the device encoder
    itself (a RuntimeError about the device), not the ValueError of an unknown encoder."""
    from enhancers import simple_enhance as se
    assert se.PNG_ENCODERS == ("host", "device", "device_lz")
    se._check_encoder("device_lz")
    with pytest.raises(RuntimeError, match="ROCm"):
        se.save_image(torch.zeros(3, 4, 4), "/nonexistent/x.png", png_encoder="device_lz")
    with pytest.raises(ValueError):
        se.save_image(torch.zeros(3, 4, 4), "/nonexistent/x.png", png_encoder="device_zip")


def test_unknown_matches_value():
    from upr import png
    x = torch.zeros((4, 5, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        png.encode(x, matches="zip")
    with pytest.raises(ValueError):
        png.encode_device(x, matches="zip")
    with pytest.raises(ValueError):
        png.bound(4, 5, matches="zip")
    with pytest.raises(RuntimeError, match="ROCm"):  # a known value gets as far as the device check
        png.encode(x, matches="lz")


@pytest.mark.parametrize("H,W,rps", SHAPES)
def test_bound_ex(H, W, rps):
    from upr import png
    rc0, nb0, ns0 = _bound("upr_png_bound", H, W, rps)
    rc1, nb1, ns1 = _bound("upr_png_bound_ex", H, W, rps, 0)
    rc2, nb2, ns2 = _bound("upr_png_bound_ex", H, W, rps, 1)
    assert rc0 == rc1 == rc2 == L.UPR_OK
    assert (nb1, ns1) == (nb0, ns0)
    assert nb2 == nb0 and ns2 >= ns0 and ns2 % 16 == 0
    # the staged filtered bytes and the parse of every strip have to fit in what is added
    assert ns2 - ns0 >= H * (3 * W + 1)
    assert png.bound(H, W, rps) == png.bound(H, W, rps, "none") == (nb0, ns0)
    assert png.bound(H, W, rps, "lz") == (nb2, ns2)


@pytest.mark.parametrize("match", [0, 1])
def test_bound_ex_refuses_what_bound_refuses(match):
    wmax = (L.UPR_PNG_MAX_STRIP_BYTES // 16 - 1) // 3
    for args in [(2, 3_000_000, 2), (16, wmax, 16), (16, wmax + 1, 16), (40000, 20000, 16), (0, 8, 1), (8, 8, 0),
                 (8, 0, 1), (-1, 8, 1)]:
        assert _bound("upr_png_bound_ex", *args, match)[0] == _bound("upr_png_bound", *args)[0], args
    assert _bound("upr_png_bound_ex", 16, wmax, 16, match)[0] == L.UPR_OK
    assert _bound("upr_png_bound_ex", 16, wmax + 1, 16, match)[0] == L.UPR_ERR_SHAPE
    assert _bound("upr_png_bound_ex", 0, 8, 1, match)[0] == L.UPR_ERR_ARG


def test_bound_ex_null_and_unknown_match():
    lib = L.lib()
    nb = ctypes.c_size_t()
    assert lib.upr_png_bound_ex(8, 8, 4, 1, None, ctypes.byref(nb)) == L.UPR_ERR_ARG
    assert lib.upr_png_bound_ex(8, 8, 4, 1, ctypes.byref(nb), None) == L.UPR_ERR_ARG
    assert _bound("upr_png_bound_ex", 8, 8, 4, -1)[0] == L.UPR_ERR_ARG
    assert _bound("upr_png_bound_ex", 8, 8, 4, 2)[0] == L.UPR_ERR_ARG


def test_encode_ex_args_rejected_without_device():
    lib = L.lib()
    assert lib.upr_png_encode_ex(None, 1, 8, 8, 5, 1, 4, None, 0, None, None, 0, None) == L.UPR_ERR_ARG
    one = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    big = 1 << 20
    for match in (-1, 2):
        assert lib.upr_png_encode_ex(one, 1, 8, 8, 5, match, 4, one, 4096, one, one, big, None) == L.UPR_ERR_ARG
    for match in (0, 1):
        assert lib.upr_png_encode_ex(None, 1, 8, 8, 5, match, 4, one, 4096, one, one, big, None) == L.UPR_ERR_ARG
        assert lib.upr_png_encode_ex(one, 1, 8, 8, 5, match, 4, None, 4096, one, one, big, None) == L.UPR_ERR_ARG
        assert lib.upr_png_encode_ex(one, 1, 8, 8, 5, match, 4, one, 4096, None, one, big, None) == L.UPR_ERR_ARG
        assert lib.upr_png_encode_ex(one, 1, 8, 8, 5, match, 4, one, 4096, one, None, big, None) == L.UPR_ERR_ARG
        assert lib.upr_png_encode_ex(one, 0, 8, 8, 5, match, 4, one, 4096, one, one, big, None) == L.UPR_ERR_ARG
        assert lib.upr_png_encode_ex(one, 1, 8, 8, 6, match, 4, one, 4096, one, one, big, None) == L.UPR_ERR_ARG
        assert lib.upr_png_encode_ex(one, 1, 8, 8, -1, match, 4, one, 4096, one, one, big, None) == L.UPR_ERR_ARG
        assert lib.upr_png_encode_ex(one, 1, 8, 8, 5, match, 0, one, 4096, one, one, big, None) == L.UPR_ERR_ARG
        # an output stride below the bound, or too little scratch, is refused before any launch
        assert lib.upr_png_encode_ex(one, 1, 8, 8, 5, match, 4, one, 100, one, one, big, None) == L.UPR_ERR_ARG
        assert lib.upr_png_encode_ex(one, 1, 8, 8, 5, match, 4, one, 4096, one, one, 16, None) == L.UPR_ERR_WORKSPACE
    # the scratch of match mode none is too little for lz
    ns0 = _bound("upr_png_bound_ex", 8, 8, 4, 0)[2]
    assert lib.upr_png_encode_ex(one, 1, 8, 8, 5, 1, 4, one, 4096, one, one, ns0, None) == L.UPR_ERR_WORKSPACE
