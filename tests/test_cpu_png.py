"""Device PNG encoder: what can be checked without a device -- the CLI flag, the refusal of CPU
tensors, upr_png_bound against the format's own size formula, null arguments."""
import ctypes

import pytest
import torch

from upr import _lib as L


def test_png_encoder_flag_parses_and_defaults_to_host():
    import main as cli
    p = cli.build_parser()
    assert p.parse_args([]).png_encoder == "host"
    assert p.parse_args(["--mode", "enhance", "--png_encoder", "device"]).png_encoder == "device"
    assert p.parse_args(["--mode", "predict", "--png_encoder", "host"]).png_encoder == "host"
    with pytest.raises(SystemExit):
        p.parse_args(["--png_encoder", "gpu"])


def test_encode_refuses_cpu_tensor():
    from upr import png
    x = torch.zeros((4, 5, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm"):
        png.encode(x)
    with pytest.raises(RuntimeError, match="ROCm"):
        png.encode_device(x, filter="sub", rows_per_strip=2)


def test_harness_refuses_unknown_encoder():
    from enhancers.simple_enhance import save_image
    with pytest.raises(ValueError):
        save_image(torch.zeros(3, 4, 4), "/nonexistent/x.png", png_encoder="gpu")


@pytest.mark.parametrize("H,W,rps", [(64, 200, 16), (64, 200, 1), (64, 100, 64), (1, 1, 1), (1, 4099, 1), (300, 1, 7),
                                     (512, 512, 16), (37, 53, 3), (16, 30000, 16)])
def test_bound_covers_the_stored_form(H, W, rps):
    """The bound is at least the stored form's size: H*(3W+1) bytes, 32 per strip (the IDAT
    chunk's 12 bytes, two stored block headers, rounded up) and 128 for the fixed parts; a strip
    longer than one stored block (65535 B) pays 5 more bytes per further block, nothing else."""
    from upr import png
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.lib().upr_png_bound(H, W, rps, ctypes.byref(nb), ctypes.byref(ns)) == L.UPR_OK
    n_strips = -(-H // rps)
    last = H - (n_strips - 1) * rps
    blocks = (n_strips - 1) * -(-(rps * (3 * W + 1)) // 65535) + -(-(last * (3 * W + 1)) // 65535)
    formula = H * (3 * W + 1) + 32 * n_strips + 128
    assert nb.value >= formula
    assert nb.value == formula + 5 * (blocks - n_strips)
    assert ns.value >= nb.value - 128 and ns.value % 16 == 0
    assert png.bound(H, W, rps) == (nb.value, ns.value)


def test_bound_refuses_over_the_limits():
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    lib = L.lib()
    assert lib.upr_png_bound(2, 3_000_000, 2, ctypes.byref(nb), ctypes.byref(ns)) == L.UPR_ERR_SHAPE
    assert lib.upr_png_bound(16, (L.UPR_PNG_MAX_STRIP_BYTES // 16 - 1) // 3, 16, ctypes.byref(nb),
                             ctypes.byref(ns)) == L.UPR_OK
    assert lib.upr_png_bound(16, (L.UPR_PNG_MAX_STRIP_BYTES // 16 - 1) // 3 + 1, 16, ctypes.byref(nb),
                             ctypes.byref(ns)) == L.UPR_ERR_SHAPE
    assert lib.upr_png_bound(40000, 20000, 16, ctypes.byref(nb), ctypes.byref(ns)) == L.UPR_ERR_SHAPE
    assert lib.upr_png_bound(0, 8, 1, ctypes.byref(nb), ctypes.byref(ns)) == L.UPR_ERR_ARG
    assert lib.upr_png_bound(8, 8, 0, ctypes.byref(nb), ctypes.byref(ns)) == L.UPR_ERR_ARG


def test_null_args_rejected_without_device():
    lib = L.lib()
    nb = ctypes.c_size_t()
    assert lib.upr_png_bound(8, 8, 4, None, ctypes.byref(nb)) == L.UPR_ERR_ARG
    assert lib.upr_png_bound(8, 8, 4, ctypes.byref(nb), None) == L.UPR_ERR_ARG
    assert lib.upr_png_encode(None, 1, 8, 8, 5, 4, None, 0, None, None, 0, None) == L.UPR_ERR_ARG
    one = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    assert lib.upr_png_encode(one, 0, 8, 8, 5, 4, one, 4096, one, one, 1 << 20, None) == L.UPR_ERR_ARG
    assert lib.upr_png_encode(one, 1, 8, 8, 6, 4, one, 4096, one, one, 1 << 20, None) == L.UPR_ERR_ARG
    assert lib.upr_png_encode(one, 1, 8, 8, -1, 4, one, 4096, one, one, 1 << 20, None) == L.UPR_ERR_ARG
    # an output stride below the bound, or too little scratch, is refused before any launch
    assert lib.upr_png_encode(one, 1, 8, 8, 5, 4, one, 100, one, one, 1 << 20, None) == L.UPR_ERR_ARG
    assert lib.upr_png_encode(one, 1, 8, 8, 5, 4, one, 4096, one, one, 16, None) == L.UPR_ERR_WORKSPACE
