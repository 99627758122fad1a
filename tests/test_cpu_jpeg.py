"""Device JPEG encoder: what can be checked without a device.  The numpy restatement of the file
format (tests/jpeg_ref.py, which tests/test_gpu_jpeg.py compares the device files with byte for
byte) against PIL / libjpeg: the tables, that its files decode, their quality and size; the CLI
flags, the refusal of CPU tensors, upr_jpeg_bound against its formula, argument checks."""
import ctypes
import functools
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref
from conftest import GOLDEN
from upr import _lib as L

# PSNR the restatement may lose against PIL's own file at the same settings, per image: the
# largest gap measured over the asserted qualities with this restatement (crop 0.33 dB at Q 90,
# noise 0.02 dB at Q 90, saturated noise 0.73 dB at Q 100; elsewhere it is level or ahead) plus
# 0.25 dB, so that a later change of the DCT's rounding does not flip the test.
PSNR_MARGIN_DB = {"crop": 0.33 + 0.25, "noise": 0.02 + 0.25, "saturated": 0.73 + 0.25}
# Size above PIL's + 6 (DRI) + 3 bytes per interval (marker and padding), per image: the largest
# excess measured (crop 2.6 % at Q 95, noise 0.3 % at Q 75, saturated noise none) plus 2 %.
SIZE_MARGIN = {"crop": 0.026 + 0.02, "noise": 0.003 + 0.02, "saturated": 0.0 + 0.02}


@functools.lru_cache(maxsize=None)
def _images():
    rng = np.random.default_rng(0)
    return {"crop": np.ascontiguousarray(np.load(os.path.join(GOLDEN, "g4_real_crop.npz"))["img_u8"]),
            "noise": rng.integers(0, 256, (40, 56, 3), dtype=np.uint8),
            "saturated": (rng.integers(0, 2, (24, 24, 3)) * 255).astype(np.uint8)}


def _pil_file(a, quality):
    f = io.BytesIO()
    Image.fromarray(a).save(f, format="JPEG", quality=quality, subsampling=0, optimize=False)
    return f.getvalue()


def _segments(data):
    """[(marker, payload)] of the segments in front of the entropy-coded data."""
    assert data[:2] == b"\xff\xd8"
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        n = int.from_bytes(data[p + 2:p + 4], "big")
        out.append((data[p + 1], data[p + 4:p + 2 + n]))
        if data[p + 1] == 0xDA:
            return out
        p += 2 + n


def _tables(data):
    dqt, dht = {}, {}
    for marker, body in _segments(data):
        while marker == 0xDB and body:
            assert body[0] >> 4 == 0
            dqt[body[0] & 15] = tuple(body[1:65])
            body = body[65:]
        while marker == 0xC4 and body:
            n = sum(body[1:17])
            dht[body[0]] = bytes(body[:17 + n])
            body = body[17 + n:]
    return dqt, dht


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("quality", [1, 50, 75, 95, 100])
def test_tables_are_the_ones_pil_writes(quality):
    dqt, dht = _tables(_pil_file(_images()["noise"], quality))
    assert dqt == {0: jpeg_ref.quant_table(jpeg_ref.BASE_LUMA, quality),
                   1: jpeg_ref.quant_table(jpeg_ref.BASE_CHROMA, quality)}
    assert dht == {0x00: jpeg_ref.dht_payload(0, 0, jpeg_ref.DC_BITS[0], jpeg_ref.DC_VALS[0]),
                   0x10: jpeg_ref.dht_payload(1, 0, jpeg_ref.AC_BITS[0], jpeg_ref.AC_VALS[0]),
                   0x01: jpeg_ref.dht_payload(0, 1, jpeg_ref.DC_BITS[1], jpeg_ref.DC_VALS[1]),
                   0x11: jpeg_ref.dht_payload(1, 1, jpeg_ref.AC_BITS[1], jpeg_ref.AC_VALS[1])}
    # and the restatement's own file carries them, in the documented segment order
    mine = jpeg_ref.encode(_images()["noise"], quality)[0]
    assert _tables(mine) == (dqt, dht)
    assert [m for m, _ in _segments(mine)] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert len(b"".join(b"\xff\0\0\0" + b for _, b in _segments(mine))) + 2 == jpeg_ref.HEADER_BYTES
    assert jpeg_ref.MAX_BLOCK_BITS == 22 + 63 * 26 == L.UPR_JPEG_MAX_BLOCK_BITS
    assert jpeg_ref.HEADER_BYTES == L.UPR_JPEG_HEADER_BYTES


@pytest.mark.parametrize("name", ["crop", "noise", "saturated"])
@pytest.mark.parametrize("quality", [50, 75, 90, 95, 100])
def test_restatement_decodes_and_is_a_sane_jpeg(name, quality):
    """PIL opens the file as RGB of the right size; its PSNR against the source is PIL's own at
    the same settings minus the margin at the most, its size PIL's plus 6 + 3 bytes per interval
    times (1 + margin) at the most.  Q 95 on the real crop is left out of the PSNR assertion: the
    restatement is 3.8 dB below PIL there (58.3 against 62.1 dB) while PIL's Q 95 beats its own
    Q 98 and Q 100 on that image, which suggests the crop was born a JPEG at that setting; a
    more precise DCT gives the same result."""
    a = _images()[name]
    data, _ = jpeg_ref.encode(a, quality)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB" and im.size == (a.shape[1], a.shape[0])
    pil = _pil_file(a, quality)
    mine_db, pil_db = _psnr(np.array(im), a), _psnr(np.array(Image.open(io.BytesIO(pil))), a)
    allowed = (len(pil) + 6 + 3 * -(-a.shape[0] // 8)) * (1 + SIZE_MARGIN[name])
    print(f"{name} Q{quality}: {mine_db:.3f} dB, PIL {pil_db:.3f} dB; {len(data)} B, PIL {len(pil)} B, "
          f"allowed {allowed:.0f}")
    if not (name == "crop" and quality == 95):
        assert mine_db >= pil_db - PSNR_MARGIN_DB[name]
    assert len(data) <= allowed


def test_restatement_restart_rows_only_move_markers():
    a = _images()["crop"]
    one, two, all_ = (jpeg_ref.encode(a, 75, rr)[0] for rr in (1, 2, 16))
    px = [np.array(Image.open(io.BytesIO(d))) for d in (one, two, all_)]
    assert np.array_equal(px[0], px[1]) and np.array_equal(px[0], px[2])
    assert len(one) > len(two) > len(all_)


def test_cli_flags_parse_and_default():
    import main as cli
    p = cli.build_parser()
    d = p.parse_args([])
    assert d.image_format == "png" and d.jpeg_quality == 95
    a = p.parse_args(["--mode", "enhance", "--image_format", "jpg", "--jpeg_quality", "80", "--png_encoder", "device"])
    assert (a.image_format, a.jpeg_quality, a.png_encoder) == ("jpg", 80, "device")
    for bad in (["--image_format", "gif"], ["--jpeg_quality", "0"], ["--jpeg_quality", "101"], ["--jpeg_quality", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_harness_refuses_unknown_format_and_quality():
    from enhancers.simple_enhance import create_comparison, run_batched, save_image
    t = torch.zeros(3, 4, 4)
    with pytest.raises(ValueError):
        save_image(t, "/nonexistent/x.gif", image_format="gif")
    with pytest.raises(ValueError):
        save_image(t, "/nonexistent/x.jpg", image_format="jpg", jpeg_quality=0)
    with pytest.raises(ValueError):
        create_comparison(t[None], t[None], "/nonexistent/x.jpg", image_format="jpeg")
    with pytest.raises(ValueError):
        run_batched(None, [], "/nonexistent", "cuda", image_format="bmp")


def test_encode_refuses_cpu_tensor():
    from upr import jpeg
    x = torch.zeros((4, 5, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm"):
        jpeg.encode(x)
    with pytest.raises(RuntimeError, match="ROCm"):
        jpeg.encode_device(x, quality=50, restart_rows=2)


@pytest.mark.parametrize("H,W,rr", [(64, 200, 16), (64, 200, 1), (64, 100, 64), (1, 1, 1), (1, 4099, 1), (300, 1, 7),
                                    (512, 512, 16), (37, 53, 3), (16, 30000, 16), (512, 512, 1)])
def test_bound_is_the_formula(H, W, rr):
    """Headers + per interval 2 ceil(blocks MAX_BLOCK_BITS / 8) + 2, recomputed from the
    restatement's tables."""
    from upr import jpeg
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.lib().upr_jpeg_bound(H, W, rr, ctypes.byref(nb), ctypes.byref(ns)) == L.UPR_OK
    assert nb.value == jpeg_ref.bound(H, W, rr)
    assert ns.value >= nb.value - jpeg_ref.HEADER_BYTES and ns.value % 16 == 0
    assert jpeg.bound(H, W, rr) == (nb.value, ns.value)


def test_bound_refuses_over_the_limits():
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    lib, ref = L.lib(), (ctypes.byref(nb), ctypes.byref(ns))
    assert lib.upr_jpeg_bound(65535, 8, 1, *ref) == L.UPR_OK
    assert lib.upr_jpeg_bound(65536, 8, 1, *ref) == L.UPR_ERR_SHAPE
    assert lib.upr_jpeg_bound(8, 65536, 1, *ref) == L.UPR_ERR_SHAPE
    assert lib.upr_jpeg_bound(64, 65535, 7, *ref) == L.UPR_OK       # Ri = 8192 * 7
    assert lib.upr_jpeg_bound(64, 65535, 8, *ref) == L.UPR_ERR_SHAPE  # Ri = 65536
    assert lib.upr_jpeg_bound(40000, 40000, 1, *ref) == L.UPR_ERR_SHAPE  # a bound above 2^31
    assert lib.upr_jpeg_bound(0, 8, 1, *ref) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_bound(8, 8, 0, *ref) == L.UPR_ERR_ARG


def test_null_args_rejected_without_device():
    lib = L.lib()
    nb = ctypes.c_size_t()
    assert lib.upr_jpeg_bound(8, 8, 1, None, ctypes.byref(nb)) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_bound(8, 8, 1, ctypes.byref(nb), None) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_encode(None, 1, 8, 8, 95, 1, None, 0, None, None, 0, None) == L.UPR_ERR_ARG
    one = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    assert lib.upr_jpeg_encode(one, 0, 8, 8, 95, 1, one, 4096, one, one, 1 << 20, None) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_encode(one, 1, 8, 8, 0, 1, one, 4096, one, one, 1 << 20, None) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_encode(one, 1, 8, 8, 101, 1, one, 4096, one, one, 1 << 20, None) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_encode(one, 1, 8, 8, 95, 0, one, 4096, one, one, 1 << 20, None) == L.UPR_ERR_ARG
    # an output stride below the bound, or too little scratch, is refused before any launch
    assert jpeg_ref.bound(8, 8, 1) <= 4096
    assert lib.upr_jpeg_encode(one, 1, 8, 8, 95, 1, one, 100, one, one, 1 << 20, None) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_encode(one, 1, 8, 8, 95, 1, one, 4096, one, one, 16, None) == L.UPR_ERR_WORKSPACE
