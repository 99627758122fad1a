"""Device-side JPEG encoder (upr.jpeg) against the numpy restatement of its file format
(tests/jpeg_ref.py): the device file equals the restatement's file byte for byte (run with
`-m gpu`).  The restatement itself is checked against PIL / libjpeg in tests/test_cpu_jpeg.py."""
import functools
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref
from conftest import GOLDEN, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]


def _crop():
    return np.ascontiguousarray(np.load(os.path.join(GOLDEN, "g4_real_crop.npz"))["img_u8"][:77, :93])


def _blocks(kind):
    """16x32: alternating all-0 / all-255 blocks (DC differences of category 11), or blocks whose
    left half is 0 and right half 255 (a first AC coefficient of category 10)."""
    a = np.zeros((16, 32, 3), np.uint8)
    for by in range(2):
        for bx in range(4):
            if kind == "alternate":
                a[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = 255 * ((by + bx) % 2)
            else:
                a[by * 8:by * 8 + 8, bx * 8 + 4:bx * 8 + 8] = 255
    return a


@functools.lru_cache(maxsize=None)
def _images():
    rng = np.random.default_rng(0)
    xx = np.arange(805)
    ramp = np.stack([xx % 256, (xx // 3) % 256, (255 - xx // 4) % 256], -1).astype(np.uint8)
    wide = np.random.default_rng(5)
    return {
        "const1x1": np.full((1, 1, 3), 201, np.uint8),
        "const8x8": np.full((8, 8, 3), 77, np.uint8),
        "const7x9": np.full((7, 9, 3), 13, np.uint8),
        "const17x23": np.array([[[9, 200, 31]]], np.uint8).repeat(17, 0).repeat(23, 1),
        "crop": _crop(),
        "noise": rng.integers(0, 256, (40, 56, 3), dtype=np.uint8),
        "saturated": (rng.integers(0, 2, (24, 24, 3)) * 255).astype(np.uint8),
        "ramp8x805": np.ascontiguousarray(np.broadcast_to(ramp, (8, 805, 3))),
        # more bits than one LDS window of the bit stream holds, in more than one pass of 256 units
        "noise16x805": wide.integers(0, 256, (16, 805, 3), dtype=np.uint8),
        "alternate": _blocks("alternate"),
        "halves": _blocks("halves"),
    }


# (image, quality, restart_rows)
CASES = ([(n, 95, 1) for n in ("const1x1", "const8x8", "const7x9", "const17x23", "ramp8x805")] +
         [("crop", q, rr) for q in (1, 50, 95, 100) for rr in (1, 2, 16)] +
         [(n, q, 1) for n in ("noise", "saturated") for q in (1, 50, 95, 100)] +
         [("noise16x805", 100, 2), ("noise16x805", 100, 1), ("alternate", 100, 1), ("halves", 100, 1)])


@functools.lru_cache(maxsize=None)
def _reference(name, quality, restart_rows):
    return jpeg_ref.encode(_images()[name], quality, restart_rows)


def _encode(a, **kw):
    from upr import jpeg
    return jpeg.encode(torch.from_numpy(np.ascontiguousarray(a)).cuda(), **kw)


def _decode(data, shape):
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB" and im.size == (shape[1], shape[0])
    return np.array(im)


def test_cases_cover_the_entropy_coders_corners():
    """Asserted on the restatement's counters over the whole set: byte stuffing, a 1-padded last
    byte that is 0xFF, ZRL, a block without EOB, the largest DC and AC categories; the crop with
    restart_rows 1 has ten intervals, so the RST index wraps."""
    tot = dict(stuffed=0, padded_ff=0, zrl=0, no_eob=0, max_dc_cat=0, max_ac_cat=0)
    for case in CASES:
        _, cnt = _reference(*case)
        for k, v in cnt.items():
            tot[k] = max(tot[k], v) if k.startswith("max") else tot[k] + v
    print(tot)
    assert tot["stuffed"] >= 1 and tot["padded_ff"] >= 1 and tot["zrl"] >= 1 and tot["no_eob"] >= 1
    assert tot["max_dc_cat"] == 11 and tot["max_ac_cat"] == 10
    assert -(-_images()["crop"].shape[0] // 8) == 10
    data, _ = _reference("crop", 95, 1)
    assert b"\xff\xd7" in data and data.count(b"\xff\xd0") >= 2


@pytest.mark.parametrize("name,quality,restart_rows", CASES)
def test_device_file_equals_the_restatement(name, quality, restart_rows):
    from upr import jpeg
    a = _images()[name]
    ref, _ = _reference(name, quality, restart_rows)
    data, = _encode(a, quality=quality, restart_rows=restart_rows)
    assert len(data) == len(ref), (len(data), len(ref))
    assert data == ref
    assert len(data) <= jpeg.bound(a.shape[0], a.shape[1], restart_rows)[0]
    _decode(data, a.shape)


def test_batch_of_three_and_reproducible():
    """A batch of three different images gives the three single-image files; a second run gives
    the same bytes; sizes[b] <= bound; bytes of buf beyond sizes[b] are not compared."""
    from upr import jpeg
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    a[1] //= 16
    a[2, :, :, 1] = 7
    files = _encode(a, quality=90)
    assert len(files) == 3
    for k in range(3):
        assert files[k] == _encode(a[k], quality=90)[0]
        assert files[k] == jpeg_ref.encode(a[k], 90, 1)[0]
        _decode(files[k], a[k].shape)
    assert files == _encode(a, quality=90)
    buf, sizes = jpeg.encode_device(torch.from_numpy(a).cuda(), quality=90)
    assert buf.shape[0] == 3 and int(sizes.max()) <= jpeg.bound(37, 53)[0] <= buf.shape[1]


def _write_inputs(folder, n, H=48, W=60):
    rng = np.random.default_rng(4)
    os.makedirs(folder, exist_ok=True)
    for k in range(n):
        a = (rng.integers(0, 256, (H, W, 3)) * 0.35).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(folder, f"in{k}.png"))


def _pil_jpeg(px, quality):
    f = io.BytesIO()
    Image.fromarray(px).save(f, format="JPEG", quality=quality, subsampling=0)
    return f.getvalue()


KINDS = ("enhanced", "illumination", "comparison")


def _check_jpg_dir(png_dir, jpg_dir, stems, expect):
    """Every .jpg of jpg_dir is `expect` of the pixels of the same run's .png; no .png there."""
    assert sorted(os.listdir(jpg_dir)) == sorted(f"{s}_{k}.jpg" for s in stems for k in KINDS)
    for s in stems:
        for k in KINDS:
            px = np.array(Image.open(os.path.join(png_dir, f"{s}_{k}.png")).convert("RGB"))
            data = open(os.path.join(jpg_dir, f"{s}_{k}.jpg"), "rb").read()
            assert data == expect(px), (s, k)
            _decode(data, px.shape)


def test_harness_enhance_single_image(tmp_path):
    from enhancers.simple_enhance import enhance_single_image
    from models.model import UP_Retinex
    from upr import jpeg
    _write_inputs(str(tmp_path / "src"), 1)
    src = str(tmp_path / "src" / "in0.png")
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=True, use_aspp=True).to("cuda").eval()
    enhance_single_image(model, src, str(tmp_path / "png"), "cuda", max_size=64, png_encoder="device")
    enhance_single_image(model, src, str(tmp_path / "dev"), "cuda", max_size=64, png_encoder="device",
                         image_format="jpg", jpeg_quality=90)
    enhance_single_image(model, src, str(tmp_path / "host"), "cuda", max_size=64, png_encoder="host",
                         image_format="jpg", jpeg_quality=90)
    _check_jpg_dir(str(tmp_path / "png"), str(tmp_path / "dev"), ["in0"],
                   lambda px: jpeg.encode(torch.from_numpy(px).cuda(), quality=90)[0])
    _check_jpg_dir(str(tmp_path / "png"), str(tmp_path / "host"), ["in0"], lambda px: _pil_jpeg(px, 90))


def test_harness_predict_cli_batched(tmp_path):
    import main as cli
    from models.model import UP_Retinex
    from upr import jpeg
    src = str(tmp_path / "src")
    _write_inputs(src, 3)
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pth")
    torch.save({"model_state_dict": UP_Retinex(use_preact=True, use_aspp=True).state_dict()}, ckpt)
    common = ["--mode", "predict", "--checkpoint", ckpt, "--input_path", src, "--use_preact", "--use_aspp",
              "--device", "cuda", "--max_size", "64", "--infer_batch", "2"]
    cli.main(common + ["--output_dir", str(tmp_path / "png"), "--png_encoder", "device"])
    cli.main(common + ["--output_dir", str(tmp_path / "dev"), "--png_encoder", "device", "--image_format", "jpg"])
    cli.main(common + ["--output_dir", str(tmp_path / "host"), "--png_encoder", "host", "--image_format", "jpg",
                       "--jpeg_quality", "80"])
    stems = ["in0", "in1", "in2"]
    _check_jpg_dir(str(tmp_path / "png"), str(tmp_path / "dev"), stems,
                   lambda px: jpeg.encode(torch.from_numpy(px).cuda(), quality=95)[0])
    _check_jpg_dir(str(tmp_path / "png"), str(tmp_path / "host"), stems, lambda px: _pil_jpeg(px, 80))


def test_limits_raise_before_any_launch():
    import ctypes
    from upr import _lib as L, jpeg
    x = torch.zeros((64, 65535, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        jpeg.encode(x, restart_rows=8)  # Ri = 8192 * 8 > 65535
    with pytest.raises(ValueError):
        jpeg.bound(65536, 8)
    with pytest.raises(ValueError):
        jpeg.encode(x[:8, :8], quality=0)
    with pytest.raises(ValueError):
        jpeg.encode(x[:8, :8], restart_rows=0)
    with pytest.raises(TypeError):
        jpeg.encode(x[:8, :8].float())
    assert jpeg.bound(64, 65535, 7)[0] > 0
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    rc = L.lib().upr_jpeg_encode(x.data_ptr(), 1, 64, 65535, 95, 8, out.data_ptr(), 64, sizes.data_ptr(),
                                 out.data_ptr(), 64, None)
    assert rc == L.UPR_ERR_SHAPE
    rc = L.lib().upr_jpeg_encode(x.data_ptr(), 1, 8, 8, 95, 1, out.data_ptr(), 64, sizes.data_ptr(),
                                 out.data_ptr(), 64, None)
    assert rc == L.UPR_ERR_ARG  # out_stride below the bound
    torch.cuda.synchronize()
    assert sizes.item() == -7 and int(out.sum()) == 0
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.lib().upr_jpeg_bound(40000, 40000, 1, ctypes.byref(nb), ctypes.byref(ns)) == L.UPR_ERR_SHAPE  # > 2^31
