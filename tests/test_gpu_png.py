"""Device-side PNG encoder (upr.png) against PIL's decoder and zlib (run with `-m gpu`).
The oracle is never an encoder: PIL must return exactly the pixels that went in, zlib must
accept the joined IDAT stream (which checks the Adler-32), every chunk CRC must match zlib's."""
import heapq
import io
import os
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

FILTERS = ("adaptive", "none", "sub", "up", "avg", "paeth")
FILTER_TYPE = {"none": 0, "sub": 1, "up": 2, "avg": 3, "paeth": 4}


def _encode(a, **kw):
    from upr import png
    return png.encode(torch.from_numpy(np.ascontiguousarray(a)).cuda(), **kw)


def _decode(data):
    im = Image.open(io.BytesIO(data))
    assert im.mode == "RGB"
    return np.array(im)


def _chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, p = [], 8
    while p < len(data):
        n, = struct.unpack(">I", data[p:p + 4])
        typ, body = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        crc, = struct.unpack(">I", data[p + 8 + n:p + 12 + n])
        assert crc == zlib.crc32(typ + body), f"CRC of chunk {typ!r} at {p}"
        out.append((typ, body))
        p += 12 + n
    assert p == len(data)
    return out


def _check_structure(data, H, W, rps, filt):
    ch = _chunks(data)
    assert ch[0][0] == b"IHDR" and ch[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    assert ch[-1] == (b"IEND", b"")
    idat = ch[1:-1]
    assert all(t == b"IDAT" for t, _ in idat)
    n_strips = -(-H // min(rps, H))
    assert len(idat) == n_strips + 1 and len(idat[-1][1]) == 4
    raw = zlib.decompress(b"".join(b for _, b in idat))
    assert len(raw) == H * (3 * W + 1)
    ftypes = np.frombuffer(raw, np.uint8).reshape(H, 3 * W + 1)[:, 0]
    if filt == "adaptive":
        assert ftypes.max() <= 4
    else:
        assert (ftypes == FILTER_TYPE[filt]).all()


def _images(golden):
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:37, 0:53]
    return {
        "real128": np.ascontiguousarray(golden("g4_real_crop.npz")["img_u8"]),
        "random": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8),
        "constant": np.full((37, 53, 3), 201, np.uint8),
        "ramp": np.stack([(yy + xx) * 3 % 256, (yy * 2 + xx) % 256, (yy + xx * 5) % 256], -1).astype(np.uint8),
        "1x1": np.array([[[9, 200, 31]]], np.uint8),
        "1x4099": rng.integers(0, 256, (1, 4099, 3), dtype=np.uint8),
        "300x1": rng.integers(0, 40, (300, 1, 3), dtype=np.uint8),
    }


@pytest.mark.parametrize("name", ["real128", "random", "constant", "ramp", "1x1", "1x4099", "300x1"])
def test_round_trip_and_structure(golden, name):
    """Tests 1 and 2: every filter x rows_per_strip in {1, 3, 16, H}; PIL returns the input,
    the chunks, CRCs, strip count, zlib stream and filter bytes are as the format says."""
    a = _images(golden)[name]
    assert a.dtype == np.uint8 and a.shape[2] == 3
    H, W = a.shape[:2]
    for filt in FILTERS:
        for rps in sorted({1, 3, 16, H}):
            data, = _encode(a, filter=filt, rows_per_strip=rps)
            assert np.array_equal(_decode(data), a), (name, filt, rps)
            _check_structure(data, H, W, rps, filt)


def test_batch_of_three():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    a[1] //= 16
    a[2, :, :, 1] = 7
    files = _encode(a)
    assert len(files) == 3
    for k in range(3):
        assert np.array_equal(_decode(files[k]), a[k])
        _check_structure(files[k], 37, 53, 16, "adaptive")


def _huffman_depth(counts):
    """Depth of an unlimited Huffman code over the non-zero counts."""
    heap = [(c, 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def test_code_deeper_than_15():
    """Test 3: Fibonacci-like counts whose unlimited Huffman code is 18 deep; the encoder has to
    limit it to 15 bits and still round-trip."""
    H, W = 16, 228
    counts = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4197]
    assert sum(counts) == H * (3 * W + 1) == 10960
    # value 0 takes the count 21, 16 of which are the filter bytes of filter "none"
    order = [6] + [k for k in range(len(counts)) if k != 6]
    values, reps = [], []
    for v, k in enumerate(order):
        values.append(v)
        reps.append(counts[k] - (16 if v == 0 else 0))
    pix = np.repeat(np.array(values, np.uint8), reps)
    np.random.default_rng(5).shuffle(pix)
    a = pix.reshape(H, W, 3)
    filtered = np.concatenate([np.zeros((H, 1), np.uint8), a.reshape(H, 3 * W)], 1)
    hist = np.bincount(filtered.ravel(), minlength=256).tolist()
    assert sorted(c for c in hist if c) == sorted(counts)
    assert _huffman_depth(hist + [1]) == 18
    data, = _encode(a, filter="none", rows_per_strip=16)
    assert np.array_equal(_decode(data), a)
    _check_structure(data, H, W, 16, "none")


@pytest.mark.parametrize("rps", [1, 16, 64])
def test_stored_fallback_and_size_bounds(rps):
    """Test 4: noise never grows beyond a fixed overhead per strip (stored fallback); a constant
    image costs about one bit per symbol plus the headers."""
    for filt in FILTERS:
        H, W = 64, 200
        n_strips = -(-H // rps)
        a = np.random.default_rng(11).integers(0, 256, (H, W, 3), dtype=np.uint8)
        data, = _encode(a, filter=filt, rows_per_strip=rps)
        print(f"noise {filt} rps {rps}: {len(data)} B, bound {H * (3 * W + 1) + 32 * n_strips + 128}")
        assert np.array_equal(_decode(data), a)
        assert len(data) <= H * (3 * W + 1) + 32 * n_strips + 128
        H, W = 64, 100
        a = np.full((H, W, 3), 77, np.uint8)
        data, = _encode(a, filter=filt, rows_per_strip=rps)
        print(f"constant {filt} rps {rps}: {len(data)} B, bound {H * (3 * W + 1) / 7 + 200 * n_strips + 128}")
        assert np.array_equal(_decode(data), a)
        assert len(data) <= H * (3 * W + 1) / 7 + 200 * n_strips + 128


def test_strip_longer_than_one_stored_block():
    """A noise strip above 65535 filtered bytes is split into several stored blocks; a compressible
    strip of that length packs more than one staging chunk per thread run."""
    H, W = 40, 600  # one strip of 40 * 1801 = 72040 bytes
    rng = np.random.default_rng(13)
    for a in (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 5, (H, W, 3), dtype=np.uint8)):
        for filt in ("none", "adaptive"):
            data, = _encode(a, filter=filt, rows_per_strip=H)
            assert np.array_equal(_decode(data), a)
            _check_structure(data, H, W, H, filt)
            assert len(data) <= H * (3 * W + 1) + 5 * 2 + 22 + 128  # two stored blocks at the most


def test_reproducible():
    """Test 5: same bytes on a second call, independent of batch position, input strides and stream."""
    from upr import png
    rng = np.random.default_rng(2)
    abc = [rng.integers(0, 256 >> k, (37, 53, 3), dtype=np.uint8) for k in (0, 3, 6)]
    three = _encode(np.stack(abc))
    assert three == _encode(np.stack(abc))
    assert three[1] == _encode(abc[1])[0]
    wide = torch.from_numpy(np.concatenate([abc[1], abc[0]], 1)).cuda()
    view = wide[:, :53]
    assert not view.is_contiguous()
    assert png.encode(view)[0] == three[1]
    st = torch.cuda.Stream()
    x = torch.from_numpy(abc[1]).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        other = png.encode(x)[0]
    assert other == three[1]


def _write_input(path, H=48, W=60):
    rng = np.random.default_rng(4)
    a = (rng.integers(0, 256, (H, W, 3)) * 0.35).astype(np.uint8)
    Image.fromarray(a).save(path)


def _same_pngs(d0, d1, names):
    for n in names:
        a, b = np.array(Image.open(os.path.join(d0, n))), np.array(Image.open(os.path.join(d1, n)))
        assert a.shape == b.shape and np.array_equal(a, b), n
        _chunks(open(os.path.join(d1, n), "rb").read())


def test_harness_enhance_single_image(tmp_path):
    """Test 6: the device encoder's three files decode to the host encoder's pixels.  The model
    takes sizes that are multiples of 8, so the 48x60 file goes through the harness's letterbox
    (max_size=64), as any such file has to with either encoder."""
    from enhancers.simple_enhance import enhance_single_image
    from models.model import UP_Retinex
    src = str(tmp_path / "in.png")
    _write_input(src)
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=True, use_aspp=True).to("cuda").eval()
    for enc in ("host", "device"):
        enhance_single_image(model, src, str(tmp_path / enc), "cuda", max_size=64, png_encoder=enc)
    names = ["in_enhanced.png", "in_illumination.png", "in_comparison.png"]
    _same_pngs(str(tmp_path / "host"), str(tmp_path / "device"), names)
    assert open(str(tmp_path / "device" / names[0]), "rb").read(8) == b"\x89PNG\r\n\x1a\n"


def test_harness_predict_cli(tmp_path):
    import main as cli
    from models.model import UP_Retinex
    src = str(tmp_path / "in.png")
    _write_input(src)
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pth")
    torch.save({"model_state_dict": UP_Retinex(use_preact=True, use_aspp=True).state_dict()}, ckpt)
    for enc in ("host", "device"):
        cli.main(["--mode", "predict", "--checkpoint", ckpt, "--input_path", src, "--output_dir",
                  str(tmp_path / enc), "--png_encoder", enc, "--use_preact", "--use_aspp", "--device", "cuda",
                  "--max_size", "64"])
    names = ["in_enhanced.png", "in_illumination.png", "in_comparison.png"]
    _same_pngs(str(tmp_path / "host"), str(tmp_path / "device"), names)
    h, w, _ = np.array(Image.open(str(tmp_path / "device" / names[0]))).shape
    assert h >= 48 and w >= 60
    assert np.array(Image.open(str(tmp_path / "device" / names[2]))).shape == (h, 3 * w, 3)  # 3 panels


def test_save_image_one_channel_map(tmp_path):
    from enhancers.simple_enhance import save_image
    m = torch.rand(1, 1, 21, 34, generator=torch.Generator().manual_seed(0)).cuda()
    save_image(m, str(tmp_path / "d.png"), png_encoder="device")
    save_image(m, str(tmp_path / "h.png"), png_encoder="host")
    d = np.array(Image.open(str(tmp_path / "d.png")))
    assert d.shape == (21, 34, 3)
    assert np.array_equal(d[..., 0], d[..., 1]) and np.array_equal(d[..., 0], d[..., 2])
    assert np.array_equal(d, np.array(Image.open(str(tmp_path / "h.png"))))


def test_limits_raise_before_any_launch():
    """Test 7: rows_per_strip * (3W + 1) above 2^24 is an error status (a ValueError), not a launch."""
    import ctypes
    from upr import _lib as L, png
    W = 3_000_000  # 2 rows of 9,000,001 filtered bytes > 2^24
    x = torch.zeros((2, W, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        png.encode(x, rows_per_strip=2)
    with pytest.raises(ValueError):
        png.bound(2, W, 2)
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.lib().upr_png_bound(2, W, 2, ctypes.byref(nb), ctypes.byref(ns)) == L.UPR_ERR_SHAPE
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    rc = L.lib().upr_png_encode(x.data_ptr(), 1, 2, W, 5, 2, out.data_ptr(), 64, sizes.data_ptr(), out.data_ptr(),
                                64, None)
    assert rc == L.UPR_ERR_SHAPE
    torch.cuda.synchronize()
    assert sizes.item() == -7 and int(out.sum()) == 0
    # the same image in single-row strips is within the limit
    assert png.bound(2, W, 1)[0] > 2 * (3 * W + 1)
    # a file bound above 2^31 bytes is refused as well
    with pytest.raises(ValueError):
        png.bound(40000, 20000, 16)
    with pytest.raises(ValueError):
        png.encode(torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda"), filter="best")
