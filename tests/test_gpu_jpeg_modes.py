"""The device JPEG encoder's further modes (upr.jpeg: subsampling "420" / "gray", optimize=True,
huffman_build) against their numpy restatement (tests/jpeg_modes_ref.py): the device file equals
the restatement's file byte for byte (run with `-m gpu`).  The restatement itself is checked
against PIL / libjpeg in tests/test_cpu_jpeg_modes.py."""
import functools
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_modes_ref as ref
from conftest import GOLDEN, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]


def _crop():
    return np.ascontiguousarray(np.load(os.path.join(GOLDEN, "g4_real_crop.npz"))["img_u8"][:77, :93])


def _blocks(kind, m):
    """2 x 4 MCUs of m x m pixels: alternating all-0 / all-255 MCUs (DC differences of category
    11), or MCUs whose left half is 0 and right half 255 (a first AC coefficient of category 10)."""
    a = np.zeros((2 * m, 4 * m, 3), np.uint8)
    for by in range(2):
        for bx in range(4):
            if kind == "alternate":
                a[by * m:(by + 1) * m, bx * m:(bx + 1) * m] = 255 * ((by + bx) % 2)
            else:
                a[by * m:(by + 1) * m, bx * m + m // 2:(bx + 1) * m] = 255
    return a


def _const(h, w, rgb):
    return np.broadcast_to(np.array(rgb, np.uint8), (h, w, 3)).copy()


@functools.lru_cache(maxsize=None)
def _images():
    rng = np.random.default_rng(0)
    crop = _crop()
    return {
        "const1x1": _const(1, 1, (201, 201, 201)),
        "const8x8": _const(8, 8, (77, 77, 77)),
        "const16x16": _const(16, 16, (9, 200, 31)),
        "const15x17": _const(15, 17, (250, 3, 99)),
        "const17x33": _const(17, 33, (9, 200, 31)),
        "const7x9": _const(7, 9, (13, 13, 13)),
        "const128": _const(17, 33, (128, 128, 128)),  # every DC difference is 0: one symbol in every table
        "crop": crop,
        "crop_green": np.ascontiguousarray(crop[:, :, 1:2].repeat(3, 2)),
        "noise": rng.integers(0, 256, (40, 56, 3), dtype=np.uint8),
        # nine MCU rows of 16 pixels: the RST index wraps
        "noise130x24": np.random.default_rng(6).integers(0, 256, (130, 24, 3), dtype=np.uint8),
        # 4:2:0: 51 MCUs, 306 units: two passes, an MCU cut by the pass border, more bits than one window
        "noise16x805": np.random.default_rng(5).integers(0, 256, (16, 805, 3), dtype=np.uint8),
        # gray at restart_rows 3: 303 units
        "noise24x805": np.random.default_rng(7).integers(0, 256, (24, 805, 3), dtype=np.uint8),
        "alternate16": _blocks("alternate", 16),
        "halves16": _blocks("halves", 16),
        "alternate8": _blocks("alternate", 8),
        "halves8": _blocks("halves", 8),  # the halves inside the Y blocks: the AC category 10 of 4:2:0
    }


# (image, quality, restart_rows, subsampling, optimize)
CASES_420 = ([(n, 95, 1, "420", False) for n in ("const1x1", "const8x8", "const16x16", "const15x17", "const17x33")] +
             [("crop", q, rr, "420", False) for q in (1, 50, 95, 100) for rr in (1, 2, 16)] +
             [("noise130x24", 90, 1, "420", False), ("noise16x805", 100, 1, "420", False),
              ("alternate16", 100, 1, "420", False), ("halves16", 100, 1, "420", False),
              ("halves8", 100, 1, "420", False)])
CASES_GRAY = [("const1x1", 95, 1, "gray", False), ("const7x9", 95, 1, "gray", False),
              ("crop_green", 95, 1, "gray", False), ("noise24x805", 100, 3, "gray", False),
              ("crop", 90, 1, "gray", False), ("alternate8", 100, 1, "gray", False)]  # crop: R != G != B
CASES_OPT = [(n, q, 1, s, True) for s in ref.SUBSAMPLINGS
             for n, q in (("const17x33", 95), ("const128", 95), ("crop", 95), ("noise", 1), ("noise", 100))]
CASES = CASES_420 + CASES_GRAY + CASES_OPT


@functools.lru_cache(maxsize=None)
def _reference(name, quality, restart_rows, subsampling, optimize):
    return ref.encode(_images()[name], quality, restart_rows, subsampling, optimize)


def _encode(a, **kw):
    from upr import jpeg
    return jpeg.encode(torch.from_numpy(np.ascontiguousarray(a)).cuda(), **kw)


def _decode(data, shape, subsampling):
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == ("L" if subsampling == "gray" else "RGB") and im.size == (shape[1], shape[0])
    return np.array(im)


def test_cases_cover_the_entropy_coders_corners():
    """On the restatement's counters, per new sampling over that sampling's cases: byte stuffing,
    a 1-padded last byte that is 0xFF, ZRL, a block without EOB; 4:2:0 reaches DC category 11 and
    AC category 10; nine MCU rows wrap the RST index; single-symbol tables occur."""
    for sub in ("420", "gray"):
        tot = dict(stuffed=0, padded_ff=0, zrl=0, no_eob=0, max_dc_cat=0, max_ac_cat=0)
        for case in CASES:
            if case[3] != sub:
                continue
            _, cnt = _reference(*case)
            for k in tot:
                tot[k] = max(tot[k], cnt[k]) if k.startswith("max") else tot[k] + cnt[k]
        print(sub, tot)
        assert tot["stuffed"] >= 1 and tot["padded_ff"] >= 1 and tot["zrl"] >= 1 and tot["no_eob"] >= 1, (sub, tot)
        assert tot["max_dc_cat"] == 11, (sub, tot)
        if sub == "420":
            assert tot["max_ac_cat"] == 10
    data, _ = _reference("noise130x24", 90, 1, "420", False)
    assert b"\xff\xd7" in data and data.count(b"\xff\xd0") >= 1
    assert ref.geometry(16, 805, 1, "420")[3] * 6 == 306 and ref.geometry(24, 805, 3, "gray")[3] == 303
    _, cnt = _reference("const128", 95, 1, "420", True)
    assert [sum(1 for c in t if c) for t in cnt["counts"]] == [1, 1, 1, 1]


@pytest.mark.parametrize("name,quality,restart_rows,subsampling,optimize", CASES)
def test_device_file_equals_the_restatement(name, quality, restart_rows, subsampling, optimize):
    from upr import jpeg
    a = _images()[name]
    want, _ = _reference(name, quality, restart_rows, subsampling, optimize)
    kw = dict(quality=quality, restart_rows=restart_rows, subsampling=subsampling, optimize=optimize)
    data, = _encode(a, **kw)
    assert len(data) == len(want), (len(data), len(want))
    assert data == want
    nb = jpeg.bound(a.shape[0], a.shape[1], restart_rows, subsampling, optimize)[0]
    assert len(data) <= nb == ref.bound(a.shape[0], a.shape[1], restart_rows, subsampling, optimize)
    _decode(data, a.shape, subsampling)
    assert _encode(a, **kw)[0] == data  # a second run gives the same bytes


def test_gray_is_the_luma_not_a_channel():
    a = _images()["noise"]
    data, = _encode(a, quality=100, subsampling="gray")
    px = _decode(data, a.shape, "gray").astype(np.int64)
    a = a.astype(np.int64)
    y = (19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 32768) >> 16
    # quantisation steps of 1: the decoder is within a few levels of Y, and far from every channel
    assert np.abs(px - y).mean() < 1.0
    assert min(np.abs(px - a[..., c]).mean() for c in range(3)) > 3.0


@pytest.mark.parametrize("subsampling", ref.SUBSAMPLINGS)
def test_optimized_batch_of_three_has_tables_per_image(subsampling):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    a[1] //= 16
    a[2, :, :, 1] = 7
    kw = dict(quality=90, subsampling=subsampling, optimize=True)
    files = _encode(a, **kw)
    assert len(files) == 3 and len({f[:700] for f in files}) == 3
    for k in range(3):
        assert files[k] == _encode(a[k], **kw)[0]
        assert files[k] == ref.encode(a[k], 90, 1, subsampling, True)[0]
        std = _encode(a[k], quality=90, subsampling=subsampling)[0]
        assert len(files[k]) < len(std)
        assert (_decode(files[k], a[k].shape, subsampling) == _decode(std, a[k].shape, subsampling)).all()
    assert files == _encode(a, **kw)


def _histograms():
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    big = [0] * 256
    big[0], big[1], big[7], big[200], big[255] = 3 << 22, 1 << 21, 5, 1, (1 << 32) - 1
    return {
        "fib_descending": fib[::-1],           # the length limit acts
        "fib_ascending": fib,                  # the tie rule keeps this tree within 16 bits
        "over_2^22": big,
        "ties": [9] * 256,
        "ties_sparse": [0, 4, 4, 0, 4, 4, 4] + [0] * 249,
        "one_symbol": [0] * 5 + [7] + [0] * 250,
        "empty": [0] * 256,
        "reserved_entry_ignored": [3, 1, 4, 1, 5] + [0] * 251 + [1000],
    }


def test_huffman_build_equals_optimal_table():
    from upr import jpeg
    hs = _histograms()
    want = {k: ref.optimal_table(v) for k, v in hs.items()}
    assert want["fib_descending"][2] > 0 and want["fib_ascending"][2] == 0
    rows = [list(v) + [0] * (257 - len(v)) for v in hs.values()]
    got = jpeg.huffman_build(torch.tensor(rows, dtype=torch.int64))
    for (name, w), g in zip(want.items(), got):
        assert g == (w[0], w[1]), name
    assert jpeg.huffman_build(torch.tensor(hs["fib_descending"] + [0] * 226)) == want["fib_descending"][:2]


def test_encode_is_encode_ex_444_standard():
    from upr import _lib as L, jpeg
    a = torch.from_numpy(_images()["crop"]).cuda()
    H, W = a.shape[:2]
    nb, ns = jpeg.bound(H, W, 2)
    outs = []
    for ex in (False, True):
        out = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        sizes = torch.zeros(1, dtype=torch.int64, device="cuda")
        scratch = torch.zeros(ns, dtype=torch.uint8, device="cuda")
        args = (a.data_ptr(), 1, H, W, 80, 2) + ((L.JPEG_SUBSAMPLINGS["444"], L.JPEG_HUFFMAN["standard"]) if ex else ())
        fn = L.lib().upr_jpeg_encode_ex if ex else L.lib().upr_jpeg_encode
        assert fn(*args, out.data_ptr(), nb, sizes.data_ptr(), scratch.data_ptr(), ns, None) == L.UPR_OK
        torch.cuda.synchronize()
        outs.append(out[:int(sizes)].cpu().numpy().tobytes())
    assert outs[0] == outs[1] == _encode(a.cpu().numpy(), quality=80, restart_rows=2)[0]
    import jpeg_ref
    assert outs[0] == jpeg_ref.encode(a.cpu().numpy(), 80, 2)[0]


def test_ex_errors_launch_nothing():
    from upr import _lib as L, jpeg
    x = torch.zeros((256, 65535, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        jpeg.encode(x, restart_rows=16, subsampling="420")  # Ri = 4096 * 16 > 65535
    assert jpeg.bound(256, 65535, 15, "420")[0] > 0
    with pytest.raises(ValueError):
        jpeg.encode(x[:8, :8], subsampling="422")
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    for sub, huff, want in ((3, 0, L.UPR_ERR_ARG), (0, 2, L.UPR_ERR_ARG), (-1, 0, L.UPR_ERR_ARG),
                            (2, 1, L.UPR_ERR_ARG)):  # the last: out_stride below the bound
        rc = L.lib().upr_jpeg_encode_ex(x.data_ptr(), 1, 8, 8, 95, 1, sub, huff, out.data_ptr(), 64,
                                        sizes.data_ptr(), out.data_ptr(), 64, None)
        assert rc == want, (sub, huff)
    rc = L.lib().upr_jpeg_encode_ex(x.data_ptr(), 1, 256, 65535, 95, 16, 1, 1, out.data_ptr(), 64, sizes.data_ptr(),
                                    out.data_ptr(), 64, None)
    assert rc == L.UPR_ERR_SHAPE
    torch.cuda.synchronize()
    assert sizes.item() == -7 and int(out.sum()) == 0


def _write_inputs(folder, n, H=48, W=60):
    rng = np.random.default_rng(4)
    os.makedirs(folder, exist_ok=True)
    for k in range(n):
        a = (rng.integers(0, 256, (H, W, 3)) * 0.35).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(folder, f"in{k}.png"))


def test_harness_predict_cli_batched_with_all_three_flags(tmp_path):
    import main as cli
    from models.model import UP_Retinex
    from upr import jpeg
    src = str(tmp_path / "src")
    _write_inputs(src, 2)
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pth")
    torch.save({"model_state_dict": UP_Retinex(use_preact=True, use_aspp=True).state_dict()}, ckpt)
    common = ["--mode", "predict", "--checkpoint", ckpt, "--input_path", src, "--use_preact", "--use_aspp",
              "--device", "cuda", "--max_size", "64", "--infer_batch", "2", "--png_encoder", "device"]
    cli.main(common + ["--output_dir", str(tmp_path / "png")])
    cli.main(common + ["--output_dir", str(tmp_path / "jpg"), "--image_format", "jpg", "--jpeg_subsampling", "420",
                       "--jpeg_optimize", "--jpeg_gray_maps"])
    kinds = {"enhanced": "420", "illumination": "gray", "comparison": "420"}
    assert sorted(os.listdir(tmp_path / "jpg")) == sorted(f"in{k}_{kind}.jpg" for k in range(2) for kind in kinds)
    for k in range(2):
        for kind, sub in kinds.items():
            px = np.array(Image.open(tmp_path / "png" / f"in{k}_{kind}.png").convert("RGB"))
            data = open(tmp_path / "jpg" / f"in{k}_{kind}.jpg", "rb").read()
            assert data == jpeg.encode(torch.from_numpy(px).cuda(), subsampling=sub, optimize=True)[0], (k, kind)
            _decode(data, px.shape, sub)
    assert Image.open(tmp_path / "jpg" / "in0_illumination.jpg").mode == "L"
