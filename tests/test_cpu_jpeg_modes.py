"""The device JPEG encoder's further modes: what can be checked without a device.  The numpy
restatement (tests/jpeg_modes_ref.py, which tests/test_gpu_jpeg_modes.py compares the device files
with byte for byte) against tests/jpeg_ref.py, PIL / libjpeg and an independent Huffman optimum;
upr_jpeg_bound_ex against its formula; argument checks; the CLI flags."""
import ctypes
import functools
import heapq
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_modes_ref as ref
import jpeg_ref
from test_cpu_jpeg import _images, _psnr, _segments
from upr import _lib as L

MODES = [(s, o) for s in ref.SUBSAMPLINGS for o in (False, True)]
QUALITIES = (50, 75, 90, 95, 100)

# PSNR the restatement may lose against PIL's own file at the same settings (subsampling=0 | 2 or
# mode "L", optimize=), per image and sampling: the largest gap measured with this restatement over
# QUALITIES (the real crop at Q 95 left out, as in tests/test_cpu_jpeg.py) plus 0.25 dB.  The
# optimised tables change no coefficient, so a gap is the same with and without them.
PSNR_GAP_DB = {("crop", "444"): 0.33, ("crop", "420"): 0.33, ("crop", "gray"): 0.33,
               ("noise", "444"): 0.02, ("noise", "420"): 0.01, ("noise", "gray"): 0.20,
               ("saturated", "444"): 0.73, ("saturated", "420"): 0.0, ("saturated", "gray"): 1.04}
# Size above PIL's + 6 (DRI) + 3 bytes per interval, the largest excess measured plus 2 %.  4:2:0 on
# the two noise images is 11 - 12 % above PIL: 40x56 and 24x24 are no multiples of 16, and where
# this format codes the repeated last row / column libjpeg codes dummy blocks (the previous DC, no
# AC); on the 128x128 crop, where no block is padding, 4:2:0 is within 3.8 % (Q 95, optimised).
SIZE_EXCESS = {("crop", "444"): 0.039, ("crop", "420"): 0.038, ("crop", "gray"): 0.042,
               ("noise", "444"): 0.003, ("noise", "420"): 0.108, ("noise", "gray"): 0.0,
               ("saturated", "444"): 0.0, ("saturated", "420"): 0.120, ("saturated", "gray"): 0.0}


def _pil_file(a, quality, subsampling, optimize):
    f = io.BytesIO()
    im = Image.fromarray(a)
    if subsampling == "gray":
        im.convert("L").save(f, format="JPEG", quality=quality, optimize=optimize)
    else:
        im.save(f, format="JPEG", quality=quality, subsampling=2 if subsampling == "420" else 0, optimize=optimize)
    return f.getvalue()


@functools.lru_cache(maxsize=None)
def _file(name, quality, restart_rows, subsampling, optimize):
    return ref.encode(_images()[name], quality, restart_rows, subsampling, optimize)


def _open(data, a, subsampling):
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == ("L" if subsampling == "gray" else "RGB") and im.size == (a.shape[1], a.shape[0])
    return np.array(im)


@pytest.mark.parametrize("name", ["crop", "noise", "saturated"])
def test_444_standard_is_jpeg_ref(name):
    a = _images()[name]
    for quality, rr in ((95, 1), (50, 2), (1, 16), (100, 1)):
        data, cnt = ref.encode(a, quality, rr)
        want, want_cnt = jpeg_ref.encode(a, quality, rr)
        assert data == want
        assert {k: cnt[k] for k in want_cnt} == want_cnt and cnt["limited"] == 0
    assert ref.bound(a.shape[0], a.shape[1], 2) == jpeg_ref.bound(a.shape[0], a.shape[1], 2)
    assert ref.HEADER_BOUND == {"444": L.UPR_JPEG_HEADER_BYTES, "420": L.UPR_JPEG_HEADER_BYTES,
                                "gray": L.UPR_JPEG_HEADER_BYTES_GRAY}
    assert ref.MAX_BLOCK_BITS == {False: L.UPR_JPEG_MAX_BLOCK_BITS, True: L.UPR_JPEG_MAX_BLOCK_BITS_OPTIMIZED}


@pytest.mark.parametrize("subsampling,optimize", MODES)
@pytest.mark.parametrize("name", ["crop", "noise", "saturated"])
def test_every_mode_decodes_and_optimized_changes_no_pixel(name, subsampling, optimize):
    a = _images()[name]
    data, cnt = _file(name, 90, 1, subsampling, optimize)
    px = _open(data, a, subsampling)
    assert len(data) <= ref.bound(a.shape[0], a.shape[1], 1, subsampling, optimize)
    markers = [m for m, _ in _segments(data)]
    dht = 2 if subsampling == "gray" else 4
    assert markers == [0xE0] + [0xDB] * (dht // 2) + [0xC0] + [0xC4] * dht + [0xDD, 0xDA]
    if optimize:  # the coefficients are the standard file's: any difference is a table bug
        std, _ = _file(name, 90, 1, subsampling, False)
        assert np.array_equal(px, _open(std, a, subsampling)) and len(data) < len(std)
        for (_, body), t in zip([s for s in _segments(data) if s[0] == 0xC4], range(4)):
            assert body[0] == ((t & 1) << 4 | t >> 1) and len(body) == 17 + sum(body[1:17])
            assert sorted(body[17:]) == [s for s, c in enumerate(cnt["counts"][t]) if c]


def _codes(bits, vals):
    return jpeg_ref.huffman_codes(bits, vals)


def _check_table(freq):
    """Prefix-free canonical codes of at most 16 bits, none all ones, one per counted symbol;
    -> (total cost in bits of the scaled counts, limited)."""
    bits, vals, limited = ref.optimal_table(freq)
    f = [int(v) for v in freq[:256]]
    assert sorted(vals) == [s for s, c in enumerate(f) if c]
    codes = _codes(bits, vals)
    words = sorted(format(c, f"0{n}b") for c, n in codes.values())
    assert all(1 <= len(w) <= 16 and set(w) != {"1"} for w in words)
    assert all(not b.startswith(a) for a, b in zip(words, words[1:]))
    assert sum(2.0 ** -len(w) for w in words) <= 1.0
    while sum(f) > ref.SCALE_LIMIT:
        f = [(v + 1) >> 1 if v else 0 for v in f]
    return sum(f[s] * n for s, (_, n) in codes.items()), limited, f


def _huffman_optimum(f, reserved=True):
    """Cost in bits of an optimal prefix code of the non-zero counts (with the reserved entry of
    count 1 among them): the sum of the merged weights."""
    heap = [c for c in f if c] + ([1] if reserved else [])
    heapq.heapify(heap)
    total = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        total += a + b
        heapq.heappush(heap, a + b)
    return total


def _fib(n=30):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def test_optimal_table_is_the_huffman_optimum_where_the_limit_does_not_act():
    rng = np.random.default_rng(1)
    hists = [list(rng.integers(0, 1000, 256)), list(rng.integers(0, 3, 256) * rng.integers(1, 10**4, 256)),
             [0, 5, 0, 9, 1, 1] + [0] * 250, [9] * 256, [7] * 12, _fib()]
    for _, cnt in (_file("crop", 90, 1, "420", True), _file("noise", 100, 1, "444", True)):
        hists += cnt["counts"]
    for h in hists:
        h = list(h) + [0] * (256 - len(h))
        cost, limited, f = _check_table(h)
        assert limited == 0
        # the reserved entry is merged first, so it lies on the tree's deepest level, the table's
        # longest length: the symbols' cost plus that length is the whole tree's, the optimum
        bits, vals, _ = ref.optimal_table(h)
        longest = max(k + 1 for k in range(16) if bits[k])
        assert cost + longest == _huffman_optimum(f)


def test_optimal_table_length_limit_scaling_ties_and_one_symbol():
    fib = _fib()
    # the largest count on symbol 0: the merges build a chain deeper than 16 and Figure K.3 acts
    cost, limited, _ = _check_table(fib[::-1] + [0] * 226)
    assert limited > 0
    assert cost >= _huffman_optimum(fib, reserved=False)  # no prefix code of the symbols costs less
    bits, vals, _ = ref.optimal_table(fib[::-1])
    assert max(k + 1 for k in range(16) if bits[k]) == 16 and len(vals) == 30
    # the smallest counts on the smallest symbols: ties go to the largest index, which keeps merged
    # nodes (at the smaller index) out of the next merge, and the tree stays within 16 bits
    assert _check_table(fib + [0] * 226)[1] == 0
    # scaling: a total above 2^22 is halved until it is not; 1 stays 1
    big = [0] * 256
    big[0], big[1], big[7], big[200], big[255] = 3 << 22, 1 << 21, 5, 1, (1 << 32) - 1
    _, limited, f = _check_table(big)
    assert sum(f) <= ref.SCALE_LIMIT < sum(big) and f[200] == 1 and f[7] == 1 and limited == 0
    assert ref.optimal_table(big) == ref.optimal_table(f)
    # one symbol: one 1-bit code, 0
    assert ref.optimal_table([0] * 5 + [7]) == ((1,) + (0,) * 15, (5,), 0)
    assert _codes(*ref.optimal_table([0] * 5 + [7])[:2]) == {5: (0, 1)}
    # all counts equal: 255 codes of 8 bits and one of 9 (the reserved entry took the other)
    bits, vals, _ = ref.optimal_table([9] * 256)
    assert bits[7] == 255 and bits[8] == 1 and vals[-1] == 255 and _check_table([9] * 256)[1] == 0
    # entry 256 of a caller's array is ignored; no counts, no codes
    assert ref.optimal_table([3, 1, 4] + [0] * 253 + [1000]) == ref.optimal_table([3, 1, 4])
    assert ref.optimal_table([0] * 256) == ((0,) * 16, (), 0)


@pytest.mark.parametrize("subsampling,optimize", [m for m in MODES if m != ("444", False)])
@pytest.mark.parametrize("name", ["crop", "noise", "saturated"])
def test_restatement_against_pil_at_the_same_settings(name, subsampling, optimize):
    """PSNR (against the RGB source; gray: against its luma, PIL's convert("L")) is PIL's own minus
    the measured gap and 0.25 dB at the most; the size PIL's plus 6 + 3 bytes per interval, times
    1 + the measured excess + 2 % at the most.  Q 95 on the real crop is left out of the PSNR
    assertion, as in tests/test_cpu_jpeg.py (3.8 dB below PIL in every mode: the crop is gray)."""
    a = _images()[name]
    src = np.array(Image.fromarray(a).convert("L")) if subsampling == "gray" else a
    for quality in QUALITIES:
        data, _ = _file(name, quality, 1, subsampling, optimize)
        pil = _pil_file(a, quality, subsampling, optimize)
        mine_db = _psnr(_open(data, a, subsampling), src)
        pil_db = _psnr(_open(pil, a, subsampling), src)
        rows = -(-a.shape[0] // ref.MCU_PIXELS[subsampling])
        allowed = (len(pil) + 6 + 3 * rows) * (1 + SIZE_EXCESS[name, subsampling] + 0.02)
        print(f"{name} {subsampling} optimize={optimize} Q{quality}: {mine_db:.3f} dB, PIL {pil_db:.3f} dB; "
              f"{len(data)} B, PIL {len(pil)} B, allowed {allowed:.0f}")
        if not (name == "crop" and quality == 95):
            assert mine_db >= pil_db - PSNR_GAP_DB[name, subsampling] - 0.25
        assert len(data) <= allowed


@pytest.mark.parametrize("subsampling,optimize", MODES)
@pytest.mark.parametrize("H,W,rr", [(1, 1, 1), (8, 8, 1), (77, 93, 1), (77, 93, 2), (77, 93, 16), (512, 512, 1),
                                    (17, 805, 3), (2160, 3840, 4)])
def test_bound_ex_is_the_documented_formula(H, W, rr, subsampling, optimize):
    from upr import jpeg
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    rc = L.lib().upr_jpeg_bound_ex(H, W, rr, L.JPEG_SUBSAMPLINGS[subsampling], int(optimize), ctypes.byref(nb),
                                   ctypes.byref(ns))
    assert rc == L.UPR_OK
    assert nb.value == ref.bound(H, W, rr, subsampling, optimize)
    assert ns.value >= nb.value - ref.HEADER_BOUND[subsampling] and ns.value % 16 == 0
    assert jpeg.bound(H, W, rr, subsampling, optimize) == (nb.value, ns.value)
    if (subsampling, optimize) == ("444", False):
        n0, s0 = ctypes.c_size_t(), ctypes.c_size_t()
        assert L.lib().upr_jpeg_bound(H, W, rr, ctypes.byref(n0), ctypes.byref(s0)) == L.UPR_OK
        assert (n0.value, s0.value) == (nb.value, ns.value)


def test_ex_argument_and_shape_errors():
    from upr import jpeg
    lib = L.lib()
    nb, ns = ctypes.c_size_t(), ctypes.c_size_t()
    r = (ctypes.byref(nb), ctypes.byref(ns))
    assert lib.upr_jpeg_bound_ex(8, 8, 1, 3, 0, *r) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_bound_ex(8, 8, 1, -1, 0, *r) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_bound_ex(8, 8, 1, 0, 2, *r) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_bound_ex(8, 8, 1, 1, 1, None, ctypes.byref(ns)) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_bound_ex(8, 8, 0, 1, 1, *r) == L.UPR_ERR_ARG
    # Ri counts MCUs: 4096 per row of a 65535-wide 4:2:0 image, 8192 of a 4:4:4 or gray one
    assert lib.upr_jpeg_bound_ex(256, 65535, 15, 1, 0, *r) == L.UPR_OK
    assert lib.upr_jpeg_bound_ex(256, 65535, 16, 1, 0, *r) == L.UPR_ERR_SHAPE
    assert lib.upr_jpeg_bound_ex(256, 65535, 8, 2, 0, *r) == L.UPR_ERR_SHAPE
    assert lib.upr_jpeg_bound_ex(65536, 8, 1, 2, 1, *r) == L.UPR_ERR_SHAPE
    assert lib.upr_jpeg_bound_ex(18000, 18000, 1, 0, 1, *r) == L.UPR_ERR_SHAPE  # a bound above 2^31
    assert lib.upr_jpeg_bound_ex(18000, 18000, 1, 2, 0, *r) == L.UPR_OK         # a third of it
    # null pointers and bad values return before anything touches a device
    assert lib.upr_jpeg_encode_ex(None, 1, 8, 8, 95, 1, 1, 1, None, 0, None, None, 0, None) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_huffman_build(None, 1, None, None, None) == L.UPR_ERR_ARG
    buf = (ctypes.c_uint32 * 257)()
    assert lib.upr_jpeg_huffman_build(buf, 0, buf, buf, None) == L.UPR_ERR_ARG
    assert lib.upr_jpeg_huffman_build(buf, 1, None, buf, None) == L.UPR_ERR_ARG
    with pytest.raises(ValueError):
        jpeg.bound(8, 8, 1, "422")
    with pytest.raises(ValueError):
        jpeg.bound(256, 65535, 16, "420")
    x = torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        jpeg.encode(x, subsampling="420", optimize=True)  # a CPU tensor
    with pytest.raises(ValueError):
        jpeg.encode(x, subsampling="4:2:0")
    with pytest.raises(TypeError):
        jpeg.huffman_build(torch.zeros(256))              # float counts
    with pytest.raises(TypeError):
        jpeg.huffman_build(torch.zeros((2, 100), dtype=torch.int64))


def test_cli_flags_parse_and_default():
    import main as cli
    import simple_enhance as root_cli
    for build in (cli.build_parser, root_cli.build_parser):
        p = build()
        req = ["--input", "x"] if build is root_cli.build_parser else ["--mode", "enhance"]
        d = p.parse_args(req)
        assert (d.jpeg_subsampling, d.jpeg_optimize, d.jpeg_gray_maps) == ("444", False, False)
        a = p.parse_args(req + ["--image_format", "jpg", "--jpeg_subsampling", "420", "--jpeg_optimize",
                                "--jpeg_gray_maps"])
        assert (a.image_format, a.jpeg_subsampling, a.jpeg_optimize, a.jpeg_gray_maps) == ("jpg", "420", True, True)
        for bad in (["--jpeg_subsampling", "gray"], ["--jpeg_subsampling", "422"], ["--jpeg_optimize", "1"]):
            with pytest.raises(SystemExit):
                p.parse_args(req + bad)
    assert cli._output_format(cli.build_parser().parse_args(
        ["--mode", "predict", "--image_format", "jpg", "--jpeg_subsampling", "420", "--jpeg_gray_maps"])) == dict(
        png_encoder="host", image_format="jpg", jpeg_quality=95, jpeg_subsampling="420", jpeg_optimize=False,
        jpeg_gray_maps=True)


def test_check_format_refuses_bad_values():
    from enhancers.simple_enhance import _check_format, create_comparison, save_image
    _check_format("jpg", 95, "420", True, True)
    _check_format("jpg", 95)
    _check_format("png", 95, "gray", "yes", 1)  # ignored with png
    for bad in (("jpg", 95, "gray"), ("jpg", 95, "422"), ("jpg", 95, 420), ("jpg", 95, "420", 1),
                ("jpg", 95, "444", False, "yes"), ("jpg", 0, "420")):
        with pytest.raises(ValueError):
            _check_format(*bad)
    t = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError):
        save_image(t, "/nonexistent/x.jpg", image_format="jpg", jpeg_subsampling="gray")
    with pytest.raises(ValueError):
        create_comparison(t[None], t[None], "/nonexistent/x.jpg", image_format="jpg", jpeg_optimize="no")


def test_host_encoder_takes_the_same_choices(tmp_path):
    """png_encoder="host": PIL gets subsampling=0|2, optimize= and convert("L") for the map."""
    from enhancers.simple_enhance import _Jpeg, _write_jpg
    a = _images()["noise"]
    g = np.ascontiguousarray(a[:, :, 1:2].repeat(3, 2))
    for jpeg, src, sub in ((_Jpeg(90, "420", True), a, "420"), (_Jpeg(90, "444", False), a, "444"),
                           (_Jpeg(90, "420", True, True), g, "gray"), (_Jpeg(80), a, "444")):
        path = str(tmp_path / "x.jpg")
        _write_jpg(src, path, "saved", jpeg)
        assert open(path, "rb").read() == _pil_file(src, jpeg.quality, sub, jpeg.optimize)
    assert np.array_equal(np.array(Image.fromarray(g).convert("L")), g[..., 0])  # exact for R = G = B
