"""Device-side PNG encoder with matches="lz" (run with `-m gpu`).  As in test_gpu_png.py the
oracle is never an encoder of ours: PIL must return exactly the pixels that went in, zlib must
accept the joined IDAT stream and every strip's payload on its own (no match reaches outside
its strip), every chunk CRC must match zlib's.  Where a test has to know what the encoder chose
(was a match taken, how deep would the code be), a small inflate parser below reads the symbols
back from the file."""
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
NAMES = ["real128", "random", "constant", "ramp", "1x1", "1x4099", "300x1"]


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
    return raw


def _strip_streams(data):
    """The raw deflate data of every strip: the IDAT payloads but the last (the Adler-32), the
    first without its 2-byte zlib header."""
    idat = [b for t, b in _chunks(data) if t == b"IDAT"][:-1]
    assert idat[0][:2] == b"\x78\x01"
    return [idat[0][2:]] + idat[1:]


def _check_strips_stand_alone(data, raw, H, W, rps):
    """Every strip inflates on its own to its rows' filtered bytes."""
    rowb, rps = 3 * W + 1, min(rps, H)
    streams = _strip_streams(data)
    for k, body in enumerate(streams):
        d = zlib.decompressobj(-15)
        out = d.decompress(body)
        assert d.unused_data == b"" and d.eof == (k == len(streams) - 1)
        assert out == raw[k * rps * rowb:(k + 1) * rps * rowb], f"strip {k}"


# ---- a small inflate that returns the symbols instead of the bytes ------------------------------
class _Bits:
    def __init__(self, data):
        self.d, self.p = data, 0

    def get(self, n):
        v = 0
        for k in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << k
            self.p += 1
        return v


def _decoder(lens):
    """{(length, code): symbol} of the canonical code (RFC 1951 3.2.2)."""
    tab, code = {}, 0
    for ln in range(1, 16):
        for s, l in enumerate(lens):
            if l == ln:
                tab[(ln, code)] = s
                code += 1
        code <<= 1
    return tab


def _sym(bits, tab):
    code = 0
    for ln in range(1, 16):
        code = code << 1 | bits.get(1)
        if (ln, code) in tab:
            return tab[(ln, code)]
    raise AssertionError("no such code")


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
          258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
          6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]


def _blocks(body):
    """Blocks of one strip's raw deflate data: dicts with `type` (0 stored, 2 dynamic) and, for a
    dynamic block, the literal/length histogram `ll` (286), the matches [(length, distance)] and
    the code lengths `ll_lens` / `d_lens` as sent."""
    bits, out = _Bits(body), []
    while True:
        final, typ = bits.get(1), bits.get(2)
        if typ == 0:
            bits.p = (bits.p + 7) & ~7
            n = bits.get(16)
            assert bits.get(16) == n ^ 0xFFFF
            bits.p += 8 * n
            out.append({"type": 0, "len": n})
        else:
            assert typ == 2
            hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
            cl = [0] * 19
            for k in range(hclen):
                cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[k]] = bits.get(3)
            cltab, lens = _decoder(cl), []
            while len(lens) < hlit + hdist:
                s = _sym(bits, cltab)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + bits.get(2))
                else:
                    lens += [0] * (3 + bits.get(3) if s == 17 else 11 + bits.get(7))
            assert len(lens) == hlit + hdist
            lltab, dtab = _decoder(lens[:hlit]), _decoder(lens[hlit:])
            ll, matches = [0] * 286, []
            while True:
                s = _sym(bits, lltab)
                ll[s] += 1
                if s == 256:
                    break
                if s > 256:
                    length = _LBASE[s - 257] + bits.get(_LEXT[s - 257])
                    dc = _sym(bits, dtab)
                    matches.append((length, _DBASE[dc] + bits.get(_DEXT[dc])))
            out.append({"type": 2, "ll": ll, "matches": matches, "ll_lens": lens[:hlit], "d_lens": lens[hlit:]})
        if final or bits.p + 7 >> 3 >= len(body):
            return out


def _huffman_depth(counts):
    """Depth of an unlimited Huffman code over the non-zero counts."""
    heap = [(c, 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


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


_files = {}


def _file(golden, name, filt, rps, matches):
    """The encoded file of one image of _images, encoded once for the tests that look at it."""
    key = (name, filt, rps, matches)
    if key not in _files:
        _files[key], = _encode(_images(golden)[name], filter=filt, rows_per_strip=rps, matches=matches)
    return _files[key]


@pytest.mark.parametrize("name", NAMES)
def test_round_trip_and_structure(golden, name):
    """Test 1: every filter x rows_per_strip in {1, 3, 16, H}; PIL returns the input, the file is
    built as the format says, and every strip's payload inflates on its own to its filtered bytes."""
    a = _images(golden)[name]
    H, W = a.shape[:2]
    for filt in FILTERS:
        for rps in sorted({1, 3, 16, H}):
            data = _file(golden, name, filt, rps, "lz")
            assert np.array_equal(_decode(data), a), (name, filt, rps)
            raw = _check_structure(data, H, W, rps, filt)
            _check_strips_stand_alone(data, raw, H, W, rps)


def test_matches_are_taken(golden):
    """The mode does something: the constant image's strips are matched blocks, and the file
    differs from the literal-only one."""
    data = _file(golden, "constant", "none", 16, "lz")
    for body in _strip_streams(data):
        blocks = _blocks(body)
        assert blocks[0]["type"] == 2 and blocks[0]["matches"]
    assert data != _file(golden, "constant", "none", 16, "none")


def _append(stream, rowb, values):
    """Append filtered bytes to `stream`; a byte that falls on a row's first position is preceded by
    that row's filter byte 0."""
    for v in values:
        if len(stream) % rowb == 0:
            stream.append(0)
        stream.append(int(v))


def _copy(stream, rowb, dist, length):
    """Append `length` bytes each equal to the byte `dist` before it (a filter byte in the way only
    interrupts the copy)."""
    for _ in range(length):
        if len(stream) % rowb == 0:
            stream.append(0)
        stream.append(stream[len(stream) - dist])


def test_every_length_and_distance_code():
    """Test 2: filter none, one strip of about 73 KB: a random block of 33 KB, then one copy per
    match length 3 .. 258 and one per distance-code boundary, random bytes between them."""
    W = 1000
    rowb = 3 * W + 1
    rng = np.random.default_rng(21)
    stream = []
    _append(stream, rowb, rng.integers(0, 256, 33000))
    for length in range(3, 259):
        _copy(stream, rowb, 5000 + 7 * length, length)
        _append(stream, rowb, rng.integers(0, 256, 3))
    dists = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577, 32768]
    for dist in dists + [d - 1 for d in dists[4:]]:
        _copy(stream, rowb, dist, 12)
        _append(stream, rowb, rng.integers(0, 256, 3))
    H = -(-len(stream) // rowb)
    _append(stream, rowb, rng.integers(0, 256, H * rowb - len(stream)))
    assert len(stream) == H * rowb > 33 * 1024
    f = np.array(stream, np.uint8).reshape(H, rowb)
    assert (f[:, 0] == 0).all()
    a = np.ascontiguousarray(f[:, 1:]).reshape(H, W, 3)
    data, = _encode(a, filter="none", rows_per_strip=H, matches="lz")
    assert np.array_equal(_decode(data), a)
    raw = _check_structure(data, H, W, H, "none")
    _check_strips_stand_alone(data, raw, H, W, H)
    block = _blocks(_strip_streams(data)[0])[0]
    lengths = {m[0] for m in block["matches"]}
    print(f"{len(block['matches'])} matches, {len(lengths)} distinct lengths, "
          f"longest distance {max(m[1] for m in block['matches'])}")
    assert block["type"] == 2 and block["matches"]


@pytest.mark.parametrize("W", [2048, 4096, 5461, 8192, 10922])
def test_far_distance_codes(W):
    """The hash tables rarely keep a position for tens of thousands of bytes, so test 2's far copies
    are seldom taken; the byte above is always tried.  Two equal rows of noise, 3W + 1 = 6145,
    12289, 16384, 24577 and 32767 bytes apart: the distance codes 25 .. 29, at a code's first
    distance and at its last, in a stream that has to round-trip."""
    row = np.random.default_rng(W).integers(0, 256, (1, W, 3), dtype=np.uint8)
    a = np.concatenate([row, row], 0)
    data, = _encode(a, filter="none", rows_per_strip=2, matches="lz")
    assert np.array_equal(_decode(data), a)
    raw = _check_structure(data, 2, W, 2, "none")
    _check_strips_stand_alone(data, raw, 2, W, 2)
    block = _blocks(_strip_streams(data)[0])[0]
    assert block["type"] == 2 and any(d == 3 * W + 1 for _, d in block["matches"])


def test_distance_limit():
    """Test 3: the only repeats of a 48016-byte strip are 42014 bytes back, further than a deflate
    distance reaches; zlib refuses a stream that uses one."""
    H, W = 16, 1000
    a = np.random.default_rng(22).integers(0, 256, (H, W, 3), dtype=np.uint8)
    a[14] = a[0]
    assert 14 * (3 * W + 1) == 42014 > 32768
    data, = _encode(a, filter="none", rows_per_strip=16, matches="lz")
    assert np.array_equal(_decode(data), a)
    raw = _check_structure(data, H, W, 16, "none")
    _check_strips_stand_alone(data, raw, H, W, 16)
    for block in _blocks(_strip_streams(data)[0]):
        assert all(d <= 32768 for _, d in block.get("matches", []))


@pytest.mark.parametrize("colour,period", [((7, 7, 7), 1), ((10, 20, 30), 3)])
def test_overlapping_matches(colour, period):
    """Test 4: constant images repeat with period 1 / 3, so a match's distance is shorter than its
    length, and few distance codes are used.  A length-258 match costs at most 15 + 15 + 13 bits,
    the dynamic header at most about 290 bytes, the first `period` literals at most 15 bits each:
    at most 6 * ceil(n / 258) + 2 * period + 320 bytes per strip of n filtered bytes, where
    Huffman-only needs at least n / 8."""
    H, W = 40, 200
    a = np.empty((H, W, 3), np.uint8)
    a[:] = colour
    data, = _encode(a, filter="none", rows_per_strip=16, matches="lz")
    assert np.array_equal(_decode(data), a)
    raw = _check_structure(data, H, W, 16, "none")
    _check_strips_stand_alone(data, raw, H, W, 16)
    for k, body in enumerate(_strip_streams(data)):
        n = min(16, H - 16 * k) * (3 * W + 1)
        bound = 6 * -(-n // 258) + 2 * period + 320
        print(f"colour {colour} strip {k}: {len(body)} B of deflate data, bound {bound}, n / 8 = {n / 8:.0f}")
        assert len(body) <= bound
        block = _blocks(body)[0]
        assert any(d < length for length, d in block["matches"])


def _deep_code_round_trip(a, what):
    """Round trip of a one-strip image under filter none whose strip has to be a matched block;
    returns the literal/length histogram read back from the file."""
    H, W = a.shape[:2]
    data, = _encode(a, filter="none", rows_per_strip=H, matches="lz")
    assert np.array_equal(_decode(data), a)
    raw = _check_structure(data, H, W, H, "none")
    _check_strips_stand_alone(data, raw, H, W, H)
    block = _blocks(_strip_streams(data)[0])[0]
    assert block["type"] == 2 and block["matches"]  # the matched block is the one written
    print(f"{what}: {len(block['matches'])} matches, unlimited depth of the parse's literal/length code "
          f"{_huffman_depth(block['ll'])}, longest code sent {max(block['ll_lens'])}")
    assert max(block["ll_lens"]) <= 15 and max(block["d_lens"]) <= 15
    return block["ll"]


def _rows_without_repeats(H0, W, chain, rng):
    """H0 rows of filtered bytes (filter byte 0, then 3W bytes) in which no sequence of 3 bytes
    occurs twice, so that no matcher can take a match in them and every byte stays a literal:
    `chain` {value: count} at random places at least 4 apart, one of 64 other values everywhere
    else, each drawn so that the 3 bytes it completes, also with a chain value behind it, are new."""
    rowb = 3 * W + 1
    n = H0 * rowb
    forced = {r * rowb: 0 for r in range(H0)}
    slots = [p for p in range(8, n - 8, 4) if 4 <= p % rowb <= rowb - 4]
    values = np.repeat(np.array(list(chain), np.int64), list(chain.values()))
    rng.shuffle(values)
    for k, p in enumerate(rng.permutation(len(slots))[:len(values)]):
        forced[slots[p]] = int(values[k])
    seen, s = set(), []
    for i in range(n):
        if i in forced:
            s.append(forced[i])
        else:
            while True:
                x = int(rng.integers(192, 256))
                if i >= 2 and (s[-2], s[-1], x) in seen:
                    continue
                if i >= 1 and i + 1 in forced and (s[-1], x, forced[i + 1]) in seen:
                    continue
                break
            s.append(x)
        if i >= 2:
            assert tuple(s[-3:]) not in seen, i
            seen.add(tuple(s[-3:]))
    return np.array(s, np.uint8).reshape(H0, rowb)


def test_code_deeper_than_15():
    """Test 5: the matched block's own literal/length alphabet asks for a code deeper than 15 bits.
    The Fibonacci-count construction of test_gpu_png.py's test_code_deeper_than_15 cannot be
    used as it is: a strip of 18 byte values is mostly matches, and what is left of the counts is
    up to the matcher.  Here the parse is fixed by the input instead.  14 rows hold no 3-byte
    sequence twice (_rows_without_repeats), so all their bytes are literals for any matcher; the
    15th row repeats the 14th, 3361 = 13 * 258 + 7 bytes: 13 matches of length 258 and one of
    length 7.  The counts of the alphabet are then end-of-block 1, length code 261 1, literal
    values 1 .. 4 with 2, 3, 5, 8, length code 285 13, value 0 21 (14 of them filter bytes), values
    5 .. 11 with 34 .. 610, and 64 values of about 650 each above them: the Fibonacci chain is
    whole up to 610, and the unlimited Huffman code is 19 deep.  Checked on the symbols read back
    from the file, together with the round trip.
    A second input, the image of the old test with every row written twice, has the literal-only
    alphabet 18 deep, which the encoder sizes the strip's other form with before it writes the
    matched block."""
    H0, W = 14, 1120
    assert 3 * W + 1 == 13 * 258 + 7
    chain = {1: 2, 2: 3, 3: 5, 4: 8, 0: 21 - H0, 5: 34, 6: 55, 7: 89, 8: 144, 9: 233, 10: 377, 11: 610}
    f = _rows_without_repeats(H0, W, chain, np.random.default_rng(31))
    assert (f[:, 0] == 0).all()
    top = np.ascontiguousarray(f[:, 1:]).reshape(H0, W, 3)
    ll = _deep_code_round_trip(np.concatenate([top, top[-1:]], 0), "no repeats but one row")
    assert _huffman_depth(ll) > 15
    # the parse is the one the input fixes
    assert [ll[v] for v in range(12)] == [21, 2, 3, 5, 8, 34, 55, 89, 144, 233, 377, 610]
    assert ll[256] == 1 and ll[261] == 1 and ll[285] == 13 and sum(ll[257:]) == 14

    counts = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4197]
    order = [6] + [k for k in range(len(counts)) if k != 6]  # value 0 takes the count 21, filter bytes included
    reps = [counts[k] - (16 if v == 0 else 0) for v, k in enumerate(order)]
    pix = np.repeat(np.arange(len(order), dtype=np.uint8), reps)
    np.random.default_rng(5).shuffle(pix)
    a = np.repeat(pix.reshape(16, 228, 3), 2, 0)
    filtered = np.concatenate([np.zeros((32, 1), np.uint8), a.reshape(32, 3 * 228)], 1)
    assert _huffman_depth(np.bincount(filtered.ravel(), minlength=256).tolist() + [1]) == 18
    _deep_code_round_trip(a, "rows doubled")


@pytest.mark.parametrize("name", NAMES)
def test_never_larger_than_literal_only(golden, name):
    """Test 6: per strip the smallest of three forms is written and two of them are what
    matches="none" chooses from, so no IDAT is longer than the literal-only one -- exactly."""
    a = _images(golden)[name]
    H = a.shape[0]
    for filt in FILTERS:
        for rps in sorted({1, 3, 16, H}):
            lz = [len(b) for t, b in _chunks(_file(golden, name, filt, rps, "lz")) if t == b"IDAT"]
            none = [len(b) for t, b in _chunks(_file(golden, name, filt, rps, "none")) if t == b"IDAT"]
            assert len(lz) == len(none)
            assert all(x <= y for x, y in zip(lz, none)), (name, filt, rps)
            if name == "random":  # nothing to gain in noise: the same size as before
                assert len(_file(golden, name, filt, rps, "lz")) == len(_file(golden, name, filt, rps, "none"))


def _real_inputs(golden):
    g = golden("g4_real_crop.npz")
    to_u8 = lambda t: (np.clip(t, 0, 1) * 255).astype(np.uint8)  # noqa: E731
    img = np.ascontiguousarray(g["img_u8"])
    enh = np.ascontiguousarray(to_u8(g["enh"][0]).transpose(1, 2, 0))
    illu = np.ascontiguousarray(np.repeat(to_u8(g["illu"][0]).transpose(1, 2, 0), 3, 2))
    return {"img_u8": img, "enh": enh, "illu": illu, "panel": np.concatenate([img, enh, illu], 1)}


def _raw_deflate(b, strategy):
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, strategy)
    return len(c.compress(b) + c.flush())


@pytest.mark.parametrize("name", ["img_u8", "illu", "panel"])
def test_matching_recovers_bytes_on_real_data(golden, name):
    """Test 7: filter sub, 16-row strips.  Against zlib level 1 on the same strips' filtered bytes
    (greedy, one candidate: the same class of matcher), Huffman-only (`huff`) and with matches
    (`l1`): the device has to recover at least half of what zlib's matcher recovers."""
    a = _real_inputs(golden)[name]
    H, W = a.shape[:2]
    data, = _encode(a, filter="sub", rows_per_strip=16, matches="lz")
    assert np.array_equal(_decode(data), a)
    raw = _check_structure(data, H, W, 16, "sub")
    streams = _strip_streams(data)
    n = 16 * (3 * W + 1)
    strips = [raw[k * n:(k + 1) * n] for k in range(len(streams))]
    dev = sum(len(s) for s in streams)
    huff = sum(_raw_deflate(s, zlib.Z_HUFFMAN_ONLY) for s in strips)
    l1 = sum(_raw_deflate(s, zlib.Z_DEFAULT_STRATEGY) for s in strips)
    print(f"{name}: device_lz {dev} B, huff {huff} B, l1 {l1} B, floor {huff - 0.5 * (huff - l1):.0f} B, "
          f"device_lz / l1 {dev / l1:.3f}")
    assert dev <= huff - 0.5 * (huff - l1)


def test_reproducible():
    """Test 8: same bytes on a second call; an image's bytes do not depend on its batch."""
    rng = np.random.default_rng(2)
    abc = [rng.integers(0, 256 >> k, (37, 53, 3), dtype=np.uint8) for k in (0, 3, 6)]
    three = _encode(np.stack(abc), matches="lz")
    assert three == _encode(np.stack(abc), matches="lz")
    assert three[1] == _encode(abc[1], matches="lz")[0]
    for k in range(3):
        assert np.array_equal(_decode(three[k]), abc[k])


def _write_input(path, H=48, W=60):
    rng = np.random.default_rng(4)
    a = (rng.integers(0, 256, (H, W, 3)) * 0.35).astype(np.uint8)
    Image.fromarray(a).save(path)


def _same_pngs(d0, d1, names):
    for n in names:
        a, b = np.array(Image.open(os.path.join(d0, n))), np.array(Image.open(os.path.join(d1, n)))
        assert a.shape == b.shape and np.array_equal(a, b), n
        _chunks(open(os.path.join(d1, n), "rb").read())


def test_harness_enhance_single_image_device_lz(tmp_path):
    """Test 9: the three files of png_encoder="device_lz" decode to the host encoder's pixels."""
    from enhancers.simple_enhance import enhance_single_image
    from models.model import UP_Retinex
    src = str(tmp_path / "in.png")
    _write_input(src)
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=True, use_aspp=True).to("cuda").eval()
    for enc in ("host", "device_lz"):
        enhance_single_image(model, src, str(tmp_path / enc), "cuda", max_size=64, png_encoder=enc)
    names = ["in_enhanced.png", "in_illumination.png", "in_comparison.png"]
    assert sorted(os.listdir(str(tmp_path / "device_lz"))) == sorted(names)
    _same_pngs(str(tmp_path / "host"), str(tmp_path / "device_lz"), names)


def test_harness_predict_cli_device_lz(tmp_path):
    import main as cli
    from models.model import UP_Retinex
    src = str(tmp_path / "in.png")
    _write_input(src)
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pth")
    torch.save({"model_state_dict": UP_Retinex(use_preact=True, use_aspp=True).state_dict()}, ckpt)
    for enc in ("host", "device_lz"):
        cli.main(["--mode", "predict", "--checkpoint", ckpt, "--input_path", src, "--output_dir",
                  str(tmp_path / enc), "--png_encoder", enc, "--use_preact", "--use_aspp", "--device", "cuda",
                  "--max_size", "64"])
    names = ["in_enhanced.png", "in_illumination.png", "in_comparison.png"]
    assert sorted(os.listdir(str(tmp_path / "device_lz"))) == sorted(names)
    _same_pngs(str(tmp_path / "host"), str(tmp_path / "device_lz"), names)
    h, w, _ = np.array(Image.open(str(tmp_path / "device_lz" / names[2]))).shape
    assert w % 3 == 0  # 3 panels
