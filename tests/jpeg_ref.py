"""Pure numpy / Python restatement of the device JPEG encoder's file (upr.jpeg):
baseline sequential SOF0, 8-bit, Y/Cb/Cr 4:4:4, the Annex K tables, one restart interval per
`restart_rows` block rows.  Every step is integer arithmetic, so the device file can be compared
byte for byte.  encode() also returns counters of what the entropy-coded data exercised.

The quantisation base tables (zigzag order) and the four Huffman tables are facts of the format;
tests/test_cpu_jpeg.py checks them against the DQT / DHT segments of a file PIL writes.
"""
import numpy as np

# natural (row-major) index of the coefficient at each zigzag position
ZIGZAG = []
for _s in range(15):
    _d = [(_y, _s - _y) for _y in range(8) if 0 <= _s - _y < 8]
    ZIGZAG += [y * 8 + x for y, x in (_d if _s % 2 else _d[::-1])]
ZIGZAG = tuple(ZIGZAG)

# Annex K.1 / K.2 at scale 100 (quality 50), in zigzag order as a DQT segment carries them
BASE_LUMA = (16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40,
             58, 51, 61, 60, 57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103,
             104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99)
BASE_CHROMA = (17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99) + (99,) * 48

# Annex K.3: (BITS, HUFFVAL) of the DC / AC tables of table class 0 (luma) and 1 (chroma)
DC_BITS = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0))
DC_VALS = (tuple(range(12)), tuple(range(12)))
AC_BITS = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119))
AC_VALS = (
    (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21,
     82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58,
     67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116,
     117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198,
     199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234,
     241, 242, 243, 244, 245, 246, 247, 248, 249, 250),
    (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35,
     51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56,
     57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151,
     152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195,
     196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232,
     233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250))

# forward DCT matrix in 2^13 fixed point: C[k][n] = round(2^13 s_k cos((2n + 1) k pi / 16))
DCT = np.array([[round(8192 * (np.sqrt(1 / 8) if k == 0 else 0.5) * np.cos((2 * n + 1) * k * np.pi / 16))
                 for n in range(8)] for k in range(8)], dtype=np.int64)

# longest DC code + 11 and 63 times the longest AC code + 10: no block is longer
MAX_BLOCK_BITS = (max(max(l + 1 for l, n in enumerate(b) if n) for b in DC_BITS) + 11 +
                  63 * (max(max(l + 1 for l, n in enumerate(b) if n) for b in AC_BITS) + 10))


def quant_table(base, quality):
    """The libjpeg scaling: what PIL's `quality` means."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"quality must be 1..100, got {quality}")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(min(255, max(1, (b * scale + 50) // 100)) for b in base)


def huffman_codes(bits, vals):
    """symbol -> (code, length) of the canonical code of a DHT table (Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def dht_payload(tc, th, bits, vals):
    return bytes([tc << 4 | th]) + bytes(bits) + bytes(vals)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def headers(H, W, quality, ri):
    """SOI .. SOS: everything in front of the entropy-coded data."""
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += _segment(0xDB, bytes([0]) + bytes(quant_table(BASE_LUMA, quality)))
    out += _segment(0xDB, bytes([1]) + bytes(quant_table(BASE_CHROMA, quality)))
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") +
                    bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc, th in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = (AC_BITS[th], AC_VALS[th]) if tc else (DC_BITS[th], DC_VALS[th])
        out += _segment(0xC4, dht_payload(tc, th, bits, vals))
    out += _segment(0xDD, ri.to_bytes(2, "big"))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


HEADER_BYTES = len(headers(8, 8, 50, 1))


def bound(H, W, restart_rows=1):
    """The encoder's file bound: the headers, per interval its blocks at MAX_BLOCK_BITS rounded up
    to bytes, doubled for stuffing, plus 2 for the marker behind it (RSTm, or EOI behind the last)."""
    bw, bh = -(-W // 8), -(-H // 8)
    rr = min(int(restart_rows), bh)
    total = HEADER_BYTES
    for r0 in range(0, bh, rr):
        blocks = 3 * bw * min(rr, bh - r0)
        total += 2 * (-(-blocks * MAX_BLOCK_BITS // 8)) + 2
    return total


def coefficients(img, quality):
    """Quantised coefficients int64 [3, bh, bw, 64] in zigzag order (components Y, Cb, Cr)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    H, W = img.shape[:2]
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    p = np.pad(img, ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge").astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    ycc = np.stack([(19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
                    (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16,
                    (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16]) - 128
    x = ycc.reshape(3, Hp // 8, 8, Wp // 8, 8).transpose(0, 1, 3, 2, 4)  # [3, bh, bw, y, n]
    t = (np.einsum("cijyn,kn->cijyk", x, DCT) + (1 << 9)) >> 10            # rows
    f = (np.einsum("kn,cijnu->cijku", DCT, t) + (1 << 15)) >> 16           # columns
    assert np.abs(f).max() < (1 << 12)
    zz = f.reshape(3, Hp // 8, Wp // 8, 64)[..., list(ZIGZAG)]
    q = np.array([quant_table(BASE_LUMA, quality), quant_table(BASE_CHROMA, quality),
                  quant_table(BASE_CHROMA, quality)], dtype=np.int64)[:, None, None, :]
    return np.sign(zz) * ((np.abs(zz) + q // 2) // q)


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = self.acc << length | code
        self.n += length


def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, cat):
    v = int(v)
    return v if v >= 0 else v + (1 << cat) - 1


def encode(img, quality=95, restart_rows=1):
    """(file bytes, counters) of one u8 [H,W,3] image.  counters: stuffed (0xFF bytes of the
    entropy-coded data, each followed by 0x00), padded_ff (intervals whose 1-padded last byte
    was 0xFF), zrl, no_eob (blocks whose coefficient 63 is non-zero), max_dc_cat, max_ac_cat."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    restart_rows = int(restart_rows)
    if restart_rows < 1:
        raise ValueError(f"restart_rows must be >= 1, got {restart_rows}")
    coef = coefficients(img, quality)
    _, bh, bw, _ = coef.shape
    rr = min(restart_rows, bh)
    ri = bw * rr
    if H > 65535 or W > 65535 or ri > 65535:
        raise ValueError("over the format's 16-bit fields")
    dc = [huffman_codes(DC_BITS[k], DC_VALS[k]) for k in (0, 1)]
    ac = [huffman_codes(AC_BITS[k], AC_VALS[k]) for k in (0, 1)]
    cnt = dict(stuffed=0, padded_ff=0, zrl=0, no_eob=0, max_dc_cat=0, max_ac_cat=0)
    out = bytearray(headers(H, W, quality, ri))
    n_int = -(-bh // rr)
    for i in range(n_int):
        bits, pred = _Bits(), [0, 0, 0]
        for by in range(i * rr, min(bh, (i + 1) * rr)):
            for bx in range(bw):
                for c in range(3):
                    blk, tab = coef[c, by, bx], min(c, 1)
                    d = int(blk[0]) - pred[c]
                    pred[c] = int(blk[0])
                    cat = _category(d)
                    cnt["max_dc_cat"] = max(cnt["max_dc_cat"], cat)
                    bits.put(*dc[tab][cat])
                    bits.put(_value_bits(d, cat), cat)
                    run = 0
                    for k in range(1, 64):
                        v = int(blk[k])
                        if v == 0:
                            run += 1
                            continue
                        while run > 15:
                            bits.put(*ac[tab][0xF0])
                            cnt["zrl"] += 1
                            run -= 16
                        cat = _category(v)
                        cnt["max_ac_cat"] = max(cnt["max_ac_cat"], cat)
                        bits.put(*ac[tab][run << 4 | cat])
                        bits.put(_value_bits(v, cat), cat)
                        run = 0
                    if run:
                        bits.put(*ac[tab][0x00])
                    else:
                        cnt["no_eob"] += 1
        pad = -bits.n % 8
        bits.put((1 << pad) - 1, pad)
        data = bits.acc.to_bytes(bits.n // 8, "big")
        cnt["stuffed"] += data.count(b"\xff")
        cnt["padded_ff"] += 1 if pad and data[-1] == 0xFF else 0
        out += data.replace(b"\xff", b"\xff\x00")
        if i != n_int - 1:
            out += bytes([0xFF, 0xD0 + i % 8])
    out += b"\xff\xd9"
    return bytes(out), cnt
