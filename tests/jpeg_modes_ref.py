"""Pure numpy / Python restatement of the device JPEG encoder's further modes (upr.jpeg,
DESIGN.md 4.6): chroma subsampling "444" | "420" | "gray" and Huffman tables "standard" (Annex K)
or optimised per image.  It extends tests/jpeg_ref.py, whose tables, DCT and quantisation it
imports; for ("444", standard) encode() returns jpeg_ref.encode's bytes.  Every step is integer
arithmetic, so the device file can be compared byte for byte.
"""
import numpy as np

from jpeg_ref import (AC_BITS, AC_VALS, BASE_CHROMA, BASE_LUMA, DC_BITS, DC_VALS, DCT, ZIGZAG, _segment,
                      huffman_codes, quant_table)

SUBSAMPLINGS = ("444", "420", "gray")
MCU_PIXELS = {"444": 8, "420": 16, "gray": 8}
UNITS_PER_MCU = {"444": 3, "420": 6, "gray": 1}
# a DC code and 11 value bits, 63 AC codes with 10 value bits each: the longest Annex K codes are
# 11 (DC) and 16 (AC) bits, an optimised table's longest code is 16 bits
MAX_BLOCK_BITS = {False: (11 + 11) + 63 * (16 + 10), True: (16 + 11) + 63 * (16 + 10)}
SCALE_LIMIT = 1 << 22


# ---- optimised Huffman tables ------------------------------------------------------------------
def optimal_table(freq):
    """(bits[16], vals, limited) of the counts freq[0..255] (entry 256, if present, is ignored):
    Annex K.2 as libjpeg's jpeg_gen_optimal_table states it, after halving the counts while their
    total exceeds 2^22.  limited: steps of the Figure K.3 length limit taken."""
    f = [int(v) for v in list(freq)[:256]]
    f += [0] * (256 - len(f))
    while sum(f) > SCALE_LIMIT:
        f = [(v + 1) >> 1 if v else 0 for v in f]
    f.append(1)  # the reserved entry: no real symbol gets the all-ones code
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):
            if f[i] and (v is None or f[i] <= v):
                c1, v = i, f[i]
        c2, v = -1, None
        for i in range(257):
            if f[i] and i != c1 and (v is None or f[i] <= v):
                c2, v = i, f[i]
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            assert codesize[i] <= 32
            bits[codesize[i]] += 1
    limited = 0
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
            limited += 1
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i:
        bits[i] -= 1  # the reserved entry leaves
    vals = [s for length in range(1, 33) for s in range(256) if codesize[s] == length]
    assert sum(bits[1:17]) == len(vals)
    return tuple(bits[1:17]), tuple(vals), limited


# ---- geometry, headers, bound -----------------------------------------------------------------
def geometry(H, W, restart_rows, subsampling):
    """(MCUs per row, MCU rows, MCU rows per interval, Ri)."""
    m = MCU_PIXELS[subsampling]
    mw, mh = -(-W // m), -(-H // m)
    rr = min(int(restart_rows), mh)
    return mw, mh, rr, mw * rr


def headers(H, W, quality, ri, subsampling="444", tables=None):
    """SOI .. SOS.  tables: None for Annex K, else [(bits, vals)] in DHT order DC0, AC0(, DC1, AC1)."""
    gray = subsampling == "gray"
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += _segment(0xDB, bytes([0]) + bytes(quant_table(BASE_LUMA, quality)))
    if not gray:
        out += _segment(0xDB, bytes([1]) + bytes(quant_table(BASE_CHROMA, quality)))
    comps = bytes([1, 1, 0x11, 0]) if gray else bytes([3, 1, 0x22 if subsampling == "420" else 0x11, 0,
                                                       2, 0x11, 1, 3, 0x11, 1])
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + comps)
    if tables is None:
        tables = [(DC_BITS[0], DC_VALS[0]), (AC_BITS[0], AC_VALS[0]), (DC_BITS[1], DC_VALS[1]),
                  (AC_BITS[1], AC_VALS[1])][:2 if gray else 4]
    for k, (bits, vals) in enumerate(tables):
        out += _segment(0xC4, bytes([(k & 1) << 4 | k >> 1]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, ri.to_bytes(2, "big"))
    out += _segment(0xDA, bytes([1, 1, 0x00, 0, 63, 0]) if gray else bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


HEADER_BOUND = {s: len(headers(8, 8, 50, 1, s)) for s in SUBSAMPLINGS}


def bound(H, W, restart_rows=1, subsampling="444", optimize=False):
    """The encoder's file bound: the header bound (an optimised DHT segment is never longer than
    the Annex K one: at most 12 DC and 162 AC symbols), per interval its blocks at MAX_BLOCK_BITS
    rounded up to bytes, doubled for stuffing, plus 2 for the marker behind it."""
    mw, mh, rr, _ = geometry(H, W, restart_rows, subsampling)
    total = HEADER_BOUND[subsampling]
    for r0 in range(0, mh, rr):
        blocks = UNITS_PER_MCU[subsampling] * mw * min(rr, mh - r0)
        total += 2 * (-(-blocks * MAX_BLOCK_BITS[bool(optimize)] // 8)) + 2
    return total


# ---- coefficients -----------------------------------------------------------------------------
def _plane_coefficients(plane, q):
    """Level-shifted plane int64 [8 bh, 8 bw] -> quantised coefficients [bh, bw, 64], zigzag order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    t = (np.einsum("ijyn,kn->ijyk", x, DCT) + (1 << 9)) >> 10
    f = (np.einsum("kn,ijnu->ijku", DCT, t) + (1 << 15)) >> 16
    zz = f.reshape(bh, bw, 64)[..., list(ZIGZAG)]
    q = np.array(q, dtype=np.int64)
    return np.sign(zz) * ((np.abs(zz) + q // 2) // q)


def coefficients(img, quality, subsampling="444"):
    """List of per-component coefficient arrays [bh_c, bw_c, 64] (Y, Cb, Cr; Y alone for gray)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    H, W = img.shape[:2]
    m = MCU_PIXELS[subsampling]
    Hp, Wp = -(-H // m) * m, -(-W // m) * m
    p = np.pad(img, ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge").astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    ql, qc = quant_table(BASE_LUMA, quality), quant_table(BASE_CHROMA, quality)
    out = [_plane_coefficients(((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128, ql)]
    if subsampling == "gray":
        return out
    for c in ((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16,
              (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16):
        if subsampling == "420":
            c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
        out.append(_plane_coefficients(c - 128, qc))
    return out


def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, cat):
    v = int(v)
    return v if v >= 0 else v + (1 << cat) - 1


def _symbols(blk, pred):
    """[(class, symbol, value bits, number of value bits)] of one block: class 0 = DC, 1 = AC."""
    d = int(blk[0]) - pred
    cat = _category(d)
    out = [(0, cat, _value_bits(d, cat), cat)]
    run = 0
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        cat = _category(v)
        out.append((1, run << 4 | cat, _value_bits(v, cat), cat))
        run = 0
    if run:
        out.append((1, 0x00, 0, 0))
    return out


def _mcu_units(subsampling):
    """(component, block row in the MCU, block column in the MCU) in scan order."""
    if subsampling == "420":
        return [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (2, 0, 0)]
    return [(c, 0, 0) for c in range(UNITS_PER_MCU[subsampling])]


def encode(img, quality=95, restart_rows=1, subsampling="444", optimize=False):
    """(file bytes, counters) of one u8 [H,W,3] image.  counters: jpeg_ref.encode's (stuffed,
    padded_ff, zrl, no_eob, max_dc_cat, max_ac_cat) plus limited (length-limit steps over the
    image's tables) and counts (per table DC0, AC0, DC1, AC1 the 256 symbol counts)."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    restart_rows = int(restart_rows)
    if restart_rows < 1:
        raise ValueError(f"restart_rows must be >= 1, got {restart_rows}")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")
    mw, mh, rr, ri = geometry(H, W, restart_rows, subsampling)
    if H > 65535 or W > 65535 or ri > 65535:
        raise ValueError("over the format's 16-bit fields")
    coef = coefficients(img, quality, subsampling)
    units = _mcu_units(subsampling)
    sub = 2 if subsampling == "420" else 1  # Y blocks per MCU side
    ncomp = len(coef)
    n_int = -(-mh // rr)
    # the symbols of every interval, in scan order
    intervals = []
    counts = [[0] * 256 for _ in range(4)]
    cnt = dict(stuffed=0, padded_ff=0, zrl=0, no_eob=0, max_dc_cat=0, max_ac_cat=0, limited=0)
    for i in range(n_int):
        syms, pred = [], [0] * ncomp
        for my in range(i * rr, min(mh, (i + 1) * rr)):
            for mx in range(mw):
                for c, by, bx in units:
                    s = sub if c == 0 else 1
                    blk = coef[c][my * s + by, mx * s + bx]
                    tab = min(c, 1)
                    for cls, sym, vb, nb in _symbols(blk, pred[c]):
                        syms.append((tab * 2 + cls, sym, vb, nb))
                        counts[tab * 2 + cls][sym] += 1
                        if cls == 0:
                            cnt["max_dc_cat"] = max(cnt["max_dc_cat"], nb)
                        else:
                            cnt["max_ac_cat"] = max(cnt["max_ac_cat"], nb)
                            cnt["zrl"] += sym == 0xF0
                    pred[c] = int(blk[0])
                    cnt["no_eob"] += int(blk[63]) != 0
        intervals.append(syms)
    ntab = 2 if subsampling == "gray" else 4
    if optimize:
        tables = []
        for t in range(ntab):
            bits, vals, limited = optimal_table(counts[t])
            tables.append((bits, vals))
            cnt["limited"] += limited
    else:
        tables = [(DC_BITS[0], DC_VALS[0]), (AC_BITS[0], AC_VALS[0]), (DC_BITS[1], DC_VALS[1]),
                  (AC_BITS[1], AC_VALS[1])][:ntab]
    codes = [huffman_codes(b, v) for b, v in tables]
    out = bytearray(headers(H, W, quality, ri, subsampling, tables if optimize else None))
    for i, syms in enumerate(intervals):
        acc, n = 0, 0
        for t, sym, vb, nb in syms:
            code, length = codes[t][sym]
            acc = (acc << length | code) << nb | vb
            n += length + nb
        pad = -n % 8
        acc, n = acc << pad | ((1 << pad) - 1), n + pad
        data = acc.to_bytes(n // 8, "big")
        cnt["stuffed"] += data.count(b"\xff")
        cnt["padded_ff"] += 1 if pad and data[-1] == 0xFF else 0
        out += data.replace(b"\xff", b"\xff\x00")
        if i != n_int - 1:
            out += bytes([0xFF, 0xD0 + i % 8])
    out += b"\xff\xd9"
    cnt["counts"] = counts
    return bytes(out), cnt
