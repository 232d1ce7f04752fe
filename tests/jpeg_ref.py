"""numpy restatement of DESIGN.md section 5, "JPEG out": an rgb24 frame (H, W, 3) uint8 -> the bytes of its baseline JPEG.  Written from the
definition, not from csrc/jpeg.hip; all of it is integer arithmetic, so the bytes are exact.  ``encode(..., wrong="...")`` gives one of the
misreadings of the definition that tests/test_jpeg_cpu.py tells apart from it."""
from __future__ import annotations

import numpy as np

HEADER_BYTES = 629
MAX_SIDE = 16384

# Annex K, Table K.1 / K.2, natural (row-major) order
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32)

# ZIGZAG[k] = natural index of the k-th coefficient of the scan
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K, Tables K.3 - K.6: code counts per length 1..16, then the symbols in code order
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

WRONG = ("no_stuffing", "zero_padding", "dc_not_reset", "rst_no_wrap", "natural_dqt", "rounding_quantiser", "limited_y", "zero_edges")


def dct_matrix():
    """M = round(2^14 A), A the orthonormal 8-point DCT-II matrix."""
    u = np.arange(8)[:, None]
    x = np.arange(8)[None, :]
    A = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    A[0] = np.sqrt(1 / 8)
    return np.round(A * 2 ** 14).astype(np.int64)


def quant_tables(quality):
    """The scaled tables (luma, chroma) in natural order, as libjpeg scales them."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must be in 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int64) for base in (BASE_LUMA, BASE_CHROMA))


def huffman_codes(table):
    """{symbol: (code, length)} of a (counts, symbols) table: the canonical codes of Annex C."""
    counts, symbols = table
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def mcu_grid(H, W, subsampling):
    side = 16 if subsampling == "420" else 8
    return side, -(-H // side), -(-W // side)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(H, W, quality, subsampling, wrong=None):
    """Everything before the scan: SOI, APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS (629 bytes)."""
    if subsampling not in ("420", "444"):
        raise ValueError("subsampling is '420' or '444'")
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("H and W must be in 1..16384")
    _, _, mcux = mcu_grid(H, W, subsampling)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, Q in enumerate(quant_tables(quality)):
        out += _segment(0xDB, bytes([i]) + bytes(int(v) for v in (Q if wrong == "natural_dqt" else Q[ZIGZAG])))
    hv = 0x22 if subsampling == "420" else 0x11
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (counts, symbols) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(counts) + bytes(symbols))
    out += _segment(0xDD, mcux.to_bytes(2, "big"))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == HEADER_BYTES
    return out


def planes(rgb, subsampling, wrong=None):
    """Y, Cb, Cr (int64) of the frame padded to whole MCUs; Cb and Cr at half size for "420"."""
    H, W, _ = rgb.shape
    side, mcuy, mcux = mcu_grid(H, W, subsampling)
    R, G, B = (rgb[..., c].astype(np.int64) for c in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    if wrong == "limited_y":
        Y = ((66 * R + 129 * G + 25 * B + 128) >> 8) + 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    pad = ((0, mcuy * side - H), (0, mcux * side - W))
    mode = dict(mode="constant") if wrong == "zero_edges" else dict(mode="edge")
    Y, Cb, Cr = (np.pad(p, pad, **mode) for p in (Y, Cb, Cr))
    if subsampling == "420":
        Cb, Cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (Cb, Cr))
    return Y, Cb, Cr


def quantised_blocks(plane, Q, wrong=None):
    """plane (8 m, 8 n) -> (m, n, 64) quantised coefficients in zigzag order."""
    M = dct_matrix()
    m, n = plane.shape[0] // 8, plane.shape[1] // 8
    X = plane.reshape(m, 8, n, 8).transpose(0, 2, 1, 3) - 128            # [m][n][y][x]
    T = (X @ M.T + (1 << 10)) >> 11                                     # rows
    U = (M @ T + (1 << 13)) >> 14                                       # columns: the coefficient x 8
    Qm = Q.reshape(8, 8)
    if wrong == "rounding_quantiser":
        c = np.round(U / (8.0 * Qm)).astype(np.int64)                   # round half to even on the exact quotient
    else:
        c = np.sign(U) * ((np.abs(U) + 4 * Qm) // (8 * Qm))
    return c.reshape(m, n, 64)[..., ZIGZAG]


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def flush(self, pad_bit=1):
        pad = -self.n % 8
        self.put(((1 << pad) - 1) * pad_bit, pad)
        return self.acc.to_bytes(self.n // 8, "big")


def _magnitude(v):
    """(category, the category's extra bits) of a non-zero or zero value."""
    cat = int(abs(v)).bit_length()
    return cat, (v if v >= 0 else v - 1) & ((1 << cat) - 1)


def _put_block(bits, c, pred, dc_codes, ac_codes, stats):
    cat, extra = _magnitude(int(c[0]) - pred)
    stats["dc_category"] = max(stats["dc_category"], cat)
    bits.put(*dc_codes[cat])
    bits.put(extra, cat)
    stats["no_eob"] += int(c[63] != 0)
    run = 0
    for k in range(1, 64):
        v = int(c[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac_codes[0xF0])
            stats["zrl"] += 1
            run -= 16
        cat, extra = _magnitude(v)
        stats["ac_category"] = max(stats["ac_category"], cat)
        bits.put(*ac_codes[(run << 4) | cat])
        bits.put(extra, cat)
        run = 0
    if run:
        bits.put(*ac_codes[0x00])
    return int(c[0])


def encode(rgb, quality=90, subsampling="420", wrong=None, stats=None):
    """The JPEG of one rgb24 frame (H, W, 3) uint8 as bytes.  ``stats``: a dict that receives what the stream reached - the largest DC and
    AC category, ZRL codes, blocks without EOB, stuffed bytes, restart markers."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    assert wrong is None or wrong in WRONG, wrong
    H, W, _ = rgb.shape
    out = bytearray(header(H, W, quality, subsampling, wrong))
    _, mcuy, mcux = mcu_grid(H, W, subsampling)
    QY, QC = quant_tables(quality)
    Y, Cb, Cr = planes(rgb, subsampling, wrong)
    cY, cCb, cCr = quantised_blocks(Y, QY, wrong), quantised_blocks(Cb, QC, wrong), quantised_blocks(Cr, QC, wrong)
    dcl, acl, dcc, acc = (huffman_codes(t) for t in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA))
    k = 2 if subsampling == "420" else 1
    pred = [0, 0, 0]
    st = dict(dc_category=0, ac_category=0, zrl=0, no_eob=0, stuffed=0, restarts=0)
    for r in range(mcuy):
        bits = _Bits()
        if wrong != "dc_not_reset":
            pred = [0, 0, 0]
        for m in range(mcux):
            for by in range(k):
                for bx in range(k):
                    pred[0] = _put_block(bits, cY[r * k + by, m * k + bx], pred[0], dcl, acl, st)
            pred[1] = _put_block(bits, cCb[r, m], pred[1], dcc, acc, st)
            pred[2] = _put_block(bits, cCr[r, m], pred[2], dcc, acc, st)
        seg = bits.flush(0 if wrong == "zero_padding" else 1)
        st["stuffed"] += seg.count(b"\xff")
        st["restarts"] += int(r + 1 < mcuy)
        out += seg if wrong == "no_stuffing" else seg.replace(b"\xff", b"\xff\x00")
        if r + 1 < mcuy:
            out += bytes([0xFF, 0xD0 + (r if wrong == "rst_no_wrap" else r % 8)])
    out += b"\xff\xd9"
    if stats is not None:
        stats.update(st)
    return bytes(out)


def default_cap(H, W):
    return H * W * 3 + 1024


def bound(H, W, subsampling):
    """A guaranteed upper bound: 20 bits of DC and 63 x 26 bits of AC a block, every byte stuffed, a marker after every MCU row."""
    _, mcuy, mcux = mcu_grid(H, W, subsampling)
    blocks = mcux * (6 if subsampling == "420" else 3)
    seg = (blocks * (20 + 63 * 26) + 7) // 8
    return HEADER_BYTES + mcuy * (2 * seg + 2)
