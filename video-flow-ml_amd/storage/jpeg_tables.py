"""Tables and header of the project's baseline JPEG: the ITU T.81 Annex K quantisation and
Huffman tables, libjpeg's quality scaling, the integer DCT matrix and the marker segments in front of the scan.
Host only, pure Python / numpy, no Pillow.  The HIP encoder (vfml/csrc/jpeg.hip) reads the same numbers from
vfml/csrc/jpeg_tables.inc, which vfml/csrc/make_jpeg_tables.py prints from this module.
"""
import struct

import numpy as np

# Annex K.1 / K.2, natural (row-major) order
QUANT_LUMA = (
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99)
QUANT_CHROMA = (
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99)

# ZIGZAG[k] = natural index of the k-th coefficient of the scan
ZIGZAG = (
    0, 1, 8, 16, 9, 2, 3, 10,
    17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34,
    27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36,
    29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46,
    53, 60, 61, 54, 47, 55, 62, 63)

# Annex K.3: (codes of each length 1..16, symbols in code order)
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa))
HUFFMAN = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)      # in the order of the DHT segments: DC0, AC0, DC1, AC1

SOI, EOI = b'\xff\xd8', b'\xff\xd9'


def quant_tables(quality):
    """uint8 [2, 64], natural order: the luma and chroma tables at `quality` (1..100), scaled as libjpeg does."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"JPEG quality {quality!r} is not in 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([QUANT_LUMA, QUANT_CHROMA], dtype=np.int64)
    return np.clip((base * s + 50) // 100, 1, 255).astype(np.uint8)


def huffman_codes(table):
    """(bits, symbols) -> {symbol: (code, length)}, the canonical codes of T.81 Annex C."""
    bits, vals = table
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def dct_matrix():
    """int64 [8, 8]: C[k][n] = rint(8192 c_k cos((2n + 1) k pi / 16)), c_0 = sqrt(1/8), c_k = 1/2."""
    k = np.arange(8, dtype=np.float64)[:, None]
    n = np.arange(8, dtype=np.float64)[None, :]
    c = np.where(k == 0, np.sqrt(0.125), 0.5)
    return np.rint(8192.0 * c * np.cos((2 * n + 1) * k * np.pi / 16)).astype(np.int64)


# sampling -> (MCU height, MCU width) in pixels
MCU_SIZE = {"4:2:0": (16, 16), "4:2:2": (8, 16), "4:4:4": (8, 8), "grey": (8, 8)}


def mcu_grid(h, w, sampling="4:2:0"):
    """(MCU rows, MCUs per row) of an h x w picture: 16 x 16 pixels each in 4:2:0, 16 wide and 8 high in 4:2:2, 8 x 8
    in 4:4:4 and in a one-component (grey) scan."""
    mh, mw = MCU_SIZE[sampling]
    return -(-int(h) // mh), -(-int(w) // mw)


def _segment(marker, payload):
    return b'\xff' + bytes([marker]) + struct.pack('>H', len(payload) + 2) + payload


def app0_segment():
    return _segment(0xE0, b'JFIF\0' + bytes([1, 1, 0]) + struct.pack('>HH', 1, 1) + bytes([0, 0]))


def dqt_segments(quality):
    q = quant_tables(quality)
    zz = list(ZIGZAG)
    return [_segment(0xDB, bytes([t]) + q[t][zz].tobytes()) for t in (0, 1)]


# sampling -> the luma component's factor byte in SOF0 (chroma is 1x1): what the encoder writes
LUMA_FACTORS = {"4:2:0": 0x22, "4:2:2": 0x21, "4:4:4": 0x11}
BLOCKS_PER_MCU = {"4:2:0": 6, "4:2:2": 4, "4:4:4": 3}      # the luma blocks, Cb, Cr


def _encoded_sampling(sampling):
    if sampling not in LUMA_FACTORS:
        raise ValueError(f"JPEG sampling {sampling!r}: the encoder builds {', '.join(LUMA_FACTORS)}")
    return sampling


def sof0_segment(h, w, sampling="4:2:0"):
    luma = LUMA_FACTORS[_encoded_sampling(sampling)]
    return _segment(0xC0, bytes([8]) + struct.pack('>HH', h, w) + bytes([3, 1, luma, 0, 2, 0x11, 1, 3, 0x11, 1]))


def dht_segments():
    return [_segment(0xC4, bytes([cls << 4 | t]) + bytes(HUFFMAN[2 * t + cls][0]) + bytes(HUFFMAN[2 * t + cls][1]))
            for t in (0, 1) for cls in (0, 1)]


def dri_segment(interval):
    return _segment(0xDD, struct.pack('>H', interval))


def sos_segment():
    return _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def jpeg_header(h, w, quality, sampling="4:2:0"):
    """Everything in front of the entropy-coded scan of an h x w picture: SOI, APP0 (JFIF 1.01), DQT x 2, SOF0 (4:2:0,
    4:2:2 or 4:4:4), DHT x 4, DRI (one MCU row of that sampling per restart interval), SOS."""
    h, w = int(h), int(w)
    _encoded_sampling(sampling)
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"JPEG picture {w}x{h}: sides of 1..65535")
    return b''.join([SOI, app0_segment(), *dqt_segments(quality), sof0_segment(h, w, sampling), *dht_segments(),
                     dri_segment(mcu_grid(h, w, sampling)[1]), sos_segment()])


def jpeg_file(header, scan_bytes):
    """header + the scan + EOI."""
    return bytes(header) + bytes(scan_bytes) + EOI
