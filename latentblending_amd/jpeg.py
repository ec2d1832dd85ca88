"""Host side of the device JPEG encoder (``csrc/jpeg.hip``): quantisation tables and the frame header.

Pure Python, no GPU: ``jpeg_tables(quality)`` is the libjpeg quality scaling of the ITU-T T.81 Annex K.1 tables (what
Pillow writes for the same ``quality``), ``jpeg_header(h, w, quality, subsampling)`` everything of a baseline JFIF file
up to and including SOS.  The header is the same for every frame of a movie; a frame is header + scan data + EOI.
"""
from __future__ import annotations

import functools
import struct
from typing import List, Tuple

SUBSAMPLINGS = {"4:2:0": 0, "4:4:4": 1}
EOI = b"\xff\xd9"

# natural (row-major) index of the k-th coefficient in zigzag order
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

# T.81 Annex K.1, natural order
_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
              72, 92, 95, 98, 112, 100, 103, 99)
_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) \
    + (99,) * 32

# T.81 Annex K.3.3: (BITS, HUFFVAL) of the four typical Huffman tables
_AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a34353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536"
    "3738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999a"
    "a2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN_SPECS = {
    ("dc", 0): (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12))),
    ("dc", 1): (bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12))),
    ("ac", 0): (bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]), _AC_LUMA_VALS),
    ("ac", 1): (bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]), _AC_CHROMA_VALS),
}
assert all(sum(bits) == len(vals) for bits, vals in HUFFMAN_SPECS.values())


def subsampling_code(subsampling) -> int:
    """0 for "4:2:0", 1 for "4:4:4" (the integer the C ABI takes); anything else is a ValueError."""
    if subsampling in SUBSAMPLINGS:
        return SUBSAMPLINGS[subsampling]
    raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLINGS)}, not {subsampling!r}")


@functools.lru_cache(maxsize=None)
def jpeg_tables(quality: int) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(luma, chroma) quantisation tables in natural order for a libjpeg ``quality`` of 1..100 (jcparam.c:
    jpeg_quality_scaling + jpeg_add_quant_table with force_baseline)."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("quality must be in 1..100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(tuple(min(255, max(1, (v * scale + 50) // 100)) for v in base) for base in (_BASE_LUMA, _BASE_CHROMA))


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def mcu_geometry(h: int, w: int, subsampling) -> Tuple[int, int]:
    """(MCU rows = restart intervals per frame, MCUs per row = the restart interval)."""
    m = 16 if subsampling_code(subsampling) == 0 else 8
    return (h + m - 1) // m, (w + m - 1) // m


@functools.lru_cache(maxsize=32)
def jpeg_header(h: int, w: int, quality: int = 92, subsampling: str = "4:2:0") -> bytes:
    """SOI, JFIF APP0, DQT, SOF0, four DHT, DRI (one MCU row), SOS of a baseline YCbCr JPEG of ``w`` x ``h`` pixels."""
    code = subsampling_code(subsampling)
    if h <= 0 or w <= 0 or h % 8 or w % 8 or h > 65528 or w > 65528:
        raise ValueError("jpeg_header: height and width must be positive multiples of 8")
    luma, chroma = jpeg_tables(quality)
    out: List[bytes] = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for idx, table in enumerate((luma, chroma)):
        out.append(_segment(0xDB, bytes([idx]) + bytes(table[n] for n in ZIGZAG)))
    y_sampling = 0x22 if code == 0 else 0x11
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, y_sampling, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for (kind, idx), (bits, vals) in HUFFMAN_SPECS.items():
        out.append(_segment(0xC4, bytes([(0x10 if kind == "ac" else 0) | idx]) + bits + vals))
    out.append(_segment(0xDD, struct.pack(">H", mcu_geometry(h, w, subsampling)[1])))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)
