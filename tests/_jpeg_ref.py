"""Reference statements for the device JPEG encoder, written from ITU-T T.81 (helper module, not a test file).

* ``reference_coefficients``: stage 1 in float64 numpy - JFIF colour transform, level shift, 2x2 chroma mean on the unrounded
  values, edge replication to whole MCUs, orthonormal 8x8 DCT-II (= T.81 A.3.3 with its 1/4 C(u) C(v) scaling), division by the
  quantisation table, round half away from zero.  Also returns the pre-rounding quotients (the tie-band test needs them).
* ``entropy_code``: a plain-Python baseline Huffman coder over a coefficient array in the device layout (per frame: Y, Cb, Cr
  planes; blocks in raster order; zigzag order inside a block): DC differences, (run, size) symbols, ZRL, EOB, byte stuffing,
  one restart interval per MCU row.
* ``make_frame``: the smooth-gradient-plus-noise test frames.
"""
import io

import numpy as np

from latentblending_amd.jpeg import EOI, HUFFMAN_SPECS, ZIGZAG, jpeg_header, jpeg_tables, mcu_geometry


def make_frame(h, w, sigma, seed=0):
    """Smooth colour gradients plus Gaussian noise of standard deviation ``sigma`` (uint8 [h, w, 3])."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([40 + 170 * x / max(w - 1, 1), 30 + 190 * y / max(h - 1, 1),
                     128 + 90 * np.sin(x / 37.0 + seed) * np.cos(y / 23.0)], axis=-1)
    return np.clip(np.rint(base + rng.normal(0.0, sigma, base.shape) if sigma else np.rint(base)), 0, 255).astype(np.uint8)


_k = np.arange(8)
DCT = np.where(_k[:, None] == 0, np.sqrt(1 / 8), 0.5 * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16))


def _plane_quotients(plane, table):
    """[H, W] float64 samples -> [blocks (raster), 64 (zigzag)] float64 coefficient / quantisation step."""
    h, w = plane.shape
    blocks = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    coef = np.einsum("uy,abyx,vx->abuv", DCT, blocks, DCT)
    quot = coef / np.asarray(table, dtype=np.float64).reshape(8, 8)
    return quot.reshape(-1, 64)[:, list(ZIGZAG)]


def reference_coefficients(frame_u8, quality=92, subsampling="4:2:0"):
    """(int16 [blocks, 64], float64 quotients [blocks, 64]) of one uint8 [H, W, 3] frame, device layout."""
    luma, chroma = jpeg_tables(quality)
    rgb = frame_u8.astype(np.float64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    ycc = [0.299 * r + 0.587 * g + 0.114 * b - 128.0,
           -0.168736 * r - 0.331264 * g + 0.5 * b + 128.0 - 128.0,
           0.5 * r - 0.418688 * g - 0.081312 * b + 128.0 - 128.0]
    h, w = r.shape
    m = 16 if subsampling == "4:2:0" else 8
    ph, pw = -h % m, -w % m
    ycc = [np.pad(p, ((0, ph), (0, pw)), mode="edge") for p in ycc]
    if subsampling == "4:2:0":
        for i in (1, 2):
            p = ycc[i]
            ycc[i] = p.reshape(p.shape[0] // 2, 2, p.shape[1] // 2, 2).mean(axis=(1, 3))
    quot = np.concatenate([_plane_quotients(ycc[0], luma), _plane_quotients(ycc[1], chroma), _plane_quotients(ycc[2], chroma)])
    rounded = np.sign(quot) * np.floor(np.abs(quot) + 0.5)
    return rounded.astype(np.int16), quot


def _code_table(bits, vals):
    """T.81 Annex C: symbol -> (code, length)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


_TABLES = {key: _code_table(*spec) for key, spec in HUFFMAN_SPECS.items()}


class _BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, length):
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def align(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _magnitude(v):
    size = abs(v).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def _code_block(bw, block, comp, pred):
    dc_table, ac_table = _TABLES[("dc", comp)], _TABLES[("ac", comp)]
    dc = int(block[0])
    size, bits = _magnitude(dc - pred)
    bw.put(*dc_table[size])
    bw.put(bits, size)
    run = 0
    for k in range(1, 64):
        v = int(block[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac_table[0xF0])
            run -= 16
        size, bits = _magnitude(v)
        bw.put(*ac_table[(run << 4) | size])
        bw.put(bits, size)
        run = 0
    if run:
        bw.put(*ac_table[0x00])
    return dc


def entropy_code(coef, h, w, subsampling="4:2:0"):
    """Scan data of one frame's coefficients ([blocks, 64], device layout): restart interval = one MCU row, RSTm between intervals."""
    coef = np.asarray(coef)
    rows, cols = mcu_geometry(h, w, subsampling)
    s420 = subsampling == "4:2:0"
    ybw, ybh = (2 * cols, 2 * rows) if s420 else (cols, rows)
    yp = coef[:ybw * ybh].reshape(ybh, ybw, 64)
    cbp = coef[ybw * ybh:ybw * ybh + rows * cols].reshape(rows, cols, 64)
    crp = coef[ybw * ybh + rows * cols:].reshape(rows, cols, 64)
    out = bytearray()
    for r in range(rows):
        bw = _BitWriter()
        pred = [0, 0, 0]
        for m in range(cols):
            if s420:
                for k in range(4):
                    pred[0] = _code_block(bw, yp[2 * r + (k >> 1), 2 * m + (k & 1)], 0, pred[0])
            else:
                pred[0] = _code_block(bw, yp[r, m], 0, pred[0])
            pred[1] = _code_block(bw, cbp[r, m], 1, pred[1])
            pred[2] = _code_block(bw, crp[r, m], 1, pred[2])
        bw.align()
        out += bw.out
        if r + 1 < rows:
            out += bytes([0xFF, 0xD0 + (r & 7)])
    return bytes(out)


def jpeg_file(coef, h, w, quality=92, subsampling="4:2:0"):
    return jpeg_header(h, w, quality, subsampling) + entropy_code(coef, h, w, subsampling) + EOI


def pillow_encode(frame_u8, quality=92, subsampling="4:2:0"):
    """Pillow's (libjpeg's) own file for the same quality and sampling, one restart interval per MCU row."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame_u8).save(buf, format="JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=1)
    return buf.getvalue()


def decode(jpeg_bytes):
    from PIL import Image
    im = Image.open(io.BytesIO(jpeg_bytes))
    im.load()
    return np.asarray(im.convert("RGB"))


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
