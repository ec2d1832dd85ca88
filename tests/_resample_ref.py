"""Pillow's 8-bit resampler restated in numpy (helper of test_resample_cpu.py / test_resample_gpu.py).

``Image.resize`` on an 8-bit image is integer arithmetic: per axis a window of input samples and 22-bit fixed-point weights for
every output sample (float64 filter weights, normalised, rounded half away from zero), a horizontal pass into a uint8 image, then
a vertical pass; a sample is ``clip((2**21 + sum px * k) >> 22, 0, 255)`` in int32, and a pass whose axis keeps its size is not
run.  test_resample_cpu.py holds this restatement to Pillow byte for byte; the device kernel is then held to Pillow as well.
"""
import math

import numpy as np
from PIL import Image

BITS = 22
SUPPORT = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
PIL_FILTER = {"box": Image.Resampling.BOX, "bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC,
              "lanczos": Image.Resampling.LANCZOS}
FILTERS = ("box", "bilinear", "bicubic", "lanczos")


def weight(name, x):
    if name == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if name == "bilinear":
        return max(1.0 - abs(x), 0.0)
    if name == "bicubic":
        x = abs(x)
        if x < 1.0:
            return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1
        return (((x - 5) * x + 8) * x - 4) * -0.5 if x < 2.0 else 0.0
    assert name == "lanczos"
    if not -3.0 <= x < 3.0:
        return 0.0

    def sinc(v):
        return 1.0 if v == 0.0 else math.sin(v * math.pi) / (v * math.pi)
    return sinc(x) * sinc(x / 3)


def windows(size_in, size_out, name):
    """[(first input sample, [int coefficient, ...]), ...] for every output sample of one axis."""
    scale = size_in / size_out
    fs = max(scale, 1.0)
    support = SUPPORT[name] * fs
    out = []
    for xx in range(size_out):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), size_in)
        ws = [weight(name, (x - center + 0.5) * (1.0 / fs)) for x in range(lo, hi)]      # (Pillow multiplies by the reciprocal)
        total = 0.0
        for w in ws:
            total += w
        if total != 0.0:
            ws = [w / total for w in ws]
        out.append((lo, [int(w * (1 << BITS) + (0.5 if w >= 0 else -0.5)) for w in ws]))
    return out


def kmax(size_in, size_out, name):
    """Pillow's row length of the coefficient table."""
    return int(math.ceil(SUPPORT[name] * max(size_in / size_out, 1.0))) * 2 + 1


def resample_axis(img, size_out, name, axis):
    """One pass over ``axis`` of a uint8 array."""
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((size_out,) + src.shape[1:], np.uint8)
    for i, (lo, coefs) in enumerate(windows(src.shape[0], size_out, name)):
        acc = np.full(src.shape[1:], 1 << (BITS - 1), np.int32)
        for k, c in enumerate(coefs):
            acc += src[lo + k] * np.int32(c)
        out[i] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, size_hw, name):
    """uint8 [H, W, C] -> [size_hw[0], size_hw[1], C]."""
    h, w = size_hw
    out = img
    if w != img.shape[1]:
        out = resample_axis(out, w, name, 1)
    if h != img.shape[0]:
        out = resample_axis(out, h, name, 0)
    return out.copy() if out is img else out


def pil_resize(img, size_hw, name):
    return np.asarray(Image.fromarray(img).resize((size_hw[1], size_hw[0]), PIL_FILTER[name], reducing_gap=None))


def random_frames(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
