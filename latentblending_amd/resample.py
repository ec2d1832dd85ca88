"""Coefficient tables of the device frame resampler (``csrc/resample.hip``, ``ops.resample_u8``).

The tables are Pillow's, computed the way Pillow's 8-bit resampler computes them (``precompute_coeffs`` and
``normalize_coeffs_8bpc`` of its Resample.c): float64 weights of a separable filter whose support widens with the downscale
factor, normalised to sum 1 per output sample and then turned into 22-bit fixed point, rounding half away from zero.  The kernel
applies them in int32 with the same rounding and clipping, so the device result equals ``PIL.Image.resize(..., reducing_gap=None)``
byte for byte.  ``"nearest"`` is not offered: Pillow resizes that by another routine.
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

PRECISION_BITS = 32 - 8 - 2          # of a coefficient; the accumulator is int32


def _box(x: float) -> float:
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# name -> (weight function, support at scale 1, Pillow's Image.Resampling number)
FILTERS = {"box": (_box, 0.5, 4), "bilinear": (_bilinear, 1.0, 2), "bicubic": (_bicubic, 2.0, 3), "lanczos": (_lanczos, 3.0, 1)}


def check_filter(name) -> str:
    if not isinstance(name, str) or name not in FILTERS:
        raise ValueError(f"resample: filter must be one of {sorted(FILTERS)}, not {name!r}")
    return name


def check_size(size, what="size") -> Tuple[int, int]:
    """The two positive integers of ``size`` (ValueError otherwise)."""
    try:
        a, b = size
        ok = int(a) == a and int(b) == b and a > 0 and b > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"resample: {what} must be two positive integers, not {size!r}")
    return int(a), int(b)


def pil_filter(name):
    """Pillow's constant for a filter name."""
    from PIL import Image
    return Image.Resampling(FILTERS[check_filter(name)][2])


def resample_tables(size_in: int, size_out: int, filter: str = "bicubic"):
    """One axis: ``(start[int32, size_out], count[int32, size_out], coef[int32, size_out, kmax])``.  Output sample ``i`` is
    ``(2**21 + sum_k in[start[i] + k] * coef[i, k]) >> 22`` over ``k < count[i]``, clipped to 0..255; entries behind ``count[i]`` are 0."""
    if int(size_in) != size_in or int(size_out) != size_out or size_in <= 0 or size_out <= 0:
        raise ValueError(f"resample_tables: sizes must be positive integers, not {size_in!r} -> {size_out!r}")
    size_in, size_out = int(size_in), int(size_out)
    weight, support0, _ = FILTERS[check_filter(filter)]
    scale = size_in / size_out
    fs = max(scale, 1.0)
    support = support0 * fs
    kmax = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / fs
    start = np.zeros(size_out, np.int32)
    count = np.zeros(size_out, np.int32)
    coef = np.zeros((size_out, kmax), np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(size_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), size_in) - xmin
        ws = [weight((x + xmin - center + 0.5) * inv) for x in range(xmax)]
        total = 0.0
        for w in ws:                                  # (summed in order, as the C loop does)
            total += w
        if total != 0.0:
            ws = [w / total for w in ws]
        start[xx], count[xx] = xmin, xmax
        coef[xx, :xmax] = [int(-0.5 + w * one) if w < 0 else int(0.5 + w * one) for w in ws]
    return start, count, coef
