"""Float64 references of wrap-around ("circular") padding, shared by test_tileable_cpu.py and test_tileable_gpu.py.

``wrap`` is the bit set of ``ConvGeom.wrap``: bit 0 = the columns wrap (x), bit 1 = the rows wrap (y).

* ``circ_conv``: the reference conv - ``F.pad(mode="circular")`` on the wrapped axes, zero padding on the other, then ``conv2d``.
* ``tile3`` / ``centre``: the tiled-image identity - the wrapped conv of X is the centre crop of the ZERO-padded conv of X repeated
  three times along each wrapped axis.  It holds to the last bit in float64 (test_tileable_cpu.py) and lets a GPU test hold a
  wrapped launch against the same launcher run unwrapped.
* ``circular_oracle``: the oracle's float64 restatement of the UNet / VAE decoder (oracle/sdxl_ref.py) with every 3x3 / pad 1 conv
  replaced by ``circ_conv`` for the length of a ``with`` block; ``circular_units`` / ``circular_taesd``: the same for
  tests/_model_units.py (the storage model of the units) and for the TAESDXL restatement tests/_taesd_ref.py.
"""
import contextlib

import torch
import torch.nn.functional as F

F64 = torch.float64


def circ_pad(x, wrap, pad=1):
    """x [B, C, H, W] padded by ``pad`` on all four sides: wrap-around on the wrapped axes, zeros on the other."""
    if wrap & 1:
        x = F.pad(x, (pad, pad, 0, 0), mode="circular")
    else:
        x = F.pad(x, (pad, pad, 0, 0))
    if wrap & 2:
        x = F.pad(x, (0, 0, pad, pad), mode="circular")
    else:
        x = F.pad(x, (0, 0, pad, pad))
    return x


def circ_conv(x, w, bias=None, wrap=0, stride=1, ups=0):
    """3x3 / pad 1 conv of x [B, C, H, W] (NCHW, any float dtype; computed in the dtype given) on the nearest-2^ups upsampled input
    with wrap-around padding on the axes of ``wrap``."""
    if ups:
        x = F.interpolate(x, scale_factor=2 ** ups, mode="nearest")
    return F.conv2d(circ_pad(x, wrap), w, bias, stride=stride, padding=0)


def tile3(x, wrap, dims=(2, 3)):
    """x repeated three times along each wrapped axis (``dims`` = (row axis, column axis) of x)."""
    reps = [1] * x.dim()
    if wrap & 2:
        reps[dims[0]] = 3
    if wrap & 1:
        reps[dims[1]] = 3
    return x.repeat(*reps)


def centre(y, wrap, H, W, dims=(2, 3)):
    """The centre H x W crop of a result computed on ``tile3`` (its wrapped axes are three times as long)."""
    if wrap & 2:
        y = y.narrow(dims[0], H, H)
    if wrap & 1:
        y = y.narrow(dims[1], W, W)
    return y


@contextlib.contextmanager
def circular_oracle(wrap):
    """oracle.sdxl_ref with wrap-around padding in every 3x3 / pad 1 conv (stride 1 and 2; the upsamplers interpolate first, so
    their conv is a plain 3x3): the module's one conv helper is substituted, nothing is edited.  1x1 / pad 0 convs are untouched."""
    from oracle import sdxl_ref as R
    zero_padded = R._conv

    def conv(x, w, p, stride=1, pad=1):
        wt = w[p + ".weight"]
        if wrap and pad == 1 and tuple(wt.shape[-2:]) == (3, 3):
            return F.conv2d(circ_pad(x, wrap), wt, w[p + ".bias"], stride=stride, padding=0)
        return zero_padded(x, w, p, stride=stride, pad=pad)
    R._conv = conv
    try:
        yield R
    finally:
        R._conv = zero_padded


def subpixel_on_wrapped_grid(x, w3, wrap, sub_weights):
    """"nearest-2x, then 3x3" as the project computes it under wrap: the four pre-summed 2x2 kernels ``sub_weights(w3)`` ->
    {(py, px): [N, 4 Cin] in (ky, kx, cin) order} applied on the LOW-resolution grid of x [B, C, H, W], where a tap outside the grid
    reads coordinate c mod size on a wrapped axis and zero on the other; output [B, N, 2H, 2W] in x's dtype."""
    B, Cc, H, W = x.shape
    N = w3.shape[0]
    xp = circ_pad(x, wrap)                                   # low-res grid with one ring: index i + 1 holds coordinate i
    out = torch.zeros(B, N, 2 * H, 2 * W, dtype=x.dtype)
    subs = sub_weights(w3)
    for py in (0, 1):
        for px in (0, 1):
            k = subs[(py, px)].to(x.dtype).reshape(N, 2, 2, Cc).permute(0, 3, 1, 2)       # [N, C, ky, kx]
            # parity (py, px): taps (ky, kx) read low-res pixel (y - (1 - py) + ky, x - (1 - px) + kx)
            win = xp[:, :, py:py + H + 1, px:px + W + 1]
            out[:, :, py::2, px::2] = F.conv2d(win, k)
    return out


@contextlib.contextmanager
def circular_units(wrap):
    """tests/_model_units.py under wrap-around padding: ``circular_oracle`` for every ``R._conv`` the units call, and the
    upsampler unit (``subpixel_conv``: REF = nearest-2x then 3x3, MODEL = the four fp16-rounded 2x2 kernels on the low-res grid) with
    its zero ring replaced by ``circ_pad``.  Same rounding points as the zero-padded units."""
    import _model_units as MU
    zero_padded = MU.subpixel_conv

    def subpixel_conv(ev, h, p):
        w, b = ev.w[p + ".weight"], ev.w[p + ".bias"]
        if not ev.store:
            return F.conv2d(circ_pad(F.interpolate(h, scale_factor=2.0, mode="nearest"), wrap), w, b)
        B, Cc, H, W = h.shape
        w64 = w.double()
        rows = {0: [w64[:, :, 0], w64[:, :, 1] + w64[:, :, 2]], 1: [w64[:, :, 0] + w64[:, :, 1], w64[:, :, 2]]}
        hp = circ_pad(h, wrap)
        out = h.new_zeros(B, w.shape[0], 2 * H, 2 * W)
        for py in (0, 1):
            for px in (0, 1):
                k = torch.zeros(w.shape[0], Cc, 2, 2, dtype=F64)
                for a in (0, 1):
                    r = rows[py][a]
                    cols = [r[:, :, 0], r[:, :, 1] + r[:, :, 2]] if px == 0 else [r[:, :, 0] + r[:, :, 1], r[:, :, 2]]
                    for c in (0, 1):
                        k[:, :, a, c] = cols[c]
                y = F.conv2d(hp, k.to(torch.float16).to(ev.dt), b)
                out[:, :, py::2, px::2] = y[:, :, py:py + H, px:px + W]
        return out
    MU.subpixel_conv = subpixel_conv
    try:
        with circular_oracle(wrap):
            yield MU
    finally:
        MU.subpixel_conv = zero_padded


@contextlib.contextmanager
def circular_taesd(wrap):
    """tests/_taesd_ref.py (the float64 TAESDXL restatement) with wrap-around padding: its ``F.conv2d(..., padding=1)`` calls go
    through a stand-in for the module's ``F`` for the length of the block; every other function of ``F`` is torch's."""
    import types

    import _taesd_ref as TR
    real = TR.F

    def conv2d(x, w, b=None, padding=0, **kw):
        if padding == 1 and tuple(w.shape[-2:]) == (3, 3):
            return real.conv2d(circ_pad(x, wrap), w, b, padding=0, **kw)
        return real.conv2d(x, w, b, padding=padding, **kw)
    TR.F = types.SimpleNamespace(conv2d=conv2d, relu=real.relu, interpolate=real.interpolate)
    try:
        yield TR
    finally:
        TR.F = real
