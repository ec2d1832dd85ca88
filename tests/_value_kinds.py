"""Seeded value-kind generators and the GEMM switches shared by the element-wise GPU tests (test_value_ranges_gpu.py,
test_gemm_epilogue_matrix_gpu.py) and the CPU model of the GEMM epilogue (_gemm_epilogue_model.py).  Everything here is computed on
the CPU from a seed; nothing depends on what a kernel returns."""
import numpy as np
import torch
import torch.nn.functional as F

from _parity import rnd

DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64


def lib():
    from latentblending_amd.hip import lib as l
    return l


class gemm_mode:
    """Variant / forced tile / forced split-K for the launches inside, the defaults afterwards."""

    def __init__(self, variant=-1, tile=0, splitk=0):
        self.v, self.t, self.s = variant, tile, splitk

    def __enter__(self):
        lib().api.lb_gemm_set_variant(self.v, 0)
        lib().api.lb_gemm_set_tuning(self.t, self.s)

    def __exit__(self, *exc):
        lib().api.lb_gemm_set_tuning(0, 0)
        lib().api.lb_gemm_set_variant(-1, 0)


# ------------------------------------------------------------------ seeded input generators
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def outlier_columns(n):
    """The fixed 1 % of columns (channels) that carry outliers: 7, 107, 207, ..."""
    return torch.arange(7, n, 100)


def outliers(shape, seed, scale=1.0):
    """N(0, 1) * scale with the outlier columns (last axis) multiplied by 64, as fp16."""
    x = torch.randn(*shape, generator=_gen(seed)) * scale
    x[..., outlier_columns(shape[-1])] *= 64.0
    return x.to(F16)


def tame_outlier_weights(w, axis=-1):
    """The matching weight columns divided by 8 (keeps outputs in range)."""
    w = w.clone().float()
    w.index_copy_(axis % w.dim(), outlier_columns(w.shape[axis]), w.index_select(axis % w.dim(), outlier_columns(w.shape[axis])) / 8.0)
    return w.to(F16)


def banded(shape, lo_exp, hi_exp, seed, positive=False):
    """sign * 2^u, u uniform in [lo_exp, hi_exp): every magnitude a normal fp16 that survives an exact rescale by 2^+-6 as long as
    lo_exp >= -8 and hi_exp <= 9."""
    g = _gen(seed)
    u = torch.rand(*shape, generator=g, dtype=F64) * (hi_exp - lo_exp) + lo_exp
    s = torch.ones(shape, dtype=F64) if positive else (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    x = (s * torch.exp2(u)).to(F16)
    assert bool((x.float().abs() >= 2.0 ** -14).all()) and bool(torch.isfinite(x).all())
    return x


def subnormal(shape, seed):
    """Every value a non-zero fp16 subnormal (bit patterns 1 .. 1023, random sign)."""
    g = _gen(seed)
    bits = torch.randint(1, 1024, shape, generator=g, dtype=torch.int32) | (torch.randint(0, 2, shape, generator=g, dtype=torch.int32) << 15)
    x = torch.from_numpy(bits.numpy().astype(np.uint16).view(np.float16).copy())
    assert bool((x != 0).all()) and bool((x.float().abs() < 2.0 ** -14).all())
    return x


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


# ------------------------------------------------------------------ convolution operands and references
def _nchw64(x_nhwc):
    return x_nhwc.double().permute(0, 3, 1, 2)


def _conv_operands(kind, xshape, cout, seed, kh=3):
    """x [B, H, W, Cin] fp16 NHWC, w [Cout, Cin, kh, kh] fp16, of one value kind."""
    B, H, Wd, cin = xshape
    wshape, wscale = (cout, cin, kh, kh), (cin * kh * kh) ** -0.5
    if kind == "normal":
        return rnd(*xshape, seed=seed), rnd(*wshape, seed=seed + 1, scale=wscale)
    if kind == "outliers":
        return outliers(xshape, seed + 2), tame_outlier_weights(rnd(*wshape, seed=seed + 3, scale=wscale), axis=1)
    if kind == "sub_a":
        return subnormal(xshape, seed + 4), banded(wshape, 8, 12, seed + 5)
    if kind == "sub_w":
        return banded(xshape, 8, 12, seed + 6), subnormal(wshape, seed + 7)
    if kind == "banded":
        return banded(xshape, -3, 1, seed + 8), banded(wshape, -4, 0, seed + 9)
    raise KeyError(kind)


def _subpixel_ref(x, k4, fn=lambda t: t):
    """fp64 result of the one-launch 2x2 sub-pixel upsampler conv from the operands the kernel reads: x [B, H, W, Cin] and the four
    stacked kernels k4 [4][Cout][2 * 2 * Cin] (parities (0,0), (0,1), (1,0), (1,1)): output pixel (2y + py, 2x + px) sees source
    pixels (y + a - 1 + py, x + b - 1 + px), a, b in {0, 1}.  ``fn`` = abs for the |x| . |w| term of the bound."""
    B, H, Wd, cin = x.shape
    cout = k4.shape[1]
    xp = F.pad(fn(_nchw64(x)), (1, 1, 1, 1))
    out = torch.zeros(B, 2 * H, 2 * Wd, cout, dtype=F64)
    for i, (py, px) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        k = fn(k4[i].double()).reshape(cout, 2, 2, cin).permute(0, 3, 1, 2)
        out[:, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + Wd + 1], k).permute(0, 2, 3, 1)
    return out
