"""Which VALUES go through the kernels: every launcher of the hot path against a float64 CPU reference, ELEMENT BY ELEMENT, on the
value ranges real checkpoints reach - outlier channels, fp16 subnormals, results at the edge of fp16, group / row means far from
zero, attention scores at the deferred-rescale threshold - where test_kernels_gpu.py draws N(0, 1) and accepts any error below
2^-8 * max|ref| + 1e-3.

Every tolerance here is one of the derived bounds of tests/_parity.py (their docstrings state the derivations) or exact equality.
Families: A contractions vs fp64; B the fp16 edge of the store; C exact power-of-two rescaling (bitwise, metamorphic); D
normalisations away from zero mean (with the fp32 torch op they replace as the yardstick, logged next to the kernel's error);
E attention at hard score patterns; F element-wise kernels at their edges (exact)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import sdxl_ref as R  # noqa: E402  (checker only)
from _parity import (ACT_LIPSCHITZ, ERF_APPROX, U16, U32, absdot, accumulate_bound, activation_bound, attention_bound,  # noqa: E402,F401
                     check_elementwise, contraction_bound, epilogue_bound, f64, geglu_bound, norm_bound, rnd, store_bound, ulp_diff_f16)
from _value_kinds import (_conv_operands, _dev, _gen, _nchw64, _subpixel_ref, banded, gemm_mode, outlier_columns, outliers,  # noqa: E402,F401
                          subnormal, tame_outlier_weights)

DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
S1, S2 = (300, 260, 128), (1000, 384, 256)            # GEMM shapes (M, N, K) the suite already runs on every tile


def ops():
    from latentblending_amd.hip import ops as o
    return o


def lib():
    from latentblending_amd.hip import lib as l
    return l


class attn_force:
    def __init__(self, force):
        self.f = force

    def __enter__(self):
        lib().api.lb_attn_set_tuning(self.f)

    def __exit__(self, *exc):
        lib().api.lb_attn_set_tuning(0)


# ------------------------------------------------------------------ seeded input generators (the shared ones: tests/_value_kinds.py)
def offset(shape, ratio, std, seed, blocks, axis, dtype=F32):
    """std * N(0, 1) + (+-ratio) * std with the sign alternating over ``blocks`` equal blocks of ``axis`` (groups of channels for
    GroupNorm, rows for LayerNorm: odd blocks get -ratio)."""
    x = torch.randn(*shape, generator=_gen(seed), dtype=F64) * std
    n = shape[axis]
    sign = 1.0 - 2.0 * ((torch.arange(n) // (n // blocks)) % 2).double()
    view = [1] * len(shape)
    view[axis] = n
    return (x + ratio * std * sign.view(view)).to(dtype)


# ------------------------------------------------------------------ A. contractions against fp64, element-wise
@functools.lru_cache(maxsize=None)
def gemm_case(kind, shape):
    """Operands (fp16 on the CPU) and the float64 products of one (kind, shape): computed once, shared, never modified."""
    M, N, K = shape
    if kind == "normal":
        A, W = rnd(M, K, seed=501), rnd(N, K, seed=502, scale=K ** -0.5)
    elif kind == "outliers":
        A, W = outliers((M, K), 503), tame_outlier_weights(rnd(N, K, seed=504, scale=K ** -0.5))
    elif kind == "sub_a":
        A, W = subnormal((M, K), 505), banded((N, K), 8, 12, 506)
    elif kind == "sub_w":
        A, W = banded((M, K), 8, 12, 507), subnormal((N, K), 508)
    else:
        raise KeyError(kind)
    bias, res, rv = rnd(N, seed=509, dtype=F32), rnd(M, N, seed=510), rnd(4, N, seed=511)
    A64, W64 = A.double(), W.double()
    return dict(A=A, W=W, bias=bias, res=res, rv=rv, base=A64 @ W64.t(), ad=absdot(A64, W64))


GEMM_RUNS = [(0, 0, S1), (1, 0, S1), (3, 0, S1), (11, 0, S1), (7, 0, S2), (9, 0, S2), (10, 0, S2), (3, 2, S1), (1, 2, S1), (3, 5, S2)]


@pytest.mark.parametrize("kind", ["normal", "outliers", "sub_a", "sub_w"])
@pytest.mark.parametrize("tile,splitk,shape", GEMM_RUNS)
@pytest.mark.parametrize("variant", [0, 1])
def test_gemm_elementwise(variant, tile, splitk, shape, kind, results_log):
    """lb_gemm_f16 on both variants, the forced tiles, the automatic policy and split-K, against fp64 with contraction_bound per
    element.  N(0, 1) / outlier operands run with bias + residual; subnormal operands (paired with magnitudes 2^8 .. 2^12, so the
    results are normal fp16) run bare: a result that is exactly zero where the reference is not fails the bound by itself - the
    check for a flushed input."""
    o = ops()
    c = gemm_case(kind, shape)
    M, N, K = shape
    bare = kind.startswith("sub")
    bias, res = (None, None) if bare else (c["bias"], c["res"])
    ref = c["base"] if bare else c["base"] + bias.double() + res.double()
    Ad, Wd, bd, rd = _dev(c["A"], c["W"], bias, res)
    with gemm_mode(variant, tile, splitk):
        got = o.gemm(Ad, Wd, bias=bd, residual=rd)
    bound = contraction_bound(None, None, K, ref, bias=bias, residual=res, absdot64=c["ad"])
    check_elementwise(results_log, f"vr_gemm_{kind}_{M}x{N}x{K}_v{variant}_t{tile}_sk{splitk}", got, ref, bound)
    if bare:
        assert int((got.cpu() == 0).sum()) == int((ref.half() == 0).sum())


EPILOGUES = ["none", "bias_res_rowvec", "f32", "silu", "geglu", "quick_gelu", "gelu", "trans", "alpha"]


@pytest.mark.parametrize("kind", ["normal", "outliers"])
@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("variant", [0, 1])
def test_gemm_epilogues_elementwise(variant, epi, kind, results_log):
    """Every epilogue of lb_gemm_f16 at (300, 260, 128): the pre-activation bound goes through the activation's derivative bound
    (activation_bound / geglu_bound); OUT_F32 | RES_F32 stores fp32; alpha = 2^-4 runs on operands 64 x 256 times larger, whose
    unscaled products leave the fp16 range (the VAE's scaled residual stream), with the bias pre-scaled by the caller."""
    o, l = ops(), lib()
    M, N, K = S1
    c = gemm_case(kind, S1)
    A, W, bias, res, rv, base, ad = c["A"], c["W"], c["bias"], c["res"], c["rv"], c["base"], c["ad"]
    name = f"vr_gemm_epi_{epi}_{kind}_v{variant}"
    Ad, Wd, bd, rd, rvd = _dev(A, W, bias, res, rv)
    with gemm_mode(variant):
        if epi == "none":
            got, ref = o.gemm(Ad, Wd), base
            bound = contraction_bound(None, None, K, ref, absdot64=ad)
        elif epi == "bias_res_rowvec":
            rows = rv.double().repeat_interleave(75, 0)
            got = o.gemm(Ad, Wd, bias=bd, residual=rd, rowvec=rvd, rows_per_batch=75)
            ref = base + bias.double() + res.double() + rows
            bound = contraction_bound(None, None, K, ref, bias=bias, residual=res, rowvec=rows, absdot64=ad)
        elif epi == "f32":
            res32 = rnd(M, N, seed=512, dtype=F32, scale=100.0)
            got = o.gemm(Ad, Wd, bias=bd, residual=res32.to(DEV), flags=l.GEMM_OUT_F32 | l.GEMM_RES_F32)
            assert got.dtype == F32
            ref = base + bias.double() + res32.double()
            bound = contraction_bound(None, None, K, ref, out_f32=True, bias=bias, residual=res32, absdot64=ad)
        elif epi in ("silu", "quick_gelu", "gelu"):
            flag = {"silu": l.GEMM_SILU, "quick_gelu": l.GEMM_QUICK_GELU, "gelu": l.GEMM_GELU}[epi]
            got = o.gemm(Ad, Wd, bias=bd, flags=flag)
            y = base + bias.double()
            ref = {"silu": F.silu(y), "quick_gelu": y * torch.sigmoid(1.702 * y), "gelu": F.gelu(y)}[epi]
            bound = activation_bound(accumulate_bound(ad, K) + epilogue_bound(y, bias), ref)
        elif epi == "geglu":
            n8 = N // 8 * 8
            got = o.gemm(Ad, Wd[:n8], bias=bd[:n8], flags=l.GEMM_GEGLU)
            assert got.shape == (M, n8 // 2)
            y = base[:, :n8] + bias.double()[:n8]
            pre = accumulate_bound(ad[:, :n8], K) + epilogue_bound(y, bias[:n8])
            (h, gt), (ph, pg) = y.chunk(2, dim=-1), pre.chunk(2, dim=-1)
            ref = h * F.gelu(gt)
            bound = geglu_bound(ph, pg, h, gt, F.gelu(gt))
        elif epi == "trans":
            got, ref = o.gemm(Ad, Wd, flags=l.GEMM_TRANS_OUT), base.t()
            bound = contraction_bound(None, None, K, ref, absdot64=ad.t())
        else:       # alpha: operands scaled up exactly (powers of two), so the unscaled product reaches ~ +-80000
            sa, sw = (256, 64) if kind == "normal" else (16, 1024)      # (the outlier columns of A are 64 x larger already)
            A2, W2 = _pow2(A, int(math.log2(sa))), (W.float() * sw).to(F16)
            assert torch.isfinite(A2).all() and torch.isfinite(W2).all() and torch.equal(W2.double(), W.double() * sw)
            full = base * (256 * 64)
            assert float(full.abs().max()) > 65504, "the unscaled product must need the down-scale"
            b2 = (bias * 1024).to(DEV)                          # the caller's pre-scaled bias: alpha * (2^14 bias)
            got = o.gemm(A2.to(DEV), W2.to(DEV), bias=b2, alpha=2.0 ** -4)
            ref = full * 2.0 ** -4 + bias.double() * 1024
            bound = contraction_bound(None, None, K, ref, alpha=2.0 ** -4, bias=bias * 1024, absdot64=ad * (256 * 64))
    check_elementwise(results_log, name, got, ref, bound)


def _run_conv(op, x, w, bias, res, f32=False, alpha=1.0, relu=False):
    """One launch of conv ``op`` on CPU operands -> device output.  halo / narrow / igemm: w [Cout, Cin, 3, 3]; upconv: w = the
    stacked kernels [4][Cout][4 Cin]."""
    o, l = ops(), lib()
    flags = (l.GEMM_OUT_F32 if f32 else 0) | (l.GEMM_RELU if relu else 0)
    xd = x.to(DEV)
    bd, rd = _dev(bias, res)
    if op == "halo":
        return o.gemm(xd, o.pack_conv_weight(w, x.shape[-1]).to(DEV), bias=bd, residual=rd, flags=flags, alpha=alpha,
                      conv=dict(KH=3, KW=3, stride=1, pad=1, halo=True))
    if op == "narrow":
        cout = w.shape[0]
        wp = torch.zeros(4, 9 * x.shape[-1], dtype=F16)
        wp[:cout] = o.pack_conv_weight(w, x.shape[-1])
        bp = torch.zeros(4, dtype=F32)
        bp[:cout] = bias
        got = o.gemm(xd, wp.to(DEV), bias=bp.to(DEV), flags=flags, alpha=alpha, conv=dict(KH=3, KW=3, stride=1, pad=1))
        assert float(got[..., cout:].float().abs().max()) == 0
        return got[..., :cout]
    if op == "igemm":
        return o.gemm(xd, o.pack_conv_weight(w, x.shape[-1]).to(DEV), bias=bd, residual=rd, flags=flags, alpha=alpha,
                      conv=dict(KH=3, KW=3, stride=2, pad=1))
    if op == "upconv":
        B, H, Wd, _ = x.shape
        out = torch.full((B, 2 * H, 2 * Wd, w.shape[1]), float("nan"), dtype=F32 if f32 else F16, device=DEV)
        o.gemm(xd, w.to(DEV).contiguous()[0], bias=bd, out=out, flags=flags, alpha=alpha, conv=dict(KH=2, KW=2, stride=1, pad=0, parity="all"))
        return out
    raise KeyError(op)


CONV_OPS = {   # op -> (x shape NHWC, Cout, has residual)
    "halo": ((2, 32, 32, 64), 128, True),
    "narrow": ((2, 32, 32, 128), 3, False),
    "upconv": ((2, 16, 16, 64), 64, False),
    "igemm": ((2, 16, 16, 64), 64, True),
}


@functools.lru_cache(maxsize=None)
def conv_case(op, kind):
    xshape, cout, has_res = CONV_OPS[op]
    cin = xshape[-1]
    seed = 520 + 20 * sorted(CONV_OPS).index(op)
    if op == "upconv":
        x, w3 = _conv_operands(kind, xshape, cout, seed)
        if kind in ("normal", "outliers"):      # the kernels a model would load: four 2x2 kernels summed from a 3x3 one
            subs = ops().subpixel_upsample_weights(w3)
            w = torch.stack([subs[(0, 0)], subs[(0, 1)], subs[(1, 0)], subs[(1, 1)]])
        else:                                   # value kinds defined on the operand the kernel reads
            w = torch.stack([_conv_operands(kind, xshape, cout, seed + 100 + i, kh=2)[1].permute(0, 2, 3, 1).reshape(cout, 4 * cin)
                             for i in range(4)])
        base, ad, K = _subpixel_ref(x, w), _subpixel_ref(x, w, torch.abs), 4 * cin
    else:
        x, w = _conv_operands(kind, xshape, cout, seed)
        st = 2 if op == "igemm" else 1
        base = F.conv2d(_nchw64(x), w.double(), stride=st, padding=1).permute(0, 2, 3, 1)
        ad = F.conv2d(_nchw64(x).abs(), w.double().abs(), stride=st, padding=1).permute(0, 2, 3, 1)
        K = 9 * cin
    bias = rnd(cout, seed=seed + 10, dtype=F32)
    res = rnd(*base.shape, seed=seed + 11) if has_res else None
    return dict(x=x, w=w, bias=bias, res=res, base=base.contiguous(), ad=ad.contiguous(), K=K)


@pytest.mark.parametrize("kind", ["normal", "outliers", "sub_a", "sub_w"])
@pytest.mark.parametrize("op,f32", [("halo", False), ("narrow", False), ("narrow", True), ("upconv", False), ("igemm", False)])
def test_conv_elementwise(op, f32, kind, results_log):
    """lb_conv3x3_halo_f16, lb_conv3x3_narrow_f16 (fp16 and fp32 output), lb_upconv2x_halo_f16 and the implicit-GEMM conv (stride 2:
    not eligible for the halo kernel) against F.conv2d in float64, |x| * |w| from the same convolution of the absolute values."""
    c = conv_case(op, kind)
    bare = kind.startswith("sub")
    bias = torch.zeros_like(c["bias"]) if bare else c["bias"]
    res = None if bare else c["res"]
    ref = c["base"] + bias.double() + (0 if res is None else res.double())
    got = _run_conv(op, c["x"], c["w"], bias, res, f32=f32)
    bound = contraction_bound(None, None, c["K"], ref, out_f32=f32, bias=bias, residual=res, absdot64=c["ad"])
    check_elementwise(results_log, f"vr_conv_{op}_{kind}_f32{int(f32)}", got, ref, bound)
    if bare and not f32:
        assert int((got.cpu() == 0).sum()) == int((ref.half() == 0).sum())


# ------------------------------------------------------------------ B. the fp16 edge of the store
EDGE_LO, EDGE_HI = 2048.0, 2390.0      # times the weight 29.297 = 60000 and 70020


def _check_edge(log, name, got16, got32, ref, bound):
    """Below the edge: finite and within the bound; beyond it: the infinity .to(float16) gives the reference; in between: not
    asserted, share logged and < 0.5 %; the same operands with an fp32 output: finite everywhere and within the fp32 bound."""
    got = got16.cpu().double()
    a = ref.abs()
    below, beyond = a + bound < 65504.0, a - bound >= 65520.0
    between = ~(below | beyond)
    share = float(between.double().mean())
    log[name + "_between_share"] = share
    print(f"[parity] {name}: below={int(below.sum())} beyond={int(beyond.sum())} between share={share:.5f}")
    assert share < 0.005
    assert int(beyond.sum()) > 0 and int((below & (a > 59000)).sum()) > 0, "the case must reach both sides of the edge"
    assert bool(torch.isfinite(got[below]).all())
    check_elementwise(log, name + "_below", got[below], ref[below], bound[below])
    want_inf = torch.where(ref[beyond] > 0, torch.full_like(ref[beyond], float("inf")), torch.full_like(ref[beyond], float("-inf")))
    assert torch.equal(got[beyond], want_inf), f"{name}: results beyond 65520 must store the infinity of their sign"
    assert torch.equal(ref.half().double()[beyond], want_inf)
    assert bool(torch.isfinite(got32).all()), f"{name}: the fp32 output must be finite everywhere"


def test_gemm_store_at_the_fp16_edge(results_log):
    """Outlier operands with the weight column LEFT UNSCALED: column 7 of W is +-29.297, rows 10..19 of A hold 2048 there (results
    +-60000 + O(1)), rows 30..39 hold 2390 (+-70020)."""
    o, l = ops(), lib()
    M, N, K = S1
    A, W = outliers((M, K), 541), rnd(N, K, seed=542, scale=K ** -0.5)
    W[:, 7] = (29.297 * (1.0 - 2.0 * (torch.arange(N) % 2))).to(F16)
    A[10:20, 7], A[30:40, 7] = EDGE_LO, EDGE_HI
    ref = A.double() @ W.double().t()
    ad = absdot(A.double(), W.double())
    bound = contraction_bound(None, None, K, ref, absdot64=ad)
    for variant in (0, 1):
        with gemm_mode(variant):
            got16 = o.gemm(A.to(DEV), W.to(DEV))
            got32 = o.gemm(A.to(DEV), W.to(DEV), flags=l.GEMM_OUT_F32)
        _check_edge(results_log, f"vr_edge_gemm_v{variant}", got16, got32, ref, bound)
        check_elementwise(results_log, f"vr_edge_gemm_f32_v{variant}", got32, ref, contraction_bound(None, None, K, ref, out_f32=True, absdot64=ad))


def test_halo_conv_store_at_the_fp16_edge(results_log):
    """The same through lb_conv3x3_halo_f16: channel 7 carries the outliers, its centre tap is +-29.297 (the other taps of that
    channel are zero), image row 5 of sample 0 holds 2048 there, row 9 of sample 1 holds 2390."""
    x, w = _conv_operands("outliers", (2, 32, 32, 64), 128, 543)
    w = rnd(128, 64, 3, 3, seed=544, scale=(9 * 64) ** -0.5)
    w[:, 7] = 0
    w[:, 7, 1, 1] = (29.297 * (1.0 - 2.0 * (torch.arange(128) % 2))).to(F16)
    x[0, 5, :, 7], x[1, 9, :, 7] = EDGE_LO, EDGE_HI
    bias = torch.zeros(128, dtype=F32)
    ref = F.conv2d(_nchw64(x), w.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    ad = F.conv2d(_nchw64(x).abs(), w.double().abs(), padding=1).permute(0, 2, 3, 1).contiguous()
    got16, got32 = _run_conv("halo", x, w, bias, None), _run_conv("halo", x, w, bias, None, f32=True)
    _check_edge(results_log, "vr_edge_halo", got16, got32, ref, contraction_bound(None, None, 576, ref, absdot64=ad))
    check_elementwise(results_log, "vr_edge_halo_f32", got32, ref, contraction_bound(None, None, 576, ref, out_f32=True, absdot64=ad))


def test_cast_f32_to_f16_saturates():
    """lb_cast_f32_to_f16 documents saturation: +-65504 at +-1e6 and +-inf, NaN stays NaN, in-range values round to nearest."""
    o = ops()
    x = torch.tensor([1e6, -1e6, float("inf"), float("-inf"), float("nan"), 65519.0, -65519.0, 1.0, 3 * 2.0 ** -24, 0.1], dtype=F32)
    got = o.cast_f32_to_f16(x.to(DEV)).cpu()
    assert got[:4].tolist() == [65504.0, -65504.0, 65504.0, -65504.0]
    assert math.isnan(float(got[4]))
    assert got[5:7].tolist() == [65504.0, -65504.0]
    assert torch.equal(got[7:], x[7:].to(F16))
    assert torch.equal(o.cast_f32_to_f16(x.to(DEV), mul=2.0 ** -4).cpu()[:2], torch.tensor([62500.0, -62500.0]).to(F16))


# ------------------------------------------------------------------ C. exact rescaling, bitwise
def _assert_scaled(name, base, scaled, factor, ref64, whole, log):
    """scaled == factor * base bit for bit; unless ``whole``, elements whose base result is an fp16 subnormal (|base| < 2^-14: it
    lost bits the scaled run keeps) are left out, and their share - by the kernel's result and by the fp64 reference alone - must
    stay below 0.1 %."""
    b, s = base.cpu(), scaled.cpu()
    want = (b.double() * factor).to(b.dtype)
    if whole:
        keep = torch.ones_like(b, dtype=torch.bool)
    else:
        keep = b.double().abs() >= 2.0 ** -14
        share, share_ref = 1 - float(keep.double().mean()), float((ref64.abs() < 2.0 ** -14).double().mean())
        log[name + "_left_out"] = {"kernel": share, "fp64_reference": share_ref}
        print(f"[parity] {name}: left out {share:.6f} (fp64 reference alone: {share_ref:.6f})")
        assert share < 1e-3 and share_ref < 1e-3
    assert torch.isfinite(s).all() and torch.isfinite(want).all()
    same = (s.view(torch.int16 if s.dtype == F16 else torch.int32) == want.view(torch.int16 if s.dtype == F16 else torch.int32)) | ((s == 0) & (want == 0))
    nbad = int((~same & keep).sum())
    log[name] = {"bitwise_mismatches": nbad}
    print(f"[parity] {name}: bitwise mismatches {nbad}/{b.numel()}")
    assert nbad == 0, f"{name}: {nbad} elements differ from the exactly rescaled result"


@functools.lru_cache(maxsize=None)
def banded_gemm_case(shape):
    M, N, K = shape
    A, W = banded((M, K), -3, 1, 551), banded((N, K), -4, 0, 552)
    bias, res = rnd(N, seed=553, dtype=F32), banded((M, N), -2, 2, 554)
    return dict(A=A, W=W, bias=bias, res=res, ref=A.double() @ W.double().t() + bias.double() + res.double())


def _pow2(t, e):
    out = (t.double() * 2.0 ** e).to(t.dtype)
    assert torch.equal(out.double(), t.double() * 2.0 ** e), "the rescale of an operand must be exact"
    return out


@pytest.mark.parametrize("a,b", [(4, -4), (3, 3)])
@pytest.mark.parametrize("tile,splitk,shape,relu", [(t, s, sh, False) for (t, s, sh) in GEMM_RUNS if s in (0, 2)] + [(0, 0, S1, True), (3, 0, S1, True)])
@pytest.mark.parametrize("variant", [0, 1])
def test_gemm_pow2_rescale_bitwise(variant, tile, splitk, shape, relu, a, b, results_log):
    """C(2^a A, 2^b W, 2^(a+b) bias, 2^(a+b) residual) == 2^(a+b) C(A, W, bias, residual) bit for bit: scaling by a power of two
    commutes with every rounding while nothing leaves the normal range."""
    o, l = ops(), lib()
    c = banded_gemm_case(shape)
    flags = l.GEMM_RELU if relu else 0
    with gemm_mode(variant, tile, splitk):
        base = o.gemm(*_dev(c["A"], c["W"]), bias=c["bias"].to(DEV), residual=c["res"].to(DEV), flags=flags)
        scaled = o.gemm(*_dev(_pow2(c["A"], a), _pow2(c["W"], b)), bias=_pow2(c["bias"], a + b).to(DEV),
                        residual=_pow2(c["res"], a + b).to(DEV), flags=flags)
    ref = F.relu(c["ref"]) if relu else c["ref"]
    if relu:        # an exact zero of the ReLU is no lost subnormal
        ref = ref[ref > 0]
    name = f"vr_pow2_gemm_{'x'.join(map(str, shape))}_v{variant}_t{tile}_sk{splitk}_relu{int(relu)}_a{a}b{b}"
    if relu and a + b:
        bb = base.cpu()
        nz = bb != 0
        _assert_scaled(name, bb[nz], scaled.cpu()[nz], 2.0 ** (a + b), ref, False, results_log)
        assert bool((scaled.cpu()[~nz] == 0).all())
    else:
        _assert_scaled(name, base, scaled, 2.0 ** (a + b), ref, a + b == 0, results_log)


@pytest.mark.parametrize("a,b", [(4, -4), (3, 3)])
@pytest.mark.parametrize("op,f32", [("halo", False), ("narrow", False), ("narrow", True), ("upconv", False)])
def test_conv_pow2_rescale_bitwise(op, f32, a, b, results_log):
    c = conv_case(op, "banded")
    bias = c["bias"]
    res = None if c["res"] is None else banded(tuple(c["res"].shape), -2, 2, 555)
    base = _run_conv(op, c["x"], c["w"], bias, res, f32=f32)
    scaled = _run_conv(op, _pow2(c["x"], a), _pow2(c["w"], b), _pow2(bias, a + b), None if res is None else _pow2(res, a + b), f32=f32)
    ref = c["base"] + bias.double() + (0 if res is None else res.double())
    _assert_scaled(f"vr_pow2_conv_{op}_f32{int(f32)}_a{a}b{b}", base, scaled, 2.0 ** (a + b), ref, a + b == 0 or f32, results_log)


def _attn(q, k, v, B, H, Sq, Skv, D, valid=None, causal=False):
    o = ops()
    C = H * D
    qd, kd, vd = q.reshape(B * Sq, C).to(DEV), k.reshape(B * Skv, C).to(DEV), v.reshape(B * Skv, C).to(DEV)
    if D == 64:
        return o.attention_d64(qd, kd, vd, B, H, Sq, Skv, valid, causal=causal).reshape(B, Sq, C)
    return o.attention_d512(qd, kd, vd, B, H, Sq, Skv, valid).reshape(B, Sq, C)


ATTN_FORMS = [(64, f) for f in (0, 1, 2, 17, 256, 513)] + [(512, 0)]
ATTN_FORMS_E = [(64, f) for f in (0, 1, 2, 17, 256, 513, 530)] + [(512, 0)]


def _attn_shape(D):
    return (1, 2, 256, 256) if D == 64 else (1, 1, 256, 256)


@pytest.mark.parametrize("D,force", ATTN_FORMS)
def test_attention_pow2_rescale_bitwise(D, force, results_log):
    """O(Q, K, 2^5 V) == 2^5 O(Q, K, V) and O(2^3 Q, 2^-3 K, V) == O(Q, K, V), bit for bit (banded operands: the pre-scaled Q of the
    streaming kernels, K / 8 and 32 V all stay normal fp16).  V is positive, so no output is an fp16 subnormal."""
    B, H, Sq, Skv = _attn_shape(D)
    C = H * D
    q, k = banded((B, Sq, C), -3, 1, 561), banded((B, Skv, C), -3, 1, 562)
    k = (k.float() * (8.0 / math.sqrt(D))).to(F16)             # keeps the scores O(1) at either head size (exact for D = 64)
    v = banded((B, Skv, C), -4, 2, 563, positive=True)
    with attn_force(force):
        base = _attn(q, k, v, B, H, Sq, Skv, D)
        v32 = _attn(q, k, _pow2(v, 5), B, H, Sq, Skv, D)
        qk = _attn(_pow2(q, 3), _pow2(k, -3), v, B, H, Sq, Skv, D)
    assert float(base.float().abs().min()) >= 2.0 ** -14
    _assert_scaled(f"vr_pow2_attn_d{D}_f{force}_v32", base, v32, 32.0, None, True, results_log)
    _assert_scaled(f"vr_pow2_attn_d{D}_f{force}_q8k8", base, qk, 1.0, None, True, results_log)


EPS32 = float(np.float32(1e-5))


def _gn(x, gamma, beta, eps, silu, fused):
    o, l = ops(), lib()
    l.api.lb_groupnorm_set_fused(fused)
    try:
        return o.groupnorm_nhwc(x.to(DEV), gamma.to(DEV), beta.to(DEV), 32, eps, silu)
    finally:
        l.api.lb_groupnorm_set_fused(1)


def _affine(C, seed):
    return rnd(C, seed=seed, dtype=F32) * 0.1 + 1, rnd(C, seed=seed + 1, dtype=F32) * 0.1


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("shape,f32_in,k", [((2, 1024, 320), False, -4), ((2, 1024, 320), False, 6), ((2, 250, 640), False, -4),
                                            ((2, 250, 640), False, 6), ((1, 4096, 512), True, -4), ((1, 4096, 512), True, 6),
                                            ((1, 4096, 512), True, 17)])
def test_groupnorm_pow2_rescale_bitwise(shape, f32_in, k, fused, results_log):
    """y(2^k x, eps 2^(2k)) == y(x, eps) bit for bit - DESIGN.md's "GroupNorm is scale-invariant once eps is scaled" - for the
    one-launch and the two-launch form; k = 17 (fp32 input only) reaches the 1.3e5 residual stream."""
    C = shape[-1]
    x = (torch.randn(*shape, generator=_gen(571)) + 0.5) if f32_in else banded(shape, -4, 2, 572)
    gamma, beta = _affine(C, 573)
    base = _gn(x, gamma, beta, EPS32, True, fused)
    scaled = _gn(_pow2(x, k), gamma, beta, EPS32 * 4.0 ** k, True, fused)
    _assert_scaled(f"vr_pow2_gn_{'x'.join(map(str, shape))}_fused{fused}_k{k}", base, scaled, 1.0, None, True, results_log)


def _conv_stats_gn(x, w, bias, alpha, eps, silu, gamma, beta, f32):
    """halo conv with LB_GEMM_CH_STATS -> (stored conv output, lb_groupnorm_from_stats of it)."""
    o, l = ops(), lib()
    B, H, Wd, cin = x.shape
    cout = w.shape[0]
    l.api.lb_gemm_set_halo(2)
    try:
        rows = o.conv_ch_stat_rows(B, H, Wd, cin, cout)
        assert rows > 0
        st = torch.full((cout, B * rows, 2), float("nan"), dtype=F32, device=DEV)
        y = o.gemm(x.to(DEV), o.pack_conv_weight(w, cin).to(DEV), bias=bias.to(DEV), flags=l.GEMM_OUT_F32 if f32 else 0, alpha=alpha,
                   conv=dict(KH=3, KW=3, stride=1, pad=1), ch_stats=st)
    finally:
        l.api.lb_gemm_set_halo(1)
    assert bool(torch.isfinite(st).all())
    return y, o.groupnorm_from_stats(y, gamma.to(DEV), beta.to(DEV), 32, eps, silu, st, rows)


@pytest.mark.parametrize("k", [-4, 6, 17])
def test_groupnorm_from_stats_pow2_rescale_bitwise(k, results_log):
    """The third GroupNorm form: statistics left by the producing conv.  The conv stores fp32 (no fp16 subnormals) and is rescaled
    exactly through alpha = 2^k with a 2^k bias; its stored output, its statistics and the normalised result must follow."""
    x, w = _conv_operands("normal", (2, 32, 32, 256), 128, 575)
    bias = rnd(128, seed=576, dtype=F32)
    gamma, beta = _affine(128, 577)
    y0, g0 = _conv_stats_gn(x, w, bias, 1.0, EPS32, True, gamma, beta, True)
    y1, g1 = _conv_stats_gn(x, w, _pow2(bias, k), 2.0 ** k, EPS32 * 4.0 ** k, True, gamma, beta, True)
    _assert_scaled(f"vr_pow2_gn_from_stats_conv_k{k}", y0, y1, 2.0 ** k, None, True, results_log)
    _assert_scaled(f"vr_pow2_gn_from_stats_k{k}", g0, g1, 1.0, None, True, results_log)


def _ln(x, gamma, beta, eps, form):
    o, l = ops(), lib()
    l.api.lb_layernorm_set_form(form)
    try:
        return o.layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), eps)
    finally:
        l.api.lb_layernorm_set_form(1)


@pytest.mark.parametrize("k", [-4, 6])
@pytest.mark.parametrize("form", [0, 1])
def test_layernorm_pow2_rescale_bitwise(form, k, results_log):
    """lb_layernorm_f16, both forms: rsqrtf of an argument scaled by 4^k (an even power of two: same significand, same exponent
    parity) returns the result scaled by 2^-k."""
    x = banded((131, 768), -4, 2, 581)
    gamma, beta = _affine(768, 582)
    base = _ln(x, gamma, beta, EPS32, form)
    scaled = _ln(_pow2(x, k), gamma, beta, EPS32 * 4.0 ** k, form)
    _assert_scaled(f"vr_pow2_ln_form{form}_k{k}", base, scaled, 1.0, None, True, results_log)


# ------------------------------------------------------------------ D. normalisations away from zero mean
def _gn_ref64(x, gamma, beta, eps, silu):
    """float64 GroupNorm(32) (+SiLU) of x [B, ..., C] (channels last)."""
    B, C = x.shape[0], x.shape[-1]
    y = F.group_norm(x.double().reshape(B, -1, C).permute(0, 2, 1), 32, gamma.double(), beta.double(), eps).permute(0, 2, 1).reshape(x.shape)
    return F.silu(y) if silu else y


def _gn_yardstick(x, gamma, beta, eps, silu):
    """The operation being replaced: F.group_norm in fp32 on the CPU."""
    B, C = x.shape[0], x.shape[-1]
    y = F.group_norm(x.float().reshape(B, -1, C).permute(0, 2, 1), 32, gamma, beta, eps).permute(0, 2, 1).reshape(x.shape)
    return F.silu(y) if silu else y


def _log_yardstick(log, name, yard, ref, bound):
    r = float(((yard.double() - ref).abs() / bound).max())
    log[name + "_yardstick_fp32_torch"] = {"worst_err_over_bound": r}
    print(f"[parity] {name}: fp32 torch yardstick worst err/bound={r:.3f}")


GN_F16 = [(0, 1.0), (8, 1.0), (64, 1.0), (64, 4.0)]
GN_F32 = [(0, 1.0), (8, 1.0), (64, 1.0), (512, 1.0), (64, 2.0 ** -6), (512, 2.0 ** -6)]
# Ratio 512 is measured, not required ("supported envelope"): the parameters that exceed the bound there are marked
# one by one with what was measured on an MI355X - worst err / bound of the kernel, then of fp32 torch (the yardstick).
_GN512 = {(1.0, False): "1.008 (fp32 torch: 0.090)", (1.0, True): "1.031 (fp32 torch: 0.054)", (2.0 ** -6, True): "1.040 (fp32 torch: 0.047)"}


def _gn_params():
    out = []
    for shape, f32_in, pairs in (((2, 1024, 320), False, GN_F16), ((2, 250, 640), False, GN_F16), ((1, 4096, 512), True, GN_F32)):
        for ratio, std in pairs:
            for fused in (0, 1):
                for silu in (False, True):
                    marks = ()
                    if ratio == 512 and (std, silu) in _GN512:
                        marks = pytest.mark.xfail(strict=True, reason="lb_groupnorm_nhwc (fp32 input: the two-launch kernels either way) at |mean| / std = 512, "
                                                  f"std = {std:g}, silu = {silu}: worst err / bound = {_GN512[(std, silu)]}; the fp32 sums of "
                                                  "x and x^2 cancel in E[x^2] - E[x]^2")
                    out.append(pytest.param(shape, f32_in, ratio, std, fused, silu, marks=marks))
    return out


@pytest.mark.parametrize("shape,f32_in,ratio,std,fused,silu", _gn_params())
def test_groupnorm_offset_mean(shape, f32_in, ratio, std, fused, silu, results_log):
    """lb_groupnorm_nhwc, both forms, fp16 and fp32 input, group means at +-ratio * std (sign alternating over the groups).  The
    statistics are accumulated as sum and sum of squares in fp32 and subtracted in float64: the cancellation grows with ratio^2."""
    C = shape[-1]
    x = offset(shape, ratio, std, 591, 32, -1, dtype=F32 if f32_in else F16)
    gamma, beta = _affine(C, 592)
    ref = _gn_ref64(x, gamma, beta, 1e-6, silu)
    bound = norm_bound(ref, gamma)
    name = f"vr_gn_{'x'.join(map(str, shape))}_r{ratio}_s{std:g}_fused{fused}_silu{int(silu)}"
    _log_yardstick(results_log, name, _gn_yardstick(x, gamma, beta, 1e-6, silu), ref, bound)
    check_elementwise(results_log, name, _gn(x, gamma, beta, 1e-6, silu, fused), ref, bound)


@pytest.mark.parametrize("f32,ratio", [(False, 0), (False, 8), (False, 64), (True, 0), (True, 8), (True, 64),
                                       pytest.param(True, 512, marks=pytest.mark.xfail(strict=True, reason=(
                                           "lb_groupnorm_from_stats on LB_GEMM_CH_STATS statistics (fp32 sums per 64-pixel row block) at "
                                           "|mean| / std = 512: worst err / bound = 2.773 without SiLU (fp32 torch: 0.096), 2.988 with (0.058)")))])
def test_groupnorm_from_stats_offset_mean(f32, ratio, results_log):
    """lb_groupnorm_from_stats fed by a real halo-conv launch with LB_GEMM_CH_STATS: the offset comes through a large conv bias
    (+-ratio per group; the conv output has std ~ 1), so the statistics are the kernel's own.  The fp64 reference normalises the
    STORED conv output."""
    cin = 256 if f32 else 128
    x, w = _conv_operands("normal", (2, 32, 32, cin), 128, 595)
    sign = 1.0 - 2.0 * ((torch.arange(128) // 4) % 2).float()
    bias = (rnd(128, seed=596, dtype=F32) * 0.1 + ratio * sign).float()
    gamma, beta = _affine(128, 597)
    failed = []
    for silu in (False, True):
        y, got = _conv_stats_gn(x, w, bias, 1.0, 1e-6, silu, gamma, beta, f32)
        ref = _gn_ref64(y.cpu(), gamma, beta, 1e-6, silu)
        bound = norm_bound(ref, gamma)
        name = f"vr_gn_from_stats_f32{int(f32)}_r{ratio}_silu{int(silu)}"
        _log_yardstick(results_log, name, _gn_yardstick(y.cpu(), gamma, beta, 1e-6, silu), ref, bound)
        try:                                    # (both forms are measured and logged before the test fails)
            check_elementwise(results_log, name, got, ref, bound)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("ratio,std", GN_F16)
def test_layernorm_offset_mean(ratio, std, form, results_log):
    """lb_layernorm_f16 (two-pass: mean, then centred squares), both forms, rows at +-ratio * std."""
    M, C = 131, 768
    x = offset((M, C), ratio, std, 601, M, 0, dtype=F16)
    gamma, beta = _affine(C, 602)
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    bound = norm_bound(ref, gamma)
    name = f"vr_ln_r{ratio}_s{std:g}_form{form}"
    _log_yardstick(results_log, name, F.layer_norm(x.float(), (C,), gamma, beta, 1e-5), ref, bound)
    check_elementwise(results_log, name, _ln(x, gamma, beta, 1e-5, form), ref, bound)


_LNA512 = {(0, False): "2.127 (fp32 torch: 0.027)", (1, False): "2.127 (fp32 torch: 0.027)", (3, False): "2.127 (fp32 torch: 0.027)",
           (11, False): "1.624 (fp32 torch: 0.027)", (0, True): "1.374 (fp32 torch: 0.019)", (1, True): "1.374 (fp32 torch: 0.019)",
           (3, True): "1.374 (fp32 torch: 0.019)"}      # (tile 11 with GEGLU holds the bound at 512: 0.977)


def _lna_params():
    out = []
    for ratio in (0, 8, 64, 512):
        for tile in (0, 1, 3, 11):
            for geglu in (False, True):
                marks = ()
                if ratio == 512 and (tile, geglu) in _LNA512:
                    marks = pytest.mark.xfail(strict=True, reason=f"LB_GEMM_LN_A (tile {tile}, geglu = {geglu}) at |mean| / std = 512: worst err / bound = "
                                              f"{_LNA512[(tile, geglu)]}; var = sq / K - mean^2 entirely in fp32 (gemm_glds.hip)")
                out.append(pytest.param(ratio, tile, geglu, marks=marks))
    return out


@pytest.mark.parametrize("ratio,tile,geglu", _lna_params())
def test_gemm_layernorm_fold_offset_mean(ratio, tile, geglu, results_log):
    """LB_GEMM_LN_A (row statistics as sum / sum of squares in fp32 inside the K loop) on the direct-to-LDS tiles via
    ops.fold_layernorm: rstd (x W'^T - mean colsum) + b'.  Reference: float64 on the folded operands the kernel reads (x, W' in
    fp16, colsum and b' in fp32); bound: the contraction bound on those operands - the accumulate term and the fp32 operations on
    x W'^T and mean * colsum, times rstd, then the bias add and the store."""
    o, l = ops(), lib()
    M, N, K = 300, 192, 128
    x = offset((M, K), ratio, 1.0, 611, M, 0, dtype=F16)
    w, b = rnd(N, K, seed=612, scale=K ** -0.5), rnd(N, seed=613, dtype=F32)
    gamma, beta = 1.0 + 0.2 * rnd(K, seed=614, dtype=F32), 0.1 * rnd(K, seed=615, dtype=F32)
    wf, colsum, b2 = o.fold_layernorm(w, b, gamma, beta)
    x64 = x.double()
    mean = x64.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x64.var(dim=1, unbiased=False, keepdim=True) + 1e-5)
    xw, mc = x64 @ wf.double().t(), mean * colsum.double()[None, :]
    ref = rstd * (xw - mc) + b2.double()
    pre = rstd * (accumulate_bound(absdot(x64, wf.double()), K) + 8 * U32 * (xw.abs() + mc.abs())) + 8 * U32 * (b2.double().abs() + ref.abs())
    if geglu:
        (h, gt), (ph, pg) = ref.chunk(2, dim=-1), pre.chunk(2, dim=-1)
        ref, bound = h * F.gelu(gt), geglu_bound(ph, pg, h, gt, F.gelu(gt))
    else:
        bound = pre * (1 + U16) + store_bound(ref)
    yard = F.layer_norm(x.float(), (K,), gamma, beta, 1e-5) @ w.float().t() + b
    if geglu:
        yh, yg = yard.chunk(2, dim=-1)
        yard = yh * F.gelu(yg)
    name = f"vr_gemm_ln_fold_r{ratio}_t{tile}_geglu{int(geglu)}"
    _log_yardstick(results_log, name, yard, ref, bound)
    with gemm_mode(1, tile):
        got = o.gemm(x.to(DEV), wf.to(DEV), bias=b2.to(DEV), flags=l.GEMM_GEGLU if geglu else 0, ln=(colsum.to(DEV), 1e-5))
    check_elementwise(results_log, name, got, ref, bound)


# ------------------------------------------------------------------ E. attention at hard score patterns
def _attn_ref64(q, k, v, H, D, valid=None, causal=False):
    """float64 softmax attention over the first ``valid`` keys -> (reference [B, Sq, H D], attention_bound of it)."""
    B, Sq = q.shape[:2]
    valid = valid or k.shape[1]
    qh, kh, vh = [t.double().reshape(B, -1, H, D).transpose(1, 2) for t in (q, k[:, :valid], v[:, :valid])]
    s = qh @ kh.transpose(-1, -2) * D ** -0.5
    if causal:
        s = s.masked_fill(torch.ones(Sq, valid, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(s, dim=-1)
    ref = p @ vh
    back = lambda t: t.transpose(1, 2).reshape(B, Sq, H * D)
    return back(ref), back(attention_bound(p, vh, ref))


def _check_attn(log, name, D, force, q, k, v, valid=None, causal=False, H=None):
    B, Sq, C = q.shape
    H = H or C // D
    ref, bound = _attn_ref64(q, k, v, H, D, valid, causal)
    with attn_force(force):
        got = _attn(q, k, v, B, H, Sq, k.shape[1], D, valid, causal)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    check_elementwise(log, name, got, ref, bound)


@functools.lru_cache(maxsize=None)
def ramp_case(D, step, descending):
    """Queries share a direction u (per head); the keys of 64-key tile t are u times t * step (in log2 units of the score) plus
    0.05 N(0, 1): the row maximum rises (or falls) by ``step`` per tile.  Key values computed in float64, rounded to fp16."""
    B, H, Sq, Skv = _attn_shape(D)
    g = _gen(621)
    u = torch.randn(H, D, generator=g, dtype=F64)
    u = u / u.norm(dim=-1, keepdim=True)
    amp_q = 4.0
    amp_k = 1.0 / (amp_q * D ** -0.5 * 1.4426950408889634)       # q . k * scale * log2(e) = t * step
    t = torch.arange(Skv) // 64
    if descending:
        t = (Skv - 1) // 64 - t
    q = (amp_q * u)[None, None].expand(B, Sq, H, D)
    k = (t.double() * step * amp_k)[None, :, None, None] * u[None, None] + 0.05 * torch.randn(B, Skv, H, D, generator=g, dtype=F64)
    v = torch.randn(B, Skv, H * D, generator=g)
    return q.reshape(B, Sq, H * D).to(F16), k.reshape(B, Skv, H * D).to(F16), v.to(F16)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("step", [7.9, 8.1, 4.0])
@pytest.mark.parametrize("D,force", ATTN_FORMS_E)
def test_attention_ramp(D, force, step, descending, results_log):
    """The deferred rescale from either side of its threshold (2^8): a maximum that rises by 7.9 log2 units per tile never moves
    the running maximum (P reaches 2^7.9 in fp16), 8.1 moves it every tile, 4.0 every second tile."""
    q, k, v = ramp_case(D, step, descending)
    _check_attn(results_log, f"vr_attn_ramp_d{D}_f{force}_step{step}_{'down' if descending else 'up'}", D, force, q, k, v)


@functools.lru_cache(maxsize=None)
def hot_case(D, v_at_range):
    B, H, Sq, Skv = _attn_shape(D)
    C = H * D
    q, k = (rnd(B, Sq, C, seed=631).float() * 8).to(F16), (rnd(B, Skv, C, seed=632).float() * 8).to(F16)
    v = banded((B, Skv, C), 10, 15, 633) if v_at_range else rnd(B, Skv, C, seed=634)
    return q, k, v


@pytest.mark.parametrize("v_at_range", [False, True])
@pytest.mark.parametrize("D,force", ATTN_FORMS_E)
def test_attention_hot_scores(D, force, v_at_range, results_log):
    """Q and K multiplied by 8: scores of several hundred in natural units, rows almost one-hot, ties broken by 1e-3 matter.
    With V banded up to 2^15 the outputs near 3e4 must be finite and within the bound.

    This test found a precision loss: until it existed attn_fwd_d64_stream_kernel and attn_fwd_d64_pp_kernel multiplied Q by
    scale * log2(e) once and rounded the product to fp16, which moves a score by up to 2^-11 sum_d |q_d k_d| scale * log2(e) -
    0.01 .. 0.04 log2 units here, several per cent on the probabilities of keys that tie: worst err / bound 29.1 (26.1 with V at
    range) on forces 0, 1, 2, 17, 513 and 530.  They now multiply Q by the power-of-two part of that factor (exact) and the fp32
    accumulators by the rest: 0.45 / 0.41, the figures of the rounds-1-5 kernel (force 256)."""
    q, k, v = hot_case(D, v_at_range)
    _check_attn(results_log, f"vr_attn_hot_d{D}_f{force}_vrange{int(v_at_range)}", D, force, q, k, v)


@functools.lru_cache(maxsize=None)
def masked_case(D, Sq, Skv, valid, H):
    q, k, v = rnd(1, Sq, H * D, seed=641), rnd(1, Skv, H * D, seed=642), rnd(1, Skv, H * D, seed=643)
    k[0, valid:] = (8.0 * q[0, 0].float()).to(F16)        # rows behind Skv_valid: large, finite, and they must be MASKED
    v[0, valid:] = 1000.0
    return q, k, v


@pytest.mark.parametrize("valid", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("D,force", ATTN_FORMS_E)
def test_attention_masked_tiles(D, force, valid, results_log):
    """Skv = 256 with Skv_valid from 1 to 130: whole key tiles of the streaming forms are masked."""
    B, H, Sq, Skv = _attn_shape(D)
    q, k, v = masked_case(D, Sq, Skv, valid, H)
    _check_attn(results_log, f"vr_attn_masked_d{D}_f{force}_valid{valid}", D, force, q, k, v, valid=valid)


@pytest.mark.parametrize("force", [0, 1, 2, 17, 256, 513, 530])
def test_attention_causal_and_one_tile(force, results_log):
    """The causal variant at S = 200 (rows whose later tiles are masked entirely), and the one-tile form at Skv = 96, valid = 5."""
    q, k, v = rnd(1, 200, 128, seed=651), rnd(1, 200, 128, seed=652), rnd(1, 200, 128, seed=653)
    _check_attn(results_log, f"vr_attn_causal_f{force}", 64, force, q, k, v, causal=True)
    if not force & 16:
        q, k, v = masked_case(64, 256, 96, 5, 2)
        _check_attn(results_log, f"vr_attn_one_tile_f{force}", 64, force, q, k, v, valid=5)


def test_softmax_rows_edges(results_log):
    """lb_softmax_rows_f16 at N = 304: a row of equal values, a row with one value 60000 above the rest at scale = 1, a row of
    -65504.  Bound: the fp16 store plus (N + 32) * 2^-24 |ref| for the fp32 part (the row sum of N terms, v_exp_f32, the
    rounding of an exponent of magnitude <= 25 - below that the result is under half an fp16 subnormal step - and the reciprocal)."""
    o = ops()
    N = 304
    x = torch.zeros(4, N, dtype=F16)
    x[0] = 3.25
    x[1] = -5000.0
    x[1, 77] = 55000.0
    x[2] = -65504.0
    x[3] = rnd(N, seed=661, scale=4.0)
    ref = torch.softmax(x.double(), dim=-1)
    got = o.softmax_rows_(x.to(DEV).clone(), 1.0)
    check_elementwise(results_log, "vr_softmax_rows_edges", got, ref, store_bound(ref) + (N + 32) * U32 * ref)


# ------------------------------------------------------------------ F. element-wise kernels at their edges: exact
@pytest.mark.parametrize("dtype", [F32, F16])
def test_postprocess_u8_rounding_edges(dtype):
    """lb_postprocess_u8 against the oracle's postprocess_u8 on inputs whose (x / 2 + 0.5) * 255 lands on (the nearest value to)
    every k + 0.5 (round half to even), one step either side of it, below -1, above 1 and at +-inf: byte for byte."""
    o = ops()
    kk = torch.arange(255, dtype=F64)
    mid = ((2 * kk + 1) / 255 - 1).to(dtype)
    info_max = torch.finfo(dtype).max
    if dtype == F32:        # "just either side": 2^-18 (32 fp32 steps at 1.0) moves (x / 2 + 0.5) * 255 by 5e-4
        lo, hi = mid - 2.0 ** -18, mid + 2.0 ** -18
    else:                   # the neighbouring fp16 values
        lo = torch.from_numpy(np.nextafter(mid.numpy(), np.float16(-2))).to(dtype)
        hi = torch.from_numpy(np.nextafter(mid.numpy(), np.float16(2))).to(dtype)
    extra = torch.tensor([-1.0, 1.0, 0.0, -1.5, 1.5, -info_max, info_max, float("-inf"), float("inf"), -1.0000001, 1.0000001, 0.5], dtype=dtype)
    vals = torch.cat([mid, lo, hi, extra])
    vals = torch.cat([vals, torch.zeros((-vals.numel()) % 3, dtype=dtype)])
    P = vals.numel() // 3
    x4 = torch.zeros(1, 1, P, 4, dtype=dtype)
    x4[0, 0, :, :3] = vals.reshape(P, 3)
    got = o.postprocess_u8(x4.to(DEV)).cpu().numpy()
    want = R.postprocess_u8(x4[..., :3].permute(0, 3, 1, 2))
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert len(np.unique(want)) == 256


def test_lpips_prep_u8_all_byte_values():
    """lb_lpips_prep_u8 on all 256 byte values in every channel: exactly the fp16 rounding of the same fp32 expression
    ((2 x / 255 - 1) - shift) / scale, and within half an fp16 ulp of its float64 value; channels 3..7 zero."""
    o = ops()
    img = torch.arange(256, dtype=torch.uint8)[:, None].expand(256, 3).contiguous()
    got = o.lpips_prep_u8(img.to(DEV)).cpu()
    shift, scale = torch.tensor([-.030, -.088, -.188]), torch.tensor([.458, .448, .450])
    want = (((2.0 * img.float() / 255.0 - 1.0) - shift) / scale).to(F16)
    assert torch.equal(got[:, :3], want) and bool((got[:, 3:] == 0).all())
    ref = ((2.0 * img.double() / 255.0 - 1.0) - shift.double()) / scale.double()
    assert bool(((got[:, :3].double() - ref).abs() <= store_bound(ref) * (1 + 2.0 ** -10)).all())


@pytest.mark.parametrize("exp", [-8, 6])
def test_slerp_scaled_latents(exp, results_log):
    """lb_slerp_*_f16 / _f32 on latents multiplied by 2^-8 and by 2^6 - there the squared norm (16384 * (3 * 64)^2 = 6e8) overflows
    fp16 and must not overflow the kernel - at fracts 0, 1 and 1e-4, against the oracle's float64 slerp with test_slerp_edge_cases'
    tolerance rule: <= 1 fp16 ulp (exact at 0 and 1), fp32 within rtol = atol = 1e-6."""
    o = ops()
    n = 16384
    p0, p1 = [(rnd(1, 4, n // 4, seed=sd, scale=3.0).float() * 2.0 ** exp).to(F16) for sd in (671, 672)]
    frd = torch.tensor([0.0, 1.0, 1e-4], dtype=F64, device=DEV)
    strided = o.slerp_strided(p0.reshape(-1).to(DEV), p1.reshape(-1).to(DEV), frd, n, broadcast0=True, broadcast1=True).cpu()
    for i, f in enumerate((0.0, 1.0, 1e-4)):
        got = o.slerp(p0.to(DEV), p1.to(DEV), f).cpu()
        ref = R.slerp(p0, p1, f)
        assert torch.isfinite(got).all() and ulp_diff_f16(got, ref) <= 1 and ulp_diff_f16(strided[i].reshape(p0.shape), ref) <= 1
        if f in (0.0, 1.0):
            assert torch.equal(got, p0 if f == 0.0 else p1) and torch.equal(strided[i].reshape(p0.shape), got)
        a32, b32 = p0.float() * 1.0009765625, p1.float() * 0.99951171875           # fp32 values that are no fp16 values
        got32 = o.slerp(a32.to(DEV), b32.to(DEV), f).cpu()
        assert got32.dtype == F32 and torch.allclose(got32, R.slerp(a32, b32, f), rtol=1e-6, atol=1e-6)
    results_log[f"vr_slerp_scaled_2^{exp}"] = {"max_ulp": 1}


@pytest.mark.parametrize("ancestral", [False, True])
def test_euler_first_and_last_step(ancestral, results_log):
    """lb_euler_step_f16 at the first step (sigma 14.6 on the 4-step ancestral schedule, 11.5 on the 30-step one; x = 14.6 N(0, 1)) and
    the last (sigma_next = 0) against the oracle
    scheduler, at the exactness of test_euler_step_matches_oracle (<= 1 fp16 ulp)."""
    o = ops()
    sched = R.EulerScheduler(ancestral=ancestral)
    sched.set_timesteps(4 if ancestral else 30)
    last = len(sched.timesteps) - 1
    assert float(sched.sigmas[0]) > 11.0 and float(sched.sigmas[last + 1]) == 0.0
    eps, noise = rnd(2, 4, 64, 64, seed=682), rnd(2, 4, 64, 64, seed=683)
    sched.noise_source = lambda shape: noise[:1]
    worst = 0
    for i in (0, last):
        s_from, s_to = float(sched.sigmas[i]), float(sched.sigmas[i + 1])
        x = (rnd(2, 4, 64, 64, seed=681).float() * (14.6 if i == 0 else s_from)).to(F16)
        t = sched.timesteps[i]
        sched._step_index = None
        scaled_ref = sched.scale_model_input(x[:1], t)
        sched._step_index = None
        ref = sched.step(eps[:1], t, x[:1])[0]
        if ancestral:
            s_up, s_down = R.ancestral_sigmas(s_from, s_to)
            row = (s_from, s_down, s_up, 0.0, s_down - s_from)
        else:
            row = (s_from, s_to, 0.0, 0.0, s_to - s_from)
        params = o.step_params([row, row], DEV)
        assert ulp_diff_f16(o.scale_model_input(x.to(DEV), params)[:1], scaled_ref) <= 1
        got = o.euler_step(x.to(DEV), eps.to(DEV), params, noise=noise[:1].expand(2, -1, -1, -1).contiguous().to(DEV), ancestral=ancestral)
        assert torch.isfinite(got).all()
        worst = max(worst, ulp_diff_f16(got[:1], ref))
    results_log[f"vr_euler_first_last_anc{int(ancestral)}_max_ulp"] = worst
    print(f"[parity] vr_euler_first_last_anc{int(ancestral)}: max ulp {worst}")
    assert worst <= 1


@pytest.mark.parametrize("cfg", [False, True])
def test_ddim_first_and_last_step(cfg, results_log):
    """lb_ddim_step_f16 at the first step (alpha_t = 0.0047: x0 = (x - sqrt(1 - a) eps) / sqrt(a) amplifies by 14.6) and the
    last (prev_timestep < 0), on x of the first step's own size (N(0, 1)) and 4 x that, against the oracle: <= 1 fp16 ulp."""
    from latentblending_amd.native.scheduler import NativeDDIMScheduler
    o = ops()
    sched, ref = NativeDDIMScheduler(device=DEV), R.DDIMScheduler()
    sched.set_timesteps(30); ref.set_timesteps(30)
    B, g = 2, 4.0
    worst = 0
    for scale in (1.0, 4.0):
        x = rnd(B, 4, 64, 64, seed=691, scale=scale)
        eps = rnd(2 * B if cfg else B, 4, 64, 64, seed=692)
        e = eps[:B] + g * (eps[B:] - eps[:B]) if cfg else eps
        for i in (0, 29):
            want = ref.step(e, int(ref.timesteps[i]), x)[0]
            params = o.step_params([sched.step_row(i, g)] * B, DEV)
            got = o.ddim_step(x.to(DEV), eps.to(DEV), params, cfg=cfg)
            assert torch.isfinite(got).all()
            worst = max(worst, ulp_diff_f16(got, want))
    results_log[f"vr_ddim_first_last_cfg{int(cfg)}_max_ulp"] = worst
    print(f"[parity] vr_ddim_first_last_cfg{int(cfg)}: max ulp {worst}")
    assert worst <= 1
