"""The memory contract of every launcher, on a real MI355X: WHERE a kernel reads and writes, not only what it computes.

Every output lives in a ``_guard.guarded`` buffer (sentinel-filled guards in front of and behind the payload, pad columns between
the rows: ldc > N, ldo > C, ...), every operand carries poisoned padding (NaN in the pad columns K..lda, N..ldr, N..ld_rowvec,
Cin..ldx and in whole rows behind the last one: memory a kernel has no right to read; adversarial FINITE values in the attention
K / V rows [Skv_valid, Skv), which exist in the models).  Each case asserts three things: the values against an fp64 CPU reference
of the same op on the fp16-rounded inputs (the tolerances of test_kernels_gpu.py: ``check_close`` with the per-op floors used
there, bit-exactness / 1 ulp where the existing test of that op has it), ``assert_intact`` (no store outside the result) and
``assert_fully_written`` (no element of the result left out).  Where a launcher does not take a layout the test asserts that it
REFUSES it (RuntimeError) and that the guarded output is untouched.

Launchers named here (every extern "C" entry point of misc / mix / norm / attn / attn512 / gemm / conv files that writes device
data): lb_gemm_f16 (both variants, every tile, every epilogue store path, implicit-GEMM and four-launch sub-pixel convs),
lb_conv3x3_halo_f16, lb_conv3x3_narrow_f16, lb_upconv2x_halo_f16, lb_attn_fwd_d64, lb_attn_fwd_d512, lb_softmax_rows_f16,
lb_layernorm_f16, lb_groupnorm_nhwc, lb_groupnorm_from_stats, lb_slerp_pairs_f16 / _f32 / _f64, lb_slerp_batched_f16,
lb_slerp_strided_f16, lb_lerp_f16 / _f32, lb_scale_model_input_f16, lb_euler_step_f16, lb_ddim_step_f16, lb_sinusoid_f16,
lb_copy_cols_f16, lb_cast_f16_to_f32, lb_cast_f32_to_f16, lb_fill_f32, lb_nchw_to_nhwc_f16, lb_nhwc_to_nchw_f16,
lb_postprocess_u8, lb_lpips_prep_u8, lb_maxpool3s2_nhwc_f16, lb_lpips_tap, lb_embed_tokens_f16, lb_gather_rows_f16,
lb_frames_lerp_u8.  The other two sampler steps have their guard-band tests beside their restatements: lb_lcm_step_f16 in
tests/test_lcm_gpu.py::test_lcm_step_memory_contract (NaN noise behind the last-step rows), lb_dpmpp2m_step_f16 in
tests/test_dpmpp_gpu.py::test_dpmpp_step_kernel_matches_the_restatement_bit_for_bit (two-plane ``out`` between guard bands, NaN
history behind the first-order rows).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import sdxl_ref as R  # noqa: E402  (checker only)
from _guard import guarded, poisoned  # noqa: E402
from _parity import check_close, rnd, ulp_diff_f16  # noqa: E402

DEV = "cuda"
NAN = float("nan")
F16, F32, F64 = torch.float16, torch.float32, torch.float64


def ops():
    from latentblending_amd.hip import ops as o
    return o


def lib():
    from latentblending_amd.hip import lib as l
    return l


def stream():
    return torch.cuda.current_stream().cuda_stream


def done(chk, name):
    """The two memory assertions of every case (after the value check)."""
    chk.assert_intact(name)
    chk.assert_fully_written(name)


def refused(fn, chk, name):
    """A layout the launcher does not take: the call raises and nothing was stored."""
    with pytest.raises(RuntimeError):
        fn()
    torch.cuda.synchronize()
    chk.assert_untouched(name)


# ====================================================================== GEMM ==================
GEMM_SHAPES = [(65, 132, 72),        # one row over a 64-row tile, N % 8 == 4, a K tail
               (300, 260, 128),
               (2, 64, 64)]
# (variant, tile, stages): register ring with its three tiles; direct-to-LDS with every tile and the ring depths of
# test_gemm_glds_variant (the 192x128 tiles and the two-K-group 64x64 tile have one depth); the ping-pong tile where eligible
GEMM_CONFIGS = ([(0, t, 0) for t in (1, 2, 3)] + [(1, t, s) for t in (1, 2, 3, 4, 5) for s in (2, 3, 4)] +
                [(1, t, 3) for t in (7, 10, 11)] + [(-1, 9, 0)])


def _rpb(M):
    return {300: 100, 65: 33, 2: 1}[M]       # M = 300: a 64-row tile straddles two samples


@functools.lru_cache(maxsize=None)
def _gemm_operands(M, N, K):
    """CPU operands (fp16-rounded), their poisoned device views and the fp64 product."""
    A, W = rnd(M, K, seed=21), rnd(N, K, seed=22, scale=K ** -0.5)
    bias = rnd(N, seed=23, dtype=F32)
    res, res32 = rnd(M, N, seed=24), rnd(M, N, seed=35, dtype=F32, scale=100.0)
    nb = (M + _rpb(M) - 1) // _rpb(M)
    rv = rnd(nb, N, seed=36)
    d = dict(A=A, W=W, bias=bias, res=res, res32=res32, rv=rv, base=A.double() @ W.double().t())
    d["A_d"] = poisoned(A, M, K, K + 8, NAN, DEV)
    d["W_d"] = poisoned(W, N, K, K, NAN, DEV)
    d["bias_d"] = poisoned(bias[None], 1, N, N + 16, NAN, DEV, extra_rows=1)[0]
    d["res_d"] = poisoned(res, M, N, N + 12, NAN, DEV)
    d["res32_d"] = poisoned(res32, M, N, N + 12, NAN, DEV)
    d["rv_d"] = poisoned(rv, nb, N, N + 8, NAN, DEV)
    return d


@functools.lru_cache(maxsize=None)
def _geglu_operands(M, K):
    N = 264
    A, W = rnd(M, K, seed=29), rnd(N, K, seed=30, scale=K ** -0.5)
    bias = rnd(N, seed=31, dtype=F32, scale=0.1)
    h, gate = (A.double() @ W.double().t() + bias.double()).chunk(2, dim=-1)
    return dict(ref=h * F.gelu(gate), A_d=poisoned(A, M, K, K + 8, NAN, DEV), W_d=poisoned(W, N, K, K, NAN, DEV),
                bias_d=poisoned(bias[None], 1, N, N + 16, NAN, DEV, extra_rows=1)[0])


@functools.lru_cache(maxsize=None)
def _ln_operands(M, N, K):
    o = ops()
    x = rnd(M, K, seed=81) * 1.5 + rnd(M, 1, seed=82) * 4.0
    w, b = rnd(N, K, seed=83, scale=K ** -0.5), rnd(N, seed=84, dtype=F32)
    gamma, beta = 1.0 + 0.2 * rnd(K, seed=85, dtype=F32), 0.1 * rnd(K, seed=86, dtype=F32)
    ref = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5) @ w.double().t() + b.double()
    wf, colsum, b2 = o.fold_layernorm(w, b, gamma, beta)
    return dict(ref=ref, A_d=poisoned(x, M, K, K + 8, NAN, DEV), W_d=poisoned(wf, N, K, K, NAN, DEV),
                colsum_d=poisoned(colsum[None], 1, N, N + 16, NAN, DEV, extra_rows=1)[0],
                bias_d=poisoned(b2[None], 1, N, N + 16, NAN, DEV, extra_rows=1)[0])


@pytest.mark.parametrize("cfg", GEMM_CONFIGS, ids=lambda c: f"v{c[0]}t{c[1]}s{c[2]}")
def test_gemm_memory_contract(cfg, results_log):
    """lb_gemm_f16: lda = K + 8 (NaN pad), NaN rows behind A / W / residual / row vector, ldc = N + 12 (a multiple of 8: the
    16-byte stores stay eligible) and N + 4 (the 8-byte path), every epilogue family, forced split-K, the LayerNorm fold (NaN pad
    columns must not enter the row statistics), and the lean-epilogue / wide-store switches."""
    o, l = ops(), lib()
    variant, tile, stages = cfg
    tag = f"v{variant}t{tile}s{stages}"

    def run(name, M, n_out, ldc, ref, call, dtype=F16, trans=False, **tol):
        if trans:
            out, chk = guarded(n_out, M, ldc, dtype, DEV)
        else:
            out, chk = guarded(M, n_out, ldc, dtype, DEV)
        call(out)
        check_close(results_log, f"bounds_gemm_{name}_{tag}", out, ref, **tol)
        done(chk, f"gemm {name} {tag}")

    l.api.lb_gemm_set_variant(variant, stages)
    l.api.lb_gemm_set_tuning(tile, 0)
    try:
        for (M, N, K) in GEMM_SHAPES:
            d = _gemm_operands(M, N, K)
            A, W, bias, base = d["A_d"], d["W_d"], d["bias_d"], d["base"]
            full = base + d["bias"].double() + d["res"].double() + d["rv"].double().repeat_interleave(_rpb(M), 0)[:M]
            sh = f"{M}x{N}x{K}"
            # (N + 12 and N + 4 are multiples of 8 when N % 8 == 4 and are not when N % 8 == 0; N + 8 is the other way round: both
            #  shapes see the 16-byte and the 8-byte store path)
            for ldc in (N + 12, N + 4, N + 8):
                run(f"plain_{sh}_ldc{ldc}", M, N, ldc, base, lambda out: o.gemm(A, W, out=out))
                run(f"bias_res_rowvec_{sh}_ldc{ldc}", M, N, ldc, full,
                    lambda out: o.gemm(A, W, bias=bias, residual=d["res_d"], rowvec=d["rv_d"], rows_per_batch=_rpb(M), out=out))
                run(f"silu_{sh}_ldc{ldc}", M, N, ldc, F.silu(base + d["bias"].double()),
                    lambda out: o.gemm(A, W, bias=bias, flags=l.GEMM_SILU, out=out))
                run(f"f32_{sh}_ldc{ldc}", M, N, ldc, 0.5 * base + d["bias"].double() + d["res32"].double(),
                    lambda out: o.gemm(A, W, bias=bias, residual=d["res32_d"], alpha=0.5, flags=l.GEMM_OUT_F32 | l.GEMM_RES_F32, out=out),
                    dtype=F32, rel=1e-4, frac=2 ** -12)
                g = _geglu_operands(M, K)
                run(f"geglu_{M}x264x{K}_ldc{ldc - N + 132}", M, 132, ldc - N + 132, g["ref"],
                    lambda out: o.gemm(g["A_d"], g["W_d"], bias=g["bias_d"], flags=l.GEMM_GEGLU, out=out))
                ln = _ln_operands(M, N, K)
                ln_call = lambda out: o.gemm(ln["A_d"], ln["W_d"], bias=ln["bias_d"], ln=(ln["colsum_d"], 1e-5), out=out)  # noqa: E731
                if variant == 0:           # the register-ring variant has no LayerNorm fold: refused before anything is stored
                    out, chk = guarded(M, N, ldc, F16, DEV)
                    refused(lambda: ln_call(out), chk, f"gemm ln {sh} {tag}")
                else:
                    run(f"ln_{sh}_ldc{ldc}", M, N, ldc, ln["ref"], ln_call, rel=3e-3, frac=2 ** -7)
            run(f"trans_{sh}", M, N, M + 3, base.t(), lambda out: o.gemm(A, W, flags=l.GEMM_TRANS_OUT, out=out), trans=True)
            # lean epilogue / wide stores toggled (defaults: both on)
            for lean, wide in ((0, 1), (1, 0), (0, 0)):
                l.api.lb_gemm_set_lean_epilogue(lean)
                l.api.lb_gemm_set_wide_store(wide)
                try:
                    run(f"bias_res_{sh}_lean{lean}wide{wide}", M, N, N + 12, base + d["bias"].double() + d["res"].double(),
                        lambda out: o.gemm(A, W, bias=bias, residual=d["res_d"], out=out))
                    run(f"rowvec_{sh}_lean{lean}wide{wide}", M, N, N + 12,
                        base + d["rv"].double().repeat_interleave(_rpb(M), 0)[:M],
                        lambda out: o.gemm(A, W, rowvec=d["rv_d"], rows_per_batch=_rpb(M), out=out))
                finally:
                    l.api.lb_gemm_set_lean_epilogue(1)
                    l.api.lb_gemm_set_wide_store(1)
        # forced split-K at K = 512 (the reduce kernel stores the output)
        for splitk in (2, 5):
            l.api.lb_gemm_set_tuning(tile, splitk)
            for (M, N, _) in GEMM_SHAPES:
                d = _gemm_operands(M, N, 512)
                for ldc in (N + 12, N + 4):
                    run(f"splitk{splitk}_{M}x{N}x512_ldc{ldc}", M, N, ldc, d["base"] + d["bias"].double() + d["res"].double(),
                        lambda out: o.gemm(d["A_d"], d["W_d"], bias=d["bias_d"], residual=d["res_d"], out=out))
        l.api.lb_gemm_set_tuning(tile, 0)
    finally:
        l.api.lb_gemm_set_variant(-1, 0)
        l.api.lb_gemm_set_tuning(0, 0)
        l.api.lb_gemm_set_lean_epilogue(1)
        l.api.lb_gemm_set_wide_store(1)


# ====================================================================== convolutions ==========
CONV_ROWS = [(1, 10, 14, 72, 96, 3, 1, 1, 0),        # non-square, Cin not a multiple of 64
             (2, 16, 16, 64, 64, 3, 2, 1, 0),        # stride 2
             (1, 8, 8, 128, 128, 3, 1, 1, 1),        # fused nearest-2x upsample
             (2, 16, 16, 4, 64, 3, 1, 1, 0)]         # Cin 4 padded to 8


def _nhwc_poisoned(x_nchw, cpad, ldx):
    """NCHW fp16 -> poisoned NHWC device view [B, H, W, cpad] with pixel stride ldx (channels C..cpad zero, cpad..ldx NaN)."""
    B, Cc, H, Wd = x_nchw.shape
    t = torch.zeros(B * H * Wd, cpad, dtype=F16)
    t[:, :Cc] = x_nchw.permute(0, 2, 3, 1).reshape(-1, Cc)
    return poisoned(t, B * H * Wd, cpad, ldx, NAN, DEV).unflatten(0, (B, H, Wd))


@functools.lru_cache(maxsize=None)
def _conv_operands(case):
    o = ops()
    B, H, Wd, Cin, Cout, k, st, pad, ups = case
    x = rnd(B, Cin, H, Wd, seed=37)
    w = rnd(Cout, Cin, k, k, seed=38, scale=(Cin * k * k) ** -0.5)
    bias = rnd(Cout, seed=39, dtype=F32)
    xin = F.interpolate(x.double(), scale_factor=2.0, mode="nearest") if ups else x.double()
    ref = F.conv2d(xin, w.double(), bias.double(), stride=st, padding=pad).permute(0, 2, 3, 1)
    cin_p, cout_p = (Cin + 7) // 8 * 8, (Cout + 3) // 4 * 4
    wp = torch.zeros(cout_p, k * k * cin_p, dtype=F16)
    wp[:Cout] = o.pack_conv_weight(w, cin_p)
    bp = torch.zeros(cout_p, dtype=F32)
    bp[:Cout] = bias
    return dict(ref=ref, x_d=_nhwc_poisoned(x, cin_p, cin_p + 8), w_d=poisoned(wp, cout_p, wp.shape[1], wp.shape[1], NAN, DEV),
                b_d=bp.to(DEV), cout_p=cout_p, x=x, w=w, bias=bias)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("tile", [1, 3])
@pytest.mark.parametrize("case", CONV_ROWS, ids=lambda c: "_".join(map(str, c)))
def test_conv_implicit_gemm_memory_contract(case, tile, variant, results_log):
    """lb_gemm_f16 as an implicit-GEMM conv with ldx = Cin_pad + 8 (NaN behind every pixel's channels and behind the image)
    and ldc = Cout_pad + 8; the upsampling case also as four sub-pixel launches scattered into one guarded [B, 2H, 2W, C]."""
    o, l = ops(), lib()
    B, H, Wd, Cin, Cout, k, st, pad, ups = case
    d = _conv_operands(case)
    ho, wo = d["ref"].shape[1:3]
    name = f"bounds_conv_{'_'.join(map(str, case))}_v{variant}t{tile}"
    l.api.lb_gemm_set_variant(variant, 0)
    l.api.lb_gemm_set_tuning(tile, 0)
    try:
        out, chk = guarded(B * ho * wo, d["cout_p"], d["cout_p"] + 8, F16, DEV)
        o.gemm(d["x_d"], d["w_d"], bias=d["b_d"], out=out.unflatten(0, (B, ho, wo)), conv=dict(KH=k, KW=k, stride=st, pad=pad, ups=ups))
        check_close(results_log, name, out[:, :Cout].reshape(B, ho, wo, Cout), d["ref"])
        done(chk, name)
        if ups:
            out, chk = guarded(B * ho * wo, Cout, Cout + 8, F16, DEV)
            for (py, px), kk in o.subpixel_upsample_weights(d["w"]).items():
                o.gemm(d["x_d"], kk.to(DEV), bias=d["b_d"], out=out.unflatten(0, (B, ho, wo)),
                       conv=dict(KH=2, KW=2, stride=1, pad=0, parity=(py, px)))
            check_close(results_log, name + "_subpixel4", out.reshape(B, ho, wo, Cout), d["ref"], rel=3e-3)
            done(chk, name + "_subpixel4")
    finally:
        l.api.lb_gemm_set_variant(-1, 0)
        l.api.lb_gemm_set_tuning(0, 0)


@pytest.mark.parametrize("ldc_pad,ldx_pad", [(8, 8), (4, 0), (0, 8)])
@pytest.mark.parametrize("case", [(3, 16, 16, 192, 132), (1, 8, 96, 64, 64), (2, 48, 16, 128, 256)], ids=lambda c: "_".join(map(str, c)))
def test_conv3x3_halo_memory_contract(case, ldc_pad, ldx_pad, results_log):
    """lb_conv3x3_halo_f16 (TW = 32 and 16 tilings, ragged N = 132) with bias + residual, pixel stride ldx > Cin, ldc > N
    (a multiple of 8: 16-byte stores / lean epilogue; N + 4: the general form), ldr > N; and through the lb_gemm_f16 router with
    LB_GEMM_CH_STATS into a guarded statistics buffer."""
    o, l = ops(), lib()
    B, H, Wd, Cin, Cout = case
    x, w = rnd(B, Cin, H, Wd, seed=90), rnd(Cout, Cin, 3, 3, seed=91, scale=(Cin * 9) ** -0.5)
    b, res = rnd(Cout, seed=92, dtype=F32), rnd(B * H * Wd, Cout, seed=93)
    ref = (F.conv2d(x.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, Cout) + res.double())
    x_d = _nhwc_poisoned(x, Cin, Cin + ldx_pad)
    wp = o.pack_conv_weight(w, Cin)
    w_d, b_d = poisoned(wp, Cout, 9 * Cin, 9 * Cin, NAN, DEV), b.to(DEV)
    res_d = poisoned(res, B * H * Wd, Cout, Cout + 12, NAN, DEV).unflatten(0, (B, H, Wd))
    name = f"bounds_halo_{'_'.join(map(str, case))}_ldc+{ldc_pad}_ldx+{ldx_pad}"
    out, chk = guarded(B * H * Wd, Cout, Cout + ldc_pad, F16, DEV)
    o.gemm(x_d, w_d, bias=b_d, residual=res_d, out=out.unflatten(0, (B, H, Wd)), conv=dict(KH=3, KW=3, stride=1, pad=1, halo=True))
    check_close(results_log, name, out, ref)
    done(chk, name)
    # routed, with the channel statistics of the stored values in a guarded buffer
    l.api.lb_gemm_set_halo(2)
    try:
        rows = o.conv_ch_stat_rows(B, H, Wd, Cin, Cout)
        assert rows > 0
        st, st_chk = guarded(Cout, B * rows * 2, B * rows * 2, F32, DEV)
        out, chk = guarded(B * H * Wd, Cout, Cout + ldc_pad, F16, DEV)
        o.gemm(x_d, w_d, bias=b_d, residual=res_d, out=out.unflatten(0, (B, H, Wd)), conv=dict(KH=3, KW=3, stride=1, pad=1),
               ch_stats=st.view(Cout, B * rows, 2))
    finally:
        l.api.lb_gemm_set_halo(1)
    check_close(results_log, name + "_routed_stats", out, ref)
    done(chk, name + "_routed_stats")
    done(st_chk, name + " ch_stats")
    yf = out.double().reshape(B, H * Wd, Cout).cpu()
    tot = st.reshape(Cout, B, rows, 2).double().sum(dim=2).permute(1, 0, 2).cpu()
    assert torch.allclose(tot[..., 0], yf.sum(dim=1), rtol=1e-4, atol=1e-2)
    assert torch.allclose(tot[..., 1], (yf ** 2).sum(dim=1), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("ldc_pad,ldx_pad", [(4, 8), (0, 0)])
@pytest.mark.parametrize("case", [(2, 32, 128, 3, True), (3, 16, 64, 7, True)], ids=lambda c: "_".join(map(str, c)))
def test_conv3x3_narrow_memory_contract(case, ldc_pad, ldx_pad, results_log):
    """lb_conv3x3_narrow_f16 (routed by lb_gemm_f16: tile code 8) with an fp32 output whose pixels are ldc > N apart and an
    input whose pixels are ldx > Cin apart; a pixel stride that is no multiple of 8 is refused."""
    o, l = ops(), lib()
    B, H, Cin, Cout, f32 = case
    x, w = rnd(B, Cin, H, H, seed=201), rnd(Cout, Cin, 3, 3, seed=202, scale=(9 * Cin) ** -0.5)
    b = rnd(Cout, seed=203, dtype=F32)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
    cout_p = (Cout + 3) // 4 * 4
    wp = torch.zeros(cout_p, 9 * Cin, dtype=F16)
    wp[:Cout] = o.pack_conv_weight(w, Cin)
    bp = torch.zeros(cout_p, dtype=F32)
    bp[:Cout] = b
    x_d, w_d = _nhwc_poisoned(x, Cin, Cin + ldx_pad), poisoned(wp, cout_p, 9 * Cin, 9 * Cin, NAN, DEV)
    flags = l.GEMM_OUT_F32 if f32 else 0
    p = l.conv_probe(B, H, H, Cin, cout_p, flags=flags, zero_page=o.zero_page(DEV).data_ptr())
    p.ldx = Cin + ldx_pad                   # (the padded pixel stride of x_d)
    t = C.c_int()
    l.api.lb_gemm_plan(C.byref(p), C.byref(t), None, None)
    assert t.value == 8
    name = f"bounds_narrow_{'_'.join(map(str, case))}_ldc+{ldc_pad}_ldx+{ldx_pad}"
    out, chk = guarded(B * H * H, cout_p, cout_p + ldc_pad, F32 if f32 else F16, DEV)
    o.gemm(x_d, w_d, bias=bp.to(DEV), flags=flags, out=out.unflatten(0, (B, H, H)), conv=dict(KH=3, KW=3, stride=1, pad=1))
    check_close(results_log, name, out[:, :Cout], ref)
    assert float(out[:, Cout:].abs().max()) == 0
    done(chk, name)
    # ldc that is no multiple of 4: refused, nothing stored
    out, chk = guarded(B * H * H, cout_p, cout_p + 2, F32 if f32 else F16, DEV)
    refused(lambda: o.gemm(x_d, w_d, bias=bp.to(DEV), flags=flags, out=out.unflatten(0, (B, H, H)),
                           conv=dict(KH=3, KW=3, stride=1, pad=1)), chk, name + " ldc % 4 != 0")


@pytest.mark.parametrize("ldc_pad,ldx_pad", [(8, 8), (4, 0)])
def test_upconv2x_halo_memory_contract(ldc_pad, ldx_pad, results_log):
    """lb_upconv2x_halo_f16 (all four parities in one launch, N = 200: a last channel block that overhangs N) scattering into a
    guarded [B, 2H, 2W, ldc] output, with the channel statistics in a guarded buffer."""
    o, l = ops(), lib()
    B, H, Wd, Cin, Cout = 2, 16, 16, 64, 200
    x, w = rnd(B, Cin, H, Wd, seed=190), rnd(Cout, Cin, 3, 3, seed=191, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=192, dtype=F32)
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), w.double(), bias.double(), padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, Cout)
    subs = o.subpixel_upsample_weights(w)
    w4 = torch.stack([subs[(0, 0)], subs[(0, 1)], subs[(1, 0)], subs[(1, 1)]]).reshape(4 * Cout, 4 * Cin)
    w_d = poisoned(w4, 4 * Cout, 4 * Cin, 4 * Cin, NAN, DEV)
    x_d = _nhwc_poisoned(x, Cin, Cin + ldx_pad)
    name = f"bounds_upconv_ldc+{ldc_pad}_ldx+{ldx_pad}"
    out, chk = guarded(B * 4 * H * Wd, Cout, Cout + ldc_pad, F16, DEV)
    o.gemm(x_d, w_d[:Cout], bias=bias.to(DEV), out=out.unflatten(0, (B, 2 * H, 2 * Wd)),
           conv=dict(KH=2, KW=2, stride=1, pad=0, parity="all"))
    check_close(results_log, name, out, ref, rel=3e-3)
    done(chk, name)
    rows = o.conv_ch_stat_rows(B, H, Wd, Cin, Cout, ks=2)
    assert rows > 0
    st, st_chk = guarded(Cout, B * rows * 2, B * rows * 2, F32, DEV)
    out, chk = guarded(B * 4 * H * Wd, Cout, Cout + ldc_pad, F16, DEV)
    o.gemm(x_d, w_d[:Cout], bias=bias.to(DEV), out=out.unflatten(0, (B, 2 * H, 2 * Wd)),
           conv=dict(KH=2, KW=2, stride=1, pad=0, parity="all"), ch_stats=st.view(Cout, B * rows, 2))
    check_close(results_log, name + "_stats", out, ref, rel=3e-3)
    done(chk, name + "_stats")
    done(st_chk, name + " ch_stats")
    yf = out.double().reshape(B, 4 * H * Wd, Cout).cpu()
    tot = st.reshape(Cout, B, rows, 2).double().sum(dim=2).permute(1, 0, 2).cpu()
    assert torch.allclose(tot[..., 0], yf.sum(dim=1), rtol=1e-4, atol=1e-2)
    assert torch.allclose(tot[..., 1], (yf ** 2).sum(dim=1), rtol=1e-4, atol=1e-2)


# ====================================================================== attention =============
ATTN_FORCES = [0, 1, 2, 17, 18, 65, 66, 129, 130, 257, 258, 273, 513, 514, 529, 530, 2049, 2066]


def _attention_ref(q, k, v, heads, valid, scale, causal=False):
    """fp64 softmax attention over the first `valid` keys; q [B, Sq, H*D], k, v [B, Skv, H*D]."""
    B, Sq, Cc = q.shape
    D = Cc // heads
    qh, kh, vh = [t.double().reshape(B, -1, heads, D).transpose(1, 2) for t in (q, k[:, :valid], v[:, :valid])]
    s = qh @ kh.transpose(-1, -2) * scale
    if causal:
        s = s.masked_fill(torch.ones(Sq, valid, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, dim=-1) @ vh).transpose(1, 2).reshape(B, Sq, Cc)


@functools.lru_cache(maxsize=None)
def _attn_operands(B, H, Sq, Skv, valid, D, causal):
    """One [tokens, 4C] device buffer laid out [q | k | v | NaN] (NaN rows behind it, and NaN where the shorter of Q / KV has no
    tokens); K / V rows in [valid, Skv) are finite and adversarial (K = 8 x a query row, V = 1000): they must be MASKED."""
    Cc = H * D
    q, k, v = rnd(B, Sq, Cc, seed=61), rnd(B, Skv, Cc, seed=62), rnd(B, Skv, Cc, seed=63)
    for b in range(B):
        k[b, valid:] = 8.0 * q[b, 0]
        v[b, valid:] = 1000.0
    ref = _attention_ref(q, k, v, H, valid, D ** -0.5, causal)
    rows = B * max(Sq, Skv)
    buf = torch.full((rows, 3 * Cc), NAN, dtype=F16)
    buf[:B * Sq, :Cc] = q.reshape(-1, Cc)
    buf[:B * Skv, Cc:2 * Cc] = k.reshape(-1, Cc)
    buf[:B * Skv, 2 * Cc:] = v.reshape(-1, Cc)
    d = poisoned(buf, rows, 3 * Cc, 4 * Cc, NAN, DEV)
    return ref, d[:B * Sq, :Cc], d[:B * Skv, Cc:2 * Cc], d[:B * Skv, 2 * Cc:]


@pytest.mark.parametrize("force", ATTN_FORCES)
@pytest.mark.parametrize("case", [(2, 2, 130, 80, 77), (1, 1, 16, 8, 5), (2, 3, 300, 300, 300), (2, 12, 77, 77, 77, "causal")],
                         ids=lambda c: "_".join(map(str, c)))
def test_attention_d64_memory_contract(case, force, results_log):
    """lb_attn_fwd_d64, every kernel variant: Q, K, V as column slices of one [tokens, 4C] buffer whose fourth quarter is NaN,
    finite adversarial K / V rows behind Skv_valid, output rows ldo = C + 64 apart in a guarded buffer."""
    o, l = ops(), lib()
    B, H, Sq, Skv, valid = case[:5]
    causal = len(case) > 5
    Cc = H * 64
    ref, q, k, v = _attn_operands(B, H, Sq, Skv, valid, 64, causal)
    name = f"bounds_attn_f{force}_{'_'.join(map(str, case))}"
    out, chk = guarded(B * Sq, Cc, Cc + 64, F16, DEV)
    l.api.lb_attn_set_tuning(force)
    try:
        o.attention_d64(q, k, v, B, H, Sq, Skv, valid, out=out, causal=causal)
    finally:
        l.api.lb_attn_set_tuning(0)
    check_close(results_log, name, out.reshape(B, Sq, Cc), ref, floor=2e-3)
    done(chk, name)


@pytest.mark.parametrize("case", [(3, 1, 130, 33, 33), (1, 2, 200, 200, 200), (2, 1, 100, 77, 70)], ids=lambda c: "_".join(map(str, c)))
def test_attention_d512_memory_contract(case, results_log):
    """lb_attn_fwd_d512 with the same operand layout and ldo = C + 8."""
    o = ops()
    B, H, Sq, Skv, valid = case
    Cc = H * 512
    ref, q, k, v = _attn_operands(B, H, Sq, Skv, valid, 512, False)
    name = f"bounds_attn512_{'_'.join(map(str, case))}"
    out, chk = guarded(B * Sq, Cc, Cc + 8, F16, DEV)
    o.attention_d512(q, k, v, B, H, Sq, Skv, valid, out=out)
    check_close(results_log, name, out.reshape(B, Sq, Cc), ref, floor=2e-3)
    done(chk, name)


def test_softmax_rows_memory_contract(results_log):
    """lb_softmax_rows_f16 in place on rows that are ld = 312 apart: the pad columns and both guards must survive.  N = 304 is the
    widest supported width under that stride (the kernel works in 16-byte vectors); the launcher REFUSES N = 300 (N % 8 != 0)
    and then leaves the buffer untouched."""
    o = ops()
    x = rnd(7, 304, seed=57, scale=4.0)
    buf, chk = guarded(7, 304, 312, F16, DEV)
    buf.copy_(x.to(DEV))
    o.softmax_rows_(buf, 0.3)
    check_close(results_log, "bounds_softmax_rows_7x304_ld312", buf, torch.softmax(x.double() * 0.3, dim=-1), floor=1e-4)
    done(chk, "softmax_rows 7x304 ld 312")
    buf, chk = guarded(7, 300, 312, F16, DEV)
    refused(lambda: o.softmax_rows_(buf, 0.3), chk, "softmax_rows 7x300 ld 312")


# ====================================================================== norms =================
@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("shape", [(9, 1032), (131, 768), (5, 64)])
def test_layernorm_memory_contract(shape, form, results_log):
    """lb_layernorm_f16, both kernels: ldx = C + 8 (NaN pad and NaN rows behind), ldy = C + 16."""
    l = lib()
    M, Cc = shape
    x = rnd(M, Cc, seed=48, scale=3.0) + 1
    gamma, beta = rnd(Cc, seed=49, dtype=F32) * 0.1 + 1, rnd(Cc, seed=50, dtype=F32) * 0.1
    ref = F.layer_norm(x.double(), (Cc,), gamma.double(), beta.double(), 1e-5)
    x_d = poisoned(x, M, Cc, Cc + 8, NAN, DEV)
    out, chk = guarded(M, Cc, Cc + 16, F16, DEV)
    g_d, b_d = gamma.to(DEV), beta.to(DEV)
    l.api.lb_layernorm_set_form(form)
    try:
        l.api.lb_layernorm_f16(x_d.data_ptr(), out.data_ptr(), g_d.data_ptr(), b_d.data_ptr(), M, Cc, Cc + 8, Cc + 16, 1e-5, stream())
    finally:
        l.api.lb_layernorm_set_form(1)
    check_close(results_log, f"bounds_layernorm_{M}_{Cc}_form{form}", out, ref, floor=2e-3)
    done(chk, f"layernorm {shape} form {form}")


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("case", [(2, 250, 640, False), (2, 64, 32, False), (3, 256, 1280, False), (1, 250, 128, True)],
                         ids=lambda c: "_".join(map(str, c)))
def test_groupnorm_memory_contract(case, silu, fused, results_log):
    """lb_groupnorm_nhwc, one-launch and statistics + apply forms, fp16 and fp32 input: pixels ldx = C + 32 apart with NaN in
    between (the statistics must not see them), output pixels ldy = C + 8 apart."""
    o, l = ops(), lib()
    B, HW, Cc, f32_in = case
    x = rnd(B * HW, Cc, seed=45, scale=2.0, dtype=F32 if f32_in else F16) + 0.5
    gamma, beta = rnd(Cc, seed=46, dtype=F32) * 0.1 + 1, rnd(Cc, seed=47, dtype=F32) * 0.1
    ref = F.group_norm(x.double().reshape(B, HW, Cc).permute(0, 2, 1), 32, gamma.double(), beta.double(), 1e-5).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    x_d = poisoned(x, B * HW, Cc, Cc + 32, NAN, DEV).unflatten(0, (B, HW))
    out, chk = guarded(B * HW, Cc, Cc + 8, F16, DEV)
    l.api.lb_groupnorm_set_fused(fused)
    try:
        o.groupnorm_nhwc(x_d, gamma.to(DEV), beta.to(DEV), 32, 1e-5, silu, ldx=Cc + 32, ldy=Cc + 8, out=out)
    finally:
        l.api.lb_groupnorm_set_fused(1)
    name = f"bounds_groupnorm_{B}_{HW}_{Cc}_{int(f32_in)}_{int(silu)}_fused{fused}"
    check_close(results_log, name, out.reshape(B, HW, Cc), ref, floor=2e-3)
    done(chk, name)


def test_groupnorm_from_stats_memory_contract(results_log):
    """lb_groupnorm_from_stats on the output of a halo conv that left its channel statistics (case (2, 32, 128, 128) of the
    existing test): the conv output read with ldx = C + 8, the normalised output written with ldy = C + 16."""
    o, l = ops(), lib()
    B, H, Cin, Cout = 2, 32, 128, 128
    x, w = rnd(B, Cin, H, H, seed=211), rnd(Cout, Cin, 3, 3, seed=212, scale=(9 * Cin) ** -0.5)
    b = rnd(Cout, seed=213, dtype=F32)
    xn, wp = x.permute(0, 2, 3, 1).contiguous().to(DEV), o.pack_conv_weight(w, Cin).to(DEV)
    l.api.lb_gemm_set_halo(2)
    try:
        rows = o.conv_ch_stat_rows(B, H, H, Cin, Cout)
        assert rows > 0
        st, st_chk = guarded(Cout, B * rows * 2, B * rows * 2, F32, DEV)
        y, y_chk = guarded(B * H * H, Cout, Cout + 8, F16, DEV)
        o.gemm(xn, wp, bias=b.to(DEV), alpha=0.5, out=y.unflatten(0, (B, H, H)), conv=dict(KH=3, KW=3, stride=1, pad=1),
               ch_stats=st.view(Cout, B * rows, 2))
    finally:
        l.api.lb_gemm_set_halo(1)
    done(y_chk, "conv output feeding groupnorm_from_stats")
    done(st_chk, "ch_stats feeding groupnorm_from_stats")
    gamma, beta = 1 + 0.1 * rnd(Cout, seed=215, dtype=F32), 0.1 * rnd(Cout, seed=216, dtype=F32)
    ref = F.silu(F.group_norm(y.double().cpu().reshape(B, H * H, Cout).permute(0, 2, 1), 32, gamma.double(), beta.double(), 1e-6))
    out, chk = guarded(B * H * H, Cout, Cout + 16, F16, DEV)
    o.groupnorm_from_stats(y.unflatten(0, (B, H, H)), gamma.to(DEV), beta.to(DEV), 32, 1e-6, True, st.view(Cout, B * rows, 2), rows,
                           ldx=Cout + 8, ldy=Cout + 16, out=out)
    check_close(results_log, "bounds_groupnorm_from_stats", out.reshape(B, H * H, Cout), ref.permute(0, 2, 1))
    done(chk, "groupnorm_from_stats")


# ====================================================================== mixing / scheduler ====
MIX_N = [8 * 37, 32768 + 8]


def _ptrs(tensors):
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return C.cast(arr, lib().c_void_pp), arr


@pytest.mark.parametrize("n", MIX_N)
def test_slerp_memory_contract(n, results_log):
    """lb_slerp_pairs_f16 / _f32 / _f64, lb_slerp_batched_f16, lb_slerp_strided_f16 (contiguous and broadcast) into guarded
    outputs, inputs with NaN behind them: <= 1 fp16 ulp against the oracle (fp32 / fp64 inputs: the existing 1e-6)."""
    l = lib()
    G = 5
    fr = [0.0, 1.0, 0.5, 0.37, 0.8]
    a, b = rnd(G, n, seed=71), rnd(G, n, seed=72)
    ref = torch.stack([R.slerp(a[g], b[g], fr[g]) for g in range(G)])
    a_d, b_d = poisoned(a, G, n, n, NAN, DEV, extra_rows=1), poisoned(b, G, n, n, NAN, DEV, extra_rows=1)
    frd = torch.tensor(fr, dtype=F64, device=DEV)
    frh = (C.c_double * G)(*fr)
    # pairs: one guarded output per pair
    outs = [guarded(1, n, n, F16, DEV, back_rows=1) for _ in range(G)]
    pa, ka = _ptrs([a_d[g] for g in range(G)])
    pb, kb = _ptrs([b_d[g] for g in range(G)])
    po, ko = _ptrs([t for t, _ in outs])
    l.api.lb_slerp_pairs_f16(pa, pb, po, frh, G, n, stream())
    for g, (t, chk) in enumerate(outs):
        assert ulp_diff_f16(t[0], ref[g]) <= 1, f"slerp_pairs_f16 n={n} pair {g}"
        done(chk, f"slerp_pairs_f16 n={n} pair {g}")
    for dt, fn in ((F32, l.api.lb_slerp_pairs_f32), (F64, l.api.lb_slerp_pairs_f64)):
        x, y = rnd(1, n, seed=4, dtype=dt), rnd(1, n, seed=5, dtype=dt)
        x_d, y_d = poisoned(x, 1, n, n, NAN, DEV, extra_rows=1), poisoned(y, 1, n, n, NAN, DEV, extra_rows=1)
        t, chk = guarded(1, n, n, F32, DEV, back_rows=1)
        px, kx = _ptrs([x_d]); py, ky = _ptrs([y_d]); pt, kt = _ptrs([t])
        fn(px, py, pt, (C.c_double * 1)(0.41), 1, n, stream())
        assert torch.allclose(t[0].cpu(), R.slerp(x[0], y[0], 0.41), rtol=1e-6, atol=1e-6)
        done(chk, f"slerp_pairs {dt} n={n}")
    # batched and strided
    out, chk = guarded(G, n, n, F16, DEV, back_rows=2)
    l.api.lb_slerp_batched_f16(a_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), frd.data_ptr(), G, n, stream())
    ub = ulp_diff_f16(out, ref)
    done(chk, f"slerp_batched n={n}")
    out, chk = guarded(G, n, n, F16, DEV, back_rows=2)
    l.api.lb_slerp_strided_f16(a_d.data_ptr(), n, b_d.data_ptr(), n, out.data_ptr(), frd.data_ptr(), G, n, stream())
    us = ulp_diff_f16(out, ref)
    done(chk, f"slerp_strided n={n}")
    out, chk = guarded(G, n, n, F16, DEV, back_rows=2)
    l.api.lb_slerp_strided_f16(a_d.data_ptr(), 0, b_d.data_ptr(), 0, out.data_ptr(), frd.data_ptr(), G, n, stream())
    u0 = ulp_diff_f16(out, torch.stack([R.slerp(a[0], b[0], f) for f in fr]))
    done(chk, f"slerp_strided broadcast n={n}")
    results_log[f"bounds_slerp_n{n}"] = {"ulp_batched": ub, "ulp_strided": us, "ulp_broadcast": u0}
    print(f"[parity] bounds_slerp_n{n}: ulp batched {ub} strided {us} broadcast {u0}")
    assert ub <= 1 and us <= 1 and u0 <= 1


@pytest.mark.parametrize("n", MIX_N + [8 * 37 + 3])
def test_lerp_memory_contract(n, results_log):
    """lb_lerp_f16 / lb_lerp_f32 into guarded outputs: bit-exact against the oracle (a length with a scalar tail included)."""
    l = lib()
    for dt, fn in ((F16, l.api.lb_lerp_f16), (F32, l.api.lb_lerp_f32)):
        a, b = rnd(1, n, seed=11, dtype=dt), rnd(1, n, seed=12, dtype=dt)
        a_d, b_d = poisoned(a, 1, n, n, NAN, DEV, extra_rows=1), poisoned(b, 1, n, n, NAN, DEV, extra_rows=1)
        for f in (0.0, 0.7321, 1.0):
            out, chk = guarded(1, n, n, dt, DEV, back_rows=1)
            fn(a_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), n, f, stream())
            assert torch.equal(out.cpu(), R.lerp(a, b, f)), f"lerp {dt} n={n} f={f}"
            done(chk, f"lerp {dt} n={n} f={f}")


@pytest.mark.parametrize("n", MIX_N + [8 * 37 + 3])
def test_scheduler_steps_memory_contract(n, results_log):
    """lb_scale_model_input_f16 (plain and duplicated for CFG), lb_euler_step_f16 (plain, ancestral, CFG combine) and
    lb_ddim_step_f16 (plain, CFG) on [B, n] latents into guarded outputs: <= 1 fp16 ulp against the oracle schedulers.
    (lb_lcm_step_f16 and lb_dpmpp2m_step_f16: see the module docstring.)"""
    from latentblending_amd.native.scheduler import NativeDDIMScheduler
    o, l = ops(), lib()
    B, g = 2, 3.5
    x, eps, noise = rnd(B, n, seed=15, scale=5.0), rnd(2 * B, n, seed=16), rnd(B, n, seed=17)
    x_d, eps_d = poisoned(x, B, n, n, NAN, DEV, extra_rows=1), poisoned(eps, 2 * B, n, n, NAN, DEV, extra_rows=1)
    noise_d = poisoned(noise, B, n, n, NAN, DEV, extra_rows=1)
    worst = {}
    for ancestral in (False, True):
        sched = R.EulerScheduler(ancestral=ancestral)
        sched.set_timesteps(4 if ancestral else 30)
        i = 2
        t = sched.timesteps[i]
        s_from, s_to = float(sched.sigmas[i]), float(sched.sigmas[i + 1])
        if ancestral:
            s_up, s_down = R.ancestral_sigmas(s_from, s_to)
            row = (s_from, s_down, s_up, g, s_down - s_from)
        else:
            row = (s_from, s_to, 0.0, g, s_to - s_from)
        params = o.step_params([row] * B, DEV)
        want = []
        for b in range(B):
            sched._step_index = None
            sched.noise_source = lambda shape, b=b: noise[b:b + 1]
            want.append(sched.step(eps[b:b + 1], t, x[b:b + 1])[0])
        out, chk = guarded(B, n, n, F16, DEV, back_rows=2)
        l.api.lb_euler_step_f16(x_d.data_ptr(), eps_d.data_ptr(), noise_d.data_ptr(), out.data_ptr(), params.data_ptr(), n, B, 0,
                                int(ancestral), stream())
        worst[f"euler_anc{int(ancestral)}"] = ulp_diff_f16(out, torch.cat(want))
        done(chk, f"euler_step ancestral={ancestral} n={n}")
        if not ancestral:
            sched._step_index = None
            for dup in (0, 1):
                out, chk = guarded(B * (1 + dup), n, n, F16, DEV, back_rows=2)
                l.api.lb_scale_model_input_f16(x_d.data_ptr(), out.data_ptr(), params.data_ptr(), n, B, dup, stream())
                sched._step_index = None
                ref = sched.scale_model_input(x, t)
                worst[f"scale_dup{dup}"] = ulp_diff_f16(out, torch.cat([ref] * (1 + dup)))
                done(chk, f"scale_model_input dup={dup} n={n}")
            # CFG combine in the Euler step (the closed form of test_euler_cfg_combine)
            eu, et = eps[:B], eps[B:]
            e = (eu + g * (et - eu)).float()
            x0 = x.float() - s_from * e
            ref = (x.float() + ((x.float() - x0) / s_from) * (s_to - s_from)).half()
            out, chk = guarded(B, n, n, F16, DEV, back_rows=2)
            l.api.lb_euler_step_f16(x_d.data_ptr(), eps_d.data_ptr(), None, out.data_ptr(), params.data_ptr(), n, B, 1, 0, stream())
            worst["euler_cfg"] = ulp_diff_f16(out, ref)
            done(chk, f"euler_step cfg n={n}")
    nd, rd = NativeDDIMScheduler(device=DEV), R.DDIMScheduler()
    nd.set_timesteps(30); rd.set_timesteps(30)
    params = o.step_params([nd.step_row(13, g)] * B, DEV)
    for cfg in (0, 1):
        e = eps[:B] + g * (eps[B:] - eps[:B]) if cfg else eps[:B]
        want = rd.step(e, int(rd.timesteps[13]), x)[0]
        out, chk = guarded(B, n, n, F16, DEV, back_rows=2)
        l.api.lb_ddim_step_f16(x_d.data_ptr(), eps_d.data_ptr(), out.data_ptr(), params.data_ptr(), n, B, cfg, stream())
        worst[f"ddim_cfg{cfg}"] = ulp_diff_f16(out, want)
        done(chk, f"ddim_step cfg={cfg} n={n}")
    results_log[f"bounds_scheduler_n{n}"] = worst
    print(f"[parity] bounds_scheduler_n{n}: max ulp {worst}")
    assert max(worst.values()) <= 1, worst


# ====================================================================== small kernels past the grid cap
# (misc.hip launches at most 2048 blocks of 256 threads: every case below has more than 524 288 work items and an odd tail, so
#  the grid-stride loop goes round at least twice and ends inside a block)
CAP = 2048 * 256


def test_copy_cols_past_grid_cap():
    o = ops()
    rows, cols = 4100, 1032
    assert rows * (cols // 8) > CAP
    src = rnd(rows, cols, seed=58)
    src_d = poisoned(src, rows, cols, 1040, NAN, DEV, extra_rows=2)
    dst, chk = guarded(rows, 2080, 2080, F16, DEV, back_rows=2)
    o.copy_cols(src_d, dst[:, :1040], 0)              # left half: columns 0..1031; 1032..1039 must stay untouched
    o.copy_cols(src_d, dst, 1040)                     # right half at dst_off 1040: columns 1040..2071
    got = dst.cpu()
    assert torch.equal(got[:, :cols], src) and torch.equal(got[:, 1040:1040 + cols], src)
    chk.assert_intact("copy_cols")
    sent = chk.bits[chk.front:chk.front + rows * 2080].view(rows, 2080)
    assert bool((sent[:, cols:1040] == chk.sentinel).all()) and bool((sent[:, 1040 + cols:] == chk.sentinel).all()), \
        "copy_cols wrote between / behind the copied column ranges"


def test_casts_and_fill_past_grid_cap():
    o = ops()
    n = CAP + 3
    h = rnd(1, n, seed=301, scale=30.0)
    out, chk = guarded(1, n, n, F32, DEV, back_rows=1)
    o.cast_f16_to_f32(poisoned(h, 1, n, n, NAN, DEV, extra_rows=1)[0], out=out[0])
    assert torch.equal(out.cpu(), h.float())
    done(chk, "cast_f16_to_f32")
    f = rnd(1, n, seed=302, dtype=F32, scale=3e4)
    f[0, :8] = torch.tensor([1e6, -1e6, float("inf"), float("-inf"), 65504.0 * 8, -65504.0 * 8, 524287.9, 8.0])
    f[0, -3:] = torch.tensor([1e6, -1e6, 1.0])
    mul = 2.0 ** -3
    out, chk = guarded(1, n, n, F16, DEV, back_rows=1)
    o.cast_f32_to_f16(poisoned(f, 1, n, n, NAN, DEV, extra_rows=1)[0], mul, out=out[0])
    ref = (f.double() * mul).clamp(-65504.0, 65504.0).to(F16)          # (x * 2^-3 is exact in fp32; one rounding to fp16 either way)
    got = out.cpu()
    assert torch.equal(got, ref)
    assert got[0, :4].tolist() == [65504.0, -65504.0, 65504.0, -65504.0] and got[0, -3:].tolist() == [65504.0, -65504.0, 0.125]
    done(chk, "cast_f32_to_f16")
    out, chk = guarded(1, n, n, F32, DEV, back_rows=1)
    o.fill_f32_(out[0], -2.5)
    assert bool((out == -2.5).all())
    done(chk, "fill_f32")


def test_layout_converts_past_grid_cap(results_log):
    """lb_nchw_to_nhwc_f16 walks B * HW * ld items, lb_nhwc_to_nchw_f16 B * C * HW: (B 2, C 4, HW 33000, ld 8) takes the first past
    the grid cap; the second runs at that size and at HW = 66001, where it passes the cap as well (odd tail)."""
    l = lib()
    B, Cc, HW, ld = 2, 4, 33000, 8
    assert B * HW * ld > CAP
    z = rnd(B, Cc, HW, seed=60)
    mul = 1 / 0.13025
    z_d = poisoned(z.reshape(1, -1), 1, z.numel(), z.numel(), NAN, DEV, extra_rows=1)
    out, chk = guarded(B * HW, ld, ld, F16, DEV, back_rows=2)         # (the kernel writes all ld channels: C..ld as zeros)
    l.api.lb_nchw_to_nhwc_f16(z_d.data_ptr(), out.data_ptr(), B, Cc, HW, ld, mul, stream())
    got = out.reshape(B, HW, ld).cpu()
    ref = (z.float() * torch.tensor(mul, dtype=F32)).half().permute(0, 2, 1)       # one fp32 multiply, one rounding: exact
    assert torch.equal(got[..., :Cc], ref) and bool((got[..., Cc:] == 0).all())
    check_close(results_log, "bounds_nchw_to_nhwc", got[..., :Cc], z.double().permute(0, 2, 1) / 0.13025)
    done(chk, "nchw_to_nhwc")
    for HW in (33000, 66001):
        z = rnd(B, Cc, HW, seed=60)
        nh = torch.full((B * HW, ld), NAN, dtype=F16)
        nh[:, :Cc] = z.permute(0, 2, 1).reshape(-1, Cc)
        nh_d = poisoned(nh, B * HW, ld, ld, NAN, DEV, extra_rows=2)
        out, chk = guarded(B * Cc, HW, HW, F16, DEV, back_rows=1)
        l.api.lb_nhwc_to_nchw_f16(nh_d.data_ptr(), out.data_ptr(), B, Cc, HW, ld, stream())
        assert torch.equal(out.reshape(B, Cc, HW).cpu(), z)
        done(chk, f"nhwc_to_nchw HW={HW}")
    assert B * Cc * 66001 > CAP


@pytest.mark.parametrize("dtype", [F16, F32])
def test_postprocess_u8_past_grid_cap(dtype):
    """uint8 output, where the sentinel byte is a legal value: run with two sentinels, require equal (and correct) results."""
    l = lib()
    H = 420
    assert H * H * 3 > CAP
    img = rnd(1, 3, H, H, seed=61, dtype=dtype)
    x4 = torch.full((H * H, 4), NAN, dtype=dtype)
    x4[:, :3] = img[0].permute(1, 2, 0).reshape(-1, 3)
    x_d = poisoned(x4, H * H, 4, 4, NAN, DEV, extra_rows=2)
    ref = R.postprocess_u8(img.float())[0]
    got = []
    for sentinel in (0xA5, 0x5A):
        out, chk = guarded(H * H, 3, 3, torch.uint8, DEV, back_rows=2, sentinel=sentinel)
        l.api.lb_postprocess_u8(x_d.data_ptr(), out.data_ptr(), H * H, 4, int(dtype == F32), stream())
        chk.assert_intact(f"postprocess_u8 {dtype} sentinel {sentinel:#x}")
        got.append(out.cpu().numpy().reshape(H, H, 3))
    assert np.array_equal(got[0], got[1]), "postprocess_u8 left bytes unwritten"
    assert np.array_equal(got[0], ref)


def test_lpips_prep_u8_past_grid_cap(results_log):
    o = ops()
    H = 730
    assert H * H > CAP
    g = torch.Generator().manual_seed(9)
    img = (torch.rand(H * H, 3, generator=g) * 256).to(torch.uint8)
    img_d = poisoned(img.reshape(1, -1), 1, img.numel(), img.numel(), 0xFF, DEV, extra_rows=1)[0].reshape(H * H, 3)
    out, chk = guarded(H * H, 8, 8, F16, DEV, back_rows=2)
    o.lpips_prep_u8(img_d, out=out)
    shift, scale = torch.tensor([-.030, -.088, -.188], dtype=F64), torch.tensor([.458, .448, .450], dtype=F64)
    ref = ((2.0 * img.double() / 255.0 - 1.0) - shift) / scale
    got = out.cpu()
    check_close(results_log, "bounds_lpips_prep_u8", got[:, :3], ref)
    assert bool((got[:, 3:] == 0).all())
    done(chk, "lpips_prep_u8")


def test_maxpool3s2_past_grid_cap():
    l = lib()
    N, H, Cc = 2, 131, 512
    Ho = (H - 3) // 2 + 1
    assert N * Ho * Ho * (Cc // 8) > CAP
    f = rnd(N, H, H, Cc, seed=62)
    ref = F.max_pool2d(f.float().permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).half()        # (a maximum is exact in any precision)
    f_d = poisoned(f.reshape(N * H * H, Cc), N * H * H, Cc, Cc, NAN, DEV, extra_rows=4)
    out, chk = guarded(N * Ho * Ho, Cc, Cc, F16, DEV, back_rows=4)
    l.api.lb_maxpool3s2_nhwc_f16(f_d.data_ptr(), out.data_ptr(), N, H, H, Cc, stream())
    assert torch.equal(out.reshape(N, Ho, Ho, Cc).cpu(), ref)
    done(chk, "maxpool3s2")


def test_sinusoid_past_grid_cap(results_log):
    o = ops()
    rows, dim, col_off, ld = 2100, 256, 24, 256 + 24 + 40
    assert rows * dim > CAP
    vals = (torch.arange(rows, dtype=F32) * 0.4763).reshape(rows, 1)
    vals_d = poisoned(vals, rows, 1, 3, NAN, DEV, extra_rows=2)           # (val_stride 3: NaN between the values)
    out, chk = guarded(rows, ld, ld, F16, DEV, back_rows=2)
    o.sinusoid(vals_d, dim, out=out, col_off=col_off)
    ref = R.sinusoid(vals.reshape(-1), dim)
    check_close(results_log, "bounds_sinusoid", out[:, col_off:col_off + dim], ref, floor=2e-3)
    chk.assert_intact("sinusoid")
    sent = chk.bits[chk.front:chk.front + rows * ld].view(rows, ld)
    assert bool((sent[:, :col_off] == chk.sentinel).all()) and bool((sent[:, col_off + dim:] == chk.sentinel).all()), \
        "sinusoid wrote outside columns col_off .. col_off + dim"
    assert not bool((sent[:, col_off:col_off + dim] == chk.sentinel).any()), "sinusoid left elements unwritten"


def test_embed_tokens_and_gather_rows_past_grid_cap():
    o = ops()
    rows, seq, Cc, vocab = 4200, 77, 1024, 1000
    assert rows * (Cc // 8) > CAP
    tok, pos = rnd(vocab, Cc, seed=401), rnd(seq, Cc, seed=402)
    g = torch.Generator().manual_seed(403)
    ids = torch.randint(0, vocab, (rows,), generator=g, dtype=torch.int32)
    ids[0], ids[1], ids[-1], ids[-2] = -1, 1005, 1005, -1                 # clamped to 0 / vocab - 1
    ref = (tok[ids.long().clamp(0, vocab - 1)].float() + pos[torch.arange(rows) % seq].float()).half()
    out, chk = guarded(rows, Cc, Cc, F16, DEV, back_rows=2)
    o.embed_tokens(ids.to(DEV), poisoned(tok, vocab, Cc, Cc, NAN, DEV, extra_rows=2), poisoned(pos, seq, Cc, Cc, NAN, DEV, extra_rows=2),
                   seq, out=out)
    assert torch.equal(out.cpu(), ref)
    done(chk, "embed_tokens")
    n, ld_src, src_rows = 4200, 1032, 300
    src = rnd(src_rows, Cc, seed=404)
    idx = torch.randint(0, src_rows, (n,), generator=g, dtype=torch.int32)
    idx[0], idx[-1] = src_rows - 1, 0
    out, chk = guarded(n, Cc, Cc, F16, DEV, back_rows=2)
    o.gather_rows(poisoned(src, src_rows, Cc, ld_src, NAN, DEV, extra_rows=2), idx.to(DEV), out=out)
    assert torch.equal(out.cpu(), src[idx.long()])
    done(chk, "gather_rows")


@pytest.mark.parametrize("npairs", [1, 16])
@pytest.mark.parametrize("Cc", [192, 100])
def test_lpips_tap_memory_contract(Cc, npairs, results_log):
    """lb_lpips_tap: HW = 1089 pixels (the block count is capped at 128: four pixels per block per trip, several trips, a ragged
    last one), C = 192 and C = 100 (not a multiple of the 64 lanes), called twice into the same accumulator, against the fp64
    formula of the kernel's comment at the tolerance of test_lpips_matches_oracle (rtol 2e-2)."""
    o = ops()
    HW = 1089
    fa = [F.relu(rnd(HW, Cc, seed=500 + i)) for i in range(npairs)]
    fb = [F.relu(rnd(HW, Cc, seed=600 + i)) for i in range(npairs)]
    lin = rnd(Cc, seed=700, dtype=F32).abs()

    def dist(a, b):
        a, b = a.double(), b.double()
        na = a / (a.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
        nb = b / (b.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
        return float((lin.double() * (na - nb) ** 2).sum(-1).mean())
    want = torch.tensor([dist(a, b) for a, b in zip(fa, fb)], dtype=F64)
    fa_d = [poisoned(t, HW, Cc, Cc, NAN, DEV, extra_rows=2) for t in fa]
    fb_d = [poisoned(t, HW, Cc, Cc, NAN, DEV, extra_rows=2) for t in fb]
    lin_d = poisoned(lin[None], 1, Cc, Cc, NAN, DEV, extra_rows=1)[0]
    acc, chk = guarded(1, npairs, npairs, F32, DEV, back_rows=1)
    ws, ws_chk = guarded(1, 16 * 128, 16 * 128, F32, DEV, back_rows=1)
    o.fill_f32_(acc[0], 0.0)
    o.lpips_tap(fa_d, fb_d, lin_d, acc[0], workspace=ws[0])
    once = acc.cpu().double()[0]
    o.lpips_tap(fa_d, fb_d, lin_d, acc[0], workspace=ws[0])
    twice = acc.cpu().double()[0]
    results_log[f"bounds_lpips_tap_C{Cc}_p{npairs}"] = {"got": once.tolist()[:3], "want": want.tolist()[:3]}
    print(f"[parity] bounds_lpips_tap C={Cc} pairs={npairs}: got {once.tolist()[:3]} want {want.tolist()[:3]}")
    assert torch.allclose(once, want, rtol=2e-2) and torch.allclose(twice, 2 * want, rtol=2e-2)
    done(chk, "lpips_tap acc")
    ws_chk.assert_intact("lpips_tap workspace")


def test_frames_lerp_u8_past_block_cap():
    """lb_frames_lerp_u8 caps blockIdx.x at 512 blocks of 256 16-byte vectors: 840 x 840 x 3 bytes are 132 300 vectors (a second,
    ragged trip).  Exact against the float64 truncating formula; two sentinels for the uint8 output."""
    o = ops()
    g = torch.Generator().manual_seed(3)
    frames = (torch.rand(3, 840, 840, 3, generator=g) * 256).to(torch.uint8)
    fb = frames[0].numel()
    assert fb // 16 > 512 * 256 and fb % 16 == 0
    left, wts = [0, 1, 1, 0], [0.25, 0.5, 0.999, 0.0]
    fn = frames.numpy().astype(np.float64)
    ref = np.stack([((1.0 - w) * fn[k] + w * fn[k + 1]).astype(np.uint8) for k, w in zip(left, wts)])
    frames_d = poisoned(frames.reshape(3, fb), 3, fb, fb, 0xFF, DEV, extra_rows=1).reshape(3, 840, 840, 3)
    got = []
    for sentinel in (0xA5, 0x5A):
        out, chk = guarded(len(left), fb, fb, torch.uint8, DEV, back_rows=1, sentinel=sentinel)
        o.frames_lerp_u8(frames_d, left, wts, out=out.reshape(len(left), 840, 840, 3))
        chk.assert_intact(f"frames_lerp_u8 sentinel {sentinel:#x}")
        got.append(out.cpu().numpy().reshape(ref.shape))
    assert np.array_equal(got[0], got[1]), "frames_lerp_u8 left bytes unwritten"
    assert np.array_equal(got[0], ref)
