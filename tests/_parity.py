"""Seeded inputs and the parity checks shared by the per-kernel GPU tests (test_kernels_gpu.py, test_kernel_bounds_gpu.py)."""
import torch


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def ulp_diff_f16(a, b):
    ai = a.cpu().view(torch.int16).to(torch.int32)
    bi = b.cpu().view(torch.int16).to(torch.int32)
    ai = torch.where(ai < 0, -32768 - ai, ai)
    bi = torch.where(bi < 0, -32768 - bi, bi)
    return int((ai - bi).abs().max())


def check_close(log, name, got, ref, rel=2e-3, frac=2 ** -8, floor=1e-3):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - ref).abs().max().item()
    rl2 = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
    bound = frac * ref.abs().max().item() + floor
    log[name] = {"max_abs": err, "rel_l2": rl2, "bound_abs": bound}
    print(f"[parity] {name}: max_abs={err:.3e} (bound {bound:.3e}) rel_l2={rl2:.3e}")
    assert rl2 <= rel, f"{name}: rel-L2 {rl2:.3e} > {rel}"
    assert err <= bound, f"{name}: max-abs {err:.3e} > {bound:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# Element-wise bounds against a float64 reference (tests/test_value_ranges_gpu.py).  check_close above accepts any error below
# 2^-8 * max|ref| + floor, so an element far smaller than the largest one is not checked at all; the bounds below are per element
# and DERIVED from the number formats - none of them was tuned on what a kernel produced.  All references are float64, computed on
# the CPU from the fp16- / fp32-rounded inputs the kernel reads.
# ---------------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24          # unit round-off of fp32 (round to nearest)
U16 = 2.0 ** -11          # unit round-off of fp16 for normal results
SUB16 = 2.0 ** -25        # half the spacing (2^-24) of fp16 subnormals: the absolute rounding error of a result below 2^-14
ACT_LIPSCHITZ = 1.13      # max |f'| over SiLU (1.0998), ReLU (1), quick-GELU (1.11), erf-GELU (1.129)
ERF_APPROX = 1.5e-7       # documented absolute error of lb_erf (lb_common.h)


def f64(t):
    return t.detach().cpu().double()


def check_elementwise(log, name, got, ref64, bound):
    """Assert |got - ref64| <= bound for EVERY element (bound: a tensor of ref64's shape, or a scalar).  A non-finite ``got`` fails
    wherever the reference is finite.  Logs the worst err / bound under ``name`` and, on failure, prints the index and both values."""
    got = f64(got)
    ref64 = f64(ref64)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    err = (got - ref64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = int((~(err <= bound)).sum())
    log[name] = {"worst_err_over_bound": worst, "max_abs": float(err.max()) if err.numel() else 0.0, "bad": bad}
    print(f"[parity] {name}: worst err/bound={worst:.3f} max_abs={log[name]['max_abs']:.3e} bad={bad}/{err.numel()}")
    if bad:
        idx = tuple(int(i) for i in torch.unravel_index(torch.argmax(ratio), ratio.shape))
        msg = (f"{name}: {bad} of {err.numel()} elements outside the bound; worst at {idx}: got {float(got[idx])!r}, "
               f"ref {float(ref64[idx])!r}, err {float(err[idx]):.3e} > bound {float(bound[idx]):.3e}")
        print("[parity] " + msg)
        raise AssertionError(msg)
    return worst


def store_bound(ref64, out_f32=False):
    """Rounding of the stored value: fp16 round-to-nearest is within 2^-11 |v| for a normal result and within 2^-25 (half a subnormal
    step) below 2^-14; an fp32 store within 2^-24 |v|."""
    a = ref64.abs()
    return U32 * a if out_f32 else torch.maximum(U16 * a, torch.full_like(a, SUB16))


def accumulate_bound(absdot64, K, alpha=1.0):
    """Error of an fp32 dot product of fp16 operands, before the epilogue.  Every product of two fp16 values is exact in fp32
    (22 significand bits); a sum of K such terms in ANY order (MFMA blocks of 16 / 32, split-K slabs, wave partials) is off by at
    most (K - 1) u sum|a_k w_k| + O(u^2) <= K * 2^-24 * (|A| . |W|^T)[i, j]  (Higham, Accuracy and Stability, eq. 4.4)."""
    return abs(alpha) * K * U32 * absdot64


def absdot(A64, W64):
    """(|A| . |W|^T) in float64."""
    return A64.abs() @ W64.abs().t()


def epilogue_bound(ref64, bias=None, residual=None, rowvec=None):
    """The epilogue's fp32 operations (alpha multiply, bias / row-vector / residual adds, conversions): each rounds to within 2^-24 of
    its result, whose magnitude is at most |bias| + |residual| + |rowvec| + |ref|; at most 8 such operations."""
    s = ref64.abs()
    for t in (bias, residual, rowvec):
        if t is not None:
            s = s + f64(t).abs()
    return 8 * U32 * s


def contraction_bound(A64, W64, K, ref64, out_f32=False, alpha=1.0, bias=None, residual=None, rowvec=None, absdot64=None):
    """Bound for C = alpha A . W^T + bias + rowvec + residual stored as fp16 (or fp32 with LB_GEMM_OUT_F32):
    accumulate_bound + epilogue_bound + store_bound.  The store rounds the COMPUTED value, which differs from the reference by the
    first two terms: they enter once more times 2^-11 (2^-24).  ``absdot64``: |A| . |W|^T where the caller computes it another
    way (convolutions: F.conv2d of the absolute values); ``bias`` / ``residual`` / ``rowvec`` broadcast against ref64."""
    ad = absdot(A64, W64) if absdot64 is None else absdot64
    pre = accumulate_bound(ad, K, alpha) + epilogue_bound(ref64, bias, residual, rowvec)
    return pre * (1 + (U32 if out_f32 else U16)) + store_bound(ref64, out_f32)


def activation_bound(pre_bound, act_ref64, out_f32=False):
    """Bound after an activation f in the epilogue (SiLU, ReLU, quick-GELU, erf-GELU), given the bound ``pre_bound`` of the
    pre-activation value (accumulate_bound + epilogue_bound, no store): |f'| <= 1.13 for all of them, plus lb_erf's documented
    1.5e-7, plus 2^-22 |f| for v_exp_f32 / v_rcp_f32 (1 ulp each) and the final multiply, plus the store."""
    pre = ACT_LIPSCHITZ * pre_bound + ERF_APPROX + 2.0 ** -22 * act_ref64.abs()
    return pre * (1 + (U32 if out_f32 else U16)) + store_bound(act_ref64, out_f32)


def geglu_bound(pre_h, pre_g, h64, g64, gelu_g64):
    """GEGLU h * gelu(g): |d(h gelu(g))| <= |gelu(g)| dh + |h| (1.13 dg + 1.5e-7 + 2^-22 |gelu(g)|) + dh * 1.13 dg, one more fp32
    rounding for the product, then the fp16 store."""
    dg = ACT_LIPSCHITZ * pre_g + ERF_APPROX + 2.0 ** -22 * gelu_g64.abs()
    ref = h64 * gelu_g64
    pre = gelu_g64.abs() * pre_h + h64.abs() * dg + pre_h * dg + U32 * ref.abs()
    return pre * (1 + U16) + store_bound(ref)


def norm_bound(ref64, gamma):
    """GroupNorm / LayerNorm (+SiLU) output: O(1) by construction.  One fp16 rounding of the result (2^-11 |ref|) plus the same again
    for everything before it (statistics, rstd, the affine FMA), and 2^-10 max|gamma| for the absolute part: an error of the
    normalised value enters times gamma.  Half the 2e-3 floor test_groupnorm / test_layernorm allow, and relative for large outputs."""
    return 2.0 ** -10 * ref64.abs() + 2.0 ** -10 * float(f64(gamma).abs().max())


def attention_bound(p64, v64, ref64):
    """Attention output = sum_k p_k v_k, a convex combination of V rows with P rounded to fp16 (2^-11 relative per p_k, whatever the
    deferred running maximum makes of its exponent) and summed in fp32, normalised by an fp32 row sum: together at most
    2^-10 sum_k p_k |v_k|; plus the fp16 store 2^-11 |ref| (2^-25 for a subnormal result).  p64: [..., Sq, Skv], v64: [..., Skv, D]."""
    return 2.0 ** -10 * (p64 @ v64.abs()) + store_bound(ref64)
