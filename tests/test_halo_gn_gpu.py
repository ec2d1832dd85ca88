"""GroupNorm (+ SiLU) folded into the consuming 3x3 conv (LB_GEMM_GN_A): the whole-tile halo conv transforms its staged halo in
LDS, the narrow-N conv likewise; lb_groupnorm_affine_from_stats supplies the (scale, shift) table.

The contract is BITWISE: the flagged conv reading the raw tensor equals lb_groupnorm_from_stats followed by the unflagged conv,
because the operand it multiplies is the very fp16 value the apply pass would have stored.  On top of that: float64 element by
element under derived bounds, the table against float64 statistics, guard bands, and the VAE program with the fold on and off."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import _parity as P
from _guard import guarded
from _halo_gn import (DEV, EPS, F16, F32, channel_stats, gn_a_switch, gn_params, run_pair, same_bits, stream_operand,  # noqa: F401
                      entry_of)
from _ksplit import conv_params, lib, nhwc_dev, stream
from _parity import rnd

pytestmark = pytest.mark.gpu


# name -> (B, H, W, Cin, N, groups, forced grid; 0 = the default grid)
SHAPES = {
    # two chunks, 4 tiles: grid 1 = one block walks all of them (tile change, sample change inside one block, every image border);
    # grid 2 = block b takes tiles b and b + 2: one tile of either sample
    "b2_16x32_c128_g1": (2, 16, 32, 128, 128, 32, 1),
    "b2_16x32_c128_g2": (2, 16, 32, 128, 128, 32, 2),
    # the TW = 16 instantiation: one chunk, two channel blocks, a partial last block; 2 channels per group
    "b2_16x16_c64_n192": (2, 16, 16, 64, 192, 32, 0),
    # four chunks, six tiles over two blocks: three tiles per block, a sample change between any two of them
    "b3_8x64_c256_g2": (3, 8, 64, 256, 128, 32, 2),
}


@functools.lru_cache(maxsize=None)
def operands(shape, const=None):
    """Device operands of a shape, made once and never modified."""
    from latentblending_amd.hip import ops as o
    B, H, W, Cin, N, groups, _ = SHAPES[shape]
    x = stream_operand(B, H, W, Cin, seed=11, const=const)
    st, rows = channel_stats(x)
    w = rnd(N, Cin, 3, 3, seed=12, scale=(9 * Cin) ** -0.5)
    return dict(x=x, xd=x.to(DEV), st=st.to(DEV), rows=rows, w=w, wd=o.pack_conv_weight(w, Cin).to(DEV),
                gamma=(1.0 + 0.25 * rnd(Cin, seed=13, dtype=F32)).to(DEV), beta=(0.5 * rnd(Cin, seed=14, dtype=F32)).to(DEV),
                bias=(rnd(N, seed=15, dtype=F32) * 2.0 ** -4).to(DEV), res=(rnd(B * H * W, N, seed=16) * 2.0 ** -4).to(DEV))


# ---------------------------------------------------------------- bitwise, per conv
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_conv_equals_groupnorm_then_conv_bitwise(shape, gn_a_switch):
    B, H, W, Cin, N, groups, grid = SHAPES[shape]
    d = operands(shape)
    gn_a_switch(2, grid)
    fused, ref, _, _ = run_pair(d["xd"], d["wd"], d["gamma"], d["beta"], groups, True, d["st"], d["rows"], bias=d["bias"], alpha=2.0 ** -4)
    assert torch.isfinite(ref.float()).all()
    assert same_bits(fused, ref), f"{shape}: {int((fused != ref).sum())} of {ref.numel()} outputs differ"


@pytest.mark.parametrize("variant", ["residual", "silu_off", "ldx_padded", "groups_of_4", "groups_of_2"])
def test_fused_conv_bitwise_variants(variant, gn_a_switch):
    shape = {"groups_of_2": "b2_16x16_c64_n192"}.get(variant, "b2_16x32_c128_g1")
    B, H, W, Cin, N, groups, grid = SHAPES[shape]
    d = operands(shape)
    gn_a_switch(2, grid)
    kw, silu, xd, ldx, guard = dict(bias=d["bias"], alpha=2.0 ** -4), True, d["xd"], None, None
    if variant == "residual":
        kw["residual"] = d["res"]
    if variant == "silu_off":
        silu = False
    if variant == "ldx_padded":
        ldx = Cin + 24
        xd, guard = nhwc_dev(d["x"], ldx)
    if variant == "groups_of_4":
        assert Cin // groups == 4
    if variant == "groups_of_2":
        assert Cin // groups == 2
    fused, ref, _, _ = run_pair(xd, d["wd"], d["gamma"], d["beta"], groups, silu, d["st"], d["rows"], ldx=ldx, **kw)
    assert torch.isfinite(ref.float()).all()
    assert same_bits(fused, ref), f"{variant}: {int((fused != ref).sum())} of {ref.numel()} outputs differ"
    if guard is not None:
        guard.assert_intact("x (the flagged conv transforms its LDS copy, never the tensor)")
        assert torch.equal(xd.cpu(), d["x"])


@pytest.mark.parametrize("out_f32", [True, False])
def test_narrow_conv_equals_groupnorm_then_conv_bitwise(out_f32, gn_a_switch):
    from latentblending_amd.hip import ops as o
    B, H, W, Cin, _, groups, _ = SHAPES["b2_16x32_c128_g1"]
    d = operands("b2_16x32_c128_g1")
    w = torch.zeros(4, Cin, 3, 3, dtype=F16)
    w[:3] = rnd(3, Cin, 3, 3, seed=21, scale=(9 * Cin) ** -0.5)         # N 3 -> 4: the VAE's conv_out with its zero pad row
    wd, bias = o.pack_conv_weight(w, Cin).to(DEV), rnd(4, seed=22, dtype=F32).to(DEV)
    gn_a_switch(2, 0)
    fused, ref, _, _ = run_pair(d["xd"], wd, d["gamma"], d["beta"], groups, True, d["st"], d["rows"], entry="narrow", out_f32=out_f32,
                                bias=bias)
    assert torch.isfinite(ref.float()).all()
    assert same_bits(fused, ref), f"{int((fused != ref).sum())} of {ref.numel()} outputs differ"
    # and through the router, as the emitter launches it
    routed = torch.full_like(ref, float("nan"))
    table = o.groupnorm_affine_from_stats(d["gamma"], d["beta"], groups, EPS, d["st"], d["rows"], B, H * W)
    p = gn_params(conv_params(d["xd"], wd, routed, bias=bias, flags=lib().GEMM_OUT_F32 if out_f32 else 0), table, True)
    entry_of("gemm")(C.byref(p), stream())
    torch.cuda.synchronize()
    assert same_bits(routed, ref)


# ---------------------------------------------------------------- the operand itself, and the table
def test_operand_is_the_value_the_apply_pass_stores(gn_a_switch):
    """Identity weights on the centre tap: the flagged conv's fp32 output IS its fp16 A operand, pixel by pixel and channel by
    channel - bit for bit what lb_groupnorm_from_stats stores (so scale and shift are the pairs gn_apply_kernel folds: 2048 different
    x per (sample, channel) leave no room for another pair)."""
    from latentblending_amd.hip import ops as o
    B, H, W, Cin, _, groups, _ = SHAPES["b2_16x32_c128_g1"]
    d = operands("b2_16x32_c128_g1")
    w = torch.zeros(Cin, Cin, 3, 3, dtype=F16)
    w[torch.arange(Cin), torch.arange(Cin), 1, 1] = 1.0
    wd = o.pack_conv_weight(w, Cin).to(DEV)
    gn_a_switch(2, 1)
    for silu in (True, False):
        fused, _, n, _ = run_pair(d["xd"], wd, d["gamma"], d["beta"], groups, silu, d["st"], d["rows"], out_f32=True)
        assert same_bits(fused.to(F16), n.reshape(-1, Cin)) and torch.equal(fused, n.reshape(-1, Cin).float())


@functools.lru_cache(maxsize=None)
def reference64(shape, silu=True):
    """float64 GroupNorm (+ SiLU) of the fp16 tensor and what enters the bounds, once per shape."""
    B, H, W, Cin, N, groups, _ = SHAPES[shape]
    d = operands(shape)
    x64 = d["x"].double()
    g = x64.reshape(B, H * W, groups, Cin // groups)
    mean, ex2 = g.mean((1, 3), keepdim=True), (g * g).mean((1, 3), keepdim=True)
    var = ex2 - mean * mean
    assert bool((mean * mean <= var).all()), "the bounds below assume |mean| <= std in every group"
    rstd = 1.0 / torch.sqrt(var + EPS)
    gamma, beta = P.f64(d["gamma"]).reshape(1, 1, groups, -1), P.f64(d["beta"]).reshape(1, 1, groups, -1)
    sc = (rstd * gamma).expand(B, 1, groups, Cin // groups).reshape(B, 1, 1, Cin)
    sh = (beta - mean * rstd * gamma).expand(B, 1, groups, Cin // groups).reshape(B, 1, 1, Cin)
    t = x64 * sc + sh
    n = t * torch.sigmoid(t) if silu else t
    # Error of the computed fp32 pre-activation t = fma(x, sc, sh), derived (U = 2^-24; rms / std <= sqrt(2) from |mean| <= std):
    #   block sums are fp32 roundings of exact sums, folded in float64: |d mean| <= U rms, E[x^2] within U relative, so
    #   var = E[x^2] - mean^2 within 3 U E[x^2] <= 6 U var; rstd within 3 U, + its fp32 rounding: 4 U; sc = rstd * gamma: 5 U relative;
    #   fp32 mean within 2 U rms; |d(mean sc)| <= 2 U rms |sc| + 6 U |mean sc| <= (3 + 6) U |gamma|; sh one more rounding: U |sh|;
    #   the FMA itself U |t|.
    gam = P.f64(d["gamma"]).abs().reshape(1, 1, 1, Cin)
    pre = P.U32 * (5 * (x64 * sc).abs() + 9 * gam + sh.abs() + t.abs())
    # the fp16 operand: activation_bound (Lipschitz 1.13, exp / rcp, the fp16 store) - or the plain store without SiLU
    dn = P.activation_bound(pre, n) if silu else pre * (1 + P.U16) + P.store_bound(n)
    return dict(sc=sc.reshape(B, Cin), sh=sh.reshape(B, Cin), n=n, dn=dn, dsc=5 * P.U32 * sc.abs().reshape(B, Cin),
                dsh=(P.U32 * (9 * gam + sh.abs())).reshape(B, Cin))


def test_affine_table_against_float64_statistics(results_log):
    from latentblending_amd.hip import ops as o
    for shape in ("b2_16x32_c128_g1", "b2_16x16_c64_n192"):
        B, H, W, Cin, _, groups, _ = SHAPES[shape]
        d, r = operands(shape), reference64(shape)
        view, guard = guarded(B, 2 * Cin, 2 * Cin, F32, DEV, back_rows=0)
        o.groupnorm_affine_from_stats(d["gamma"], d["beta"], groups, EPS, d["st"], d["rows"], B, H * W, out=view)
        torch.cuda.synchronize()
        guard.assert_intact("affine table")
        guard.assert_fully_written("affine table")
        table = view.reshape(B, Cin, 2)
        P.check_elementwise(results_log, f"gn_a_table_scale_{shape}", table[..., 0], r["sc"], r["dsc"])
        P.check_elementwise(results_log, f"gn_a_table_shift_{shape}", table[..., 1], r["sh"], r["dsh"])


@pytest.mark.parametrize("kernel", ["halo", "narrow"])
def test_fused_conv_against_float64(kernel, results_log, gn_a_switch):
    """float64 GroupNorm + SiLU + conv2d of the fp16 tensor, element by element.  Bound = contraction_bound of the conv over the
    EXACT normalised operand n, plus what the operand's own error dn (reference64: statistics, affine map, SiLU, fp16 rounding)
    contributes: sum_k dn_k |w_k| exactly, and dn enters the accumulation bound through |n| + dn."""
    from latentblending_amd.hip import ops as o
    shape = "b2_16x32_c128_g1"
    B, H, W, Cin, N, groups, grid = SHAPES[shape]
    d, r = operands(shape), reference64(shape)
    if kernel == "narrow":
        w = torch.zeros(4, Cin, 3, 3, dtype=F16)
        w[:3] = rnd(3, Cin, 3, 3, seed=21, scale=(9 * Cin) ** -0.5)
        bias = rnd(4, seed=22, dtype=F32)
    else:
        w, bias = d["w"], d["bias"].cpu()
    wd = o.pack_conv_weight(w, Cin).to(DEV)
    gn_a_switch(2, grid)
    table = o.groupnorm_affine_from_stats(d["gamma"], d["beta"], groups, EPS, d["st"], d["rows"], B, H * W)
    got = torch.full((B * H * W, w.shape[0]), float("nan"), dtype=F16, device=DEV)
    entry_of(kernel)(C.byref(gn_params(conv_params(d["xd"], wd, got, bias=bias.to(DEV)), table, True)), stream())
    torch.cuda.synchronize()
    w64, nchw = w.double(), lambda t: t.permute(0, 3, 1, 2)
    ref = F.conv2d(nchw(r["n"]), w64, bias.double(), padding=1).permute(0, 2, 3, 1)
    operand_err = F.conv2d(nchw(r["dn"]), w64.abs(), None, padding=1).permute(0, 2, 3, 1)
    absdot = F.conv2d(nchw(r["n"].abs() + r["dn"]), w64.abs(), None, padding=1).permute(0, 2, 3, 1)
    bound = P.contraction_bound(None, None, 9 * Cin, ref, bias=bias.double(), absdot64=absdot) + operand_err * (1 + P.U16)
    P.check_elementwise(results_log, f"gn_a_fp64_{kernel}", got.reshape(B, H, W, -1), ref, bound)


# ---------------------------------------------------------------- memory contract
def test_memory_contract_and_zero_padding(gn_a_switch):
    """Guard bands round x (padded rows), the table, the weights and the output; a CONSTANT activation, whose GroupNorm is
    silu(beta) != 0 everywhere: a border piece that was transformed instead of staying zero changes every border output."""
    from latentblending_amd.hip import ops as o
    shape = "b2_16x32_c128_g1"
    B, H, W, Cin, N, groups, _ = SHAPES[shape]
    d = operands(shape, const=0.25)
    ldx = Cin + 8
    xd, x_guard = nhwc_dev(d["x"], ldx)
    wv, w_guard = guarded(N, 9 * Cin, 9 * Cin, F16, DEV, back_rows=0)
    wv.copy_(d["wd"])
    tv, t_guard = guarded(B, 2 * Cin, 2 * Cin, F32, DEV, back_rows=0)
    o.groupnorm_affine_from_stats(d["gamma"], d["beta"], groups, EPS, d["st"], d["rows"], B, H * W, out=tv)
    out, out_guard = guarded(B * H * W, N, N + 4, F16, DEV)
    for grid in (1, 2):
        gn_a_switch(2, grid)
        entry_of("halo")(C.byref(gn_params(conv_params(xd, wv, out, bias=d["bias"]), tv, True)), stream())
        torch.cuda.synchronize()
        for g, name in ((x_guard, "x"), (w_guard, "weights"), (t_guard, "table"), (out_guard, "output")):
            g.assert_intact(name)
        out_guard.assert_fully_written("output")
        n = o.groupnorm_from_stats(xd, d["gamma"], d["beta"], groups, EPS, True, d["st"], d["rows"], ldx=ldx,
                                   out=torch.empty(B, H, W, Cin, dtype=F16, device=DEV))
        ref = torch.empty(B * H * W, N, dtype=F16, device=DEV)
        entry_of("halo")(C.byref(conv_params(n, d["wd"], ref, bias=d["bias"])), stream())
        torch.cuda.synchronize()
        assert float(n.float().abs().min()) > 0, "the constant image must normalise to a non-zero value"
        assert same_bits(out.contiguous(), ref)
        # and against an independent zero-padded convolution of the normalised image (fp32 on the host)
        host = F.conv2d(n.cpu().float().permute(0, 3, 1, 2), d["w"].float(), d["bias"].cpu(), padding=1).permute(0, 2, 3, 1)
        P.check_close({}, f"gn_a_zero_padding_grid{grid}", out.reshape(B, H, W, N), host)


# ---------------------------------------------------------------- the VAE program
@functools.lru_cache(maxsize=None)
def _vae():
    import latentblending_amd.native as n
    return n.NativeVAEDecoder(n.VAEConfig(block_channels=(64, 128, 128, 128)), n.SyntheticProvider(5), DEV)


def test_vae_program_fold_on_equals_off(gn_a_switch):
    """B = 2, L = 16 decode (64- and 128-channel levels up to 128^2, every eligible conv on the halo kernel): identical uint8
    frames with the fold forced on and off - eager, as a graph replay and after re-recording - and the op lists as specified."""
    api = lib().api
    vae = _vae()
    z = rnd(2, 4, 16, 16, seed=31).to(DEV)
    api.lb_gemm_set_halo(2)
    try:
        gn_a_switch(0, 0)
        off = vae.build(2, 16)
        names_off = off.prog.op_names()
        off.z_in.copy_(z)
        off.prog.run()
        torch.cuda.synchronize()
        frames_off = off.frames.clone()
        assert "lb_groupnorm_affine_from_stats" not in names_off
        gn_a_switch(1, 0)
        api.lb_gemm_set_halo(1)
        default_route = vae.build(2, 16)
        api.lb_gemm_set_halo(2)
        gn_a_switch(2, 0)
        on = vae.build(2, 16)
        names_on = on.prog.op_names()
        n_tab = names_on.count("lb_groupnorm_affine_from_stats")
        assert n_tab >= 8 and names_on.count("lb_groupnorm_from_stats") == names_off.count("lb_groupnorm_from_stats") - n_tab
        for i, nm in enumerate(names_on):           # a table kernel feeds a conv (a shortcut GEMM may sit between); no apply pass before it
            if nm == "lb_groupnorm_affine_from_stats":
                nxt = [m for m in names_on[i + 1:i + 3] if m in ("lb_conv3x3_halo_f16", "lb_conv3x3_narrow_f16")]
                assert nxt, names_on[i:i + 3]
        assert names_on[-2] == "lb_conv3x3_narrow_f16" and names_on[-3] == "lb_groupnorm_affine_from_stats"
        # the table kernel stands exactly where the apply pass stood; nothing else moved
        assert ["lb_groupnorm_from_stats" if m == "lb_groupnorm_affine_from_stats" else m for m in names_on] == names_off
        # fold off: the GroupNorm launches of ever - one per GroupNorm of the decoder (two per resnet, mid attention, conv_norm_out)
        n_resnets = 2 + 3 * 4
        assert sum(m.startswith("lb_groupnorm_") for m in names_off) == 2 * n_resnets + 2
        on.z_in.copy_(z)
        on.prog.run()
        torch.cuda.synchronize()
        assert torch.equal(on.frames, frames_off), "eager run"
        on.frames.zero_()
        assert torch.equal(on.decode(z), frames_off), "program launch"
        on.prog.instantiate()
        on.frames.zero_()
        on.decode(z)
        torch.cuda.synchronize()
        assert torch.equal(on.frames, frames_off), "graph replay"
        again = vae.build(2, 16)                    # re-recorded under the same switch: the same ops, the same frames
        assert again.prog.op_names() == names_on
        again.prog.instantiate()
        again.decode(z)
        torch.cuda.synchronize()
        assert torch.equal(again.frames, frames_off), "replay after re-recording"
        # the default route (halo only where the grid fills the chip) with the default policy: same frames as its own fold-off build
        default_route.decode(z)
        torch.cuda.synchronize()
        gn_a_switch(0, 0)
        api.lb_gemm_set_halo(1)
        base = vae.build(2, 16)
        base.decode(z)
        torch.cuda.synchronize()
        assert torch.equal(default_route.frames, base.frames), "default route and policy"
    finally:
        api.lb_gemm_set_halo(1)
