"""Non-square renders on a real MI355X: the ragged-tile form of the 3x3 halo conv (LB_GEMM_HALO_RAGGED) and the (H, W) launch
programs built on it.

Kernel: against float64 ``F.conv2d``, bit for bit against the shipped kernel on a zero-padded copy, its memory contract, its
channel statistics, its routing and its recorded / replayed / graph launches.  Programs: the tiny UNet and a VAE decoder at
non-square latents against the CPU oracle, the whole branched transition at 192 x 128 against the oracle engine, the refusal
of a size the UNet's levels do not divide, and a device-encoded movie of the non-square run.

Bars: conv rel-L2 <= 2e-3 and max-abs <= 2^-8 max|ref| against float64; UNet forward rel-L2 <= 1e-2;
frames mean |du8| <= 2 and >= 99 % within +-4.
"""
import dataclasses
import os
import struct
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import pipe as OP  # noqa: E402  (checker only)
from oracle import sdxl_ref as R  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lcm_ref as LR  # noqa: E402
from _guard import guarded, poisoned  # noqa: E402
from _parity import check_close, rnd  # noqa: E402

DEV = "cuda"

# (B, H, W, Cin, Cout): ragged in x; ragged in y; both directions + two samples + ragged N; image smaller than one tile (samples closer
# than a tile); more work items than CUs (the persistent walk crosses ragged and whole tiles).  The last one is the only shape here
# whose cheaper tiling is 16 x 16 (3 x 2 tiles against 2 x 4 of 32 x 8): the second ragged instantiation.
SHAPES = [(1, 8, 40, 64, 64), (1, 12, 32, 64, 64), (2, 20, 24, 64, 132), (3, 5, 9, 128, 64), (9, 36, 68, 64, 256), (2, 30, 40, 64, 64)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]


def ops():
    from latentblending_amd.hip import ops as o
    return o


def lib():
    from latentblending_amd.hip import lib as l
    return l


def native():
    import latentblending_amd.native as n
    return n


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def ceil_div(a, b):
    return -(-a // b)


_CASES = {}


def case(shape):
    """Seeded operands of one shape and its float64 references (computed once, shared by the tests, never modified)."""
    if shape not in _CASES:
        B, H, W, Cin, Cout = shape
        seed = 1000 + 7 * SHAPES.index(shape)
        x = rnd(B, Cin, H, W, seed=seed)
        w = rnd(Cout, Cin, 3, 3, seed=seed + 1, scale=(9 * Cin) ** -0.5)
        bias = rnd(Cout, seed=seed + 2, dtype=torch.float32)
        res = rnd(B, H, W, Cout, seed=seed + 3)
        rowvec = rnd(B, Cout, seed=seed + 4)
        conv64 = F.conv2d(x.double(), w.double(), padding=1).permute(0, 2, 3, 1).contiguous()
        full64 = conv64 + bias.double() + rowvec.double()[:, None, None, :] + res.double()
        _CASES[shape] = dict(x=x, w=w, bias=bias, res=res, rowvec=rowvec, conv64=conv64, full64=full64,
                             xn=x.permute(0, 2, 3, 1).contiguous())
    return _CASES[shape]


def halo_conv(shape, c, full, ragged=True, **kw):
    """lb_conv3x3_halo_f16 called directly on device copies of the case's operands."""
    o, l = ops(), lib()
    B, H, W, Cin, Cout = shape
    xn = kw.pop("xn", None)
    xn = c["xn"].to(DEV) if xn is None else xn
    wp = o.pack_conv_weight(c["w"], Cin).to(DEV)
    extra = dict(bias=c["bias"].to(DEV), residual=kw.pop("residual", c["res"].to(DEV)), rowvec=c["rowvec"].to(DEV),
                 rows_per_batch=H * W) if full else {}
    return o.gemm(xn, wp, flags=l.GEMM_HALO_RAGGED if ragged else 0, splitk_ws=False,
                  conv=dict(KH=3, KW=3, stride=1, pad=1, halo=True), **extra, **kw)


def check_conv(log, name, got, ref64):
    """The conv bar: rel-L2 <= 2e-3 and max-abs <= 2^-8 max|ref| against float64."""
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape and torch.isfinite(got).all(), name
    err = (got - ref64).abs().max().item()
    rl2 = ((got - ref64).norm() / ref64.norm()).item()
    bound = 2.0 ** -8 * ref64.abs().max().item()
    log[name] = {"max_abs": err, "rel_l2": rl2, "bound_abs": bound}
    print(f"[parity] {name}: max_abs={err:.3e} (bound {bound:.3e}) rel_l2={rl2:.3e}")
    assert rl2 <= 2e-3, f"{name}: rel-L2 {rl2:.3e}"
    assert err <= bound, f"{name}: max-abs {err:.3e} > {bound:.3e}"


# ------------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("full", [True, False], ids=["bias_res_rowvec", "plain"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_ragged_conv_matches_float64(shape, full, results_log):
    c = case(shape)
    B, H, W, Cin, Cout = shape
    kind, tw, items, grid = ops().conv_halo_plan(B, H, W, Cin, Cout, flags=lib().GEMM_HALO_RAGGED)
    assert kind == 3 and items == B * ceil_div(H, 256 // tw) * ceil_div(W, tw) * ceil_div(Cout, 128)
    got = halo_conv(shape, c, full)
    check_conv(results_log, f"ragged_conv_{'x'.join(map(str, shape))}_{'full' if full else 'plain'}", got, c["full64"] if full else c["conv64"])


def test_persistent_walk_equals_one_item_per_block():
    """More items than CUs: the persistent blocks' request streams cross ragged and whole tiles; one item per block must give the same bits."""
    shape = SHAPES[4]
    c, l = case(shape), lib()
    _, _, items, grid = ops().conv_halo_plan(*shape, flags=l.GEMM_HALO_RAGGED)
    assert grid < items, "the case does not walk: every item has a block of its own"
    out = {}
    for full in (True, False):
        out[full] = halo_conv(shape, c, full)
    l.api.lb_conv_halo_set_persistent(0)
    try:
        for full in (True, False):
            assert torch.equal(halo_conv(shape, c, full), out[full])
    finally:
        l.api.lb_conv_halo_set_persistent(1)


# ------------------------------------------------------------------------------------------------ 2. bit identity
@pytest.mark.parametrize("full", [True, False], ids=["bias_res_rowvec", "plain"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_ragged_conv_is_the_shipped_kernel_on_a_zero_padded_image(shape, full):
    """Every sample zero-padded to the next size the shipped kernel takes WITH THE SAME TILE WIDTH, run without the flag: the
    zeros beyond the edge are what the ragged loader stages, so every valid pixel must come out with the same bits."""
    o, l = ops(), lib()
    c = case(shape)
    B, H, W, Cin, Cout = shape
    _, tw, _, _ = o.conv_halo_plan(B, H, W, Cin, Cout, flags=l.GEMM_HALO_RAGGED)
    th = 256 // tw
    Hp, Wp = ceil_div(H, th) * th, ceil_div(W, tw) * tw
    while o.conv_halo_plan(B, Hp, Wp, Cin, Cout)[:2] != (3, tw):        # (a 16-wide padding that 32 x 8 tiles divide as well)
        Wp += tw
    xp = torch.zeros(B, Hp, Wp, Cin, dtype=torch.float16)
    xp[:, :H, :W] = c["xn"]
    rp = torch.zeros(B, Hp, Wp, Cout, dtype=torch.float16)
    rp[:, :H, :W] = c["res"]
    wp = o.pack_conv_weight(c["w"], Cin).to(DEV)
    extra = dict(bias=c["bias"].to(DEV), residual=rp.to(DEV), rowvec=c["rowvec"].to(DEV), rows_per_batch=Hp * Wp) if full else {}
    padded = o.gemm(xp.to(DEV), wp, splitk_ws=False, conv=dict(KH=3, KW=3, stride=1, pad=1, halo=True), **extra)
    ragged = halo_conv(shape, c, full)
    assert torch.equal(ragged, padded[:, :H, :W]), f"{(ragged.float() - padded[:, :H, :W].float()).abs().max().item():.3e}"


# ------------------------------------------------------------------------------------------------ 3. memory contract
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_ragged_conv_memory_contract(shape, results_log):
    """NaN pad columns (ldx > Cin, ldc > Cout, ldr > Cout), NaN rows right behind the last sample of the input and of the residual,
    sentinel guards around the output; then every sample ALONE in a guarded buffer of its own rows, fed from the middle of the
    batch: a tile of a non-last sample that overhangs the image must not reach into the next sample's rows either."""
    o, l = ops(), lib()
    c = case(shape)
    B, H, W, Cin, Cout = shape
    nan = float("nan")
    M = B * H * W
    xin = poisoned(c["xn"].reshape(M, Cin), M, Cin, Cin + 8, nan, DEV).unflatten(0, (B, H, W))
    res = poisoned(c["res"].reshape(M, Cout), M, Cout, Cout + 4, nan, DEV).unflatten(0, (B, H, W))
    out, guard = guarded(M, Cout, Cout + 8, torch.float16, DEV)
    got = halo_conv(shape, c, True, xn=xin, residual=res, out=out.unflatten(0, (B, H, W)))
    guard.assert_intact("ragged conv output")
    guard.assert_fully_written("ragged conv output")
    check_conv(results_log, f"ragged_conv_guarded_{'x'.join(map(str, shape))}", got, c["full64"])
    whole = got.clone()
    if B == 1:
        return
    # sample b alone: its input is a view INTO the batch (the neighbours' pixels lie right before and behind it), its output a
    # guarded buffer of exactly H x W rows - what the batch run may write for sample b is what this run writes
    wp = o.pack_conv_weight(c["w"], Cin).to(DEV)
    for b in range(B):
        out1, guard1 = guarded(H * W, Cout, Cout + 8, torch.float16, DEV)
        o.gemm(xin[b:b + 1], wp, bias=c["bias"].to(DEV), residual=res[b:b + 1], rowvec=c["rowvec"][b:b + 1].to(DEV), rows_per_batch=H * W,
               flags=l.GEMM_HALO_RAGGED, splitk_ws=False, out=out1.unflatten(0, (1, H, W)), conv=dict(KH=3, KW=3, stride=1, pad=1, halo=True))
        guard1.assert_intact(f"sample {b}")
        guard1.assert_fully_written(f"sample {b}")
        assert torch.equal(out1.unflatten(0, (1, H, W))[0], whole[b])


# ------------------------------------------------------------------------------------------------ 4. channel statistics
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[4]], ids=[SHAPE_IDS[3], SHAPE_IDS[4]])
def test_ragged_conv_channel_statistics(shape, results_log):
    """Pixels outside the image contribute exactly 0 to both sums (unmasked they would add bias^2): the statistics match the
    stored tensor, and lb_groupnorm_from_stats on them matches the two-pass GroupNorm of the stored output (tolerances of
    test_conv_channel_stats_and_groupnorm_from_them)."""
    o, l = ops(), lib()
    c = case(shape)
    B, H, W, Cin, Cout = shape
    _, tw, items, _ = o.conv_halo_plan(B, H, W, Cin, Cout, flags=l.GEMM_HALO_RAGGED)
    l.api.lb_gemm_set_halo(2)
    try:
        rows = o.conv_ch_stat_rows(B, H, W, Cin, Cout, flags=l.GEMM_HALO_RAGGED)
        assert o.conv_ch_stat_rows(B, H, W, Cin, Cout) == 0             # (without the flag: not a halo launch)
    finally:
        l.api.lb_gemm_set_halo(1)
    assert rows == ceil_div(H, 256 // tw) * ceil_div(W, tw) * 4 == items // ceil_div(Cout, 128) // B * 4
    st = torch.full((Cout, B * rows, 2), float("nan"), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError):
        halo_conv(shape, c, True, ch_stats=st[:, :-1])
    y = halo_conv(shape, c, True, ch_stats=st)
    assert torch.equal(y, halo_conv(shape, c, True)), "the statistics epilogue must not change what the conv stores"
    assert torch.isfinite(st).all(), "every (row block, channel) slot must be written"
    yf = y.float().reshape(B, H * W, Cout)
    tot = st.reshape(Cout, B, rows, 2).double().sum(dim=2).permute(1, 0, 2).cpu()
    want_s, want_q = yf.double().sum(dim=1).cpu(), (yf.double() ** 2).sum(dim=1).cpu()
    assert torch.allclose(tot[..., 0], want_s, rtol=1e-4, atol=1e-2) and torch.allclose(tot[..., 1], want_q, rtol=1e-4, atol=1e-2)
    gamma, beta = (1 + 0.1 * rnd(Cout, seed=215, dtype=torch.float32)).to(DEV), (0.1 * rnd(Cout, seed=216, dtype=torch.float32)).to(DEV)
    got = o.groupnorm_from_stats(y, gamma, beta, 32, 1e-6, True, st, rows)
    two_pass = o.groupnorm_nhwc(y, gamma, beta, 32, 1e-6, True)
    ref = F.silu(F.group_norm(y.float().permute(0, 3, 1, 2), 32, gamma, beta, 1e-6)).permute(0, 2, 3, 1)
    check_close(results_log, f"groupnorm_from_ragged_conv_stats_{'x'.join(map(str, shape))}", got, ref)
    assert (got.float() - two_pass.float()).abs().max().item() <= 2e-3 * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------ 5. routing
def _gemm_plan(shape, flags):
    import ctypes as C
    l = lib()
    B, H, W, Cin, Cout = shape
    g = l.ConvGeom.conv3x3(H, W, Cin)
    p = l.gemm_params(M=g.M(B), N=Cout, K=g.K, ldw=g.K, ldc=Cout, conv=g, flags=flags, zero_page=64)
    t, sk, nb = C.c_int(), C.c_int(), C.c_long()
    l.api.lb_gemm_plan(C.byref(p), C.byref(t), C.byref(sk), C.byref(nb))
    return t.value, sk.value, nb.value


def test_routing_without_the_flag_stays_put():
    o, l = ops(), lib()
    for shape in SHAPES:
        assert o.conv_halo_plan(*shape)[0] == 0
        l.api.lb_gemm_set_halo(0)
        try:
            never = _gemm_plan(shape, 0)
        finally:
            l.api.lb_gemm_set_halo(2)
        try:
            assert _gemm_plan(shape, 0) == never and never[0] != 6      # unflagged: the implicit GEMM's own tile, as with the halo route off
            code, _, blocks = _gemm_plan(shape, l.GEMM_HALO_RAGGED)
            assert code == 6 and blocks == o.conv_halo_plan(*shape, flags=l.GEMM_HALO_RAGGED)[2]
        finally:
            l.api.lb_gemm_set_halo(1)
    # a shape that divides: the flag changes neither the plan nor a bit of the result
    even = (2, 16, 32, 64, 64)
    assert o.conv_halo_plan(*even) == o.conv_halo_plan(*even, flags=l.GEMM_HALO_RAGGED) and o.conv_halo_plan(*even)[0] == 3
    x, w = rnd(2, 16, 32, 64, seed=31).to(DEV), o.pack_conv_weight(rnd(64, 64, 3, 3, seed=32, scale=1 / 24.0), 64).to(DEV)
    b = rnd(64, seed=33, dtype=torch.float32).to(DEV)
    outs = [o.gemm(x, w, bias=b, flags=f, splitk_ws=False, conv=dict(KH=3, KW=3, stride=1, pad=1, halo=True)) for f in (0, l.GEMM_HALO_RAGGED)]
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ 6. program replay
def test_ragged_conv_recorded_replayed_and_graph_launched():
    """Two chained ragged convs (the second reads the first's output) recorded into a Program: eager replay, a run_range split
    and instantiate + launch each reproduce the direct calls bit for bit."""
    from latentblending_amd.native.runtime import Program
    o, l = ops(), lib()
    shape = SHAPES[2]
    B, H, W, Cin, Cout = shape
    c = case(shape)
    xn, wp = c["xn"].to(DEV), o.pack_conv_weight(c["w"], Cin).to(DEV)
    w2 = o.pack_conv_weight(rnd(64, 136, 3, 3, seed=77, scale=(9 * 132) ** -0.5)[:, :Cout], Cout)
    w2p = torch.zeros(64, 9, 192, dtype=torch.float16)                  # second conv: Cin padded to 192 (a multiple of 64), ldx = 192
    w2p[:, :, :Cout] = w2.reshape(64, 9, Cout)
    w2p = w2p.reshape(64, 9 * 192).to(DEV)
    bias, res, rv = c["bias"].to(DEV), c["res"].to(DEV), c["rowvec"].to(DEV)

    def emit(mid, out):
        o.gemm(xn, wp, bias=bias, residual=res, rowvec=rv, rows_per_batch=H * W, flags=l.GEMM_HALO_RAGGED, splitk_ws=False,
               out=mid[..., :Cout], conv=dict(KH=3, KW=3, stride=1, pad=1, halo=True))
        o.gemm(mid, w2p, flags=l.GEMM_HALO_RAGGED, splitk_ws=False, out=out, conv=dict(KH=3, KW=3, stride=1, pad=1, halo=True))
    mid_d, out_d = torch.zeros(B, H, W, 192, dtype=torch.float16, device=DEV), torch.empty(B, H, W, 64, dtype=torch.float16, device=DEV)
    emit(mid_d, out_d)
    want_mid, want = mid_d.clone(), out_d.clone()
    mid, out = torch.zeros_like(mid_d), torch.empty_like(out_d)
    prog = Program("ragged-convs")
    with prog.record():
        emit(mid, out)
    assert prog.op_names() == ["lb_conv3x3_halo_f16", "lb_conv3x3_halo_f16"]
    stream = torch.cuda.current_stream().cuda_stream

    def fresh():
        mid.zero_()
        out.fill_(float("nan"))
    fresh(); prog.run(stream)
    assert torch.equal(mid, want_mid) and torch.equal(out, want)
    fresh(); prog.run_range(0, 1, stream)
    assert torch.equal(mid, want_mid)
    prog.run_range(1, 2, stream)
    assert torch.equal(out, want)
    fresh(); prog.instantiate(); prog.launch(stream)
    assert torch.equal(mid, want_mid) and torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ 7. UNet
def test_unet_nonsquare_matches_oracle(results_log):
    """Tiny UNet (64, 128, 256 channels) at latent 24 x 72, B = 2: levels 24 x 72, 12 x 36 and 6 x 18, none of which divides
    into halo tiles.  With ragged_halo the step program runs lb_conv3x3_halo_f16 launches the ragged_halo=False program has not;
    both meet the bar, graph replay equals eager replay."""
    n, l = native(), lib()
    cfg = R.tiny_unet_cfg()
    w = R.make_weights(R.unet_spec(cfg), 0)
    net = n.NativeUNet(n.UNetConfig(**dataclasses.asdict(cfg)), n.SyntheticProvider(0), DEV)
    B, H, W = 2, 24, 72
    g = torch.Generator().manual_seed(2472)
    x = torch.randn(B, 4, H, W, generator=g).half()
    ctx = torch.randn(B, 77, cfg.cross_dim, generator=g).half()
    te = torch.randn(B, cfg.pooled_dim, generator=g).half()
    ids = torch.tensor([[128.0, 128.0, 0.0, 0.0, 128.0, 128.0]] * B)
    ref = R.unet_forward(cfg, w, x, torch.tensor(499.0), ctx, te, ids)
    l.api.lb_gemm_set_halo(2)          # (18 halo blocks at this size: the router's chip-filling threshold would keep them off the kernel)
    try:
        progs = {flag: net.build(B, (H, W), ragged_halo=flag) for flag in (True, False)}
    finally:
        l.api.lb_gemm_set_halo(1)
    got = {}
    for flag, prog in progs.items():
        assert (prog.H, prog.W, prog.L) == (H, W, None) and prog.ragged_halo == flag
        prog.set_conditioning(ctx.to(DEV), te.to(DEV), ids.to(DEV))
        got[flag] = prog.forward(x.to(DEV), torch.full((B,), 499.0)).clone()
        r = rel_l2(got[flag], ref)
        results_log[f"unet_tiny_B{B}_{H}x{W}_ragged{int(flag)}_rel_l2"] = r
        print(f"[parity] unet tiny B={B} {H}x{W} ragged_halo={flag}: rel_l2={r:.3e} ops={prog.prog_step.num_ops}")
        assert got[flag].shape == (B, 4, H, W) and torch.isfinite(got[flag]).all() and r <= 1e-2
        prog.enable_graphs()
        assert torch.equal(prog.forward(x.to(DEV), torch.full((B,), 499.0)), got[flag])
    names = {flag: progs[flag].prog_step.op_names() for flag in progs}
    assert names[True].count("lb_conv3x3_halo_f16") > 0 and names[False].count("lb_conv3x3_halo_f16") == 0
    assert len(names[True]) == len(names[False])
    results_log[f"unet_tiny_B{B}_{H}x{W}_ragged_vs_gemm_rel_l2"] = rel_l2(got[True], got[False])          # (logged, not gated)


# ------------------------------------------------------------------------------------------------ 8. VAE
def test_vae_nonsquare_matches_oracle(results_log):
    """VAE decoder at (64, 128, 256, 256) channels, B = 2, latent 12 x 20 -> frames 96 x 160."""
    n, l = native(), lib()
    cfg = R.VAECfg(block_channels=(64, 128, 256, 256))
    w = R.make_weights(R.vae_decoder_spec(cfg), 1)
    net = n.NativeVAEDecoder(n.VAEConfig(**dataclasses.asdict(cfg)), n.SyntheticProvider(1), DEV)
    z = torch.randn(2, 4, 12, 20, generator=torch.Generator().manual_seed(1220)).half()
    ref_img = R.vae_decode(cfg, w, z.float() / cfg.scaling_factor)
    ref_u8 = R.postprocess_u8(ref_img)
    l.api.lb_gemm_set_halo(2)
    try:
        prog = net.build(2, (12, 20))
    finally:
        l.api.lb_gemm_set_halo(1)
    assert (prog.H, prog.W, prog.L) == (12, 20, None) and "lb_conv3x3_halo_f16" in prog.prog.op_names()
    got_u8 = prog.decode(z.to(DEV)).cpu().numpy()
    assert got_u8.shape == (2, 96, 160, 3)
    d = np.abs(got_u8.astype(np.int32) - ref_u8.astype(np.int32))
    results_log["vae_12x20"] = {"mean_abs_u8": float(d.mean()), "frac_within_4": float((d <= 4).mean())}
    print(f"[parity] vae 12x20: mean|du8|={d.mean():.3f} within4={(d <= 4).mean():.4f}")
    assert d.mean() <= 2 and (d <= 4).mean() >= 0.99
    prog.prog.instantiate()
    assert np.array_equal(prog.decode(z.to(DEV)).cpu().numpy(), got_u8)


# ------------------------------------------------------------------------------------------------ 9. whole transition, 11. movie
SEEDS = [1000, 1001]


def _transition(frontier, scheduler, results_log, key):
    from latentblending_amd import BlendingEngine
    from latentblending_amd.backend import set_backend
    n = native()
    ucfg, vcfg = R.tiny_unet_cfg(), R.tiny_vae_cfg()
    o = OP.StableDiffusionXLPipeline(turbo=True, unet_cfg=ucfg, vae_cfg=vcfg, seed=0)
    if scheduler == "lcm":
        o.scheduler = LR.LCMRefScheduler(noise_source=o.noise)
    p = n.NativeSDXLPipe(turbo=True, unet_cfg=n.UNetConfig(**dataclasses.asdict(ucfg)), vae_cfg=n.VAEConfig(**dataclasses.asdict(vcfg)),
                         seed=0, scheduler=scheduler)
    tape = OP.NoiseTape(12345)
    p.scheduler.noise_source = tape
    np.random.seed(0)
    set_backend(R.TorchCpuBackend())
    be_o = BlendingEngine(o, metric=R.OracleLPIPS(7), verbose=False, frontier_width=frontier)
    set_backend(None)
    be_p = BlendingEngine(p, verbose=False, frontier_width=frontier)
    for be in (be_o, be_p):
        be.set_dimensions((192, 128))
        be.set_num_inference_steps(4)
        be.set_branching(nmb_max_branches=5)
        be.set_prompt1("photo of a reef")
        be.set_prompt2("rendering of an alien planet")
    set_backend(R.TorchCpuBackend())
    threads = torch.get_num_threads()
    torch.set_num_threads(min(os.cpu_count() or 1, 8))
    try:
        o.noise.reset()
        imgs_o = be_o.run_transition(fixed_seeds=SEEDS)
    finally:
        torch.set_num_threads(threads)
        set_backend(None)
    tape.reset()
    imgs_p = be_p.run_transition(fixed_seeds=SEEDS)
    # (the engine's warm-up leaves square programs of its default size behind; the transition's own are keyed (B, H, W) in latent pixels)
    for cache in (p._unet_programs, p._vae_programs):
        assert any(k[1:] == (16, 24) for k in cache) and all(len(k) == 2 or k[1:] == (16, 24) for k in cache), list(cache)
    assert len(imgs_o) == len(imgs_p) and np.asarray(imgs_p[0]).shape == (128, 192, 3)
    assert be_o.tree_fracts == be_p.tree_fracts and be_o.tree_idx_injection == be_p.tree_idx_injection, (be_o.tree_fracts, be_p.tree_fracts)
    d = np.stack([np.abs(np.asarray(a).astype(np.int32) - np.asarray(b).astype(np.int32)) for a, b in zip(imgs_p, imgs_o)])
    results_log[key] = {"frames": len(imgs_p), "mean_abs_u8": float(d.mean()), "frac_within_4": float((d <= 4).mean()), "same_tree": True,
                        "fracts": be_p.tree_fracts}
    print(f"[parity] {key}: frames={len(imgs_p)} mean|du8|={d.mean():.3f} within4={(d <= 4).mean():.4f} fracts={be_p.tree_fracts}")
    assert d.mean() <= 2 and (d <= 4).mean() >= 0.99
    return be_p, imgs_p


@pytest.mark.parametrize("frontier", [1, 4])
def test_transition_192x128_matches_oracle(frontier, results_log, tmp_path):
    """The whole branched transition at 192 x 128 (latent 16 x 24), Turbo, 4 steps, 5 branches: same tree as the engine on the
    CPU oracle pipe at the same frontier, frames within the bar.
    Seeds 1000 / 1001, chosen on the CPU with the oracle engine alone so that every greedy choice of the oracle (the tree's
    widest gap against its runner-up, (widest - runner-up) / widest, whenever two or more gaps are scored) is at least 5 % clear:
    margins 12.8 %, 61.6 %, 9.0 %, 8.5 % at frontier 1 and the same at frontier 4 (seeds 420 / 421 had 2.5 %, 67 %, 2.3 %, 0.3 %).
    At frontier 4 the run is also written as a device-encoded movie: the AVI header must report 192 x 128."""
    be, imgs = _transition(frontier, None, results_log, f"transition_192x128_frontier{frontier}")
    if frontier == 4:
        path = str(tmp_path / "nonsquare.avi")
        be.write_movie_transition(path, duration_transition=1.0, fps=8, encoder="device")
        with open(path, "rb") as fh:
            head = fh.read(4096)
        assert head[:4] == b"RIFF" and head[8:12] == b"AVI "
        at = head.index(b"avih")
        width, height = struct.unpack("<II", head[at + 8 + 32:at + 8 + 40])      # MainAVIHeader.dwWidth / dwHeight
        assert (width, height) == (192, 128)


def test_transition_192x128_lcm_matches_oracle(results_log):
    """The same transition under ``scheduler="lcm"`` at frontier 4.  Oracle margins of seeds 1000 / 1001 under this sampler (measured as above):
    14.8 %, 60.6 %, 8.5 %, 10.4 %."""
    _transition(4, "lcm", results_log, "transition_192x128_lcm_frontier4")


def test_recycled_anchor_dead_step_elision_and_ddim_at_192x128():
    """The rest of the native path at a non-square size, native pipe only: a chained transition (swap_forward + recycle_img1)
    through the fused wavefront with a known anchor, the same chain with ``elide_dead_steps`` (bit-identical frames from fewer
    UNet samples), and one transition under the DDIM sampler."""
    from latentblending_amd import BlendingEngine
    from latentblending_amd.backend import set_backend
    n = native()
    set_backend(None)
    cfgs = dict(unet_cfg=n.UNetConfig(**dataclasses.asdict(R.tiny_unet_cfg())), vae_cfg=n.VAEConfig(**dataclasses.asdict(R.tiny_vae_cfg())))
    p = n.NativeSDXLPipe(turbo=True, seed=0, allow_synthetic=True, **cfgs)
    tape = OP.NoiseTape(12345)
    p.scheduler.noise_source = tape

    def chain(elide):
        np.random.seed(0)
        be = BlendingEngine(p, verbose=False, frontier_width=4)
        be.elide_dead_steps = elide
        be.set_dimensions((192, 128))
        be.set_branching(nmb_max_branches=5)
        be.set_prompt1("photo of a reef")
        be.set_prompt2("rendering of an alien planet")
        tape.reset()
        p.stats["unet_samples"] = 0
        first = [np.asarray(f) for f in be.run_transition(fixed_seeds=SEEDS)]
        be.swap_forward()
        be.set_prompt2("a forest in the fog")
        second = [np.asarray(f) for f in be.run_transition(recycle_img1=True, fixed_seeds=[SEEDS[1], 999])]
        return first, second, p.stats["unet_samples"]
    first, second, samples = chain(False)
    assert all(f.shape == (128, 192, 3) for f in first + second) and np.array_equal(second[0], first[-1])
    first_e, second_e, samples_e = chain(True)
    assert samples_e < samples, "no step was dead: the case proves nothing"
    assert all(np.array_equal(a, b) for a, b in zip(first + second, first_e + second_e))
    d = n.NativeSDXLPipe(turbo=True, seed=0, allow_synthetic=True, scheduler="ddim", unet_native=p.unet_native, vae_native=p.vae_native)
    be = BlendingEngine(d, verbose=False, frontier_width=4)
    be.set_dimensions((192, 128))
    be.set_branching(nmb_max_branches=3)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    frames = [np.asarray(f) for f in be.run_transition(fixed_seeds=SEEDS)]
    assert all(f.shape == (128, 192, 3) for f in frames) and any(k[1:] == (16, 24) for k in d._unet_programs)


# ------------------------------------------------------------------------------------------------ 10. invalid size
def test_invalid_latent_size_is_refused_with_the_nearest_valid_sizes():
    n = native()
    p = n.NativeSDXLPipe(turbo=True, unet_cfg=n.UNetConfig(**dataclasses.asdict(R.tiny_unet_cfg())),
                         vae_cfg=n.VAEConfig(**dataclasses.asdict(R.tiny_vae_cfg())), seed=0, allow_synthetic=True)
    with pytest.raises(ValueError) as e:
        p.unet_program(1, (16, 26))                 # three levels: sides must be multiples of 4
    assert "16 x 24" in str(e.value) and "16 x 28" in str(e.value)
    with pytest.raises(ValueError) as e:
        p.unet_program(1, 18)
    assert "16 x 16" in str(e.value) and "20 x 20" in str(e.value)
    assert not p._unet_programs, "a refused size must not leave a program behind"
