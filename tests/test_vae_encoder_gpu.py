"""The native SDXL VAE encoder on a real MI355X.

1. *Far-edge gather*: ``lb_gemm_f16`` on ``ConvGeom.down3x3`` - stride 2, pad 0, the last output row and column one pixel past the
   image - in both implicit-GEMM families, on every tile ``lb_gemm_set_tuning`` can force for a conv, unsplit and split-K, against
   float64 ``conv2d(F.pad(x, (0, 1, 0, 1)), stride=2)`` per element under the bound tests/test_gemm_epilogue_matrix_gpu.py holds
   implicit convs to.  The samples lie back to back, sample b + 1 opens with a row of values around 1e3 and NaNs follow the last
   sample: a missing bottom mask is a wrong or non-finite last row.
2. *Units against float64*, teacher-forced, ``compare`` with FACTOR = 4 (tests/_model_units.py), after a census of the routes.
3. *Free-running taps and latents* against the float64 forward; 4. *full width*; 5. *the overflow regime* of the residual stream;
6. *lifetimes* (journal, NaN-poisoned replay) and eager = hipGraph; 7. *pipe-level equalities*; 8. *engine and replay*.
"""
import ctypes as C
import dataclasses
import functools
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _gemm_epilogue_model as E  # noqa: E402
import _model_units as MU  # noqa: E402
import _vae_encoder_ref as ER  # noqa: E402
from _parity import check_elementwise, rnd  # noqa: E402
from _value_kinds import gemm_mode  # noqa: E402
from oracle import sdxl_ref as R  # noqa: E402

DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
VAE_CH = (64, 128, 128, 128)
GEMM, HALO, NARROW = "lb_gemm_f16", "lb_conv3x3_halo_f16", "lb_conv3x3_narrow_f16"
GN, GN_STATS, GN_TABLE = "lb_groupnorm_nhwc", "lb_groupnorm_from_stats", "lb_groupnorm_affine_from_stats"
SOFTMAX, ATTN512 = "lb_softmax_rows_f16", "lb_attn_fwd_d512"


def native():
    import latentblending_amd.native as n
    return n


def lib():
    from latentblending_amd.hip import lib as l
    return l


def ops():
    from latentblending_amd.hip import ops as o
    return o


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def to_cpu_nchw(t):
    t = t.detach().cpu()
    return MU.nchw(t).contiguous() if t.dim() == 4 else t


def pictures(B, H, W, seed):
    return torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ====================================================================== 1. the far-edge gather
# (B, H, W, Cin, N, ldx): the issue's three shapes, and the second once more with pixels 8 elements further apart
EDGE_SHAPES = [(2, 8, 8, 64, 64, 64), (2, 6, 10, 128, 128, 128), (3, 16, 32, 256, 256, 256), (2, 6, 10, 128, 128, 136)]
EDGE_TILES = E.UNSPLIT + E.SPLIT          # (variant, tile, splitk): everything the matrix forces; what cannot take a conv is listed


@functools.lru_cache(maxsize=None)
def edge_case(B, H, W, cin, n, ldx):
    """Operands, the float64 reference and |x| * |w| of one shape: computed once, never modified.  The first row of every sample but
    the first holds values around 1e3: the row a missing bottom mask would read for the sample before it.  With ``ldx > cin`` the
    pad elements behind every pixel are NaN, and the first COLUMN of every row is large as well: pixel (y, W) is pixel (y + 1, 0), what
    a missing right mask would read."""
    seed = 900 + H * W + cin
    x = rnd(B, H, W, cin, seed=seed)
    x[1:, 0] = (x[1:, 0].float() * 1e3).to(F16)
    if ldx > cin:
        x[:, :, 0] = (x[:, :, 0].float().clamp(-30, 30) * 1e3).to(F16)
    w = rnd(n, cin, 3, 3, seed=seed + 1, scale=(9 * cin) ** -0.5)
    bias = rnd(n, seed=seed + 2, dtype=F32)
    x64 = x.double().permute(0, 3, 1, 2)
    pad = lambda t: F.pad(t, (0, 1, 0, 1))      # noqa: E731
    ref = (F.conv2d(pad(x64), w.double(), stride=2) + bias.double()[None, :, None, None]).permute(0, 2, 3, 1).contiguous()
    ad = F.conv2d(pad(x64.abs()), w.double().abs(), stride=2).permute(0, 2, 3, 1).contiguous()
    assert tuple(ref.shape) == (B, H // 2, W // 2, n)
    buf = torch.full((B * H * W + 4 * W + 64, ldx), float("nan"), dtype=F16)      # NaNs behind the last sample (and in the pad elements)
    buf[:B * H * W, :cin] = x.reshape(-1, cin)
    return dict(x=buf.to(DEV), w=ops().pack_conv_weight(w, cin).to(DEV), bias=bias.to(DEV), ref=ref, ad=ad,
                bound=E.contraction_bound(None, None, 9 * cin, ref, bias=bias, absdot64=ad))


@pytest.mark.parametrize("B,H,W,cin,n,ldx", EDGE_SHAPES)
def test_far_edge_gather_on_every_tile(B, H, W, cin, n, ldx, results_log):
    l = lib()
    c = edge_case(B, H, W, cin, n, ldx)
    g = l.ConvGeom.down3x3(H, W, cin, ldx=ldx)
    assert (g.stride, g.pad, g.Hout, g.Wout, g.ldx) == (2, 0, H // 2, W // 2, ldx)
    ws = torch.full((l.api.lb_gemm_workspace_bytes(g.M(B), n) // 4,), float("nan"), dtype=F32, device=DEV)
    k_tiles = (g.K + 63) // 64
    failed, ran, refused = [], [], []
    for variant, tile, splitk in EDGE_TILES:
        out = torch.full((g.M(B), n), float("nan"), dtype=F16, device=DEV)
        p = l.gemm_params(A=c["x"].data_ptr(), W=c["w"].data_ptr(), C=out.data_ptr(), M=g.M(B), N=n, K=g.K, ldw=c["w"].stride(0), ldc=n,
                          conv=g, bias=c["bias"].data_ptr(), partial=ws.data_ptr(), zero_page=ops().zero_page(c["x"].device).data_ptr())
        with gemm_mode(variant, tile, splitk):
            t, sk = C.c_int(), C.c_int()
            l.api.lb_gemm_plan(C.byref(p), C.byref(t), C.byref(sk), None)
            assert l.conv_plan(p).route == l.ROUTE_GEMM
            if t.value != tile:             # lb_gemm_plan's own word that the forced tile does not take this conv: listed, not skipped
                refused.append((variant, tile, splitk, t.value))
                continue
            assert sk.value == min(splitk, k_tiles), (variant, tile, splitk, sk.value)
            l.api.lb_gemm_f16(C.byref(p), ops().stream_ptr())
        got = out.cpu().view(B, H // 2, W // 2, n)
        name = f"vae_enc_edge_B{B}_{H}x{W}_c{cin}_ldx{ldx}_v{variant}_t{tile}_sk{splitk}"
        ran.append((variant, tile, splitk))
        if not bool(torch.isfinite(got).all()):
            failed.append(f"{name}: non-finite output (rows {sorted(set(torch.nonzero(~torch.isfinite(got))[:, 1].tolist()))} of the maps)")
            continue
        try:
            check_elementwise(results_log, name, got, c["ref"], c["bound"])
        except AssertionError as e:
            failed.append(str(e))
    print(f"[vae-encoder] far edge B{B} {H}x{W} c{cin} ldx{ldx}: ran {ran}; lb_gemm_plan refuses the forced tile for (variant, tile, "
          f"splitk, planned instead) {refused}")
    results_log[f"vae_enc_edge_B{B}_{H}x{W}_c{cin}_ldx{ldx}_refused"] = refused
    assert not failed, "\n".join(failed)
    # both families, unsplit and split, did run; and what was refused is the ping-pong tile (a plain-GEMM kernel) and nothing else
    assert {v for v, _, _ in ran} == {0, 1} and any(s > 1 for _, _, s in ran) and any(s == 1 for _, _, s in ran)
    assert all(tile == 9 for _, tile, _, _ in refused), refused


# ====================================================================== 2. units against float64
ENC_CASES = {
    "enc_B3_128_scaled": dict(B=3, L=16, halo=1, kw=dict(stream_fp16_scaled=True), have=(GEMM, HALO, NARROW, GN, GN_STATS, SOFTMAX), lack=(ATTN512,)),
    "enc_B3_128_f32": dict(B=3, L=16, halo=1, kw=dict(stream_fp16_scaled=False), have=(GEMM, HALO, NARROW, GN, GN_STATS, SOFTMAX), lack=(GN_TABLE, ATTN512)),
    "enc_B2_128_halo2": dict(B=2, L=16, halo=2, kw={}, have=(GEMM, HALO, NARROW, GN, GN_STATS, GN_TABLE, SOFTMAX), lack=(ATTN512,)),
    "enc_top512_B2_128_halo2": dict(B=2, L=16, halo=2, ch=(64, 128, 128, 512), kw={}, have=(GEMM, HALO, NARROW, GN, GN_STATS, GN_TABLE, ATTN512), lack=(SOFTMAX,)),
    # 96 x 160 pictures: maps of 96 x 160, 48 x 80, 24 x 40 and 12 x 20 - ragged halo tiles, non-square downsamplers; the 12 x 20 map
    # is no multiple of 16, so the moments conv is an implicit GEMM here
    "enc_B2_96x160_halo2": dict(B=2, L=(12, 20), halo=2, kw={}, have=(GEMM, HALO, GN, GN_STATS, SOFTMAX), lack=(NARROW, ATTN512)),
}


def enc_cfg(case):
    return R.VAECfg(block_channels=ENC_CASES[case].get("ch", VAE_CH))


def build_case(cfg, kw, B, L, halo, w=None, seed=None):
    """Build (journal on), encode once, capture: everything the tests of one case share."""
    n = native()
    provider = n.SyntheticProvider(1) if w is None else n.DictProvider(w)
    w = R.make_weights(ER.encoder_spec(cfg), 1) if w is None else w
    net = n.NativeVAEEncoder(n.VAEConfig(**dataclasses.asdict(cfg), **kw), provider, DEV)
    H, W = (L, L) if isinstance(L, int) else L
    u8 = pictures(B, 8 * H, 8 * W, B * 1000 + 8 * H if seed is None else seed)
    lib().api.lb_gemm_set_halo(halo)
    try:
        prog = net.build(B, L, journal=True)
    finally:
        lib().api.lb_gemm_set_halo(1)
    latents = prog.encode(u8.to(DEV)).clone()
    moments = prog.moments().clone()
    x_in = prog.x_in.clone()
    taps = {k: to_cpu_nchw(v) for k, v in prog.capture().items()}
    torch.cuda.synchronize()
    ref, model = MU.evs(w)
    return types.SimpleNamespace(cfg=cfg, prog=prog, net=net, u8=u8, latents=latents, moments=moments, x_in=x_in, taps=taps,
                                 latents_after_capture=prog.latents.clone(), moments_after_capture=prog.moments().clone(),
                                 inputs=dict(x_in=ER.picture(u8)), ref=ref, model=model, w=w,
                                 scaled=bool(kw.get("stream_fp16_scaled", True)), one=ATTN512 in prog.prog.op_names())


@functools.lru_cache(maxsize=None)
def enc_case(case):
    c = ENC_CASES[case]
    s = build_case(enc_cfg(case), c["kw"], c["B"], c["L"], c["halo"])
    s.case, s.c = case, c
    return s


@pytest.mark.parametrize("case", list(ENC_CASES))
def test_routes_marks_and_capture(case):
    s = enc_case(case)
    l = lib()
    names = s.prog.prog.op_names()
    for op in s.c["have"]:
        assert op in names, f"{op} was not recorded: the case does not reach the route it exists for"
    for op in s.c["lack"]:
        assert op not in names, f"{op} was recorded where the case exists for its absence"
    assert names[-2:] == ["lb_cast_f32_to_f16", "lb_nhwc_to_nchw_f16"]
    assert [(m.name, m.kind, m.inputs) for m in s.prog.marks] == ER.encoder_units(s.cfg)
    assert s.prog.tap_names == ER.encoder_tap_names(s.cfg)
    MU.check_marks(s.prog.marks, {s.prog.prog.name: s.prog.prog}, ("x_in",))
    assert s.prog.marks[-1].op_end == s.prog.prog.num_ops - 2 and s.prog.marks[-1].out is s.prog.moments_f32
    # the downsamplers: lb_conv_plan sends each to the implicit GEMM (under the switch the case was built with), and the unit each is
    # consists of that one launch (and the cast of an fp32 stream in front of it)
    B, (H, W) = s.c["B"], (s.prog.SH, s.prog.SW)
    by = {m.name: i for i, m in enumerate(s.prog.marks)}
    l.api.lb_gemm_set_halo(s.c["halo"])
    try:
        for bi, c in enumerate(s.cfg.block_channels[:-1]):
            g = l.ConvGeom.down3x3(H, W, c)
            plan = l.conv_plan(l.gemm_params(M=g.M(B), N=c, K=g.K, ldw=g.K, ldc=c, conv=g, flags=0 if s.scaled else l.GEMM_OUT_F32, zero_page=64))
            assert plan.route == l.ROUTE_GEMM and plan.stat_rows == 0
            i = by[f"encoder.down_blocks.{bi}.downsamplers.0.conv"]
            unit_ops = names[s.prog.marks[i - 1].op_end:s.prog.marks[i].op_end]
            assert unit_ops == ([] if s.scaled else ["lb_cast_f32_to_f16"]) + [GEMM], unit_ops
            # ... no statistics: the GroupNorm behind it is the two-pass launch
            assert names[s.prog.marks[i].op_end] == GN
            assert tuple(s.prog.marks[i].out.shape) == (B, H // 2, W // 2, c)
            H, W = H // 2, W // 2
    finally:
        l.api.lb_gemm_set_halo(1)
    assert (H, W) == (s.prog.H, s.prog.W)
    if s.c["halo"] == 1:        # the journal changes no op
        assert s.net.build(B, s.c["L"]).prog.op_names() == names
    assert s.prog.ragged_halo == (s.prog.H != s.prog.W)
    # a capture is a replay: it leaves the outputs as the launch did, and its last tap is the moments
    assert torch.equal(s.latents_after_capture, s.latents) and torch.equal(s.moments_after_capture, s.moments)
    assert torch.equal(s.taps["moments"], MU.nchw(s.moments.cpu()))
    assert set(s.taps) == {m.name for m in s.prog.marks} | set(s.prog.tap_names)
    assert all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in s.taps.values())
    # the staged picture: f16(fp32(u8) / 127.5 - 1) in three of eight channels, zeros in the rest
    assert torch.equal(MU.nchw(s.x_in[..., :3].cpu()), s.inputs["x_in"]) and not bool(s.x_in[..., 3:].any())
    # latents = fp16(mean * scaling_factor), one multiply in fp32 and one rounding, NCHW
    want = (s.moments[..., :4] * torch.tensor(s.cfg.scaling_factor, dtype=F32)).to(F16).permute(0, 3, 1, 2)
    assert torch.equal(s.latents, want)


def _unit_params():
    return [pytest.param(case, name, kind, ins, id=f"{case}-{name}") for case in ENC_CASES for name, kind, ins in ER.encoder_units(enc_cfg(case))]


@pytest.mark.parametrize("case,name,kind,ins", _unit_params())
def test_unit_matches_fp64(case, name, kind, ins, results_log):
    s = enc_case(case)
    given = [s.inputs[i] if i in s.inputs else s.taps[i] for i in ins]
    ref64 = ER.encoder_unit(s.ref, s.cfg, name, kind, given, s.scaled, s.one)
    model = ER.encoder_unit(s.model, s.cfg, name, kind, given, s.scaled, s.one)
    bad = MU.compare(results_log, f"vae_encoder_units/{case}/{name}", s.taps[name], model, ref64)
    assert bad is None, bad


# ====================================================================== 3. free-running taps and latents
@pytest.mark.parametrize("case", list(ENC_CASES))
def test_free_running_taps_and_latents(case, results_log):
    """The rule of test_vae_free_running_taps: every block tap (and here the moments and the latents) against a free-running float64
    forward, rel-L2 <= 1e-2 each - a hand-over between units that is consistent but wrong cannot pass this one."""
    s = enc_case(case)
    taps = {}
    moments = ER.encode_ref(s.cfg, s.ref.w, s.inputs["x_in"], taps=taps, dtype=F64)
    worst = {tap: rel_l2(s.taps[tap], taps[tap]) for tap in s.prog.tap_names}
    worst["moments"] = rel_l2(s.taps["moments"], moments)
    worst["latents"] = rel_l2(s.latents, ER.latents_of(s.cfg, moments))
    results_log[f"vae_encoder_units/{case}/free_running_rel_l2"] = worst
    print(f"[vae-encoder] {case} free-running: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert set(worst) == {"down0", "down1", "down2", "down3", "mid", "moments", "latents"}
    assert all(v <= 1e-2 for v in worst.values()), worst


# ====================================================================== 4. full width
def test_full_width_latents(results_log):
    """The SDXL VAE's own widths (128, 256, 512, 512), 34.2 M encoder parameters, at 64 x 64 pictures, B = 2: latents against the
    restatement under the decoder's full-size bar (tests/test_fullsize_gpu.py, test_full_vae_B17_matches_oracle: rel-L2 <= 1e-2)."""
    n = native()
    cfg = R.VAECfg()
    w = R.make_weights(ER.encoder_spec(cfg), 1)
    net = n.NativeVAEEncoder(n.VAEConfig(), n.DictProvider(w), DEV)
    u8 = pictures(2, 64, 64, 64)
    prog = net.build(2, 8)
    names = prog.prog.op_names()
    assert ATTN512 in names and names.count(GEMM) >= 3
    got = prog.encode(u8.to(DEV)).clone()
    with torch.no_grad():
        moments = ER.encode_ref(cfg, w, ER.picture(u8).float())
    want = ER.latents_of(cfg, moments)
    worst = max(rel_l2(got[b:b + 1], want[b:b + 1]) for b in range(2))
    results_log["vae_encoder_full_width_B2_64"] = {"worst_rel_l2": worst, "moments_rel_l2": rel_l2(MU.nchw(prog.moments()), moments)}
    print(f"[vae-encoder] FULL SDXL VAE encoder B=2 64^2: worst latents rel_l2={worst:.3e}")
    assert torch.isfinite(got).all() and worst <= 1e-2
    del prog
    torch.cuda.empty_cache()


# ====================================================================== 5. the overflow regime
@functools.lru_cache(maxsize=None)
def overflow_weights():
    """conv_in scaled by 2^16 (a power of two: still fp16-representable): the residual stream then runs at 1e5 and more from the first
    unit to the last - beyond the fp16 maximum, inside what the 2^-4 scale of the fp16 stream can hold."""
    cfg = R.VAECfg(block_channels=VAE_CH)
    w = R.make_weights(ER.encoder_spec(cfg), 1)
    for k in ("encoder.conv_in.weight", "encoder.conv_in.bias"):
        w[k] = w[k] * 2.0 ** 16
    return cfg, w


@pytest.mark.parametrize("scaled", [True, False])
def test_overflow_regime(scaled, results_log):
    cfg, w = overflow_weights()
    s = build_case(cfg, dict(stream_fp16_scaled=scaled), 2, 16, 1, w=w, seed=2128)
    # the precondition, on the CPU reference: every unit of the raw stream peaks above 65504 and below 2^4 * 65504
    run = ER.free_run(s.ref, cfg, s.inputs["x_in"])
    peaks = {k: float(v.abs().max()) for k, v in run.items() if k not in ("x_in", "moments", "latents")}
    assert all(65504.0 < p < 16 * 65504.0 for p in peaks.values()), peaks
    assert torch.isfinite(s.latents).all() and torch.isfinite(s.moments).all()
    failed = []
    for name, kind, ins in ER.encoder_units(cfg):
        given = [s.inputs[i] if i in s.inputs else s.taps[i] for i in ins]
        assert torch.isfinite(s.taps[name]).all(), name
        ref64 = ER.encoder_unit(s.ref, cfg, name, kind, given, scaled, s.one)
        model = ER.encoder_unit(s.model, cfg, name, kind, given, scaled, s.one)
        bad = MU.compare(results_log, f"vae_encoder_units/overflow_{'f16s' if scaled else 'f32'}/{name}", s.taps[name], model, ref64)
        if bad:
            failed.append(bad)
    assert not failed, "\n".join(failed)
    assert max(float(s.taps[k].abs().max()) for k in peaks) > 65504.0, "the native stream is in the regime too"


# ====================================================================== 6. lifetimes, eager = graph
def test_reads_no_free_buffer():
    """Op-by-op replay with every arena buffer the journal says is free (or fresh and unwritten) filled with NaNs, as
    test_vae_reads_no_free_buffer does: the outputs are those of an ordinary launch, bit for bit."""
    import test_model_units_gpu as TMU
    for case in ("enc_B3_128_scaled", "enc_B3_128_f32"):
        s = enc_case(case)
        p = s.prog
        p.x_in.copy_(s.x_in)
        TMU.check_lifetimes(p.prog, p.arena, p.prog.launch, lambda: [p.latents, p.moments_f32])
        assert torch.equal(p.latents, s.latents) and torch.equal(p.moments(), s.moments)


@pytest.mark.parametrize("L", [16, (12, 20)])
def test_eager_equals_graph(L):
    n = native()
    cfg = R.VAECfg(block_channels=VAE_CH)
    net = n.NativeVAEEncoder(n.VAEConfig(**dataclasses.asdict(cfg)), n.SyntheticProvider(1), DEV)
    H, W = (L, L) if isinstance(L, int) else L
    u8 = pictures(2, 8 * H, 8 * W, 5).to(DEV)
    prog = net.build(2, L)
    eager_z, eager_m = prog.encode(u8).clone(), prog.moments().clone()
    prog.enable_graphs()
    assert prog.prog.graph_ready
    prog.latents.zero_(); prog.moments_f32.zero_()
    for _ in range(2):
        assert torch.equal(prog.encode(u8), eager_z) and torch.equal(prog.moments(), eager_m)
    with pytest.raises(ValueError, match="uint8"):
        prog.encode(u8.float())
    with pytest.raises(ValueError, match="expected"):
        prog.encode(u8[:1])


# ====================================================================== 7. pipe-level equalities
def make_pipe(scheduler="ddim", **kw):
    n = native()
    return n.NativeSDXLPipe(turbo=True, unet_cfg=n.UNetConfig(**dataclasses.asdict(R.tiny_unet_cfg())),
                            vae_cfg=n.VAEConfig(**dataclasses.asdict(R.tiny_vae_cfg())), seed=0, scheduler=scheduler,
                            allow_synthetic=True, **kw)


def make_engine(pipe, size=(128, 128), **kw):
    from latentblending_amd import BlendingEngine
    np.random.seed(0)
    be = BlendingEngine(pipe, verbose=False, **kw)
    be.set_dimensions(size)
    be.set_num_inference_steps(4)
    be.set_branching(depth_strength=0.5, nmb_max_branches=5)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    return be


def picture(size=(128, 128), seed=1):
    return Image.fromarray(pictures(1, size[1], size[0], seed)[0].numpy())


def ordered(h):
    """fp16 bit patterns as integers that count representable values in order (sign-magnitude -> two's complement)."""
    i = h.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def test_pipe_full_encoder_equalities(results_log):
    p = make_pipe(encoder="full")
    assert p.encoder == "full" and p.vae_encoder_native is None, "built on first use"
    be = make_engine(p)
    img = picture()
    p.render_size = (128, 128)
    before = p.vae_encodes
    z = p.native_image2latent(img)
    assert tuple(z.shape) == (1, 4, 16, 16) and z.dtype == F16 and z.is_cuda and p.vae_encodes == before + 1
    assert p._vae_encoder_programs and not p._tiny_encoder_programs and p.tiny_vae_encoder_native is None
    # against the float64 restatement on the stand-in's weights (the pipe packs SyntheticProvider(seed + 1))
    cfg = R.tiny_vae_cfg()
    w = R.make_weights(ER.encoder_spec(cfg), 1)
    u8 = torch.from_numpy(np.asarray(img).copy())[None]
    want = ER.latents_of(cfg, ER.encode_ref(cfg, w, ER.picture(u8), dtype=F64))
    results_log["vae_encoder_pipe_rel_l2"] = rel_l2(z, want)
    assert rel_l2(z, want) <= 1e-2
    # = mode() * scaling_factor from the facade, bit for bit
    x = (u8.permute(0, 3, 1, 2).float() / 127.5 - 1.0).to(DEV)
    dist = p.vae.encode(x).latent_dist
    assert dist.mean.dtype == F32 and tuple(dist.mean.shape) == (1, 4, 16, 16) and torch.equal(dist.mode(), dist.mean)
    assert torch.equal((dist.mode() * p.vae_cfg.scaling_factor).to(F16), z)
    assert torch.equal(p.vae.encode(x.half()).latent_dist.mean, dist.mean) and torch.equal(p.vae.encode(x.double()).latent_dist.mean, dist.mean)
    assert p.vae_encodes == before + 1, "vae.encode is not native_image2latent: the counter counts the latter"
    # = the generic branch of DiffusersHolder.image2latent (a pipe that is not native, with this VAE), bit for bit
    holder, real = be.dh, be.dh.pipe
    assert torch.equal(holder.image2latent(img), z)
    holder.pipe = types.SimpleNamespace(vae=p.vae, _execution_device=p.device)
    try:
        generic = holder.image2latent(img)
    finally:
        holder.pipe = real
    assert generic.dtype == F16 and torch.equal(generic, z)
    # sample(generator): float64 mean + std * eps from the program's own moments, within 1 fp16 ulp (fp32 arithmetic, one rounding)
    prog = p.vae_encoder_program(1, 16)
    prog.encode(u8.to(DEV))
    m64 = MU.nchw(prog.moments()).double().cpu()
    gen = torch.Generator(device=DEV).manual_seed(77)
    got = p.vae.encode(x).latent_dist.sample(gen)
    eps = torch.randn((1, 4, 16, 16), generator=torch.Generator(device=DEV).manual_seed(77), device=DEV, dtype=F32)
    want = ER.sample_ref(m64, eps.double().cpu())
    assert got.dtype == F32 and int((ordered(got.half().cpu()) - ordered(want.to(F16))).abs().max()) <= 1
    assert not torch.equal(got, dist.mean) and torch.equal(dist.logvar, MU.nchw(prog.moments())[:, 4:].clamp(-30, 20))
    # lists, arrays and tensors; the size rule; the LRU cache; the switch back
    assert torch.equal(p.native_image2latent(np.asarray(img)), z) and torch.equal(p.native_image2latent([img, img])[1:], z)
    with pytest.raises(ValueError, match=r"200 x 90.*128 x 128"):
        p.native_image2latent(picture((200, 90)))
    assert set(p._vae_encoder_programs) == {(1, 16), (2, 16)}
    p.encoder = "tiny"
    zt = p.native_image2latent(img)
    assert p._tiny_encoder_programs and not torch.equal(zt, z)
    with pytest.raises(ValueError, match="encoder must be"):
        p.encoder = "bogus"
    assert p.encoder == "tiny"


def test_default_pipe_builds_only_the_tiny_encoder():
    p = make_pipe()
    assert p.encoder == "tiny"
    p.render_size = (128, 128)
    p.native_image2latent(picture())
    assert p._tiny_encoder_programs and not p._vae_encoder_programs and p.vae_encoder_native is None
    # a ready-made decoder without its provider: the default pipe takes it as ever, the full encoder refuses
    n = native()
    q = make_pipe(vae_native=p.vae_native)
    with pytest.raises(ValueError, match="never paired"):
        q.encoder = "full"
    with pytest.raises(ValueError, match="never paired"):
        q.vae.encode(torch.zeros(1, 3, 128, 128, device=DEV))
    with pytest.raises(ValueError, match="never paired"):
        make_pipe(vae_native=p.vae_native, encoder="full")
    ready = n.NativeVAEEncoder(p.vae_cfg, n.SyntheticProvider(1), DEV)
    r = make_pipe(vae_native=p.vae_native, vae_encoder_native=ready, encoder="full")
    r.render_size = (128, 128)
    assert r.native_image2latent(picture()).shape == (1, 4, 16, 16) and r.vae_encoder_native is ready


# ====================================================================== 8. engine and replay
def test_engine_anchor_under_the_full_encoder(tmp_path):
    from latentblending_amd import replay
    p = make_pipe(encoder="full")
    be = make_engine(p)
    img = picture(seed=3)
    # strength 0: the anchor's final entry is the full encoder's latents, at no UNet cost
    be.seed1 = 420
    be.set_anchor_image1(img, 0.0)
    s0 = p.stats["unet_samples"]
    traj = be.compute_latents_image(1)
    assert p.stats["unet_samples"] == s0 and len(traj) == 4
    x0 = p.native_image2latent(img)
    a, b = p.scheduler.noise_level(4)
    assert torch.equal(traj[-1], (a * x0.float() + b * be.dh.get_unit_noise(420).float()).half())
    p.encoder = "tiny"
    assert not torch.equal(p.native_image2latent(img), x0)
    p.encoder = "full"
    # strength 0.5 runs a transition
    be.set_anchor_image1(img, 0.5)
    frames = be.run_transition(fixed_seeds=[420, 421])
    assert len(frames) >= 3 and p.stats["unet_samples"] > s0
    be.clear_anchor_images()
    # the movie JSON's header key selects the encoder for the movie and the pipe is restored afterwards
    p.encoder = "tiny"
    img.save(tmp_path / "key.png")
    prompts, seeds = ["a reef", "a photo"], [21, 22]
    items = [{"iteration": i, "seed": s, "prompt": t, "negative_prompt": ""} for i, (s, t) in enumerate(zip(seeds, prompts))]
    items[1].update(image="key.png", image_strength=0.0)
    replay.save_movie_json(str(tmp_path / "full.json"), be, items, image_encoder="full")
    replay.save_movie_json(str(tmp_path / "tiny.json"), be, items)
    with open(tmp_path / "tiny.json") as fh:
        assert "image_encoder" not in json.load(fh)[0]
    full_programs = len(p._vae_encoder_programs)
    encodes = p.vae_encodes
    replay.run_movie_json(make_engine(p), str(tmp_path / "full.json"))
    be_full_last = p.vae_encodes
    assert p.encoder == "tiny" and be_full_last == encodes + 1 and len(p._vae_encoder_programs) >= max(full_programs, 1)
    be2 = make_engine(p)
    replay.run_movie_json(be2, str(tmp_path / "full.json"))
    z_full = be2.tree_latents[-1][-1].clone()
    be3 = make_engine(p)
    replay.run_movie_json(be3, str(tmp_path / "tiny.json"))
    z_tiny = be3.tree_latents[-1][-1].clone()
    be4 = make_engine(p)
    replay.run_movie_json(be4, str(tmp_path / "tiny.json"), image_encoder="full")
    a, b = p.scheduler.noise_level(4)
    want_full = (a * x0.float() + b * be2.dh.get_unit_noise(22).float()).half()
    assert torch.equal(z_full, want_full) and torch.equal(be4.tree_latents[-1][-1], want_full) and not torch.equal(z_tiny, z_full)
    assert p.encoder == "tiny"
