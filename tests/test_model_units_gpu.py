"""The UNet and VAE programs, unit by unit, on the routes the production shapes take (a real MI355X).

1. *Route census*: every case first asserts that the ops it exists for were recorded (halo-tile 3x3 convs, the one-launch
   upsampler, the narrow conv, GroupNorm from producer statistics and its fold into the consumer, the stand-alone or folded
   LayerNorm, the streaming attention shapes), and that the program's marks are the units tests/_model_units.py derives.
2. *Teacher-forced unit parity*: every unit's native output against the same unit in float64 on the CPU, fed with the NATIVE
   inputs of that unit.  The bound is 4x the error of the storage model (the unit in fp32 with a rounding wherever the program
   stores): measured against the reference, never against the kernels.  Every element counts.
3. *Free-running taps*: the block taps against a free-running float64 forward, rel-L2 <= 1e-2 each: a hand-over between units that
   is consistent but wrong cannot pass this one.
4. *Lifetimes*: the programs replayed op by op with every arena buffer that the journal says is free (or fresh and unwritten)
   filled with fp16 NaNs: the output must be that of an ordinary launch, bit for bit.
"""
import dataclasses
import functools
import types

import pytest
import torch

import _model_units as MU
from oracle import sdxl_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, F64 = torch.float16, torch.float64
TCOND = 32
VAE_CH = (64, 128, 128, 128)

HALO, UPHALO, NARROW = "lb_conv3x3_halo_f16", "lb_upconv2x_halo_f16", "lb_conv3x3_narrow_f16"
GN_STATS, GN_TABLE, LN, ATTN64 = "lb_groupnorm_from_stats", "lb_groupnorm_affine_from_stats", "lb_layernorm_f16", "lb_attn_fwd_d64"
SOFTMAX, ATTN512 = "lb_softmax_rows_f16", "lb_attn_fwd_d512"

# B = 6, L = 64: 96 halo tiles at level 0, the 96-block one-launch upsampler, the narrow conv_out, S = 1024 self-attention at level 1;
# "auto" would leave the LayerNorms unfused here, so both forms are asked for by name.  B = 2, L = 32 with every eligible conv on the
# halo kernel: 16-wide tiles at 32 x 32 and 16 x 16, and "auto" folds the LayerNorms.
UNET_CASES = {
    "unet_B6_L64_ln_unfused": dict(B=6, L=64, halo=1, fuse=False, guided=False, have=(HALO, UPHALO, NARROW, LN, ATTN64), lack=()),
    "unet_B6_L64_ln_fused": dict(B=6, L=64, halo=1, fuse=True, guided=False, have=(HALO, UPHALO, NARROW, ATTN64), lack=(LN,)),
    "unet_B2_L32_halo2": dict(B=2, L=32, halo=2, fuse="auto", guided=False, have=(HALO, NARROW, ATTN64), lack=(LN,)),
    "unet_guided_B2_L16": dict(B=2, L=16, halo=1, fuse="auto", guided=True, have=(ATTN64,), lack=(LN,)),
    # a latent of amplitude 2^-6: the groups of conv_in's output then vary by about 5e-4, the only place in these models where a
    # GroupNorm's eps (1e-5) is not far below the variance it is added to - a wrong eps moves the first resnet by a percent here and by
    # less than an fp16 ulp everywhere else
    "unet_quiet_B2_L16": dict(B=2, L=16, halo=1, fuse="auto", guided=False, amplitude=2.0 ** -6, have=(ATTN64,), lack=(LN,)),
}
# the 128-channel top level runs the mid attention as GEMM - row softmax - GEMM whatever ``fused_mid_attention`` says (the one-launch
# kernel is for 512 channels): both values are run, as two records of the same ops.  An fp32 stream cannot fold a GroupNorm.
VAE_CASES = {
    "vae_B3_L16_scaled": dict(B=3, L=16, halo=1, kw=dict(stream_fp16_scaled=True), have=(HALO, UPHALO, NARROW, GN_STATS, GN_TABLE, SOFTMAX), lack=(ATTN512,)),
    "vae_B3_L16_f32": dict(B=3, L=16, halo=1, kw=dict(stream_fp16_scaled=False), have=(HALO, UPHALO, NARROW, GN_STATS, SOFTMAX), lack=(GN_TABLE, ATTN512)),
    "vae_B2_L16_halo2_fused": dict(B=2, L=16, halo=2, kw=dict(fused_mid_attention=True), have=(HALO, UPHALO, NARROW, GN_STATS, GN_TABLE, SOFTMAX), lack=(ATTN512,)),
    "vae_B2_L16_halo2_unfused": dict(B=2, L=16, halo=2, kw=dict(fused_mid_attention=False), have=(HALO, UPHALO, NARROW, GN_STATS, GN_TABLE, SOFTMAX), lack=(ATTN512,)),
    # ... so one more record, with a 512-channel top level, for the one-launch mid attention
    "vae_top512_B2_L16_halo2": dict(B=2, L=16, halo=2, ch=(64, 128, 128, 512), kw={}, have=(HALO, UPHALO, NARROW, GN_STATS, GN_TABLE, ATTN512), lack=(SOFTMAX,)),
}


def native():
    import latentblending_amd.native as n
    return n


def lib():
    from latentblending_amd.hip import lib as l
    return l


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def unet_cfg(case):
    cfg = R.tiny_unet_cfg()
    return dataclasses.replace(cfg, time_cond_proj_dim=TCOND) if UNET_CASES[case]["guided"] else cfg


def vae_cfg(case):
    return R.VAECfg(block_channels=VAE_CASES[case].get("ch", VAE_CH))


def to_cpu_nchw(t):
    t = t.detach().cpu()
    return MU.nchw(t).contiguous() if t.dim() == 4 else t


# ---------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def unet_case(case):
    """Build (journal on), run once as ever, capture; everything the tests of this case share, computed once."""
    n, c, cfg = native(), UNET_CASES[case], unet_cfg(case)
    plain = R.tiny_unet_cfg()
    w = R.make_weights(R.unet_spec(plain), 0)
    net = n.NativeUNet(n.UNetConfig(**dataclasses.asdict(cfg)), n.SyntheticProvider(0), DEV, fuse_layernorm=c["fuse"])
    B, L = c["B"], c["L"]
    g = torch.Generator().manual_seed(B * 1000 + L)
    inputs = dict(x_in=(torch.randn(B, 4, L, L, generator=g) * c.get("amplitude", 1.0)).half(), tvals=torch.full((B,), 499.0),
                  ctx=torch.randn(B, 77, cfg.cross_dim, generator=g).half(), text_embeds=torch.randn(B, cfg.pooled_dim, generator=g).half(),
                  time_ids=torch.tensor([[128.0, 128.0, 0.0, 0.0, 128.0, 128.0]] * B))
    wc = None
    if c["guided"]:
        inputs["timestep_cond"] = n.NativeSDXLPipe.get_guidance_scale_embedding([2.0, 7.0][:B], embedding_dim=TCOND).to(F16).cpu()
        wc = n.SyntheticProvider(0).weight("time_embedding.cond_proj.weight", (cfg.block_channels[0], TCOND), TCOND)
    lib().api.lb_gemm_set_halo(c["halo"])
    try:
        prog = net.build(B, L, journal=True)
    finally:
        lib().api.lb_gemm_set_halo(1)

    def feed():
        prog.set_conditioning(inputs["ctx"].to(DEV), inputs["text_embeds"].to(DEV), inputs["time_ids"].to(DEV),
                              **({"timestep_cond": inputs["timestep_cond"].to(DEV)} if c["guided"] else {}))
        return prog.forward(inputs["x_in"].to(DEV), inputs["tvals"]).clone()
    eps = feed()
    taps = {k: v.cpu() if k == "eps" else to_cpu_nchw(v) for k, v in prog.capture().items()}      # (eps: the NCHW output buffer)
    torch.cuda.synchronize()
    ref, model = MU.evs(w)
    return types.SimpleNamespace(case=case, c=c, cfg=cfg, plain=plain, prog=prog, feed=feed, eps=eps, eps_after_capture=prog.eps.clone(),
                                 taps=taps, inputs=inputs, ref=ref, model=model, wc=wc, fused=prog.ln_mode is True)


@functools.lru_cache(maxsize=None)
def vae_case(case):
    n, c, cfg = native(), VAE_CASES[case], vae_cfg(case)
    w = R.make_weights(R.vae_decoder_spec(cfg), 1)
    net = n.NativeVAEDecoder(n.VAEConfig(**dataclasses.asdict(cfg), **c["kw"]), n.SyntheticProvider(1), DEV)
    B, L = c["B"], c["L"]
    z = torch.randn(B, 4, L, L, generator=torch.Generator().manual_seed(B * 1000 + L)).half()
    lib().api.lb_gemm_set_halo(c["halo"])
    try:
        prog = net.build(B, L, journal=True)
    finally:
        lib().api.lb_gemm_set_halo(1)
    frames = prog.decode(z.to(DEV)).clone()
    image = prog.image_f32.clone()
    taps = {k: to_cpu_nchw(v) for k, v in prog.capture().items()}
    taps["image_f32"] = taps["image_f32"][:, :cfg.out_channels].contiguous()
    torch.cuda.synchronize()
    ref, model = MU.evs(w)
    return types.SimpleNamespace(case=case, c=c, cfg=cfg, prog=prog, z=z, frames=frames, image=image, frames_after_capture=prog.frames.clone(),
                                 image_after_capture=prog.image_f32.clone(), taps=taps, inputs=dict(z_in=z), ref=ref, model=model,
                                 scaled=bool(c["kw"].get("stream_fp16_scaled", True)))


def census(names, have, lack):
    for op in have:
        assert op in names, f"{op} was not recorded: the case does not reach the route it exists for"
    for op in lack:
        assert op not in names, f"{op} was recorded where the case exists for its absence"


# ---------------------------------------------------------------------------------------------------------------- UNet
@pytest.mark.parametrize("case", list(UNET_CASES))
def test_unet_routes_marks_and_capture(case):
    s = unet_case(case)
    names = s.prog.prog_step.op_names()
    census(names, s.c["have"], s.c["lack"])
    B, L = s.c["B"], s.c["L"]
    if L == 64:     # the shapes of the streaming kernel: S = 1024 at level 1
        assert any(e["Sq"] == 1024 and e["Skv"] == 1024 for e in s.prog.em.attn_log)
    assert s.fused == (s.c["fuse"] if s.c["fuse"] != "auto" else True)
    assert [(m.name, m.kind, m.inputs) for m in s.prog.marks] == MU.unet_units(s.cfg, s.c["guided"])
    assert s.prog.tap_names == MU.unet_tap_names(s.cfg)
    plain = s.prog.net.build(B, L) if s.c["halo"] == 1 else None            # the journal changes no op
    if plain is not None:
        assert plain.prog_step.op_names() == names and plain.prog_cond.op_names() == s.prog.prog_cond.op_names()
    # a capture is a replay: it leaves eps as the launch did, and its last tap is eps
    assert torch.equal(s.eps_after_capture, s.eps) and torch.equal(s.taps["eps"], s.eps.cpu())
    assert set(s.taps) == {m.name for m in s.prog.marks} | set(s.prog.tap_names)
    assert all(torch.isfinite(t.float()).all() for t in s.taps.values())


def _unet_unit_params():
    out = []
    for case, c in UNET_CASES.items():
        for name, kind, ins in MU.unet_units(unet_cfg(case), c["guided"]):
            if c["guided"] and name != "temb_all":          # this case is about the guidance projection in front of linear_1
                continue
            out.append(pytest.param(case, name, kind, ins, id=f"{case}-{name}"))
    return out


@pytest.mark.parametrize("case,name,kind,ins", _unet_unit_params())
def test_unet_unit_matches_fp64(case, name, kind, ins, results_log):
    s = unet_case(case)
    given = [s.inputs[i] if i in s.inputs else s.taps[i] for i in ins]
    ref64 = MU.unet_unit(s.ref, s.plain, name, kind, given, s.fused, s.wc)
    model = MU.unet_unit(s.model, s.plain, name, kind, given, s.fused, s.wc)
    bad = MU.compare(results_log, f"units/{case}/{name}", s.taps[name], model, ref64)
    assert bad is None, bad


@functools.lru_cache(maxsize=None)
def unet_free_running(case):
    s = unet_case(case)
    i, t = s.inputs, torch.tensor(499.0)
    if not s.c["guided"]:
        taps = {}
        eps = R.unet_forward(s.plain, s.ref.w, i["x_in"], t, i["ctx"], i["text_embeds"], i["time_ids"], taps=taps, dtype=F64)
        return eps, taps
    # linear_1(tsin + Wc c) = linear_1(tsin) + W1 Wc c: the unchanged oracle, one sample at a time, with that bias
    eps, taps = [], []
    for b in range(s.c["B"]):
        w2 = dict(s.ref.w)
        w2["time_embedding.linear_1.bias"] = s.ref.w["time_embedding.linear_1.bias"] + \
            s.ref.w["time_embedding.linear_1.weight"] @ (s.wc.double() @ i["timestep_cond"][b].double())
        tb = {}
        eps.append(R.unet_forward(s.plain, w2, i["x_in"][b:b + 1], t, i["ctx"][b:b + 1], i["text_embeds"][b:b + 1],
                                  i["time_ids"][b:b + 1], taps=tb, dtype=F64))
        taps.append(tb)
    return torch.cat(eps), {k: torch.cat([tb[k] for tb in taps]) for k in taps[0] if k != "emb"}


@pytest.mark.parametrize("case", list(UNET_CASES))
def test_unet_free_running_taps(case, results_log):
    s = unet_case(case)
    eps, taps = unet_free_running(case)
    worst = {}
    for tap in s.prog.tap_names:
        worst[tap] = rel_l2(s.taps[tap], taps[tap])
    worst["eps"] = rel_l2(s.eps, eps)
    results_log[f"units/{case}/free_running_rel_l2"] = worst
    print(f"[units] {case} free-running: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert all(v <= 1e-2 for v in worst.values()), worst


# ---------------------------------------------------------------------------------------------------------------- VAE
@pytest.mark.parametrize("case", list(VAE_CASES))
def test_vae_routes_marks_and_capture(case):
    s = vae_case(case)
    names = s.prog.prog.op_names()
    census(names, s.c["have"], s.c["lack"])
    assert [(m.name, m.kind, m.inputs) for m in s.prog.marks] == MU.vae_units(s.cfg)
    assert s.prog.tap_names == MU.vae_tap_names(s.cfg)
    if s.c["halo"] == 1:
        assert s.prog.net.build(s.c["B"], s.c["L"]).prog.op_names() == names
    assert torch.equal(s.frames_after_capture, s.frames) and torch.equal(s.image_after_capture, s.image)
    assert torch.equal(s.taps["image_f32"], MU.nchw(s.image.cpu())[:, :3])
    assert all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in s.taps.values())


def _vae_unit_params():
    return [pytest.param(case, name, kind, ins, id=f"{case}-{name}") for case in VAE_CASES for name, kind, ins in MU.vae_units(vae_cfg(case))]


@pytest.mark.parametrize("case,name,kind,ins", _vae_unit_params())
def test_vae_unit_matches_fp64(case, name, kind, ins, results_log):
    s = vae_case(case)
    given = [s.inputs[i] if i in s.inputs else s.taps[i] for i in ins]
    one = ATTN512 in s.prog.prog.op_names()
    ref64 = MU.vae_unit(s.ref, s.cfg, name, kind, given, s.scaled, one)
    model = MU.vae_unit(s.model, s.cfg, name, kind, given, s.scaled, one)
    bad = MU.compare(results_log, f"units/{case}/{name}", s.taps[name], model, ref64)
    assert bad is None, bad


@pytest.mark.parametrize("case", list(VAE_CASES))
def test_vae_free_running_taps(case, results_log):
    s = vae_case(case)
    taps = {}
    img = R.vae_decode(s.cfg, s.ref.w, s.z.double() / s.cfg.scaling_factor, taps=taps, dtype=F64)
    worst = {tap: rel_l2(s.taps[tap], taps[tap]) for tap in s.prog.tap_names}
    worst["image_f32"] = rel_l2(s.taps["image_f32"], img)
    results_log[f"units/{case}/free_running_rel_l2"] = worst
    print(f"[units] {case} free-running: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert all(v <= 1e-2 for v in worst.values()), worst


# ---------------------------------------------------------------------------------------------------------------- lifetimes
def poison(raw):
    raw.view(torch.int16).fill_(0x7FFF)             # fp16 NaN in every half word (an fp32 NaN in every word)


def poisoned_replay(prog, arena, start=0):
    """Replay ``prog`` one op at a time; before op i >= ``start``, fill every arena buffer that is free at i - and every buffer
    allocated for op i, which nobody has written yet - with NaNs.  Only arena buffers: inputs, outputs, weights, the zero page and the
    emitter's workspaces are not the arena's."""
    for i in range(prog.num_ops):
        if i >= start:
            live, fresh = MU.journal_state(arena.journal, len(arena.all), upto=(prog.name, i))
            for b, raw in enumerate(arena.all):
                if b not in live or b in fresh:
                    poison(raw)
        prog.run_range(i, i + 1)
    torch.cuda.synchronize()


def last_reader(prog, arena, ordinary, outputs, want):
    """The failure's address: the largest op index k such that poisoning from op k on still changes the outputs - the (last) op that
    reads a buffer while the journal has it free or fresh.  Every probe starts from the state an ordinary launch leaves."""
    def differs(k):
        ordinary()
        poisoned_replay(prog, arena, start=k)
        return any(not torch.equal(o, w) for o, w in zip(outputs(), want))
    lo, hi = 0, prog.num_ops                        # differs(lo) is known, differs(num_ops) poisons nothing
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if differs(mid):
            lo = mid
        else:
            hi = mid
    return lo


def check_lifetimes(prog, arena, ordinary, outputs):
    ordinary()
    torch.cuda.synchronize()
    want = [o.clone() for o in outputs()]
    assert not any(torch.isnan(o.float()).any() for o in want)
    for o in outputs():
        o.zero_()
    poisoned_replay(prog, arena)
    got = [o.clone() for o in outputs()]
    if all(torch.equal(g, w) for g, w in zip(got, want)):
        return
    nan = any(bool(torch.isnan(g.float()).any()) for g in got)
    k = last_reader(prog, arena, ordinary, outputs, want)
    raise AssertionError(f"{prog.name}: with the free and the fresh arena buffers poisoned the output {'holds NaNs' if nan else 'differs'}: "
                         f"op {k} ({prog.op_names()[k]}) reads a buffer that is released, or bytes of a fresh one nobody wrote")


def test_unet_reads_no_free_buffer():
    s = unet_case("unet_B6_L64_ln_unfused")
    p = s.prog
    s.feed()
    torch.cuda.synchronize()
    aug, ctx_kv = p.aug.clone(), p.ctx_kv.clone()
    check_lifetimes(p.prog_cond, p.arena, p.prog_cond.launch, lambda: [p.aug, p.ctx_kv])
    assert torch.equal(p.aug, aug) and torch.equal(p.ctx_kv, ctx_kv)
    check_lifetimes(p.prog_step, p.arena, p.prog_step.launch, lambda: [p.eps])
    assert torch.equal(p.eps, s.eps)


def test_vae_reads_no_free_buffer():
    s = vae_case("vae_B3_L16_scaled")
    p = s.prog
    p.z_in.copy_(s.z.to(DEV))
    check_lifetimes(p.prog, p.arena, p.prog.launch, lambda: [p.frames, p.image_f32])
    assert torch.equal(p.frames, s.frames) and torch.equal(p.image_f32, s.image)
