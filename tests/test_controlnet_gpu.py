"""The native ControlNet on a real MI355X, against tests/_controlnet_ref.py in float64.

1. the hint embedding (the conv shapes no kernel here had run: Cin 8 / 16 / 32 / 96 / 256, stride 2 at image resolution), conv by
   conv, at three picture sizes (two of them ragged for the halo tiles) with and without wrap-around padding;
2. the zero conv fused with the skip add - one in-place GEMM epilogue - at the real SDXL widths;
3. the controlled step program unit by unit (``control.*`` marks and eps), free-running, and replayed with every free or fresh
   arena buffer poisoned;
4. exact properties: zero zero-convs / scale 0 / no hint leave the plain program's eps bit for bit; ``set_control_scale`` under an
   instantiated graph;
5. the three native loops, the generic loop through the facades, a whole ``run_transition``, and roll equivariance under ``tileable``.

Every element-wise bound is ``MU.compare``'s: four times the storage model's own error against float64 (tests/_model_units.py).
"""
import ctypes as C
import dataclasses
import functools
import types

import numpy as np
import pytest
import torch
from PIL import Image

import _controlnet_ref as CR
import _model_units as MU
import _tileable_ref as T
from oracle import sdxl_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
DEEP, SHALLOW = (0, 1, 2), (0, 0, 1)
SCALE = 0.75


def native():
    import latentblending_amd.native as n
    return n


def lib():
    from latentblending_amd.hip import lib as l
    return l


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def max_err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def nchw(t):
    t = t.detach().cpu()
    return MU.nchw(t).contiguous() if t.dim() == 4 else t


@functools.lru_cache(maxsize=None)
def unet_weights():
    return R.make_weights(R.unet_spec(R.tiny_unet_cfg()), 0)


@functools.lru_cache(maxsize=None)
def unet_net():
    n, cfg = native(), R.tiny_unet_cfg()
    return n.NativeUNet(n.UNetConfig(**dataclasses.asdict(cfg)), n.SyntheticProvider(0), DEV)


@functools.lru_cache(maxsize=None)
def control(depth, zeroed=False, scale=SCALE):
    """(native ControlNet loaded from the reference's state dict, its oracle config, its weights)."""
    n, ucfg = native(), R.tiny_unet_cfg()
    ccfg = CR.control_cfg(ucfg, depth)
    cw = CR.control_weights(ccfg)
    if zeroed:
        cw = {k: (torch.zeros_like(v) if k.startswith(("controlnet_down_blocks.", "controlnet_mid_block.")) else v) for k, v in cw.items()}
    cfg = n.ControlNetConfig.for_unet(unet_net().cfg, transformer_depth=depth)
    assert cfg.cond_embed_channels == CR.COND_EMBED
    net = n.NativeControlNet.from_state_dict(cw, cfg, device=DEV, scale=scale)
    return net, ccfg, cw


def hint_u8(H, W, seed=0, period=None):
    g = torch.Generator().manual_seed(100 + seed)
    u8 = (torch.rand(H, period or W, 3, generator=g) * 255).to(torch.uint8)
    return u8.repeat(1, W // period, 1).contiguous() if period else u8


def hint_of(u8):
    from latentblending_amd.native.controlnet import hint_tensor
    return hint_tensor(u8.numpy())


# ================================================================================================ 1. hint embedding
HINT_SIZES = [(64, 64), (128, 96), (96, 160)]


@functools.lru_cache(maxsize=None)
def hint_case(size, wrap):
    net, ccfg, cw = control(SHALLOW)
    prog = net.build_hint(size, wrap=wrap, journal=True)
    hint = hint_of(hint_u8(*size, seed=size[1]))
    emb = prog.embed(hint).clone()
    taps = {k: nchw(v) for k, v in prog.capture().items()}
    torch.cuda.synchronize()
    ref, model = MU.evs(cw)
    return types.SimpleNamespace(prog=prog, emb=emb, taps=taps, image=nchw(prog.image[..., :3]), ref=ref, model=model, ccfg=ccfg)


@pytest.mark.parametrize("wrap", [0, 3])
@pytest.mark.parametrize("size", HINT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hint_embedding_matches_fp64_conv_by_conv(size, wrap, results_log):
    s = hint_case(size, wrap)
    convs = CR.hint_convs(s.ccfg)
    assert [m.name for m in s.prog.marks] == ["control." + c[0] for c in convs]
    assert tuple(s.emb.shape) == (1, size[0] // 8, size[1] // 8, 64), "the output has the latent grid's size"
    assert torch.equal(s.taps["control." + convs[-1][0]], nchw(s.emb))
    print(f"[controlnet] hint {size} wrap {wrap} ops: {s.prog.prog.op_names()}")
    x, bad = s.image, []
    for name, cin, cout, stride, silu in convs:
        ref64 = CR.hint_unit(s.ref, name, x, stride, silu, wrap)
        model = CR.hint_unit(s.model, name, x, stride, silu, wrap)
        bad.append(MU.compare(results_log, f"controlnet/hint_{size[0]}x{size[1]}_w{wrap}/{name}", s.taps["control." + name], model, ref64))
        x = s.taps["control." + name]           # teacher forcing: the next conv is fed the native output
    assert not any(bad), [b for b in bad if b]
    # free running against float64
    free = CR.hint_embedding(s.ccfg, s.ref.w, s.image.double(), wrap=wrap)
    assert rel_l2(nchw(s.emb), free) <= 1e-2


# ================================================================================================ 2. zero conv + add in one epilogue
@pytest.mark.parametrize("M", [120, 512])
@pytest.mark.parametrize("N", [320, 640, 1280])
def test_zero_conv_fused_with_the_add_in_place(N, M, results_log):
    from latentblending_amd.native.runtime import Arena, Emitter
    g = torch.Generator().manual_seed(N + M)
    W = (torch.randn(N, N, generator=g) * (0.5 / N ** 0.5)).half().float()
    b = (torch.randn(N, generator=g) * 0.02).half().float()
    h = torch.randn(M, N, generator=g).half()
    skip = torch.randn(M, N, generator=g).half()
    Ws, bs = (SCALE * W.double()).to(F16), (SCALE * b.double()).to(F32)             # pre-scaled, as NativeControlNet packs them
    em = Emitter(Arena(torch.device(DEV)))
    hd, Wd, bd, out = h.to(DEV), Ws.to(DEV), bs.to(DEV), skip.to(DEV).clone()
    p = em._gemm_params(hd, Wd, out, M=M, bias=bd, residual=out)
    p.partial = em._gemm_ws(M, N).data_ptr() if em._gemm_ws(M, N) is not None else None
    tile, splitk, blocks = C.c_int(), C.c_int(), C.c_long()
    lib().api.lb_gemm_plan(C.byref(p), C.byref(tile), C.byref(splitk), C.byref(blocks))
    print(f"[controlnet] zero conv M={M} N=K={N}: tile code {tile.value}, split-K {splitk.value}, {blocks.value} blocks")
    assert tile.value > 0 and blocks.value > 0 and p.C == p.residual
    results_log[f"controlnet/zero_M{M}_N{N}/plan"] = {"tile": tile.value, "splitk": splitk.value, "blocks": blocks.value}
    em.gemm(hd, Wd, out, M=M, bias=bd, residual=out)
    torch.cuda.synchronize()
    ref64 = skip.double() + SCALE * (h.double() @ W.double().T + b.double())
    model = (skip.float() + (h.float() @ Ws.float().T + bs)).to(F16).float()
    bad = MU.compare(results_log, f"controlnet/zero_M{M}_N{N}", out.cpu(), model, ref64)
    assert bad is None, bad


# ================================================================================================ 3. controlled step program
STEP_CASES = {
    "B1_16x16_deep": dict(B=1, L=(16, 16), depth=DEEP),
    "B3_16x24_shallow": dict(B=3, L=(16, 24), depth=SHALLOW),
    "B4_16x16_shallow": dict(B=4, L=(16, 16), depth=SHALLOW),
    "B4_16x24_deep": dict(B=4, L=(16, 24), depth=DEEP),
}


def step_inputs(B, L, seed=0):
    cfg = R.tiny_unet_cfg()
    g = torch.Generator().manual_seed(B * 1000 + L[0] + L[1] + seed)
    return dict(x_in=torch.randn(B, 4, *L, generator=g).half(), tvals=torch.full((B,), 499.0), ctx=torch.randn(B, 77, cfg.cross_dim, generator=g).half(),
                text_embeds=torch.randn(B, cfg.pooled_dim, generator=g).half(), time_ids=torch.tensor([[128.0, 128.0, 0.0, 0.0, 128.0, 128.0]] * B))


@functools.lru_cache(maxsize=None)
def step_case(case):
    c = STEP_CASES[case]
    B, L = c["B"], c["L"]
    net, ccfg, cw = control(c["depth"])
    ucfg = R.tiny_unet_cfg()
    hint = hint_of(hint_u8(8 * L[0], 8 * L[1], seed=B))
    hp = net.build_hint((8 * L[0], 8 * L[1]))
    emb = hp.embed(hint).clone()
    prog = unet_net().build(B, L, journal=True, control=net)
    prog.set_hint(emb)
    i = step_inputs(B, L)

    def feed():
        prog.set_conditioning(i["ctx"].to(DEV), i["text_embeds"].to(DEV), i["time_ids"].to(DEV))
        return prog.forward(i["x_in"].to(DEV), i["tvals"]).clone()
    eps = feed()
    taps = {k: v.cpu() if k == "eps" else nchw(v) for k, v in prog.capture().items()}
    after = prog.eps.clone()
    torch.cuda.synchronize()
    inputs = dict(i, hint_emb=nchw(prog.hint_emb))
    uref, umodel = MU.evs(unet_weights())
    cref, cmodel = MU.evs(cw)
    return types.SimpleNamespace(c=c, prog=prog, feed=feed, eps=eps, after=after, taps=taps, inputs=inputs, ucfg=ucfg, ccfg=ccfg, cw=cw,
                                 uref=uref, umodel=umodel, cref=cref, cmodel=cmodel, fused=prog.ln_mode is True,
                                 hint_image=nchw(hp.image[..., :3]))


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_controlled_program_marks_and_capture(case):
    s = step_case(case)
    units, zero = CR.control_units(s.ucfg, s.ccfg)
    marks = [(m.name, m.kind, m.inputs) for m in s.prog.marks]
    assert [m for m in marks if m[0].startswith("control.") and m[1] != "zero"] == units
    assert [m for m in marks if m[1] == "zero"] == zero
    plain = [m for m in marks if not m[0].startswith("control.")]
    want = MU.unet_units(s.ucfg)
    renamed = {z[2][1]: z[0] for z in zero}                     # the UNet unit a zero conv adds into -> the unit the up path reads
    assert [m[0] for m in plain] == [u[0] for u in want]
    for got, (name, kind, ins) in zip(plain, want):      # only the up path reads the units the zero convs left
        assert got[1] == kind and got[2] == (tuple(renamed.get(i, i) for i in ins) if name.startswith("up_blocks.") else ins), (name, got, ins)
    MU.check_marks(s.prog.marks, {p.name: p for p in s.prog.programs}, set(s.inputs) | {"hint_emb"})
    names = s.prog.prog_step.op_names()
    mid_end = next(m.op_end for m in s.prog.marks if m.name == "mid_block.resnets.1")
    assert all(n == "lb_gemm_f16" for n in names[mid_end:mid_end + 10]) and s.prog.op_mid_end == mid_end, "ten fused launches after the mid block"
    assert torch.equal(s.after, s.eps) and torch.equal(s.taps["eps"], s.eps.cpu())
    assert all(torch.isfinite(t.float()).all() for t in s.taps.values())
    # the journal changes no op
    assert unet_net().build(s.c["B"], s.c["L"], control=s.prog.control).prog_step.op_names() == names


def _step_unit_params():
    out = []
    ucfg = R.tiny_unet_cfg()
    for case, c in STEP_CASES.items():
        units, zero = CR.control_units(ucfg, CR.control_cfg(ucfg, c["depth"]))
        for name, kind, ins in units + zero + [("eps", "out", None)]:
            out.append(pytest.param(case, name, kind, ins, id=f"{case}-{name}"))
    return out


@pytest.mark.parametrize("case,name,kind,ins", _step_unit_params())
def test_controlled_unit_matches_fp64(case, name, kind, ins, results_log):
    s = step_case(case)
    if name == "eps":
        ins = next(m.inputs for m in s.prog.marks if m.name == "eps")
        given = [s.taps[i] for i in ins]
        ref64 = MU.unet_unit(s.uref, s.ucfg, "eps", "out", given, s.fused)
        model = MU.unet_unit(s.umodel, s.ucfg, "eps", "out", given, s.fused)
    else:
        given = [s.inputs[i] if i in s.inputs else s.taps[i] for i in ins]
        if kind == "zero":
            k = name.rsplit(".", 1)[1]
            k = k if k == "mid" else int(k)
            ref64 = CR.zero_unit(s.cref, s.cw, k, SCALE, *given)
            model = CR.zero_unit(s.cmodel, s.cw, k, SCALE, *given)
        else:
            ref64 = CR.control_unit(s.cref, s.ccfg, name[len("control."):], kind, given, s.fused)
            model = CR.control_unit(s.cmodel, s.ccfg, name[len("control."):], kind, given, s.fused)
    bad = MU.compare(results_log, f"controlnet/{case}/{name}", s.taps[name], model, ref64)
    assert bad is None, bad


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_controlled_eps_free_running(case, results_log):
    s = step_case(case)
    i = s.inputs
    eps64 = CR.controlled_eps(s.ucfg, s.uref.w, s.ccfg, s.cref.w, i["x_in"], torch.tensor(499.0), i["ctx"], i["text_embeds"], i["time_ids"],
                              s.hint_image.double(), SCALE, dtype=F64)
    plain64 = R.unet_forward(s.ucfg, s.uref.w, i["x_in"], torch.tensor(499.0), i["ctx"], i["text_embeds"], i["time_ids"], dtype=F64)
    r, moved = rel_l2(s.eps, eps64), rel_l2(plain64, eps64)
    results_log[f"controlnet/{case}/free_running"] = {"eps_rel_l2": r, "control_moves_eps_by": moved}
    print(f"[controlnet] {case}: free-running eps rel-L2 {r:.3e}; the control moves eps by {moved:.3e}")
    assert r <= 1e-2 and moved > 10 * 1e-2, "the bar of tests/test_model_units_gpu.py - and the control is no small perturbation"


def test_controlled_program_reads_no_free_buffer():
    from test_model_units_gpu import check_lifetimes
    s = step_case("B3_16x24_shallow")
    p = s.prog
    s.feed()
    torch.cuda.synchronize()
    cs = p._control_side
    check_lifetimes(p.prog_cond, p.arena, p.prog_cond.launch, lambda: [p.aug, p.ctx_kv, cs.aug, cs.ctx_kv])
    check_lifetimes(p.prog_step, p.arena, p.prog_step.launch, lambda: [p.eps])
    assert torch.equal(p.eps, s.eps), "a hidden map released too early would show here"


# ================================================================================================ 4. exact properties
def plain_eps(B, L, i):
    prog = unet_net().build(B, L)
    prog.set_conditioning(i["ctx"].to(DEV), i["text_embeds"].to(DEV), i["time_ids"].to(DEV))
    return prog.forward(i["x_in"].to(DEV), i["tvals"]).clone(), prog


def controlled_eps(net, B, L, i, emb=None, graphs=False):
    prog = unet_net().build(B, L, control=net)
    if emb is None:
        emb = net.build_hint((8 * L[0], 8 * L[1])).embed(hint_of(hint_u8(8 * L[0], 8 * L[1], seed=7))).clone()
    prog.set_hint(emb)
    if graphs:
        prog.enable_graphs()
    prog.set_conditioning(i["ctx"].to(DEV), i["text_embeds"].to(DEV), i["time_ids"].to(DEV))
    return prog.forward(i["x_in"].to(DEV), i["tvals"]).clone(), prog


@pytest.mark.parametrize("B,L", [(2, (16, 16)), (3, (16, 24))])
def test_zero_zero_convs_and_scale_zero_leave_eps_bit_for_bit(B, L):
    i = step_inputs(B, L, seed=1)
    want, _ = plain_eps(B, L, i)
    zeroed, _, _ = control(SHALLOW, zeroed=True)
    got, _ = controlled_eps(zeroed, B, L, i)
    assert torch.equal(got, want), "zero-conv weights and biases all zero: fp16 skip + 0 is exact"
    net, _, _ = control(DEEP, scale=0.0)
    assert all(float(net.w[k].abs().max()) == 0.0 for k in net.w if k.startswith(("controlnet_down_blocks.", "controlnet_mid_block.")))
    got, _ = controlled_eps(net, B, L, i)
    assert torch.equal(got, want), "conditioning scale 0"
    live, _, _ = control(SHALLOW)
    moved, _ = controlled_eps(live, B, L, i)
    assert not torch.equal(moved, want)


def tiny_pipe(controlnet=None, **kw):
    n = native()
    ucfg, vcfg = R.tiny_unet_cfg(), R.tiny_vae_cfg()
    return n.NativeSDXLPipe(turbo=False, unet_cfg=n.UNetConfig(**dataclasses.asdict(ucfg)), vae_cfg=n.VAEConfig(**dataclasses.asdict(vcfg)),
                            seed=0, scheduler="ddim", allow_synthetic=True, controlnet=controlnet, **kw)


def pipe_controlnet(depth=SHALLOW):
    n = native()
    _, _, cw = control(depth)
    return (n.ControlNetConfig.for_unet(unet_net().cfg, transformer_depth=depth), n.DictProvider(cw))


def test_a_loaded_controlnet_without_a_hint_changes_nothing():
    i = step_inputs(2, (16, 16), seed=2)
    outs = []
    for p in (tiny_pipe(), tiny_pipe(controlnet=pipe_controlnet())):
        prog = p.unet_program(2, 16)
        prog.set_conditioning(i["ctx"].to(DEV), i["text_embeds"].to(DEV), i["time_ids"].to(DEV))
        outs.append((prog.prog_step.op_names(), prog.prog_cond.op_names(), prog.forward(i["x_in"].to(DEV), i["tvals"]).clone(), p, prog))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])
    p, prog = outs[1][3], outs[1][4]
    assert not p.control_active and prog.control is None
    # a hint switches to the controlled program under another key; clearing it brings the plain one back - the same object
    p.set_control_image(hint_u8(128, 128).numpy(), 0.5)
    cprog = p.unet_program(2, 16)
    assert p.control_active and cprog is not prog and cprog.control is p.controlnet_native and p.unet_program(2, 16, control=False) is prog
    p.clear_control()
    assert p.unet_program(2, 16) is prog
    p.unload_controlnet()
    with pytest.raises(ValueError, match="no ControlNet is loaded"):
        p.set_control_image(hint_u8(128, 128).numpy())
    with pytest.raises(ValueError):       # a ControlNet that does not fit the UNet is refused when it is loaded
        n = native()
        p.load_controlnet(n.ControlNetConfig())


def test_set_control_scale_under_an_instantiated_graph():
    B, L = 2, (16, 16)
    i = step_inputs(B, L, seed=3)
    n = native()
    _, ccfg, cw = control(SHALLOW)
    cfg = n.ControlNetConfig.for_unet(unet_net().cfg, transformer_depth=SHALLOW)
    net = n.NativeControlNet.from_state_dict(cw, cfg, device=DEV, scale=1.0)
    emb = net.build_hint((128, 128)).embed(hint_of(hint_u8(128, 128, seed=7))).clone()
    first, prog = controlled_eps(net, B, L, i, emb=emb, graphs=True)
    assert prog.prog_step.graph_ready
    ptrs = {k: t.data_ptr() for k, t in net.w.items() if t is not None}
    net.set_scale(0.4)
    assert {k: t.data_ptr() for k, t in net.w.items() if t is not None} == ptrs and prog.prog_step.graph_ready
    replay = prog.forward(i["x_in"].to(DEV), i["tvals"]).clone()
    fresh_net = n.NativeControlNet.from_state_dict(cw, cfg, device=DEV, scale=0.4)
    fresh, _ = controlled_eps(fresh_net, B, L, i, emb=emb)
    assert torch.equal(replay, fresh) and not torch.equal(replay, first)
    for k in net.w:
        if net.w[k] is not None:
            assert torch.equal(net.w[k], fresh_net.w[k]), k


# ================================================================================================ 5. loops
STEPS, GUIDANCE = 4, 4.0


@functools.lru_cache(maxsize=None)
def loop_world():
    from latentblending_amd import DiffusersHolder
    p = tiny_pipe(controlnet=pipe_controlnet())
    dh = DiffusersHolder(p)
    dh.set_dimensions((128, 128))
    dh.set_num_inference_steps(STEPS)
    dh.guidance_scale = GUIDANCE
    hint = Image.fromarray(hint_u8(128, 128, seed=9).numpy())
    return p, dh, hint


def test_the_native_loops_and_the_generic_loop_agree_under_a_control_image(results_log):
    from latentblending_amd.backend import set_backend
    from latentblending_amd.hip import ops
    set_backend(None)
    p, dh, hint = loop_world()
    emb1, emb2 = dh.get_text_embedding("a reef"), dh.get_text_embedding("an alien planet")
    z1, z2 = dh.get_noise(1), dh.get_noise(2)
    zero = [0.0] * STEPS
    plain = p.native_run_diffusion(emb1, z1, 0, None, zero, STEPS, GUIDANCE)
    dh.set_control(hint, SCALE)
    try:
        assert p.control_active
        generic = [dh._denoise_generic(e, z, 0, None, zero) for e, z in ((emb1, z1), (emb2, z2))]
        batch = p.native_run_diffusion_batch([emb1, emb2], [z1, z2], 0, [None, None], [zero, zero], STEPS, [GUIDANCE, GUIDANCE])
        idx = 2
        a1, a2, mids = p.native_run_wavefront([emb1, emb2], [z1, z2], [emb1], [0.5], [zero], idx, STEPS, GUIDANCE, [GUIDANCE])
        start = ops.slerp_pairs([batch[0][idx - 1]], [batch[1][idx - 1]], [0.5])[0]
        mid = p.native_run_diffusion_batch([emb1], [start], idx, [None], [zero], STEPS, [GUIDANCE])[0]
        mid_generic = dh._denoise_generic(emb1, start, idx, None, zero)
    finally:
        dh.set_control(None)
    assert not p.control_active
    figures = {"batch_vs_generic": max(rel_l2(a, b) for g in (0, 1) for a, b in zip(batch[g], generic[g])),
               "wavefront_anchor_vs_generic": max(rel_l2(a, b) for w, g in ((a1, 0), (a2, 1)) for a, b in zip(w, generic[g])),
               "wavefront_mid_vs_batch": max(rel_l2(a, b) for a, b in zip(mids[0][idx:], mid[idx:])),
               "mid_vs_generic": max(rel_l2(a, b) for a, b in zip(mid[idx:], mid_generic[idx:])),
               "control_moves_the_trajectory_by": rel_l2(plain[-1], batch[0][-1])}
    results_log["controlnet/loops"] = figures
    print(f"[controlnet] loops: {figures}")
    assert all(figures[k] <= 2e-2 for k in ("batch_vs_generic", "wavefront_anchor_vs_generic", "wavefront_mid_vs_batch", "mid_vs_generic")), figures
    assert figures["control_moves_the_trajectory_by"] > 2e-2
    assert torch.equal(p.native_run_diffusion(emb1, z1, 0, None, zero, STEPS, GUIDANCE)[-1], plain[-1]), "no hint: the plain run again"


def test_run_transition_under_a_control_image(results_log):
    from latentblending_amd import BlendingEngine
    from latentblending_amd.backend import set_backend
    set_backend(None)
    p, _, hint = loop_world()
    np.random.seed(0)
    be = BlendingEngine(p, verbose=False)
    be.set_dimensions((128, 128))
    be.set_num_inference_steps(STEPS)
    be.set_branching(depth_strength=0.5, nmb_max_branches=3)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")

    def frames():
        be.set_guidance_scale(GUIDANCE)
        return [np.asarray(f).copy() for f in be.run_transition(fixed_seeds=[11, 12])]
    plain = frames()
    be.set_control_image(hint, SCALE)
    controlled = frames()
    assert len(controlled) == len(plain) >= 3 and p.control_active and p.control_scale == SCALE
    assert all(not np.array_equal(a, b) for a, b in zip(controlled, plain))
    be.swap_forward()
    assert be.control_image is hint
    be.clear_control_image()
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    again = frames()
    assert not p.control_active and all(np.array_equal(a, b) for a, b in zip(again, plain)), "clear_control_image: the uncontrolled frames bit for bit"


def test_tileable_controlled_eps_is_roll_equivariant(results_log):
    """``tileable="x"`` and a hint that is periodic in x (period 32 pixels = 4 latent columns): eps(roll(x, 4)) == roll(eps(x), 4)
    within 2 e, e = the native eps' max-abs distance from the circular float64 model - the bound of tests/test_tileable_gpu.py."""
    p = tiny_pipe(controlnet=pipe_controlnet(), tileable="x")
    L = (16, 24)
    u8 = hint_u8(128, 192, seed=11, period=32)
    p.set_control_image(u8.numpy(), SCALE)
    prog = p.unet_program(2, L)
    assert prog.wrap == 1 and prog.control is not None
    i = step_inputs(2, L, seed=4)

    def eps_of(x):
        prog.set_conditioning(i["ctx"].to(DEV), i["text_embeds"].to(DEV), i["time_ids"].to(DEV))
        return prog.forward(x.to(DEV), i["tvals"]).clone().cpu()
    eps = eps_of(i["x_in"])
    _, ccfg, cw = control(SHALLOW)
    uref, _ = MU.evs(unet_weights())
    cref, _ = MU.evs(cw)
    hint = (hint_of(u8).half().double()).permute(0, 3, 1, 2)
    with T.circular_oracle(1):
        eps64 = CR.controlled_eps(R.tiny_unet_cfg(), uref.w, ccfg, cref.w, i["x_in"], torch.tensor(499.0), i["ctx"], i["text_embeds"],
                                  i["time_ids"], hint, SCALE, dtype=F64)
    e = max_err(eps, eps64)
    assert rel_l2(eps, eps64) <= 1e-2
    defect_x = max_err(eps_of(torch.roll(i["x_in"], 4, 3)), torch.roll(eps, 4, 3))
    defect_y = max_err(eps_of(torch.roll(i["x_in"], 4, 2)), torch.roll(eps, 4, 2))
    results_log["controlnet/tileable_x"] = {"e": e, "defect_x": defect_x, "defect_y": defect_y}
    print(f"[controlnet] tileable x: e {e:.3e}, defect along x {defect_x:.3e} (allowance {2 * e:.3e}), along y {defect_y:.3e}")
    assert defect_x <= 2 * e and defect_y > 2 * e
    # another tileable setting drops the controlled programs and embeds the hint again
    p.tileable = ""
    assert not p._control_programs and not p._control_emb
    assert p.unet_program(2, L).wrap == 0 and p.unet_program(2, L).control is not None
