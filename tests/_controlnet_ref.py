"""Reference for the ControlNet tests (tests/test_controlnet_cpu.py, tests/test_controlnet_gpu.py).

RESTATED, NOT PINNED: neither diffusers nor a ControlNet checkpoint is available here.  The forward follows the published architecture
of diffusers' SDXL ``ControlNetModel`` and is composed from the oracle's untouched primitives (``R.resnet_block``, ``R.transformer_2d``,
``R._conv``, ``R.unet_embedding``); ``unet_forward_controlled`` with all residuals zero equals ``R.unet_forward`` bit for bit, which
pins the restated UNet half to the oracle.

The zero convs are synthetic and NOT zero: gain ``ZERO_GAIN`` (W ~ N(0, ZERO_GAIN^2 / C)), so that a residual's rms is a real fraction
of its skip's (test_controlnet_cpu.py asserts >= 0.1 for every one).  A hidden map of rms r gives a residual of rms about
ZERO_GAIN r, and the ControlNet's hidden maps are the size of the UNet's skips (same architecture, same initialisation).

Unit evaluators (``control_unit``) follow tests/_model_units.py: REF = float64, MODEL = fp32 with a rounding wherever the program
stores; the bound is ``MU.compare``'s (4x the storage model's own error).  ``MU.unet_layout`` reads the column layout of the fused
projections from the UNet's weight enumeration; a ControlNet has no up blocks, so its own layout is swapped in (``control_layout``)
while its units are evaluated.
"""
import contextlib
import dataclasses

import torch
import torch.nn.functional as F

import _model_units as MU
from oracle import sdxl_ref as R

F16, F32, F64 = torch.float16, torch.float32, torch.float64
COND_EMBED = (16, 32, 96, 256)
ZERO_GAIN = 0.5
CONTROL_SEED = 3


def control_cfg(unet_cfg, depth=None):
    """The ControlNet's config as an oracle ``UNetCfg``: the UNet's, with the ControlNet's own transformer depths."""
    return dataclasses.replace(unet_cfg, transformer_depth=tuple(depth if depth is not None else unet_cfg.transformer_depth))


def hint_convs(cfg, embed=COND_EMBED):
    p = "controlnet_cond_embedding."
    out = [(p + "conv_in", 3, embed[0], 1, True)]
    for i in range(len(embed) - 1):
        out.append((f"{p}blocks.{2 * i}", embed[i], embed[i], 1, True))
        out.append((f"{p}blocks.{2 * i + 1}", embed[i], embed[i + 1], 2, True))
    out.append((p + "conv_out", embed[-1], cfg.block_channels[0], 1, False))
    return out


def controlnet_spec(cfg, embed=COND_EMBED, zero_gain=ZERO_GAIN) -> R._Spec:
    """Weight enumeration of a ControlNet of config ``cfg`` (``control_cfg``), diffusers key names."""
    s = R._Spec()
    ch, T = cfg.block_channels, cfg.time_embed_dim
    s.conv("conv_in", cfg.in_channels, ch[0], 3)
    s.linear("time_embedding.linear_1", ch[0], T)
    s.linear("time_embedding.linear_2", T, T)
    s.linear("add_embedding.linear_1", cfg.add_in_dim, T)
    s.linear("add_embedding.linear_2", T, T)
    for name, cin, cout, _, _ in hint_convs(cfg, embed):
        s.conv(name, cin, cout, 3)
    prev = ch[0]
    for bi, c in enumerate(ch):
        for li in range(cfg.layers_per_block):
            R._resnet_spec(s, f"down_blocks.{bi}.resnets.{li}", prev, c, T)
            if cfg.transformer_depth[bi]:
                R._transformer_spec(s, f"down_blocks.{bi}.attentions.{li}", c, cfg.transformer_depth[bi], cfg.cross_dim)
            prev = c
        if bi < len(ch) - 1:
            s.conv(f"down_blocks.{bi}.downsamplers.0.conv", c, c, 3)
    for k, c in enumerate(R.unet_skip_channels(cfg)):
        s.conv(f"controlnet_down_blocks.{k}", c, c, 1, gain=zero_gain)
    s.conv("controlnet_mid_block", ch[-1], ch[-1], 1, gain=zero_gain)
    R._resnet_spec(s, "mid_block.resnets.0", ch[-1], ch[-1], T)
    R._transformer_spec(s, "mid_block.attentions.0", ch[-1], cfg.transformer_depth[-1], cfg.cross_dim)
    R._resnet_spec(s, "mid_block.resnets.1", ch[-1], ch[-1], T)
    return s


def control_weights(cfg, seed=CONTROL_SEED, embed=COND_EMBED):
    return R.make_weights(controlnet_spec(cfg, embed), seed)


def hint_embedding(cfg, w, hint, embed=COND_EMBED, taps=None, wrap=0):
    """hint [B, 3, H, W] in [0, 1] -> [B, C0, H / 8, W / 8].  ``wrap``: bit 0 the columns, bit 1 the rows pad by wrap-around."""
    h = hint
    for name, _, _, stride, silu in hint_convs(cfg, embed):
        h = conv_wrapped(h, w, name, stride, wrap)
        if silu:
            h = F.silu(h)
        if taps is not None:
            taps[name] = h
    return h


def conv_wrapped(x, w, name, stride=1, wrap=0):
    if not wrap:
        return R._conv(x, w, name, stride=stride, pad=1)
    x = F.pad(x, (1, 1, 0, 0), mode="circular" if wrap & 1 else "constant")
    x = F.pad(x, (0, 0, 1, 1), mode="circular" if wrap & 2 else "constant")
    return R._conv(x, w, name, stride=stride, pad=0)


def controlnet_forward(cfg, w, sample, t, ctx, text_embeds, time_ids, hint, scale=1.0, dtype=torch.float32, taps=None, embed=COND_EMBED,
                       drop_hint=False):
    """-> (down residuals in skip order, mid residual), each ``scale * zero_conv(hidden map)``.  ``taps``: the hidden maps by unit name."""
    g = cfg.norm_groups
    x, ctx = sample.to(dtype), ctx.to(dtype)
    emb = R.unet_embedding(cfg, w, torch.as_tensor(t), text_embeds, time_ids, dtype)
    ch = cfg.block_channels
    h = R._conv(x, w, "conv_in")
    if not drop_hint:
        h = h + hint_embedding(cfg, w, hint.to(dtype), embed)
    hs = [h]
    if taps is not None:
        taps["conv_in"] = h
    for bi, c in enumerate(ch):
        for li in range(cfg.layers_per_block):
            h = R.resnet_block(h, emb, w, f"down_blocks.{bi}.resnets.{li}", g, 1e-5)
            if cfg.transformer_depth[bi]:
                h = R.transformer_2d(h, ctx, w, f"down_blocks.{bi}.attentions.{li}", cfg.transformer_depth[bi], c // cfg.head_dim, g)
            hs.append(h)
        if bi < len(ch) - 1:
            h = R._conv(h, w, f"down_blocks.{bi}.downsamplers.0.conv", stride=2, pad=1)
            hs.append(h)
    c = ch[-1]
    h = R.resnet_block(h, emb, w, "mid_block.resnets.0", g, 1e-5)
    h = R.transformer_2d(h, ctx, w, "mid_block.attentions.0", cfg.transformer_depth[-1], c // cfg.head_dim, g)
    h = R.resnet_block(h, emb, w, "mid_block.resnets.1", g, 1e-5)
    if taps is not None:
        taps["hidden"], taps["mid"] = hs, h
    down = [scale * R._conv(hk, w, f"controlnet_down_blocks.{k}", pad=0) for k, hk in enumerate(hs)]
    return down, scale * R._conv(h, w, "controlnet_mid_block", pad=0)


def unet_forward_controlled(cfg, w, sample, t, ctx, text_embeds, time_ids, down_res, mid_res, taps=None, dtype=torch.float32, mutant=None):
    """``R.unet_forward`` with the ControlNet's residuals: ``down_res[k]`` is added to the k-th SKIP COPY only - the hidden state that
    continues down the encoder is not changed -, ``mid_res`` to the mid block's output.  ``mutant`` (the tests' wrong variants):
    ``("drop_zero", k)``, ``"drop_mid"``, ``"hidden"`` = the residual goes into the continuing hidden state instead of the skip copy."""
    g = cfg.norm_groups
    x, ctx = sample.to(dtype), ctx.to(dtype)
    emb = R.unet_embedding(cfg, w, torch.as_tensor(t), text_embeds, time_ids, dtype)
    ch = cfg.block_channels
    res = list(down_res)
    if isinstance(mutant, tuple) and mutant[0] == "drop_zero":
        res[mutant[1]] = torch.zeros_like(res[mutant[1]])
    hidden = mutant == "hidden"

    def keep(h):
        """(the skip copy, the hidden state that goes on) after unit number len(skips)"""
        r = res[len(skips)]
        return (h, h + r) if hidden else (h + r, h)

    skips = []
    h = R._conv(x, w, "conv_in")
    if taps is not None:
        taps["emb"], taps["conv_in"] = emb, h
    s, h = keep(h)
    skips.append(s)
    for bi, c in enumerate(ch):
        for li in range(cfg.layers_per_block):
            h = R.resnet_block(h, emb, w, f"down_blocks.{bi}.resnets.{li}", g, 1e-5)
            if cfg.transformer_depth[bi]:
                h = R.transformer_2d(h, ctx, w, f"down_blocks.{bi}.attentions.{li}", cfg.transformer_depth[bi], c // cfg.head_dim, g)
            s, h = keep(h)
            skips.append(s)
        if bi < len(ch) - 1:
            h = R._conv(h, w, f"down_blocks.{bi}.downsamplers.0.conv", stride=2, pad=1)
            s, h = keep(h)
            skips.append(s)
        if taps is not None:
            taps[f"down{bi}"] = h
    c = ch[-1]
    h = R.resnet_block(h, emb, w, "mid_block.resnets.0", g, 1e-5)
    h = R.transformer_2d(h, ctx, w, "mid_block.attentions.0", cfg.transformer_depth[-1], c // cfg.head_dim, g)
    h = R.resnet_block(h, emb, w, "mid_block.resnets.1", g, 1e-5)
    if mutant != "drop_mid":
        h = h + mid_res
    if taps is not None:
        taps["mid"], taps["skips"] = h, list(skips)
    depths = list(reversed(cfg.transformer_depth))
    for ui, (c, cins) in enumerate(R.unet_up_plan(cfg)):
        for li in range(len(cins)):
            h = torch.cat([h, skips.pop()], dim=1)
            h = R.resnet_block(h, emb, w, f"up_blocks.{ui}.resnets.{li}", g, 1e-5)
            if depths[ui]:
                h = R.transformer_2d(h, ctx, w, f"up_blocks.{ui}.attentions.{li}", depths[ui], c // cfg.head_dim, g)
        if ui < len(ch) - 1:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = R._conv(h, w, f"up_blocks.{ui}.upsamplers.0.conv")
        if taps is not None:
            taps[f"up{ui}"] = h
    h = F.silu(R._gn(h, w, "conv_norm_out", g, 1e-5))
    return R._conv(h, w, "conv_out")


def controlled_eps(ucfg, uw, ccfg, cw, sample, t, ctx, text_embeds, time_ids, hint, scale=1.0, dtype=torch.float32, mutant=None, taps=None):
    """eps of the UNet guided by the ControlNet, both in ``dtype`` (weights ``uw`` / ``cw`` of that type)."""
    down, mid = controlnet_forward(ccfg, cw, sample, t, ctx, text_embeds, time_ids, hint, scale, dtype, drop_hint=mutant == "drop_hint")
    if taps is not None:
        taps["down_res"], taps["mid_res"] = down, mid
    return unet_forward_controlled(ucfg, uw, sample, t, ctx, text_embeds, time_ids, down, mid, taps=taps, dtype=dtype,
                                   mutant=None if mutant == "drop_hint" else mutant)


def cast(w, dtype):
    return {k: v.to(dtype) for k, v in w.items()}


# ---------------------------------------------------------------------------------------------------------------- units
def layout_of(spec):
    temb, ctx, nt, nc = {}, {}, 0, 0
    for name, shape, _, _ in spec.items:
        if name.endswith(".time_emb_proj.weight"):
            temb[name[:-len(".time_emb_proj.weight")]] = (nt, shape[0])
            nt += shape[0]
        elif name.endswith(".attn2.to_k.weight"):
            ctx[name[:-len(".attn2.to_k.weight")]] = (nc, shape[0])
            nc += shape[0]
    return temb, nt, ctx, nc


@contextlib.contextmanager
def control_layout(ccfg):
    """While the block runs, ``MU``'s unit evaluators read the column layout of the CONTROLNET's fused projections."""
    layout, old = layout_of(controlnet_spec(ccfg)), MU.unet_layout
    MU.unet_layout = lambda cfg: layout
    try:
        yield
    finally:
        MU.unet_layout = old


def control_units(ucfg, ccfg):
    """[(name, kind, inputs)] of the ``control.*`` marks of a controlled step program (conditioning program first), in order."""
    ch = ccfg.block_channels
    units = [("control.aug", "aug", ("text_embeds", "time_ids")), ("control.ctx_kv", "ctx_kv", ("ctx",)),
             ("control.temb_all", "temb_all", ("tvals", "control.aug")), ("control.conv_in", "conv_in", ("x_in", "hint_emb"))]
    at, hidden = "control.conv_in", ["control.conv_in"]

    def add(name, kind, *more):
        nonlocal at
        units.append(("control." + name, kind, (at,) + more))
        at = "control." + name

    for bi in range(len(ch)):
        for li in range(ccfg.layers_per_block):
            add(f"down_blocks.{bi}.resnets.{li}", "resnet", "control.temb_all")
            if ccfg.transformer_depth[bi]:
                add(f"down_blocks.{bi}.attentions.{li}", "transformer", "control.ctx_kv")
            hidden.append(at)
        if bi < len(ch) - 1:
            add(f"down_blocks.{bi}.downsamplers.0.conv", "downsample")
            hidden.append(at)
    add("mid_block.resnets.0", "resnet", "control.temb_all")
    add("mid_block.attentions.0", "transformer", "control.ctx_kv")
    add("mid_block.resnets.1", "resnet", "control.temb_all")
    # the UNet's own skip units, from the plain program's unit list
    skips = ["conv_in"]
    for bi in range(len(ch)):
        for li in range(ucfg.layers_per_block):
            skips.append(f"down_blocks.{bi}.attentions.{li}" if ucfg.transformer_depth[bi] else f"down_blocks.{bi}.resnets.{li}")
        if bi < len(ch) - 1:
            skips.append(f"down_blocks.{bi}.downsamplers.0.conv")
    zero = [(f"control.zero.{k}", "zero", (hidden[k], skips[k])) for k in range(len(hidden))]
    zero.append(("control.zero.mid", "zero", (at, "mid_block.resnets.1")))
    return units, zero


def zero_unit(ev, cw, k, scale, h, skip):
    """skip + scale * (W h + b) as the program computes it: ONE GEMM epilogue, the weight stored as fp16(scale W), the bias as fp32."""
    name = "controlnet_mid_block" if k == "mid" else f"controlnet_down_blocks.{k}"
    W, b = cw[name + ".weight"].double() * scale, cw[name + ".bias"].double() * scale
    if ev.store:
        W, b = W.to(F16), b.to(F32)
    return ev.q(F.conv2d(ev.t(h), W.to(ev.dt), b.to(ev.dt)) + ev.t(skip))


def control_unit(ev, ccfg, name, kind, ins, fused_ln):
    """One ``control.*`` unit of the encoder (``ev``: an ``MU.Ev`` over the ControlNet's weights).  ``name`` without the prefix."""
    with control_layout(ccfg):
        if kind == "conv_in":
            x, e = [ev.t(t) for t in ins]
            return ev.q(R._conv(x, ev.w, "conv_in") + e)
        if kind == "ctx_kv" and not layout_of(controlnet_spec(ccfg))[3]:
            raise KeyError("a ControlNet without cross-attention has no ctx_kv unit")
        return MU.unet_unit(ev, ccfg, name, kind, ins, fused_ln)


def hint_unit(ev, name, x, stride, silu, wrap=0):
    y = conv_wrapped(ev.t(x), ev.w, name, stride, wrap)
    return ev.q(F.silu(y) if silu else y)
