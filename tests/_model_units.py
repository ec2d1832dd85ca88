"""Unit-by-unit references for the native UNet / VAE programs (tests/test_model_units_gpu.py, tests/test_model_units_cpu.py).

A *unit* is what the programs mark (``UNetProgram.marks`` / ``VAEProgram.marks``): a resnet, a transformer, a down- or upsampler,
the embedding GEMMs, the first and the last conv.  Every unit is evaluated here from the oracle's primitives (``oracle.sdxl_ref``:
``_gn``, ``_conv``, ``_lin``, ``attention``, ``sinusoid``) in one of two modes (``Ev``):

* ``REF``   - float64 arithmetic, float64 weights, nothing rounded: the reference;
* ``MODEL`` - the *storage model*: the same unit in float32 with a rounding wherever the program stores a tensor (fp16 for fp16
  tensors, nothing for fp32 outputs), after the fused epilogue (bias, row vector, residual, SiLU / GEGLU).  Its error against REF
  is the yardstick the native unit is held to (``compare``): it is a property of the number formats, never of the kernels.

The inputs of a unit are the tensors the native program produced (teacher forcing), so errors do not add up across units.
Unit names, kinds and inputs (``unet_units`` / ``vae_units``) and the column layout of the two fused projections are derived here
from the oracle's weight enumeration, not read from the programs.  Feature maps are NCHW here; ``nchw`` / ``nhwc`` convert.
"""
import math

import torch
import torch.nn.functional as F

from oracle import sdxl_ref as R

F16, F32, F64 = torch.float16, torch.float32, torch.float64
STREAM = 1.0 / 16.0          # the VAE's scaled fp16 residual stream holds value * 2^-4
CTX_TOKENS, CTX_PAD = 77, 80
FACTOR = 4.0                 # two bits over the storage model: accumulation order, exp2-based softmax / SiLU, a moved rounding point


class Ev:
    """One way to evaluate a unit: arithmetic type, weights of that type, and whether stores round."""

    def __init__(self, dtype, w, store):
        self.dt, self.store = dtype, store
        self.w = {k: v.to(dtype) for k, v in w.items()}

    def t(self, x):
        return x.detach().cpu().to(self.dt)

    def q(self, x):
        """A tensor the program stores as fp16 (or feeds to the MFMA as an fp16 operand)."""
        return x.to(F16).to(self.dt) if self.store else x

    def q_scaled(self, x):
        """fp16 holding value * 2^-4 (the scaled stream; the raw-stream operand of the fp32-stream VAE)."""
        return (x * STREAM).to(F16).to(self.dt) / STREAM if self.store else x

    def q_stream(self, x, scaled):
        """The VAE's residual stream: scaled fp16, or fp32 (no rounding beyond the model's own arithmetic)."""
        return self.q_scaled(x) if scaled else x


def evs(w):
    """(REF, MODEL) over one set of fp32 weights (fp16-representable values: both see the same parameters)."""
    return Ev(F64, w, False), Ev(F32, w, True)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------------------------- comparison
def errors(x, ref64):
    d = x.detach().cpu().double() - ref64
    return float(d.norm() / (ref64.norm() + 1e-300)), float(d.abs().max())


def compare(log, key, native, model, ref64):
    """Every element of ``native`` against the float64 reference, bounded by FACTOR times the storage model's own error.  Logs the
    four numbers (and the two ratios) under ``key``; returns None or the failure text."""
    ref64 = ref64.detach().cpu().double()
    assert tuple(native.shape) == tuple(ref64.shape) == tuple(model.shape), (key, native.shape, model.shape, ref64.shape)
    m_l2, m_max = errors(model, ref64)
    n_l2, n_max = errors(native, ref64)
    finite = bool(torch.isfinite(native.detach().cpu().float()).all())
    r_l2, r_max = n_l2 / max(m_l2, 1e-300), n_max / max(m_max, 1e-300)
    log[key] = {"e_model_l2": m_l2, "e_model_max": m_max, "e_native_l2": n_l2, "e_native_max": n_max,
                "ratio_l2": r_l2, "ratio_max": r_max}
    print(f"[units] {key}: native l2={n_l2:.3e} max={n_max:.3e} | model l2={m_l2:.3e} max={m_max:.3e} | "
          f"ratio l2={r_l2:.2f} max={r_max:.2f}")
    if not finite:
        return f"{key}: non-finite native output"
    if not (n_l2 <= FACTOR * m_l2 and n_max <= FACTOR * m_max):
        return (f"{key}: native rel-L2 {n_l2:.3e} (model {m_l2:.3e}, ratio {r_l2:.2f}), max-abs {n_max:.3e} "
                f"(model {m_max:.3e}, ratio {r_max:.2f}) - over {FACTOR:g}x the storage model")
    return None


# ---------------------------------------------------------------------------------------------------------------- shared pieces
def gn(ev, x, p, groups, eps, silu):
    """GroupNorm (+ SiLU) as the programs store it: fp16 - a GroupNorm launch writes an fp16 tensor, and a conv that applies the
    GroupNorm itself (LB_GEMM_GN_A) rounds the normalised value to the fp16 MFMA operand: the same rounding point either way."""
    y = R._gn(x, ev.w, p, groups, eps)
    return ev.q(F.silu(y) if silu else y)


def subpixel_conv(ev, h, p):
    """nearest-2x upsample + 3x3 conv.  REF: literally that.  MODEL: the four 2x2 sub-pixel kernels the programs launch - the taps
    of the 3x3 kernel that fall on the same source pixel are summed and the SUM is rounded to fp16 (the packed weight the kernel
    reads): a rounding point of the weights, present in every route of the upsampler."""
    w, b = ev.w[p + ".weight"], ev.w[p + ".bias"]
    if not ev.store:
        return F.conv2d(F.interpolate(h, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    B, C, H, W = h.shape
    w64 = w.double()
    rows = {0: [w64[:, :, 0], w64[:, :, 1] + w64[:, :, 2]], 1: [w64[:, :, 0] + w64[:, :, 1], w64[:, :, 2]]}     # [Cout, Cin, kx]
    hp = F.pad(h, (1, 1, 1, 1))
    out = h.new_zeros(B, w.shape[0], 2 * H, 2 * W)
    for py in (0, 1):
        for px in (0, 1):
            k = torch.zeros(w.shape[0], C, 2, 2, dtype=F64)
            for a in (0, 1):
                r = rows[py][a]
                cols = [r[:, :, 0], r[:, :, 1] + r[:, :, 2]] if px == 0 else [r[:, :, 0] + r[:, :, 1], r[:, :, 2]]
                for c in (0, 1):
                    k[:, :, a, c] = cols[c]
            y = F.conv2d(hp, k.to(F16).to(ev.dt), b)                    # [B, Cout, H + 1, W + 1]: entry (i, j) sees rows i-1, i
            out[:, :, py::2, px::2] = y[:, :, py:py + H, px:px + W]
    return out


def ln_linear(ev, h, w_ln, b_ln, W, b, fused):
    """Linear(LayerNorm(h)) (eps 1e-5) as the programs compute it.  Unfused: the LayerNorm launch stores fp16.  Fused
    (LB_GEMM_LN_A): nothing is stored in between; the GEMM runs on the raw h with W' = fp16(W diag(gamma)), and the epilogue
    applies rstd * (h W'^T - mean * colsum(W')) + (b + W beta) - the rounding of W' is a rounding point of the packed weights."""
    C = h.shape[-1]
    if not ev.store or not fused:
        n = ev.q(F.layer_norm(h, (C,), w_ln, b_ln, 1e-5))
        return F.linear(n, W, b)
    Wf = (W.double() * w_ln.double()[None, :]).to(F16).double()
    colsum = Wf.sum(dim=1).to(F32).to(ev.dt)
    b2 = W.double() @ b_ln.double()
    if b is not None:
        b2 = b2 + b.double()
    mean = h.mean(dim=-1, keepdim=True)
    rstd = torch.rsqrt(h.var(dim=-1, unbiased=False, keepdim=True) + 1e-5)
    return rstd * (F.linear(h, Wf.to(ev.dt)) - mean * colsum[None, :]) + b2.to(F32).to(ev.dt)


# ---------------------------------------------------------------------------------------------------------------- UNet
def unet_layout(cfg):
    """Column offsets of the two fused projections, from the oracle's weight enumeration: resnet prefix -> (offset, cout) in
    ``temb_all``; transformer block prefix -> (offset, C) in each half of ``ctx_kv`` = [K of all blocks | V of all blocks]."""
    temb, ctx, nt, nc = {}, {}, 0, 0
    for name, shape, _, _ in R.unet_spec(cfg).items:
        if name.endswith(".time_emb_proj.weight"):
            temb[name[:-len(".time_emb_proj.weight")]] = (nt, shape[0])
            nt += shape[0]
        elif name.endswith(".attn2.to_k.weight"):
            ctx[name[:-len(".attn2.to_k.weight")]] = (nc, shape[0])
            nc += shape[0]
    return temb, nt, ctx, nc


def unet_units(cfg, guided=False):
    """[(name, kind, inputs)] of a UNet program, conditioning program first - what ``UNetProgram.marks`` must list."""
    ch = cfg.block_channels
    units = [("aug", "aug", ("text_embeds", "time_ids")), ("ctx_kv", "ctx_kv", ("ctx",)),
             ("temb_all", "temb_all", ("tvals", "aug") + (("timestep_cond",) if guided else ())),
             ("conv_in", "conv_in", ("x_in",))]
    at, skips = "conv_in", ["conv_in"]

    def add(name, kind, *more):
        nonlocal at
        units.append((name, kind, (at,) + more))
        at = name

    for bi in range(len(ch)):
        for li in range(cfg.layers_per_block):
            add(f"down_blocks.{bi}.resnets.{li}", "resnet", "temb_all")
            if cfg.transformer_depth[bi]:
                add(f"down_blocks.{bi}.attentions.{li}", "transformer", "ctx_kv")
            skips.append(at)
        if bi < len(ch) - 1:
            add(f"down_blocks.{bi}.downsamplers.0.conv", "downsample")
            skips.append(at)
    add("mid_block.resnets.0", "resnet", "temb_all")
    add("mid_block.attentions.0", "transformer", "ctx_kv")
    add("mid_block.resnets.1", "resnet", "temb_all")
    depths = list(reversed(cfg.transformer_depth))
    for ui in range(len(ch)):
        for li in range(cfg.layers_per_block + 1):
            add(f"up_blocks.{ui}.resnets.{li}", "resnet", skips.pop(), "temb_all")
            if depths[ui]:
                add(f"up_blocks.{ui}.attentions.{li}", "transformer", "ctx_kv")
        if ui < len(ch) - 1:
            add(f"up_blocks.{ui}.upsamplers.0.conv", "upsample")
    add("eps", "out")
    return units


def unet_tap_names(cfg):
    """The oracle's block taps -> the unit whose output each is."""
    ch, taps = cfg.block_channels, {"conv_in": "conv_in", "mid": "mid_block.resnets.1"}
    depths = list(reversed(cfg.transformer_depth))
    for bi in range(len(ch)):
        last = cfg.layers_per_block - 1
        taps[f"down{bi}"] = f"down_blocks.{bi}.downsamplers.0.conv" if bi < len(ch) - 1 else \
            (f"down_blocks.{bi}.attentions.{last}" if cfg.transformer_depth[bi] else f"down_blocks.{bi}.resnets.{last}")
    for ui in range(len(ch)):
        last = cfg.layers_per_block
        taps[f"up{ui}"] = f"up_blocks.{ui}.upsamplers.0.conv" if ui < len(ch) - 1 else \
            (f"up_blocks.{ui}.attentions.{last}" if depths[ui] else f"up_blocks.{ui}.resnets.{last}")
    return taps


def unet_aug(ev, cfg, text_embeds, time_ids):
    B = text_embeds.shape[0]
    ids = ev.q(R.sinusoid(ev.t(time_ids).reshape(-1), cfg.add_time_dim, ev.dt)).reshape(B, -1)
    add_in = torch.cat([ev.t(text_embeds), ids], dim=-1)
    a1 = ev.q(F.silu(R._lin(add_in, ev.w, "add_embedding.linear_1")))
    return ev.q(R._lin(a1, ev.w, "add_embedding.linear_2"))


def unet_ctx_kv(ev, cfg, ctx):
    """[B * 80, 2 n_ctx]: K of every cross-attention block, then V of every block; context rows 77..79 are zero padding."""
    _, _, slices, _ = unet_layout(cfg)
    Wkv = torch.cat([ev.w[b + ".attn2.to_k.weight"] for b in slices] + [ev.w[b + ".attn2.to_v.weight"] for b in slices], 0)
    c = F.pad(ev.t(ctx), (0, 0, 0, CTX_PAD - CTX_TOKENS))
    return ev.q(F.linear(c.reshape(-1, c.shape[-1]), Wkv))


def unet_temb_all(ev, cfg, tvals, aug, tcond=None, wc=None):
    """[B, n_temb]: the time-embedding projections of all resnets, of silu(time_embedding(t) + aug)."""
    slices, _, _, _ = unet_layout(cfg)
    tsin = ev.q(R.sinusoid(ev.t(tvals).reshape(-1), cfg.block_channels[0], ev.dt))
    if tcond is not None:
        tsin = ev.q(F.linear(ev.t(tcond), ev.t(wc)) + tsin)
    t1 = ev.q(F.silu(R._lin(tsin, ev.w, "time_embedding.linear_1")))
    emb = ev.q(F.silu(R._lin(t1, ev.w, "time_embedding.linear_2") + ev.t(aug)))
    Wp = torch.cat([ev.w[p + ".time_emb_proj.weight"] for p in slices], 0)
    bp = torch.cat([ev.w[p + ".time_emb_proj.bias"] for p in slices], 0)
    return ev.q(F.linear(emb, Wp, bp))


def unet_resnet(ev, cfg, p, x, temb_all):
    """x [B, cin, H, W] (an up-block resnet: the concatenation [h | skip]); the time term is this resnet's slice of ``temb_all``,
    added as a row vector in conv1's epilogue."""
    w, g = ev.w, cfg.norm_groups
    off, cout = unet_layout(cfg)[0][p]
    n1 = gn(ev, x, p + ".norm1", g, 1e-5, True)
    h = ev.q(R._conv(n1, w, p + ".conv1") + ev.t(temb_all)[:, off:off + cout, None, None])
    n2 = gn(ev, h, p + ".norm2", g, 1e-5, True)
    xs = ev.q(R._conv(x, w, p + ".conv_shortcut", pad=0)) if (p + ".conv_shortcut.weight") in w else x
    return ev.q(R._conv(n2, w, p + ".conv2") + xs)


def unet_transformer(ev, cfg, p, x, ctx_kv, depth, fused_ln):
    """x [B, C, H, W]; ``ctx_kv`` as the conditioning program left it: the blocks' K / V of the text context are its column slices."""
    w = ev.w
    B, C, H, W = x.shape
    heads = C // cfg.head_dim
    _, _, slices, n_ctx = unet_layout(cfg)
    kv = ev.t(ctx_kv).reshape(B, CTX_PAD, 2 * n_ctx)[:, :CTX_TOKENS]
    n = nhwc(gn(ev, x, p + ".norm", cfg.norm_groups, 1e-6, False)).reshape(B, H * W, C)
    h = ev.q(R._lin(n, w, p + ".proj_in"))
    for d in range(depth):
        b = f"{p}.transformer_blocks.{d}"
        Wqkv = torch.cat([w[f"{b}.attn1.{nm}.weight"] for nm in ("to_q", "to_k", "to_v")], 0)
        qkv = ev.q(ln_linear(ev, h, w[b + ".norm1.weight"], w[b + ".norm1.bias"], Wqkv, None, fused_ln))
        q, k, v = qkv.chunk(3, dim=-1)
        a = ev.q(R.attention(q.contiguous(), k.contiguous(), v.contiguous(), heads))
        h = ev.q(R._lin(a, w, b + ".attn1.to_out.0") + h)
        q = ev.q(ln_linear(ev, h, w[b + ".norm2.weight"], w[b + ".norm2.bias"], w[b + ".attn2.to_q.weight"], None, fused_ln))
        off, c = slices[b]
        a = ev.q(R.attention(q, kv[..., off:off + c].contiguous(), kv[..., n_ctx + off:n_ctx + off + c].contiguous(), heads))
        h = ev.q(R._lin(a, w, b + ".attn2.to_out.0") + h)
        ff = ln_linear(ev, h, w[b + ".norm3.weight"], w[b + ".norm3.bias"], w[b + ".ff.net.0.proj.weight"],
                       w[b + ".ff.net.0.proj.bias"], fused_ln)
        hh, gate = ff.chunk(2, dim=-1)
        h = ev.q(R._lin(ev.q(hh * F.gelu(gate)), w, b + ".ff.net.2") + h)         # GEGLU in the epilogue: one store
    return ev.q(nchw(R._lin(h, w, p + ".proj_out").reshape(B, H, W, C)) + x)


def unet_unit(ev, cfg, name, kind, ins, fused_ln, wc=None):
    """Evaluate one UNet unit.  ``ins``: the unit's inputs in the order ``unet_units`` lists them - feature maps NCHW."""
    ins = [ev.t(t) for t in ins]
    if kind == "aug":
        return unet_aug(ev, cfg, *ins)
    if kind == "ctx_kv":
        return unet_ctx_kv(ev, cfg, *ins)
    if kind == "temb_all":
        return unet_temb_all(ev, cfg, ins[0], ins[1], ins[2] if len(ins) > 2 else None, wc)
    if kind == "conv_in":
        return ev.q(R._conv(ins[0], ev.w, "conv_in"))
    if kind == "resnet":
        x = ins[0] if len(ins) == 2 else torch.cat([ins[0], ins[1]], dim=1)
        return unet_resnet(ev, cfg, name, x, ins[-1])
    if kind == "transformer":
        depth = sum(1 for k in ev.w if k.startswith(name + ".transformer_blocks.") and k.endswith(".norm1.weight"))
        return unet_transformer(ev, cfg, name, ins[0], ins[1], depth, fused_ln)
    if kind == "downsample":
        return ev.q(R._conv(ins[0], ev.w, name, stride=2, pad=1))
    if kind == "upsample":
        return ev.q(subpixel_conv(ev, ins[0], name))
    if kind == "out":
        n = gn(ev, ins[0], "conv_norm_out", cfg.norm_groups, 1e-5, True)
        return ev.q(R._conv(n, ev.w, "conv_out"))
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------------------- VAE
def vae_units(cfg):
    """[(name, kind, inputs)] of a VAE decode program - what ``VAEProgram.marks`` must list."""
    units, at = [("conv_in", "conv_in", ("z_in",))], "conv_in"

    def add(name, kind):
        nonlocal at
        units.append((name, kind, (at,)))
        at = name

    add("decoder.mid_block.resnets.0", "resnet")
    add("mid_attention", "mid_attention")
    add("decoder.mid_block.resnets.1", "resnet")
    n = len(cfg.block_channels)
    for ui in range(n):
        for li in range(cfg.layers_per_block + 1):
            add(f"decoder.up_blocks.{ui}.resnets.{li}", "resnet")
        if ui < n - 1:
            add(f"decoder.up_blocks.{ui}.upsamplers.0.conv", "upsample")
    add("image_f32", "out")
    return units


def vae_tap_names(cfg):
    n = len(cfg.block_channels)
    taps = {"mid": "decoder.mid_block.resnets.1"}
    for ui in range(n):
        taps[f"up{ui}"] = f"decoder.up_blocks.{ui}.upsamplers.0.conv" if ui < n - 1 else \
            f"decoder.up_blocks.{ui}.resnets.{cfg.layers_per_block}"
    return taps


def vae_resnet(ev, cfg, p, x, scaled):
    """x: the residual stream in real units.  The 1x1 shortcut reads the raw stream as an fp16 operand carrying the 2^-4 scale (the
    scaled stream as it is; a cast of the fp32 stream)."""
    w, g = ev.w, cfg.norm_groups
    n1 = gn(ev, x, p + ".norm1", g, 1e-6, True)
    h = ev.q_stream(R._conv(n1, w, p + ".conv1"), scaled)
    n2 = gn(ev, h, p + ".norm2", g, 1e-6, True)
    xs = ev.q_stream(R._conv(ev.q_scaled(x), w, p + ".conv_shortcut", pad=0), scaled) if (p + ".conv_shortcut.weight") in w else x
    return ev.q_stream(R._conv(n2, w, p + ".conv2") + xs, scaled)


def vae_mid_attention(ev, cfg, h, scaled, one_launch):
    """One head over all channels.  The programs fold the V bias into the output projection's bias (softmax rows sum to 1): the
    same function.  ``one_launch`` (lb_attn_fwd_d512): scores and probabilities never leave the kernel; otherwise the scaled scores
    are stored fp16 (a GEMM output) and lb_softmax_rows_f16 replaces them by fp16 probabilities in place."""
    w, a = ev.w, "decoder.mid_block.attentions.0"
    B, C, H, W = h.shape
    n = nhwc(gn(ev, h, a + ".group_norm", cfg.norm_groups, 1e-6, False)).reshape(B, H * W, C)
    q, k = ev.q(R._lin(n, w, a + ".to_q")), ev.q(R._lin(n, w, a + ".to_k"))
    if not ev.store:
        o = R.attention(q, k, R._lin(n, w, a + ".to_v"), 1)
        bias = w[a + ".to_out.0.bias"]
    else:
        v = ev.q(F.linear(n, w[a + ".to_v.weight"]))
        bias = w[a + ".to_out.0.bias"] + w[a + ".to_out.0.weight"] @ w[a + ".to_v.bias"]
        if one_launch:
            o = ev.q(R.attention(q, k, v, 1))
        else:
            p = ev.q(torch.softmax(ev.q(q @ k.transpose(-1, -2) * float(C) ** -0.5), dim=-1))
            o = ev.q(p @ v)
    out = F.linear(o, w[a + ".to_out.0.weight"], bias)
    return ev.q_stream(nchw(out.reshape(B, H, W, C)) + h, scaled)


def vae_unit(ev, cfg, name, kind, ins, scaled, one_launch=False):
    """Evaluate one VAE unit.  ``ins``: [z_in NCHW fp16] for ``conv_in``, else [the stream, NCHW, real units]."""
    x = ev.t(ins[0])
    if kind == "conv_in":
        z8 = ev.q(x / cfg.scaling_factor)
        pq = ev.q(R._conv(z8, ev.w, "post_quant_conv", pad=0))
        return ev.q_stream(R._conv(pq, ev.w, "decoder.conv_in"), scaled)
    if kind == "resnet":
        return vae_resnet(ev, cfg, name, x, scaled)
    if kind == "mid_attention":
        return vae_mid_attention(ev, cfg, x, scaled, one_launch)
    if kind == "upsample":
        return ev.q_stream(subpixel_conv(ev, ev.q_scaled(x), name), scaled)
    if kind == "out":
        n = gn(ev, x, "decoder.conv_norm_out", cfg.norm_groups, 1e-6, True)
        return R._conv(n, ev.w, "decoder.conv_out")                       # image_f32: an fp32 store
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------------------- journal
def journal_state(journal, n_buffers, upto=None):
    """Walk an arena journal and check it as a ledger.  ``upto`` = (program, op index): only the entries made before that op was
    recorded count (entries of other programs count in full when they were recorded earlier).  Returns (live ids, ids allocated
    exactly at ``upto``); raises AssertionError on a double release, a release of something never allocated, or an allocation of
    a live buffer."""
    live, fresh, seen = set(), set(), set()
    for event, buf, prog, op in journal:
        assert 0 <= buf < n_buffers, (event, buf, prog, op)
        if upto is not None and prog == upto[0] and op > upto[1]:
            break
        if event == "alloc":
            assert buf not in live, f"buffer {buf} allocated at {prog}:{op} while live"
            live.add(buf)
            seen.add(buf)
            if upto is not None and (prog, op) == tuple(upto):
                fresh.add(buf)
        else:
            assert event == "release", event
            assert buf in seen, f"buffer {buf} released at {prog}:{op} without having been allocated"
            assert buf in live, f"buffer {buf} released twice (second time at {prog}:{op})"
            live.discard(buf)
            fresh.discard(buf)
    return live, fresh


def check_marks(marks, progs, inputs):
    """Marks are ordered, inside their programs, and read only what exists: earlier marks or program inputs."""
    known, last = set(inputs), {}
    for m in marks:
        assert m.program in progs, m
        assert 0 <= m.op_end <= progs[m.program].num_ops, m
        assert m.op_end >= last.get(m.program, 0), f"mark {m.name}: op index {m.op_end} before {last[m.program]}"
        last[m.program] = m.op_end
        for i in m.inputs:
            assert i in known, f"mark {m.name} reads {i!r}: neither an earlier unit nor a program input"
        assert m.name not in known, f"mark {m.name} twice"
        known.add(m.name)


assert math.isclose(STREAM, 2.0 ** -4)
