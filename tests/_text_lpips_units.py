"""Unit-by-unit references for the native CLIP text towers and the LPIPS-Alex metric (tests/test_text_lpips_units_cpu.py,
tests/test_text_lpips_units_gpu.py), in the two modes of tests/_model_units.py (``Ev``): REF - float64, nothing rounded - and MODEL -
float32 with an fp16 rounding exactly where the programs store a tensor.

CLIP storage points: the embedding sum, the output of a LayerNorm launch, every GEMM output after its fused epilogue (bias, residual,
quick-GELU ``x * sigmoid(1.702 x)`` or erf-GELU) and the attention output; inside the attention kernel the un-normalised
probabilities exp(s - max) are an fp16 MFMA operand, and the row sum is taken over those rounded values (a ones-vector MFMA).
LPIPS storage points: ``prep`` (the fp32 expression of lpips_prep_kernel, then fp16), ``max_pool2d(3, 2)`` (exact) and each conv with
fp32 accumulation + fp32 bias + ReLU stored as fp16.  The distance is plain fp32 over fp16 taps with a float32 result.

Unit names, kinds and inputs come from the config here, never from the programs; weights are keyed by the ``transformers`` state-dict
names (``text_model.`` prefix) and by the oracle's LPIPS names.  Feature maps are NCHW here.
"""
import math

import torch
import torch.nn.functional as F

import _model_units as MU
from oracle import sdxl_ref as R

F16, F32, F64 = MU.F16, MU.F32, MU.F64
SEQ, HEAD_DIM = 77, 64
CAUSAL_DIAGONAL = 0         # key k is visible to query q when k <= q + this (the CPU test shifts it to show that a slip is caught)
WINDOW = 2.0 ** -9          # a unit's storage model may be at most this far (rel-L2) from REF, and never at zero distance
TM = "text_model."


# ---------------------------------------------------------------------------------------------------------------- CLIP: weights, ids
def clip_weights(cfg, seed):
    """HF-keyed synthetic parameters of one tower, fp16-representable fp32: projections N(0, 1 / fan_in) (0.5 of that for the two
    that write the residual stream), embeddings N(0, 0.02^2) / N(0, 0.01^2), biases N(0, 0.02^2), LayerNorm weights 1 + N(0, 0.05^2)."""
    g = torch.Generator().manual_seed(seed)
    c, m = cfg.hidden_size, cfg.intermediate_size

    def rnd(shape, std, mean=0.0):
        return (torch.randn(shape, generator=g) * std + mean).half().float()
    w = {TM + "embeddings.token_embedding.weight": rnd((cfg.vocab_size, c), 0.02),
         TM + "embeddings.position_embedding.weight": rnd((cfg.max_position_embeddings, c), 0.01)}
    for i in range(cfg.num_hidden_layers):
        L = f"{TM}encoder.layers.{i}."
        for n in ("q", "k", "v"):
            w[L + f"self_attn.{n}_proj.weight"], w[L + f"self_attn.{n}_proj.bias"] = rnd((c, c), c ** -0.5), rnd((c,), 0.02)
        w[L + "self_attn.out_proj.weight"], w[L + "self_attn.out_proj.bias"] = rnd((c, c), 0.5 * c ** -0.5), rnd((c,), 0.02)
        for n in ("layer_norm1", "layer_norm2"):
            w[L + n + ".weight"], w[L + n + ".bias"] = rnd((c,), 0.05, 1.0), rnd((c,), 0.02)
        w[L + "mlp.fc1.weight"], w[L + "mlp.fc1.bias"] = rnd((m, c), c ** -0.5), rnd((m,), 0.02)
        w[L + "mlp.fc2.weight"], w[L + "mlp.fc2.bias"] = rnd((c, m), 0.5 * m ** -0.5), rnd((c,), 0.02)
    w[TM + "final_layer_norm.weight"], w[TM + "final_layer_norm.bias"] = rnd((c,), 0.05, 1.0), rnd((c,), 0.02)
    if cfg.projection_dim:
        w["text_projection.weight"] = rnd((cfg.projection_dim, c), c ** -0.5)
    return w


HOT_CHANNELS = (5, 77)
HOT_BOS, HOT_POS = 256.0, 8192.0


def make_hot(w, cfg):
    """The "massive activation" pattern of trained CLIP towers, which synthetic weights lack: the BOS embedding row times 256 and two
    fixed channels of the position table times 4096 (powers of two: the parameters stay fp16-representable).  Every row of the
    residual stream then carries two channels of magnitude about 50 among channels of magnitude about 0.4, and row 0 is large
    throughout (tests/test_text_lpips_units_cpu.py measures the ratio)."""
    w = dict(w)
    tok, pos = w[TM + "embeddings.token_embedding.weight"].clone(), w[TM + "embeddings.position_embedding.weight"].clone()
    tok[cfg.bos_token_id] *= HOT_BOS
    pos[:, list(HOT_CHANNELS)] *= HOT_POS
    w[TM + "embeddings.token_embedding.weight"], w[TM + "embeddings.position_embedding.weight"] = tok, pos
    assert torch.equal(tok.half().float(), tok) and torch.equal(pos.half().float(), pos)
    return w


def make_ids(cfg, eos_at, seed=11):
    """[len(eos_at), 77] prompts: BOS, random word ids, EOS at the given position, pad ids behind it."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, cfg.bos_token_id - 1, (len(eos_at), SEQ), generator=g)
    ids[:, 0] = cfg.bos_token_id
    for b, n in enumerate(eos_at):
        assert 1 <= n < SEQ
        ids[b, n] = cfg.eos_token_id
        ids[b, n + 1:] = cfg.pad_token_id
    return ids


def eos_rows(cfg, ids):
    """transformers' rule for the pooled token: legacy configs (eos id 2) take the argmax of the ids, all others the first EOS."""
    ids = ids.to(torch.int64)
    pos = ids.argmax(dim=-1) if cfg.eos_token_id == 2 else (ids == cfg.eos_token_id).int().argmax(dim=-1)
    return torch.arange(ids.shape[0]) * ids.shape[1] + pos


# ---------------------------------------------------------------------------------------------------------------- CLIP: units
def clip_units(cfg):
    """[(name, kind, inputs)] of a tower program in emission order - what ``_CLIPProgram.marks`` must list.  ``penultimate`` is the
    copy of the last layer's input and stands where it is emitted: in front of that layer."""
    units, at = [("embed", "embed", ("ids",))], "embed"
    for i in range(cfg.num_hidden_layers):
        if i == cfg.num_hidden_layers - 1:
            units.append(("penultimate", "penultimate", (at,)))
        units.append((f"L{i}.qkv", "qkv", (at,)))
        units.append((f"L{i}.attn", "attn", (f"L{i}.qkv",)))
        units.append((f"L{i}.out", "out", (f"L{i}.attn", at)))
        at = f"L{i}.out"
        units.append((f"L{i}.fc1", "fc1", (at,)))
        units.append((f"L{i}.fc2", "fc2", (f"L{i}.fc1", at)))
        at = f"L{i}.fc2"
    if cfg.projection_dim:
        units.append(("pooled", "pooled", (at, "ids")))
    return units


def layer_norm(ev, x, p, eps):
    return ev.q(F.layer_norm(x, (x.shape[-1],), ev.w[p + ".weight"], ev.w[p + ".bias"], eps))


def causal_attention(ev, qkv, B, heads):
    """qkv [B * 77, 3 C] -> [B * 77, C].  REF: softmax(Q K^T / 8 + causal mask) V.  MODEL: what lb_attn_fwd_d64 keeps - fp32 scores,
    p = fp16(exp(s - max)) as the second MFMA's operand, the row sum over those rounded p, O / sum stored fp16."""
    M, C3 = qkv.shape
    C = C3 // 3
    q, k, v = (t.reshape(B, SEQ, heads, HEAD_DIM).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    s = q @ k.transpose(-1, -2) * HEAD_DIM ** -0.5
    mask = torch.ones(SEQ, SEQ, dtype=torch.bool).tril(CAUSAL_DIAGONAL)
    s = s.masked_fill(~mask, float("-inf"))
    if not ev.store:
        o = torch.softmax(s, dim=-1) @ v
    else:
        p = ev.q(torch.exp(s - s.amax(dim=-1, keepdim=True)))
        o = (p @ v) / p.sum(dim=-1, keepdim=True)
    return ev.q(o.transpose(1, 2).reshape(M, C))


def activation(cfg, x):
    return x * torch.sigmoid(1.702 * x) if cfg.hidden_act == "quick_gelu" else F.gelu(x)


def fc1_pre(ev, cfg, i, x):
    """The pre-activation of layer ``i``'s fc1: Linear(LayerNorm 2 (x)) - in MODEL mode it is never stored (the activation is the
    GEMM's epilogue)."""
    L = f"{TM}encoder.layers.{i}."
    return F.linear(layer_norm(ev, ev.t(x), L + "layer_norm2", cfg.layer_norm_eps), ev.w[L + "mlp.fc1.weight"], ev.w[L + "mlp.fc1.bias"])


def quick_gelu_fit(out, pre64, e_rms):
    """The quick-GELU constant an fc1 output was computed with, as a least-squares shift from 1.702, and the bound the shift is held to.
    A constant of 1.7 moves an output by at most 3e-4 - x^2 s (1 - s) * 0.002 with s = sigmoid(1.702 x), largest near |x| = 1.4 - which
    is less than the rounding of one fp16 store, so no element-wise bound can see it.  But it moves every output the same way, along
    g = d out / d k = x^2 s (1 - s), while rounding errors have no preferred sign: the projection dk = <out - ref, g> / <g, g> of errors
    that are independent with zero mean and rms ``e_rms`` has standard deviation e_rms / |g|.  -> (dk, 6 e_rms / |g|)."""
    s = torch.sigmoid(1.702 * pre64)
    g = pre64 * pre64 * s * (1 - s)
    err = out.detach().cpu().double() - pre64 * s
    return float((err * g).sum() / (g * g).sum()), 6.0 * e_rms / float(g.norm())


def clip_unit(ev, cfg, name, kind, ins):
    """Evaluate one unit.  ``ins``: its inputs in the order ``clip_units`` lists them (``ids``: [B, 77] integers; hidden states
    [B * 77, C])."""
    w, eps = ev.w, cfg.layer_norm_eps
    if kind == "embed":
        ids = ins[0].to(torch.int64)
        tok, pos = w[TM + "embeddings.token_embedding.weight"], w[TM + "embeddings.position_embedding.weight"]
        return ev.q(tok[ids.reshape(-1)] + pos[torch.arange(SEQ).repeat(ids.shape[0])])
    if kind == "penultimate":
        x = ev.t(ins[0])
        return x.reshape(-1, SEQ, x.shape[-1])
    if kind == "pooled":
        h, ids = ev.t(ins[0]), ins[1]
        fin = layer_norm(ev, h[eos_rows(cfg, ids)], TM + "final_layer_norm", eps)
        return ev.q(F.linear(fin, w["text_projection.weight"]))
    i = int(name[1:name.index(".")])
    L = f"{TM}encoder.layers.{i}."
    x = ev.t(ins[0])
    if kind == "qkv":
        W = torch.cat([w[L + f"self_attn.{n}_proj.weight"] for n in ("q", "k", "v")], 0)
        b = torch.cat([w[L + f"self_attn.{n}_proj.bias"] for n in ("q", "k", "v")], 0)
        return ev.q(F.linear(layer_norm(ev, x, L + "layer_norm1", eps), W, b))
    if kind == "attn":
        return causal_attention(ev, x, x.shape[0] // SEQ, cfg.num_attention_heads)
    if kind == "out":
        return ev.q(F.linear(x, w[L + "self_attn.out_proj.weight"], w[L + "self_attn.out_proj.bias"]) + ev.t(ins[1]))
    if kind == "fc1":
        return ev.q(activation(cfg, fc1_pre(ev, cfg, i, x)))
    if kind == "fc2":
        return ev.q(F.linear(x, w[L + "mlp.fc2.weight"], w[L + "mlp.fc2.bias"]) + ev.t(ins[1]))
    raise KeyError(kind)


def clip_forward(ev, cfg, ids):
    """Free-running: every unit on the outputs of the units before it -> {unit name: output}."""
    out = {"ids": ids}
    for name, kind, ins in clip_units(cfg):
        out[name] = clip_unit(ev, cfg, name, kind, [out[i] for i in ins])
    del out["ids"]
    return out


# ---------------------------------------------------------------------------------------------------------------- LPIPS
LP_SHIFT, LP_SCALE = (-.030, -.088, -.188), (.458, .448, .450)
LPIPS_TAPS = [f"conv{i + 1}" for i in range(5)]


def lpips_units():
    """[(name, inputs)]: conv1 reads the uint8 frames (prep is part of it: ``features`` returns no prep tensor), every other conv the
    tap before it (through the exact max-pool in front of conv2 and conv3)."""
    return [("conv1", ("frames",))] + [(f"conv{i + 1}", (f"conv{i}",)) for i in range(1, 5)]


def lpips_prep(ev, frames_u8):
    """[N, H, W, 3] uint8 -> [N, 3, H, W]: ((2 x / 255 - 1) - shift) / scale; MODEL in the fp32 operation order of lpips_prep_kernel
    (2.f * x / 255.f - 1.f, minus the shift, divided by the scale), stored fp16."""
    x = frames_u8.detach().cpu().permute(0, 3, 1, 2).to(ev.dt)
    shift, scale = (torch.tensor(LP_SHIFT, dtype=ev.dt).view(1, 3, 1, 1), torch.tensor(LP_SCALE, dtype=ev.dt).view(1, 3, 1, 1))
    return ev.q(((2.0 * x / 255.0 - 1.0) - shift) / scale)


def lpips_unit(ev, name, x, pool=3):
    """One conv unit.  ``x``: the uint8 frames [N, H, W, 3] for conv1, else the previous tap, NCHW."""
    i = int(name[4:]) - 1
    _, _, _, stride, pad = R.LPIPS_CONVS[i]
    h = lpips_prep(ev, x) if i == 0 else ev.t(x)
    if i in (1, 2):
        h = F.max_pool2d(h, pool, 2)
    return ev.q(F.relu(R._conv(h, ev.w, f"net.conv{i + 1}", stride=stride, pad=pad)))


def lpips_forward(ev, frames_u8):
    """Free-running trunk -> the five taps, NCHW."""
    taps, h = [], frames_u8
    for name, _ in lpips_units():
        h = lpips_unit(ev, name, h)
        taps.append(h)
    return taps


def lpips_tap_terms(ev, ta, tb):
    """The five addends of the distance of one pair: taps NCHW [1, C, H, W] (or [C, H, W]) -> tensor [5] of ``ev``'s type."""
    terms = []
    for i, (fa, fb) in enumerate(zip(ta, tb)):
        fa, fb = ev.t(fa), ev.t(fb)
        c = fa.shape[-3]
        na = fa / (fa.pow(2).sum(-3, keepdim=True).sqrt() + 1e-10)
        nb = fb / (fb.pow(2).sum(-3, keepdim=True).sqrt() + 1e-10)
        lin = ev.w[f"lin{i}.weight"].view(c, 1, 1)
        terms.append(((na - nb).pow(2) * lin).sum(-3).mean())
    return torch.stack(terms)


def lpips_chain(HW, C):
    """The longest serial chain of fp32 additions behind one tap's addend in lpips_tap_kernel / lpips_fold_kernel: a lane adds C / 64
    channel terms, the wave sum adds 6 levels, the wave adds one pixel after another - ceil(HW / (4 nblk)) of them, nblk =
    min(ceil(HW / 4), 128) blocks of 4 waves - and 4 more cover the block's four waves and the addition into the accumulator (the
    sum over blocks is taken in double)."""
    nblk = min((HW + 3) // 4, 128)
    return C // 64 + math.ceil(HW / (4 * nblk)) + 6 + 4


def lpips_distance_bound(terms64, shapes):
    """sum over taps of (L + 16) * 2^-24 * ref: every addend is non-negative, so a sum of n terms rounded at every step is within
    n * 2^-24 of its exact value, relatively; 16 covers the per-element arithmetic in front of the sums (two squares, the square root,
    the reciprocal, two products, the difference, its square, the product with ``lin``: 9 roundings) and the final scaling.
    ``shapes``: [(HW, C)] per tap."""
    return sum((lpips_chain(hw, c) + 16) * 2.0 ** -24 * float(t) for t, (hw, c) in zip(terms64, shapes))


def smooth_frames(n, H, W, seed):
    """``n`` smooth uint8 frames [n, H, W, 3]: low-pass-filtered noise over a gradient, plus a little texture."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        coarse = torch.rand(1, 3, H // 32 + 2, W // 32 + 2, generator=g)
        img = F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False)[0]
        ramp = torch.linspace(0, 1, W).view(1, 1, W) * 0.3 + torch.linspace(0, 1, H).view(1, H, 1) * 0.2
        tex = F.avg_pool2d(torch.rand(1, 3, H + 2, W + 2, generator=g), 3, 1)[0] * 0.12
        out.append(((img * 0.6 + ramp + tex).clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0))
    return torch.stack(out)


def lerp_u8(a, b, f):
    return (a.float() * (1 - f) + b.float() * f).round().clamp(0, 255).to(torch.uint8)


def nudge(frame):
    """``frame`` with every 97th byte + 1 (255 stays): a near-identical neighbour."""
    flat = frame.clone().reshape(-1)
    flat[::97] = (flat[::97].to(torch.int16) + 1).clamp(max=255).to(torch.uint8)
    return flat.view_as(frame)


def tap_nchw(tap, H, W):
    """A native tap [N, H W, C] -> NCHW on the CPU."""
    t = tap.detach().cpu()
    return t.view(t.shape[0], H, W, t.shape[-1]).permute(0, 3, 1, 2).contiguous()


def lpips_geometry(H, W):
    """[(Hin, Win, Hout, Wout, C)] of the five convs for an H x W frame (input size after the pool, where there is one)."""
    out, h, w = [], H, W
    for i, (_, cout, k, stride, pad) in enumerate(R.LPIPS_CONVS):
        if i in (1, 2):
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        out.append((h, w, ho, wo, cout))
        h, w = ho, wo
    return out
