"""Float64 reference and storage model of the native SDXL VAE encoder (tests/test_vae_encoder_cpu.py, tests/test_vae_encoder_gpu.py).

``AutoencoderKL.encode`` restated from the oracle's own primitives (``oracle.sdxl_ref``: ``_conv``, ``_gn``, ``resnet_block``, ``_lin``,
``attention``) - the CPU test pins this restatement against the latent-diffusion encoder ``transformers`` ships - and the same encoder
unit by unit in the two modes of tests/_model_units.py (``Ev``): REF (float64, nothing rounded) and MODEL (float32 with a rounding
wherever the program stores).  Feature maps are NCHW here.

``encode_ref`` takes *mutations* - the bugs most likely to be written - so that the CPU test can show each of them falls outside the
bound the GPU tests hold the native encoder to.
"""
import copy

import torch
import torch.nn.functional as F

import _model_units as MU
from oracle import sdxl_ref as R

F16, F32, F64 = torch.float16, torch.float32, torch.float64
A_ENC, A_DEC = "encoder.mid_block.attentions.0", "decoder.mid_block.attentions.0"


# ---------------------------------------------------------------------------------------------------------------- enumeration
def encoder_spec(cfg: R.VAECfg) -> R._Spec:
    """The encoder's parameters in layer order, HF ``AutoencoderKL`` key names (``encoder.*``, ``quant_conv.*``)."""
    s = R._Spec()
    ch = cfg.block_channels
    top, mc = ch[-1], 2 * cfg.latent_channels
    s.conv("encoder.conv_in", cfg.out_channels, ch[0], 3)
    prev = ch[0]
    for bi, c in enumerate(ch):
        for li in range(cfg.layers_per_block):
            R._resnet_spec(s, f"encoder.down_blocks.{bi}.resnets.{li}", prev, c, None)
            prev = c
        if bi < len(ch) - 1:
            s.conv(f"encoder.down_blocks.{bi}.downsamplers.0.conv", c, c, 3)
    R._resnet_spec(s, "encoder.mid_block.resnets.0", top, top, None)
    s.norm(A_ENC + ".group_norm", top)
    for nm in ("to_q", "to_k", "to_v"):
        s.linear(f"{A_ENC}.{nm}", top, top)
    s.linear(A_ENC + ".to_out.0", top, top, gain=0.5)
    R._resnet_spec(s, "encoder.mid_block.resnets.1", top, top, None)
    s.norm("encoder.conv_norm_out", top)
    s.conv("encoder.conv_out", top, mc, 3, gain=0.5)
    s.conv("quant_conv", mc, mc, 1)
    return s


def encoder_units(cfg):
    """[(name, kind, inputs)] of an encode program - what ``VAEEncoderProgram.marks`` must list."""
    units, at = [("conv_in", "conv_in", ("x_in",))], "conv_in"

    def add(name, kind):
        nonlocal at
        units.append((name, kind, (at,)))
        at = name

    n = len(cfg.block_channels)
    for bi in range(n):
        for li in range(cfg.layers_per_block):
            add(f"encoder.down_blocks.{bi}.resnets.{li}", "resnet")
        if bi < n - 1:
            add(f"encoder.down_blocks.{bi}.downsamplers.0.conv", "downsample")
    add("encoder.mid_block.resnets.0", "resnet")
    add("mid_attention", "mid_attention")
    add("encoder.mid_block.resnets.1", "resnet")
    add("moments", "out")
    return units


def encoder_tap_names(cfg):
    n = len(cfg.block_channels)
    taps = {"mid": "encoder.mid_block.resnets.1"}
    for bi in range(n):
        taps[f"down{bi}"] = f"encoder.down_blocks.{bi}.downsamplers.0.conv" if bi < n - 1 else \
            f"encoder.down_blocks.{bi}.resnets.{cfg.layers_per_block - 1}"
    return taps


def picture(u8):
    """uint8 [B, H, W, 3] -> the encoder's input as the program stages it: f16(fp32(u8) / 127.5 - 1), NCHW."""
    return (u8.to(F32) / 127.5 - 1.0).to(F16).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------- the restatement
def downsample(x, w, p, pad="br"):
    """``pad``: "br" = one zero row at the bottom and one zero column at the right (the encoder); the mutants: "sym" = pad 1 on
    every side (stride 2: the same output size), "tl" = the zero row on top and the zero column at the left."""
    if pad == "sym":
        return F.conv2d(x, w[p + ".weight"], w[p + ".bias"], stride=2, padding=1)
    return F.conv2d(F.pad(x, (0, 1, 0, 1) if pad == "br" else (1, 0, 1, 0)), w[p + ".weight"], w[p + ".bias"], stride=2)


def encode_ref(cfg, w, x, taps=None, dtype=F32, pad="br", eps=1e-6, quant=True, swap=False):
    """x [B, 3, H, W] in [-1, 1] -> ``moments`` [B, 8, H / 8, W / 8] (mean | logvar), unscaled.  ``taps``: ``down0`` .. and ``mid``.
    The keyword arguments are the mutations (defaults: the encoder)."""
    g = cfg.norm_groups
    w = {k: v.to(dtype) for k, v in w.items()}
    ch = cfg.block_channels
    h = R._conv(x.to(dtype), w, "encoder.conv_in")
    for bi in range(len(ch)):
        for li in range(cfg.layers_per_block):
            h = R.resnet_block(h, None, w, f"encoder.down_blocks.{bi}.resnets.{li}", g, eps)
        if bi < len(ch) - 1:
            h = downsample(h, w, f"encoder.down_blocks.{bi}.downsamplers.0.conv", pad)
        if taps is not None:
            taps[f"down{bi}"] = h
    h = R.resnet_block(h, None, w, "encoder.mid_block.resnets.0", g, eps)
    B, C, H, W = h.shape
    n = R._gn(h, w, A_ENC + ".group_norm", g, eps).view(B, C, H * W).transpose(1, 2)
    att = R.attention(R._lin(n, w, A_ENC + ".to_q"), R._lin(n, w, A_ENC + ".to_k"), R._lin(n, w, A_ENC + ".to_v"), 1)
    h = h + R._lin(att, w, A_ENC + ".to_out.0").transpose(1, 2).reshape(B, C, H, W)
    h = R.resnet_block(h, None, w, "encoder.mid_block.resnets.1", g, eps)
    if taps is not None:
        taps["mid"] = h
    h = R._conv(F.silu(R._gn(h, w, "encoder.conv_norm_out", g, eps)), w, "encoder.conv_out")
    if quant:
        h = R._conv(h, w, "quant_conv", pad=0)
    if swap:
        h = torch.cat(list(reversed(h.chunk(2, dim=1))), dim=1)
    return h


def latents_of(cfg, moments, scale=True):
    """UNet latents: ``mode()`` (the mean half) times the scaling factor."""
    mean = moments.chunk(2, dim=1)[0]
    return mean * cfg.scaling_factor if scale else mean


def sample_ref(moments64, eps64):
    """``DiagonalGaussianDistribution.sample`` in float64, channels on dim 1."""
    mean, logvar = moments64.chunk(2, dim=1)
    return mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * eps64


# ---------------------------------------------------------------------------------------------------------------- units
def folded_moments_weights(w, fold="f64"):
    """``quant_conv`` folded into ``encoder.conv_out`` as the loader folds it: W' = Wq Wout, b' = Wq bout + bq in float64, the weight
    rounded ONCE to fp16 (the bias stays fp32).  ``fold="f16"`` is the mutant: the same products and sums in fp16 arithmetic, a rounding
    after every multiply and every add."""
    wo, bo = w["encoder.conv_out.weight"].double(), w["encoder.conv_out.bias"].double()
    wq, bq = w["quant_conv.weight"].double().flatten(1), w["quant_conv.bias"].double()
    if fold == "f64":
        return torch.einsum("om,mcyx->ocyx", wq, wo).to(F16).double(), (wq @ bo + bq).to(F32).double()
    r = lambda t: t.to(F16).double()
    acc_w, acc_b = torch.zeros(wq.shape[0], *wo.shape[1:], dtype=F64), r(bq)
    for m in range(wq.shape[1]):
        acc_w = r(acc_w + r(wq[:, m, None, None, None] * wo[m][None]))
        acc_b = r(acc_b + r(wq[:, m] * bo[m]))
    return acc_w, acc_b


def moments_unit(ev, cfg, x, fold="f64"):
    """conv_norm_out + SiLU -> conv_out -> quant_conv.  REF: literally that.  MODEL: the folded conv on the fp16 GroupNorm output,
    an fp32 store."""
    n = MU.gn(ev, x, "encoder.conv_norm_out", cfg.norm_groups, 1e-6, True)
    if not ev.store:
        return R._conv(R._conv(n, ev.w, "encoder.conv_out"), ev.w, "quant_conv", pad=0)
    wf, bf = folded_moments_weights(ev.w, fold)
    return F.conv2d(n, wf.to(ev.dt), bf.to(ev.dt), padding=1)


def downsample_unit(ev, x, p, scaled, pad="br"):
    """REF: literally ``F.pad`` + ``conv2d``.  MODEL: the conv reads the raw stream as an fp16 operand carrying the 2^-4 scale (the
    scaled stream as it is; a cast of the fp32 stream) and stores to the stream."""
    return ev.q_stream(downsample(ev.q_scaled(x), ev.w, p, pad), scaled)


def latents_unit(ev, cfg, moments, scale=True):
    """``latents`` from the fp32 moments: fp16(mean * scaling_factor) - one multiply in fp32, one rounding."""
    return ev.q(latents_of(cfg, ev.t(moments), scale))


def _as_decoder_attention(ev):
    """``MU.vae_mid_attention`` reads its weights under the decoder's prefix: the same evaluation with the encoder's in their place."""
    alias = copy.copy(ev)
    alias.w = {A_DEC + k[len(A_ENC):]: v for k, v in ev.w.items() if k.startswith(A_ENC)}
    return alias


def encoder_unit(ev, cfg, name, kind, ins, scaled, one_launch=False):
    """Evaluate one encoder unit.  ``ins``: [the picture NCHW fp16 values] for ``conv_in``, else [the stream, NCHW, real units]."""
    x = ev.t(ins[0])
    if kind == "conv_in":
        return ev.q_stream(R._conv(x, ev.w, "encoder.conv_in"), scaled)
    if kind == "resnet":
        return MU.vae_resnet(ev, cfg, name, x, scaled)
    if kind == "mid_attention":
        return MU.vae_mid_attention(_as_decoder_attention(ev), cfg, x, scaled, one_launch)
    if kind == "downsample":
        return downsample_unit(ev, x, name, scaled)
    if kind == "out":
        return moments_unit(ev, cfg, x)                       # moments_f32: an fp32 store
    raise KeyError(kind)


def free_run(ev, cfg, x, scaled=True, one_launch=False):
    """Every unit fed with the outputs of the same evaluation: name -> output, plus ``latents``."""
    out = {"x_in": x}
    for name, kind, ins in encoder_units(cfg):
        out[name] = encoder_unit(ev, cfg, name, kind, [out[i] for i in ins], scaled, one_launch)
    out["latents"] = latents_unit(ev, cfg, out["moments"])
    return out
