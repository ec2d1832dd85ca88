"""Native SDXL ControlNet: structure guidance for the UNet programs.

Architecture = diffusers ``ControlNetModel`` as published for SDXL (key names included): the UNet's encoder and mid block over again
(``conv_in``, ``time_embedding``, ``add_embedding``, ``down_blocks.*``, ``mid_block.*``), a small conv stack that embeds the control
image at IMAGE resolution down to the latent grid (``controlnet_cond_embedding``), and one 1x1 "zero conv" per UNet skip plus one
for the mid block (``controlnet_down_blocks.k``, ``controlnet_mid_block``).

    h = conv_in(sample) + cond_embedding(hint);  the encoder runs as in the UNet, collecting h_k after conv_in, after every resnet
    (and its transformer) and after every downsampler;  then the mid block.
    residual_k = scale * zero_k(h_k),  residual_mid = scale * zero_mid(h_mid)

The UNet adds residual_k to its SKIP COPIES only (the hidden state that continues down its encoder is not changed) and residual_mid
to its mid block's output.  What is MI355X-specific here:

* the encoder is packed and emitted by the UNet's own code (``unet.EncoderPacking``, ``UNetProgram._emit_encoder``): fused ``temb_proj``,
  hoisted ``ctx_kv``, LayerNorm-folded copies under the same ``fuse_layernorm`` rule;
* zero conv AND add are ONE GEMM epilogue, in place on the UNet's skip (``UNetProgram._emit_control_adds``): no residual tensor
  exists; the conditioning scale is baked into the packed zero-conv weights (``fp16(scale W)``, ``scale b``, formed in float64), and
  ``set_scale`` rewrites those small tensors in place under live programs and graphs;
* the hint embedding depends on neither latent nor timestep: a program of its own per picture size (``HintProgram``), run once per
  control image.

RESTATED, NOT PINNED: neither diffusers nor a ControlNet checkpoint is available offline, so the key list is written from the published
format and guarded structurally (``check_state``: every key consumed, unknown keys and misfit shapes refused).
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ..hip import lib
from .geometry import check_unet_latent_size, latent_hw
from .runtime import Program, RecordedProgram, F16, F32
from .unet import CTX_PAD, EncoderPacking, UNetProgram, _Side
from .weights import DictProvider, Packer, pad_to


@dataclass
class ControlNetConfig:
    in_channels: int = 4
    block_channels: Tuple[int, ...] = (320, 640, 1280)      # must equal the UNet's: the residuals fit its skips
    layers_per_block: int = 2                               # must equal the UNet's
    transformer_depth: Tuple[int, ...] = (0, 2, 10)         # the ControlNet's own (the published "small" / "mid" ones have fewer)
    head_dim: int = 64
    cross_dim: int = 2048
    pooled_dim: int = 1280
    add_time_dim: int = 256
    norm_groups: int = 32
    cond_channels: int = 3
    cond_embed_channels: Tuple[int, ...] = (16, 32, 96, 256)

    @property
    def time_embed_dim(self) -> int:
        return self.block_channels[0] * 4

    @property
    def add_in_dim(self) -> int:
        return self.pooled_dim + 6 * self.add_time_dim

    @classmethod
    def for_unet(cls, unet_cfg, transformer_depth=None, **kw) -> "ControlNetConfig":
        """The config that fits a UNet (``unet_cfg``: anything with the UNet config's fields); ``transformer_depth`` defaults to its."""
        return cls(in_channels=unet_cfg.in_channels, block_channels=tuple(unet_cfg.block_channels), layers_per_block=unet_cfg.layers_per_block,
                   transformer_depth=tuple(transformer_depth if transformer_depth is not None else unet_cfg.transformer_depth),
                   head_dim=unet_cfg.head_dim, cross_dim=unet_cfg.cross_dim, pooled_dim=unet_cfg.pooled_dim,
                   add_time_dim=unet_cfg.add_time_dim, norm_groups=unet_cfg.norm_groups, **kw)

    @classmethod
    def from_diffusers(cls, d: dict) -> "ControlNetConfig":
        """From the ``config.json`` of a diffusers SDXL ``ControlNetModel``.  What this implementation does not do is refused by name."""
        ch = tuple(int(c) for c in d.get("block_out_channels", (320, 640, 1280)))
        for key, want in (("addition_embed_type", "text_time"), ("class_embed_type", None), ("global_pool_conditions", False),
                          ("only_cross_attention", False), ("use_linear_projection", True), ("upcast_attention", (None, False)),
                          ("resnet_time_scale_shift", "default"), ("encoder_hid_dim", None)):
            have = d.get(key, want[0] if isinstance(want, tuple) else want)
            if have not in (want if isinstance(want, tuple) else (want,)):
                raise ValueError(f"ControlNetConfig.from_diffusers: {key} = {have!r} is not supported (expected {want!r})")
        depth = d.get("transformer_layers_per_block", 1)
        depth = tuple(int(v) for v in depth) if isinstance(depth, (list, tuple)) else (int(depth),) * len(ch)
        types = d.get("down_block_types")
        if types is not None:               # a level without cross-attention has no transformer, whatever the depth list says
            depth = tuple(v if "CrossAttn" in t else 0 for v, t in zip(depth, types))
        heads = d.get("attention_head_dim", 8)          # (diffusers' historic name: for SDXL it holds the number of HEADS per level)
        heads = tuple(int(v) for v in heads) if isinstance(heads, (list, tuple)) else (int(heads),) * len(ch)
        head_dims = {c // h for c, h, v in zip(ch, heads, depth) if v} | {ch[-1] // heads[-1]}
        if len(head_dims) != 1:
            raise ValueError(f"ControlNetConfig.from_diffusers: the levels' head dimensions differ ({sorted(head_dims)})")
        add_time = int(d.get("addition_time_embed_dim", 256))
        return cls(in_channels=int(d.get("in_channels", 4)), block_channels=ch, layers_per_block=int(d.get("layers_per_block", 2)),
                   transformer_depth=depth, head_dim=head_dims.pop(), cross_dim=int(d.get("cross_attention_dim", 2048)),
                   pooled_dim=int(d.get("projection_class_embeddings_input_dim", 2816)) - 6 * add_time, add_time_dim=add_time,
                   norm_groups=int(d.get("norm_num_groups", 32)), cond_channels=int(d.get("conditioning_channels", 3)),
                   cond_embed_channels=tuple(int(c) for c in d.get("conditioning_embedding_out_channels", (16, 32, 96, 256))))


def check_cfg_fits(cfg: ControlNetConfig, unet_cfg) -> None:
    """The residuals must fit the UNet's skips and both networks read the same conditioning: ``ValueError`` names the first field that differs."""
    for f in ("in_channels", "block_channels", "layers_per_block", "head_dim", "cross_dim", "pooled_dim", "add_time_dim"):
        if tuple(np.atleast_1d(getattr(cfg, f))) != tuple(np.atleast_1d(getattr(unet_cfg, f))):
            raise ValueError(f"ControlNet does not fit the UNet: {f} = {getattr(cfg, f)} vs {getattr(unet_cfg, f)}")


def skip_channels(cfg) -> List[int]:
    ch = cfg.block_channels
    skips = [ch[0]]
    for bi, c in enumerate(ch):
        skips += [c] * cfg.layers_per_block
        if bi < len(ch) - 1:
            skips.append(c)
    return skips


def hint_convs(cfg) -> List[Tuple[str, int, int, int, bool]]:
    """[(name, cin, cout, stride, silu)] of ``controlnet_cond_embedding``: conv_in, blocks 0 .. 2 n - 3 (pairs: c -> c, then c -> next
    at stride 2), conv_out (no activation)."""
    e, p = cfg.cond_embed_channels, "controlnet_cond_embedding."
    out = [(p + "conv_in", cfg.cond_channels, e[0], 1, True)]
    for i in range(len(e) - 1):
        out.append((f"{p}blocks.{2 * i}", e[i], e[i], 1, True))
        out.append((f"{p}blocks.{2 * i + 1}", e[i], e[i + 1], 2, True))
    out.append((p + "conv_out", e[-1], cfg.block_channels[0], 1, False))
    return out


def expected_keys(cfg: ControlNetConfig) -> Dict[str, Tuple[int, ...]]:
    """Every key of a diffusers ControlNet state dict of this config -> its shape, in the order the model lists them.  Written from the
    published format, independently of the packing code (``NativeControlNet._load`` must consume exactly these: ``check_state``)."""
    k: Dict[str, Tuple[int, ...]] = {}
    ch, T, X = cfg.block_channels, cfg.time_embed_dim, cfg.cross_dim

    def lin(n, cin, cout, bias=True):
        k[n + ".weight"] = (cout, cin)
        if bias:
            k[n + ".bias"] = (cout,)

    def conv(n, cin, cout, ks):
        k[n + ".weight"], k[n + ".bias"] = (cout, cin, ks, ks), (cout,)

    def norm(n, c):
        k[n + ".weight"], k[n + ".bias"] = (c,), (c,)

    def resnet(p, cin, cout):
        norm(p + ".norm1", cin)
        conv(p + ".conv1", cin, cout, 3)
        lin(p + ".time_emb_proj", T, cout)
        norm(p + ".norm2", cout)
        conv(p + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(p + ".conv_shortcut", cin, cout, 1)

    def transformer(p, c, depth):
        norm(p + ".norm", c)
        lin(p + ".proj_in", c, c)
        for d in range(depth):
            b = f"{p}.transformer_blocks.{d}"
            norm(b + ".norm1", c)
            for nm in ("to_q", "to_k", "to_v"):
                lin(f"{b}.attn1.{nm}", c, c, bias=False)
            lin(b + ".attn1.to_out.0", c, c)
            norm(b + ".norm2", c)
            lin(b + ".attn2.to_q", c, c, bias=False)
            lin(b + ".attn2.to_k", X, c, bias=False)
            lin(b + ".attn2.to_v", X, c, bias=False)
            lin(b + ".attn2.to_out.0", c, c)
            norm(b + ".norm3", c)
            lin(b + ".ff.net.0.proj", c, 8 * c)
            lin(b + ".ff.net.2", 4 * c, c)
        lin(p + ".proj_out", c, c)

    conv("conv_in", cfg.in_channels, ch[0], 3)
    lin("time_embedding.linear_1", ch[0], T)
    lin("time_embedding.linear_2", T, T)
    lin("add_embedding.linear_1", cfg.add_in_dim, T)
    lin("add_embedding.linear_2", T, T)
    for name, cin, cout, _, _ in hint_convs(cfg):
        conv(name, cin, cout, 3)
    prev = ch[0]
    for bi, c in enumerate(ch):
        for li in range(cfg.layers_per_block):
            resnet(f"down_blocks.{bi}.resnets.{li}", prev, c)
            if cfg.transformer_depth[bi]:
                transformer(f"down_blocks.{bi}.attentions.{li}", c, cfg.transformer_depth[bi])
            prev = c
        if bi < len(ch) - 1:
            conv(f"down_blocks.{bi}.downsamplers.0.conv", c, c, 3)
    for i, c in enumerate(skip_channels(cfg)):
        conv(f"controlnet_down_blocks.{i}", c, c, 1)
    conv("controlnet_mid_block", ch[-1], ch[-1], 1)
    resnet("mid_block.resnets.0", ch[-1], ch[-1])
    transformer("mid_block.attentions.0", ch[-1], cfg.transformer_depth[-1])
    resnet("mid_block.resnets.1", ch[-1], ch[-1])
    return k


def check_state(cfg: ControlNetConfig, state: Dict[str, torch.Tensor]) -> None:
    """The structural guard of a loaded state dict: a key the config does not list, a listed key that is missing, or a shape that
    does not fit raises (``KeyError`` / ``ValueError``), naming the first few."""
    want = expected_keys(cfg)
    unknown = sorted(set(state) - set(want))
    if unknown:
        raise KeyError(f"ControlNet state dict: {len(unknown)} keys this config does not have ({unknown[:4]} ...)")
    missing = [n for n in want if n not in state]
    if missing:
        raise KeyError(f"ControlNet state dict: {len(missing)} keys are missing ({missing[:4]} ...)")
    for n, shape in want.items():
        if tuple(state[n].shape) != shape:
            raise ValueError(f"ControlNet state dict: '{n}' has shape {tuple(state[n].shape)}, expected {shape}")


def hint_tensor(image, size_hw: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """A control image - PIL image or uint8 [H, W, 3] - as the fp32 NHWC tensor [1, H, W, 3] in [0, 1] diffusers' control image
    processor makes of it (resized with LANCZOS to ``size_hw`` when it has another size; NOT normalised to +-1)."""
    from PIL import Image
    if isinstance(image, Image.Image):
        image = image.convert("RGB")
        if size_hw is not None and image.size != (size_hw[1], size_hw[0]):
            image = image.resize((size_hw[1], size_hw[0]), Image.LANCZOS)
        arr = np.asarray(image, dtype=np.uint8)
    else:
        arr = np.asarray(image.cpu() if torch.is_tensor(image) else image)
        if arr.ndim != 3 or arr.shape[-1] != 3 or arr.dtype != np.uint8:
            raise ValueError(f"control image: expected a PIL image or a uint8 [H, W, 3] picture (got {arr.dtype} {arr.shape})")
        if size_hw is not None and tuple(arr.shape[:2]) != tuple(size_hw):
            arr = np.asarray(Image.fromarray(arr).resize((size_hw[1], size_hw[0]), Image.LANCZOS), dtype=np.uint8)
    return torch.from_numpy(arr.copy()).to(torch.float32)[None] / 255.0


class NativeControlNet(EncoderPacking):
    def __init__(self, cfg: ControlNetConfig, provider, device="cuda", fuse_layernorm="auto", scale: float = 1.0):
        """``fuse_layernorm``: as for ``NativeUNet`` - and the same value as the UNet it guides (``check_fits``), for the step program
        decides the LayerNorm form once for both networks.  ``scale``: the conditioning scale baked into the zero convs."""
        if len(cfg.cond_embed_channels) < 1 or cfg.cond_channels > 8:
            raise ValueError(f"ControlNetConfig: cond_channels {cfg.cond_channels} / cond_embed_channels {cfg.cond_embed_channels} not supported")
        self._init_packing(cfg, device, fuse_layernorm)
        self.scale = float(scale)
        self._zero_host: Dict[str, torch.Tensor] = {}          # the unscaled zero-conv weights and biases (float64, host)
        self._load(provider)

    @classmethod
    def from_dir(cls, path: str, device="cuda", **kw) -> "NativeControlNet":
        """A diffusers ControlNet folder: ``config.json`` plus ``*.safetensors``."""
        with open(os.path.join(path, "config.json")) as f:
            cfg = ControlNetConfig.from_diffusers(json.load(f))
        return cls.from_safetensors(path, cfg, device=device, **kw)

    @classmethod
    def from_safetensors(cls, path: str, cfg: ControlNetConfig, device="cuda", **kw) -> "NativeControlNet":
        from .weights import from_safetensors
        return cls.from_state_dict(from_safetensors(path).state, cfg, device=device, **kw)

    @classmethod
    def from_state_dict(cls, state: Dict[str, torch.Tensor], cfg: ControlNetConfig, device="cuda", **kw) -> "NativeControlNet":
        check_state(cfg, state)
        return cls(cfg, DictProvider(state), device=device, **kw)

    def check_fits(self, unet) -> None:
        check_cfg_fits(self.cfg, unet.cfg)
        if self.fuse_layernorm != unet.fuse_layernorm:
            raise ValueError(f"ControlNet packed with fuse_layernorm={self.fuse_layernorm!r}, the UNet with {unet.fuse_layernorm!r}")
        if self.device != unet.device:
            raise ValueError("ControlNet and UNet live on different devices")

    # ------------------------------------------------------------------ weights -----------
    def _zero(self, pk, name, c):
        w = pk.pv.weight(name + ".weight", (c, c, 1, 1), c, 0.5).reshape(c, c).to(torch.float64)
        b = pk.pv.bias(name + ".bias", c).to(torch.float64)
        self._zero_host[name + ".weight"], self._zero_host[name + ".bias"] = w, b
        self.w[name + ".weight"] = pk.dev((self.scale * w).to(torch.float16), F16)
        self.w[name + ".bias"] = pk.dev(self.scale * b, F32)

    def _load(self, pv):
        cfg, pk = self.cfg, Packer(pv, self.w, self.device)
        temb_acc = {"w": [], "b": [], "n": 0}
        ctx_acc = {"k": [], "v": [], "n": 0}
        self._load_encoder(pk, temb_acc, ctx_acc)
        for name, cin, cout, _, _ in hint_convs(cfg):
            pk.conv(name, cin, cout, 3)
        for i, c in enumerate(self.skip_channels()):
            self._zero(pk, f"controlnet_down_blocks.{i}", c)
        self._zero(pk, "controlnet_mid_block", cfg.block_channels[-1])
        if ctx_acc["n"]:
            self._load_fused(pk, temb_acc, ctx_acc)
        else:                           # no cross-attention block anywhere: no fused context projection
            self.w["temb_proj.weight"] = pk.dev(torch.cat(temb_acc["w"], 0), F16)
            self.w["temb_proj.bias"] = pk.dev(torch.cat(temb_acc["b"], 0), F32)
            self.n_temb, self.n_ctx = temb_acc["n"], 0

    def set_scale(self, scale: float) -> None:
        """Rewrite the zero convs at ``scale`` IN PLACE (``Reloadable``'s path: synchronise, ``copy_`` into the live tensors): no
        ``data_ptr()`` changes, no program is dropped, an instantiated graph replays against the new values."""
        self.scale = float(scale)
        fresh = {k: ((self.scale * t).to(torch.float16) if k.endswith(".weight") else (self.scale * t).to(torch.float32)).to(self.device)
                 for k, t in self._zero_host.items()}
        self._write_live(fresh)

    # ------------------------------------------------------------------ programs ----------
    def build_hint(self, size_hw, ragged_halo: bool = True, journal: bool = False, wrap: int = 0) -> "HintProgram":
        return HintProgram(self, size_hw, ragged_halo=ragged_halo, journal=journal, wrap=wrap)

    def build(self, B: int, L, ragged_halo: bool = True, journal: bool = False, wrap: int = 0) -> "ControlNetProgram":
        """The ControlNet ALONE, residuals as tensors: what the diffusers-style ``pipe.controlnet(...)`` facade runs.  The native
        loops never do - their step programs hold both networks (``NativeUNet.build(..., control=net)``)."""
        return ControlNetProgram(self, B, L, ragged_halo=ragged_halo, journal=journal, wrap=wrap)


class HintProgram(RecordedProgram):
    """``controlnet_cond_embedding`` for ONE picture of ``size_hw`` = (H, W) pixels, multiples of 2^(stride-2 convs): 3x3 convs, each
    followed by SiLU (in the conv's epilogue) but the last; the output ``emb`` [1, h, w, C0] has the latent grid's size.  ``wrap``
    applies to every conv (a tileable render wants a hint embedded on the same cylinder / torus)."""

    def __init__(self, net: NativeControlNet, size_hw, ragged_halo: bool = True, journal: bool = False, wrap: int = 0):
        H, W = latent_hw(size_hw)
        convs = hint_convs(net.cfg)
        f = 2 ** sum(1 for c in convs if c[3] == 2)
        if H % f or W % f or H <= 0 or W <= 0:
            raise ValueError(f"HintProgram: the picture size {W} x {H} is no multiple of {f}")
        super().__init__(net, 1, (H, W), ragged_halo=ragged_halo, journal=journal, wrap=wrap)
        cfg, dev = net.cfg, net.device
        self.image = torch.zeros(1, H, W, pad_to(cfg.cond_channels, 8), dtype=F16, device=dev)     # NHWC, channels padded with zeros
        self.emb = torch.zeros(1, H // f, W // f, cfg.block_channels[0], dtype=F16, device=dev)
        self.prog = Program("control-hint")
        with self._recording(self.prog):
            em, w, ar = self.em, net.w, self.arena
            h, sh, sw, at = self.image, H, W, "image"
            for i, (name, cin, cout, stride, silu) in enumerate(convs):
                g = lib.ConvGeom(sh, sw, pad_to(cin, 8), 3, 3, stride=stride, pad=1)
                last = i == len(convs) - 1
                out = self.emb if last else ar.alloc((1, g.Hout, g.Wout, pad_to(cout, 4)))
                em.gemm(h, w[name + ".weight"], out, M=g.M(1), bias=w[name + ".bias"], flags=lib.GEMM_SILU if silu else 0, conv=g)
                if h is not self.image:
                    ar.release(h)
                h, sh, sw = out, g.Hout, g.Wout
                at = self._mark("control." + name, "hint_conv", h, at)

    @torch.no_grad()
    def embed(self, hint: torch.Tensor) -> torch.Tensor:
        """``hint`` [1, H, W, 3] in [0, 1] (``hint_tensor``) -> the program-owned ``emb`` [1, h, w, C0] fp16."""
        c = self.net.cfg.cond_channels
        if tuple(hint.shape) != (1, self.H, self.W, c):
            raise ValueError(f"HintProgram.embed: the hint is {tuple(hint.shape)}, expected {(1, self.H, self.W, c)}")
        self.image[..., :c].copy_(hint.to(self.image.device, F16))
        self.prog.launch()
        return self.emb


class ControlNetProgram(UNetProgram):
    """The ControlNet alone for a fixed (batch, latent size): ``forward`` returns the scaled residuals as program-owned NHWC tensors
    (``down`` in ``skip_channels()`` order, ``mid``).  A ``UNetProgram`` in everything but what its step program holds - the
    ControlNet's encoder and mid block, then the zero convs written out of place - so ``set_conditioning``, ``set_hint`` and
    ``capture`` are the UNet program's."""

    def __init__(self, net: NativeControlNet, B: int, L, ragged_halo: bool = True, journal: bool = False, wrap: int = 0):
        RecordedProgram.__init__(self, net, B, L, ragged_halo=ragged_halo, journal=journal, wrap=wrap)
        cfg, dev, H, W = net.cfg, net.device, self.H, self.W
        check_unet_latent_size(H, W, len(cfg.block_channels))
        self.ln_mode = net.fuse_layernorm if net.fuse_layernorm != "auto" else (B * max(H // 4, 1) * max(W // 4, 1) <= 1024)
        self.x_in = torch.zeros(B, cfg.in_channels, H, W, dtype=F16, device=dev)
        self.tvals = torch.zeros(B, 1, dtype=F32, device=dev)
        self.time_ids = torch.zeros(B, 6, dtype=F32, device=dev)
        self.ctx = torch.zeros(B, CTX_PAD, cfg.cross_dim, dtype=F16, device=dev)
        self.text_embeds = torch.zeros(B, cfg.pooled_dim, dtype=F16, device=dev)
        self.timestep_cond, self.control = None, None
        self.hint_emb = torch.zeros(B, H, W, cfg.block_channels[0], dtype=F16, device=dev)
        side = _Side(net, "control.", torch.zeros(B, cfg.time_embed_dim, dtype=F16, device=dev),
                     torch.zeros(B * CTX_PAD, 2 * net.n_ctx, dtype=F16, device=dev) if net.n_ctx else None)
        self.side = self._unet_side = side
        self.prog_cond, self.prog_step = Program("control-cond"), Program("control-step")
        with self._recording(self.prog_cond):
            self._emit_cond(side)
        with self._recording(self.prog_step):
            skips, h, at, _, _ = self._emit_encoder(side, residual=self.hint_emb)
            em, ar, w = self.em, self.arena, net.w
            self.down: List[torch.Tensor] = []
            for k, (hk, c, k_at) in enumerate(skips):
                out = torch.zeros_like(hk)
                em.gemm(hk, w[f"controlnet_down_blocks.{k}.weight"], out, M=hk.numel() // c, bias=w[f"controlnet_down_blocks.{k}.bias"])
                ar.release(hk)
                self.down.append(out)
                self._mark(f"control.zero.{k}", "zero", out, k_at)
            self.mid = torch.zeros_like(h)
            c = cfg.block_channels[-1]
            em.gemm(h, w["controlnet_mid_block.weight"], self.mid, M=h.numel() // c, bias=w["controlnet_mid_block.bias"])
            ar.release(h)
            self._mark("control.zero.mid", "zero", self.mid, at)

    def forward(self, x_in: torch.Tensor, tvals: torch.Tensor):
        self.x_in.copy_(x_in)
        self.tvals.copy_(tvals.reshape(-1, 1).to(F32))
        self.prog_step.launch()
        return self.down, self.mid
