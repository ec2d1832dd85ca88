"""``NativeSDXLPipe`` — the SDXL pipeline object of the MI355X path.

It is two things at once:

1. a **duck-typed diffusers pipeline** (SURVEY.md Appendix A): every attribute the reference's
   ``DiffusersHolder`` touches exists with the same meaning (``unet(...)``, ``scheduler``,
   ``vae.decode``, ``encode_prompt``, ``prepare_latents``, ``image_processor`` ...), so the
   unchanged reference host code can drive it step by step.  The class is named
   ``StableDiffusionXLPipeline`` because the reference dispatches on that class name
   (/root/reference/latentblending/diffusers_holder.py:41);
2. the **native fast path** (``is_lb_native``) used by ``latentblending_amd.DiffusersHolder``: the
   whole restartable denoising loop for one branch or a BATCH of branches — crossfeed slerps,
   input scaling, UNet program, CFG + Euler(-ancestral) update — with device-resident state and
   one recorded launch program per UNet forward; VAE decode to uint8 frames on device; LPIPS on
   device frames with cached features.

Text encoders: CLIP weights/vocabularies are not available offline, so ``encode_prompt`` returns
seeded synthetic embeddings of the right shapes unless ``text_encoder_fn`` is supplied
(the step before the hot path).
"""
from __future__ import annotations

import os
import warnings
import zlib
from collections import OrderedDict
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from ..hip import ops
from ..hip.lib import api
from .frames import DeviceImage
from .geometry import latent_hw, program_key, check_tileable, TILEABLE_WRAP
from .lpips import NativeLPIPS
from ..planner import noise_draws_per_run
from .noise import CounterNoise
from .scheduler import make_scheduler
from .unet import NativeUNet, UNetConfig, UNetProgram
from .controlnet import ControlNetConfig, ControlNetProgram, HintProgram, NativeControlNet, check_cfg_fits, hint_tensor
from .tiny_vae import NativeTinyVAEDecoder, NativeTinyVAEEncoder, TinyEncoderProgram, TinyVAEConfig, TinyVAEProgram
from .vae import NativeVAEDecoder, NativeVAEEncoder, VAEConfig, VAEEncoderProgram, VAEProgram, sample_moments
from ..replay import lora_entries
from .lora import COMPONENTS, TEXT_KEY_PREFIXES, LoRARecord, load_state, read_lora
from .weights import LoRAProvider, SyntheticProvider

F16, F32 = torch.float16, torch.float32
NOISE_MODES = ("stream", "counter")


class _Adapter:
    """One loaded LoRA adapter: its normalised record, its scale, and the path it came from (None for a state dict)."""

    def __init__(self, record: LoRARecord, scale: float, path):
        self.record, self.scale, self.path = record, scale, path


def _synthetic_embedding(text: str, shape, salt: int) -> torch.Tensor:
    g = torch.Generator().manual_seed((zlib.crc32(text.encode()) + 7919 * salt) & 0x7FFFFFFF)
    return torch.randn(shape, generator=g, dtype=torch.float32)


class _UNetFacade:
    def __init__(self, pipe):
        self._pipe = pipe
        c = pipe.unet_cfg
        self.config = SimpleNamespace(sample_size=c.sample_size, in_channels=c.in_channels,
                                      time_cond_proj_dim=c.time_cond_proj_dim)

    def __call__(self, sample, timestep, encoder_hidden_states=None, timestep_cond=None,
                 cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False,
                 down_block_additional_residuals=None, mid_block_additional_residual=None):
        """``down_block_additional_residuals`` / ``mid_block_additional_residual`` (NCHW, what ``pipe.controlnet`` returns): added to
        the skip copies and to the mid block's output (``UNetProgram.forward_with_residuals``; always on the PLAIN program)."""
        pipe = self._pipe
        if self.config.time_cond_proj_dim is not None and timestep_cond is None:
            raise ValueError("NativeSDXLPipe.unet: this UNet is guidance-embedded (time_cond_proj_dim = "
                             f"{self.config.time_cond_proj_dim}); timestep_cond is required "
                             "(pipe.get_guidance_scale_embedding(guidance_scale - 1, embedding_dim=time_cond_proj_dim))")
        B, _, H, W = sample.shape
        prog = pipe.unet_program(B, (H, W), control=False)
        prog.set_conditioning(encoder_hidden_states, added_cond_kwargs["text_embeds"],
                              added_cond_kwargs["time_ids"],
                              timestep_cond=None if timestep_cond is None else timestep_cond.to(sample.device, F16))
        t = torch.as_tensor(timestep, dtype=F32).reshape(-1).expand(B)
        if down_block_additional_residuals is None and mid_block_additional_residual is None:
            return (prog.forward(sample.to(F16), t.to(sample.device)).clone(),)
        nhwc = lambda r: r.to(pipe.device, F16).permute(0, 2, 3, 1).contiguous()          # noqa: E731
        down = [nhwc(r) for r in (down_block_additional_residuals or ())]
        mid = None if mid_block_additional_residual is None else nhwc(mid_block_additional_residual)
        return (prog.forward_with_residuals(sample.to(F16), t.to(sample.device), down, mid).clone(),)


class _ControlNetFacade:
    """diffusers' ``ControlNetModel`` call on the pipe's loaded ControlNet: ``(down_block_res_samples, mid_block_res_sample)`` in NCHW.
    ``controlnet_cond``: [B or 1, 3, H, W] in [0, 1] (the FIRST picture serves every sample: the native programs hold one hint)."""

    def __init__(self, pipe):
        self._pipe = pipe

    @property
    def config(self):
        net = self._pipe._require_controlnet("pipe.controlnet")
        return SimpleNamespace(conditioning_channels=net.cfg.cond_channels, global_pool_conditions=False)

    @torch.no_grad()
    def __call__(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale=1.0,
                 added_cond_kwargs=None, guess_mode=False, return_dict=False, **_):
        pipe = self._pipe
        net = pipe._require_controlnet("pipe.controlnet")
        if guess_mode:
            raise NotImplementedError("pipe.controlnet: guess mode is not implemented")
        if controlnet_cond is None:
            raise ValueError("pipe.controlnet: controlnet_cond is required")
        B, _, H, W = sample.shape
        pipe.set_control_scale(conditioning_scale)
        cond = controlnet_cond[:1].to(pipe.device, F32).permute(0, 2, 3, 1)
        emb = pipe._hint_program((int(cond.shape[1]), int(cond.shape[2]))).embed(cond)
        prog = pipe._controlnet_program(B, (H, W))
        prog.set_hint(emb)
        prog.set_conditioning(encoder_hidden_states, added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"])
        t = torch.as_tensor(timestep, dtype=F32).reshape(-1).expand(B)
        down, mid = prog.forward(sample.to(F16), t.to(sample.device))
        nchw = lambda r: r.permute(0, 3, 1, 2).contiguous()          # noqa: E731
        out = ([nchw(d) for d in down], nchw(mid))
        return out if not return_dict else SimpleNamespace(down_block_res_samples=out[0], mid_block_res_sample=out[1])


class _VAEFacade:
    def __init__(self, pipe):
        self._pipe = pipe
        self.dtype = F16
        self.post_quant_conv = SimpleNamespace(parameters=lambda: iter([torch.zeros(1, dtype=F16)]))

    @property
    def config(self):
        """Of the pipe's ACTIVE decoder: the tiny decoder takes the latents as they are (scaling_factor 1.0)."""
        return SimpleNamespace(force_upcast=False, scaling_factor=self._pipe.active_vae_cfg.scaling_factor)

    def decode(self, z, return_dict=False):
        """z = latents / scaling_factor -> float image [B,3,H,W] (diffusers convention)."""
        prog = self._pipe.vae_program(z.shape[0], (z.shape[-2], z.shape[-1]))
        prog.decode((z.float() * self._pipe.active_vae_cfg.scaling_factor).to(F16))
        return (prog.image_f32[..., :3].permute(0, 3, 1, 2).clone(),)

    @torch.no_grad()
    def encode(self, x, return_dict=True):
        """x [B, 3, H, W] in [-1, 1], any float dtype (diffusers convention) -> an object with ``latent_dist`` (``.mean``,
        ``.logvar``, ``.mode()``, ``.sample(generator=None)``, NCHW fp32 in UNSCALED units: multiply by the SDXL VAE's
        ``scaling_factor``).  Always the full ``AutoencoderKL`` encoder, whatever ``pipe.encoder`` says."""
        pipe = self._pipe
        f = pipe.vae_cfg.scale_factor
        B, _, H, W = x.shape
        if H % f or W % f:
            raise ValueError(f"vae.encode: the picture size {W} x {H} is no multiple of {f}")
        prog = pipe.vae_encoder_program(B, (H // f, W // f))
        prog.encode_normalized(x.to(pipe.device))
        out = SimpleNamespace(latent_dist=_LatentDist(prog.moments().clone()))
        return out if return_dict else (out.latent_dist,)

    def to(self, *a, **k):
        return self


class _LatentDist:
    """diffusers' ``DiagonalGaussianDistribution`` over the fp32 moments [B, h, w, 2 C] of one encode (channels last: mean |
    logvar); what it hands out is NCHW fp32, unscaled.  The sample is computed in torch (``vae.sample_moments``): the clamp, ``exp``
    and a ``randn`` on the device from the generator."""

    def __init__(self, moments: torch.Tensor):
        self._moments = moments

    @staticmethod
    def _nchw(t):
        return t.permute(0, 3, 1, 2).contiguous()

    @property
    def mean(self):
        return self._nchw(self._moments.chunk(2, dim=-1)[0])

    @property
    def logvar(self):
        return self._nchw(torch.clamp(self._moments.chunk(2, dim=-1)[1], -30.0, 20.0))

    def mode(self):
        return self.mean

    def sample(self, generator=None):
        B, h, w, c2 = self._moments.shape          # (eps is drawn in NCHW order, as diffusers' randn_tensor(mean.shape) draws it)
        eps = torch.randn((B, c2 // 2, h, w), generator=generator, device=self._moments.device, dtype=self._moments.dtype)
        return self._nchw(sample_moments(self._moments, eps=eps.permute(0, 2, 3, 1)))


class _ImageProcessor:
    @staticmethod
    def postprocess(image, output_type="pil"):
        x = image.permute(0, 2, 3, 1).contiguous()
        if x.shape[-1] < 4:
            x = torch.cat([x, torch.zeros_like(x[..., :1])], dim=-1).contiguous()
        if output_type == "np":     # diffusers' VaeImageProcessor: denormalise + clamp, float32 HWC, NOT quantised (diffusers_holder.py:141)
            return [f.cpu().numpy() for f in (x[..., :3].float() / 2 + 0.5).clamp(0, 1)]
        u8 = ops.postprocess_u8(x.float())
        return [DeviceImage(f) for f in u8]


class StableDiffusionXLPipeline:
    is_lb_native = True

    def __init__(self, turbo: bool = True, unet_cfg: Optional[UNetConfig] = None,
                 vae_cfg: Optional[VAEConfig] = None, unet_provider=None, vae_provider=None,
                 lpips_provider=None, device="cuda", seed: int = 0, name_or_path: Optional[str] = None,
                 text_encoder_fn=None, unet_native: Optional[NativeUNet] = None,
                 vae_native: Optional[NativeVAEDecoder] = None, allow_synthetic: Optional[bool] = None,
                 scheduler: Optional[str] = None, decoder: str = "full", tiny_vae_provider=None,
                 tiny_vae_native: Optional[NativeTinyVAEDecoder] = None, noise: str = "stream", encoders=None, loras=None,
                 encoder: str = "tiny", vae_encoder_native: Optional[NativeVAEEncoder] = None, tileable=None, controlnet=None):
        """``controlnet``: a ControlNet loaded right after construction (``load_controlnet``: a ``NativeControlNet``, a
        ``ControlNetConfig`` - seeded synthetic weights, announced -, a provider, a ``(config, provider)`` pair or the path of a
        diffusers ControlNet folder); None (default): none - and with one loaded, nothing changes until ``set_control_image``.
        ``tileable``: seamless renders - None / False / "" (default) = off; "x" = the left and right edges of a frame join (a 360
        degree strip), "y" = top and bottom, "xy" (or True) = all four (a tileable texture); anything else raises ``ValueError``.
        Every 3x3 conv, downsampler and upsampler of the UNet and of the active decoder (full or tiny) then pads by wrap-around
        instead of zeros (``ConvGeom.wrap``), which makes the networks functions on a cylinder / torus: the zero padding is the
        only position cue they have.  The ENCODERS (image anchors) and the LPIPS metric stay zero-padded: a picture one anchors on
        need not tile, and the metric is the metric.  ``pipe.tileable`` switches it afterwards (the cached UNet / decoder programs
        are dropped); a pipe that never sets it records the programs it always recorded.
        ``loras``: [(src, scale), ...] = LoRA adapters loaded right after construction, in order (``load_lora``).
        ``encoders``: a ``clip.NativeTextEncoders``; its ``encode`` becomes ``text_encoder_fn`` (unless one is given) and, when it
        carries the providers its towers were packed from, LoRA adapters reach the text towers too.  Adapters are merged from the
        providers the pipe was built with (``unet_provider``, ``encoders.providers``): a pipe given a ready-made ``unet_native``
        needs the provider that UNet was packed from beside it (``unet_provider=``) before ``load_lora`` can touch it.
        ``noise``: "stream" (default) = per-step sampler noise (Euler-ancestral, LCM) drawn from a generator, as ever - the value an
        element receives depends on the draws before it; "counter" = counter-based noise (``native/noise.py``): every value is a
        function of (trajectory, step, element), so a seed renders the same whatever batch, order or rank serves the draw.
        ``pipe.noise`` switches it afterwards.  The START latents stay host-seeded under both.
        ``decoder``: "full" (default) = the SDXL ``AutoencoderKL`` decoder; "tiny" = the TAESDXL tiny decoder (``native/tiny_vae.py``:
        a speed / preview option - a distilled approximation, its LPIPS tree is computed on its own frames).  Case-insensitive,
        anything else raises ``ValueError``; ``pipe.decoder`` switches it afterwards (preview tiny, render full).  The tiny network
        is built on first use from ``tiny_vae_native`` / ``tiny_vae_provider`` (``native.from_safetensors(<dir>/taesdxl)``), else
        from the seeded synthetic stand-in (announced like the others).  The same provider serves the TAESDXL ENCODER
        (``native_image2latent``: pictures -> latents, whatever ``decoder`` says), built on first use as well.
        ``encoder``: what ``native_image2latent`` (image anchors) encodes pictures with: "tiny" (default) = the TAESDXL encoder, as ever;
        "full" = the SDXL ``AutoencoderKL`` encoder (``native/vae.py``: ``vae.encode(x).latent_dist.mode() * scaling_factor``, the
        autoencoder the full decoder belongs to).  Case-insensitive, anything else raises ``ValueError``; ``pipe.encoder`` switches
        it afterwards.  The full encoder is built on first use from ``vae_encoder_native`` or from ``vae_provider`` (the ``encoder.*``
        / ``quant_conv.*`` keys of the same ``vae/*.safetensors``); with neither a provider nor a ``vae_native`` it is the seeded
        synthetic stand-in (announced like the others).  A ready-made ``vae_native`` WITHOUT ``vae_provider`` raises ``ValueError``
        there: a real decoder is never paired with a synthetic encoder silently.
        ``scheduler``: None or "euler" = the reference pipes' choice (Euler-ancestral for Turbo, Euler for base); "ddim" = diffusers'
        DDIMScheduler (eta 0) behind the same native loops - also with ``turbo=True`` (the Turbo guidance / branching defaults
        stay, only the sampler changes: deterministic, "leading" spacing); "lcm" = the latent-consistency sampler (diffusers'
        LCMScheduler: few-step sampling of a distilled UNet or a merged LCM-LoRA, 1..50 steps, one noise draw per step but the
        last), with ``turbo=True`` and ``False`` alike; "dpmpp_2m" / "dpmpp_2m_karras" = DPM-Solver++ 2M (second-order multistep,
        diffusers' DPMSolverMultistepScheduler with its dpmsolver++ / midpoint defaults) on uniform / Karras sigmas (commonly run at about
        20 steps; at most 44 on Karras sigmas).  Case-insensitive; anything else raises ``ValueError``
        (a misspelt "DDIM " or a scheduler object used to fall through to Euler silently).
        ``allow_synthetic``: seeded synthetic stand-ins (UNet / VAE / LPIPS weights when no provider is given,
        prompt embeddings when no ``text_encoder_fn`` is given) are used silently when True (tests, bench: also
        ``LB_ALLOW_SYNTHETIC=1``); otherwise each stand-in announces itself ONCE with a ``UserWarning`` - frames
        rendered from them are noise-like and prompts have no semantic effect."""
        # (a bad name is refused before anything else - also on a machine without a device; the reference's SDXL pipes carry Euler /
        # Euler-ancestral schedulers, the other names are this pipe's own)
        self.scheduler = make_scheduler(scheduler, turbo, torch.device(device))
        self._decoder = self._check_decoder(decoder)
        self._encoder = self._check_encoder(encoder)
        self._tileable = self._check_tileable(tileable)
        self._vae_provider, self._vae_seed = vae_provider, seed + 1
        self._vae_native_given = vae_native is not None
        self.vae_encoder_native = vae_encoder_native
        if self._encoder == "full":
            self._full_encoder_source()
        if not torch.cuda.is_available():
            raise RuntimeError("NativeSDXLPipe needs an MI355X (HIP device); there is no CPU fallback")
        self.device = torch.device(device)
        self._execution_device = self.device
        # (already packed modules may be shared between pipes: 5.5 GB of UNet weights need not be packed twice)
        self.unet_cfg = unet_native.cfg if unet_native is not None else (unet_cfg or UNetConfig(sample_size=64 if turbo else 128))
        self.vae_cfg = vae_native.cfg if vae_native is not None else (vae_cfg or VAEConfig())
        self._name_or_path = name_or_path or ("stabilityai/sdxl-turbo" if turbo else
                                              "stabilityai/stable-diffusion-xl-base-1.0")
        self.dtype = F16
        self.allow_synthetic = bool(allow_synthetic) if allow_synthetic is not None else os.environ.get("LB_ALLOW_SYNTHETIC") == "1"
        self._warned = set()
        if unet_native is None and unet_provider is None:
            self._synthetic_notice("UNet weights", "pass unet_provider=native.from_safetensors(<dir>/unet) or set LB_WEIGHTS_DIR")
        if vae_native is None and vae_provider is None:
            self._synthetic_notice("VAE weights", "pass vae_provider=native.from_safetensors(<dir>/vae) or set LB_WEIGHTS_DIR")
        if lpips_provider is None:
            self._synthetic_notice("LPIPS-Alex weights (the branch-insertion metric is then NOT LPIPS)",
                                   "pass lpips_provider=native.lpips_provider(alexnet_state_dict, lpips_lin_state_dict)")
        # the base providers LoRA adapters are merged from (load_lora); None = a ready-made module whose provider nobody named
        self._unet_provider = unet_provider if (unet_native is not None or unet_provider is not None) else SyntheticProvider(seed)
        self.encoders = encoders
        self._loras: "OrderedDict[str, _Adapter]" = OrderedDict()
        self.unet_native = unet_native or NativeUNet(self.unet_cfg, self._unet_provider, self.device)
        self.vae_native = vae_native or NativeVAEDecoder(self.vae_cfg, vae_provider or SyntheticProvider(seed + 1), self.device)
        self.lpips_metric = NativeLPIPS(lpips_provider or SyntheticProvider(7), self.device)
        self.tiny_vae_native, self._tiny_vae_provider, self._tiny_seed = tiny_vae_native, tiny_vae_provider, seed + 2
        self.tiny_vae_cfg = tiny_vae_native.cfg if tiny_vae_native is not None else TinyVAEConfig()
        self.unet = _UNetFacade(self)
        self.vae = _VAEFacade(self)
        self.image_processor = _ImageProcessor()
        self.vae_scale_factor = self.vae_cfg.scale_factor
        self.default_sample_size = self.unet_cfg.sample_size
        self.text_encoder_2 = None
        self.text_encoder_fn = text_encoder_fn if (text_encoder_fn is not None or encoders is None) else encoders.encode
        self._guidance_scale = 0.0 if turbo else 5.0
        self._guidance_rescale = 0.0
        self._clip_skip = None
        self._cross_attention_kwargs = None
        self._denoising_end = None
        self._interrupt = False
        self._num_timesteps = 0
        # recorded launch programs, keyed by geometry.program_key: (batch, latent side) or (batch, latent height, latent width); each owns its activation arena (+ hipGraph), so the
        # caches are LRU-bounded: speculative rounds of varying width must not pile up SDXL-sized arenas
        self._unet_programs: "OrderedDict[Tuple[int, ...], UNetProgram]" = OrderedDict()
        self._vae_programs: "OrderedDict[Tuple[int, ...], VAEProgram]" = OrderedDict()
        self._tiny_vae_programs: "OrderedDict[Tuple[int, ...], TinyVAEProgram]" = OrderedDict()     # (decoder="tiny": same bound)
        # the tiny decoder's 64 -> 64 convs ask for the LDS-resident-weights kernel (LB_GEMM_C64) where tiny_vae.use_c64 says so;
        # False = the library's own routing everywhere (A/B runs, tests).  Read when a program is BUILT: the setter drops the
        # cached tiny programs.
        self._tiny_conv_c64 = True
        # the TAESDXL encoder (native_image2latent): built on first use from the tiny decoder's provider; its programs are cached
        # like the tiny decoder's and dropped by the same switch
        self.tiny_vae_encoder_native: Optional[NativeTinyVAEEncoder] = None
        self._tiny_encoder_programs: "OrderedDict[Tuple[int, ...], TinyEncoderProgram]" = OrderedDict()
        self._vae_encoder_programs: "OrderedDict[Tuple[int, ...], VAEEncoderProgram]" = OrderedDict()  # (encoder="full" / vae.encode)
        self.vae_encodes = 0                # pictures encoded by native_image2latent
        side = self.unet_cfg.sample_size * self.vae_cfg.scale_factor
        self.render_size = (side, side)     # (H, W) of the pictures this pipe is rendering: what prepare_latents was last asked for
        # non-square programs send 3x3 convs whose level does not divide into halo tiles to the ragged-tile form of the halo kernel
        # (geometry.use_ragged_halo); False = the implicit GEMM there (A/B runs, tests).  Read when a program is BUILT: the
        # setter drops the cached non-square programs.
        self._ragged_halo = True
        self.max_cached_programs = 8
        self._embed_cache: OrderedDict = OrderedDict()           # text -> (prompt_embeds, pooled); cleared when the encoder changes
        self._use_graphs = False
        self._feat_scratch: Dict[int, list] = {}
        self.stats = {"unet_forwards": 0, "unet_samples": 0, "vae_decodes": 0, "slerps": 0, "lpips_pairs": 0}
        self._side_stream = None            # lazily created: conditioning programs of big batches run here beside the small anchor steps
        self._noise = "stream"
        self.noise = noise
        # ControlNet (load_controlnet / set_control_image): the controlled UNet programs live in a cache of their own, so the plain
        # programs - and everything a pipe without a hint does - stay what they were
        self._seed = seed
        self.controlnet_native: Optional[NativeControlNet] = None
        self.controlnet = _ControlNetFacade(self)
        self._control_hint: Optional[torch.Tensor] = None       # the control image as given ([1, H0, W0, 3] uint8 on the host), or None
        self._control_scale = 1.0
        self._control_emb: Dict[Tuple[int, int], torch.Tensor] = {}     # latent (H, W) -> the embedded hint (one size at a time)
        self._control_programs: "OrderedDict[Tuple[int, ...], UNetProgram]" = OrderedDict()
        self._controlnet_programs: "OrderedDict[Tuple[int, ...], ControlNetProgram]" = OrderedDict()     # (the facade's)
        self._hint_programs: "OrderedDict[Tuple[int, ...], HintProgram]" = OrderedDict()
        if controlnet is not None:
            self.load_controlnet(controlnet)
        for src, scale in lora_entries(loras):
            self.load_lora(src, scale)

    # ---- ControlNet -----------------------------------------------------------------------
    def _require_controlnet(self, who: str) -> NativeControlNet:
        if self.controlnet_native is None:
            raise ValueError(f"{who}: no ControlNet is loaded (NativeSDXLPipe(controlnet=...) or pipe.load_controlnet(src))")
        return self.controlnet_native

    def _drop_control_programs(self, hint_too: bool = True) -> None:
        caches = (self._control_programs, self._controlnet_programs) + ((self._hint_programs,) if hint_too else ())
        if any(caches):
            torch.cuda.synchronize(self.device)
        for cache in caches:
            cache.clear()
        self._control_emb.clear()

    def load_controlnet(self, src) -> NativeControlNet:
        """Load a ControlNet: a ready ``NativeControlNet``; a ``ControlNetConfig`` (seeded synthetic weights, announced like the other
        stand-ins); a provider (the config that fits the UNet, the UNet's transformer depths); a ``(config, provider)`` pair; or the
        path of a diffusers ControlNet folder (``config.json`` + ``*.safetensors``).  Replaces a loaded one; a control image that is
        set stays set.  Until ``set_control_image`` nothing the pipe renders changes."""
        fuse = self.unet_native.fuse_layernorm
        kw = dict(device=self.device, fuse_layernorm=fuse, scale=self._control_scale)
        if isinstance(src, NativeControlNet):
            net = src
            net.set_scale(self._control_scale)
        elif isinstance(src, (str, os.PathLike)):
            net = NativeControlNet.from_dir(os.fspath(src), **kw)
        else:
            cfg, provider = src if isinstance(src, tuple) else ((src, None) if isinstance(src, ControlNetConfig) else (None, src))
            if cfg is None:
                cfg = ControlNetConfig.for_unet(self.unet_cfg)
            check_cfg_fits(cfg, self.unet_cfg)          # (before a gigabyte of weights is packed)
            if provider is None:
                self._synthetic_notice("ControlNet weights (the hint then guides nothing meaningful)",
                                       "pass controlnet=<folder of a diffusers ControlNet> or a (config, provider) pair")
                provider = SyntheticProvider(self._seed + 3)
            net = NativeControlNet(cfg, provider, **kw)
        net.check_fits(self.unet_native)
        self._drop_control_programs()
        self.controlnet_native = net
        return net

    def unload_controlnet(self) -> None:
        """Drop the ControlNet, its programs and the control image."""
        self._drop_control_programs()
        self.controlnet_native, self._control_hint = None, None

    @property
    def control_active(self) -> bool:
        """A ControlNet is loaded AND a control image is set: the native loops run the controlled programs."""
        return self.controlnet_native is not None and self._control_hint is not None

    @property
    def control_scale(self) -> float:
        return self._control_scale

    def set_control_image(self, image, scale: Optional[float] = 1.0) -> None:
        """Hold ``image`` - a PIL image or uint8 [H, W, 3] - as the hint of every UNet evaluation from now on: resized with LANCZOS to
        the render size, fp16 in [0, 1] (not normalised to +-1), the same hint for both CFG halves and every sample.  ``scale``:
        the conditioning scale (``set_control_scale``; None keeps the current one).  The hint is embedded once per render size."""
        self._require_controlnet("set_control_image")
        self._control_hint = (hint_tensor(image) * 255.0).round().to(torch.uint8)      # (validated; kept at its own size: re-embedded per render size)
        self._control_emb.clear()
        if scale is not None:
            self.set_control_scale(scale)

    def set_control_scale(self, scale: float) -> None:
        """The conditioning scale: rewritten into the packed zero convs in place - no program is dropped, graphs keep replaying."""
        scale = float(scale)
        if self.controlnet_native is not None and (scale != self._control_scale or scale != self.controlnet_native.scale):
            self.controlnet_native.set_scale(scale)
        self._control_scale = scale

    def clear_control(self) -> None:
        """No hint: the plain programs again, bit for bit (the ControlNet stays loaded, the controlled programs stay cached)."""
        self._control_hint = None
        self._control_emb.clear()

    def _hint_program(self, size_hw) -> HintProgram:
        net = self._require_controlnet("control image")

        def build():
            prog = net.build_hint(size_hw, ragged_halo=self._ragged_halo, wrap=self._wrap)
            if self._use_graphs:
                prog.enable_graphs()
            return prog
        return self._cached(self._hint_programs, program_key(1, tuple(size_hw)), build)

    def _controlnet_program(self, B: int, L) -> ControlNetProgram:
        net = self._require_controlnet("pipe.controlnet")

        def build():
            prog = net.build(B, L, ragged_halo=self._ragged_halo, wrap=self._wrap)
            if self._use_graphs:
                prog.enable_graphs()
            return prog
        return self._cached(self._controlnet_programs, program_key(B, L), build)

    def _control_embedding(self, LH: int, LW: int) -> torch.Tensor:
        """The hint embedded for a latent grid of ``LH x LW`` (a clone of the hint program's output); one size is kept - another
        render size drops the controlled programs of the old one and embeds the hint again."""
        emb = self._control_emb.get((LH, LW))
        if emb is None:
            stale = [k for k in self._control_programs if k != program_key(k[0], (LH, LW))]
            if stale:
                torch.cuda.synchronize(self.device)
            for k in stale:
                del self._control_programs[k]
            self._control_emb.clear()
            f = self.vae_scale_factor
            hint = hint_tensor(self._control_hint[0].numpy(), (LH * f, LW * f))
            emb = self._control_emb[(LH, LW)] = self._hint_program((LH * f, LW * f)).embed(hint).clone()
            for k, prog in self._control_programs.items():
                prog.set_hint(emb)
        return emb

    # ---- LoRA adapters --------------------------------------------------------------------
    @property
    def loras(self) -> "OrderedDict[str, float]":
        """Loaded adapters in load order: name -> scale."""
        return OrderedDict((n, a.scale) for n, a in self._loras.items())

    def _lora_component(self, comp: str):
        """(model, base provider, prefix of the adapters' names over the model's) of "unet" / "te1" / "te2"; the provider is None
        when the pipe was not told it, the model is None when the pipe has no such component."""
        if comp == "unet":
            return self.unet_native, self._unet_provider, ""
        enc = self.encoders
        if enc is None:
            return None, None, ""
        tower = enc.enc1 if comp == "te1" else enc.enc2
        base = None if enc.providers is None else enc.providers[0 if comp == "te1" else 1]
        return tower, base, "" if tower.prefix.endswith("text_model.") else "text_model."

    def _lora_check(self, comps) -> None:
        for comp in comps:
            net, base, _ = self._lora_component(comp)
            if comp == "unet" and base is None:
                raise ValueError("NativeSDXLPipe.load_lora: this pipe was given a ready-made unet_native without the provider it was packed "
                                 "from, so there are no base weights to merge an adapter into; pass unet_provider=<that provider> beside "
                                 "unet_native= (or let the pipe build the UNet from unet_provider=)")
            if comp != "unet" and net is None:
                raise ValueError(f"NativeSDXLPipe.load_lora: the adapter targets the text encoder '{comp}' but the pipe has no native text "
                                 "towers; pass encoders=native.NativeTextEncoders.from_dir(<dir>) (or strict=False to leave these deltas out)")
            if comp != "unet" and base is None:
                raise ValueError(f"NativeSDXLPipe.load_lora: the adapter targets the text encoder '{comp}' but encoders= carries no providers; "
                                 "build it with NativeTextEncoders(..., providers=(provider_1, provider_2)) or NativeTextEncoders.from_dir")

    def _lora_apply(self, comps) -> None:
        """Rebuild the merged provider of every component in ``comps`` from the adapters now loaded and reload that model in place."""
        for comp in comps:
            net, base, prefix = self._lora_component(comp)
            if net is None:
                continue
            adapters = [(a.record.components[comp], a.scale) for a in self._loras.values() if a.record.components[comp]]
            net.reload(LoRAProvider(base, adapters, prefix) if adapters else base)
            if comp != "unet":
                self._embed_cache.clear()               # embeddings of the towers as they were

    def load_lora(self, src, scale: float = 1.0, name: Optional[str] = None, strict: bool = True) -> str:
        """Merge the LoRA adapter ``src`` (a ``.safetensors`` file, a directory holding one, or a loaded state dict; ``lora.read_lora``
        for the accepted namings) into the UNet and the text towers it targets, at ``scale``, on top of the adapters already loaded.
        The packed weights are rewritten in place: every recorded program and instantiated graph keeps working.  Returns the
        adapter's name (``name``, else the file's stem, else ``lora<k>``).  ``strict=False``: keys that resolve to nothing, and deltas
        for text towers this pipe does not have, are left out."""
        enc = self.encoders
        state = load_state(src)
        if enc is None:             # no towers to resolve text-encoder keys against: say so (or leave them out) before anything else
            te_keys = [k for k in state if k.startswith(TEXT_KEY_PREFIXES)]
            if te_keys and strict:
                self._lora_check(("te1",))
            state = {k: v for k, v in state.items() if k not in set(te_keys)}
        rec = read_lora(state, unet_cfg=self.unet_cfg, te_cfgs=(enc.enc1.cfg, enc.enc2.cfg) if enc is not None else (None, None),
                        strict=strict)
        self._lora_check(rec.touched())
        if name is None:
            stem = os.path.splitext(os.path.basename(os.fspath(src)))[0] if isinstance(src, (str, os.PathLike)) else ""
            name, k = stem or f"lora{len(self._loras)}", 0
            while name in self._loras:
                k += 1
                name = f"{stem or 'lora'}_{k}"
        elif name in self._loras:
            raise ValueError(f"NativeSDXLPipe.load_lora: an adapter named '{name}' is loaded already ({list(self._loras)})")
        self._loras[name] = _Adapter(rec, float(scale), src if isinstance(src, (str, os.PathLike)) else None)
        try:
            self._lora_apply(rec.touched())
        except Exception:
            del self._loras[name]
            self._lora_apply(rec.touched())             # (a component reloaded before the failure goes back to what is loaded now)
            raise
        return name

    def set_lora_scale(self, name: str, scale: float) -> None:
        if name not in self._loras:
            raise KeyError(f"NativeSDXLPipe.set_lora_scale: no adapter named '{name}' ({list(self._loras)})")
        a = self._loras[name]
        if float(scale) != a.scale:
            a.scale = float(scale)
            self._lora_apply(a.record.touched())

    def unload_lora(self, name: Optional[str] = None) -> None:
        """Unload one adapter, or all (``None``): the components it touched are reloaded from the base providers and what stays."""
        if name is not None and name not in self._loras:
            raise KeyError(f"NativeSDXLPipe.unload_lora: no adapter named '{name}' ({list(self._loras)})")
        gone = [self._loras.pop(n) for n in ([name] if name is not None else list(self._loras))]
        self._lora_apply([c for c in COMPONENTS if any(c in a.record.touched() for a in gone)])

    # the names diffusers users type
    def load_lora_weights(self, path, adapter_name: Optional[str] = None, **_):
        self.load_lora(path, name=adapter_name)

    def set_adapters(self, names, adapter_weights=None) -> None:
        """diffusers' meaning: the named adapters are active at ``adapter_weights`` (default 1.0 each), every other one at 0."""
        names = [names] if isinstance(names, str) else list(names)
        weights = [1.0] * len(names) if adapter_weights is None else \
            ([float(adapter_weights)] * len(names) if isinstance(adapter_weights, (int, float)) else [float(w) for w in adapter_weights])
        if len(weights) != len(names):
            raise ValueError("set_adapters: one weight per adapter name")
        unknown = [n for n in names if n not in self._loras]
        if unknown:
            raise KeyError(f"set_adapters: no adapter named {unknown} ({list(self._loras)})")
        want = dict(zip(names, weights))
        changed = []
        for n, a in self._loras.items():
            s = want.get(n, 0.0)
            if s != a.scale:
                a.scale = s
                changed += list(a.record.touched())
        self._lora_apply([c for c in COMPONENTS if c in changed])

    def unload_lora_weights(self) -> None:
        self.unload_lora()

    def fuse_lora(self, *_a, **_k) -> None:
        """No-op: adapters are always merged into the packed weights here (there is no unfused low-rank side path to fuse)."""

    def unfuse_lora(self, *_a, **_k) -> None:
        """No-op, for the same reason: ``unload_lora_weights`` / ``set_adapters`` restore or rescale the merged weights."""

    def _synthetic_notice(self, what: str, how: str):
        if self.allow_synthetic or what in self._warned:
            return
        self._warned.add(what)
        warnings.warn(f"NativeSDXLPipe: using seeded SYNTHETIC {what} ({how}; allow_synthetic=True silences this)",
                      UserWarning, stacklevel=3)

    # ---- sampler noise ------------------------------------------------------------------
    @property
    def noise(self) -> str:
        return self._noise

    @noise.setter
    def noise(self, value):
        name = value.strip().lower() if isinstance(value, str) else value
        if name not in NOISE_MODES:
            raise ValueError(f"NativeSDXLPipe: noise must be one of {NOISE_MODES} (got {value!r})")
        if name == "counter":
            if not isinstance(self.scheduler.noise_source, CounterNoise):
                self.scheduler.noise_source = CounterNoise(self.device, scheduler=self.scheduler)
        elif isinstance(self.scheduler.noise_source, CounterNoise):
            self.scheduler.noise_source = None          # (a source the user installed is not this switch's to remove)
        self._noise = name

    @staticmethod
    def _keyed_noise(sched, noise_ids, pairs, shape1):
        """The counter-based draws ``pairs`` = [(index into ``noise_ids``, step), ...] in ONE launch: [len(pairs), *shape1[1:]]."""
        if noise_ids is None:
            raise ValueError("the scheduler's noise source is counter-based (noise='counter'): the native loops need noise_ids= "
                             "(one trajectory id per sample, native/noise.py)")
        return sched.noise_source.keyed([(int(noise_ids[s]), i) for s, i in pairs], (len(pairs),) + tuple(shape1[1:]))

    # ---- diffusers duck type ------------------------------------------------------------
    guidance_scale = property(lambda s: s._guidance_scale)
    guidance_rescale = property(lambda s: s._guidance_rescale)
    cross_attention_kwargs = property(lambda s: s._cross_attention_kwargs)

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1 and self.unet.config.time_cond_proj_dim is None

    def uses_cfg(self, guidance_scale: float) -> bool:
        return float(guidance_scale) > 1 and self.unet.config.time_cond_proj_dim is None

    @staticmethod
    def get_guidance_scale_embedding(w, embedding_dim: int = 512, dtype=torch.float32) -> torch.Tensor:
        """The guidance-scale embedding a guidance-distilled UNet takes as ``timestep_cond`` (diffusers'
        ``get_guidance_scale_embedding``; the reference's latentblending/diffusers_holder.py:303-309): ``w`` = guidance_scale - 1,
        one value per row -> [len(w), embedding_dim] = [sin(1000 w f) | cos(1000 w f)], f_i = exp(-i ln(10000) / (half - 1)),
        SIN first; one zero column pads an odd dimension.  fp32 on the host: it is tiny and per branch."""
        w = torch.as_tensor(w, dtype=torch.float32).reshape(-1).cpu() * 1000.0
        half = int(embedding_dim) // 2
        if half < 2:
            raise ValueError(f"get_guidance_scale_embedding: embedding_dim must be at least 4 (got {embedding_dim})")
        freq = torch.exp(torch.arange(half, dtype=torch.float32) * -(torch.log(torch.tensor(10000.0)) / (half - 1)))
        ang = w.to(dtype)[:, None] * freq.to(dtype)[None, :]
        emb = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
        if int(embedding_dim) % 2 == 1:
            emb = torch.nn.functional.pad(emb, (0, 1))
        return emb

    def _timestep_cond(self, guidance_scales: Sequence[float]) -> Optional[torch.Tensor]:
        """[len(guidance_scales), time_cond_proj_dim] fp16 on the device - each sample's embedding from the guidance IT runs under
        (mid-dampened guidance differs from branch to branch) - or None for a UNet that takes none."""
        dim = self.unet_cfg.time_cond_proj_dim
        if dim is None:
            return None
        w = [float(g) - 1.0 for g in guidance_scales]
        return self.get_guidance_scale_embedding(w, embedding_dim=dim).to(self.device, F16)

    def _conditioning(self, conds: Sequence[tuple], cfg: bool):
        """(context, pooled, time ids) of a UNet batch over ``conds`` = [(pos ctx, neg ctx, pos pooled, neg pooled), ...]: under CFG
        the negative half first, then the positive one."""
        ctx = torch.cat([c[0] for c in conds]).to(self.device, F16)
        pooled = torch.cat([c[2] for c in conds]).to(self.device, F16)
        if cfg:
            neg_ctx = torch.cat([c[1] for c in conds]).to(self.device, F16)
            neg_pool = torch.cat([c[3] for c in conds]).to(self.device, F16)
            ctx, pooled = torch.cat([neg_ctx, ctx]), torch.cat([neg_pool, pooled])
        time_ids = torch.tensor([self._time_ids_row()] * ctx.shape[0], dtype=F32, device=self.device)
        return ctx, pooled, time_ids

    def _launch_unet_step(self, prog, lat, params, n: int, cfg: bool, i: int, stream):
        """One UNet forward of step ``i`` over the ``n`` latents ``lat`` (scaled into the program's input; eps = ``prog.eps``)."""
        api.lb_scale_model_input_f16(lat.data_ptr(), prog.x_in.data_ptr(), params.data_ptr(), lat.numel() // n, n, int(cfg), stream)
        prog.tvals.fill_(float(self.scheduler.timesteps_np[i]))
        prog.prog_step.launch(stream)
        self.stats["unet_forwards"] += 1
        self.stats["unet_samples"] += prog.B

    @staticmethod
    def _noise_slots(noise_slots, G: int) -> Tuple[int, List[int]]:
        """(branches of the round noise is drawn for, which of them are this call's ``G``): all and every one without a farm."""
        return (G, list(range(G))) if noise_slots is None else (int(noise_slots[0]), list(noise_slots[1]))

    def _device_step(self, lat, hists, eps, params, noise, cfg: bool, i: int, carry=None, mixed: bool = True):
        """One batched scheduler step -> (latents, history, carry).  A single-step sampler has neither history nor carry (None).
        A multistep one gets a two-plane state: plane 0 the latents - AFTER any crossfeed / parental mix, which touch the latents
        only - and plane 1 the samples' previous x0 predictions.  ``carry`` is the state the previous call returned for the SAME
        batch: the kernel's contract is that ``out`` of step i is ``x`` of step i + 1, so it goes straight back in (after one copy
        of the latents into its plane 0 when they were ``mixed`` since) and nothing is allocated or gathered.  Without a carry
        (first step; a wavefront batch that just changed its size) the state is assembled from ``lat`` and ``hists`` =
        [(tensor or None, rows), ...] in batch order; a part without history (its rows are first-order rows) leaves its share of
        plane 1 unwritten - the kernel does not read it.  The latents returned are a COPY of plane 0: the loops keep them in
        trajectories, which must neither pin the x0-prediction plane nor see the carry's plane 0 overwritten by a later mix."""
        sched = self.scheduler
        if not sched.multistep:
            return sched.device_step(lat, eps, params, noise=noise, cfg=cfg, **sched.device_step_kwargs(i)), None, None
        if carry is not None:
            assert carry.shape[1:] == lat.shape
            state = carry
            if mixed:
                state[0].copy_(lat)
        else:
            state = torch.empty((2,) + tuple(lat.shape), dtype=F16, device=lat.device)
            state[0].copy_(lat)
            at = 0
            for h, rows in hists:
                if h is not None and rows:
                    state[1, at:at + rows].copy_(h)
                at += rows
            assert at == lat.shape[0]
        out = sched.device_step(state, eps, params, cfg=cfg, **sched.device_step_kwargs(i))
        return out[0].clone(), out[1], out

    def to(self, *_a, **_k):
        return self

    def upcast_vae(self):
        pass

    def prepare_extra_step_kwargs(self, generator, eta):
        return {"generator": generator}

    @property
    def text_encoder_fn(self):
        return self._text_encoder_fn

    @text_encoder_fn.setter
    def text_encoder_fn(self, fn):
        self._text_encoder_fn = fn
        cache = getattr(self, "_embed_cache", None)
        if cache is not None:
            cache.clear()                                 # embeddings of another encoder are not this one's

    def encode_prompt(self, prompt=None, prompt_2=None, device=None, num_images_per_prompt=1,
                      do_classifier_free_guidance=True, negative_prompt=None, negative_prompt_2=None, **_):
        c = self.unet_cfg

        def embed(text):
            # embedding cache keyed by the text: chained transitions re-encode the prompt they share
            hit = self._embed_cache.get(text)
            if hit is not None:
                self._embed_cache.move_to_end(text)
                return hit[0].clone(), hit[1].clone()
            if self.text_encoder_fn is not None:
                pe, pooled = self.text_encoder_fn(text)
            else:
                self._synthetic_notice("prompt embeddings (prompts have no semantic effect)",
                                       "pass text_encoder_fn=native.clip.NativeTextEncoders(...).encode")
                pe = _synthetic_embedding(text, (1, 77, c.cross_dim), 1)
                pooled = _synthetic_embedding(text, (1, c.pooled_dim), 2)
            pe, pooled = pe.to(self.device, F16), pooled.to(self.device, F16)
            self._embed_cache[text] = (pe.clone(), pooled.clone())
            while len(self._embed_cache) > 64:
                self._embed_cache.popitem(last=False)
            return pe, pooled

        text = prompt if isinstance(prompt, str) else prompt[0]
        pe, pooled = embed(text)
        if not do_classifier_free_guidance:
            return pe, None, pooled, None
        # diffusers' StableDiffusionXLPipeline.encode_prompt: zeros ONLY for ``negative_prompt is None`` (with the SDXL
        # checkpoints' force_zeros_for_empty_prompt); any given negative prompt - including the reference holder's default
        # "" (/root/reference/latentblending/diffusers_holder.py:23,87) - is tokenised and ENCODED
        if negative_prompt is None:
            return pe, torch.zeros_like(pe), pooled, torch.zeros_like(pooled)
        neg = negative_prompt[0] if isinstance(negative_prompt, (list, tuple)) else negative_prompt
        npe, npooled = embed(neg if neg is not None else "")
        return pe, npe, pooled, npooled

    def prepare_latents(self, batch, channels, height, width, dtype, device, generator, latents=None):
        """Seeded noise drawn on the HOST (so a seed means the same latent on every device and in
        the CPU oracle), scaled by the scheduler's initial sigma.  Drawn IN ``dtype`` like diffusers'
        ``randn_tensor(shape, generator, device, dtype)`` (reached from
        /root/reference/latentblending/diffusers_holder.py:98-111 with dtype = float16): on the CPU generator an fp16
        draw is a different stream from an fp32 draw that is cast afterwards."""
        self.render_size = (int(height), int(width))
        return (self._host_noise(batch, channels, height, width, dtype, generator) * self.scheduler.init_noise_sigma).to(self.device)

    def _host_noise(self, batch, channels, height, width, dtype, generator) -> torch.Tensor:
        shape = (batch, channels, height // self.vae_scale_factor, width // self.vae_scale_factor)
        host_gen = torch.Generator().manual_seed(generator.initial_seed())
        return torch.randn(shape, generator=host_gen, dtype=dtype)

    def unit_noise(self, batch, channels, height, width, dtype, device, generator) -> torch.Tensor:
        """The draw of ``prepare_latents`` (same generator, shape and dtype) WITHOUT the scheduler's initial sigma: the ``eps`` of a
        forward-noised picture."""
        return self._host_noise(batch, channels, height, width, dtype, generator).to(self.device)

    def _get_add_time_ids(self, original_size, crops_coords_top_left, target_size, dtype,
                          text_encoder_projection_dim=None):
        ids = list(original_size) + list(crops_coords_top_left) + list(target_size)
        return torch.tensor([ids], dtype=dtype, device=self.device)

    # ---- programs -----------------------------------------------------------------------
    def _cached(self, cache: OrderedDict, key, build):
        if key in cache:
            cache.move_to_end(key)
            return cache[key]
        while len(cache) >= max(1, self.max_cached_programs):
            torch.cuda.synchronize(self.device)          # (its launches may still be in flight on the stream)
            cache.popitem(last=False)                    # least recently used: arena, workspaces and graph go with it
        cache[key] = build()
        return cache[key]

    @property
    def ragged_halo(self) -> bool:
        return self._ragged_halo

    @ragged_halo.setter
    def ragged_halo(self, flag: bool):
        flag = bool(flag)
        if flag != self._ragged_halo:
            self._ragged_halo = flag
            for cache in (self._unet_programs, self._vae_programs, self._vae_encoder_programs):
                stale = [k for k in cache if len(k) == 3]           # (square programs, keyed (B, L), never carry the flag)
                if stale:
                    torch.cuda.synchronize(self.device)
                for k in stale:
                    del cache[k]
            self._drop_control_programs()

    @staticmethod
    def _check_tileable(value) -> str:
        """None / False / "" -> "" (off); "x", "y", "xy" (case-insensitive) -> themselves; True -> "xy" (``geometry.check_tileable``)."""
        return check_tileable(value)

    @property
    def tileable(self) -> str:
        """"" (off), "x", "y" or "xy": the axes along which rendered frames join (see the constructor)."""
        return self._tileable

    @tileable.setter
    def tileable(self, value):
        value = self._check_tileable(value)
        if value != self._tileable:
            self._tileable = value
            caches = (self._unet_programs, self._vae_programs, self._tiny_vae_programs)        # (the encoders never wrap)
            if any(caches):
                torch.cuda.synchronize(self.device)
            for cache in caches:
                cache.clear()
            self._drop_control_programs()           # (the ControlNet's convs and the hint embedding wrap with the UNet's)

    @property
    def _wrap(self) -> int:
        return TILEABLE_WRAP[self._tileable]

    @staticmethod
    def _check_decoder(name) -> str:
        if not isinstance(name, str) or name.strip().lower() not in ("full", "tiny"):
            raise ValueError(f"NativeSDXLPipe: decoder must be 'full' or 'tiny' (got {name!r})")
        return name.strip().lower()

    @property
    def decoder(self) -> str:
        return self._decoder

    @decoder.setter
    def decoder(self, name: str):
        self._decoder = self._check_decoder(name)

    @staticmethod
    def _check_encoder(name) -> str:
        if not isinstance(name, str) or name.strip().lower() not in ("full", "tiny"):
            raise ValueError(f"NativeSDXLPipe: encoder must be 'tiny' or 'full' (got {name!r})")
        return name.strip().lower()

    @property
    def encoder(self) -> str:
        return self._encoder

    @encoder.setter
    def encoder(self, name: str):
        name = self._check_encoder(name)
        if name == "full":
            self._full_encoder_source()
        self._encoder = name

    def _full_encoder_source(self):
        """What the full encoder is (or would be) packed from: None = the ready-made ``vae_encoder_native``, else a provider.  A
        ready-made decoder without the provider it was packed from has no encoder weights to offer: ``ValueError``."""
        if self.vae_encoder_native is not None:
            return None
        if self._vae_provider is not None:
            return self._vae_provider
        if self._vae_native_given:
            raise ValueError("NativeSDXLPipe: the full VAE encoder needs weights, and the pipe was given a ready-made vae_native= without "
                             "the provider it was packed from; pass vae_provider= (the encoder.* / quant_conv.* keys of the same "
                             "checkpoint) or vae_encoder_native= beside it - a synthetic encoder is never paired with a given decoder")
        return SyntheticProvider(self._vae_seed)

    def _vae_encoder_net(self) -> NativeVAEEncoder:
        if self.vae_encoder_native is None:
            source = self._full_encoder_source()
            if self._vae_provider is None:
                self._synthetic_notice("VAE encoder weights", "pass vae_provider=native.from_safetensors(<dir>/vae)")
            self.vae_encoder_native = NativeVAEEncoder(self.vae_cfg, source, self.device)
        return self.vae_encoder_native

    def vae_encoder_program(self, B: int, L) -> VAEEncoderProgram:
        """The full SDXL VAE encoder's program for ``B`` pictures of latent size ``L`` (side or ``(H, W)``)."""
        def build():
            prog = self._vae_encoder_net().build(B, L, ragged_halo=self._ragged_halo)
            if self._use_graphs:
                prog.enable_graphs()
            return prog
        return self._cached(self._vae_encoder_programs, program_key(B, L), build)

    @property
    def active_vae_cfg(self):
        return self.tiny_vae_cfg if self._decoder == "tiny" else self.vae_cfg

    @property
    def tiny_conv_c64(self) -> bool:
        return self._tiny_conv_c64

    @tiny_conv_c64.setter
    def tiny_conv_c64(self, flag: bool):
        flag = bool(flag)
        if flag != self._tiny_conv_c64:
            self._tiny_conv_c64 = flag
            if self._tiny_vae_programs or self._tiny_encoder_programs:
                torch.cuda.synchronize(self.device)
            self._tiny_vae_programs.clear()
            self._tiny_encoder_programs.clear()

    def _tiny_net(self) -> NativeTinyVAEDecoder:
        if self.tiny_vae_native is None:
            if self._tiny_vae_provider is None:
                self._synthetic_notice("tiny VAE (TAESDXL) weights", "pass tiny_vae_provider=native.from_safetensors(<dir>/taesdxl)")
            self.tiny_vae_native = NativeTinyVAEDecoder(self.tiny_vae_cfg, self._tiny_vae_provider or SyntheticProvider(self._tiny_seed),
                                                        self.device)
        return self.tiny_vae_native

    def _tiny_encoder_net(self) -> NativeTinyVAEEncoder:
        if self.tiny_vae_encoder_native is None:
            if self._tiny_vae_provider is None:
                self._synthetic_notice("tiny VAE encoder (TAESDXL) weights", "pass tiny_vae_provider=native.from_safetensors(<dir>/taesdxl)")
            self.tiny_vae_encoder_native = NativeTinyVAEEncoder(self.tiny_vae_cfg, self._tiny_vae_provider or SyntheticProvider(self._tiny_seed),
                                                                self.device)
        return self.tiny_vae_encoder_native

    def tiny_encoder_program(self, B: int, L) -> TinyEncoderProgram:
        """The TAESDXL encoder's program for ``B`` pictures of latent size ``L`` (side or ``(H, W)``)."""
        def build():
            prog = self._tiny_encoder_net().build(B, L, c64=self._tiny_conv_c64)
            if self._use_graphs:
                prog.enable_graphs()
            return prog
        return self._cached(self._tiny_encoder_programs, program_key(B, L), build)

    def unet_program(self, B: int, L, control: Optional[bool] = None) -> UNetProgram:
        """``L``: latent side or ``(H, W)``.  A size the UNet's levels do not divide raises ``ValueError`` (nearest valid sizes named).
        ``control``: None (default) = the controlled program - both networks in one step program, the hint in place - while a
        control image is active (``control_active``), else the plain one; False = the plain program whatever is set.  The two
        kinds are cached under different keys."""
        if control is None:
            control = self.control_active
        if control:
            net = self._require_controlnet("unet_program(control=True)")
            if self._control_hint is None:
                raise ValueError("unet_program(control=True): no control image is set (set_control_image)")
            LH, LW = latent_hw(L)
            emb = self._control_embedding(LH, LW)

            def build_controlled():
                prog = self.unet_native.build(B, L, ragged_halo=self._ragged_halo, wrap=self._wrap, control=net)
                prog.set_hint(emb)
                if self._use_graphs:
                    prog.enable_graphs()
                return prog
            return self._cached(self._control_programs, program_key(B, L), build_controlled)

        def build():
            prog = self.unet_native.build(B, L, ragged_halo=self._ragged_halo, wrap=self._wrap)
            if self._use_graphs:
                prog.enable_graphs()
            return prog
        return self._cached(self._unet_programs, program_key(B, L), build)

    def vae_program(self, B: int, L):
        """The ACTIVE decoder's program (``pipe.decoder``): a ``VAEProgram`` or a ``TinyVAEProgram`` - the same surface."""
        tiny = self._decoder == "tiny"

        def build():
            prog = self._tiny_net().build(B, L, c64=self._tiny_conv_c64, wrap=self._wrap) if tiny else \
                self.vae_native.build(B, L, ragged_halo=self._ragged_halo, wrap=self._wrap)
            if self._use_graphs:
                prog.enable_graphs()
            return prog
        return self._cached(self._tiny_vae_programs if tiny else self._vae_programs, program_key(B, L), build)

    def enable_graphs(self, flag: bool = True):
        self._use_graphs = bool(flag)
        if flag:
            for cache in (self._unet_programs, self._vae_programs, self._tiny_vae_programs, self._tiny_encoder_programs,
                          self._vae_encoder_programs, self._control_programs, self._controlnet_programs, self._hint_programs):
                for p in cache.values():
                    p.enable_graphs()

    def synchronize(self):
        torch.cuda.synchronize(self.device)

    # ---- native fast path -----------------------------------------------------------------
    def _time_ids_row(self) -> List[float]:
        side = float(self.default_sample_size * self.vae_scale_factor)
        return [side, side, 0.0, 0.0, side, side]      # native size, not render size (reference quirk)

    def native_run_diffusion(self, text_embeddings, latents_start, idx_start, list_latents_mixing, coeffs,
                             num_inference_steps, guidance_scale, noise_id: Optional[int] = None):
        """One branch.  ``noise_id``: its trajectory id under counter-based noise; None = the id bound on the source (the engine
        binds it around the holder's run), else a free one - a caller that says nothing still gets noise, merely unaddressed."""
        src = self.scheduler.noise_source
        if noise_id is None and hasattr(src, "keyed"):
            noise_id = src.bound_id() if hasattr(src, "bound_id") else None
        return self.native_run_diffusion_batch([text_embeddings], [latents_start], idx_start,
                                               [list_latents_mixing], [coeffs], num_inference_steps,
                                               [guidance_scale], noise_ids=None if noise_id is None else [noise_id])[0]

    @torch.no_grad()
    def native_run_diffusion_batch(self, conds: Sequence[tuple], starts: Sequence[torch.Tensor], idx_start: int,
                                   mixings: Sequence[Optional[list]], coeffs_list: Sequence[Sequence[float]],
                                   num_inference_steps: int, guidance_scales: Sequence[float],
                                   noise_slots: Optional[Tuple[int, Sequence[int]]] = None,
                                   noise_ids: Optional[Sequence[int]] = None):
        """Denoise G branches in lock-step from ``idx_start``.  Returns per branch a list with one
        entry per step (``None`` below ``idx_start``, else the [1,4,L,L] latent after that step).
        ``noise_slots`` = (n_total, my_indices): these G branches are numbers ``my_indices`` of a round of
        ``n_total`` branches evaluated by several ranks; ancestral noise is then drawn for all ``n_total`` in
        order and only this rank's share is used, so a shared noise stream stays aligned across ranks.
        ``noise_ids``: one trajectory id per branch (native/noise.py), read when the scheduler's noise source is counter-based
        (it has ``keyed``): the rows of these G branches' own steps are built and served by one launch, and ``noise_slots`` is
        ignored - there is no stream to keep aligned."""
        G = len(conds)
        sched = self.scheduler
        if sched.num_inference_steps != num_inference_steps:
            sched.set_timesteps(num_inference_steps)
        # classifier-free guidance is a per-branch predicate in the reference (guidance_scale > 1,
        # diffusers_holder.py:80,282): a batch mixing both kinds is run as two homogeneous sub-batches
        wants = [self.uses_cfg(g) for g in guidance_scales]
        if any(wants) and not all(wants):
            out: List[Optional[list]] = [None] * G
            assert noise_slots is None, "mixed CFG / non-CFG rounds are not supported under a farm"
            for flag in (False, True):
                idx = [g for g in range(G) if wants[g] == flag]
                part = self.native_run_diffusion_batch([conds[g] for g in idx], [starts[g] for g in idx], idx_start,
                                                       [mixings[g] for g in idx], [coeffs_list[g] for g in idx],
                                                       num_inference_steps, [guidance_scales[g] for g in idx],
                                                       noise_ids=None if noise_ids is None else [noise_ids[g] for g in idx])
                for g, traj in zip(idx, part):
                    out[g] = traj
            return out
        self._guidance_scale = float(guidance_scales[-1])
        cfg = wants[0]
        LH, LW = int(starts[0].shape[-2]), int(starts[0].shape[-1])
        prog = self.unet_program(G * (2 if cfg else 1), (LH, LW))
        prog.set_conditioning(*self._conditioning(conds, cfg), timestep_cond=self._timestep_cond(guidance_scales))

        latents = torch.cat([s.to(self.device, F16).reshape(1, -1, LH, LW) for s in starts]).contiguous()
        trajs: List[List[Optional[torch.Tensor]]] = [[None] * idx_start for _ in range(G)]
        stream = torch.cuda.current_stream().cuda_stream
        # every step's scalar coefficients in ONE upload: [steps][G][8]
        rows = [sched.step_row(i, float(guidance_scales[g]), first=i == idx_start) for i in range(idx_start, num_inference_steps)
                for g in range(G)]
        params_all = ops.step_params(rows, self.device).view(-1, G, 8) if rows else None
        # ancestral noise is drawn sample-major (all steps of branch 0, then branch 1, ...): the same
        # order a sequential engine consumes a noise tape in, so batching does not change results
        noise_all = None
        nm = noise_draws_per_run(sched, num_inference_steps, idx_start)     # (ancestral: every step; LCM: every step but the last)
        if nm > 0:
            shape1 = (1,) + tuple(latents.shape[1:])
            if hasattr(sched.noise_source, "keyed"):      # counter-based: step-major rows of this call's own samples, one launch
                noise_all = self._keyed_noise(sched, noise_ids, [(g, i) for i in range(idx_start, idx_start + nm) for g in range(G)],
                                              shape1).view(nm, G, *shape1[1:])
            else:
                n_draw, keep = self._noise_slots(noise_slots, G)
                drawn = sched.draw_noise_many(n_draw * nm, shape1, self.device).view(n_draw, nm, *shape1[1:])
                noise_all = drawn[keep].transpose(0, 1).contiguous()                             # [steps, G, 4, L, L]
        hist = carry = None         # (a multistep sampler's previous x0 predictions / two-plane state; every run starts without)
        for i in range(idx_start, num_inference_steps):
            mix = []
            if i > 0:
                mix = [g for g in range(G) if coeffs_list[g][i] > 0]
                if mix:
                    outs = ops.slerp_pairs([latents[g:g + 1] for g in mix],
                                           [mixings[g][i - 1].to(self.device, F16) for g in mix],
                                           [float(coeffs_list[g][i]) for g in mix])
                    self.stats["slerps"] += len(mix)
                    if len(mix) == G:
                        latents = torch.cat(outs)
                    else:
                        latents = latents.clone()
                        for g, o in zip(mix, outs):
                            latents[g:g + 1] = o
            params = params_all[i - idx_start]
            self._launch_unet_step(prog, latents, params, G, cfg, i, stream)
            noise = noise_all[i - idx_start] if noise_all is not None and i - idx_start < nm else None
            latents, hist, carry = self._device_step(latents, [(hist, G)], prog.eps, params, noise, cfg, i, carry=carry, mixed=bool(mix))
            for g in range(G):
                trajs[g].append(latents[g:g + 1])
        return trajs

    @torch.no_grad()
    def native_run_wavefront(self, anchor_conds: Sequence[tuple], anchor_starts: Sequence[torch.Tensor],
                             mid_conds: Sequence[tuple], mid_fracts: Sequence[float],
                             mid_coeffs: Sequence[Sequence[float]], idx_injection: int, num_inference_steps: int,
                             guidance_anchor: float, guidance_mids: Sequence[float],
                             noise_slots: Optional[Tuple[int, Sequence[int]]] = None, elide_dead_steps: bool = False,
                             known_anchors: Sequence[Optional[Sequence[torch.Tensor]]] = (None, None),
                             noise_ids: Optional[Tuple[Sequence[int], Sequence[int]]] = None):
        """Both anchors AND a set of mid branches whose parents are the anchors, in one wavefront.

        A mid branch at step i only needs the anchors' latents of step i-1 (its start latent and its
        crossfeed targets are slerps of the anchors' previous-step latents, blending_engine.py:443-464
        of the reference), so from ``idx_injection`` on the anchors' step i and every mid branch's step
        i share ONE UNet batch of 2+G samples: 2 small + (steps-idx) large forwards instead of
        ``steps`` small + (steps-idx) large ones.  Arithmetic per sample is the same as in the
        separate runs.  Returns (trajectory anchor 1, trajectory anchor 2, [mid trajectories]).
        ``noise_slots`` = (n_total, my_indices) as in ``native_run_diffusion_batch`` (farm: every rank runs both
        anchors plus its own share of the round's mid branches).
        ``elide_dead_steps`` (opt-in): a mid step whose result the NEXT step's crossfeed overwrites
        completely (crossfeed coefficient exactly 1.0 - the SDXL-Turbo defaults, reference blending_engine.py:193-199,
        452-457 and diffusers_holder.py:322-324: slerp(x, target, 1.0) == target) is not computed: that step runs the
        anchors only, the mids' trajectory entry is ``None``.  Frames and final latents are bit-identical (noise draws
        are still consumed in the same order); the reference itself performs the dead forward, so the default is off.
        ``known_anchors[k]`` = a finished trajectory of anchor k (a recycled key frame, blending_engine.py:333-342 of the
        reference: ``recycle_img1`` after ``swap_forward``): that anchor is not denoised again - the small batches carry only
        the other anchor, the mids mix from the stored latents - and is returned as given.
        Under a MULTISTEP sampler every sample carries its previous x0 prediction from step to step: when the batch grows at
        ``idx_injection`` the anchors keep theirs and the mids enter without (first-order rows - the order is a property of the
        row, so one launch serves the mixed batch).  A skipped step would leave no x0 prediction behind for the step after it, so
        ``elide_dead_steps`` is ignored under such a sampler (with one warning per pipe).
        ``noise_ids`` = (the two anchors' trajectory ids, the mids' ids), read when the scheduler's noise source is counter-based:
        the rows of the steps this call really runs (no anchor that is known, no mid step that is dead) are served by one launch;
        ``noise_slots`` is then ignored."""
        known = [None if t is None else list(t) for t in known_anchors]
        live = [k for k in (0, 1) if known[k] is None]          # anchors denoised here
        # ``mid_conds`` may be a CALLABLE returning the list (round 6): the mids' conditionings (two lerp launches each) are then built -
        # and the big batch's conditioning program launched - AFTER the first anchors-only step is on the stream, i.e. the host work runs
        # beside 11 ms of GPU work instead of in front of it (a cfg-2 transition spent ~2 ms of host time before its first launch)
        lazy_mids = callable(mid_conds)
        A, G = len(live), len(mid_fracts)
        assert lazy_mids or len(mid_conds) == G
        assert A + G > 0, "native_run_wavefront: nothing to denoise"
        assert all(t is None or len(t) == num_inference_steps for t in known), "known anchors must be full trajectories"
        anchor_conds = [anchor_conds[k] for k in live]
        sched, steps = self.scheduler, num_inference_steps
        if sched.num_inference_steps != steps:
            sched.set_timesteps(steps)
        all_g = [float(guidance_anchor)] * A + [float(g) for g in guidance_mids]
        self._guidance_scale = all_g[-1]
        cfg = self.uses_cfg(all_g[0])
        ref_start = anchor_starts[0]
        anchor_starts = [anchor_starts[k] for k in live]
        assert all(self.uses_cfg(g) == cfg for g in all_g), "wavefront batches must be uniformly CFG or non-CFG"
        mul = 2 if cfg else 1
        LH, LW = int(ref_start.shape[-2]), int(ref_start.shape[-1])

        def prepared(conds, side=None, after=None, guid=None):
            # (the program - arena, workspaces, first-time graph instantiation - is always obtained on the MAIN stream: its
            # allocations then belong to the main stream's allocator pool; only the conditioning launches move to `side`)
            # `conds` may be a callable (evaluated on the stream the conditioning launches run on); `after` = an event of the main
            # stream the side stream waits for INSTEAD of everything queued on the main stream so far (the deferred form: the first
            # small UNet step is already queued - waiting for it would also park the host in the side stream's host-to-device copies)
            n_conds = A + G if callable(conds) else len(conds)
            prog = self.unet_program(n_conds * mul, (LH, LW))

            def set_conditioning():
                # (copies into program-owned buffers, then the conditioning program: all on the stream that is current here - under
                # `side` the temporaries never meet another stream)
                prog.set_conditioning(*self._conditioning(conds() if callable(conds) else conds, cfg),
                                      timestep_cond=self._timestep_cond(guid))
            if side is None:
                set_conditioning()
                return prog, None
            if after is not None:
                side.wait_event(after)
            else:
                side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                set_conditioning()
                return prog, side.record_event()

        # G == 0: a farm rank that owns no mid branch of the round (fewer gaps than ranks) still runs both anchors
        if elide_dead_steps and sched.multistep:
            if "elide-multistep" not in self._warned:
                self._warned.add("elide-multistep")
                warnings.warn(f"elide_dead_steps is ignored under the multistep sampler {sched.kind!r}: a skipped step leaves no x0 "
                              f"prediction behind for the next step's second-order update", UserWarning, stacklevel=2)
            elide_dead_steps = False
        dead = [bool(elide_dead_steps) and G > 0 and i >= idx_injection and i + 1 < steps and
                all(float(mid_coeffs[g][i + 1]) == 1.0 for g in range(G)) for i in range(steps)]
        prog_a = prepared(list(anchor_conds), guid=all_g[:A])[0] if A and (idx_injection > 0 or G == 0 or any(dead)) else None
        # The big batch's conditioning program (every branch's context K | V projection: ~1.1 ms at 17 samples) does not depend
        # on any latent: when small anchor-only steps come first it runs on a SIDE stream beside them (they leave most of the
        # chip idle) and the main stream waits for it only before the first big step.  Different programs own different
        # arenas / workspaces, so the two streams share nothing but read-only weights.
        cond_ready = None
        deferred = False
        if G and prog_a is not None and idx_injection > 0:
            if self._side_stream is None:
                self._side_stream = torch.cuda.Stream(device=self.device)
            if lazy_mids and A:
                deferred, prog_all = True, None         # (prepared right behind the first small step's launch, below)
                before_first = torch.cuda.Event()
                before_first.record()                   # everything the mids' conditionings read (the prompt embeddings) is older than this
            else:
                prog_all, cond_ready = prepared(list(anchor_conds) + list(mid_conds() if lazy_mids else mid_conds), side=self._side_stream, guid=all_g)
        else:
            prog_all = prepared(list(anchor_conds) + list(mid_conds() if lazy_mids else mid_conds), guid=all_g)[0] if G else prog_a
        stream = torch.cuda.current_stream().cuda_stream
        rows_a = [sched.step_row(i, all_g[0], first=i == 0) for i in range(steps)]
        par_a = ops.step_params([r for r in rows_a for _ in range(A)], self.device).view(steps, A, 8) if A else None
        par_all = ops.step_params([sched.step_row(i, all_g[s], first=i == (0 if s < A else idx_injection)) for i in range(idx_injection, steps)
                                   for s in range(A + G)], self.device).view(-1, A + G, 8) if G else None
        shape1 = (1,) + tuple(ref_start.shape[1:])
        noise_a = noise_m = None
        # draws per run: an anchor's (from step 0) and a mid branch's (from idx_injection) - ancestral: one per step; LCM: one per
        # step but the schedule's last, so both kinds of run have noise at exactly the steps < nd_a
        nd_a, nm = noise_draws_per_run(sched, steps, 0), noise_draws_per_run(sched, steps, idx_injection)
        if nd_a > 0 and hasattr(sched.noise_source, "keyed"):
            # counter-based: rows (trajectory, step) of the anchors denoised here at every drawing step, then of the mids at the
            # steps they run - step-major, so each step's share is contiguous
            ids = None if noise_ids is None else [noise_ids[0][k] for k in live] + list(noise_ids[1])
            mid_steps = [i for i in range(idx_injection, nd_a) if not dead[i]] if G else []
            flat = self._keyed_noise(sched, ids, [(s, i) for i in range(nd_a) for s in range(A)]
                                     + [(A + g, i) for i in mid_steps for g in range(G)], shape1)
            noise_a = flat[:A * nd_a].view(nd_a, A, *shape1[1:]) if A else None
            if mid_steps:
                per_step = flat[A * nd_a:].view(len(mid_steps), G, *shape1[1:])
                noise_m = [None] * nm                       # (indexed like the stream's [nm, G, ...]; a dead step has no entry)
                for j, i in enumerate(mid_steps):
                    noise_m[i - idx_injection] = per_step[j]
        elif nd_a > 0:            # sample-major draws: anchor 1, anchor 2 (those denoised here), then every mid branch
            n_draw, keep = self._noise_slots(noise_slots, G)
            flat = sched.draw_noise_many(A * nd_a + n_draw * nm, shape1, self.device)      # ONE launch on the device RNG
            # (contiguous per step: the step kernels take noise[i] by pointer)
            noise_a = flat[:A * nd_a].view(A, nd_a, *shape1[1:]).transpose(0, 1).contiguous() if A else None          # [nd_a, A, 4, L, L]
            noise_m = flat[A * nd_a:].view(n_draw, nm, *shape1[1:])[keep].transpose(0, 1).contiguous() if G and nm else None   # [nm, G, 4, L, L]
        lat_shape = (int(ref_start.shape[-3]), LH, LW)
        lat_a = torch.cat([s.to(self.device, F16).reshape(1, -1, LH, LW) for s in anchor_starts]).contiguous() if A else \
            torch.empty((0,) + lat_shape, dtype=F16, device=self.device)
        lat_m = None
        hist_a = hist_m = None      # (a multistep sampler's previous x0 predictions: the anchors' [A, ...] and the mids' [G, ...])
        traj_a = [[] if known[k] is None else [t.to(self.device, F16).reshape(1, -1, LH, LW) for t in known[k]] for k in (0, 1)]
        traj_m: List[List[Optional[torch.Tensor]]] = [[None] * idx_injection for _ in range(G)]
        # mixing fractions / crossfeed coefficients live on the device: every step's parental mix (ONE pair of anchor
        # latents at G fractions) and crossfeed (G pairs) is one strided-slerp launch, no host pointer tables
        n_lat = ref_start[0].numel()
        fr_dev = torch.tensor([float(f) for f in mid_fracts], dtype=torch.float64, device=self.device) if G else None
        coef_dev = torch.tensor([[float(mid_coeffs[g][i]) for g in range(G)] for i in range(steps)],
                                dtype=torch.float64, device=self.device) if G else None
        try:
            for i in range(steps):
                if i < idx_injection or G == 0 or dead[i]:
                    if dead[i] and i == idx_injection:
                        # the mids' (never denoised) start value: the parental mix of step i-1, exactly what the live path starts
                        # from - the next step's crossfeed slerp at coefficient 1.0 replaces it bit for bit, but its FIRST operand
                        # must be a proper latent (a zero tensor has no direction: 0 / 0 in the slerp's cosine)
                        lat_m = ops.slerp_strided(traj_a[0][i - 1].contiguous(), traj_a[1][i - 1].contiguous(), fr_dev, n_lat,
                                                  broadcast0=True, broadcast1=True).view(G, *lat_shape)
                        self.stats["slerps"] += G
                    if A == 0:                  # both anchors known: nothing runs before the injection step (or in a dead one)
                        if i >= idx_injection and G and dead[i]:
                            for g in range(G):
                                traj_m[g].append(None)
                        continue
                    prog, lat, params, n = prog_a, lat_a, par_a[i], A
                    hists = [(hist_a, A)]
                    noise = noise_a[i] if noise_a is not None and i < nd_a else None
                else:
                    prev1, prev2 = traj_a[0][i - 1].contiguous(), traj_a[1][i - 1].contiguous()
                    mix_prev = ops.slerp_strided(prev1, prev2, fr_dev, n_lat, broadcast0=True, broadcast1=True)   # parental mix of step i-1
                    self.stats["slerps"] += G
                    if i == idx_injection:
                        lat_m = mix_prev.view(G, *lat_shape)
                    elif dead[i - 1]:
                        assert all(float(mid_coeffs[g][i]) == 1.0 for g in range(G))
                    nfeed = sum(1 for g in range(G) if mid_coeffs[g][i] > 0)
                    if nfeed:       # (a coefficient of 0 returns the first operand bit-exactly, like the reference's skipped slerp)
                        lat_m = ops.slerp_strided(lat_m.contiguous().view(G, n_lat), mix_prev, coef_dev[i], n_lat).view(G, *lat_shape)
                        self.stats["slerps"] += nfeed
                    prog, lat, params, n = prog_all, (torch.cat([lat_a, lat_m]) if A else lat_m.contiguous()), par_all[i - idx_injection], A + G
                    hists = [(hist_a, A), (hist_m, G)]
                    if cond_ready is not None:
                        torch.cuda.current_stream().wait_event(cond_ready)
                        cond_ready = None
                    noise = None
                    if noise_m is not None and i < nd_a:
                        noise = torch.cat([noise_a[i], noise_m[i - idx_injection]]) if A else noise_m[i - idx_injection]
                self._launch_unet_step(prog, lat, params, n, cfg, i, stream)
                out, hist, _ = self._device_step(lat, hists, prog.eps, params, noise, cfg, i)      # (the batch changes size: no carry)
                if deferred:            # the first small step is launched: now the host work the big batch needs (runs beside it)
                    deferred = False
                    prog_all, cond_ready = prepared(lambda: list(anchor_conds) + list(mid_conds()), side=self._side_stream, after=before_first, guid=all_g)
                lat_a = out[:A]
                if hist is not None:
                    hist_a, hist_m = hist[:A], (hist[A:] if n > A else hist_m)
                for j, k in enumerate(live):
                    traj_a[k].append(out[j:j + 1])
                if i >= idx_injection and G and dead[i]:
                    for g in range(G):
                        traj_m[g].append(None)
                elif i >= idx_injection and G:
                    lat_m = out[A:]
                    for g in range(G):
                        traj_m[g].append(out[A + g:A + g + 1])
        finally:
            if cond_ready is not None:      # (an exception before the first big step: never leave the side stream's conditioning
                torch.cuda.current_stream().wait_event(cond_ready)    # launches un-joined - a later call reuses the cached program)
        return traj_a[0], traj_a[1], traj_m

    @torch.no_grad()
    def native_latent2image_batch(self, latents: Sequence[torch.Tensor], output_type="pil"):
        z = torch.cat([t.to(self.device, F16).reshape(1, -1, t.shape[-2], t.shape[-1]) for t in latents])
        prog = self.vae_program(z.shape[0], (z.shape[-2], z.shape[-1]))
        frames = prog.decode(z).clone()
        self.stats["vae_decodes"] += z.shape[0]
        if output_type == "np":     # the reference's postprocess(..., "np"): (x / 2 + 0.5).clamp(0, 1) as float32 HWC, unquantised
            img = (prog.image_f32[..., :3].float() / 2 + 0.5).clamp(0, 1)
            return [f.cpu().numpy() for f in img]
        return [DeviceImage(f) for f in frames]

    def native_latent2image(self, latents, output_type="pil"):
        return self.native_latent2image_batch([latents], output_type)[0]

    def _pictures_u8(self, images) -> torch.Tensor:
        """A PIL image / device frame, a list of them, or a uint8 [B, H, W, 3] (or [H, W, 3]) tensor or array -> uint8 [B, H, W, 3]
        on the device."""
        if isinstance(images, (Image.Image, DeviceImage)):
            images = [images]
        if isinstance(images, (list, tuple)):
            if not images:
                raise ValueError("native_image2latent: no picture given")
            one = [self._frame_u8(im) if isinstance(im, DeviceImage) else
                   torch.from_numpy(np.array(im.convert("RGB") if isinstance(im, Image.Image) else im)) for im in images]
            if any(t.ndim != 3 or t.shape != one[0].shape for t in one):
                raise ValueError(f"native_image2latent: the pictures must share one [H, W, 3] shape (got {[tuple(t.shape) for t in one]})")
            u8 = torch.stack(one)
        else:
            u8 = images if torch.is_tensor(images) else torch.from_numpy(np.array(images))
            if u8.ndim == 3:
                u8 = u8[None]
        if u8.dtype != torch.uint8 or u8.ndim != 4 or u8.shape[-1] != 3:
            raise ValueError(f"native_image2latent: pictures must be uint8 [B, H, W, 3] (got {u8.dtype} {tuple(u8.shape)})")
        return u8.to(self.device).contiguous()

    @torch.no_grad()
    def native_image2latent(self, images) -> torch.Tensor:
        """Pictures -> the latents the pipe's ``encoder`` gives them ("tiny": TAESDXL; "full": the SDXL VAE's ``encode(x).mode() *
        scaling_factor``): fp16 [B, 4, H / 8, W / 8] on the device, in scaled units
        (UNet latents as they stand, whatever ``decoder`` is active).  ``images``: a PIL image, a list of them, or a uint8
        [B, H, W, 3] tensor or array; H and W must be the pipe's current render size (``render_size``: what ``prepare_latents``
        was last asked for - the holder states its own before it calls) - any other size is a ``ValueError``."""
        u8 = self._pictures_u8(images)
        H, W = int(u8.shape[1]), int(u8.shape[2])
        if (H, W) != tuple(self.render_size):
            raise ValueError(f"native_image2latent: the pictures are {W} x {H} (width x height) but the pipe renders "
                             f"{self.render_size[1]} x {self.render_size[0]}; resize them first")
        full = self._encoder == "full"
        f = (self.vae_cfg if full else self.tiny_vae_cfg).scale_factor
        if H % f or W % f:
            raise ValueError(f"native_image2latent: the render size {W} x {H} is no multiple of {f}")
        prog = (self.vae_encoder_program if full else self.tiny_encoder_program)(u8.shape[0], (H // f, W // f))
        z = prog.encode(u8).clone()
        self.vae_encodes += int(u8.shape[0])
        return z

    @torch.no_grad()
    def native_frame_distances(self, pairs) -> List[float]:
        """LPIPS distance for (frameA, frameB) pairs of ``DeviceImage`` / PIL / numpy frames."""
        frames = []
        for a, b in pairs:
            frames += [a, b]
        missing, seen = [], set()
        for f in frames:
            if getattr(f, "_lb_feats", None) is None and id(f) not in seen:
                seen.add(id(f))
                missing.append(f)
        if missing:
            u8 = torch.stack([self._frame_u8(f) for f in missing])
            taps = self.lpips_metric.features(u8)
            for n, f in enumerate(missing):
                feats = [t[n] for t in taps]
                try:
                    f._lb_feats = feats
                except AttributeError:
                    pass
                self._feat_scratch[id(f)] = feats
        feat_of = lambda f: getattr(f, "_lb_feats", None) or self._feat_scratch[id(f)]
        d = self.lpips_metric.distances([(feat_of(a), feat_of(b)) for a, b in pairs])
        self.stats["lpips_pairs"] += len(pairs)
        self._feat_scratch.clear()
        return [float(v) for v in d.tolist()]

    def _frame_u8(self, f) -> torch.Tensor:
        if isinstance(f, DeviceImage):
            return f._lb_u8.to(self.device)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(f, dtype=np.uint8))).to(self.device)


NativeSDXLPipe = StableDiffusionXLPipeline
