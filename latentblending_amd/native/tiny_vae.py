"""Native TAESDXL tiny decoder (diffusers ``AutoencoderTiny`` decoder as published for ``madebyollin/taesdxl``; the reference
loads it at latentblending/blending_engine.py:797-806 and diffusers_holder.py:373-379) for gfx950: the
preview / real-time alternative to the full ``AutoencoderKL`` decode of ``native/vae.py``.

Architecture (restated from the published one; ``diffusers`` is not available here, so the decoder is NOT pinned against a
diffusers run - the tests hold it to a float64 restatement of this description, ``tests/_taesd_ref.py``):

    x = tanh(z / 3) * 3                                      z: latents in SCALED units (scaling_factor 1.0: nothing is divided out)
    decoder.layers.0        conv 4 -> 64, bias, ReLU
    per stage i (num_blocks (3, 3, 3, 1)):
        block               relu(conv(relu(conv(relu(conv(x))))) + x), three biased 64 -> 64 convs at decoder.layers.N.conv.{0,2,4}
        every stage but the last:  nearest-2x upsample, then conv 64 -> 64 WITHOUT bias
        the last stage:            conv 64 -> 3 with bias
    image = 2 x - 1  in [-1, 1]
    layer indices: 0, [2-4], 6, [7-9], 11, [12-14], 16, [17], 18; the checkpoint's ``encoder.*`` keys are the encoder's (below).

No normalisation, no attention: the program is ``lb_nchw_to_nhwc_f16``, about thirty 3x3 convs and ``lb_postprocess_u8``.  The
64 -> 64 convs (block convs; the three upsample convs with ``ups = 1``: the gather reads the low-resolution map) go through
``lb_gemm_f16`` with ``LB_GEMM_C64`` - the kernel with LDS-resident weights, csrc/conv3_c64.hip - where ``use_c64`` says so, and
through the library's own routing (halo-tile kernel / implicit GEMM) otherwise: ``c64=False`` records the same launches without the
bit, which is the A/B and the fallback.  The last conv takes the narrow-N route with ``OUT_F32``; ``2 x - 1`` is folded into its
weights and bias at load time (``W * 2``, ``b * 2 - 1``).

The tanh clamp has no launcher of its own (the library's C ABI is closed: every exported launcher must have a replay case in the
program tests, and this pull request adds no symbol): it is one torch elementwise over ``B * 4 * H * W`` values, applied where
``decode()`` stages the latents.

Quality: TAESDXL is a distilled approximation of the SDXL VAE - a speed / preview option.  With the seeded synthetic stand-in
weights nothing can be said about it; an LPIPS tree built under ``decoder="tiny"`` is computed on the tiny decoder's own frames.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

import torch

from ..hip import lib
from ..hip.lib import api
from .runtime import Program, RecordedProgram, F16, F32, _stream
from .weights import Packer, SyntheticProvider, pad_to

# LB_GEMM_C64 is set on a 64 -> 64 conv only where the flagged launch measured faster than the library's own route for the same
# problem by more than the run-to-run spread (tools/tiny_vae_bench.py -> profiles/tiny_vae.txt, one MI355X, both launches
# interleaved in one process, bias + ReLU; unflagged time / flagged time):
#    B  output map  ups   tiles  speedup        B  output map  ups   tiles  speedup
#   17    64 x 64     0     272    1.61         2    64 x 64     0      32    1.00   <- a tie: 32 blocks on 256 CUs either way
#   17   128 x 128    0    1088    1.74         2   128 x 128    0     128    1.48
#   17   256 x 256    0    4352    1.77         2   256 x 256    0     512    1.58
#   17   512 x 512    0   17408    1.80         2   512 x 512    0    2048    1.79
#   17   128 x 128    1    1088    1.58         2   128 x 128    1     128    1.08
#   17   256 x 256    1    4352    1.92         2   256 x 256    1     512    1.62
#   17   512 x 512    1   17408    1.91         2   512 x 512    1    2048    1.87
# Every shape of at least 128 output tiles (16 x 16 pixels) wins, the one below (32 tiles) does not; nothing in between was
# measured, so the bit stays off there: the constant is the smallest tile count that was measured to win.
C64_MIN_TILES = 128


def use_c64(B: int, Hout: int, Wout: int, min_tiles: int = None) -> bool:
    """The emitter's rule for one 64 -> 64 conv whose OUTPUT map is ``Hout x Wout`` at batch ``B`` (``min_tiles``: default
    ``C64_MIN_TILES``, read at call time)."""
    return B * -(-Hout // 16) * -(-Wout // 16) >= (C64_MIN_TILES if min_tiles is None else min_tiles)


@dataclass
class TinyVAEConfig:
    latent_channels: int = 4
    out_channels: int = 3
    block_channels: Tuple[int, ...] = (64, 64, 64, 64)
    num_blocks: Tuple[int, ...] = (3, 3, 3, 1)
    latent_magnitude: float = 3.0
    scaling_factor: float = 1.0          # the latents arrive in scaled units
    force_upcast: bool = False

    def __post_init__(self):
        if any(int(c) != 64 for c in self.block_channels):
            raise ValueError(f"TinyVAEConfig: every block width must be 64 (TAESDXL), got {tuple(self.block_channels)}")
        if len(self.block_channels) != len(self.num_blocks) or not self.num_blocks:
            raise ValueError("TinyVAEConfig: block_channels and num_blocks must have the same, non-zero length")

    @property
    def scale_factor(self) -> int:
        return 2 ** (len(self.block_channels) - 1)


def layer_plan(cfg: TinyVAEConfig):
    """The decoder's parameterised layers in order: ("in" | "block" | "up" | "out", index into ``decoder.layers``)."""
    plan, idx = [("in", 0)], 2                          # (layers.1 is the ReLU behind conv_in)
    for i, n in enumerate(cfg.num_blocks):
        for _ in range(n):
            plan.append(("block", idx))
            idx += 1
        if i < len(cfg.num_blocks) - 1:
            plan.append(("up", idx + 1))                # (layers.idx is the Upsample)
            idx += 2
        else:
            plan.append(("out", idx))
            idx += 1
    return plan


def state_dict_keys(cfg: TinyVAEConfig = None):
    """The ``decoder.*`` keys of ``taesdxl``'s ``diffusion_pytorch_model.safetensors`` this decoder reads, in layer order."""
    keys = []
    for kind, n in layer_plan(cfg or TinyVAEConfig()):
        p = f"decoder.layers.{n}"
        if kind == "block":
            for k in (0, 2, 4):
                keys += [f"{p}.conv.{k}.weight", f"{p}.conv.{k}.bias"]
        elif kind == "up":
            keys.append(p + ".weight")
        else:
            keys += [p + ".weight", p + ".bias"]
    return keys


class _TinyNet:
    """What the two halves of TAESDXL share: the packed weights of a stack of 3x3 convs, loaded from one provider."""

    def __init__(self, cfg: TinyVAEConfig, provider, device="cuda"):
        self.cfg, self.device = cfg, torch.device(device)
        self.w: Dict[str, torch.Tensor] = {}
        self._load(Packer(provider, self.w, self.device))


class NativeTinyVAEDecoder(_TinyNet):
    def _load(self, pk):
        cfg = self.cfg
        # the synthetic stand-in: the last conv at gain 0.5 with 0.5 added to its biases, so that frames centre on mid-grey
        # instead of saturating at black; a real checkpoint (DictProvider) is taken as it is
        synthetic = isinstance(pk.pv, SyntheticProvider)
        for kind, n in layer_plan(cfg):
            p = f"decoder.layers.{n}"
            if kind == "in":
                pk.conv(p, cfg.latent_channels, 64, 3)
            elif kind == "block":
                for k in (0, 2, 4):
                    pk.conv(f"{p}.conv.{k}", 64, 64, 3)
            elif kind == "up":
                pk.conv(p, 64, 64, 3, bias=False)
            else:       # the decoder's final ``2 x - 1`` goes into the last conv
                pk.conv(p, 64, cfg.out_channels, 3, gain=0.5, bias_shift=0.5 if synthetic else 0.0, fold=True)

    def build(self, B: int, L, c64: bool = True, wrap: int = 0) -> "TinyVAEProgram":
        """``L``: latent side, or a pair ``(H, W)`` in latent pixels.  ``c64``: LB_GEMM_C64 on the 64 -> 64 convs where ``use_c64``
        says so (False: the same launches without the bit).  ``wrap``: wrap-around padding of every conv (``RecordedProgram``)."""
        return TinyVAEProgram(self, B, L, c64=c64, wrap=wrap)


class _TinyProgram(RecordedProgram):
    """What the programs of the two halves share: the 64 -> 64 conv with its LB_GEMM_C64 rule, and the residual block.  (A
    non-square program's unflagged 3x3 convs may take the ragged halo form, as in ``VAEProgram``.)"""

    def __init__(self, net: _TinyNet, B: int, L, c64: bool = True, wrap: int = 0):
        super().__init__(net, B, L, wrap=wrap)
        self.c64 = bool(c64)
        self.c64_launches = 0                   # convs recorded with the bit

    def _conv64(self, x, name, B, hin, win, *, ups=0, relu=True, residual=None):
        """One 64 -> 64 conv (on the nearest-2x upsampled map when ``ups``): flagged where the rule says so."""
        w = self.net.w
        g = lib.ConvGeom.conv3x3(hin, win, 64, ups=ups)
        ho, wo = g.Hout, g.Wout
        out = self.arena.alloc((B, ho, wo, 64))
        flags = lib.GEMM_RELU if relu else 0
        if self.c64 and use_c64(B, ho, wo):
            flags |= lib.GEMM_C64
            self.c64_launches += 1
        self.em.gemm(x, w[name + ".weight"], out, M=g.M(B), bias=w[name + ".bias"], residual=residual, flags=flags, splitk=False, conv=g)
        return out

    def _block(self, h, p, B, sh, sw):
        """relu(conv(relu(conv(relu(conv(h))))) + h) at ``p``.conv.{0,2,4}; takes ``h`` back to the arena."""
        ar = self.arena
        a = self._conv64(h, p + ".conv.0", B, sh, sw)
        b = self._conv64(a, p + ".conv.2", B, sh, sw)
        ar.release(a)
        o = self._conv64(b, p + ".conv.4", B, sh, sw, residual=h)
        ar.release(b)
        ar.release(h)
        return o


class TinyVAEProgram(_TinyProgram):
    """One recorded tiny decode for a fixed (batch, latent size); the surface of ``VAEProgram``."""

    def __init__(self, net: NativeTinyVAEDecoder, B: int, L, c64: bool = True, wrap: int = 0):
        super().__init__(net, B, L, c64, wrap=wrap)
        cfg, H, W, dev = net.cfg, self.H, self.W, net.device
        SH, SW = H * cfg.scale_factor, W * cfg.scale_factor
        self.z_in = torch.zeros(B, cfg.latent_channels, H, W, dtype=F16, device=dev)
        self.frames = torch.zeros(B, SH, SW, 3, dtype=torch.uint8, device=dev)
        self.image_f32 = torch.zeros(B, SH, SW, pad_to(cfg.out_channels, 4), dtype=F32, device=dev)
        self.prog = Program("tiny-vae-decode")
        with self._recording(self.prog):
            self._emit()

    def _emit(self):
        cfg, em, w, ar, B = self.net.cfg, self.em, self.net.w, self.arena, self.B
        sh, sw = self.H, self.W
        lc, lc_p = cfg.latent_channels, pad_to(cfg.latent_channels, 8)
        z8 = ar.alloc((B, sh, sw, lc_p))            # (pad channels written as zeros by the layout kernel)
        api.lb_nchw_to_nhwc_f16(self.z_in.data_ptr(), z8.data_ptr(), B, lc, sh * sw, lc_p, 1.0, _stream())
        h = None
        for kind, n in layer_plan(cfg):
            p = f"decoder.layers.{n}"
            if kind == "in":
                h = ar.alloc((B, sh, sw, 64))
                em.gemm(z8, w[p + ".weight"], h, M=B * sh * sw, bias=w[p + ".bias"], flags=lib.GEMM_RELU, splitk=False,
                        conv=lib.ConvGeom.conv3x3(sh, sw, lc_p))
                ar.release(z8)
            elif kind == "block":
                h = self._block(h, p, B, sh, sw)
            elif kind == "up":
                o = self._conv64(h, p, B, sh, sw, ups=1, relu=False)
                ar.release(h)
                h = o
                sh, sw = 2 * sh, 2 * sw
            else:
                em.gemm(h, w[p + ".weight"], self.image_f32, M=B * sh * sw, bias=w[p + ".bias"], flags=lib.GEMM_OUT_F32, splitk=False,
                        conv=lib.ConvGeom.conv3x3(sh, sw, 64))
                ar.release(h)
        api.lb_postprocess_u8(self.image_f32.data_ptr(), self.frames.data_ptr(), B * sh * sw, pad_to(cfg.out_channels, 4), 1, _stream())

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """z [B,4,H,W] final latents (scaled units) -> uint8 [B,8H,8W,3].  The decoder's input clamp ``tanh(z / 3) * 3`` is applied
        here, in torch (see the module docstring)."""
        m = float(self.net.cfg.latent_magnitude)
        self.z_in.copy_((m * torch.tanh(z.float() / m)).half())
        self.prog.launch()
        return self.frames


# ====================================================================== encoder
# The other half of the same checkpoint (``encoder.*``): the decoder's mirror image, restated from the published AutoencoderTiny
# encoder and held to a float64 restatement (tests/_taesd_enc_ref.py), as the decoder is:
#
#     x01 = (x + 1) / 2 with x in [-1, 1]                  (a uint8 picture: u8 / 255)
#     encoder.layers.0        conv 3 -> 64, bias, NO activation
#     per stage i (num_blocks mirrored: (1, 3, 3, 3)):
#         every stage but the first:  conv 64 -> 64, stride 2, pad 1, WITHOUT bias, no activation
#         block               relu(conv(relu(conv(relu(conv(x))))) + x), biased 64 -> 64 convs at encoder.layers.N.conv.{0,2,4}
#     encoder.layers.14       conv 64 -> 4, bias
#     layer indices: 0, [1], 2, [3-5], 6, [7-9], 10, [11-13], 14
#
# The output is latents in SCALED units (scaling_factor 1.0): UNet latents as they stand.  35 convs and one layout launch: the
# thirty block convs are the shape LB_GEMM_C64 was written for and take it where ``use_c64`` says so (``c64=False``: the same
# launches without the bit); the three stride-2 convs and conv_in (Cin padded to 8) run on the library's own routing - the
# implicit GEMM takes ``stride`` - and the last conv takes the narrow-N route.  No new kernel: LB_GEMM_C64 refuses stride 2 and
# three launches on maps of at most a quarter of the picture do not justify widening it (tools/tiny_encoder_bench.py ->
# profiles/tiny_encoder.txt holds the per-op record).  The picture is staged as fp16 ``u8 / 255`` by one torch elementwise
# (the counterpart of the decoder's tanh; the C ABI stays closed).  With the seeded synthetic stand-in weights nothing can be
# said about reconstruction quality.
def encoder_layer_plan(cfg: TinyVAEConfig = None):
    """The encoder's parameterised layers in order: ("in" | "down" | "block" | "out", index into ``encoder.layers``)."""
    cfg = cfg or TinyVAEConfig()
    plan, idx = [("in", 0)], 1
    for i, n in enumerate(reversed(cfg.num_blocks)):
        if i:
            plan.append(("down", idx))
            idx += 1
        for _ in range(n):
            plan.append(("block", idx))
            idx += 1
    plan.append(("out", idx))
    return plan


def encoder_state_dict_keys(cfg: TinyVAEConfig = None):
    """The ``encoder.*`` keys of ``taesdxl``'s ``diffusion_pytorch_model.safetensors`` the encoder reads, in layer order."""
    keys = []
    for kind, n in encoder_layer_plan(cfg):
        p = f"encoder.layers.{n}"
        if kind == "block":
            for k in (0, 2, 4):
                keys += [f"{p}.conv.{k}.weight", f"{p}.conv.{k}.bias"]
        elif kind == "down":
            keys.append(p + ".weight")
        else:
            keys += [p + ".weight", p + ".bias"]
    return keys


class NativeTinyVAEEncoder(_TinyNet):
    def _load(self, pk):
        cfg = self.cfg
        for kind, n in encoder_layer_plan(cfg):
            p = f"encoder.layers.{n}"
            if kind == "in":
                pk.conv(p, cfg.out_channels, 64, 3)
            elif kind == "block":
                for k in (0, 2, 4):
                    pk.conv(f"{p}.conv.{k}", 64, 64, 3)
            elif kind == "down":
                pk.conv(p, 64, 64, 3, bias=False)
            else:
                pk.conv(p, 64, cfg.latent_channels, 3)

    def build(self, B: int, L, c64: bool = True) -> "TinyEncoderProgram":
        """``L``: LATENT side, or a pair ``(H, W)`` in latent pixels (the picture is 8 times that).  ``c64`` as in the decoder."""
        return TinyEncoderProgram(self, B, L, c64=c64)


class TinyEncoderProgram(_TinyProgram):
    """One recorded tiny encode for a fixed (batch, latent size): uint8 pictures [B, 8H, 8W, 3] -> fp16 latents [B, 4, H, W]."""

    def __init__(self, net: NativeTinyVAEEncoder, B: int, L, c64: bool = True):
        super().__init__(net, B, L, c64)
        cfg, H, W, dev = net.cfg, self.H, self.W, net.device
        self.SH, self.SW = H * cfg.scale_factor, W * cfg.scale_factor
        self.pc, self.pc_p = cfg.out_channels, pad_to(cfg.out_channels, 8)
        self.x_in = torch.zeros(B, self.SH, self.SW, self.pc_p, dtype=F16, device=dev)      # NHWC; the pad channels stay zero
        self.latents = torch.zeros(B, cfg.latent_channels, H, W, dtype=F16, device=dev)
        self.prog = Program("tiny-vae-encode")
        with self._recording(self.prog):
            self._emit()

    def _emit(self):
        cfg, em, w, ar, B = self.net.cfg, self.em, self.net.w, self.arena, self.B
        sh, sw = self.SH, self.SW
        lc_p = pad_to(cfg.latent_channels, 4)
        h = None
        for kind, n in encoder_layer_plan(cfg):
            p = f"encoder.layers.{n}"
            if kind == "in":
                h = ar.alloc((B, sh, sw, 64))
                em.gemm(self.x_in, w[p + ".weight"], h, M=B * sh * sw, bias=w[p + ".bias"], flags=0, splitk=False,
                        conv=lib.ConvGeom.conv3x3(sh, sw, self.pc_p))
            elif kind == "block":
                h = self._block(h, p, B, sh, sw)
            elif kind == "down":
                g = lib.ConvGeom.conv3x3(sh, sw, 64, stride=2)
                ho, wo = g.Hout, g.Wout
                o = ar.alloc((B, ho, wo, 64))
                em.gemm(h, w[p + ".weight"], o, M=g.M(B), flags=0, splitk=False, conv=g)
                ar.release(h)
                h, sh, sw = o, ho, wo
            else:
                o = ar.alloc((B, sh, sw, lc_p))
                em.gemm(h, w[p + ".weight"], o, M=B * sh * sw, bias=w[p + ".bias"], flags=0, splitk=False,
                        conv=lib.ConvGeom.conv3x3(sh, sw, 64))
                ar.release(h)
                api.lb_nhwc_to_nchw_f16(o.data_ptr(), self.latents.data_ptr(), B, cfg.latent_channels, sh * sw, lc_p, _stream())
                ar.release(o)
        assert (sh, sw) == (self.H, self.W)

    def encode(self, u8: torch.Tensor) -> torch.Tensor:
        """uint8 pictures [B, 8H, 8W, 3] on the device -> fp16 latents [B, 4, H, W] in scaled units (the program's own buffer:
        clone what must outlive the next call).  ``u8 / 255`` is staged here, in torch (see the note above)."""
        if tuple(u8.shape) != (self.B, self.SH, self.SW, self.pc) or u8.dtype != torch.uint8:
            raise ValueError(f"TinyEncoderProgram.encode: expected uint8 {(self.B, self.SH, self.SW, self.pc)}, "
                             f"got {u8.dtype} {tuple(u8.shape)}")
        torch.div(u8, 255.0, out=self.x_in[..., :self.pc])
        self.prog.launch()
        return self.latents
