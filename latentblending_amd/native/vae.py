"""Native SDXL VAE decoder (diffusers ``AutoencoderKL.decode`` + ``VaeImageProcessor.postprocess``,
reached from /root/reference/latentblending/diffusers_holder.py:115-143) for gfx950.

Precision plan (replaces the reference's "upcast the whole VAE to fp32 on every decode",
diffusers_holder.py:129-139): the SDXL VAE overflows fp16 in its residual stream, not in its
normalised activations.  GroupNorm(+SiLU) outputs are bounded, so they are the fp16 MFMA operands
(fp32 accumulate); the residual stream itself (and conv outputs that only feed the next GroupNorm)
is kept in one of two formats:
  * ``stream_fp16_scaled`` (default): fp16 holding value * 2^-4 — range +-1e6, ~5e-4 relative
    precision, half the HBM traffic of fp32 for the bandwidth-bound GroupNorm passes and conv
    epilogues.  The scale rides along for free: conv epilogues use alpha = 2^-4 and biases
    pre-multiplied by 2^-4 (exact), GroupNorm is scale invariant once eps is scaled by 2^-8, and the
    1x1 shortcut / upsampler convs consume the scaled stream directly (linear ops);
  * fp32 stream (``stream_fp16_scaled=False``): ``OUT_F32`` epilogues, GroupNorm reads fp32, the
    two raw-stream contractions cast with the same 2^-4 scale and multiply back in the epilogue.
Either way the MFMA work runs at the fp16 rate (16x the fp32 MFMA rate on gfx950).
The mid-block attention (1 head, d = 512) is GEMM -> row softmax -> GEMM; its V bias is folded
into the output projection bias at load time (softmax rows sum to 1).
Output is quantised on device to uint8 NHWC frames.

The encoder (``AutoencoderKL.encode``: ``NativeVAEEncoder`` / ``VAEEncoderProgram``, at the end of this file) shares the weight
layouts (``_VAENet``) and the residual stream with its units (``_VAEStreamProgram``) with the decoder.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

import torch

from ..hip import lib
from ..hip.lib import api
from .runtime import Program, RecordedProgram, F16, F32, _stream
from .weights import Packer, pad_to

STREAM_SCALE = 1.0 / 16.0


@dataclass
class VAEConfig:
    latent_channels: int = 4
    out_channels: int = 3
    block_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_groups: int = 32
    scaling_factor: float = 0.13025
    force_upcast: bool = True
    stream_fp16_scaled: bool = True      # residual stream as fp16 * 2^-4 (False: fp32 stream)
    fuse_gn_stats: bool = True           # GroupNorm statistics from the producing conv's epilogue (LB_GEMM_CH_STATS): one pass over x
    fused_mid_attention: bool = True     # 512-channel mid-block attention as one lb_attn_fwd_d512 launch (no S x S score buffer)

    @property
    def scale_factor(self) -> int:
        return 2 ** (len(self.block_channels) - 1)


class _VAENet:
    """What the two halves of the SDXL VAE share: the packed weights, loaded from one provider - resnets, the mid-block attention
    (fused ``qkv`` when the top width is 512, V bias folded into ``to_out``) and the biases in stream units."""

    def __init__(self, cfg: VAEConfig, provider, device="cuda"):
        self.cfg, self.device = cfg, torch.device(device)
        self.w: Dict[str, torch.Tensor] = {}
        self._load(provider)

    def _resnet(self, pk, p, cin, cout):
        pk.norm(p + ".norm1", cin)
        pk.conv(p + ".conv1", cin, cout, 3)
        pk.norm(p + ".norm2", cout)
        pk.conv(p + ".conv2", cout, cout, 3, gain=0.5)
        if cin != cout:
            w = pk.pv.weight(p + ".conv_shortcut.weight", (cout, cin, 1, 1), cin, 1.0)
            self.w[p + ".conv_shortcut.weight"] = pk.dev(w.reshape(cout, cin), F16)
            self.w[p + ".conv_shortcut.bias"] = pk.dev(pk.pv.bias(p + ".conv_shortcut.bias", cout), F32)

    def _attention(self, pk, a, top):
        pv = pk.pv
        pk.norm(a + ".group_norm", top)
        pk.linear(a + ".to_q", top, top)
        pk.linear(a + ".to_k", top, top)
        wv = pv.weight(a + ".to_v.weight", (top, top), top)
        bv = pv.bias(a + ".to_v.bias", top)
        wo = pv.weight(a + ".to_out.0.weight", (top, top), top, 0.5)
        bo = pv.bias(a + ".to_out.0.bias", top)
        self.w[a + ".to_v.weight"] = pk.dev(wv, F16)
        self.w[a + ".to_out.0.weight"] = pk.dev(wo, F16)
        self.w[a + ".to_out.0.bias"] = pk.dev(bo + wo.half().float() @ bv, F32)   # V bias folded
        if top == 512:                      # fused form: ONE q | k | v projection feeding lb_attn_fwd_d512 (V bias folded as above)
            self.w[a + ".qkv.weight"] = torch.cat([self.w[a + ".to_q.weight"], self.w[a + ".to_k.weight"], self.w[a + ".to_v.weight"]], 0).contiguous()
            self.w[a + ".qkv.bias"] = torch.cat([self.w[a + ".to_q.bias"], self.w[a + ".to_k.bias"],
                                                 torch.zeros_like(self.w[a + ".to_q.bias"])], 0).contiguous()

    def _stream_biases(self):
        for key in [k for k in self.w if k.endswith(".bias")]:          # biases in stream units (x 2^-4, exact)
            self.w[key + "_s"] = self.w[key] * STREAM_SCALE


class NativeVAEDecoder(_VAENet):
    def _load(self, pv):
        cfg, pk = self.cfg, Packer(pv, self.w, self.device)
        rev = list(reversed(cfg.block_channels))
        top = rev[0]
        pk.conv("post_quant_conv", cfg.latent_channels, cfg.latent_channels, 1)
        pk.conv("decoder.conv_in", cfg.latent_channels, top, 3)
        self._resnet(pk, "decoder.mid_block.resnets.0", top, top)
        self._attention(pk, "decoder.mid_block.attentions.0", top)
        self._resnet(pk, "decoder.mid_block.resnets.1", top, top)
        prev = top
        for ui, c in enumerate(rev):
            for li in range(cfg.layers_per_block + 1):
                self._resnet(pk, f"decoder.up_blocks.{ui}.resnets.{li}", prev, c)
                prev = c
            if ui < len(rev) - 1:
                pk.upconv(f"decoder.up_blocks.{ui}.upsamplers.0.conv", c)
        pk.norm("decoder.conv_norm_out", rev[-1])
        pk.conv("decoder.conv_out", rev[-1], cfg.out_channels, 3, gain=0.5)
        self._stream_biases()

    def build(self, B: int, L, ragged_halo: bool = True, journal: bool = False, wrap: int = 0) -> "VAEProgram":
        """``L``: latent side, or a pair ``(H, W)`` in latent pixels (an int means ``(L, L)``).  ``journal``: the program's arena
        keeps its alloc / release journal (``Arena``); the recorded ops are the same."""
        return VAEProgram(self, B, L, ragged_halo=ragged_halo, journal=journal, wrap=wrap)


class _VAEStreamProgram(RecordedProgram):
    """What the programs of the two halves share: the residual stream in its two formats (module docstring) and the units built on it -
    stream convs with their GroupNorm operands and producer statistics, resnets, the mid-block attention."""

    def __init__(self, net: _VAENet, B: int, L, ragged_halo: bool = True, journal: bool = False, wrap: int = 0):
        super().__init__(net, B, L, ragged_halo=ragged_halo, journal=journal, wrap=wrap)
        cfg = net.cfg
        self.scaled = bool(cfg.stream_fp16_scaled)
        self.fuse_gn_stats = bool(getattr(cfg, "fuse_gn_stats", True))
        self.fused_mid_attention = bool(getattr(cfg, "fused_mid_attention", True))

    def _stream_units(self, m, t):
        """``capture``'s conversion: stream tensors in real units as fp32 (the 2^-4 of the scaled fp16 stream undone, exactly)."""
        return t.float() / STREAM_SCALE if (self.scaled and m.kind != "out") else t

    # ---- residual-stream format --------------------------------------------------------------
    # scaled (default): stream tensors hold value * 2^-4 in fp16;  f32: plain fp32 (see module docstring)
    def _stats_for(self, out, B, H, W, cin_p, cout_p, ks=3):
        """GroupNorm statistics from the producing conv's epilogue (LB_GEMM_CH_STATS): when the conv runs on the halo-tile
        kernel, attach a statistics buffer to its output tensor; the GroupNorm that consumes the tensor then skips its
        statistics pass (one read of the activation instead of two).  Returns the buffer or None."""
        rows = self.em.halo_stat_rows(B, H, W, cin_p, cout_p, ks) if self.fuse_gn_stats else 0
        if not rows:
            return None
        buf = self.arena.alloc((cout_p, B * rows, 2), F32)        # channel-major
        out._lb_chstats = (buf, rows)
        return buf

    def _stream_conv_args(self, H, W, cin, residual):
        """(flags, geometry) of a stream conv: the one copy ``_gn_for_conv`` plans with and ``_stream_conv`` launches."""
        flags = 0 if self.scaled else (lib.GEMM_OUT_F32 | (lib.GEMM_RES_F32 if residual else 0))
        return flags, lib.ConvGeom.conv3x3(H, W, pad_to(cin, 8))

    def _gn_for_conv(self, x, norm, silu, name, B, H, W, cin, *, residual=False):
        """The GroupNorm ``norm`` of ``x`` whose only consumer is the stream conv ``name``: emitted here (see ``Emitter.gn_operand``:
        the table kernel of a conv that applies the GroupNorm itself, or the GroupNorm launch as ever); pass the result to
        ``_stream_conv(x, name, ..., gn=...)``."""
        flags, conv = self._stream_conv_args(H, W, cin, residual)
        op = self.em.gn_operand(x, self.net.w[name + ".weight"], M=B * H * W, conv=conv, flags=flags, has_residual=residual,
                                **self._gn_args(x, norm, B, H * W, cin, silu))
        self._gn_done(x)
        return op

    def _stream_conv(self, x, name, B, H, W, cin, cout, *, residual=None, out=None, stats=True, gn=None):
        """3x3 conv whose output goes to the residual stream (or feeds only the next GroupNorm).  ``gn`` = what ``_gn_for_conv``
        returned for this conv: it consumes GroupNorm(x)."""
        w, sc = self.net.w, self.scaled
        cin_p, cout_p = pad_to(cin, 8), pad_to(cout, 4)
        if out is None:
            out = self.arena.alloc((B, H, W, cout_p), F16 if sc else F32)
        flags, conv = self._stream_conv_args(H, W, cin, residual is not None)
        st = self._stats_for(out, B, H, W, cin_p, cout_p) if stats else None
        self.em.gemm(x, w[name + ".weight"], out, M=B * H * W, bias=w[name + (".bias_s" if sc else ".bias")],
                     residual=residual, flags=flags, alpha=STREAM_SCALE if sc else 1.0, ch_stats=st, conv=conv, gn=gn)
        return out

    def _gn_args(self, x, name, B, HW, c, silu):
        """The GroupNorm ``name`` of ``x`` as the ``gn`` argument of ``Emitter.gemm`` (same numbers as ``_gn``)."""
        w = self.net.w
        eps = 1e-6 * (STREAM_SCALE * STREAM_SCALE if self.scaled else 1.0)     # GroupNorm of a scaled tensor
        return dict(gamma=w[name + ".weight"], beta=w[name + ".bias"], B=B, HW=HW, C_=c, eps=eps, silu=silu,
                    groups=self.net.cfg.norm_groups, ch_stats=getattr(x, "_lb_chstats", None))

    def _gn_done(self, x):
        st = getattr(x, "_lb_chstats", None)
        if st is not None:
            self.arena.release(st[0])
            x._lb_chstats = None

    def _gn(self, x, out, name, B, HW, c, silu):
        w = self.net.w
        eps = 1e-6 * (STREAM_SCALE * STREAM_SCALE if self.scaled else 1.0)     # GroupNorm of a scaled tensor
        st = getattr(x, "_lb_chstats", None)                                   # left by the conv that produced x?
        self.em.groupnorm(x, out, w[name + ".weight"], w[name + ".bias"], B=B, HW=HW, C_=c, eps=eps, silu=silu,
                          groups=self.net.cfg.norm_groups, ch_stats=st)
        if st is not None:
            self.arena.release(st[0])
            x._lb_chstats = None

    def _stream_as_operand(self, x, B, H, W, c):
        """The raw stream as an fp16 MFMA operand carrying the 2^-4 scale: free in scaled mode, a
        saturating down-scaling cast in fp32 mode.  Returns (tensor, owned)."""
        if self.scaled:
            return x, False
        x16 = self.arena.alloc((B, H, W, c))
        api.lb_cast_f32_to_f16(x.data_ptr(), x16.data_ptr(), x.numel(), STREAM_SCALE, _stream())
        return x16, True

    def _resnet(self, x, p, B, H, W, cin, cout):
        em, w, ar, sc = self.em, self.net.w, self.arena, self.scaled
        g1 = self._gn_for_conv(x, p + ".norm1", True, p + ".conv1", B, H, W, cin)
        h = self._stream_conv(x, p + ".conv1", B, H, W, cin, cout, gn=g1)
        g2 = self._gn_for_conv(h, p + ".norm2", True, p + ".conv2", B, H, W, cout, residual=True)
        if cin != cout:
            x16, owned = self._stream_as_operand(x, B, H, W, cin)
            xs = ar.alloc((B, H, W, cout), F16 if sc else F32)
            # operand carries the 2^-4 scale: scaled mode keeps it (bias pre-scaled), fp32 mode multiplies back
            em.gemm(x16, w[p + ".conv_shortcut.weight"], xs, M=B * H * W,
                    bias=w[p + (".conv_shortcut.bias_s" if sc else ".conv_shortcut.bias")],
                    flags=0 if sc else lib.GEMM_OUT_F32, alpha=1.0 if sc else 1.0 / STREAM_SCALE)
            if owned:
                ar.release(x16)
        else:
            xs = x
        out = self._stream_conv(h, p + ".conv2", B, H, W, cout, cout, residual=xs, gn=g2)
        ar.release(h)
        if xs is not x:
            ar.release(xs)
        return out

    def _mid_attention(self, h, a, B, H, W, c):
        """The mid-block attention whose weights sit under the prefix ``a``, added onto the stream ``h`` in place."""
        em, w, ar, sc = self.em, self.net.w, self.arena, self.scaled
        S = H * W
        n = ar.alloc((B * S, c))
        self._gn(h, n, a + ".group_norm", B, S, c, False)
        if self.fused_mid_attention and (a + ".qkv.weight") in w:
            qkv = ar.alloc((B * S, 3 * c))
            em.gemm(n, w[a + ".qkv.weight"], qkv, M=B * S, bias=w[a + ".qkv.bias"])
            ar.release(n)
            o = ar.alloc((B * S, c))
            em.attention(qkv.data_ptr(), qkv.data_ptr() + 2 * c, qkv.data_ptr() + 4 * c, o, B=B, H=1, Sq=S, Skv=S, valid=S,
                         ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c, head_dim=512)
            ar.release(qkv)
            return self._attn_out(o, h, a, B, S)
        q, k = ar.alloc((B * S, c)), ar.alloc((B * S, c))
        em.gemm(n, w[a + ".to_q.weight"], q, M=B * S, bias=w[a + ".to_q.bias"])
        em.gemm(n, w[a + ".to_k.weight"], k, M=B * S, bias=w[a + ".to_k.bias"])
        vt = ar.alloc((c, B * S))
        em.gemm(w[a + ".to_v.weight"], n, vt, M=c)                      # V^T (bias folded into to_out)
        ar.release(n)
        o = ar.alloc((B * S, c))
        scores = ar.alloc((S, S))
        for b in range(B):
            qb, kb, ob = q[b * S:(b + 1) * S], k[b * S:(b + 1) * S], o[b * S:(b + 1) * S]
            em.gemm(qb, kb, scores, M=S, alpha=float(c) ** -0.5)
            api.lb_softmax_rows_f16(scores.data_ptr(), S, S, S, 1.0, _stream())
            em.gemm(scores, vt[:, b * S:(b + 1) * S], ob, M=S, lda=S)    # W = V^T slice [c, S], ldw = B*S
        ar.release(scores); ar.release(q); ar.release(k); ar.release(vt)
        return self._attn_out(o, h, a, B, S)

    def _attn_out(self, o, h, a, B, S):
        em, w, ar, sc = self.em, self.net.w, self.arena, self.scaled
        em.gemm(o, w[a + ".to_out.0.weight"], h, M=B * S, bias=w[a + (".to_out.0.bias_s" if sc else ".to_out.0.bias")],
                residual=h, flags=0 if sc else (lib.GEMM_OUT_F32 | lib.GEMM_RES_F32), alpha=STREAM_SCALE if sc else 1.0)
        ar.release(o)
        return h


class VAEProgram(_VAEStreamProgram):
    """One recorded decode for a fixed (batch, latent size); ``L`` / ``ragged_halo`` / ``wrap``: ``RecordedProgram``.
    ``marks``: one ``Mark`` per emission unit (``conv_in`` = post_quant_conv + conv_in, every resnet and upsampler by its weight
    prefix, ``mid_attention``, ``image_f32``); ``tap_names`` maps the oracle's block taps (``mid``, ``up0`` ..) to units;
    ``capture()`` fills ``taps``."""

    def __init__(self, net: NativeVAEDecoder, B: int, L, ragged_halo: bool = True, journal: bool = False, wrap: int = 0):
        super().__init__(net, B, L, ragged_halo=ragged_halo, journal=journal, wrap=wrap)
        cfg, H, W = net.cfg, self.H, self.W
        dev = net.device
        SH, SW = H * cfg.scale_factor, W * cfg.scale_factor
        self.z_in = torch.zeros(B, cfg.latent_channels, H, W, dtype=F16, device=dev)
        self.frames = torch.zeros(B, SH, SW, 3, dtype=torch.uint8, device=dev)
        self.image_f32 = torch.zeros(B, SH, SW, pad_to(cfg.out_channels, 4), dtype=F32, device=dev)
        self._pq = torch.zeros(B, H, W, pad_to(cfg.latent_channels, 8), dtype=F16, device=dev)  # pad channels stay 0
        self.prog = Program("vae-decode")
        with self._recording(self.prog):
            self._emit()

    def capture(self) -> Dict[str, torch.Tensor]:
        """``RecordedProgram.capture`` on the latent ``z_in`` holds now (taps are NHWC).  Stream tensors come back in real units as
        fp32: the 2^-4 of the scaled fp16 stream is undone (exactly).  Leaves ``frames`` / ``image_f32`` as a ``decode`` would."""
        return super().capture(self._stream_units)

    def _emit(self):
        net, cfg, em, w, ar, B, LH, LW = self.net, self.net.cfg, self.em, self.net.w, self.arena, self.B, self.H, self.W
        sc = self.scaled
        rev = list(reversed(cfg.block_channels))
        top, lc = rev[0], cfg.latent_channels
        lc_p = pad_to(lc, 8)
        z8 = ar.alloc((B, LH, LW, lc_p))
        api.lb_nchw_to_nhwc_f16(self.z_in.data_ptr(), z8.data_ptr(), B, lc, LH * LW, lc_p, 1.0 / cfg.scaling_factor,
                                _stream())
        # post_quant_conv (1x1) writes the first `lc` channels of a zero-padded buffer
        em.gemm(z8, w["post_quant_conv.weight"], self._pq, M=B * LH * LW, bias=w["post_quant_conv.bias"], ldc=lc_p)
        ar.release(z8)
        h = self._stream_conv(self._pq, "decoder.conv_in", B, LH, LW, lc, top)
        at = self._mark("conv_in", "conv_in", h, "z_in")        # ``at``: the unit whose output h is
        nxt = self._resnet(h, "decoder.mid_block.resnets.0", B, LH, LW, top, top); ar.release(h); h = nxt
        at = self._mark("decoder.mid_block.resnets.0", "resnet", h, at)
        h = self._mid_attention(h, "decoder.mid_block.attentions.0", B, LH, LW, top)
        at = self._mark("mid_attention", "mid_attention", h, at)
        nxt = self._resnet(h, "decoder.mid_block.resnets.1", B, LH, LW, top, top); ar.release(h); h = nxt
        at = self.tap_names["mid"] = self._mark("decoder.mid_block.resnets.1", "resnet", h, at)
        sh, sw, prev = LH, LW, top                              # the current level's map is sh x sw
        for ui, c in enumerate(rev):
            for li in range(cfg.layers_per_block + 1):
                p = f"decoder.up_blocks.{ui}.resnets.{li}"
                nxt = self._resnet(h, p, B, sh, sw, prev, c)
                ar.release(h); h = nxt
                at = self._mark(p, "resnet", h, at)
                prev = c
            if ui < len(rev) - 1:
                h16, owned = self._stream_as_operand(h, B, sh, sw, c)
                name = f"decoder.up_blocks.{ui}.upsamplers.0.conv"
                up = ar.alloc((B, 2 * sh, 2 * sw, c), F16 if sc else F32)
                # (statistics only where the four sub-pixel convs run as ONE launch of the halo kernel: else _stats_for gives None)
                em.upconv(h16, w, name + ".weight", up, B=B, H=sh, W=sw, c=c, bias=w[name + (".bias_s" if sc else ".bias")],
                          flags=0 if sc else lib.GEMM_OUT_F32, alpha=1.0 if sc else 1.0 / STREAM_SCALE,
                          ch_stats=self._stats_for(up, B, sh, sw, c, c, ks=2))
                if owned:
                    ar.release(h16)
                ar.release(h)
                h = up
                sh, sw = 2 * sh, 2 * sw
                at = self._mark(name, "upsample", h, at)
            self.tap_names[f"up{ui}"] = at
        conv_out = lib.ConvGeom.conv3x3(sh, sw, pad_to(rev[-1], 8))
        g = em.gn_operand(h, w["decoder.conv_out.weight"], M=B * sh * sw, conv=conv_out, flags=lib.GEMM_OUT_F32,
                          **self._gn_args(h, "decoder.conv_norm_out", B, sh * sw, rev[-1], True))
        self._gn_done(h)
        em.gemm(h, w["decoder.conv_out.weight"], self.image_f32, M=B * sh * sw, bias=w["decoder.conv_out.bias"],
                flags=lib.GEMM_OUT_F32, conv=conv_out, gn=g)
        ar.release(h)
        self._mark("image_f32", "out", self.image_f32, at)
        api.lb_postprocess_u8(self.image_f32.data_ptr(), self.frames.data_ptr(), B * sh * sw,
                              pad_to(cfg.out_channels, 4), 1, _stream())

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """z [B,4,H,W] fp16 final latents (NOT yet divided by the scaling factor) -> uint8 [B,8H,8W,3]."""
        self.z_in.copy_(z)
        self.prog.launch()
        return self.frames


# ====================================================================== encoder
# The other half of the same checkpoint (``encoder.*``, ``quant_conv.*``): diffusers' ``AutoencoderKL.encode``, restated (no diffusers
# here; the tests pin the restatement against the latent-diffusion encoder that ``transformers`` ships as ``JanusVQVAEEncoder``):
#
#     x in [-1, 1]                                             (a uint8 picture: u8 / 127.5 - 1)
#     encoder.conv_in                     conv 3 -> ch[0], 3x3, pad 1
#     encoder.down_blocks.{i}.resnets.{0,1}                    widths ch = (128, 256, 512, 512); a 1x1 conv_shortcut where cin != cout
#     encoder.down_blocks.{0,1,2}.downsamplers.0.conv          3x3, stride 2, pad 0 on F.pad(x, (0, 1, 0, 1)): ONE zero row at the
#                                                              bottom and ONE zero column at the right (``ConvGeom.down3x3``)
#     encoder.mid_block.resnets.0, .attentions.0, .resnets.1   one head over all channels, as in the decoder
#     encoder.conv_norm_out -> SiLU -> encoder.conv_out        ch[-1] -> 8 (mean | logvar)
#     quant_conv                          8 -> 8, 1x1
#     moments -> mean, logvar = chunk(2); mode() = mean; sample = mean + exp(0.5 clamp(logvar, -30, 20)) randn
#     UNet latents = that * scaling_factor
#
# GroupNorm: 32 groups, eps 1e-6.  ``quant_conv`` is folded into ``encoder.conv_out`` at pack time, in float64 (W' = Wq Wout,
# b' = Wq bout + bq, rounded once): one narrow-N launch with N = 8 that writes the fp32 moments, no fp16 rounding between the two
# linear maps.  No new kernel: the stride-1 convs, GroupNorms and the attention are the decoder's launches; the three downsamplers
# run on the implicit GEMM, whose gather masks the far edge (every other conv route refuses stride 2 / pad 0).  The residual stream
# is the decoder's, in both formats: diffusers upcasts the whole VAE for ``encode`` as well.
def encoder_state_dict_keys(cfg: VAEConfig = None):
    """The ``encoder.*`` / ``quant_conv.*`` keys of the SDXL VAE's ``diffusion_pytorch_model.safetensors`` the encoder reads, in
    layer order (the order ``NativeVAEEncoder`` asks its provider for them)."""
    cfg = cfg or VAEConfig()
    ch = cfg.block_channels
    keys = []

    def both(p):
        keys.extend([p + ".weight", p + ".bias"])

    def resnet(p, cin, cout):
        for part in ("norm1", "conv1", "norm2", "conv2") + (("conv_shortcut",) if cin != cout else ()):
            both(f"{p}.{part}")

    both("encoder.conv_in")
    prev = ch[0]
    for bi, c in enumerate(ch):
        for li in range(cfg.layers_per_block):
            resnet(f"encoder.down_blocks.{bi}.resnets.{li}", prev, c)
            prev = c
        if bi < len(ch) - 1:
            both(f"encoder.down_blocks.{bi}.downsamplers.0.conv")
    resnet("encoder.mid_block.resnets.0", prev, prev)
    for part in ("group_norm", "to_q", "to_k", "to_v", "to_out.0"):
        both(f"encoder.mid_block.attentions.0.{part}")
    resnet("encoder.mid_block.resnets.1", prev, prev)
    both("encoder.conv_norm_out")
    both("encoder.conv_out")
    both("quant_conv")
    return keys


class NativeVAEEncoder(_VAENet):
    def _load(self, pv):
        cfg, pk = self.cfg, Packer(pv, self.w, self.device)
        ch = cfg.block_channels
        top, mc = ch[-1], 2 * cfg.latent_channels
        pk.conv("encoder.conv_in", cfg.out_channels, ch[0], 3)          # (Cin 3 padded to 8)
        prev = ch[0]
        for bi, c in enumerate(ch):
            for li in range(cfg.layers_per_block):
                self._resnet(pk, f"encoder.down_blocks.{bi}.resnets.{li}", prev, c)
                prev = c
            if bi < len(ch) - 1:
                pk.conv(f"encoder.down_blocks.{bi}.downsamplers.0.conv", c, c, 3)      # (the packing does not depend on the stride)
        self._resnet(pk, "encoder.mid_block.resnets.0", top, top)
        self._attention(pk, "encoder.mid_block.attentions.0", top)
        self._resnet(pk, "encoder.mid_block.resnets.1", top, top)
        pk.norm("encoder.conv_norm_out", top)
        # quant_conv (1x1) folded into conv_out, in float64, rounded once: ``encoder.moments`` = the conv that writes the moments
        wo = pv.weight("encoder.conv_out.weight", (mc, top, 3, 3), top * 9, 0.5).double()
        bo = pv.bias("encoder.conv_out.bias", mc).double()
        wq = pv.weight("quant_conv.weight", (mc, mc, 1, 1), mc).double().reshape(mc, mc)
        bq = pv.bias("quant_conv.bias", mc).double()
        mc_p = pad_to(mc, 4)
        packed = torch.zeros(mc_p, 3, 3, top, dtype=torch.float64)
        packed[:mc] = torch.einsum("om,mcyx->oyxc", wq, wo)
        bias = torch.zeros(mc_p, dtype=torch.float64)
        bias[:mc] = wq @ bo + bq
        self.w["encoder.moments.weight"] = pk.dev(packed.reshape(mc_p, 9 * top), F16)
        self.w["encoder.moments.bias"] = pk.dev(bias, F32)
        self._stream_biases()

    def build(self, B: int, L, ragged_halo: bool = True, journal: bool = False) -> "VAEEncoderProgram":
        """``L``: LATENT side, or a pair ``(H, W)`` in latent pixels (the picture is ``cfg.scale_factor`` times that)."""
        return VAEEncoderProgram(self, B, L, ragged_halo=ragged_halo, journal=journal)


def sample_moments(moments: torch.Tensor, generator=None, eps: torch.Tensor = None) -> torch.Tensor:
    """diffusers' ``DiagonalGaussianDistribution.sample`` on ``moments`` [..., 2 C] (channels last: mean | logvar):
    ``mean + exp(0.5 clamp(logvar, -30, 20)) eps`` in the moments' own arithmetic; ``eps``: given, or ``randn`` on the moments'
    device from ``generator``."""
    mean, logvar = moments.chunk(2, dim=-1)
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    if eps is None:
        eps = torch.randn(mean.shape, generator=generator, device=moments.device, dtype=moments.dtype)
    return mean + std * eps


class VAEEncoderProgram(_VAEStreamProgram):
    """One recorded encode for a fixed (batch, latent size): pictures [B, 8H, 8W, 3] -> fp32 ``moments_f32`` [B, H, W, 8] (mean | logvar,
    unscaled) and fp16 ``latents`` [B, 4, H, W] = mean * scaling_factor.  ``marks``: ``conv_in``, every resnet and downsampler by
    its weight prefix, ``mid_attention``, ``moments``; ``tap_names``: ``down0`` .. and ``mid``; ``capture()`` fills ``taps``."""

    def __init__(self, net: NativeVAEEncoder, B: int, L, ragged_halo: bool = True, journal: bool = False):
        super().__init__(net, B, L, ragged_halo=ragged_halo, journal=journal)
        cfg, H, W, dev = net.cfg, self.H, self.W, net.device
        self.SH, self.SW = H * cfg.scale_factor, W * cfg.scale_factor
        self.pc, self.pc_p = cfg.out_channels, pad_to(cfg.out_channels, 8)
        self.x_in = torch.zeros(B, self.SH, self.SW, self.pc_p, dtype=F16, device=dev)      # NHWC; the pad channels stay zero
        self.moments_f32 = torch.zeros(B, H, W, pad_to(2 * cfg.latent_channels, 4), dtype=F32, device=dev)
        self.latents = torch.zeros(B, cfg.latent_channels, H, W, dtype=F16, device=dev)
        self.prog = Program("vae-encode")
        with self._recording(self.prog):
            self._emit()

    def capture(self) -> Dict[str, torch.Tensor]:
        """``RecordedProgram.capture`` on the picture ``x_in`` holds now (taps are NHWC, stream tensors in real units as fp32).
        Leaves ``moments_f32`` / ``latents`` as an ``encode`` would."""
        return super().capture(self._stream_units)

    def _emit(self):
        cfg, em, w, ar, B, sc = self.net.cfg, self.em, self.net.w, self.arena, self.B, self.scaled
        ch = cfg.block_channels
        top, lc = ch[-1], cfg.latent_channels
        sh, sw = self.SH, self.SW
        h = self._stream_conv(self.x_in, "encoder.conv_in", B, sh, sw, self.pc, ch[0])
        at = self._mark("conv_in", "conv_in", h, "x_in")
        prev = ch[0]
        for bi, c in enumerate(ch):
            for li in range(cfg.layers_per_block):
                p = f"encoder.down_blocks.{bi}.resnets.{li}"
                nxt = self._resnet(h, p, B, sh, sw, prev, c)
                ar.release(h); h = nxt
                at = self._mark(p, "resnet", h, at)
                prev = c
            if bi < len(ch) - 1:
                name = f"encoder.down_blocks.{bi}.downsamplers.0.conv"
                g = lib.ConvGeom.down3x3(sh, sw, c)
                h16, owned = self._stream_as_operand(h, B, sh, sw, c)
                dn = ar.alloc((B, g.Hout, g.Wout, c), F16 if sc else F32)
                # operand carries the 2^-4 scale (as the decoder's upsampler): scaled mode keeps it, fp32 mode multiplies back.  The
                # implicit GEMM leaves no statistics: the GroupNorm behind it runs its two-pass form
                em.gemm(h16, w[name + ".weight"], dn, M=g.M(B), bias=w[name + (".bias_s" if sc else ".bias")],
                        flags=0 if sc else lib.GEMM_OUT_F32, alpha=1.0 if sc else 1.0 / STREAM_SCALE, conv=g)
                if owned:
                    ar.release(h16)
                ar.release(h)
                h, sh, sw = dn, g.Hout, g.Wout
                at = self._mark(name, "downsample", h, at)
            self.tap_names[f"down{bi}"] = at
        assert (sh, sw) == (self.H, self.W)
        nxt = self._resnet(h, "encoder.mid_block.resnets.0", B, sh, sw, top, top); ar.release(h); h = nxt
        at = self._mark("encoder.mid_block.resnets.0", "resnet", h, at)
        h = self._mid_attention(h, "encoder.mid_block.attentions.0", B, sh, sw, top)
        at = self._mark("mid_attention", "mid_attention", h, at)
        nxt = self._resnet(h, "encoder.mid_block.resnets.1", B, sh, sw, top, top); ar.release(h); h = nxt
        at = self.tap_names["mid"] = self._mark("encoder.mid_block.resnets.1", "resnet", h, at)
        conv_out = lib.ConvGeom.conv3x3(sh, sw, top)
        g = em.gn_operand(h, w["encoder.moments.weight"], M=B * sh * sw, conv=conv_out, flags=lib.GEMM_OUT_F32,
                          **self._gn_args(h, "encoder.conv_norm_out", B, sh * sw, top, True))
        self._gn_done(h)
        em.gemm(h, w["encoder.moments.weight"], self.moments_f32, M=B * sh * sw, bias=w["encoder.moments.bias"],
                flags=lib.GEMM_OUT_F32, conv=conv_out, gn=g)
        ar.release(h)
        self._mark("moments", "out", self.moments_f32, at)
        mc_p = self.moments_f32.shape[-1]
        m16 = ar.alloc((B, sh, sw, mc_p))
        api.lb_cast_f32_to_f16(self.moments_f32.data_ptr(), m16.data_ptr(), self.moments_f32.numel(), float(cfg.scaling_factor), _stream())
        api.lb_nhwc_to_nchw_f16(m16.data_ptr(), self.latents.data_ptr(), B, lc, sh * sw, mc_p, _stream())     # (the mean half)
        ar.release(m16)

    def encode_normalized(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, 3, 8H, 8W] in [-1, 1] (any float dtype) -> ``latents``; the picture is rounded to the fp16 operand here."""
        if tuple(x.shape) != (self.B, self.pc, self.SH, self.SW) or not x.is_floating_point():
            raise ValueError(f"VAEEncoderProgram.encode_normalized: expected a float tensor {(self.B, self.pc, self.SH, self.SW)}, "
                             f"got {x.dtype} {tuple(x.shape)}")
        self.x_in[..., :self.pc].copy_(x.permute(0, 2, 3, 1))
        self.prog.launch()
        return self.latents

    def encode(self, u8: torch.Tensor) -> torch.Tensor:
        """uint8 pictures [B, 8H, 8W, 3] on the device -> fp16 latents [B, 4, H, W] in scaled units (the program's own buffer:
        clone what must outlive the next call).  ``f16(fp32(u8) / 127.5 - 1)`` is staged here, in torch, as the tiny encoder stages
        ``u8 / 255``."""
        if tuple(u8.shape) != (self.B, self.SH, self.SW, self.pc) or u8.dtype != torch.uint8:
            raise ValueError(f"VAEEncoderProgram.encode: expected uint8 {(self.B, self.SH, self.SW, self.pc)}, "
                             f"got {u8.dtype} {tuple(u8.shape)}")
        self.x_in[..., :self.pc].copy_(u8.to(F32) / 127.5 - 1.0)
        self.prog.launch()
        return self.latents

    def moments(self) -> torch.Tensor:
        """The fp32 moments [B, H, W, 8] (mean | logvar, unscaled) of the last encode: the program's own buffer."""
        return self.moments_f32[..., :2 * self.net.cfg.latent_channels]
