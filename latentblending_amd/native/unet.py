"""Native SDXL UNet: weight packing + launch-program builder for gfx950.

Architecture = diffusers ``UNet2DConditionModel`` as configured for SDXL base / turbo (SURVEY.md
Appendix B.1; reached from /root/reference/latentblending/diffusers_holder.py:336).  What is
MI355X-specific here:

* NHWC fp16 activations end to end: a feature map IS the [tokens, channels] matrix the
  transformer blocks consume, so resnets and transformers share buffers with no permutes;
* every Linear / Conv is one launch of the MFMA GEMM / implicit-GEMM kernel with its bias,
  time-embedding add, residual add or GEGLU fused into the epilogue; nearest-2x upsampling and
  stride-2 downsampling are folded into the conv's gather;
* work that does not depend on the image is batched into a few fat GEMMs instead of hundreds of
  tiny launches: all 17 resnets' time-embedding projections = 1 GEMM; all 70 cross-attention
  K and V projections of the (padded) text context = 1 GEMM (N = 166,400), kept in a separate
  *conditioning program* that only re-runs when the conditioning changes;
* Q, K and V of a self-attention come out of ONE [tokens, 3C] projection and the attention kernel reads the
  three column slices in place (V through the LDS transpose read): no V^T copy, one launch instead of two;
* the whole forward is recorded once per (batch, latent size) and replayed from C++ / hipGraph.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..hip import lib
from ..hip.lib import api
from .geometry import check_unet_latent_size, latent_hw
from .runtime import Program, RecordedProgram, F16, F32, _stream
from .weights import Packer, Reloadable, pad_to

CTX_TOKENS = 77
CTX_PAD = 80


@dataclass
class UNetConfig:
    in_channels: int = 4
    out_channels: int = 4
    block_channels: Tuple[int, ...] = (320, 640, 1280)
    layers_per_block: int = 2
    transformer_depth: Tuple[int, ...] = (0, 2, 10)
    head_dim: int = 64
    cross_dim: int = 2048
    pooled_dim: int = 1280
    add_time_dim: int = 256
    sample_size: int = 128
    norm_groups: int = 32
    time_cond_proj_dim: Optional[int] = None

    @property
    def time_embed_dim(self) -> int:
        return self.block_channels[0] * 4

    @property
    def add_in_dim(self) -> int:
        return self.pooled_dim + 6 * self.add_time_dim


class EncoderPacking(Reloadable):
    """Weight packing of the UNet's encoder half - conv_in, the two embedding MLPs, the down blocks and the mid block - and of the two
    fused projections (``temb_proj``, ``ctx_kv``) over whatever resnets and cross-attention blocks a model packed: shared by
    ``NativeUNet`` and ``controlnet.NativeControlNet``, whose encoder is the UNet's over again.  A subclass sets ``cfg``, ``device``,
    ``w``, ``fuse_layernorm`` / ``keep_ln_weights`` and the two slice tables before it packs."""

    def _init_packing(self, cfg, device, fuse_layernorm):
        assert cfg.head_dim == 64, "attention kernel is specialised for head_dim 64"
        assert fuse_layernorm in (False, True, "auto")
        self.cfg, self.device = cfg, torch.device(device)
        self.fuse_layernorm = fuse_layernorm
        self.keep_ln_weights = fuse_layernorm is not True
        self.w: Dict[str, torch.Tensor] = {}
        self.temb_slices: Dict[str, Tuple[int, int]] = {}      # resnet -> (offset, cout) in the fused projection
        self.ctx_slices: Dict[str, Tuple[int, int]] = {}       # transformer block -> (offset, C) in fused ctx K / V

    # ------------------------------------------------------------------ weights -----------
    def _ln_linear(self, pk, norm_name, key, w: torch.Tensor, bias: Optional[torch.Tensor], c: int):
        """LayerNorm folded into the Linear that consumes it (``LB_GEMM_LN_A``): y = LN(x) W^T + b becomes
        rstd * (x W'^T - mean * colsum) + b' with W' = W diag(gamma) (rounded to fp16: the MFMA operand),
        colsum[n] = sum_k W'[n][k] (of the ROUNDED values) and b' = b + W beta.  ``key`` names the packed tensors."""
        g, beta = pk.norm(norm_name, c, keep_host=not self.keep_ln_weights)
        if self.fuse_layernorm is False:        # stand-alone LayerNorms only: no folded copies of the weights in HBM
            return
        wf = (w.double() * g.double()[None, :]).to(torch.float16)
        self.w[key + ".weight"] = wf.to(self.device).contiguous()
        self.w[key + ".colsum"] = pk.dev(wf.double().sum(dim=1), F32)
        b2 = w.double() @ beta.double()
        if bias is not None:
            b2 = b2 + bias.double()
        self.w[key + ".bias"] = pk.dev(b2, F32)

    def _resnet(self, pk, p, cin, cout, temb_acc):
        T = self.cfg.time_embed_dim
        pk.norm(p + ".norm1", cin)
        pk.conv(p + ".conv1", cin, cout, 3)
        tw = pk.pv.weight(p + ".time_emb_proj.weight", (cout, T), T, 1.0)
        tb = pk.pv.bias(p + ".time_emb_proj.bias", cout)
        self.temb_slices[p] = (temb_acc["n"], cout)
        temb_acc["w"].append(tw)
        temb_acc["b"].append(tb)
        temb_acc["n"] += cout
        pk.norm(p + ".norm2", cout)
        pk.conv(p + ".conv2", cout, cout, 3, gain=0.5)
        if cin != cout:
            # 1x1 shortcut as a plain GEMM on [tokens, cin]
            w = pk.pv.weight(p + ".conv_shortcut.weight", (cout, cin, 1, 1), cin, 1.0)
            self.w[p + ".conv_shortcut.weight"] = pk.dev(w.reshape(cout, cin), F16)
            self.w[p + ".conv_shortcut.bias"] = pk.dev(pk.pv.bias(p + ".conv_shortcut.bias", cout), F32)

    def _transformer(self, pk, p, c, depth, ctx_acc):
        X = self.cfg.cross_dim
        pk.norm(p + ".norm", c)
        pk.linear(p + ".proj_in", c, c)
        for d in range(depth):
            b = f"{p}.transformer_blocks.{d}"
            q = pk.linear(b + ".attn1.to_q", c, c, bias=False, keep_host=True)
            k = pk.linear(b + ".attn1.to_k", c, c, bias=False, keep_host=True)
            v = pk.linear(b + ".attn1.to_v", c, c, bias=False, keep_host=True)
            qkv = torch.cat([q, k, v], 0)                                             # one [3C, C] projection
            if self.keep_ln_weights:
                self.w[b + ".attn1.qkv"] = pk.dev(qkv, F16)
            self._ln_linear(pk, b + ".norm1", b + ".attn1.qkv_ln", qkv, None, c)
            pk.linear(b + ".attn1.to_out.0", c, c, gain=0.5)
            q2 = pk.linear(b + ".attn2.to_q", c, c, bias=False, keep_host=not self.keep_ln_weights)
            self._ln_linear(pk, b + ".norm2", b + ".attn2.to_q_ln", q2, None, c)
            ck = pk.linear(b + ".attn2.to_k", X, c, bias=False, keep_host=True)
            cv = pk.linear(b + ".attn2.to_v", X, c, bias=False, keep_host=True)
            self.ctx_slices[b] = (ctx_acc["n"], c)
            ctx_acc["k"].append(ck)
            ctx_acc["v"].append(cv)
            ctx_acc["n"] += c
            pk.linear(b + ".attn2.to_out.0", c, c, gain=0.5)
            ff = pk.linear(b + ".ff.net.0.proj", c, 8 * c, keep_host=not self.keep_ln_weights)
            ffb = pk.pv.bias(b + ".ff.net.0.proj.bias", 8 * c)                   # (same seeded tensor linear stored)
            self._ln_linear(pk, b + ".norm3", b + ".ff.net.0.proj_ln", ff, ffb, c)
            pk.linear(b + ".ff.net.2", 4 * c, c, gain=0.5)
        pk.linear(p + ".proj_out", c, c, gain=0.5)

    def skip_channels(self) -> List[int]:
        ch = self.cfg.block_channels
        skips = [ch[0]]
        for bi, c in enumerate(ch):
            skips += [c] * self.cfg.layers_per_block
            if bi < len(ch) - 1:
                skips.append(c)
        return skips

    def _load_encoder(self, pk, temb_acc, ctx_acc):
        """conv_in, the embedding MLPs, the down blocks and the mid block, in the order the state dict lists them."""
        cfg = self.cfg
        ch, T = cfg.block_channels, cfg.time_embed_dim
        pk.conv("conv_in", cfg.in_channels, ch[0], 3)
        if getattr(cfg, "time_cond_proj_dim", None) is not None:
            # guidance-distilled UNets (LCM-SDXL and its kin): the guidance-scale embedding is projected onto the timestep
            # sinusoid in front of linear_1 (diffusers TimestepEmbedding.cond_proj: Linear(time_cond_proj_dim, C0, bias=False))
            if cfg.time_cond_proj_dim <= 0 or cfg.time_cond_proj_dim % 8:
                raise ValueError(f"UNetConfig.time_cond_proj_dim must be a positive multiple of 8 (got {cfg.time_cond_proj_dim})")
            pk.linear("time_embedding.cond_proj", cfg.time_cond_proj_dim, ch[0], bias=False)
        pk.linear("time_embedding.linear_1", ch[0], T)
        pk.linear("time_embedding.linear_2", T, T)
        pk.linear("add_embedding.linear_1", cfg.add_in_dim, T)
        pk.linear("add_embedding.linear_2", T, T)
        prev = ch[0]
        for bi, c in enumerate(ch):
            for li in range(cfg.layers_per_block):
                self._resnet(pk, f"down_blocks.{bi}.resnets.{li}", prev, c, temb_acc)
                if cfg.transformer_depth[bi]:
                    self._transformer(pk, f"down_blocks.{bi}.attentions.{li}", c, cfg.transformer_depth[bi], ctx_acc)
                prev = c
            if bi < len(ch) - 1:
                pk.conv(f"down_blocks.{bi}.downsamplers.0.conv", c, c, 3)
        c = ch[-1]
        self._resnet(pk, "mid_block.resnets.0", c, c, temb_acc)
        self._transformer(pk, "mid_block.attentions.0", c, cfg.transformer_depth[-1], ctx_acc)
        self._resnet(pk, "mid_block.resnets.1", c, c, temb_acc)

    def _load_fused(self, pk, temb_acc, ctx_acc):
        """The two fused projections over everything packed so far."""
        self.w["temb_proj.weight"] = pk.dev(torch.cat(temb_acc["w"], 0), F16)
        self.w["temb_proj.bias"] = pk.dev(torch.cat(temb_acc["b"], 0), F32)
        # every cross-attention K projection, then every V projection, of the text context: ONE [2 n_ctx, X] weight
        self.w["ctx_kv.weight"] = pk.dev(torch.cat(ctx_acc["k"] + ctx_acc["v"], 0), F16)
        self.n_temb, self.n_ctx = temb_acc["n"], ctx_acc["n"]

    def weight_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.w.values() if t is not None)


class NativeUNet(EncoderPacking):
    def __init__(self, cfg: UNetConfig, provider, device="cuda", fuse_layernorm="auto"):
        """``fuse_layernorm``: fold the three LayerNorms of every transformer block into the GEMMs that consume them
        (LB_GEMM_LN_A: no LayerNorm launch, no normalised copy of the hidden state).
        ``"auto"`` (default): per launch program - folded (``True`` form) when the program is LAUNCH-bound, i.e. at most 1024
        tokens at the deepest level (the B = 2 anchor program at 512^2: 916 -> 706 launches, 12.40 -> 11.94 ms per forward),
        stand-alone LayerNorms otherwise (B = 17: the fold costs 38.1 -> 42.0 ms; profiles/r03_ln_inloop_ab.txt).  Both
        weight forms stay resident (+2.4 GB of 288 GB).
        ``True``: row statistics accumulated inside the consumer's K loop.  Not for MFMA-bound programs: on MI355X the 64 v_dot2 per
        K-tile and wave cost the MFMA loop more than the 6 us LayerNorm launch they replace
        (profiles/r02_ln_gemm_bench.txt: QKV 57.1 + 6.4 us separate vs 70.0 us fused at B=17; GEGLU 132 + 6 vs 166).
        (A third form - row statistics written by the PRODUCING GEMM's epilogue - was measured slower than the stand-alone
        LayerNorm at B = 2 and B = 17 alike and removed in round 3: profiles/r02_ln_stats_ab.txt.)"""
        self._init_packing(cfg, device, fuse_layernorm)
        self._load(provider)

    def up_plan(self):
        skips = self.skip_channels()
        plan, hidden = [], self.cfg.block_channels[-1]
        for c in reversed(self.cfg.block_channels):
            cins = []
            for _ in range(self.cfg.layers_per_block + 1):
                cins.append((hidden, skips.pop()))
                hidden = c
            plan.append((c, cins))
        return plan

    def _load(self, pv):
        cfg, pk = self.cfg, Packer(pv, self.w, self.device)
        ch = cfg.block_channels
        temb_acc = {"w": [], "b": [], "n": 0}
        ctx_acc = {"k": [], "v": [], "n": 0}
        self._load_encoder(pk, temb_acc, ctx_acc)
        depths = list(reversed(cfg.transformer_depth))
        for ui, (c, cins) in enumerate(self.up_plan()):
            for li, (hid, skip) in enumerate(cins):
                self._resnet(pk, f"up_blocks.{ui}.resnets.{li}", hid + skip, c, temb_acc)
                if depths[ui]:
                    self._transformer(pk, f"up_blocks.{ui}.attentions.{li}", c, depths[ui], ctx_acc)
            if ui < len(ch) - 1:
                pk.upconv(f"up_blocks.{ui}.upsamplers.0.conv", c)
        pk.norm("conv_norm_out", ch[0])
        pk.conv("conv_out", ch[0], cfg.out_channels, 3, gain=0.5)
        self._load_fused(pk, temb_acc, ctx_acc)

    # ------------------------------------------------------------------ program -----------
    def build(self, B: int, L, ragged_halo: bool = True, journal: bool = False, wrap: int = 0, control=None) -> "UNetProgram":
        """``L``: latent side, or a pair ``(H, W)`` in latent pixels (an int means ``(L, L)``).  ``journal``: the program's arena
        keeps its alloc / release journal (``Arena``); the recorded ops are the same.  ``wrap``: wrap-around padding of conv_in, every
        resnet conv, downsampler, upsampler and conv_out (bit 0: the columns wrap, bit 1: the rows; ``RecordedProgram``).
        ``control``: a ``NativeControlNet`` whose residuals the step program adds (``UNetProgram``); None: the plain program."""
        return UNetProgram(self, B, L, ragged_halo=ragged_halo, journal=journal, wrap=wrap, control=control)


class _Side:
    """One network of a UNet program as the shared emitters read it: the packed model (weights, the layouts of its two fused
    projections), the outputs of its conditioning units (``aug``, ``ctx_kv``), its ``temb_all`` once emitted, and the prefix its
    marks carry ("" for the UNet, "control." for a ControlNet)."""

    def __init__(self, net, prefix: str, aug: torch.Tensor, ctx_kv: Optional[torch.Tensor], timestep_cond=None):
        self.net, self.prefix, self.aug, self.ctx_kv, self.timestep_cond = net, prefix, aug, ctx_kv, timestep_cond
        self.temb_all: Optional[torch.Tensor] = None


class UNetProgram(RecordedProgram):
    """One recorded forward for a fixed (batch, latent size).  Inputs are device buffers the
    caller fills (torch copies on the launch stream); ``run`` replays the launches.  ``L`` / ``ragged_halo`` / ``wrap``: ``RecordedProgram``.
    ``marks``: one ``Mark`` per emission unit (``aug`` and ``ctx_kv`` of the conditioning program; ``temb_all``, ``conv_in``, every
    resnet / transformer / downsampler / upsampler by its weight prefix, and ``eps``); ``tap_names`` maps the block taps of the
    oracle (``conv_in``, ``down0`` .., ``mid``, ``up0`` ..) to the unit whose output they are.  ``capture()`` fills ``taps`` from the
    inputs ``set_conditioning`` / ``forward`` left in the buffers (fp16, NHWC for feature maps) and leaves ``eps`` as a ``forward`` would.

    ``control``: a ``controlnet.NativeControlNet`` - the step program then holds BOTH networks.  The ControlNet's encoder and mid block
    run first on ``x_in`` (its conv_in adds ``hint_emb``, the embedded control image: ``set_hint``) and keep their hidden maps; after
    the UNet's own mid block one GEMM per skip computes the zero conv and adds it to the UNet's skip copy in place (``control.zero.k``;
    ``control.zero.mid`` into the mid block's output), then the up path runs.  Its units are marked ``control.<name>``; the
    conditioning program also computes ``control.aug`` and ``control.ctx_kv``.  ``None``: the program of ever, op for op."""

    def __init__(self, net: NativeUNet, B: int, L, ragged_halo: bool = True, journal: bool = False, wrap: int = 0, control=None):
        cfg = net.cfg
        H, W = latent_hw(L)
        check_unet_latent_size(H, W, len(cfg.block_channels))
        super().__init__(net, B, L, ragged_halo=ragged_halo, journal=journal, wrap=wrap)
        # LayerNorm handling of THIS program ("auto": fold into the consumers only where the program is launch-bound)
        self.ln_mode = net.fuse_layernorm if net.fuse_layernorm != "auto" else (B * max(H // 4, 1) * max(W // 4, 1) <= 1024)
        dev = net.device
        T = cfg.time_embed_dim
        # ---- inputs / outputs (persistent) ----
        self.x_in = torch.zeros(B, cfg.in_channels, H, W, dtype=F16, device=dev)
        self.tvals = torch.zeros(B, 1, dtype=F32, device=dev)
        self.time_ids = torch.zeros(B, 6, dtype=F32, device=dev)
        self.ctx = torch.zeros(B, CTX_PAD, cfg.cross_dim, dtype=F16, device=dev)     # rows 77..79 stay zero
        self.text_embeds = torch.zeros(B, cfg.pooled_dim, dtype=F16, device=dev)
        self.eps = torch.zeros(B, cfg.out_channels, H, W, dtype=F16, device=dev)
        # guidance-scale embedding of guidance-distilled UNets, one row per sample (None for every other config)
        self.timestep_cond = None if cfg.time_cond_proj_dim is None else torch.zeros(B, cfg.time_cond_proj_dim, dtype=F16, device=dev)
        # ---- conditioning-program outputs (persistent) ----
        self.aug = torch.zeros(B, T, dtype=F16, device=dev)
        self.ctx_kv = torch.zeros(B * CTX_PAD, 2 * net.n_ctx, dtype=F16, device=dev)   # [K of all blocks | V of all blocks]
        self.side = self._unet_side = _Side(net, "", self.aug, self.ctx_kv, self.timestep_cond)
        self.control, self._control_side, self.hint_emb = control, None, None
        if control is not None:
            control.check_fits(net)
            self.hint_emb = torch.zeros(B, H, W, cfg.block_channels[0], dtype=F16, device=dev)     # the embedded hint, one copy per sample
            self._control_side = _Side(control, "control.", torch.zeros(B, T, dtype=F16, device=dev),
                                       torch.zeros(B * CTX_PAD, 2 * control.n_ctx, dtype=F16, device=dev) if control.n_ctx else None)
        self.prog_cond = Program("unet-cond")
        self.prog_step = Program("unet-step")
        with self._recording(self.prog_cond):
            self._emit_cond(self._unet_side)
            if control is not None:
                self._emit_cond(self._control_side)
        with self._recording(self.prog_step):
            self._emit_step()

    def set_hint(self, emb: torch.Tensor) -> None:
        """``emb`` [1, H, W, C0] fp16 (``controlnet.HintProgram.embed``): the same embedded hint for every sample of the batch."""
        if self.hint_emb is None:
            raise ValueError("UNetProgram.set_hint: this program was built without a ControlNet")
        if tuple(emb.shape[-3:]) != tuple(self.hint_emb.shape[1:]):
            raise ValueError(f"UNetProgram.set_hint: the embedded hint is {tuple(emb.shape)} but the program takes {tuple(self.hint_emb.shape[1:])}")
        self.hint_emb.copy_(emb.reshape(1, *self.hint_emb.shape[1:]).expand_as(self.hint_emb))

    # ---- helpers ------------------------------------------------------------------------
    def _conv(self, x, name, B, H, W, cin, cout, *, stride=1, ups=0, rowvec=None, ld_rowvec=None,
              residual=None, out=None, flags=0, k=3, pad=1):
        em, w = self.em, self.side.net.w
        cin_p, cout_p = pad_to(cin, 8), pad_to(cout, 4)
        g = lib.ConvGeom(H, W, cin_p, k, k, stride=stride, pad=pad, ups=ups)
        ho, wo = g.Hout, g.Wout
        if out is None:
            out = self.arena.alloc((B, ho, wo, cout_p), F32 if flags & lib.GEMM_OUT_F32 else F16)
        em.gemm(x, w[name + ".weight"], out, M=g.M(B), bias=w[name + ".bias"], residual=residual,
                rowvec=rowvec, rows_per_batch=ho * wo, ld_rowvec=ld_rowvec, flags=flags, conv=g)
        return out, ho, wo

    def _upconv(self, x, name, B, H, W, c):
        """nearest-2x upsample + 3x3 conv as sub-pixel 2x2 convs scattered into the 2H x 2W output (``Emitter.upconv``)."""
        w = self.side.net.w
        out = self.arena.alloc((B, 2 * H, 2 * W, c))
        self.em.upconv(x, w, name + ".weight", out, B=B, H=H, W=W, c=c, bias=w[name + ".bias"])
        return out, 2 * H, 2 * W

    def _resnet(self, x, p, B, H, W, cin, cout):
        s = self.side
        em, w, ar, g = self.em, s.net.w, self.arena, s.net.cfg.norm_groups
        n1 = ar.alloc((B, H, W, cin))
        em.groupnorm(x, n1, w[p + ".norm1.weight"], w[p + ".norm1.bias"], B=B, HW=H * W, C_=cin, eps=1e-5,
                     silu=True, groups=g)
        off, _ = s.net.temb_slices[p]
        rv = s.temb_all[:, off:]                        # column slice: pointer offset + ld = n_temb
        h, _, _ = self._conv(n1, p + ".conv1", B, H, W, cin, cout, rowvec=rv, ld_rowvec=s.net.n_temb)
        ar.release(n1)
        n2 = ar.alloc((B, H, W, cout))
        em.groupnorm(h, n2, w[p + ".norm2.weight"], w[p + ".norm2.bias"], B=B, HW=H * W, C_=cout, eps=1e-5,
                     silu=True, groups=g)
        ar.release(h)
        if cin != cout:
            xs = ar.alloc((B, H, W, cout))
            em.gemm(x, w[p + ".conv_shortcut.weight"], xs, M=B * H * W, bias=w[p + ".conv_shortcut.bias"])
        else:
            xs = x
        out, _, _ = self._conv(n2, p + ".conv2", B, H, W, cout, cout, residual=xs)
        ar.release(n2)
        if xs is not x:
            ar.release(xs)
        return out

    def _transformer(self, x, p, B, H, W, c, depth):
        s = self.side
        em, w, ar = self.em, s.net.w, self.arena
        M, S, heads = B * H * W, H * W, c // 64
        n = ar.alloc((M, c))
        em.groupnorm(x, n, w[p + ".norm.weight"], w[p + ".norm.bias"], B=B, HW=S, C_=c, eps=1e-6, silu=False,
                     groups=s.net.cfg.norm_groups)
        h = ar.alloc((M, c))
        mode = self.ln_mode
        em.gemm(n, w[p + ".proj_in.weight"], h, M=M, bias=w[p + ".proj_in.bias"])
        ar.release(n)
        for d in range(depth):
            b = f"{p}.transformer_blocks.{d}"
            # --- self attention ---
            fuse = mode is True
            qkv = ar.alloc((M, 3 * c))
            if fuse:        # LayerNorm folded into the projection: affine in the epilogue, statistics from the A fragments or from `st`
                em.gemm(h, w[b + ".attn1.qkv_ln.weight"], qkv, M=M, bias=w[b + ".attn1.qkv_ln.bias"],
                        ln=(w[b + ".attn1.qkv_ln.colsum"], 1e-5))
            else:
                ln = ar.alloc((M, c))
                em.layernorm(h, ln, w[b + ".norm1.weight"], w[b + ".norm1.bias"], M=M, C_=c)
                em.gemm(ln, w[b + ".attn1.qkv"], qkv, M=M)              # Q | K | V in one launch
                ar.release(ln)
            a = ar.alloc((M, c))
            em.attention(qkv.data_ptr(), qkv.data_ptr() + c * 2, qkv.data_ptr() + 2 * c * 2, a, B=B, H=heads, Sq=S,
                         Skv=S, valid=S, ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c)
            ar.release(qkv)
            em.gemm(a, w[b + ".attn1.to_out.0.weight"], h, M=M, bias=w[b + ".attn1.to_out.0.bias"], residual=h)
            ar.release(a)
            # --- cross attention (K / V^T of the text context come from the conditioning program) ---
            q = ar.alloc((M, c))
            if fuse:
                em.gemm(h, w[b + ".attn2.to_q_ln.weight"], q, M=M, bias=w[b + ".attn2.to_q_ln.bias"],
                        ln=(w[b + ".attn2.to_q_ln.colsum"], 1e-5))
            else:
                ln = ar.alloc((M, c))
                em.layernorm(h, ln, w[b + ".norm2.weight"], w[b + ".norm2.bias"], M=M, C_=c)
                em.gemm(ln, w[b + ".attn2.to_q.weight"], q, M=M)
                ar.release(ln)
            off, _ = s.net.ctx_slices[b]
            a = ar.alloc((M, c))
            em.attention(q.data_ptr(), s.ctx_kv.data_ptr() + off * 2,
                         s.ctx_kv.data_ptr() + (s.net.n_ctx + off) * 2, a, B=B, H=heads, Sq=S, Skv=CTX_PAD,
                         valid=CTX_TOKENS, ldq=c, ldk=2 * s.net.n_ctx, ldv=2 * s.net.n_ctx, ldo=c)
            ar.release(q)
            em.gemm(a, w[b + ".attn2.to_out.0.weight"], h, M=M, bias=w[b + ".attn2.to_out.0.bias"], residual=h)
            ar.release(a)
            # --- GEGLU feed-forward ---
            ff = ar.alloc((M, 4 * c))
            if fuse:
                em.gemm(h, w[b + ".ff.net.0.proj_ln.weight"], ff, M=M, bias=w[b + ".ff.net.0.proj_ln.bias"],
                        flags=lib.GEMM_GEGLU, ln=(w[b + ".ff.net.0.proj_ln.colsum"], 1e-5))
            else:
                ln = ar.alloc((M, c))
                em.layernorm(h, ln, w[b + ".norm3.weight"], w[b + ".norm3.bias"], M=M, C_=c)
                em.gemm(ln, w[b + ".ff.net.0.proj.weight"], ff, M=M, bias=w[b + ".ff.net.0.proj.bias"],
                        flags=lib.GEMM_GEGLU)
                ar.release(ln)
            em.gemm(ff, w[b + ".ff.net.2.weight"], h, M=M, bias=w[b + ".ff.net.2.bias"], residual=h)
            ar.release(ff)
        out = ar.alloc((B, H, W, c))
        em.gemm(h, w[p + ".proj_out.weight"], out, M=M, bias=w[p + ".proj_out.bias"], residual=x)
        ar.release(h)
        return out

    # ---- conditioning program: everything that depends on (text context, pooled, time ids) only
    def _emit_cond(self, s: _Side):
        """``aug`` and ``ctx_kv`` of one network (the ControlNet has embedding MLPs and cross-attention blocks of its own)."""
        cfg, em, w, ar, B = self.net.cfg, self.em, s.net.w, self.arena, self.B
        add_in = ar.alloc((B, cfg.add_in_dim))
        em.copy_cols(self.text_embeds, add_in, rows=B, cols=cfg.pooled_dim, ld_src=cfg.pooled_dim,
                     ld_dst=cfg.add_in_dim, dst_off=0)
        api.lb_sinusoid_f16(self.time_ids.data_ptr(), B, 6, 6, cfg.add_time_dim, add_in.data_ptr(), cfg.add_in_dim,
                            cfg.pooled_dim, _stream())
        a1 = ar.alloc((B, cfg.time_embed_dim))
        em.gemm(add_in, w["add_embedding.linear_1.weight"], a1, M=B, bias=w["add_embedding.linear_1.bias"],
                flags=lib.GEMM_SILU)
        em.gemm(a1, w["add_embedding.linear_2.weight"], s.aug, M=B, bias=w["add_embedding.linear_2.bias"])
        ar.release(add_in)
        ar.release(a1)
        self._mark(s.prefix + "aug", "aug", s.aug, "text_embeds", "time_ids")
        if s.ctx_kv is None:        # (a ControlNet without any cross-attention block)
            return
        ctx2d = self.ctx.view(B * CTX_PAD, cfg.cross_dim)
        em.gemm(ctx2d, w["ctx_kv.weight"], s.ctx_kv, M=B * CTX_PAD)
        self._mark(s.prefix + "ctx_kv", "ctx_kv", s.ctx_kv, "ctx")

    # ---- step program: depends on the latent and the timestep
    def _emit_encoder(self, s: _Side, residual: Optional[torch.Tensor] = None):
        """The encoder half of network ``s`` on ``x_in`` - time embedding, conv_in (+ ``residual``), the down blocks, the mid block -
        shared by the UNet and a ControlNet.  Returns (skips = [(map, channels, unit)] in ``skip_channels()`` order, all still
        allocated; the mid block's output; its unit; the deepest level's height and width)."""
        self.side = s
        try:
            return self._emit_encoder_of(s, residual)
        finally:
            self.side = self._unet_side

    def _emit_encoder_of(self, s: _Side, residual):
        net, cfg, em, w, ar, B, px = s.net, s.net.cfg, self.em, s.net.w, self.arena, self.B, s.prefix
        ch, T = cfg.block_channels, cfg.time_embed_dim
        # time embedding: silu(temb + aug) feeds every resnet's projection -> one fused GEMM
        tsin = ar.alloc((B, ch[0]))
        api.lb_sinusoid_f16(self.tvals.data_ptr(), B, 1, 1, ch[0], tsin.data_ptr(), ch[0], 0, _stream())
        if s.timestep_cond is not None:      # tsum = timestep_cond . Wc^T + tsin (diffusers: sample + cond_proj(condition))
            tsum = ar.alloc((B, ch[0]))
            em.gemm(s.timestep_cond, w["time_embedding.cond_proj.weight"], tsum, M=B, residual=tsin)
            ar.release(tsin)
            tsin = tsum
        t1 = ar.alloc((B, T))
        em.gemm(tsin, w["time_embedding.linear_1.weight"], t1, M=B, bias=w["time_embedding.linear_1.bias"],
                flags=lib.GEMM_SILU)
        emb = ar.alloc((B, T))
        em.gemm(t1, w["time_embedding.linear_2.weight"], emb, M=B, bias=w["time_embedding.linear_2.bias"],
                residual=s.aug, flags=lib.GEMM_SILU)
        s.temb_all = ar.alloc((B, net.n_temb))
        em.gemm(emb, w["temb_proj.weight"], s.temb_all, M=B, bias=w["temb_proj.bias"])
        ar.release(tsin)
        ar.release(t1)
        ar.release(emb)
        self.persistent.append(s.temb_all)
        temb = self._mark(px + "temb_all", "temb_all", s.temb_all, "tvals", px + "aug", *(("timestep_cond",) if s.timestep_cond is not None else ()))
        ctx_kv = px + "ctx_kv"
        # input: NCHW latent -> NHWC (channels padded to 8)
        cin_p = pad_to(cfg.in_channels, 8)
        x8 = ar.alloc((B, self.H, self.W, cin_p))
        api.lb_nchw_to_nhwc_f16(self.x_in.data_ptr(), x8.data_ptr(), B, cfg.in_channels, self.H * self.W, cin_p, 1.0, _stream())
        h, _, _ = self._conv(x8, "conv_in", B, self.H, self.W, cfg.in_channels, ch[0], residual=residual)
        ar.release(x8)
        at = self._mark(px + "conv_in", "conv_in", h, "x_in", *(("hint_emb",) if residual is not None else ()))     # ``at``: the unit whose output h is
        if not px:
            self.tap_names["conv_in"] = at
        skips = [(h, ch[0], at)]
        sh, sw, prev = self.H, self.W, ch[0]                    # the current level's map is sh x sw
        for bi, c in enumerate(ch):
            for li in range(cfg.layers_per_block):
                p = f"down_blocks.{bi}.resnets.{li}"
                nxt = self._resnet(h, p, B, sh, sw, prev, c)
                if not any(h is k for k, _, _ in skips):
                    ar.release(h)
                h = nxt
                at = self._mark(px + p, "resnet", h, at, temb)
                if cfg.transformer_depth[bi]:
                    p = f"down_blocks.{bi}.attentions.{li}"
                    nxt = self._transformer(h, p, B, sh, sw, c, cfg.transformer_depth[bi])
                    ar.release(h)
                    h = nxt
                    at = self._mark(px + p, "transformer", h, at, ctx_kv)
                skips.append((h, c, at))
                prev = c
            if bi < len(ch) - 1:
                p = f"down_blocks.{bi}.downsamplers.0.conv"
                h, sh, sw = self._conv(h, p, B, sh, sw, c, c, stride=2)
                at = self._mark(px + p, "downsample", h, at)
                skips.append((h, c, at))
            if not px:
                self.tap_names[f"down{bi}"] = at
        c = ch[-1]
        nxt = self._resnet(h, "mid_block.resnets.0", B, sh, sw, c, c)     # h is a skip: not released
        h = nxt
        at = self._mark(px + "mid_block.resnets.0", "resnet", h, at, temb)
        nxt = self._transformer(h, "mid_block.attentions.0", B, sh, sw, c, cfg.transformer_depth[-1])
        ar.release(h)
        h = nxt
        at = self._mark(px + "mid_block.attentions.0", "transformer", h, at, ctx_kv)
        nxt = self._resnet(h, "mid_block.resnets.1", B, sh, sw, c, c)
        ar.release(h)
        h = nxt
        at = self._mark(px + "mid_block.resnets.1", "resnet", h, at, temb)
        if not px:
            self.tap_names["mid"] = at
        return skips, h, at, sh, sw

    def _emit_control_adds(self, c_skips, c_mid, c_mid_at, skips, h, at):
        """One GEMM per residual: zero conv (1x1, weights and bias pre-scaled by the conditioning scale) of the ControlNet's hidden map,
        added in the epilogue to the UNet's skip copy IN PLACE - every down-path reader of that copy has been emitted; the mid
        residual goes into the mid block's output.  Returns (the skips under their new units, the mid unit)."""
        em, cw, ar, B = self.em, self.control.w, self.arena, self.B
        out = []
        for k, ((ck, cc, c_at), (sk, sc, s_at)) in enumerate(zip(c_skips, skips)):
            assert cc == sc and ck.shape == sk.shape
            M = sk.numel() // sc
            em.gemm(ck, cw[f"controlnet_down_blocks.{k}.weight"], sk, M=M, bias=cw[f"controlnet_down_blocks.{k}.bias"], residual=sk)
            ar.release(ck)
            out.append((sk, sc, self._mark(f"control.zero.{k}", "zero", sk, c_at, s_at)))
        c = self.net.cfg.block_channels[-1]
        em.gemm(c_mid, cw["controlnet_mid_block.weight"], h, M=h.numel() // c, bias=cw["controlnet_mid_block.bias"], residual=h)
        ar.release(c_mid)
        return out, self._mark("control.zero.mid", "zero", h, c_mid_at, at)

    def _emit_step(self):
        net, cfg, em, w, ar, B = self.net, self.net.cfg, self.em, self.net.w, self.arena, self.B
        ch = cfg.block_channels
        if self.control is not None:       # the ControlNet first: its ten hidden maps wait for the UNet's skips
            c_skips, c_mid, c_mid_at, _, _ = self._emit_encoder(self._control_side, residual=self.hint_emb)
        skips, h, at, sh, sw = self._emit_encoder(self._unet_side)
        self.temb_all = self._unet_side.temb_all
        self.skip_maps = [k for k, _, _ in skips]      # (valid between the mid block and the up path: ``run_with_residuals``)
        self.mid_map, self.op_mid_end = h, self.prog_step.num_ops
        if self.control is not None:
            skips, at = self._emit_control_adds(c_skips, c_mid, c_mid_at, skips, h, at)
        depths = list(reversed(cfg.transformer_depth))
        for ui, (c, cins) in enumerate(net.up_plan()):
            for li, (hid, sc) in enumerate(cins):
                skip, sch, skip_at = skips.pop()
                assert sch == sc
                M = B * sh * sw
                cat = ar.alloc((B, sh, sw, hid + sc))
                em.copy_cols(h, cat, rows=M, cols=hid, ld_src=hid, ld_dst=hid + sc, dst_off=0)
                em.copy_cols(skip, cat, rows=M, cols=sc, ld_src=sc, ld_dst=hid + sc, dst_off=hid)
                ar.release(h)
                ar.release(skip)
                p = f"up_blocks.{ui}.resnets.{li}"
                h = self._resnet(cat, p, B, sh, sw, hid + sc, c)
                ar.release(cat)
                at = self._mark(p, "resnet", h, at, skip_at, "temb_all")      # (reads the concatenation [h | skip])
                if depths[ui]:
                    p = f"up_blocks.{ui}.attentions.{li}"
                    nxt = self._transformer(h, p, B, sh, sw, c, depths[ui])
                    ar.release(h)
                    h = nxt
                    at = self._mark(p, "transformer", h, at, "ctx_kv")
            if ui < len(ch) - 1:
                p = f"up_blocks.{ui}.upsamplers.0.conv"
                nxt, sh, sw = self._upconv(h, p, B, sh, sw, c)
                ar.release(h)
                h = nxt
                at = self._mark(p, "upsample", h, at)
            self.tap_names[f"up{ui}"] = at
        n = ar.alloc((B, sh, sw, ch[0]))
        em.groupnorm(h, n, w["conv_norm_out.weight"], w["conv_norm_out.bias"], B=B, HW=sh * sw, C_=ch[0],
                     eps=1e-5, silu=True, groups=cfg.norm_groups)
        ar.release(h)
        o, _, _ = self._conv(n, "conv_out", B, sh, sw, ch[0], cfg.out_channels)
        ar.release(n)
        api.lb_nhwc_to_nchw_f16(o.data_ptr(), self.eps.data_ptr(), B, cfg.out_channels, self.H * self.W,
                                pad_to(cfg.out_channels, 4), _stream())
        ar.release(o)
        self._mark("eps", "out", self.eps, at)

    # ---- execution ------------------------------------------------------------------------
    def set_conditioning(self, ctx: torch.Tensor, text_embeds: torch.Tensor, time_ids: torch.Tensor,
                         timestep_cond: Optional[torch.Tensor] = None):
        """ctx [B,77,X] fp16, text_embeds [B,P] fp16, time_ids [B,6] (any float dtype); ``timestep_cond`` [B, time_cond_proj_dim]
        (or one row for all samples): the guidance-scale embedding - required when the config has that dimension, refused when
        it has not (the step program reads it; the conditioning program does not depend on it)."""
        if self.timestep_cond is None:
            if timestep_cond is not None:
                raise ValueError("UNetProgram.set_conditioning: timestep_cond given, but the UNet config has no time_cond_proj_dim")
        else:
            if timestep_cond is None:
                raise ValueError("UNetProgram.set_conditioning: this UNet is guidance-embedded (time_cond_proj_dim = "
                                 f"{self.net.cfg.time_cond_proj_dim}): timestep_cond is required")
            tc = timestep_cond.reshape(-1, timestep_cond.shape[-1])
            if tc.shape[-1] != self.timestep_cond.shape[1] or tc.shape[0] not in (1, self.B):
                raise ValueError(f"UNetProgram.set_conditioning: timestep_cond of shape {tuple(timestep_cond.shape)}, "
                                 f"expected [{self.B} or 1, {self.timestep_cond.shape[1]}]")
            self.timestep_cond.copy_(tc.expand(self.B, -1))
        self.ctx[:, :CTX_TOKENS].copy_(ctx)
        self.text_embeds.copy_(text_embeds)
        self.time_ids.copy_(time_ids.to(F32))
        self.prog_cond.launch()

    def forward(self, x_in: torch.Tensor, tvals: torch.Tensor) -> torch.Tensor:
        """x_in [B,4,H,W] fp16 (already scaled), tvals [B] -> eps [B,4,H,W] fp16 (program-owned buffer)."""
        self.x_in.copy_(x_in)
        self.tvals.copy_(tvals.reshape(-1, 1).to(F32))
        self.prog_step.launch()
        return self.eps

    def forward_with_residuals(self, x_in: torch.Tensor, tvals: torch.Tensor, down: Sequence[torch.Tensor], mid: Optional[torch.Tensor]) -> torch.Tensor:
        """``forward`` with residuals GIVEN as tensors (diffusers' ``down_block_additional_residuals`` / ``mid_block_additional_residual``,
        NHWC fp16 here): the step program runs up to the end of the mid block, the residuals are added to the skip copies and to the
        mid block's output, the up path runs.  The compatibility path of the ``pipe.unet`` facade - eager between two halves of the
        program, one more fp16 rounding than the fused form; the native loops use a program built with ``control=``."""
        if self.control is not None:
            raise ValueError("UNetProgram.forward_with_residuals: this program adds its own ControlNet's residuals already")
        if len(down) != len(self.skip_maps):
            raise ValueError(f"UNetProgram.forward_with_residuals: {len(down)} residuals for {len(self.skip_maps)} skips")
        self.x_in.copy_(x_in)
        self.tvals.copy_(tvals.reshape(-1, 1).to(F32))
        self.prog_step.run_range(0, self.op_mid_end)
        for skip, res in zip(self.skip_maps, down):
            skip.add_(res.to(F16).reshape(skip.shape))
        if mid is not None:
            self.mid_map.add_(mid.to(F16).reshape(self.mid_map.shape))
        self.prog_step.run_range(self.op_mid_end, self.prog_step.num_ops)
        return self.eps
