"""Device-side plumbing for the native model programs.

* ``Arena``   — size-class pool over torch device tensors.  A recorded program replays in stream
  order, so a buffer can be handed to the next op as soon as its last reader has been emitted;
  reuse keeps the working set of a UNet forward inside L2 / Infinity Cache instead of walking
  through fresh HBM for every op.
* ``Program`` — owner of a C++ launch program (``lb_program_*``): ``with prog.record(): ...`` runs
  the emitting Python ONCE; afterwards ``prog.launch()`` replays ~1000 kernel launches from C++
  (optionally as one hipGraph) with a single ctypes call.
* ``Emitter`` — thin typed helpers that fill the C structs and call the launchers (in record mode
  these calls are captured, in eager mode they launch immediately — same code path).
* ``RecordedProgram`` — what every model's program object is: arena + emitter, the recording context, the unit marks
  (``Mark``) and their replay (``capture_marks``), graph instantiation.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from ..hip import lib
from ..hip.lib import api, LbGemmParams, LbAttnParams
from .geometry import latent_hw, use_ragged_halo

F16, F32 = torch.float16, torch.float32


class Arena:
    """``journal=True``: every ``alloc`` / ``release`` appends ``(event, buffer id, program name, op index)`` to ``self.journal`` -
    the buffer id is the raw buffer's index in ``self.all``, the last two come from ``self.clock`` (set by the program that is
    recording: ``Arena.clocked``; ``(None, -1)`` outside a recording).  The journal only listens: which buffer an ``alloc`` hands
    out, and so every recorded pointer, is the same with it on or off."""

    def __init__(self, device, journal: bool = False):
        self.device = device
        self.free: Dict[int, List[torch.Tensor]] = {}
        self.all: List[torch.Tensor] = []
        self.bytes_allocated = 0
        self.journal: Optional[List[Tuple[str, int, Optional[str], int]]] = [] if journal else None
        self.clock = None                   # () -> (program name, number of ops recorded so far)
        self._ids: Dict[int, int] = {}      # id(raw) -> index in self.all (journal only)

    @contextlib.contextmanager
    def clocked(self, prog: "Program"):
        """While ``prog`` records: journal entries carry its name and the index of the op that will be recorded next."""
        self.clock = lambda: (prog.name, prog.num_ops)
        try:
            yield
        finally:
            self.clock = None

    def _log(self, event: str, raw: torch.Tensor) -> None:
        name, op = self.clock() if self.clock is not None else (None, -1)
        self.journal.append((event, self._ids[id(raw)], name, op))

    @staticmethod
    def _cls(nbytes: int) -> int:
        return max(512, (nbytes + 511) // 512 * 512)

    def alloc(self, shape, dtype=F16) -> torch.Tensor:
        n = 1
        for s in shape:
            n *= int(s)
        esz = torch.empty((), dtype=dtype).element_size()
        cls = self._cls(n * esz)
        pool = self.free.get(cls)
        if pool:
            raw = pool.pop()
        else:
            raw = torch.empty(cls, dtype=torch.uint8, device=self.device)
            self.all.append(raw)
            self.bytes_allocated += cls
            if self.journal is not None:
                self._ids[id(raw)] = len(self.all) - 1
        if self.journal is not None:
            self._log("alloc", raw)
        t = raw[: n * esz].view(dtype).view(*shape)
        t._lb_raw = raw
        return t

    def release(self, t: Optional[torch.Tensor]) -> None:
        if t is None:
            return
        st = getattr(t, "_lb_chstats", None)     # statistics buffer of a conv output nobody normalised: goes back with it
        if st is not None:
            t._lb_chstats = None
            self.release(st[0])
        raw = getattr(t, "_lb_raw", None)
        if raw is None:
            return
        t._lb_raw = None
        if self.journal is not None:
            self._log("release", raw)
        self.free.setdefault(raw.numel(), []).append(raw)


class Program:
    def __init__(self, name: str = "program"):
        self.name = name
        self.handle = api.lb_program_create()
        self.keep: List[object] = []       # tensors / arenas the recorded pointers refer to
        self.graph_ready = False

    def __del__(self):
        try:
            if self.handle:
                api.lb_program_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    @contextlib.contextmanager
    def record(self):
        api.lb_program_begin_record(self.handle)
        self.graph_ready = False           # (the library dropped the graph: launch() is eager until the next instantiate())
        try:
            yield self
        finally:
            api.lb_program_end_record(self.handle)

    @property
    def num_ops(self) -> int:
        return api.lb_program_num_ops(self.handle)

    def op_names(self) -> List[str]:
        return [api.lb_program_op_name(self.handle, i).decode() for i in range(self.num_ops)]

    def run(self, stream: Optional[int] = None) -> None:
        api.lb_program_run(self.handle, stream if stream is not None else _stream())

    def run_range(self, begin: int, end: int, stream: Optional[int] = None) -> None:
        api.lb_program_run_range(self.handle, begin, end, stream if stream is not None else _stream())

    def instantiate(self) -> None:
        api.lb_program_instantiate(self.handle)
        self.graph_ready = True

    def launch(self, stream: Optional[int] = None) -> None:
        api.lb_program_launch(self.handle, stream if stream is not None else _stream())

    def time_ops(self, stream: Optional[int] = None) -> List[float]:
        """Eager replay with hipEvents between ops -> per-op milliseconds (synchronises)."""
        n = self.num_ops
        buf = (C.c_float * n)()
        api.lb_program_time_ops(self.handle, stream if stream is not None else _stream(), buf)
        return list(buf)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class GnOperand:
    """A GroupNorm whose consumer is one 3x3 conv (``Emitter.gn_operand``): the raw tensor, the GroupNorm's arguments, and what was
    emitted for it - the affine table of a conv that applies the GroupNorm itself, or the scratch buffer a GroupNorm launch filled."""

    def __init__(self, x: torch.Tensor, args: dict):
        self.x, self.args = x, args
        self.table: Optional[torch.Tensor] = None
        self.scratch: Optional[torch.Tensor] = None
        self.conv: Optional[tuple] = None       # geometry of the conv the fold was planned for (``table`` set)


def _conv_key(p: LbGemmParams) -> tuple:
    return (p.M, p.N, p.K, p.Hin, p.Win, p.Cin, p.ldx)


class Emitter:
    """Helpers shared by the UNet / VAE / LPIPS program builders.  All tensors are views into an
    ``Arena`` (activations) or packed weights; nothing here synchronises or allocates through
    torch while a program is being recorded except via the arena."""

    def __init__(self, arena: Arena):
        self.arena = arena
        self.device = arena.device
        # one split-K slab region and one GroupNorm workspace shared by all ops of a program
        self.ws_gemm: Optional[torch.Tensor] = None
        self.ws_gn: Optional[torch.Tensor] = None
        # algorithmic work of every emitted contraction, in emission order (bench.py roofline)
        self.gemm_log: List[dict] = []
        self.attn_log: List[dict] = []
        self.norm_log: List[dict] = []      # GroupNorm / LayerNorm launches: algorithmic HBM bytes
        self._retired: List[torch.Tensor] = []
        self.zero_page = torch.zeros(64, dtype=torch.uint8, device=self.device)
        # set by the builder of a NON-SQUARE program (and its pipe's ``ragged_halo`` switch): 3x3 convs whose level does not divide
        # into halo tiles ask for the ragged-tile form (LB_GEMM_HALO_RAGGED) where ``geometry.use_ragged_halo`` says so.  False
        # (every square program): no flag - the recorded ops are those of ever.
        self.ragged_halo = False
        # 3x3 halo-tile convs whose tiles fill the last round of CUs badly run the K-split form (LB_GEMM_HALO_KSPLIT) where the
        # library's own plan says so (the K-split part of lb_conv_plan's record); False: no flag.  One workspace per emitter: a fixed
        # counter area (zeroed once: every launch leaves its counters zero) in front of the slabs all launches share.
        self.halo_ksplit = True
        self.ws_ksplit: Optional[torch.Tensor] = None
        # a GroupNorm (+ SiLU) that reads its statistics from the producing conv and feeds one 3x3 conv is folded into that conv
        # (LB_GEMM_GN_A: ``gemm(..., gn=...)``) where the library's own plan says so (the GN_A part of lb_conv_plan's record); False:
        # the GroupNorm launch and its output buffer as ever
        self.gn_a = True
        # wrap-around padding of every "same" conv this emitter launches (``ConvGeom.wrap`` bits: 1 = the columns wrap, 2 = the rows,
        # 3 = both): set by ``RecordedProgram(..., wrap=...)`` for the programs of a tileable render.  Applied in ONE place, ``_geom``,
        # which ``gemm``, ``gn_operand``, ``upconv`` and the probes go through: 3x3 / pad 1 convs (stride 1 and 2, ``ups``) and the
        # sub-pixel upsampler forms get the bits, every other conv (1x1, pad 0, the encoder's ``down3x3``, LPIPS' 11x11 / 5x5) and
        # every plain GEMM is left alone.  0 (default): the geometries, blocks and ops of ever.
        self.wrap = 0

    def _geom(self, conv: Optional[lib.ConvGeom]) -> Optional[lib.ConvGeom]:
        """``conv`` as this emitter launches it: a "same" conv - 3x3 / pad 1, or a sub-pixel form - gets the emitter's ``wrap``;
        every other conv is left alone.  A same conv that cannot take the bits (stride 2 over an odd side of a wrapped axis) raises
        ``ValueError``: a program that calls itself tileable never records a zero-padded 3x3 conv."""
        if not self.wrap or conv is None or conv.wrap:
            return conv
        if conv.parity is None and (conv.KH, conv.KW, conv.pad) != (3, 3, 1):
            return conv
        return conv.with_wrap(self.wrap)

    def _conv_plan(self, p: LbGemmParams) -> lib.LbConvPlan:
        """The one planning step of a conv: ONE lb_conv_plan call says where lb_gemm_f16 takes ``p`` and in which form.  Sets the
        emitter's two opt-in bits on ``p`` - LB_GEMM_HALO_RAGGED where ``geometry.use_ragged_halo`` says so, LB_GEMM_HALO_KSPLIT (asked
        as a hint: it never changes the route) where the conv goes to the halo-tile kernel and the library's plan splits it - and
        returns the record of ``p`` as flagged.  Allocates nothing: probes (``halo_stat_rows``, ``gn_operand``) plan with it too.
        Convs of at most 16 output channels are never flagged ragged: the narrow-N kernel's domain, 128-column halo blocks would idle."""
        if self.halo_ksplit:
            p.flags |= lib.GEMM_HALO_KSPLIT
        plan = lib.conv_plan(p)
        if self.ragged_halo and p.N > 16 and use_ragged_halo(True, plan.halo_kind, plan.ragged_kind, p.Hin, p.Win, plan.ragged_tile_w):
            p.flags |= lib.GEMM_HALO_RAGGED
            plan = lib.conv_plan(p)          # (non-square programs only: the record of the launch as it is now flagged)
        splits = plan.route == lib.ROUTE_HALO3 and plan.ksplit_split
        if self.halo_ksplit and not (splits and plan.ksplit_counter_bytes <= self._KSPLIT_COUNTER_BYTES):
            p.flags &= ~lib.GEMM_HALO_KSPLIT
            if splits:                       # (more than 262,144 tiles: past the counter area, launched - and planned - unflagged)
                plan = lib.conv_plan(p)
        return plan

    # -- workspaces -------------------------------------------------------------------------
    def _gemm_ws(self, M: int, N: int) -> Optional[torch.Tensor]:
        """Split-K slab region.  The launcher only splits grids of at most 640 64x64 tiles (<= 256 blocks of
        the tile it then picks), so larger problems get no workspace (and cannot split).  A grown workspace never replaces the
        old one in already-recorded ops: superseded buffers are kept alive."""
        if ((M + 63) // 64) * ((N + 63) // 64) > 640:
            return None
        need = api.lb_gemm_workspace_bytes(M, N) // 4
        if self.ws_gemm is None or self.ws_gemm.numel() < need:
            if self.ws_gemm is not None:
                self._retired.append(self.ws_gemm)
            self.ws_gemm = torch.empty(max(need, 1 << 22), dtype=F32, device=self.device)
        return self.ws_gemm

    _KSPLIT_COUNTER_BYTES = 1 << 20

    def _halo_ksplit(self, p: LbGemmParams, plan: lib.LbConvPlan) -> bool:
        """Apply the K-split part of ``plan`` to the 3x3 conv ``p``: where ``_conv_plan`` left it flagged, point ``partial`` at the
        workspace, sized by the library's own numbers.  The launch's counters end where the shared slab area begins, so no launch's
        slabs ever overlap another launch's counters."""
        if not (self.halo_ksplit and p.flags & lib.GEMM_HALO_KSPLIT and plan.ksplit_split):
            return False
        total = self._KSPLIT_COUNTER_BYTES + plan.ksplit_slab_bytes
        if self.ws_ksplit is None or self.ws_ksplit.numel() < total:
            if self.ws_ksplit is not None:      # (recorded ops keep pointing into the old buffer)
                self._retired.append(self.ws_ksplit)
            self.ws_ksplit = torch.zeros(total, dtype=torch.uint8, device=self.device)
        p.partial = self.ws_ksplit.data_ptr() + self._KSPLIT_COUNTER_BYTES - plan.ksplit_counter_bytes
        return True

    def _gn_ws(self, B: int, groups: int) -> torch.Tensor:
        need = api.lb_groupnorm_workspace_bytes(B, groups) // 8
        if self.ws_gn is None or self.ws_gn.numel() < need:
            if self.ws_gn is not None:
                self._retired.append(self.ws_gn)
            self.ws_gn = torch.empty(need, dtype=torch.float64, device=self.device)
        return self.ws_gn

    # -- dense ------------------------------------------------------------------------------
    def gemm(self, A: torch.Tensor, W: torch.Tensor, out: torch.Tensor, *, M: int, bias=None,
             residual=None, rowvec=None, rows_per_batch: int = 0, flags: int = 0, alpha: float = 1.0,
             lda: Optional[int] = None, ldc: Optional[int] = None, ldr: Optional[int] = None,
             ld_rowvec: Optional[int] = None, conv: Optional[lib.ConvGeom] = None, splitk: bool = True,
             ln: Optional[Tuple[torch.Tensor, float]] = None, ch_stats: Optional[torch.Tensor] = None,
             gn: Optional["GnOperand"] = None):
        """``ln`` = (colsum [N] fp32, eps): A is consumed through a LayerNorm folded into this GEMM (LB_GEMM_LN_A; W and
        bias must already carry gamma / beta, see ``NativeUNet._ln_linear``); row statistics from the A fragments in the K loop.

        ``gn`` = what ``gn_operand`` returned for this very conv (A = the raw tensor): the conv consumes GroupNorm(A), either through
        the affine table (LB_GEMM_GN_A) or from the scratch buffer the GroupNorm launch filled; both go back to the arena here."""
        fold = gn is not None and gn.table is not None      # (the fold was decided by gn_operand; a flagged conv is never split along K)
        conv = self._geom(conv)
        p = self._gemm_params(A if gn is None or fold else gn.scratch, W, out, M=M, bias=bias, residual=residual, rowvec=rowvec,
                              rows_per_batch=rows_per_batch, flags=flags, alpha=alpha, lda=lda, ldc=ldc, ldr=ldr, ld_rowvec=ld_rowvec,
                              conv=conv, ln=ln, ch_stats=ch_stats, gn=(gn.table, gn.args["silu"]) if fold else None)
        N, K = W.shape
        n_out = N // 2 if flags & lib.GEMM_GEGLU else N
        if splitk and not (flags & lib.GEMM_GEGLU) and ln is None:
            p.partial = _p(self._gemm_ws(M, N))
        if fold and gn.conv != _conv_key(p):
            raise RuntimeError("Emitter.gemm: the conv is not the one gn_operand planned the GroupNorm fold for")
        if conv is not None:
            self._halo_ksplit(p, self._conv_plan(p))
        api.lb_gemm_f16(C.byref(p), _stream())
        if gn is not None:
            self.arena.release(gn.scratch)
            self.arena.release(gn.table)
            gn.scratch = gn.table = None
        mult = 4.0 if p.scatter == 2 else 1.0          # (four parities: four times the rows, weights and outputs)
        self.gemm_log.append({"M": M, "N": N, "K": K, "flops": mult * 2.0 * M * N * K, "conv": conv is not None,
                              "bytes": mult * 2.0 * (N * K + M * n_out) + (2.0 * M * K if conv is None else 0.0)})
        return out

    def gn_operand(self, x: torch.Tensor, W: torch.Tensor, *, M: int, conv: lib.ConvGeom, flags: int = 0, has_residual: bool = False,
                   **gn) -> "GnOperand":
        """Emit the GroupNorm side of "3x3 conv of GroupNorm(x)" NOW and return the operand for the conv's ``gemm(x, ..., gn=...)``.
        ``gn`` = the keyword arguments of ``groupnorm`` plus gamma / beta.  Where the library's plan fuses (the GN_A part of the conv's
        record: route, whole tiles, unsplit, measured policy) the emitted op is the table kernel
        (lb_groupnorm_affine_from_stats) and the conv will carry LB_GEMM_GN_A and read the raw x: no normalised buffer, no
        lb_groupnorm_from_stats.  Everywhere else: the GroupNorm launch into a scratch buffer, exactly as ever."""
        op = GnOperand(x, dict(gn))
        conv = self._geom(conv)
        p = self._gemm_params(x, W, x, M=M, residual=x if has_residual else None, flags=flags, conv=conv)     # (pointers: only their nullness counts)
        # only with producer statistics and an fp16 stream tensor whose channels are the conv's (no padding in between)
        able = self.gn_a and gn.get("ch_stats") is not None and x.dtype == F16 and p.Cin == int(gn["C_"]) and p.ldx == p.Cin and \
            gn.get("ldx") in (None, p.Cin)
        if able and self._conv_plan(p).gn_a_fuse:
            op.conv = _conv_key(p)
            B_, C_, st = int(gn["B"]), int(gn["C_"]), gn["ch_stats"]
            op.table = self.arena.alloc((B_, C_, 2), F32)
            api.lb_groupnorm_affine_from_stats(st[0].data_ptr(), gn["gamma"].data_ptr(), gn["beta"].data_ptr(), op.table.data_ptr(),
                                               B_, int(gn["HW"]), C_, int(gn.get("groups", 32)), float(gn["eps"]), int(st[1]),
                                               _stream())
        else:
            op.scratch = self.arena.alloc(tuple(x.shape[:-1]) + (int(gn["C_"]),))
            self.groupnorm(x, op.scratch, gn["gamma"], gn["beta"], **{k: v for k, v in gn.items() if k not in ("gamma", "beta")})
        return op

    def _gemm_params(self, A, W, out, *, M, bias=None, residual=None, rowvec=None, rows_per_batch=0, flags=0, alpha=1.0, lda=None,
                     ldc=None, ldr=None, ld_rowvec=None, conv=None, ln=None, ch_stats=None, gn=None) -> LbGemmParams:
        """The parameter block ``gemm`` launches, before anything is planned for it: no workspace, none of the emitter's opt-in bits.
        Leading dimensions default to dense; ``gn`` = (affine table, silu): LB_GEMM_GN_A."""
        N, K = W.shape
        n_out = N // 2 if flags & lib.GEMM_GEGLU else N
        if ch_stats is not None:       # halo-tile convs only (see halo_stat_rows): GroupNorm statistics of the stored output
            assert conv is not None and ch_stats.dtype == F32
        return lib.gemm_params(
            A=A.data_ptr(), W=W.data_ptr(), C=out.data_ptr(), M=M, N=N, K=K, ldw=W.stride(0), conv=conv,
            lda=0 if conv is not None else lda if lda is not None else K,
            ldc=ldc if ldc is not None else (M if flags & lib.GEMM_TRANS_OUT else n_out), bias=_p(bias), residual=_p(residual),
            ldr=ldr if ldr is not None else n_out, rowvec=_p(rowvec), ld_rowvec=ld_rowvec if ld_rowvec is not None else N,
            rows_per_batch=rows_per_batch, alpha=alpha, flags=flags, zero_page=self.zero_page.data_ptr(),
            ln=None if ln is None else (ln[0].data_ptr(), ln[1]),
            ch_stats=None if ch_stats is None else (ch_stats.data_ptr(), ch_stats.shape[1]),      # [N][B * rows][2]: checked by the launcher
            gn=None if gn is None else (gn[0].data_ptr(), gn[1]))

    def halo_stat_rows(self, B: int, H: int, W: int, cin: int, cout: int, ks: int = 3) -> int:
        """Rows per sample of the LB_GEMM_CH_STATS buffer ([cout][B * rows] float2, channel-major) if a 3x3 conv (ks = 3) or a one-launch
        sub-pixel upsampler conv (ks = 2) of this geometry runs on the halo-tile kernel - whose epilogue can leave the
        GroupNorm statistics of what it stores - else 0 (the consumer then runs the two-pass GroupNorm)."""
        if ks == 2 and not self.upconv_one_launch(B, H, W, cin, cout):
            return 0
        p = lib.conv_probe(B, H, W, cin, cout, ks, zero_page=self.zero_page.data_ptr(), wrap=self.wrap)
        return self._conv_plan(p).stat_rows     # the library's own routing + tile constants, with the bits ``gemm`` will set (0: not a halo launch)

    @staticmethod
    def upconv_one_launch(B: int, H: int, W: int, cin: int, cout: int) -> bool:
        """The halo kernel's sub-pixel form takes this upsampler conv in one launch (else: four implicit-GEMM launches): the library
        says whether it can, the emitter asks for a grid of at least 96 blocks."""
        return lib.conv_plan(lib.conv_probe(B, H, W, cin, cout, 2)).halo_kind == 2 and B * (H * W // 256) * 4 * ((cout + 127) // 128) >= 96

    def upconv(self, x: torch.Tensor, weights: dict, stem: str, out: torch.Tensor, *, B: int, H: int, W: int, c: int, bias,
               flags: int = 0, alpha: float = 1.0, ch_stats: Optional[torch.Tensor] = None):
        """nearest-2x upsample + 3x3 conv (c -> c) of x [B, H, W, c] into out [B, 2H, 2W, c], as sub-pixel 2x2 convs on the low-res
        grid: ONE halo-kernel launch of the four stacked kernels ``weights[stem + ".sub4"]`` where ``upconv_one_launch`` says so, else
        four implicit-GEMM launches of ``weights[stem + ".sub{py}{px}"]``.  ``ch_stats``: what ``halo_stat_rows(..., ks=2)`` sized -
        only the one-launch form leaves statistics."""
        one = self.upconv_one_launch(B, H, W, c, c)
        assert one or ch_stats is None
        forms = [("all", weights[f"{stem}.sub4"][0])] if one else \
            [((py, px), weights[f"{stem}.sub{py}{px}"]) for py in (0, 1) for px in (0, 1)]
        for parity, wt in forms:
            self.gemm(x, wt, out, M=B * H * W, bias=bias, ldc=c, flags=flags, alpha=alpha, ch_stats=ch_stats,
                      conv=lib.ConvGeom.subpixel(H, W, c, parity))
        return out

    def groupnorm(self, x: torch.Tensor, out: torch.Tensor, gamma, beta, *, B: int, HW: int, C_: int,
                  eps: float, silu: bool, groups: int = 32, ldx: Optional[int] = None,
                  ch_stats: Optional[Tuple[torch.Tensor, int]] = None):
        """``ch_stats`` = (buffer, rows per sample) left by the conv that produced ``x`` (LB_GEMM_CH_STATS): one pass over x."""
        if ch_stats is not None:
            api.lb_groupnorm_from_stats(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ch_stats[0].data_ptr(),
                                        self._gn_ws(B, groups).data_ptr(), B, HW, C_, ldx or C_, C_, groups, eps, int(silu),
                                        int(x.dtype == F32), int(ch_stats[1]), _stream())
            self.norm_log.append({"op": "lb_groupnorm_from_stats", "bytes": float(B * HW * C_) * (x.element_size() + 2)})
            return out
        api.lb_groupnorm_nhwc(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                              self._gn_ws(B, groups).data_ptr(), B, HW, C_, ldx or C_, C_, groups, eps,
                              int(silu), int(x.dtype == F32), _stream())
        # algorithmic traffic: the statistics pass reads x, the apply pass reads x and writes fp16 y; the one-launch form (round 6: slab in
        # registers) reads x once
        one = bool(api.lb_groupnorm_plan(HW, C_, groups, int(x.dtype == F32)))
        self.norm_log.append({"op": "lb_groupnorm_nhwc", "bytes": float(B * HW * C_) * ((1 if one else 2) * x.element_size() + 2), "one_launch": one})
        return out

    def layernorm(self, x, out, gamma, beta, *, M: int, C_: int, eps: float = 1e-5):
        api.lb_layernorm_f16(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), M, C_, C_, C_,
                             eps, _stream())
        self.norm_log.append({"op": "lb_layernorm_f16", "bytes": float(M * C_) * 4})
        return out

    def attention(self, q_ptr: int, k_ptr: int, v_ptr: int, out: torch.Tensor, *, B, H, Sq, Skv, valid,
                  ldq, ldk, ldv, ldo, causal: bool = False, head_dim: int = 64):
        """``head_dim`` 64: lb_attn_fwd_d64 (UNet, CLIP towers); 512: lb_attn_fwd_d512 (VAE mid block, no causal form)."""
        assert head_dim in (64, 512) and not (causal and head_dim == 512)
        p = LbAttnParams()
        p.Q, p.K, p.V, p.O = q_ptr, k_ptr, v_ptr, out.data_ptr()
        p.B, p.H, p.Sq, p.Skv, p.Skv_valid = B, H, Sq, Skv, valid
        p.ldq, p.ldk, p.ldv, p.ldo = ldq, ldk, ldv, ldo
        p.scale = float(head_dim) ** -0.5
        p.causal = int(causal)
        p.zero_page = self.zero_page.data_ptr()
        (api.lb_attn_fwd_d512 if head_dim == 512 else api.lb_attn_fwd_d64)(C.byref(p), _stream())
        self.attn_log.append({"flops": 4.0 * B * H * Sq * valid * head_dim, "Sq": Sq, "Skv": Skv, "head_dim": head_dim})
        return out

    def copy_cols(self, src, dst, *, rows, cols, ld_src, ld_dst, dst_off):
        api.lb_copy_cols_f16(src.data_ptr(), dst.data_ptr(), rows, cols, ld_src, ld_dst, dst_off, _stream())

    def copy(self, dst: torch.Tensor, src: torch.Tensor):
        assert dst.numel() * dst.element_size() == src.numel() * src.element_size()
        api.lb_copy_d2d(dst.data_ptr(), src.data_ptr(), src.numel() * src.element_size(), _stream())


class Mark(NamedTuple):
    """End of one emission unit of a recorded program (``RecordedProgram.marks``): the unit's ops are those from the previous mark of
    the same program up to ``op_end`` (exclusive), ``out`` is the view its result is read through - valid right after op
    ``op_end - 1``, the arena may hand the buffer on later - and ``inputs`` names the units (or program inputs) it read."""
    name: str
    kind: str
    program: str
    op_end: int
    out: torch.Tensor
    inputs: Tuple[str, ...]


def capture_marks(progs: Dict[str, Program], marks: List[Mark], convert=None) -> Dict[str, torch.Tensor]:
    """Replay ``progs`` (in order) from mark to mark with ``run_range`` and clone every unit's output right after its last op.
    ``convert(mark, clone)`` may turn the clone into what the caller wants to see."""
    taps: Dict[str, torch.Tensor] = {}
    for pname, prog in progs.items():
        at = 0
        for m in marks:
            if m.program != pname:
                continue
            if m.op_end > at:
                prog.run_range(at, m.op_end)
                at = m.op_end
            t = m.out.clone()
            taps[m.name] = convert(m, t) if convert is not None else t
        if at < prog.num_ops:
            prog.run_range(at, prog.num_ops)
    return taps


class RecordedProgram:
    """Base of a model's program object: the launches of ``net`` for a fixed batch ``B`` (and latent size), recorded once.
    ``L``: latent side or ``(H, W)`` -> ``.H`` / ``.W`` always, ``.L`` for square programs (else None); ``ragged_halo``: a
    non-square program may send 3x3 convs whose level does not divide into halo tiles to the ragged-tile form of the halo kernel
    (``geometry.use_ragged_halo``); a square program records what it always recorded.  ``L=None``: a program without geometry.
    ``wrap``: wrap-around padding of every 3x3 conv, downsampler and upsampler the program emits (``Emitter.wrap``; 0: none).
    A subclass allocates its buffers, then records each ``Program`` it owns inside ``with self._recording(prog):``; its emitting
    code calls ``_mark`` at the end of every unit it wants to be seen.  ``programs``: the recorded ``Program``s in order."""

    def __init__(self, net, B: int, L=None, ragged_halo: bool = True, journal: bool = False, wrap: int = 0):
        self.net, self.B = net, B
        self.arena = Arena(net.device, journal=journal)
        self.em = Emitter(self.arena)
        if int(wrap) & ~3 or int(wrap) < 0:
            raise ValueError(f"RecordedProgram: wrap must be 0, 1 (x), 2 (y) or 3 (both), got {wrap!r}")
        self.wrap = self.em.wrap = int(wrap)
        if L is not None:
            self.H, self.W = latent_hw(L)
            self.L = self.H if self.H == self.W else None
            self.ragged_halo = self.em.ragged_halo = bool(ragged_halo) and self.H != self.W
        self.marks: List[Mark] = []
        self.tap_names: Dict[str, str] = {}            # alias (the oracle's block taps) -> the unit whose output it is
        self.taps: Dict[str, torch.Tensor] = {}
        self.persistent: List[torch.Tensor] = []       # arena tensors that stay live after emission
        self.programs: Tuple[Program, ...] = ()
        self._rec: Optional[Program] = None

    @contextlib.contextmanager
    def _recording(self, prog: Program):
        """``prog`` records, the arena's journal carries its clock, ``_mark`` counts its ops."""
        self.programs += (prog,)
        self._rec = prog
        try:
            with prog.record(), self.arena.clocked(prog):
                yield prog
        finally:
            self._rec = None

    def _mark(self, name: str, kind: str, out: torch.Tensor, *inputs: str) -> str:
        self.marks.append(Mark(name, kind, self._rec.name, self._rec.num_ops, out, tuple(inputs)))
        return name

    def capture(self, convert=None) -> Dict[str, torch.Tensor]:
        """Replay the programs on what the input buffers hold now, unit by unit, and keep a clone of every unit's output in ``taps``
        (``convert(mark, clone)`` may change what is kept), also under the aliases of ``tap_names``.  Leaves the outputs as a plain
        run would."""
        taps = capture_marks({p.name: p for p in self.programs}, self.marks, convert)
        for tap, unit in self.tap_names.items():
            taps[tap] = taps[unit]
        self.taps = taps
        return taps

    def enable_graphs(self) -> None:
        for p in self.programs:
            p.instantiate()
