"""ctypes binding of ``liblbhip.so`` (contract: ``include/lb_hip.h``).

The library is built in-tree by ``latentblending_amd/csrc/build.py`` (``__graft_entry__.build()``)
and loaded AFTER ``import torch`` so that both share one HIP runtime.  There is no fallback: a
missing library raises ``ImportError``; a failing launch raises ``RuntimeError`` with the
library's own error string.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional, Tuple, Union

import torch  # noqa: F401  (must be imported first: shares libamdhip64 with the extension)

_HERE = os.path.dirname(os.path.abspath(__file__))
# LB_HIP_LIBRARY: an alternate build of the SAME library (kernel ablation studies, tools/gemm_ablate.py)
LIB_PATH = os.environ.get("LB_HIP_LIBRARY") or os.path.join(_HERE, "liblbhip.so")

c_void_pp = C.POINTER(C.c_void_p)


class LbGemmParams(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p),
        ("residual", C.c_void_p), ("rowvec", C.c_void_p), ("partial", C.c_void_p),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("lda", C.c_int), ("ldw", C.c_int), ("ldc", C.c_int), ("ldr", C.c_int),
        ("ld_rowvec", C.c_int), ("rows_per_batch", C.c_int),
        ("alpha", C.c_float), ("flags", C.c_int),
        ("conv", C.c_int), ("Hin", C.c_int), ("Win", C.c_int), ("Cin", C.c_int),
        ("Hout", C.c_int), ("Wout", C.c_int), ("KH", C.c_int), ("KW", C.c_int),
        ("stride", C.c_int), ("pad", C.c_int), ("ups", C.c_int), ("ldx", C.c_int),
        ("splitk", C.c_int), ("zero_page", C.c_void_p),
        ("scatter", C.c_int), ("sc_py", C.c_int), ("sc_px", C.c_int), ("reserved_", C.c_int),
        ("ln_colsum", C.c_void_p), ("ln_eps", C.c_float), ("reserved2_", C.c_int), ("ch_stats", C.c_void_p), ("ch_stats_rows", C.c_int),
        ("gn_table", C.c_void_p), ("gn_silu", C.c_int), ("wrap", C.c_int),
    ]


class LbConvPlan(C.Structure):
    """What lb_conv_plan answers for one conv (include/lb_hip.h); ``route`` is one of ROUTE_*."""
    _fields_ = [
        ("route", C.c_int), ("tile", C.c_int), ("splitk", C.c_int), ("blocks", C.c_long),
        ("halo_kind", C.c_int), ("halo_tile_w", C.c_int), ("halo_items", C.c_long), ("halo_grid", C.c_long),
        ("stat_rows", C.c_int), ("ksplit_split", C.c_int),
        ("ksplit_units", C.c_long), ("ksplit_grid", C.c_long), ("ksplit_counter_bytes", C.c_long), ("ksplit_slab_bytes", C.c_long),
        ("gn_a_fuse", C.c_int), ("gn_a_kind", C.c_int), ("ragged_kind", C.c_int), ("ragged_tile_w", C.c_int),
    ]


ROUTE_GEMM, ROUTE_C64, ROUTE_UPCONV_HALO, ROUTE_NARROW, ROUTE_HALO3 = range(5)


class LbAttnParams(C.Structure):
    _fields_ = [
        ("Q", C.c_void_p), ("K", C.c_void_p), ("V", C.c_void_p), ("O", C.c_void_p),
        ("B", C.c_int), ("H", C.c_int), ("Sq", C.c_int), ("Skv", C.c_int), ("Skv_valid", C.c_int),
        ("ldq", C.c_int), ("ldk", C.c_int), ("ldv", C.c_int), ("ldo", C.c_int),
        ("scale", C.c_float), ("causal", C.c_int), ("zero_page", C.c_void_p), ("reserved_", C.c_int),
    ]


GEMM_OUT_F32, GEMM_RES_F32, GEMM_GEGLU, GEMM_TRANS_OUT, GEMM_SILU, GEMM_RELU, GEMM_LN_A = 1, 2, 4, 8, 16, 32, 64
GEMM_QUICK_GELU, GEMM_GELU, GEMM_CH_STATS = 128, 256, 512
GEMM_HALO_RAGGED = 1024      # opt-in ragged tiles of the 3x3 halo conv (include/lb_hip.h)
GEMM_HALO_KSPLIT = 4096     # opt-in K-split form of the 3x3 halo conv: partial = lb_conv_halo_ksplit_workspace_bytes (include/lb_hip.h)
GEMM_GN_A = 8192            # A consumed through a GroupNorm affine table (gn_table / gn_silu): halo and narrow-N 3x3 convs (include/lb_hip.h)
GEMM_C64 = 2048              # opt-in 64 -> 64 channel 3x3 conv with LDS-resident weights: that kernel or a refusal (include/lb_hip.h)


class _ConvGeomFields(NamedTuple):
    Hin: int
    Win: int
    Cin: int
    KH: int
    KW: int
    stride: int
    pad: int
    ups: int
    ldx: int
    parity: Union[None, str, Tuple[int, int]]
    Hout: int
    Wout: int


class ConvGeom(_ConvGeomFields):
    """The geometry of one implicit-GEMM convolution over an NHWC input whose pixels are ``ldx`` elements apart (None: ``Cin``): a
    frozen value.  ``ups``: the conv reads the nearest-2^ups upsampled input.  ``parity``: a sub-pixel upsampler conv on the low-res
    grid that scatters into the 2H x 2W output - ``(py, px)`` one of the four, ``"all"`` the four in one launch (W stacked
    [4][N][K]).  ``Hout`` / ``Wout`` are derived here and nowhere else: the rows and columns the launch computes per sample - of the
    output, or of the low-res grid for a sub-pixel conv.  (A tuple underneath: the emitters build one per launch.)

    ``wrap``: wrap-around ("circular") padding, bit 0 = the columns wrap (left and right edges join), bit 1 = the rows wrap
    (LbGemmParams.wrap, include/lb_hip.h).  Defined for the "same" geometries only - 3x3 / pad 1 at stride 1, at stride 2 with an even
    effective side on every wrapped axis, ``ups`` 0 or 1, and the sub-pixel forms (on the low-res grid) - anything else raises
    ``ValueError``.  It is a TRAILING element that exists only when it is not zero: a geometry built without it is the twelve-element
    value it always was, a wrapped one carries a thirteenth - so equality and hash tell them apart, and ``g.wrap`` reads 0 or the bits.
    (The shape is forced: the twelve-element value of an unwrapped geometry is pinned by the tests, and ``wrap`` has to take part in
    equality and hash.)  Consequences: read a geometry through its attributes or ``g[:12]``, never by a twelve-way unpack of the
    whole tuple; ``_asdict`` and ``_replace`` know about ``wrap`` (below), ``_make`` - which cannot tell the two shapes apart - is
    refused."""
    __slots__ = ()

    def __new__(cls, Hin: int, Win: int, Cin: int, KH: int, KW: int, stride: int = 1, pad: int = 0, ups: int = 0,
                ldx: Optional[int] = None, parity=None, wrap: int = 0):
        if parity is None:
            Hout, Wout = ((Hin << ups) + 2 * pad - KH) // stride + 1, ((Win << ups) + 2 * pad - KW) // stride + 1
        else:
            Hout, Wout = Hin, Win
        g = tuple.__new__(cls, (Hin, Win, Cin, KH, KW, stride, pad, ups, Cin if ldx is None else ldx, parity, Hout, Wout))
        return g.with_wrap(wrap)

    def with_wrap(self, wrap: int) -> "ConvGeom":
        """This geometry with ``wrap`` (0: without any); ``ValueError`` where wrap-around padding is not defined (see the class)."""
        wrap = int(wrap)
        if not wrap:
            return self if len(self) == 12 else tuple.__new__(type(self), self[:12])
        why = self.wrap_refusal(wrap)
        if why:
            raise ValueError(f"ConvGeom: wrap={wrap} {why}")
        return tuple.__new__(type(self), self[:12] + (wrap,))

    def wrap_refusal(self, wrap: int) -> Optional[str]:
        """Why this geometry cannot wrap with these bits (None: it can) - the host twin of lb_wrap_defined (csrc/lb_gemm.h)."""
        if wrap & ~3 or wrap < 0:
            return "has bits other than 0 (x: the columns wrap) and 1 (y: the rows wrap)"
        if self.parity is not None:
            return None if (self.KH, self.KW, self.stride, self.ups) == (2, 2, 1, 0) else "needs the 2x2 sub-pixel form"
        if (self.KH, self.KW, self.pad) != (3, 3, 1) or self.stride not in (1, 2) or self.ups not in (0, 1):
            return f"is defined for 3x3 / pad 1 convs of stride 1 or 2 only (got {self.KH}x{self.KW}, stride {self.stride}, pad {self.pad}, ups {self.ups})"
        if self.stride == 2 and ((wrap & 2 and (self.Hin << self.ups) % 2) or (wrap & 1 and (self.Win << self.ups) % 2)):
            return f"at stride 2 needs an even side on every wrapped axis (got {self.Hin << self.ups} x {self.Win << self.ups})"
        return None

    @property
    def wrap(self) -> int:
        return self[12] if len(self) > 12 else 0

    def _asdict(self) -> dict:
        d = dict(zip(self._fields, self))
        if self.wrap:
            d["wrap"] = self.wrap
        return d

    def _replace(self, **kw) -> "ConvGeom":
        """A geometry with the named CONSTRUCTOR fields (``Hin`` .. ``parity``, ``wrap``) replaced; ``Hout`` / ``Wout`` are derived
        anew, so they cannot be named.  (A ``down3x3`` geometry, whose ``Hout`` a symmetric pad cannot express, is refused.)"""
        args = ("Hin", "Win", "Cin", "KH", "KW", "stride", "pad", "ups", "ldx", "parity")
        bad = set(kw) - set(args) - {"wrap"}
        if bad:
            raise ValueError(f"ConvGeom._replace: cannot replace {sorted(bad)} (Hout / Wout are derived)")
        cur = {k: getattr(self, k) for k in args}
        if self[:12] != type(self)(**cur)[:12]:
            raise ValueError("ConvGeom._replace: this geometry was not built by the general constructor (down3x3)")
        cur.update({k: v for k, v in kw.items() if k != "wrap"})
        return type(self)(**cur, wrap=kw.get("wrap", self.wrap))

    @classmethod
    def _make(cls, iterable):
        raise TypeError("ConvGeom._make: build a geometry through ConvGeom(...), conv3x3, down3x3 or subpixel")

    def __repr__(self) -> str:
        body = ", ".join(f"{n}={v!r}" for n, v in zip(self._fields, self))
        return f"ConvGeom({body}" + (f", wrap={self.wrap})" if self.wrap else ")")

    @classmethod
    def conv3x3(cls, H: int, W: int, cin: int, stride: int = 1, ups: int = 0, ldx: Optional[int] = None, wrap: int = 0) -> "ConvGeom":
        return cls(H, W, cin, 3, 3, stride, 1, ups, ldx, wrap=wrap)

    @classmethod
    def down3x3(cls, H: int, W: int, cin: int, ldx: Optional[int] = None) -> "ConvGeom":
        """The SDXL VAE encoder's downsampler: 3x3 / stride 2 / pad 0 over the input padded by one zero row at the bottom and one
        zero column at the right ONLY (``F.pad(x, (0, 1, 0, 1))``).  Output (oy, ox) reads rows 2 oy .. 2 oy + 2, so the last output
        row and column reach one pixel past the image: the implicit-GEMM gather masks them (``iy < Hin``, ``ix < Win``).  ``Hout`` =
        H / 2 is what a symmetric ``pad`` cannot express; H and W must be even (an odd side would need no far pad at all).
        (It pads one side only: wrap-around padding is not defined for it, and ``with_wrap`` refuses it.)"""
        if H <= 0 or W <= 0 or H % 2 or W % 2:
            raise ValueError(f"ConvGeom.down3x3: H and W must be positive and even (got {H} x {W})")
        return tuple.__new__(cls, (H, W, cin, 3, 3, 2, 0, 0, cin if ldx is None else ldx, None, H // 2, W // 2))

    @classmethod
    def subpixel(cls, H: int, W: int, cin: int, parity, ldx: Optional[int] = None, wrap: int = 0) -> "ConvGeom":
        return cls(H, W, cin, 2, 2, ldx=ldx, parity=parity, wrap=wrap)

    @property
    def scatter(self) -> int:
        return 0 if self.parity is None else 2 if self.parity == "all" else 1

    @property
    def K(self) -> int:
        return self.KH * self.KW * self.Cin

    def M(self, B: int) -> int:
        return B * self.Hout * self.Wout


def gemm_params(*, M: int, N: int, K: int, ldw: int, ldc: int, lda: int = 0, A: Optional[int] = None, W: Optional[int] = None,
                C: Optional[int] = None, conv: Optional[ConvGeom] = None, bias: Optional[int] = None, residual: Optional[int] = None,
                ldr: int = 0, rowvec: Optional[int] = None, ld_rowvec: int = 0, rows_per_batch: int = 0, alpha: float = 1.0,
                flags: int = 0, zero_page: Optional[int] = None, partial: Optional[int] = None, ln=None, ch_stats=None,
                gn=None, make=LbGemmParams) -> LbGemmParams:
    """THE constructor of the block lb_gemm_f16 and the plan calls read: integers in, block out - no tensor, no allocation, no
    launch, no plan.  Pointers are addresses or None.  ``lda`` counts for a plain GEMM, ``conv`` for a convolution; ``ld_rowvec`` /
    ``rows_per_batch`` only with a ``rowvec``.  ``ln`` = (colsum pointer, eps), ``ch_stats`` = (pointer, rows), ``gn`` = (table
    pointer, silu) each set their flag bit (LB_GEMM_LN_A / LB_GEMM_CH_STATS / LB_GEMM_GN_A).  ``splitk`` and the reserved words stay
    zero.  ``make``: what creates the empty block - ``ops.gemm`` passes its module's own ``LbGemmParams``, the name the replay tests
    wrap to find (and later destroy) every block a wrapper built."""
    p = make()
    p.A, p.W, p.C, p.bias, p.residual, p.rowvec, p.partial = A, W, C, bias, residual, rowvec, partial
    p.M, p.N, p.K, p.lda, p.ldw, p.ldc, p.ldr = M, N, K, lda, ldw, ldc, ldr
    if rowvec is not None:
        p.ld_rowvec, p.rows_per_batch = ld_rowvec, rows_per_batch
    p.alpha, p.flags, p.zero_page = alpha, flags, zero_page
    if conv is not None:
        p.conv = 1
        p.Hin, p.Win, p.Cin, p.KH, p.KW, p.stride, p.pad, p.ups, p.ldx, parity, p.Hout, p.Wout = conv[:12]
        if conv.wrap:
            p.wrap = conv.wrap
        if parity is not None:
            p.scatter = conv.scatter
            if parity != "all":
                p.sc_py, p.sc_px = int(parity[0]), int(parity[1])
    if ln is not None:
        p.flags |= GEMM_LN_A
        p.ln_colsum, p.ln_eps = ln[0], float(ln[1])
    if ch_stats is not None:
        p.flags |= GEMM_CH_STATS
        p.ch_stats, p.ch_stats_rows = ch_stats
    if gn is not None:
        p.flags |= GEMM_GN_A
        p.gn_table, p.gn_silu = gn[0], int(bool(gn[1]))
    return p

_vp, _i, _l, _f, _d = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double
_pp, _pi, _pl = C.POINTER(LbGemmParams), C.POINTER(_i), C.POINTER(_l)

# What an entry point is to a caller, and with it how it is bound:
#   _L "launcher": takes the stream as its last void*, returns an int status and can be recorded into a program (tests/_replay.py
#                  holds one replay case per launcher); bound through the checking wrapper
#   _S "status":   returns an int status but is nothing a program records; bound through the checking wrapper
#   _V "value":    returns a value or nothing (sizes, plans that answer through out-pointers, setters); bound raw
_L, _S, _V = "launcher", "status", "value"

# every symbol include/lb_hip.h declares outside its study block: name -> (restype, argtypes, role)
SIGNATURES = {
    "lb_version": (_i, [], _V),
    "lb_last_error_string": (C.c_char_p, [], _V),
    "lb_device_info": (_i, [_i, _pi, _pl, C.c_char_p, _i], _S),
    "lb_slerp_pairs_f16": (_i, [c_void_pp, c_void_pp, c_void_pp, C.POINTER(_d), _i, _l, _vp], _L),
    "lb_slerp_pairs_f32": (_i, [c_void_pp, c_void_pp, c_void_pp, C.POINTER(_d), _i, _l, _vp], _L),
    "lb_slerp_pairs_f64": (_i, [c_void_pp, c_void_pp, c_void_pp, C.POINTER(_d), _i, _l, _vp], _L),
    "lb_slerp_batched_f16": (_i, [_vp, _vp, _vp, _vp, _l, _l, _vp], _L),
    "lb_slerp_strided_f16": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _l, _vp], _L),
    "lb_lerp_f16": (_i, [_vp, _vp, _vp, _l, _d, _vp], _L),
    "lb_lerp_f32": (_i, [_vp, _vp, _vp, _l, _d, _vp], _L),
    "lb_scale_model_input_f16": (_i, [_vp, _vp, _vp, _l, _i, _i, _vp], _L),
    "lb_euler_step_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _vp], _L),
    "lb_ddim_step_f16": (_i, [_vp, _vp, _vp, _vp, _l, _i, _i, _vp], _L),
    "lb_lcm_step_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _vp], _L),
    "lb_dpmpp2m_step_f16": (_i, [_vp, _vp, _vp, _vp, _l, _i, _i, _vp], _L),
    "lb_counter_noise_f16": (_i, [_vp, _vp, _l, _i, _i, _vp], _L),
    "lb_gemm_f16": (_i, [_pp, _vp], _L),
    "lb_gemm_workspace_bytes": (_l, [_i, _i], _V),
    "lb_gemm_set_tuning": (None, [_i, _i], _V),
    "lb_gemm_set_depth": (None, [_i], _V),
    "lb_gemm_set_variant": (None, [_i, _i], _V),
    "lb_gemm_set_wide_store": (None, [_i], _V),
    "lb_gemm_set_lean_epilogue": (None, [_i], _V),
    "lb_gemm_set_t192_waves8": (None, [_i], _V),
    "lb_gemm_set_kgroups": (None, [_i], _V),
    "lb_gemm_pp_set_group": (None, [_i], _V),
    "lb_gemm_set_pp_auto": (None, [_i], _V),
    "lb_gemm_set_halo": (None, [_i], _V),
    "lb_conv3x3_halo_f16": (_i, [_pp, _vp], _L),
    "lb_conv3x3_narrow_f16": (_i, [_pp, _vp], _L),
    "lb_upconv2x_halo_f16": (_i, [_pp, _vp], _L),
    "lb_conv_halo_set_persistent": (None, [_i], _V),
    "lb_gemm_ch_stat_rows": (_i, [_pp], _V),
    "lb_conv_halo_plan": (None, [_pp, _pi, _pi, _pl, _pl], _V),
    "lb_conv_halo_ksplit_plan": (None, [_pp, _pl, _pl, _pi], _V),
    "lb_conv_halo_ksplit_workspace_bytes": (_l, [_pp], _V),
    "lb_conv_halo_set_ksplit": (None, [_i, _i], _V),
    "lb_conv_halo_gn_a_plan": (None, [_pp, _pi, _pi], _V),
    "lb_conv_halo_set_gn_a": (None, [_i, _i], _V),
    "lb_gemm_plan": (_i, [_pp, _pi, _pi, _pl], _S),
    "lb_conv_plan": (_i, [_pp, C.POINTER(LbConvPlan)], _S),
    "lb_groupnorm_workspace_bytes": (_l, [_i, _i], _V),
    "lb_groupnorm_set_l3_chunk": (None, [_l], _V),
    "lb_groupnorm_nhwc": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _i, _vp], _L),
    "lb_groupnorm_from_stats": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _vp], _L),
    "lb_groupnorm_affine_from_stats": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp], _L),
    "lb_layernorm_f16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp], _L),
    "lb_attn_fwd_d64": (_i, [C.POINTER(LbAttnParams), _vp], _L),
    "lb_attn_fwd_d512": (_i, [C.POINTER(LbAttnParams), _vp], _L),
    "lb_attn_set_tuning": (None, [_i], _V),
    "lb_layernorm_set_form": (None, [_i], _V),
    "lb_groupnorm_set_fused": (None, [_i], _V),
    "lb_groupnorm_plan": (_i, [_i, _i, _i, _i], _V),
    "lb_softmax_rows_f16": (_i, [_vp, _i, _i, _i, _f, _vp], _L),
    "lb_sinusoid_f16": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp], _L),
    "lb_copy_cols_f16": (_i, [_vp, _vp, _l, _i, _i, _i, _i, _vp], _L),
    "lb_cast_f16_to_f32": (_i, [_vp, _vp, _l, _vp], _L),
    "lb_cast_f32_to_f16": (_i, [_vp, _vp, _l, _f, _vp], _L),
    "lb_nchw_to_nhwc_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp], _L),
    "lb_nhwc_to_nchw_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp], _L),
    "lb_postprocess_u8": (_i, [_vp, _vp, _l, _i, _i, _vp], _L),
    "lb_lpips_prep_u8": (_i, [_vp, _vp, _l, _vp], _L),
    "lb_maxpool3s2_nhwc_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp], _L),
    "lb_lpips_tap": (_i, [c_void_pp, c_void_pp, _vp, _vp, _vp, _i, _i, _i, _vp], _L),
    "lb_fill_f32": (_i, [_vp, _l, _f, _vp], _L),
    "lb_embed_tokens_f16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _L),
    "lb_frames_lerp_u8": (_i, [_vp, _vp, _vp, _vp, _l, _l, _vp], _L),
    "lb_gather_rows_f16": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp], _L),
    "lb_copy_d2d": (_i, [_vp, _vp, _l, _vp], _L),
    "lb_jpeg_dct_quant_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp], _L),
    "lb_jpeg_coefficient_count": (_l, [_i, _i, _i, _i], _V),
    "lb_jpeg_entropy": (_i, [_vp, _vp, _vp, _l, _vp, _i, _i, _i, _i, _vp], _L),
    "lb_jpeg_workspace_bytes": (_l, [_i, _i, _i, _i], _V),
    "lb_resample_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp], _L),
    "lb_program_create": (_vp, [], _V),
    "lb_program_destroy": (None, [_vp], _V),
    "lb_program_begin_record": (_i, [_vp], _S),
    "lb_program_end_record": (_i, [_vp], _S),
    "lb_program_recording": (_i, [], _V),
    "lb_program_num_ops": (_i, [_vp], _V),
    "lb_program_op_name": (C.c_char_p, [_vp, _i], _V),
    "lb_program_run": (_i, [_vp, _vp], _S),
    "lb_program_run_range": (_i, [_vp, _i, _i, _vp], _S),
    "lb_program_instantiate": (_i, [_vp], _S),
    "lb_program_launch": (_i, [_vp, _vp], _S),
    "lb_program_time_ops": (_i, [_vp, _vp, C.POINTER(_f)], _S),
}

# exported only by study builds (-DLB_STUDY_BUILD, liblbhip_study.so): switches that change the arithmetic / the tile policy;
# absent from the product library, so bound only where the loaded library has them
STUDY_SIGNATURES = {
    "lb_slerp_set_study": (None, [_i], _V),
    "lb_gemm_set_policy": (None, [_i], _V),
    "lb_conv_halo_set_study": (None, [_i], _V),
}


def _load():
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            f"latentblending_amd: {LIB_PATH} is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
            "There is no CPU fallback for the kernel path.")
    return C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)


_lib = _load()


class _Api:
    pass


def _wrap(name, fn):
    def checked(*args):
        rc = fn(*args)
        if rc != 0:
            msg = _lib.lb_last_error_string()
            raise RuntimeError(f"{name} failed ({rc}): {msg.decode() if msg else '?'}")
        return rc
    checked.__name__ = name
    return checked


api = _Api()
for _name, (_res, _args, _role) in {**SIGNATURES, **STUDY_SIGNATURES}.items():
    if _name in STUDY_SIGNATURES and not hasattr(_lib, _name):
        continue
    _fn = getattr(_lib, _name)          # AttributeError here == header/library mismatch
    _fn.restype = _res
    _fn.argtypes = _args
    setattr(api, _name, _fn if _role == _V else _wrap(_name, _fn))

if os.environ.get("LB_GEMM_WIDE_STORE"):        # tuning experiments (tools/): 16-byte epilogue stores
    api.lb_gemm_set_wide_store(int(os.environ["LB_GEMM_WIDE_STORE"]))
if os.environ.get("LB_GEMM_LEAN_EPILOGUE"):     # A/B studies (tools/): 0 = the per-row tile epilogue everywhere
    api.lb_gemm_set_lean_epilogue(int(os.environ["LB_GEMM_LEAN_EPILOGUE"]))
if os.environ.get("LB_GEMM_PP_AUTO"):           # A/B studies (tools/): 0 = the tile policy never picks the ping-pong GEMM
    api.lb_gemm_set_pp_auto(int(os.environ["LB_GEMM_PP_AUTO"]))


def conv_plan(p: LbGemmParams) -> LbConvPlan:
    """lb_conv_plan's record for ``p``: the route lb_gemm_f16 takes and every plan answer for it, in one call."""
    plan = LbConvPlan()
    api.lb_conv_plan(C.byref(p), C.byref(plan))
    return plan


def conv_probe(B: int, H: int, W: int, cin: int, cout: int, ks: int = 3, flags: int = 0, zero_page: int = 64, wrap: int = 0) -> LbGemmParams:
    """The parameter block of a 3x3 / stride 1 / pad 1 conv (``ks`` = 3) or a one-launch sub-pixel upsampler conv (``ks`` = 2) of
    this geometry, for the plan calls: host arithmetic only reads whether ``zero_page`` is set."""
    g = ConvGeom.conv3x3(H, W, cin, wrap=wrap) if ks == 3 else ConvGeom(H, W, cin, ks, ks, parity="all", wrap=wrap)
    return gemm_params(M=g.M(B), N=cout, K=g.K, ldw=0, ldc=0, conv=g, alpha=0.0, flags=flags, zero_page=zero_page)
