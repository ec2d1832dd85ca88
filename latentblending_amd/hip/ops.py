"""Tensor-level wrappers over the C-ABI launchers (torch is used for device memory and the
current stream only).  These are what the parity tests and the thin host layer call; the model
programs in ``latentblending_amd.native`` talk to ``lib.api`` directly with raw pointers.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch

from . import lib
from .lib import api, LbGemmParams, LbAttnParams

F16, F32, F64 = torch.float16, torch.float32, torch.float64


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _own_buffer(wrapper: str, what: str) -> None:
    """A wrapper about to allocate a device buffer it does not return calls this first: while the calling thread records a
    program the closure would keep a pointer that the caching allocator reuses as soon as the wrapper returns."""
    if api.lb_program_recording():
        raise RuntimeError(f"{wrapper}: called while a program is recording without a caller-owned {what}; "
                           f"pass one in (and keep it alive as long as the program) or call lib.api directly")


def _operand(wrapper: str, given: torch.Tensor, used: torch.Tensor) -> torch.Tensor:
    """``used`` is ``given`` made contiguous / converted: a temporary copy, if one had to be made, is such a buffer too."""
    if used.data_ptr() != given.data_ptr():
        _own_buffer(wrapper, "contiguous operand of the kernel's dtype (the wrapper had to copy this one)")
    return used


def _ptr_array(tensors: Sequence[torch.Tensor]):
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return C.cast(arr, lib.c_void_pp), arr


# ------------------------------------------------------------------------------ mixing -----
def slerp_pairs(p0: List[torch.Tensor], p1: List[torch.Tensor], fracts: List[float]) -> List[torch.Tensor]:
    assert len(p0) == len(p1) == len(fracts) and len(p0) > 0
    dt = p0[0].dtype
    if dt not in (F16, F32, F64):            # bf16 etc.: the reference would return fp32 as well
        p0 = [t.float() for t in p0]
        p1 = [t.float() for t in p1]
        dt = F32
    a = [_operand("slerp_pairs", t, t.contiguous()) for t in p0]
    b = [_operand("slerp_pairs", t, t.to(dt).contiguous()) for t in p1]
    n = a[0].numel()
    assert all(t.numel() == n and t.is_cuda for t in a + b), "slerp_pairs: equal-sized device tensors"
    outs = [torch.empty(t.shape, dtype=F16 if dt == F16 else F32, device=t.device) for t in a]
    pa, keep_a = _ptr_array(a)
    pb, keep_b = _ptr_array(b)
    po, keep_o = _ptr_array(outs)
    fr = (C.c_double * len(fracts))(*[float(f) for f in fracts])
    fn = {F16: api.lb_slerp_pairs_f16, F32: api.lb_slerp_pairs_f32, F64: api.lb_slerp_pairs_f64}[dt]
    fn(pa, pb, po, fr, len(a), n, stream_ptr())
    return outs


def slerp(p0: torch.Tensor, p1: torch.Tensor, fract: float) -> torch.Tensor:
    return slerp_pairs([p0], [p1], [fract])[0]


def slerp_batched(p0: torch.Tensor, p1: torch.Tensor, fracts_dev: torch.Tensor) -> torch.Tensor:
    """p0, p1: [npairs, n] fp16 contiguous; fracts_dev: float64 [npairs] on device."""
    assert p0.dtype == F16 and p0.is_contiguous() and p1.is_contiguous() and fracts_dev.dtype == F64
    out = torch.empty_like(p0)
    api.lb_slerp_batched_f16(p0.data_ptr(), p1.data_ptr(), out.data_ptr(), fracts_dev.data_ptr(),
                             p0.shape[0], p0.shape[1], stream_ptr())
    return out


def slerp_strided(p0: torch.Tensor, p1: torch.Tensor, fracts_dev: torch.Tensor, n: int,
                  broadcast0: bool = False, broadcast1: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[g] = slerp(p0[g or 0], p1[g or 0], fracts_dev[g]) for g < len(fracts_dev); inputs fp16, contiguous
    [G, n] (or one tensor of n elements when broadcast); fracts_dev float64 on device.  One launch, no host pointers."""
    G = fracts_dev.numel()
    assert p0.dtype == F16 and p1.dtype == F16 and fracts_dev.dtype == F64 and p0.is_contiguous() and p1.is_contiguous()
    if out is None:
        out = torch.empty(G, n, dtype=F16, device=p0.device)
    api.lb_slerp_strided_f16(p0.data_ptr(), 0 if broadcast0 else n, p1.data_ptr(), 0 if broadcast1 else n, out.data_ptr(),
                             fracts_dev.data_ptr(), G, n, stream_ptr())
    return out


def lerp(p0: torch.Tensor, p1: torch.Tensor, fract: float) -> torch.Tensor:
    a, b = _operand("lerp", p0, p0.contiguous()), _operand("lerp", p1, p1.contiguous())
    if a.dtype == F16 and b.dtype == F16:
        out = torch.empty_like(a)
        api.lb_lerp_f16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), float(fract), stream_ptr())
        return out
    a, b = _operand("lerp", a, a.float()), _operand("lerp", b, b.float())
    out = torch.empty_like(a)
    api.lb_lerp_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), float(fract), stream_ptr())
    return out


# ------------------------------------------------------------------------------ scheduler --
def step_params(rows: Sequence[Sequence[float]], device) -> torch.Tensor:
    """rows of (sigma_from, sigma_next, sigma_up, guidance, dt) -> float32 [B, 8] on device."""
    # (ONE host tensor from nested lists - a cfg-2 wavefront uploads 34 + 8 rows: the per-row tensor constructions of rounds 1-5 cost
    #  ~0.1 ms of host time in front of a transition's first launch)
    t = torch.tensor([[float(v) for v in r] + [0.0] * (8 - len(r)) for r in rows], dtype=F32).reshape(len(rows), 8)
    dev = t.to(device)
    dev._lb_host_rows = t           # host mirror (lcm_step decides from it whether a null noise pointer is legal; views lose it)
    return dev


def scale_model_input(x: torch.Tensor, params: torch.Tensor, dup_for_cfg: bool = False) -> torch.Tensor:
    B = x.shape[0]
    out = torch.empty((2 * B if dup_for_cfg else B,) + tuple(x.shape[1:]), dtype=F16, device=x.device)
    api.lb_scale_model_input_f16(x.data_ptr(), out.data_ptr(), params.data_ptr(), x[0].numel(), B,
                                 int(dup_for_cfg), stream_ptr())
    return out


def euler_step(x, eps, params, noise=None, cfg=False, ancestral=False) -> torch.Tensor:
    assert x.is_contiguous() and eps.is_contiguous(), "euler_step: the kernel takes its operands by pointer"
    if noise is not None and not noise.is_contiguous():
        noise = _operand("euler_step", noise, noise.contiguous())
    out = torch.empty_like(x)
    api.lb_euler_step_f16(x.data_ptr(), eps.data_ptr(), _ptr(noise), out.data_ptr(), params.data_ptr(),
                          x[0].numel(), x.shape[0], int(bool(cfg)), int(bool(ancestral)), stream_ptr())
    return out


def lcm_step(x, eps, params, noise=None, cfg=False, all_last: Optional[bool] = None) -> torch.Tensor:
    """Latent-consistency step (``lb_lcm_step_f16``); ``params`` rows as NativeLCMScheduler.step_row builds them.
    ``noise`` may be None only when EVERY row is a last step of its schedule (slot 5 == 0: the denoised latent is the result
    and the noise is not read).  That is decided on the host, never by reading the rows back: from the host mirror
    ``step_params`` leaves on the tensor it returns, or - for a view of such a tensor, which has none - from ``all_last``,
    the caller's own statement about the rows it built.  A null ``noise`` that neither establishes as legal is refused
    here, before anything is launched."""
    assert x.is_contiguous() and eps.is_contiguous(), "lcm_step: the kernel takes its operands by pointer"
    host = getattr(params, "_lb_host_rows", None)
    known = None if host is None else bool((host.reshape(-1, 8)[:, 5] == 0).all())
    if known is not None and all_last is not None and bool(all_last) and not known:
        raise ValueError("lcm_step: all_last=True, but the host rows hold a step that is not the last of its schedule")
    flag = known if known is not None else (bool(all_last) if all_last is not None else None)
    if noise is None and flag is not True:
        raise ValueError("lcm_step: noise=None needs every row to be a last step (slot 5 == 0)"
                         + ("; these rows are not" if flag is False else
                            "; that cannot be established on the host for this params tensor (pass all_last=)"))
    if noise is not None and not noise.is_contiguous():
        noise = _operand("lcm_step", noise, noise.contiguous())
    if noise is not None:
        assert noise.shape == x.shape and noise.dtype == F16, "lcm_step: noise must be an fp16 tensor of the latent's shape"
    out = torch.empty_like(x)
    api.lb_lcm_step_f16(x.data_ptr(), eps.data_ptr(), _ptr(noise), out.data_ptr(), params.data_ptr(),
                        x[0].numel(), x.shape[0], int(bool(cfg)), int(noise is None), stream_ptr())
    return out


def ddim_step(x, eps, params, cfg=False) -> torch.Tensor:
    """DDIM step (eta = 0); ``params`` rows as NativeDDIMScheduler.step_row builds them."""
    out = torch.empty_like(x)
    api.lb_ddim_step_f16(x.data_ptr(), eps.data_ptr(), out.data_ptr(), params.data_ptr(), x[0].numel(), x.shape[0],
                         int(bool(cfg)), stream_ptr())
    return out


def dpmpp2m_step(state, eps, params, cfg=False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """DPM-Solver++ 2M step (``lb_dpmpp2m_step_f16``); ``params`` rows as NativeDPMSolverPP2MScheduler.step_row
    builds them.  ``state`` is ``[2, B, ...]`` fp16: plane 0 the latents, plane 1 the previous step's x0 prediction (not read for
    a first-order row).  Returns the new state - next latents and this step's x0 prediction - in ``out``, which must not share
    memory with ``state``; while a program records, the caller owns ``out``."""
    if state.dim() < 3 or state.shape[0] != 2:
        raise ValueError(f"dpmpp2m_step: state must have two planes, [2, B, ...] (got shape {tuple(state.shape)})")
    assert state.dtype == F16 and eps.dtype == F16 and state.is_contiguous() and eps.is_contiguous(), \
        "dpmpp2m_step: the kernel takes contiguous fp16 operands by pointer"
    B = state.shape[1]
    if eps.shape[0] != B * (2 if cfg else 1) or eps[0].numel() != state[0, 0].numel():
        raise ValueError(f"dpmpp2m_step: eps of shape {tuple(eps.shape)} does not go with a state of shape {tuple(state.shape)} (cfg={bool(cfg)})")
    if out is None:
        _own_buffer("dpmpp2m_step", "out")
        out = torch.empty_like(state)
    if out.shape != state.shape or out.dtype != F16 or not out.is_contiguous():
        raise ValueError(f"dpmpp2m_step: out must be a contiguous fp16 tensor of the state's shape, two planes (got {tuple(out.shape)})")
    nbytes = state.numel() * state.element_size()
    if out.data_ptr() < state.data_ptr() + nbytes and state.data_ptr() < out.data_ptr() + nbytes:
        raise ValueError("dpmpp2m_step: out aliases state (the step reads plane 1 of state while it writes plane 1 of out)")
    api.lb_dpmpp2m_step_f16(state.data_ptr(), eps.data_ptr(), out.data_ptr(), params.data_ptr(), state[0, 0].numel(), B,
                            int(bool(cfg)), stream_ptr())
    return out


def noise_rows(rows, device) -> torch.Tensor:
    """Host rows of ``(key0, key1, ctr1, ctr2, ctr3)`` (32-bit words) -> int32 [n, 8] on ``device``, in ONE copy: the ``rows_dev``
    operand of ``lb_counter_noise_f16``."""
    import numpy as np
    host = np.zeros((len(rows), 8), dtype=np.uint32)
    if len(rows):
        host[:, :5] = np.asarray([[int(v) & 0xFFFFFFFF for v in r] for r in rows], dtype=np.uint64).reshape(len(rows), 5)
    return torch.from_numpy(host.view(np.int32)).to(device)


def counter_noise(rows, shape, raw: bool = False, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """Counter-based noise (``lb_counter_noise_f16``): ``rows`` is a host sequence of n 5-tuples ``(key0, key1, ctr1, ctr2,
    ctr3)``, uploaded in one copy - or an int32 [n, 8] device tensor ``noise_rows`` made, which a caller that records a program
    owns and keeps alive (the op reads it at every replay).  ``shape`` = (n, ...): the result is fp16 of that shape, or with
    ``raw`` int32 of that shape holding the Philox words.  ``out``: caller-owned, contiguous, 16-byte aligned."""
    shape = tuple(int(s) for s in shape)
    n = shape[0] if shape else 0
    per_sample = 1
    for s in shape[1:]:
        per_sample *= s
    dt = torch.int32 if raw else F16
    if out is not None:
        device = out.device
        if out.dtype != dt or not out.is_contiguous() or out.numel() != n * per_sample:
            raise ValueError(f"counter_noise: out must be a contiguous {dt} tensor of {n * per_sample} elements")
    elif device is None:
        device = rows.device if isinstance(rows, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    if isinstance(rows, torch.Tensor):
        if rows.dtype != torch.int32 or not rows.is_contiguous() or tuple(rows.shape) != (n, 8) or rows.device != torch.device(device):
            raise ValueError(f"counter_noise: device rows must be a contiguous int32 [{n}, 8] tensor on {device}")
        rows_dev = rows
    else:
        if len(rows) != n:
            raise ValueError(f"counter_noise: {len(rows)} rows for a result of shape {shape}")
        if n > 0:
            _own_buffer("counter_noise", "device `rows` (noise_rows)")
        rows_dev = noise_rows(rows, device)
    if out is None:
        out = torch.empty(shape, dtype=dt, device=device)
    api.lb_counter_noise_f16(rows_dev.data_ptr() if n > 0 else None, out.data_ptr() if out.numel() else None, per_sample, n,
                             int(bool(raw)), stream_ptr())
    return out


# ------------------------------------------------------------------------------ GEMM / conv
def pack_linear_weight(w: torch.Tensor) -> torch.Tensor:
    """[N, K] -> fp16 [N, K] contiguous (K padded to a multiple of 8 with zeros)."""
    n, k = w.shape
    kp = (k + 7) // 8 * 8
    out = torch.zeros(n, kp, dtype=F16, device=w.device)
    out[:, :k] = w.to(F16)
    return out


def pack_conv_weight(w: torch.Tensor, cin_pad: Optional[int] = None) -> torch.Tensor:
    """[Cout, Cin, KH, KW] -> fp16 [Cout, KH*KW*Cin_pad] with (ky, kx, cin) K order."""
    cout, cin, kh, kw = w.shape
    cp = cin_pad or (cin + 7) // 8 * 8
    out = torch.zeros(cout, kh, kw, cp, dtype=F16, device=w.device)
    out[..., :cin] = w.permute(0, 2, 3, 1).to(F16)
    return out.reshape(cout, kh * kw * cp)


def subpixel_upsample_weights(w: torch.Tensor, cin_pad: Optional[int] = None):
    """3x3 conv weight [Cout, Cin, 3, 3] applied after a nearest-2x upsample  ->  four packed 2x2 kernels
    {(py, px): fp16 [Cout, 2*2*Cin_pad]} acting on the low-res grid: output pixel (2y+py, 2x+px) sees only
    a 2x2 low-res neighbourhood, the taps that fall on the same source pixel are summed (in fp32)."""
    cout, cin, _, _ = w.shape
    cp = cin_pad or (cin + 7) // 8 * 8
    w = w.float()
    rows = {0: [w[:, :, 0], w[:, :, 1] + w[:, :, 2]], 1: [w[:, :, 0] + w[:, :, 1], w[:, :, 2]]}   # [Cout,Cin,3(kx)]
    out = {}
    for py in (0, 1):
        for px in (0, 1):
            k = torch.zeros(cout, 2, 2, cp, dtype=torch.float32, device=w.device)
            for a in (0, 1):
                r = rows[py][a]                                            # [Cout, Cin, 3]
                cols = [r[:, :, 0], r[:, :, 1] + r[:, :, 2]] if px == 0 else [r[:, :, 0] + r[:, :, 1], r[:, :, 2]]
                for b in (0, 1):
                    k[:, a, b, :cin] = cols[b]
            out[(py, px)] = k.reshape(cout, 4 * cp).to(F16).contiguous()
    return out


def gemm(A: torch.Tensor, W: torch.Tensor, bias=None, residual=None, rowvec=None, rows_per_batch=0,
         flags: int = 0, alpha: float = 1.0, out: Optional[torch.Tensor] = None, splitk_ws: bool = True,
         conv: Optional[dict] = None, M: Optional[int] = None, ln=None, ch_stats: Optional[torch.Tensor] = None,
         workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C = epilogue(A . W^T).  A: [M, K] fp16 (or NHWC [B,H,W,C] with ``conv``), W: [N, K] fp16.
    ``workspace``: caller-owned fp32 split-K slabs (>= lb_gemm_workspace_bytes(M, N) bytes) instead of a temporary one.
    ``conv``: dict(KH, KW, stride, pad, ups) for an implicit-GEMM convolution.
    ``ln`` = (colsum [N] fp32, eps): LayerNorm over A's columns folded into the GEMM (see ``fold_layernorm``)."""
    N, K = W.shape
    dev = A.device
    geom = None
    if conv is not None:
        B, H, Wd, Cin = A.shape
        geom = lib.ConvGeom(H, Wd, Cin, conv["KH"], conv["KW"], stride=conv.get("stride", 1), pad=conv.get("pad", 0),
                            ups=int(conv.get("ups", 0)), ldx=A.stride(2), parity=conv.get("parity"))
        if geom.parity is not None and out is None:
            raise ValueError("gemm: a sub-pixel upsampling conv scatters into a [B, 2H, 2W, N] `out` the caller supplies")
        Mv = geom.M(B)
        out_shape = (B, geom.Hout, geom.Wout)
    else:
        Mv = M if M is not None else A.shape[0]
        out_shape = (Mv,)
    n_out = N // 2 if flags & lib.GEMM_GEGLU else N
    if out is None:
        odt = F32 if flags & lib.GEMM_OUT_F32 else F16
        if flags & lib.GEMM_TRANS_OUT:
            out = torch.empty(n_out, Mv, dtype=odt, device=dev)
        else:
            out = torch.empty(out_shape + (n_out,), dtype=odt, device=dev)
    ws = None
    if splitk_ws and not (flags & lib.GEMM_GEGLU) and ln is None:
        ws = workspace
        if ws is None:
            _own_buffer("gemm", "split-K `workspace` (or splitk_ws=False)")
            ws = torch.empty(api.lb_gemm_workspace_bytes(Mv, N) // 4, dtype=F32, device=dev)
        assert ws.numel() * ws.element_size() >= api.lb_gemm_workspace_bytes(Mv, N), "gemm: split-K workspace too small"
    p = lib.gemm_params(
        A=A.data_ptr(), W=W.data_ptr(), C=out.data_ptr(), M=Mv, N=N, K=K, lda=A.stride(0) if conv is None else 0, ldw=W.stride(0),
        ldc=out.stride(0) if (flags & lib.GEMM_TRANS_OUT) else out.stride(-2), conv=geom, bias=_ptr(bias), residual=_ptr(residual),
        ldr=residual.stride(-2) if residual is not None else 0, rowvec=_ptr(rowvec),
        ld_rowvec=rowvec.stride(0) if rowvec is not None else 0, rows_per_batch=rows_per_batch, alpha=alpha, flags=flags,
        zero_page=zero_page(dev).data_ptr(), partial=_ptr(ws), ln=None if ln is None else (ln[0].data_ptr(), ln[1]),
        # ch_stats: halo-tile convs only, the GroupNorm statistics of the stored output, [N][B * rows][2] fp32
        ch_stats=None if ch_stats is None else (ch_stats.data_ptr(), ch_stats.shape[1]), make=LbGemmParams)
    if conv is not None and conv.get("halo"):         # experimental halo-tile 3x3 kernel (csrc/conv3_halo.hip)
        api.lb_conv3x3_halo_f16(C.byref(p), stream_ptr())
    else:
        api.lb_gemm_f16(C.byref(p), stream_ptr())
    return out


def fold_layernorm(w: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """(W', colsum, b') for ``gemm(..., ln=(colsum, eps))``: LN(x) W^T + b = rstd (x W'^T - mean colsum) + b'."""
    wf = (w.double() * gamma.double()[None, :]).to(F16)
    b2 = w.double() @ beta.double()
    if bias is not None:
        b2 = b2 + bias.double()
    return wf, wf.double().sum(dim=1).to(F32), b2.to(F32)


# ------------------------------------------------------------------------------ norms ------
def groupnorm_nhwc(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float,
                   silu: bool, ldx: Optional[int] = None, ldy: Optional[int] = None,
                   out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x: [B, H, W, C] (or [B, HW, C]) fp16 / fp32 -> fp16.  ``ldx`` / ``ldy``: pixel strides in elements (default C: dense);
    ``out``: caller-owned fp16 output whose pixels are ``ldy`` apart; ``workspace``: caller-owned float64 statistics buffer
    (lb_groupnorm_workspace_bytes(B, groups) bytes) instead of a temporary one."""
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    y = torch.empty(x.shape, dtype=F16, device=x.device) if out is None else out
    ws = _groupnorm_workspace("groupnorm_nhwc", workspace, B, groups, x.device)
    api.lb_groupnorm_nhwc(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(),
                          B, HW, C, C if ldx is None else ldx, C if ldy is None else ldy, groups, eps, int(silu),
                          int(x.dtype == F32), stream_ptr())
    return y


def _groupnorm_workspace(wrapper: str, workspace: Optional[torch.Tensor], B: int, groups: int, device) -> torch.Tensor:
    nbytes = api.lb_groupnorm_workspace_bytes(B, groups)
    if workspace is None:
        _own_buffer(wrapper, "`workspace`")
        return torch.empty(nbytes // 8, dtype=F64, device=device)
    assert workspace.numel() * workspace.element_size() >= nbytes, f"{wrapper}: workspace too small"
    return workspace


def conv_halo_plan(B: int, H: int, W: int, cin: int, cout: int, ks: int = 3, flags: int = 0):
    """(kind, tile width, work items, grid) of the halo-tile kernel for this conv geometry (kind 0: not eligible).
    ``flags``: ``lib.GEMM_HALO_RAGGED`` asks for the ragged-tile plan of a 3x3 conv."""
    p = lib.conv_probe(B, H, W, cin, cout, ks, flags)
    kind, tw, items, grid = C.c_int(), C.c_int(), C.c_long(), C.c_long()
    api.lb_conv_halo_plan(C.byref(p), C.byref(kind), C.byref(tw), C.byref(items), C.byref(grid))
    return kind.value, tw.value, items.value, grid.value


def conv_ch_stat_rows(B: int, H: int, W: int, cin: int, cout: int, ks: int = 3, flags: int = 0) -> int:
    """Row blocks per sample of the LB_GEMM_CH_STATS buffer a 3x3 conv (ks = 3) / one-launch sub-pixel upsampler conv (ks = 2) of
    this geometry writes when ``gemm`` launches it (lb_gemm_ch_stat_rows: the library's own routing and tile constants); 0 = it
    does not run on a halo-tile kernel.  ``flags``: ``lib.GEMM_HALO_RAGGED`` for the ragged-tile launch."""
    p = lib.conv_probe(B, H, W, cin, cout, ks, flags)
    return int(api.lb_gemm_ch_stat_rows(C.byref(p)))


def groupnorm_from_stats(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool,
                         ch_stats: torch.Tensor, rows_per_sample: int, ldx: Optional[int] = None, ldy: Optional[int] = None,
                         out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GroupNorm of x [B, H, W, C] whose (sum, sum of squares) per (64-pixel row block, channel) the producing conv left in
    ``ch_stats`` ([C, B * rows_per_sample, 2] fp32, channel-major, LB_GEMM_CH_STATS).  ``ldx`` / ``ldy`` / ``out`` as in
    ``groupnorm_nhwc``; ``workspace`` likewise."""
    B, C_ = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C_)
    y = torch.empty(x.shape, dtype=F16, device=x.device) if out is None else out
    ws = _groupnorm_workspace("groupnorm_from_stats", workspace, B, groups, x.device)
    api.lb_groupnorm_from_stats(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ch_stats.data_ptr(), ws.data_ptr(),
                                B, HW, C_, C_ if ldx is None else ldx, C_ if ldy is None else ldy, groups, eps, int(silu),
                                int(x.dtype == F32), rows_per_sample, stream_ptr())
    return y


def groupnorm_affine_from_stats(gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, ch_stats: torch.Tensor,
                                rows_per_sample: int, B: int, HW: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The GroupNorm ``groupnorm_from_stats`` would apply, as a table [B, C, 2] fp32 of (scale, shift) per (sample, channel):
    y = x * scale + shift.  The operand of a conv flagged ``lib.GEMM_GN_A`` (``gn_table``); x itself is not read."""
    C_ = gamma.numel()
    table = torch.empty(B, C_, 2, dtype=F32, device=gamma.device) if out is None else out
    api.lb_groupnorm_affine_from_stats(ch_stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), table.data_ptr(), B, HW, C_, groups,
                                       eps, rows_per_sample, stream_ptr())
    return table


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    M, Cc = x.shape
    y = torch.empty_like(x)
    api.lb_layernorm_f16(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), M, Cc,
                         x.stride(0), y.stride(0), eps, stream_ptr())
    return y


# ------------------------------------------------------------------------------ attention --
_ZERO_PAGES = {}


def zero_page(device) -> torch.Tensor:
    """64 zero bytes per device: the source of masked direct-to-LDS loads (GEMM tails, attention rows >= Skv)."""
    key = str(device)
    if key not in _ZERO_PAGES:
        _ZERO_PAGES[key] = torch.zeros(64, dtype=torch.uint8, device=device)
    return _ZERO_PAGES[key]


def attention_d64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, H: int, Sq: int, Skv: int,
                  skv_valid: Optional[int] = None, ldq=None, ldk=None, ldv=None,
                  out: Optional[torch.Tensor] = None, causal: bool = False) -> torch.Tensor:
    """q: [B*Sq, >=H*64], k, v: [B*Skv, >=H*64] (row strides may exceed widths: slices of a fused QKV buffer)."""
    p = LbAttnParams()
    if out is None:
        out = torch.empty(B * Sq, H * 64, dtype=F16, device=q.device)
    p.Q, p.K, p.V, p.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    p.B, p.H, p.Sq, p.Skv, p.Skv_valid = B, H, Sq, Skv, skv_valid or Skv
    p.ldq, p.ldk, p.ldv, p.ldo = ldq or q.stride(0), ldk or k.stride(0), ldv or v.stride(0), out.stride(0)
    p.scale = 0.125
    p.causal = int(causal)
    p.zero_page = zero_page(q.device).data_ptr()
    api.lb_attn_fwd_d64(C.byref(p), stream_ptr())
    return out


def attention_d512(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, H: int, Sq: int, Skv: int,
                   skv_valid: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Head dim 512 (the VAE mid-block attention): q [B*Sq, >=H*512], k, v [B*Skv, >=H*512]; one launch, no S x S buffer."""
    p = LbAttnParams()
    if out is None:
        out = torch.empty(B * Sq, H * 512, dtype=F16, device=q.device)
    p.Q, p.K, p.V, p.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    p.B, p.H, p.Sq, p.Skv, p.Skv_valid = B, H, Sq, Skv, skv_valid or Skv
    p.ldq, p.ldk, p.ldv, p.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    p.scale = 512.0 ** -0.5
    p.causal = 0
    p.zero_page = zero_page(q.device).data_ptr()
    api.lb_attn_fwd_d512(C.byref(p), stream_ptr())
    return out


def softmax_rows_(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    M, N = x.shape
    api.lb_softmax_rows_f16(x.data_ptr(), M, N, x.stride(0), scale, stream_ptr())
    return x


# ------------------------------------------------------------------------------ small ------
def sinusoid(vals: torch.Tensor, dim: int, out: Optional[torch.Tensor] = None, col_off: int = 0) -> torch.Tensor:
    """vals: float32 [rows, per_row] on device -> fp16 [rows, per_row*dim] ([cos|sin] per value)."""
    rows, per_row = vals.shape
    if out is None:
        out = torch.empty(rows, per_row * dim, dtype=F16, device=vals.device)
    api.lb_sinusoid_f16(vals.data_ptr(), rows, per_row, vals.stride(0), dim, out.data_ptr(), out.stride(0),
                        col_off, stream_ptr())
    return out


def copy_cols(src: torch.Tensor, dst: torch.Tensor, dst_off: int):
    rows = src.numel() // src.shape[-1]
    api.lb_copy_cols_f16(src.data_ptr(), dst.data_ptr(), rows, src.shape[-1], src.stride(-2), dst.stride(-2),
                         dst_off, stream_ptr())


def nchw_to_nhwc(x: torch.Tensor, ld: int, mul: float = 1.0) -> torch.Tensor:
    B, Cc, H, W = x.shape
    y = torch.empty(B, H, W, ld, dtype=F16, device=x.device)
    x = _operand("nchw_to_nhwc", x, x.contiguous())
    api.lb_nchw_to_nhwc_f16(x.data_ptr(), y.data_ptr(), B, Cc, H * W, ld, mul, stream_ptr())
    return y


def nhwc_to_nchw(x: torch.Tensor, channels: int) -> torch.Tensor:
    B, H, W, ld = x.shape
    y = torch.empty(B, channels, H, W, dtype=F16, device=x.device)
    api.lb_nhwc_to_nchw_f16(x.data_ptr(), y.data_ptr(), B, channels, H * W, ld, stream_ptr())
    return y


def postprocess_u8(x: torch.Tensor) -> torch.Tensor:
    """x: [B, H, W, ld>=3] fp16/fp32 -> uint8 [B, H, W, 3]."""
    B, H, W, ld = x.shape
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=x.device)
    api.lb_postprocess_u8(x.data_ptr(), out.data_ptr(), B * H * W, ld, int(x.dtype == F32), stream_ptr())
    return out


def maxpool3s2(x: torch.Tensor) -> torch.Tensor:
    N, H, W, Cc = x.shape
    y = torch.empty(N, (H - 3) // 2 + 1, (W - 3) // 2 + 1, Cc, dtype=F16, device=x.device)
    api.lb_maxpool3s2_nhwc_f16(x.data_ptr(), y.data_ptr(), N, H, W, Cc, stream_ptr())
    return y


def frames_lerp_u8(frames: torch.Tensor, left, weights, out: Optional[torch.Tensor] = None, tables=None) -> torch.Tensor:
    """frames: [n_key, H, W, 3] uint8 on the device; out[k] = uint8((1 - w[k]) * frames[left[k]] + w[k] * frames[left[k] + 1])
    in float64 with a truncating cast (reference utils.py:97 as numpy >= 2 evaluates it on the movie's key frames).
    ``tables`` = (left int32 [n_out], weights float64 [n_out]) already on the device, caller-owned, instead of an upload of
    ``left`` / ``weights`` (which then only give the count)."""
    assert frames.dtype == torch.uint8 and frames.is_contiguous()
    n_out = len(left)
    fb = frames[0].numel()
    if tables is None:
        _own_buffer("frames_lerp_u8", "`tables` (left, weights) on the device")
        left_d = torch.tensor(list(left), dtype=torch.int32, device=frames.device)
        w_d = torch.tensor(list(weights), dtype=F64, device=frames.device)
    else:
        left_d, w_d = tables
        assert left_d.dtype == torch.int32 and w_d.dtype == F64 and left_d.numel() >= n_out and w_d.numel() >= n_out
    if out is None:
        out = torch.empty((n_out,) + tuple(frames.shape[1:]), dtype=torch.uint8, device=frames.device)
    for k0 in range(0, n_out, 65535):
        k1 = min(n_out, k0 + 65535)
        api.lb_frames_lerp_u8(frames.data_ptr(), left_d[k0:].data_ptr(), w_d[k0:].data_ptr(), out[k0:].data_ptr(), k1 - k0, fb,
                              stream_ptr())
    return out


def cast_f16_to_f32(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert x.dtype == F16 and x.is_contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=F32, device=x.device)
    api.lb_cast_f16_to_f32(x.data_ptr(), out.data_ptr(), x.numel(), stream_ptr())
    return out


def cast_f32_to_f16(x: torch.Tensor, mul: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp16(saturate(x * mul)): values beyond the fp16 range (+-inf included) come back as +-65504, a NaN stays a NaN."""
    assert x.dtype == F32 and x.is_contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=F16, device=x.device)
    api.lb_cast_f32_to_f16(x.data_ptr(), out.data_ptr(), x.numel(), float(mul), stream_ptr())
    return out


def fill_f32_(x: torch.Tensor, value: float) -> torch.Tensor:
    assert x.dtype == F32 and x.is_contiguous()
    api.lb_fill_f32(x.data_ptr(), x.numel(), float(value), stream_ptr())
    return x


def lpips_prep_u8(img: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """img: [..., 3] uint8 -> fp16 [..., 8]: the LPIPS scaling layer on 2 x / 255 - 1, channels 3..7 zero."""
    assert img.dtype == torch.uint8 and img.is_contiguous() and img.shape[-1] == 3
    if out is None:
        out = torch.empty(tuple(img.shape[:-1]) + (8,), dtype=F16, device=img.device)
    api.lb_lpips_prep_u8(img.data_ptr(), out.data_ptr(), img.numel() // 3, stream_ptr())
    return out


def lpips_tap(feats_a: Sequence[torch.Tensor], feats_b: Sequence[torch.Tensor], lin: torch.Tensor, acc: torch.Tensor,
              workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """acc[pair] += mean over pixels of sum_c lin[c] * (a / (|a| + eps) - b / (|b| + eps))^2 for up to 16 pairs of [HW, C] fp16
    features; ``acc``: fp32, at least one slot per pair, zeroed by the caller before the first tap."""
    assert len(feats_a) == len(feats_b) and 0 < len(feats_a) <= 16 and acc.dtype == F32 and acc.numel() >= len(feats_a)
    hw, c = feats_a[0].shape[-2], feats_a[0].shape[-1]
    assert all(t.dtype == F16 and t.is_contiguous() and t.shape[-2:] == (hw, c) for t in list(feats_a) + list(feats_b))
    if workspace is None:
        _own_buffer("lpips_tap", "`workspace`")
        workspace = torch.empty(16 * 128, dtype=F32, device=acc.device)
    pa, keep_a = _ptr_array(feats_a)
    pb, keep_b = _ptr_array(feats_b)
    api.lb_lpips_tap(pa, pb, lin.data_ptr(), acc.data_ptr(), workspace.data_ptr(), len(feats_a), hw, c, stream_ptr())
    return acc


def embed_tokens(ids: torch.Tensor, tok_emb: torch.Tensor, pos_emb: torch.Tensor, seq: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = tok_emb[clamp(ids[r], 0, vocab - 1)] + pos_emb[r % seq] (CLIPTextEmbeddings); ids: int32 [rows]."""
    assert ids.dtype == torch.int32 and tok_emb.dtype == F16 and pos_emb.dtype == F16
    assert tok_emb.is_contiguous() and pos_emb.is_contiguous() and pos_emb.shape[0] >= seq
    rows, (vocab, c) = ids.numel(), tok_emb.shape
    if out is None:
        out = torch.empty(rows, c, dtype=F16, device=ids.device)
    api.lb_embed_tokens_f16(ids.data_ptr(), tok_emb.data_ptr(), pos_emb.data_ptr(), out.data_ptr(), rows, seq, c, vocab,
                            stream_ptr())
    return out


def gather_rows(src: torch.Tensor, rows_idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = src[rows_idx[i]]; src: fp16 [rows, C] whose rows may be further apart than C; rows_idx: int32."""
    assert src.dtype == F16 and rows_idx.dtype == torch.int32 and src.stride(1) == 1
    n, c = rows_idx.numel(), src.shape[1]
    if out is None:
        out = torch.empty(n, c, dtype=F16, device=src.device)
    api.lb_gather_rows_f16(src.data_ptr(), rows_idx.data_ptr(), out.data_ptr(), n, c, src.stride(0), stream_ptr())
    return out


# -------------------------------------------------------------------------- movie frames -----
_JPEG_WORKSPACE_BUDGET = 1 << 30        # bytes of entropy-coder workspace per chunk of frames (slots are sized for the worst case)
_JPEG_QTABLES: dict = {}
_JPEG_PINNED: dict = {}


def _jpeg_qtables(quality: int, device) -> torch.Tensor:
    """[2][64] uint16 on the device, natural order (one upload per quality and device)."""
    key = (int(quality), str(device))
    if key not in _JPEG_QTABLES:
        from ..jpeg import jpeg_tables
        _JPEG_QTABLES[key] = torch.tensor(jpeg_tables(quality), dtype=torch.int16).to(device)      # values <= 255
    return _JPEG_QTABLES[key]


def _jpeg_frames(frames_u8: torch.Tensor):
    assert frames_u8.dtype == torch.uint8 and frames_u8.is_cuda and frames_u8.dim() == 4 and frames_u8.shape[-1] == 3, \
        "jpeg: [n, H, W, 3] uint8 frames on the device"
    frames_u8 = frames_u8.contiguous()
    n, h, w, _ = frames_u8.shape
    return frames_u8, n, h, w


def jpeg_dct_quant_into(frames_u8: torch.Tensor, qtables: torch.Tensor, coef: torch.Tensor, subsampling_code: int) -> None:
    """Stage 1 launcher on caller-owned buffers (capturable)."""
    n, h, w, _ = frames_u8.shape
    api.lb_jpeg_dct_quant_u8(frames_u8.data_ptr(), qtables.data_ptr(), coef.data_ptr(), n, h, w, subsampling_code, stream_ptr())


def jpeg_entropy_into(coef: torch.Tensor, workspace: torch.Tensor, out: torch.Tensor, frame_bytes: torch.Tensor, n: int, h: int,
                      w: int, subsampling_code: int) -> None:
    """Stage 2 launcher (entropy coding, scan, compaction) on caller-owned buffers (capturable)."""
    api.lb_jpeg_entropy(coef.data_ptr(), workspace.data_ptr(), out.data_ptr(), out.numel(), frame_bytes.data_ptr(), n, h, w,
                        subsampling_code, stream_ptr())


def jpeg_coefficients_u8(frames_u8: torch.Tensor, quality: int = 92, subsampling: str = "4:2:0") -> torch.Tensor:
    """Quantised DCT coefficients of [n, H, W, 3] uint8 device frames: int16 [n, blocks, 64] - per frame the Y, Cb, Cr planes
    (whole MCUs), blocks in raster order, zigzag order inside a block."""
    from ..jpeg import subsampling_code
    code = subsampling_code(subsampling)
    frames_u8, n, h, w = _jpeg_frames(frames_u8)
    count = api.lb_jpeg_coefficient_count(n, h, w, code)
    coef = torch.empty((n, max(count, 0) // (64 * n), 64), dtype=torch.int16, device=frames_u8.device)
    jpeg_dct_quant_into(frames_u8, _jpeg_qtables(quality, frames_u8.device), coef, code)      # (raises for an unsupported size)
    return coef


def _jpeg_to_host(t: torch.Tensor, nbytes: int):
    """memoryview of the first nbytes of a uint8 device tensor, through one page-locked staging buffer that grows on demand."""
    key = t.device.index
    pinned = _JPEG_PINNED.get(key)
    if pinned is None or pinned.numel() < nbytes:
        pinned = _JPEG_PINNED[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
    pinned[:nbytes].copy_(t[:nbytes], non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return memoryview(pinned.numpy())[:nbytes]


def jpeg_scan_from_coefficients(coef: torch.Tensor, h: int, w: int, subsampling: str = "4:2:0") -> List[bytes]:
    """Entropy-coded scan data (restart markers in place, no header, no EOI) of every frame of a stage-1 tensor."""
    from ..jpeg import subsampling_code
    code = subsampling_code(subsampling)
    n = coef.shape[0]
    assert coef.dtype == torch.int16 and coef.is_cuda and coef.is_contiguous()
    assert coef.numel() == api.lb_jpeg_coefficient_count(n, h, w, code), "jpeg: coefficient tensor does not match (n, H, W, subsampling)"
    dev = coef.device
    _own_buffer("jpeg_scan_from_coefficients", "workspace (use jpeg_entropy_into)")
    workspace = torch.empty(api.lb_jpeg_workspace_bytes(n, h, w, code), dtype=torch.uint8, device=dev)
    frame_bytes = torch.empty(n, dtype=torch.int32, device=dev)
    capacity = n * (h * w + 4096)                  # ~3x what quality 92 needs on noisy frames; the true sizes come back either way
    while True:
        out = torch.empty(capacity, dtype=torch.uint8, device=dev)
        jpeg_entropy_into(coef, workspace, out, frame_bytes, n, h, w, code)
        sizes = frame_bytes.cpu().tolist()
        total = sum(sizes)
        if total <= capacity:
            break
        capacity = total                           # (rare: quality ~100 on noise) once more with the exact size
    host = _jpeg_to_host(out, total)
    scans, pos = [], 0
    for s in sizes:
        scans.append(bytes(host[pos:pos + s]))
        pos += s
    return scans


def jpeg_encode_u8(frames_u8: torch.Tensor, quality: int = 92, subsampling: str = "4:2:0") -> List[bytes]:
    """Complete baseline JPEG files (header + scan + EOI) of [n, H, W, 3] uint8 device frames, encoded on the device in chunks of
    frames; only the compressed bytes are copied to the host.  Raises RuntimeError for a size the kernels do not take."""
    from ..jpeg import EOI, jpeg_header, subsampling_code
    code = subsampling_code(subsampling)
    frames_u8, n, h, w = _jpeg_frames(frames_u8)
    per_frame = api.lb_jpeg_workspace_bytes(1, h, w, code)
    if per_frame <= 0:
        raise RuntimeError(f"jpeg_encode_u8: unsupported frame size {h} x {w} (height and width must be multiples of 8)")
    header = jpeg_header(h, w, int(quality), subsampling)
    chunk = max(1, min(n, 1024, _JPEG_WORKSPACE_BUDGET // per_frame))
    out: List[bytes] = []
    for k0 in range(0, n, chunk):
        part = frames_u8[k0:k0 + chunk]
        coef = jpeg_coefficients_u8(part, quality, subsampling)
        out.extend(b"".join((header, scan, EOI)) for scan in jpeg_scan_from_coefficients(coef, h, w, subsampling))
    return out


_RESAMPLE_TABLES: dict = {}


def _resample_tables(hin: int, win: int, hout: int, wout: int, filter: str, device):
    """((start, count, coef, kmax) for x, the same for y) on the device; None for an axis that keeps its size.  One upload per
    (sizes, filter, device)."""
    key = (hin, win, hout, wout, filter, str(device))
    if key not in _RESAMPLE_TABLES:
        from ..resample import resample_tables

        def axis(size_in, size_out):
            if size_in == size_out:
                return None
            start, count, coef = resample_tables(size_in, size_out, filter)
            return (torch.from_numpy(start).to(device), torch.from_numpy(count).to(device),
                    torch.from_numpy(coef).contiguous().to(device), int(coef.shape[1]))
        _RESAMPLE_TABLES[key] = (axis(win, wout), axis(hin, hout))
    return _RESAMPLE_TABLES[key]


def resample_u8_into(frames: torch.Tensor, tmp: Optional[torch.Tensor], out: torch.Tensor, tables_x, tables_y) -> None:
    """The launcher on caller-owned buffers (capturable): frames [n, Hin, Win, 3] -> out [n, Hout, Wout, 3] through tmp
    [n, Hin, Wout, 3]; ``tables_*`` = (start, count, coef, kmax) on the device, None for an axis that keeps its size (tmp may be
    None unless both axes change).  At most 65535 frames."""
    n, hin, win, _ = frames.shape
    hout, wout = out.shape[1:3]
    sx, cx, kx, kmx = tables_x if tables_x is not None else (None, None, None, 0)
    sy, cy, ky, kmy = tables_y if tables_y is not None else (None, None, None, 0)
    api.lb_resample_u8(frames.data_ptr(), _ptr(tmp), out.data_ptr(), n, hin, win, hout, wout, _ptr(sx), _ptr(cx), _ptr(kx), kmx,
                       _ptr(sy), _ptr(cy), _ptr(ky), kmy, stream_ptr())


def resample_u8(frames: torch.Tensor, size_hw, filter: str = "bicubic", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n, Hin, Win, 3] uint8 device frames resized to ``size_hw = (Hout, Wout)``: Pillow's ``Image.resize`` with ``filter``
    ("box", "bilinear", "bicubic", "lanczos") and ``reducing_gap=None``, byte for byte."""
    from ..resample import check_filter, check_size
    check_filter(filter)
    hout, wout = check_size(size_hw, "size_hw")
    assert frames.dtype == torch.uint8 and frames.is_cuda and frames.dim() == 4 and frames.shape[-1] == 3, \
        "resample_u8: [n, H, W, 3] uint8 frames on the device"
    frames = frames.contiguous()
    n, hin, win, _ = frames.shape
    dev = frames.device
    if out is None:
        out = torch.empty((n, hout, wout, 3), dtype=torch.uint8, device=dev)
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (n, hout, wout, 3) and out.device == dev
    tx, ty = _resample_tables(hin, win, hout, wout, filter, dev)
    chunk = min(n, 65535)
    if tx is not None and ty is not None:
        _own_buffer("resample_u8", "`tmp` (use resample_u8_into)")
    tmp = torch.empty((chunk, hin, wout, 3), dtype=torch.uint8, device=dev) if tx is not None and ty is not None else None
    for k0 in range(0, n, 65535):
        k1 = min(n, k0 + 65535)
        resample_u8_into(frames[k0:k1], None if tmp is None else tmp[:k1 - k0], out[k0:k1], tx, ty)
    return out
