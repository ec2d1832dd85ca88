"""Shared by the tests of the K-split form of the 3x3 halo-tile conv (LB_GEMM_HALO_KSPLIT): the shapes with their forced grids, the
parameter builder, the two entry points, the switch fixture and the guarded workspace.

Flagged launches are built here and never through ops.gemm: that helper hands its split-K slabs to ``partial``, which a flagged halo
launch reads as its counters."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from _guard import guarded
from _parity import rnd

DEV = "cuda"
F16, F32 = torch.float16, torch.float32
SLAB_BYTES = 256 * 128 * 4

# name -> (B, H, W, Cin, N, forced grid; 0 = the default grid, one block per CU)
SHAPES = {
    "tail_whole_whole": (4, 16, 32, 128, 128, 3),      # 16 units over 3 blocks: block 0 ends, block 1 starts inside tile 2
    "tail_whole_head": (4, 16, 32, 192, 128, 5),       # block 3: the tail of one tile, a whole tile, the head of the next
    "three_sharers": (1, 32, 16, 320, 132, 7),         # a tile shared by three blocks; the last channel block overhangs N
    "tile_boundaries": (2, 16, 16, 192, 256, 4),       # ranges end on tile boundaries: no partial sums; two channel blocks
    "one_unit_per_block": (1, 16, 16, 1280, 128, 20),  # one tile, 20 units, 20 blocks: 20 contributors, c_lo = c, c_end = c + 1 in each
    "default_grid": (4, 32, 32, 1280, 256, 0),         # 640 units on the default grid: more units than CUs
}
ALPHA = 0.5


def lib():
    from latentblending_amd.hip import lib as l
    return l


def stream():
    return torch.cuda.current_stream().cuda_stream


def nhwc_dev(x_nhwc, ldx=None):
    """CPU [B, H, W, Cin] -> the device operand: contiguous, or (``ldx``) rows of ldx elements inside a guarded buffer whose pad
    columns hold NaN sentinels -> (tensor [B, H, W, Cin], GuardChecker or None)."""
    if ldx is None:
        return x_nhwc.contiguous().to(DEV), None
    B, H, W, cin = x_nhwc.shape
    view, guard = guarded(B * H * W, cin, ldx, x_nhwc.dtype, DEV)
    view.copy_(x_nhwc.reshape(B * H * W, cin))
    return view.as_strided((B, H, W, cin), (H * W * ldx, W * ldx, ldx, 1)), guard


def conv_params(x, w, out, *, bias=None, residual=None, rowvec=None, alpha=1.0, flags=0, stats=None, ksplit=False, ws=None, stride=1,
                zero=None):
    """LbGemmParams of a 3x3 / pad 1 conv: x [B, H, W, Cin] fp16 on the device (pixel stride = ldx), w the packed [N, 9 Cin] weight,
    out [M, N] (row stride = ldc; fp32 with LB_GEMM_OUT_F32 in ``flags``), residual [M, N] (row stride = ldr; fp32 with
    LB_GEMM_RES_F32), rowvec [B, N].  ``ksplit``: flag the launch and hand it ``ws`` (a tensor, or None = no workspace)."""
    from latentblending_amd.hip import ops as o
    l = lib()
    B, H, W, Cin = x.shape
    N = w.shape[0]
    g = l.ConvGeom.conv3x3(H, W, Cin, stride=stride, ldx=x.stride(2))
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    return l.gemm_params(
        A=x.data_ptr(), W=w.data_ptr(), C=out.data_ptr(), M=g.M(B), N=N, K=g.K, ldw=w.stride(0), ldc=out.stride(0), conv=g,
        bias=ptr(bias), residual=ptr(residual), ldr=N if residual is None else residual.stride(0), rowvec=ptr(rowvec),
        ld_rowvec=0 if rowvec is None else rowvec.stride(0), rows_per_batch=g.Hout * g.Wout, alpha=alpha,
        flags=flags | (l.GEMM_HALO_KSPLIT if ksplit else 0), zero_page=(o.zero_page(DEV) if zero is None else zero).data_ptr(),
        partial=ptr(ws) if ksplit else None, ch_stats=None if stats is None else (stats.data_ptr(), stats.shape[1]))


@functools.lru_cache(maxsize=None)
def operands(shape):
    """Inputs on the device and the fp32 conv2d of every epilogue, computed once per shape and never modified."""
    from latentblending_amd.hip import ops as o
    B, H, W, Cin, N, _ = SHAPES[shape]
    x = rnd(B, Cin, H, W, seed=301)
    w = rnd(N, Cin, 3, 3, seed=302, scale=(9 * Cin) ** -0.5)
    bias = rnd(N, seed=303, dtype=F32)
    res = rnd(B, H, W, N, seed=304)
    rowvec = rnd(B, N, seed=305)
    raw = F.conv2d(x.float(), w.float(), None, padding=1).permute(0, 2, 3, 1)
    conv = raw + bias                                   # (the epilogue: alpha * sum + bias [+ residual | + row vector])
    refs = {"plain": conv, "stats": conv, "res": ALPHA * raw + bias + res.float(), "rowvec": conv + rowvec.float()[:, None, None, :]}
    dev = dict(x=x.permute(0, 2, 3, 1).contiguous().to(DEV), w=o.pack_conv_weight(w, Cin).to(DEV), bias=bias.to(DEV), res=res.to(DEV),
               rowvec=rowvec.to(DEV), zero=o.zero_page(DEV))
    return dev, refs


def params(shape, epi, out, ksplit, ws=None, stats=None):
    """The launch of ``operands(shape)`` with epilogue ``epi``: plain / stats = bias only, res = bias + fp16 residual + alpha,
    rowvec = bias + row vector."""
    B, H, W, Cin, N, _ = SHAPES[shape]
    d, _ = operands(shape)
    return conv_params(d["x"], d["w"], out, bias=d["bias"], residual=d["res"].view(B * H * W, N) if epi == "res" else None,
                       rowvec=d["rowvec"] if epi == "rowvec" else None, alpha=ALPHA if epi == "res" else 1.0, stats=stats,
                       ksplit=ksplit, ws=ws, zero=d["zero"])


def launch(p, entry="halo"):
    """``halo``: lb_conv3x3_halo_f16 directly; ``gemm``: through the router lb_gemm_f16, as the emitter does."""
    api = lib().api
    (api.lb_conv3x3_halo_f16 if entry == "halo" else api.lb_gemm_f16)(C.byref(p), stream())


def ksplit_plan(p):
    units, grid, split = C.c_long(), C.c_long(), C.c_int()
    lib().api.lb_conv_halo_ksplit_plan(C.byref(p), C.byref(units), C.byref(grid), C.byref(split))
    return units.value, grid.value, split.value


def guarded_workspace(p):
    """The workspace the header asks for, for the flagged params ``p`` under the current switch: lb_conv_halo_ksplit_workspace_bytes
    bytes between guard bands, the counters zeroed, the slabs left as NaN sentinels -> (ws [1, floats], GuardChecker, counter floats)."""
    need = lib().api.lb_conv_halo_ksplit_workspace_bytes(C.byref(p))
    _, grid, split = ksplit_plan(p)
    assert split == 1 and need > 2 * grid * SLAB_BYTES and need % 4 == 0, "the launch does not split"
    counter_floats = (need - 2 * grid * SLAB_BYTES) // 4
    ws, ws_guard = guarded(1, need // 4, need // 4, F32, DEV, back_rows=0)
    ws[0, :counter_floats] = 0
    return ws, ws_guard, counter_floats


def counters_zero(ws, counter_floats):
    return int(ws[0, :counter_floats].view(torch.int32).abs().max()) == 0


def run_conv(x, w, *, split=True, ws=None, out=None, entry="halo", **kw):
    """One launch of conv_params(x, w, out, **kw) -> out ([M, N], NaN-filled beforehand unless given).  ``split``: flagged, on ``ws``
    (as guarded_workspace returns it) or on a fresh guarded workspace of its own, which is then checked after the launch: guard
    bands intact, counters zero."""
    B, H, W, _ = x.shape
    stride = kw.get("stride", 1)
    M, N = B * ((H - 1) // stride + 1) * ((W - 1) // stride + 1), w.shape[0]
    if out is None:
        out = torch.full((M, N), float("nan"), dtype=F32 if kw.get("flags", 0) & lib().GEMM_OUT_F32 else F16, device=DEV)
    if not split:
        launch(conv_params(x, w, out, **kw), entry)
        return out
    own = ws is None
    if own:
        ws, guard, counter_floats = guarded_workspace(conv_params(x, w, out, ksplit=True, **kw))
    launch(conv_params(x, w, out, ksplit=True, ws=ws[0], **kw), entry)
    if own:
        torch.cuda.synchronize()
        guard.assert_intact("K-split workspace")
        assert counters_zero(ws, counter_floats), "the kernel must leave its counters zero"
    return out


@pytest.fixture
def forced_split():
    """mode 2 ("always") with the case's grid for the whole test - recorded ops read the switch when they are replayed."""
    api = lib().api

    def force(shape):
        api.lb_conv_halo_set_ksplit(2, SHAPES[shape][5])
    yield force
    api.lb_conv_halo_set_ksplit(1, 0)
