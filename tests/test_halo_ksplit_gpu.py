"""K-split form of the 3x3 halo-tile conv (LB_GEMM_HALO_KSPLIT, csrc/conv3_halo.hip) on the GPU: tiny shapes under mode 2 with a forced
small grid, so that every path of the in-launch reduction runs - a block whose range starts and ends inside tiles, a tile shared by
three blocks, ranges that end on tile boundaries (no reduction at all), an overhanging channel block - with every epilogue the UNet
uses.  tests/test_halo_ksplit_cpu.py checks that the walks of these cases have those features.

Per case: the result (and the channel statistics) against F.conv2d in fp32 under the bar of test_conv3x3_halo_against_conv2d; ten
launches bit-equal; slabs that start out as NaN never reach the result; guard bands around output and workspace intact; counters zero
afterwards; eager = recorded replay = graph launch bit for bit.  The distance to the unsplit kernel is logged, not gated: fp32
re-association of the chunk sums."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _guard import guarded  # noqa: E402
from _parity import check_close, rnd  # noqa: E402

DEV = "cuda"
F16, F32 = torch.float16, torch.float32

# name -> (B, H, W, Cin, N, forced grid)
SHAPES = {
    "tail_whole_whole": (4, 16, 32, 128, 128, 3),      # 16 units over 3 blocks: block 0 ends, block 1 starts inside tile 2
    "tail_whole_head": (4, 16, 32, 192, 128, 5),       # block 3: the tail of one tile, a whole tile, the head of the next
    "three_sharers": (1, 32, 16, 320, 132, 7),         # a tile shared by three blocks; the last channel block overhangs N
    "tile_boundaries": (2, 16, 16, 192, 256, 4),       # ranges end on tile boundaries: no partial sums; two channel blocks
}
# (shape, epilogue): plain = bias only; res = bias + fp16 residual + alpha; rowvec = bias + time-embedding row vector; stats = bias +
# LB_GEMM_CH_STATS
CASES = [("tail_whole_whole", "plain"), ("tail_whole_head", "plain"), ("three_sharers", "plain"), ("tile_boundaries", "plain"),
         ("tail_whole_whole", "res"), ("tail_whole_whole", "rowvec"), ("tail_whole_whole", "stats"), ("tile_boundaries", "stats"),
         ("three_sharers", "stats")]
ALPHA = 0.5


def lib():
    from latentblending_amd.hip import lib as l
    return l


def stream():
    return torch.cuda.current_stream().cuda_stream


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
    l = lib()
    B, H, W, Cin, N, _ = SHAPES[shape]
    d, _ = operands(shape)
    p = l.LbGemmParams()
    p.A, p.W, p.C, p.bias = d["x"].data_ptr(), d["w"].data_ptr(), out.data_ptr(), d["bias"].data_ptr()
    p.M, p.N, p.K, p.ldw, p.ldc, p.ldr = B * H * W, N, 9 * Cin, d["w"].stride(0), out.stride(0), N
    p.conv, p.Hin, p.Hout, p.Win, p.Wout = 1, H, H, W, W
    p.Cin, p.KH, p.KW, p.stride, p.pad, p.ldx = Cin, 3, 3, 1, 1, Cin
    p.alpha, p.zero_page = 1.0, d["zero"].data_ptr()
    if epi == "res":
        p.residual, p.alpha = d["res"].data_ptr(), ALPHA
    if epi == "rowvec":
        p.rowvec, p.ld_rowvec, p.rows_per_batch = d["rowvec"].data_ptr(), N, H * W
    if stats is not None:
        p.flags |= l.GEMM_CH_STATS
        p.ch_stats, p.ch_stats_rows = stats.data_ptr(), stats.shape[1]
    if ksplit:
        p.flags |= l.GEMM_HALO_KSPLIT
        p.partial = ws.data_ptr() if ws is not None else None
    return p


def launch(p):
    lib().api.lb_conv3x3_halo_f16(C.byref(p), stream())


@pytest.fixture
def forced_split():
    """mode 2 ("always") with the case's grid for the whole test - recorded ops read the switch when they are replayed."""
    api = lib().api

    def force(shape):
        api.lb_conv_halo_set_ksplit(2, SHAPES[shape][5])
    yield force
    api.lb_conv_halo_set_ksplit(1, 0)


@pytest.mark.parametrize("shape,epi", CASES)
def test_ksplit_conv(shape, epi, forced_split, results_log):
    from latentblending_amd.native.runtime import Program
    l = lib()
    B, H, W, Cin, N, G = SHAPES[shape]
    M, name = B * H * W, f"halo_ksplit_{shape}_{epi}"
    _, refs = operands(shape)
    forced_split(shape)
    with_stats = epi == "stats"
    stat_rows = M // 256 * 4

    def fresh_stats():
        return torch.full((N, stat_rows, 2), float("nan"), dtype=F32, device=DEV) if with_stats else None

    # ---- the plan splits, the workspace is what the header says: counters (zeroed), then slabs (left as NaN sentinels)
    probe = params(shape, epi, torch.empty(1, N, dtype=F16, device=DEV), True, stats=fresh_stats())
    units, grid, split = C.c_long(), C.c_long(), C.c_int()
    l.api.lb_conv_halo_ksplit_plan(C.byref(probe), C.byref(units), C.byref(grid), C.byref(split))
    assert split.value == 1 and grid.value == G and units.value == (M // 256) * ((N + 127) // 128) * (Cin // 64)
    need = l.api.lb_conv_halo_ksplit_workspace_bytes(C.byref(probe))
    n_counters = (M // 256) * ((N + 127) // 128)
    counter_floats = (n_counters * 4 + 255) // 256 * 64
    assert need == counter_floats * 4 + 2 * G * 256 * 128 * 4
    ws, ws_guard = guarded(1, need // 4, need // 4, F32, DEV, back_rows=0)
    ws[0, :counter_floats] = 0
    with pytest.raises(RuntimeError):                   # a split launch without a workspace is refused before anything runs
        launch(params(shape, epi, torch.empty(M, N, dtype=F16, device=DEV), True, ws=None, stats=fresh_stats()))

    # ---- eager, into guarded buffers
    out, out_guard = guarded(M, N, N + 8, F16, DEV)
    st = fresh_stats()
    launch(params(shape, epi, out, True, ws[0], st))
    torch.cuda.synchronize()
    out_guard.assert_intact(name + " output")
    out_guard.assert_fully_written(name + " output")
    ws_guard.assert_intact(name + " workspace")
    assert int(ws[0, :counter_floats].view(torch.int32).abs().max()) == 0, "the kernel must leave its counters zero"
    first = out.clone()
    check_close(results_log, name, first.reshape(B, H, W, N), refs[epi])
    if with_stats:
        assert torch.isfinite(st).all(), "every (row block, channel) slot must be written"
        yf = refs[epi].reshape(B, H * W, N).double()
        tot = st.reshape(N, B, stat_rows // B, 2).double().sum(dim=2).permute(1, 0, 2).cpu()
        check_close(results_log, name + "_sum", tot[..., 0], yf.sum(dim=1))
        check_close(results_log, name + "_sumsq", tot[..., 1], (yf ** 2).sum(dim=1))
        stored = first.double().reshape(B, H * W, N).cpu()           # and tightly: they are the statistics of what was STORED
        assert torch.allclose(tot[..., 0], stored.sum(dim=1), rtol=1e-4, atol=1e-2)
        assert torch.allclose(tot[..., 1], (stored ** 2).sum(dim=1), rtol=1e-4, atol=1e-2)
    first_st = st.clone() if with_stats else None

    # ---- distance to the unsplit kernel on the same operands: recorded, not gated (fp32 re-association only)
    plain = torch.empty(M, N, dtype=F16, device=DEV)
    launch(params(shape, epi, plain, False, stats=fresh_stats()))
    d = (first.float() - plain.float()).abs()
    results_log[name + "_vs_unsplit"] = {"max_abs": float(d.max()), "differing": int((d != 0).sum()), "elements": M * N}
    print(f"[parity] {name}: vs unsplit max_abs={float(d.max()):.3e}, {int((d != 0).sum())} of {M * N} elements differ")

    # ---- ten launches: the same bits (the sum does not depend on which block arrives last)
    for _ in range(10):
        again, st2 = torch.full((M, N), float("nan"), dtype=F16, device=DEV), fresh_stats()
        launch(params(shape, epi, again, True, ws[0], st2))
        assert torch.equal(again, first), "a repeated launch changed the result"
        assert not with_stats or torch.equal(st2, first_st), "a repeated launch changed the statistics"

    # ---- recorded, replayed and as a graph: all bits equal to the eager launch
    rec, st3 = torch.full((M, N), float("nan"), dtype=F16, device=DEV), fresh_stats()
    prog = Program(name)
    with prog.record():
        launch(params(shape, epi, rec, True, ws[0], st3))
    assert prog.num_ops == 1 and torch.isnan(rec).all(), "a recording launches nothing"
    prog.run()
    assert torch.equal(rec, first) and (not with_stats or torch.equal(st3, first_st)), "replay differs from the eager launch"
    prog.instantiate()
    for _ in range(2):
        rec.fill_(float("nan"))
        if with_stats:
            st3.fill_(float("nan"))
        prog.launch()
        assert torch.equal(rec, first) and (not with_stats or torch.equal(st3, first_st)), "graph launch differs from the eager launch"
    torch.cuda.synchronize()
    ws_guard.assert_intact(name + " workspace")
    assert int(ws[0, :counter_floats].view(torch.int32).abs().max()) == 0


def test_unflagged_launch_is_untouched_by_the_switch(forced_split):
    """Without the bit the switch changes nothing: same bits under mode 0 and mode 2, and no workspace is asked for."""
    l = lib()
    shape = "tail_whole_whole"
    B, H, W, Cin, N, _ = SHAPES[shape]
    outs = []
    for mode in (0, 2):
        l.api.lb_conv_halo_set_ksplit(mode, 3)
        out = torch.full((B * H * W, N), float("nan"), dtype=F16, device=DEV)
        launch(params(shape, "plain", out, False))
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    forced_split(shape)
