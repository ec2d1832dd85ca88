"""K-split form of the 3x3 halo-tile conv (LB_GEMM_HALO_KSPLIT, csrc/conv3_halo.hip) on the GPU: tiny shapes under mode 2 with a forced
small grid, so that every path of the in-launch reduction runs - a block whose range starts and ends inside tiles, a tile shared by
three blocks, ranges that end on tile boundaries (no reduction at all), an overhanging channel block - with every epilogue the UNet
uses.  tests/test_halo_ksplit_cpu.py checks that the walks of these cases have those features.

Per case: the result (and the channel statistics) against F.conv2d in fp32 under the bar of test_conv3x3_halo_against_conv2d; ten
launches bit-equal; slabs that start out as NaN never reach the result; guard bands around output and workspace intact; counters zero
afterwards; eager = recorded replay = graph launch bit for bit.  The distance to the unsplit kernel is logged here (fp32
re-association of the chunk sums) and gated, with the values against fp64, in tests/test_halo_ksplit_values_gpu.py; builder, launch
and fixture are shared through tests/_ksplit.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from _guard import guarded  # noqa: E402
from _ksplit import DEV, F16, F32, SHAPES, forced_split, guarded_workspace, launch, lib, operands, params  # noqa: E402,F401
from _parity import check_close  # noqa: E402

# (shape, epilogue): plain = bias only; res = bias + fp16 residual + alpha; rowvec = bias + time-embedding row vector; stats = bias +
# LB_GEMM_CH_STATS
CASES = [("tail_whole_whole", "plain"), ("tail_whole_head", "plain"), ("three_sharers", "plain"), ("tile_boundaries", "plain"),
         ("tail_whole_whole", "res"), ("tail_whole_whole", "rowvec"), ("tail_whole_whole", "stats"), ("tile_boundaries", "stats"),
         ("three_sharers", "stats")]


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
    ws, ws_guard, zeroed = guarded_workspace(probe)
    assert zeroed == counter_floats and ws.shape == (1, need // 4)
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
