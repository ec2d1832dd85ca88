"""K-split form of the 3x3 halo-tile conv (LB_GEMM_HALO_KSPLIT): the host arithmetic of lb_conv_halo_ksplit_plan against an
emulation of the kernel's unit walk (csrc/conv3_halo.hip).  Units are (channel block, pixel tile, 64-channel chunk), chunk fastest;
block b of G walks [b U / G, (b + 1) U / G); a tile cut by a range boundary is summed by the last of its contributors."""
import ctypes

import pytest

from latentblending_amd.hip import lib

SLAB_BYTES = 256 * 128 * 4


def conv_params(B, H, W, Cin, N, flags=0):
    g = lib.ConvGeom.conv3x3(H, W, Cin)
    return lib.gemm_params(M=g.M(B), N=N, K=g.K, ldw=g.K, ldc=N, conv=g, flags=flags, zero_page=64)


def ksplit_plan(p):
    units, grid, split = ctypes.c_long(), ctypes.c_long(), ctypes.c_int()
    lib.api.lb_conv_halo_ksplit_plan(ctypes.byref(p), ctypes.byref(units), ctypes.byref(grid), ctypes.byref(split))
    return units.value, grid.value, split.value


def halo_plan(p):
    kind, tw, items, grid = ctypes.c_int(), ctypes.c_int(), ctypes.c_long(), ctypes.c_long()
    lib.api.lb_conv_halo_plan(ctypes.byref(p), ctypes.byref(kind), ctypes.byref(tw), ctypes.byref(items), ctypes.byref(grid))
    return kind.value, tw.value, items.value, grid.value


@pytest.fixture
def ksplit_switch():
    yield lib.api.lb_conv_halo_set_ksplit
    lib.api.lb_conv_halo_set_ksplit(1, 0)


def walk(units, grid, nchunks):
    """The kernel's walk: per block its segments (tile, c_lo, c_end, slab or None), per tile the contributors the kernel derives."""
    covered = [0] * units
    segments, slabs_used, arrivals = [], set(), {}
    for b in range(grid):
        u_lo, u_hi = b * units // grid, (b + 1) * units // grid
        assert u_lo < u_hi, "a block without a unit"
        first_item = u_lo // nchunks
        item, c_lo = first_item, u_lo - first_item * nchunks
        while True:
            c_end = min(nchunks, u_hi - item * nchunks)
            for c in range(c_lo, c_end):
                covered[item * nchunks + c] += 1
            slab = None
            if c_lo != 0 or c_end != nchunks:
                slab = 2 * b + (0 if item == first_item else 1)
                assert slab not in slabs_used, "two partial sums in one slab"
                slabs_used.add(slab)
                arrivals.setdefault(item, []).append((b, slab))
            segments.append((b, item, c_lo, c_end, slab))
            if (item + 1) * nchunks >= u_hi:
                break
            item, c_lo = item + 1, 0
    return covered, segments, slabs_used, arrivals


def kernel_contributors(item, units, grid, nchunks):
    """What the last arriver computes: first / last contributing block and the slab each one wrote."""
    t0 = item * nchunks
    b_first, b_last = ((t0 + 1) * grid - 1) // units, ((t0 + nchunks) * grid - 1) // units
    return [(b, 2 * b + (0 if (b * units // grid) // nchunks == item else 1)) for b in range(b_first, b_last + 1)]


SPLIT_SHAPES = [(17, 16, 16, 1280, 1280), (17, 32, 32, 640, 640), (17, 64, 64, 320, 320), (2, 64, 64, 320, 320), (17, 64, 64, 512, 512)]
WHOLE_ROUND_SHAPES = [(17, 512, 512, 128, 128), (17, 128, 128, 512, 512)]


@pytest.mark.parametrize("shape", SPLIT_SHAPES)
def test_policy_splits_partial_rounds(shape):
    """The five shapes the K-split form was built for: the policy splits them, on one block per CU.

    Measured (profiles/halo_ksplit_ab.txt, us per launch unsplit -> split, one MI355X): (17,16,16,1280,1280) 121.7 -> 111.8,
    (17,32,32,640,640) 141.8 -> 116.4, (17,64,64,320,320) 144.7 -> 136.7, (2,64,64,320,320) 33.9 -> 32.1, (17,64,64,512,512)
    287.0 -> 270.4."""
    B, H, W, Cin, N = shape
    p = conv_params(B, H, W, Cin, N, lib.GEMM_HALO_KSPLIT)
    kind, _, items, _ = halo_plan(p)
    assert kind == 3
    units, grid, split = ksplit_plan(p)
    cus = halo_plan(conv_params(17, 512, 512, 128, 128))[3]      # a launch of 17408 one-channel-block items: one block per CU
    assert split == 1 and grid == cus and units == items * (Cin // 64)
    # the unflagged plan is what it was, and an unflagged launch never splits
    assert halo_plan(conv_params(B, H, W, Cin, N))[2:] == halo_plan(p)[2:]
    assert ksplit_plan(conv_params(B, H, W, Cin, N)) == (0, 0, 0)
    assert lib.api.lb_conv_halo_ksplit_workspace_bytes(ctypes.byref(conv_params(B, H, W, Cin, N))) == 0


@pytest.mark.parametrize("shape", WHOLE_ROUND_SHAPES)
def test_policy_leaves_whole_rounds_unsplit(shape):
    p = conv_params(*shape, lib.GEMM_HALO_KSPLIT)
    _, _, items, grid = halo_plan(p)
    assert items % grid == 0                                     # 68 / 17 whole rounds
    assert ksplit_plan(p)[2] == 0
    assert lib.api.lb_conv_halo_ksplit_workspace_bytes(ctypes.byref(p)) == 0


def test_switch_modes(ksplit_switch):
    p = conv_params(17, 32, 32, 640, 640, lib.GEMM_HALO_KSPLIT)
    ksplit_switch(0, 0)
    assert ksplit_plan(p)[2] == 0
    ksplit_switch(2, 0)
    assert ksplit_plan(p)[2] == 1
    assert ksplit_plan(conv_params(17, 128, 128, 512, 512, lib.GEMM_HALO_KSPLIT))[2] == 1      # mode 2: every flagged launch ...
    assert ksplit_plan(conv_params(17, 64, 64, 64, 128, lib.GEMM_HALO_KSPLIT))[2] == 0         # ... with Cin >= 128
    assert ksplit_plan(conv_params(1, 40, 24, 128, 128, lib.GEMM_HALO_KSPLIT | lib.GEMM_HALO_RAGGED))[2] == 0    # ragged: out of scope
    ksplit_switch(2, 7)
    assert ksplit_plan(p)[1] == 7
    ksplit_switch(2, 10 ** 6)                                    # never more blocks than units
    units, grid, _ = ksplit_plan(p)
    assert grid == units


WALK_CASES = [(s, 0) for s in SPLIT_SHAPES] + [((4, 16, 32, 128, 128), 3), ((1, 32, 16, 320, 132), 7), ((2, 16, 16, 192, 256), 4),
                                                ((1, 16, 16, 640, 128), 10), ((3, 16, 16, 128, 384), 5), ((1, 16, 16, 128, 128), 2),
                                                # one_unit_per_block and default_grid of tests/_ksplit.py (the latter on 256 blocks here)
                                                ((1, 16, 16, 1280, 128), 20), ((4, 32, 32, 1280, 256), 256)]


@pytest.mark.parametrize("shape,forced_grid", WALK_CASES)
def test_unit_walk(shape, forced_grid, ksplit_switch):
    B, H, W, Cin, N = shape
    ksplit_switch(2, forced_grid)                                # (the walk, not the policy: 0 = one block per CU)
    p = conv_params(B, H, W, Cin, N, lib.GEMM_HALO_KSPLIT)
    units, grid, split = ksplit_plan(p)
    nchunks = Cin // 64
    assert split == 1 and units == halo_plan(p)[2] * nchunks and (not forced_grid or grid == min(forced_grid, units))
    covered, segments, slabs_used, arrivals = walk(units, grid, nchunks)
    assert covered == [1] * units                                # every unit exactly once
    for item, who in arrivals.items():                           # the contributors the kernel derives = the blocks that arrive
        assert who == kernel_contributors(item, units, grid, nchunks)
        assert sum(c_end - c_lo for b, it, c_lo, c_end, _ in segments if it == item) == nchunks
    for b, item, c_lo, c_end, slab in segments:                  # whole tiles take no ticket
        assert (slab is None) == (c_lo == 0 and c_end == nchunks)
    need = lib.api.lb_conv_halo_ksplit_workspace_bytes(ctypes.byref(p))
    counters = (units // nchunks * 4 + 255) // 256 * 256
    assert need >= counters + (max(slabs_used) + 1 if slabs_used else 0) * SLAB_BYTES
    assert need == counters + 2 * grid * SLAB_BYTES


def test_cases_of_the_gpu_test_are_what_they_claim(ksplit_switch):
    """The three protocol cases of tests/test_halo_ksplit_gpu.py: the walk has the features their descriptions promise."""
    ksplit_switch(2, 3)
    units, grid, _ = ksplit_plan(conv_params(4, 16, 32, 128, 128, lib.GEMM_HALO_KSPLIT))
    _, segments, _, _ = walk(units, grid, 2)
    # 16 units over 3 blocks = [0, 5), [5, 10), [10, 16): the head of tile 2 | its tail and two whole tiles | whole tiles
    assert [(c_lo, c_end) for b, _, c_lo, c_end, _ in segments if b == 0] == [(0, 2), (0, 2), (0, 1)]
    assert [(c_lo, c_end) for b, _, c_lo, c_end, _ in segments if b == 1] == [(1, 2), (0, 2), (0, 2)]
    # (the same image with three chunks over 5 blocks: block 3 holds the tail of one tile, a whole tile and the head of the next)
    ksplit_switch(2, 5)
    units, grid, _ = ksplit_plan(conv_params(4, 16, 32, 192, 128, lib.GEMM_HALO_KSPLIT))
    _, segments, _, _ = walk(units, grid, 3)
    assert [(c_lo, c_end) for b, _, c_lo, c_end, _ in segments if b == 3] == [(2, 3), (0, 3), (0, 1)]
    ksplit_switch(2, 7)
    units, grid, _ = ksplit_plan(conv_params(1, 32, 16, 320, 132, lib.GEMM_HALO_KSPLIT))
    _, _, _, arrivals = walk(units, grid, 5)
    assert max(len(v) for v in arrivals.values()) == 3                           # a tile shared by three blocks
    ksplit_switch(2, 4)
    units, grid, _ = ksplit_plan(conv_params(2, 16, 16, 192, 256, lib.GEMM_HALO_KSPLIT))
    _, _, slabs_used, arrivals = walk(units, grid, 3)
    assert not slabs_used and not arrivals                                       # ranges end on tile boundaries: no partials


def test_new_cases_of_the_gpu_tests_are_what_they_claim(ksplit_switch):
    """one_unit_per_block and default_grid of tests/_ksplit.py (tests/test_halo_ksplit_values_gpu.py)."""
    ksplit_switch(2, 20)
    units, grid, _ = ksplit_plan(conv_params(1, 16, 16, 1280, 128, lib.GEMM_HALO_KSPLIT))
    assert (units, grid) == (20, 20)
    _, segments, slabs_used, arrivals = walk(units, grid, 20)
    assert [(b, item, c_lo, c_end) for b, item, c_lo, c_end, _ in segments] == [(c, 0, c, c + 1) for c in range(20)]
    assert list(arrivals) == [0] and len(arrivals[0]) == 20 and slabs_used == {2 * b for b in range(20)}   # 20 contributors to one tile
    ksplit_switch(2, 256)
    units, grid, _ = ksplit_plan(conv_params(4, 32, 32, 1280, 256, lib.GEMM_HALO_KSPLIT))
    assert (units, grid) == (640, 256)                                           # more units than blocks: 2.5 units per block
    _, segments, _, arrivals = walk(units, grid, 20)
    assert len(arrivals) == 32 and {len(v) for v in arrivals.values()} == {8}    # every tile is cut, into 8 partial sums of 2 or 3 chunks
    assert {c_end - c_lo for _, _, c_lo, c_end, _ in segments} == {2, 3}


def gemm_plan(p):
    tile, splitk, blocks = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    lib.api.lb_gemm_plan(ctypes.byref(p), ctypes.byref(tile), ctypes.byref(splitk), ctypes.byref(blocks))
    return tile.value, splitk.value, blocks.value


@pytest.fixture
def halo_switch():
    yield lib.api.lb_gemm_set_halo
    lib.api.lb_gemm_set_halo(1)


# (B, H, W, Cin, N, stride): 3x3 convs lb_gemm_f16 does not take to the halo kernel by default (too few halo blocks; stride 2; N = 4:
# the narrow-N kernel, tile code 8, whenever the halo switch is not 0)
PLAN_SHAPES = [(1, 16, 16, 1280, 128, 1), (2, 16, 16, 640, 320, 1), (1, 32, 32, 320, 64, 1), (2, 32, 32, 320, 320, 2),
               (4, 16, 32, 128, 4, 1)]


@pytest.mark.parametrize("shape", PLAN_SHAPES)
def test_gemm_plan_of_a_flagged_conv_is_the_plan_of_the_launch(shape, ksplit_switch, halo_switch):
    """lb_gemm_plan is "the tile / split-K / grid lb_gemm_f16 would use".  lb_gemm_f16 runs a flagged conv it does not route to the
    halo kernel without the flag and without ``partial`` (the K-split workspace is no split-K workspace): the plan of the flagged
    problem with ``partial`` set must be the plan of the unflagged problem without it - split-K 1, not 11 / 5 / 2 -, whatever the
    two switches say."""
    B, H, W, Cin, N, stride = shape

    def problem(flagged):
        p = conv_params(B, H, W, Cin, N, lib.GEMM_HALO_KSPLIT if flagged else 0)
        p.stride, p.Hout, p.Wout = stride, (H - 1) // stride + 1, (W - 1) // stride + 1
        p.M = B * p.Hout * p.Wout
        p.partial = 4096 if flagged else None            # (host arithmetic only: never dereferenced)
        return p

    for halo_mode in (1, 0, 2):
        halo_switch(halo_mode)
        for mode in (0, 2):
            ksplit_switch(mode, 0)
            want = gemm_plan(problem(False))
            assert gemm_plan(problem(True)) == want, (halo_mode, mode)
            assert want[1] == 1 and (want[0] == 6) == (halo_mode == 2 and stride == 1 and N > 16)
            assert (want[0] == 8) == (halo_mode != 0 and N <= 16)
