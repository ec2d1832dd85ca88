"""Host arithmetic of the non-square path (no GPU): the ragged-tile plan of the 3x3 halo conv (LB_GEMM_HALO_RAGGED), the
emitters' fill rule, the programs' cache keys and the refusal of latent sizes the UNet's levels do not divide."""
import pytest

from latentblending_amd.native import geometry as G


def ops():
    from latentblending_amd.hip import ops as o
    return o


def lib():
    from latentblending_amd.hip import lib as l
    return l


def ceil_div(a, b):
    return -(-a // b)


def shipped_tile(H, W):
    """Tile width of the unflagged kernel (0: refused) - the two divisibility lines of lb_conv3x3_halo_eligible."""
    if W % 32 == 0 and H % 8 == 0:
        return 32
    if W % 16 == 0 and H % 16 == 0:
        return 16
    return 0


GRID = [(h, w) for h in (1, 5, 7, 8, 9, 12, 14, 16, 17, 18, 24, 28, 30, 32, 36, 48, 56, 72, 96)
        for w in (1, 9, 15, 16, 17, 24, 31, 32, 33, 40, 42, 48, 64, 68, 84, 96, 128, 168)]


def test_ragged_plan_counts_tiles_with_ceiling_division_and_picks_the_cheaper_tile():
    o, l = ops(), lib()
    B, cin, cout = 3, 64, 200                       # two channel blocks
    for H, W in GRID:
        plain = o.conv_halo_plan(B, H, W, cin, cout)
        ragged = o.conv_halo_plan(B, H, W, cin, cout, flags=l.GEMM_HALO_RAGGED)
        tw0 = shipped_tile(H, W)
        if tw0:                                     # a shape that divides: today's answer, flag or no flag
            assert plain == ragged and plain[:3] == (3, tw0, B * (H * W // 256) * 2), (H, W, plain, ragged)
            continue
        assert plain == (0, 0, 0, 0), (H, W, plain)                     # without the flag: not eligible, as ever
        t32, t16 = ceil_div(W, 32) * ceil_div(H, 8), ceil_div(W, 16) * ceil_div(H, 16)
        tw = 16 if t16 < t32 else 32                                    # fewer tile pixels over the image; ties go to 32
        kind, got_tw, items, grid = ragged
        assert (kind, got_tw, items) == (3, tw, B * min(t32, t16) * 2), (H, W, ragged)
        assert 0 < grid <= items and grid % 2 == 0                      # (a block keeps one channel block)
        assert G.halo_tile_shape(H, W) == (256 // tw, tw)
        assert G.halo_ragged_fill(H, W, tw) == pytest.approx(H * W / (min(t32, t16) * 256.0))


def test_the_flag_lifts_only_the_divisibility_rule():
    o, l = ops(), lib()
    f = l.GEMM_HALO_RAGGED
    assert o.conv_halo_plan(2, 20, 24, 64, 64, flags=f)[0] == 3
    assert o.conv_halo_plan(2, 20, 24, 72, 64, flags=f)[0] == 0         # Cin % 64
    assert o.conv_halo_plan(2, 20, 24, 64, 66, flags=f)[0] == 0         # N % 4
    assert o.conv_halo_plan(2, 20, 24, 64, 64, ks=2, flags=f)[0] == 0   # the 2x2 sub-pixel form has no ragged tiles
    assert o.conv_halo_plan(2, 16, 32, 64, 64, ks=2, flags=f) == o.conv_halo_plan(2, 16, 32, 64, 64, ks=2)


def test_ch_stat_rows_follow_the_ragged_plan():
    o, l = ops(), lib()
    l.api.lb_gemm_set_halo(2)
    try:
        for (B, H, W, cin, cout) in [(3, 5, 9, 128, 64), (9, 36, 68, 64, 256), (2, 30, 40, 64, 64)]:
            assert o.conv_ch_stat_rows(B, H, W, cin, cout) == 0
            th, tw = G.halo_tile_shape(H, W)
            assert o.conv_ch_stat_rows(B, H, W, cin, cout, flags=l.GEMM_HALO_RAGGED) == ceil_div(H, th) * ceil_div(W, tw) * 4
        assert o.conv_ch_stat_rows(2, 16, 32, 64, 64, flags=l.GEMM_HALO_RAGGED) == o.conv_ch_stat_rows(2, 16, 32, 64, 64) == 8
    finally:
        l.api.lb_gemm_set_halo(1)


def test_fill_rule_of_the_emitters():
    use = G.use_ragged_halo
    assert G.halo_ragged_fill(96, 168, 32) == pytest.approx(96 * 168 / (12 * 6 * 256.0))        # 1344 x 768, level 0: 0.875
    assert G.halo_ragged_fill(16, 32, 32) == 1.0
    # all three conditions, then the threshold
    assert use(True, 0, 3, 24, 42, 32, min_fill=0.5)
    assert not use(False, 0, 3, 24, 42, 32, min_fill=0.0)               # square program: never
    assert not use(True, 3, 3, 16, 32, 32, min_fill=0.0)                # the shipped kernel takes the shape already
    assert not use(True, 0, 0, 24, 42, 32, min_fill=0.0)                # not eligible even with the flag (Cin % 64, ...)
    fill = G.halo_ragged_fill(24, 42, 32)                               # 3 x 2 tiles: 1008 / 1536
    assert fill == pytest.approx(0.65625)
    assert use(True, 0, 3, 24, 42, 32, min_fill=fill) and not use(True, 0, 3, 24, 42, 32, min_fill=fill + 1e-9)
    assert use(True, 0, 3, 24, 42, 32) == (fill >= G.HALO_RAGGED_MIN_FILL)
    assert 0.0 <= G.HALO_RAGGED_MIN_FILL <= 1.0


def test_a_side_and_a_pair_name_the_same_program():
    assert G.latent_hw(64) == G.latent_hw((64, 64)) == (64, 64)
    assert G.program_key(17, 64) == G.program_key(17, (64, 64)) == G.program_key(17, [64, 64])
    assert G.program_key(17, (56, 96)) == (17, 56, 96) != G.program_key(17, (96, 56))
    assert G.program_key(2, 64) != G.program_key(17, 64)
    for bad in ((64, 64, 64), (0, 64), -8):
        with pytest.raises(ValueError):
            G.latent_hw(bad)


def test_unet_latent_sizes_must_divide_by_the_levels():
    G.check_unet_latent_size(96, 168, 3)            # 1344 x 768
    G.check_unet_latent_size(72, 128, 3)            # 1024 x 576
    G.check_unet_latent_size(56, 96, 3)             # 768 x 448
    with pytest.raises(ValueError) as e:
        G.check_unet_latent_size(90, 160, 3)        # 1280 x 720: 90 is not a multiple of 4
    assert "88 x 160" in str(e.value) and "92 x 160" in str(e.value) and "1280x704" in str(e.value) and "1280x736" in str(e.value)
    with pytest.raises(ValueError) as e:
        G.check_unet_latent_size(2, 2, 3)
    assert "4 x 4" in str(e.value)
