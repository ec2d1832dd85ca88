"""Host side of the tiny decoder and of LB_GEMM_C64 (no GPU: plans, refusals and recordings are host arithmetic; the float64
restatement of the decoder runs on the CPU)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _taesd_ref as T  # noqa: E402


def lib():
    from latentblending_amd.hip import lib as l
    return l


def c64_params(B=2, H=12, W=20, Cin=64, N=64, ups=0, stride=1, flags=None, **over):
    """An eligible flagged problem (fake pointers: nothing here launches), then the overrides."""
    l = lib()
    g = l.ConvGeom.conv3x3(H, W, Cin, stride=stride, ups=ups)
    p = l.gemm_params(A=4096, W=8192, C=12288, zero_page=64, M=g.M(B), N=N, K=g.K, ldw=g.K, ldc=N, ldr=N, conv=g,
                      flags=l.GEMM_C64 if flags is None else flags)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def plan(p):
    t, sk, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    lib().api.lb_gemm_plan(ctypes.byref(p), ctypes.byref(t), ctypes.byref(sk), ctypes.byref(nb))
    return t.value, sk.value, nb.value


def test_flag_constant_matches_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "lb_hip.h")) as fh:
        assert "LB_GEMM_C64 = 2048" in fh.read()
    assert lib().GEMM_C64 == 2048


def test_plan_reports_tile_code_12_and_the_persistent_grid():
    """Eligible + flagged: tile code 12, no split, blocks = min(tiles, CUs) with tiles counted by ceiling division.  The grid is
    bounded by the CU count, which the library reads from the device (256 when there is none): only the bound is asserted."""
    assert plan(c64_params(B=2, H=12, W=20)) == (12, 1, 2 * 1 * 2)                  # 4 tiles: fewer than any chip has CUs
    assert plan(c64_params(B=1, H=4, W=4)) == (12, 1, 1)                            # smaller than one tile
    assert plan(c64_params(B=1, H=20, W=18, ups=1)) == (12, 1, 3 * 3)               # 40 x 36 output: 3 x 3 ragged tiles
    t, sk, nb = plan(c64_params(B=17, H=512, W=512))
    assert (t, sk) == (12, 1) and 0 < nb <= 17 * 1024 and nb <= 1024                # persistent: not one block per tile


def test_unflagged_plans_are_the_parents():
    """Without the bit nothing moves: the same 64 -> 64 problems plan what they planned before the flag existed (halo-tile kernel,
    tile code 6, one block per 256 pixels, where the image divides into tiles and the grid has >= 96 blocks; 64x64 implicit-GEMM
    tiles below that), and lb_conv_halo_plan / lb_gemm_ch_stat_rows see the flagged problem as 'not a halo launch'."""
    l = lib()
    assert plan(c64_params(B=17, H=64, W=64, flags=0))[::2] == (6, 17 * 16)         # conv_plan(17, 64, 64, 64) of the policy test
    assert plan(c64_params(B=17, H=512, W=512, flags=0))[::2] == (6, 17 * 1024)
    assert plan(c64_params(B=2, H=12, W=20, flags=0)) == (3, 1, 8)                  # 480 rows of 64x64 tiles (no workspace: no split)
    assert plan(c64_params(B=2, H=32, W=32, flags=0)) == (3, 1, 32)                 # 8 halo blocks < 96: implicit GEMM
    kind, tw, items, grid = ctypes.c_int(), ctypes.c_int(), ctypes.c_long(), ctypes.c_long()
    for flags, want in ((0, 3), (l.GEMM_C64, 0)):
        p = c64_params(B=17, H=64, W=64, flags=flags)
        l.api.lb_conv_halo_plan(ctypes.byref(p), ctypes.byref(kind), ctypes.byref(tw), ctypes.byref(items), ctypes.byref(grid))
        assert kind.value == want
    assert l.api.lb_gemm_ch_stat_rows(ctypes.byref(c64_params(B=17, H=64, W=64, flags=0))) == 16 * 4
    assert l.api.lb_gemm_ch_stat_rows(ctypes.byref(c64_params(B=17, H=64, W=64))) == 0


def refusals():
    l = lib()
    C = l.GEMM_C64
    return [
        ("Cin 128", dict(Cin=128), "Cin must be 64"),
        ("N 128", dict(N=128), "N must be 64"),
        ("N 60", dict(N=60), "N must be 64"),
        ("stride 2", dict(stride=2), "stride must be 1"),
        ("OUT_F32", dict(flags=C | l.GEMM_OUT_F32), "LB_GEMM_OUT_F32 is not supported"),
        ("SILU", dict(flags=C | l.GEMM_SILU), "LB_GEMM_SILU is not supported"),
        ("CH_STATS", dict(flags=C | l.GEMM_CH_STATS, ch_stats=4096, ch_stats_rows=4), "LB_GEMM_CH_STATS is not supported"),
        ("RES_F32", dict(flags=C | l.GEMM_RES_F32), "LB_GEMM_RES_F32 is not supported"),
        ("GELU", dict(flags=C | l.GEMM_GELU), "GELU flags are not supported"),
        ("rowvec", dict(rowvec=4096, ld_rowvec=64, rows_per_batch=240), "rowvec is not supported"),
        ("partial", dict(partial=4096), "partial (split-K) is not supported"),
        ("Hout != Hin << ups", dict(ups=1, Hout=12, Wout=20, M=2 * 12 * 20), "Hout == Hin << ups"),
        ("ups 2", dict(ups=2, Hout=48, Wout=80, M=2 * 48 * 80), "ups must be 0 or 1"),
        ("null zero page", dict(zero_page=None), "zero_page must be set"),
        ("pad 0", dict(pad=0), "pad must be 1"),
        ("scatter", dict(scatter=1, KH=2, KW=2, K=256), "KH = KW = 3"),
        ("ldx 56", dict(ldx=56), "ldx must be a multiple of 8, at least 64"),
        ("not a conv", dict(conv=0, lda=576), "needs a convolution"),
    ]


@pytest.mark.parametrize("i", range(18))
def test_flagged_problems_of_another_shape_are_refused_by_name(i):
    """lb_gemm_f16 with the bit set never takes another route: every violated condition fails with a message that names it, in a
    direct call (before any launch: this runs without a device) and while recording - where the refusal records nothing.  The plan
    refuses the same problems."""
    l = lib()
    name, over, message = refusals()[i]
    p = c64_params(**over)
    with pytest.raises(RuntimeError, match="LB_GEMM_C64") as e:
        l.api.lb_gemm_f16(ctypes.byref(p), None)
    assert message in str(e.value), (name, str(e.value))
    prog = l.api.lb_program_create()
    try:
        l.api.lb_program_begin_record(prog)
        try:
            with pytest.raises(RuntimeError, match="LB_GEMM_C64") as e:
                l.api.lb_gemm_f16(ctypes.byref(p), None)
            assert message in str(e.value), (name, str(e.value))
        finally:
            l.api.lb_program_end_record(prog)
        assert l.api.lb_program_num_ops(prog) == 0
    finally:
        l.api.lb_program_destroy(prog)
    with pytest.raises(RuntimeError) as e:
        plan(p)
    assert message in str(e.value)


def test_refusal_list_is_complete():
    assert len(refusals()) == 18


def test_an_eligible_call_records_one_op_under_its_own_name():
    l = lib()
    prog = l.api.lb_program_create()
    try:
        l.api.lb_program_begin_record(prog)
        try:
            for kw in (dict(), dict(ups=1, H=6, W=10), dict(flags=l.GEMM_C64 | l.GEMM_RELU, bias=4096, residual=8192, ldr=76, ldx=72, ldc=68)):
                l.api.lb_gemm_f16(ctypes.byref(c64_params(**kw)), None)
            l.api.lb_gemm_f16(ctypes.byref(c64_params(B=17, H=64, W=64, flags=0)), None)       # the same conv without the bit
        finally:
            l.api.lb_program_end_record(prog)
        names = [l.api.lb_program_op_name(prog, k).decode() for k in range(l.api.lb_program_num_ops(prog))]
        assert names == ["conv3x3_c64"] * 3 + ["lb_conv3x3_halo_f16"]
    finally:
        l.api.lb_program_destroy(prog)


# ---------------------------------------------------------------------------------------------- the decoder's restatement
LATENTS = [(3, 4, 4, 4), (2, 4, 4, 12), (1, 4, 8, 8)]


def latents(shape, seed=5):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).half()


def test_state_dict_keys_are_the_checkpoints():
    from latentblending_amd.native import tiny_vae
    want = (["decoder.layers.0.weight", "decoder.layers.0.bias"]
            + [f"decoder.layers.{n}.conv.{c}.{wb}" for n in (2, 3, 4) for c in (0, 2, 4) for wb in ("weight", "bias")]
            + ["decoder.layers.6.weight"]
            + [f"decoder.layers.{n}.conv.{c}.{wb}" for n in (7, 8, 9) for c in (0, 2, 4) for wb in ("weight", "bias")]
            + ["decoder.layers.11.weight"]
            + [f"decoder.layers.{n}.conv.{c}.{wb}" for n in (12, 13, 14) for c in (0, 2, 4) for wb in ("weight", "bias")]
            + ["decoder.layers.16.weight"]
            + [f"decoder.layers.17.conv.{c}.{wb}" for c in (0, 2, 4) for wb in ("weight", "bias")]
            + ["decoder.layers.18.weight", "decoder.layers.18.bias"])
    assert T.KEYS == want
    assert sorted(T.synthetic_state_dict(0)) == sorted(want)
    assert tiny_vae.state_dict_keys() == want
    sd = T.synthetic_state_dict(0)
    assert sd["decoder.layers.0.weight"].shape == (64, 4, 3, 3) and sd["decoder.layers.18.weight"].shape == (3, 64, 3, 3)
    assert sd["decoder.layers.6.weight"].shape == (64, 64, 3, 3) and "decoder.layers.6.bias" not in sd
    assert all(torch.equal(v, v.half().float()) for v in sd.values())              # fp16-representable: both sides read the same bits


def test_config_is_taesdxls_and_refuses_other_widths():
    from latentblending_amd.native import TinyVAEConfig
    c = TinyVAEConfig()
    assert (c.latent_channels, c.out_channels, c.block_channels, c.num_blocks) == (4, 3, (64, 64, 64, 64), (3, 3, 3, 1))
    assert (c.latent_magnitude, c.scaling_factor, c.scale_factor) == (3.0, 1.0, 8)
    with pytest.raises(ValueError, match="64"):
        TinyVAEConfig(block_channels=(64, 64, 128, 64))


@pytest.mark.parametrize("shape", LATENTS)
def test_restatement_float32_agrees_with_float64(shape):
    """The checker itself: float32 against float64 to round-off.  About 30 convs of K <= 576 on O(1) values: each fp32 conv is
    within K * 2^-24 * sum|x w| <= 576 * 6e-8 * O(1) of its exact value and the blocks' residual form passes errors on with gain
    about 1, so 1e-4 absolute is two orders of magnitude above the expected 1e-6 and far below a u8 step (2 / 255 = 7.8e-3)."""
    sd, z = T.synthetic_state_dict(0), latents(shape)
    i64, i32 = T.decode(sd, z), T.decode(sd, z, torch.float32)
    assert i64.shape == (shape[0], 3, 8 * shape[2], 8 * shape[3]) and i64.dtype == torch.float64
    assert float((i32.double() - i64).abs().max()) < 1e-4


@pytest.mark.parametrize("shape", LATENTS)
def test_synthetic_frames_are_not_saturated(shape):
    """The condition under which the decoder's byte-level bars mean something: at most 1 % of the float64 reference's bytes are 0 or
    255 on the test's weights and latents (a saturated byte agrees with anything beyond the clamp)."""
    u8 = T.to_u8(T.decode(T.synthetic_state_dict(0), latents(shape)))
    share = float(((u8 == 0) | (u8 == 255)).float().mean())
    assert share <= 0.01, share
    assert 15.0 < float(u8.float().std()) < 60.0                                    # a picture, not a flat field


# ---------------------------------------------------------------------------------------------- pipe arguments (no device)
def test_pipe_refuses_unknown_decoders_before_it_needs_a_device():
    from latentblending_amd.native import NativeSDXLPipe
    for bad in ("medium", "", None, 3, "tiny2"):
        with pytest.raises(ValueError, match="decoder"):
            NativeSDXLPipe(decoder=bad, allow_synthetic=True)
    assert NativeSDXLPipe._check_decoder(" TINY ") == "tiny" and NativeSDXLPipe._check_decoder("Full") == "full"


def test_emitter_rule_counts_output_tiles():
    from latentblending_amd.native import tiny_vae
    assert tiny_vae.use_c64(17, 512, 512) and tiny_vae.use_c64(1, 4, 4, min_tiles=1)
    assert tiny_vae.use_c64(2, 12, 20, min_tiles=4) and not tiny_vae.use_c64(2, 12, 20, min_tiles=5)
