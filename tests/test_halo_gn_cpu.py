"""Host side of the GroupNorm-on-A form of the 3x3 convs (LB_GEMM_GN_A): the plan's decisions for the VAE's shapes, what the
launchers refuse (before anything is launched: no GPU needed) and the emitter's fallbacks, recorded on the CPU."""
import ctypes as C

import pytest
import torch

from _halo_gn import gn_a_plan, gn_a_switch, host_conv_params  # noqa: F401

from latentblending_amd.hip import lib
from latentblending_amd.hip.lib import api

# the GroupNorm -> 3x3 conv pairs of the VAE decode at 512^2: (H = W, Cin, N), and whether the measured policy folds them at
# B = 17 (profiles/halo_gn_ab.txt: one channel block in, more out; at B = 2 - 8 tiles per block - no halo launch passed; the
# narrow-N conv_out in at both)
VAE_PAIRS = [(64, 512, 512, False), (128, 512, 512, False), (256, 512, 256, False), (256, 256, 256, False),
             (512, 256, 128, True), (512, 128, 128, True)]


@pytest.mark.parametrize("B", [17, 2])
def test_plan_for_the_vae_shapes(B, gn_a_switch):
    for mode in (1, 0, 2):
        gn_a_switch(mode, 0)
        for H, Cin, N, policy in VAE_PAIRS:
            p = host_conv_params(B, H, H, Cin, N)
            tile = C.c_int()
            api.lb_gemm_plan(C.byref(p), C.byref(tile), None, None)
            split = C.c_int()
            q = host_conv_params(B, H, H, Cin, N, flags=lib.GEMM_HALO_KSPLIT)
            api.lb_conv_halo_ksplit_plan(C.byref(q), None, None, C.byref(split))
            fuse, kind = gn_a_plan(p)
            if tile.value != 6:                     # (a B = 2 level whose grid does not fill the chip: not a halo launch)
                assert (fuse, kind) == (0, 0), (B, H, Cin, N)
                continue
            assert kind == 3 and fuse == {0: 0, 1: int(policy and B == 17), 2: 1}[mode], (mode, B, H, Cin, N, fuse, kind)
            # the same launch as the emitter flags it where the K-split plan splits: no GroupNorm fold there
            q.partial = 4096
            assert gn_a_plan(q) == ((0, 0) if split.value else (fuse, 3)), (mode, B, H, Cin, N)
        out = host_conv_params(B, 512, 512, 128, 4, flags=lib.GEMM_OUT_F32)
        assert gn_a_plan(out) == (int(mode != 0), 8)


def test_plan_refuses_what_no_kernel_implements(gn_a_switch):
    gn_a_switch(2, 0)
    assert gn_a_plan(host_conv_params(17, 512, 512, 128, 128)) == (1, 3)
    assert gn_a_plan(host_conv_params(17, 512, 512, 128, 128, flags=lib.GEMM_GN_A)) == (0, 0)       # asked with the flag already set
    assert gn_a_plan(host_conv_params(17, 512, 512, 128, 128, flags=lib.GEMM_C64)) == (0, 0)
    assert gn_a_plan(host_conv_params(17, 520, 520, 128, 128, flags=lib.GEMM_HALO_RAGGED)) == (0, 0)  # ragged tiles
    assert gn_a_plan(host_conv_params(17, 256, 256, 128, 128, ks=2)) == (0, 0)                      # sub-pixel upconv
    assert gn_a_plan(host_conv_params(17, 512, 512, 96, 128)) == (0, 0)                             # Cin % 64: implicit GEMM
    p = host_conv_params(17, 512, 512, 128, 128)
    p.stride, p.Hout, p.Wout, p.M = 2, 256, 256, 17 * 256 * 256
    assert gn_a_plan(p) == (0, 0)
    api.lb_gemm_set_halo(0)
    try:
        assert gn_a_plan(host_conv_params(17, 512, 512, 128, 128)) == (0, 0)
        assert gn_a_plan(host_conv_params(17, 512, 512, 128, 4)) == (0, 0)
    finally:
        api.lb_gemm_set_halo(1)


def _flagged(p, table=4096):
    p.flags |= lib.GEMM_GN_A
    p.gn_table, p.gn_silu = table, 1
    return p


def test_launchers_refuse_before_launching():
    P = host_conv_params
    with pytest.raises(RuntimeError, match="gn_table"):
        api.lb_conv3x3_halo_f16(C.byref(_flagged(P(2, 16, 32, 128, 128), table=None)), None)
    with pytest.raises(RuntimeError, match="gn_table"):
        api.lb_conv3x3_narrow_f16(C.byref(_flagged(P(2, 16, 32, 128, 4), table=None)), None)
    with pytest.raises(RuntimeError, match="16-byte"):
        api.lb_conv3x3_halo_f16(C.byref(_flagged(P(2, 16, 32, 128, 128), table=4100)), None)
    with pytest.raises(RuntimeError, match="whole tiles"):
        api.lb_conv3x3_halo_f16(C.byref(_flagged(P(2, 20, 40, 128, 128, flags=lib.GEMM_HALO_RAGGED))), None)
    ks = _flagged(P(17, 64, 64, 320, 320, flags=lib.GEMM_HALO_KSPLIT))
    ks.partial = 4096
    with pytest.raises(RuntimeError, match="exclude each other"):
        api.lb_conv3x3_halo_f16(C.byref(ks), None)
    with pytest.raises(RuntimeError, match="exclude each other"):
        api.lb_gemm_f16(C.byref(ks), None)
    up = _flagged(P(17, 64, 64, 128, 128, ks=2))
    up.W = 4096
    with pytest.raises(RuntimeError, match="LB_GEMM_GN_A"):
        api.lb_upconv2x_halo_f16(C.byref(up), None)
    with pytest.raises(RuntimeError, match="LB_GEMM_GN_A"):
        api.lb_gemm_f16(C.byref(up), None)
    with pytest.raises(RuntimeError, match="LB_GEMM_GN_A"):       # a conv the router sends to the implicit GEMM
        api.lb_gemm_f16(C.byref(_flagged(P(2, 16, 32, 96, 128))), None)
    with pytest.raises(RuntimeError, match="LB_GEMM_GN_A"):       # a plain GEMM
        g = lib.gemm_params(A=4096, W=4096, C=4096, zero_page=4096, M=64, N=64, K=64, lda=64, ldw=64, ldc=64)
        api.lb_gemm_f16(C.byref(_flagged(g)), None)
    with pytest.raises(RuntimeError, match="LB_GEMM_GN_A"):
        api.lb_gemm_f16(C.byref(_flagged(P(2, 16, 16, 64, 64, flags=lib.GEMM_C64))), None)
    with pytest.raises(RuntimeError, match="sizes"):
        api.lb_groupnorm_affine_from_stats(None, 4096, 4096, 4096, 2, 64, 64, 32, 1e-6, 1, None)
    with pytest.raises(RuntimeError, match="groups"):
        api.lb_groupnorm_affine_from_stats(4096, 4096, 4096, 4096, 2, 64, 64, 48, 1e-6, 1, None)


# ---------------------------------------------------------------- the emitter, recorded on the CPU
@pytest.fixture
def cpu_emitter(monkeypatch):
    import latentblending_amd.native.runtime as rt
    monkeypatch.setattr(rt, "_stream", lambda: None)
    em = rt.Emitter(rt.Arena("cpu"))
    return rt, em


def _conv_of_groupnorm(rt, em, B, H, Cin, N, *, x_dtype=torch.float16, stats=True, flags=0, residual=False):
    """Record "3x3 conv of GroupNorm(x)" the way VAEProgram does -> the recorded op names."""
    F32 = torch.float32
    x = torch.empty(B, H, H, Cin, dtype=x_dtype)            # (never touched: only shapes, dtypes and addresses count)
    w = torch.empty(N, 9 * Cin, dtype=torch.float16)
    out = torch.empty(B * H * H, N, dtype=F32 if flags & lib.GEMM_OUT_F32 else torch.float16)
    gamma = torch.ones(Cin, dtype=F32)
    st = (torch.zeros(Cin, B * 4, 2, dtype=F32), 4) if stats else None
    conv = lib.ConvGeom.conv3x3(H, H, Cin)
    prog = rt.Program("t")
    with prog.record():
        g = em.gn_operand(x, w, M=B * H * H, conv=conv, flags=flags, has_residual=residual, gamma=gamma, beta=gamma, B=B, HW=H * H,
                          C_=Cin, eps=1e-6, silu=True, groups=32, ch_stats=st)
        em.gemm(x, w, out, M=B * H * H, conv=conv, flags=flags, residual=out if residual else None, gn=g)
    assert g.table is None and g.scratch is None            # both went back to the arena
    return prog.op_names()


def test_emitter_folds_and_falls_back(cpu_emitter, gn_a_switch):
    rt, em = cpu_emitter
    FOLD, PAIR = ["lb_groupnorm_affine_from_stats", "lb_conv3x3_halo_f16"], ["lb_groupnorm_from_stats", "lb_conv3x3_halo_f16"]
    gn_a_switch(1, 0)
    n_norm = len(em.norm_log)
    assert _conv_of_groupnorm(rt, em, 17, 512, 128, 128) == FOLD
    assert _conv_of_groupnorm(rt, em, 17, 512, 128, 128, residual=True) == FOLD
    assert len(em.norm_log) == n_norm and len(em.gemm_log) == 2          # no classified GroupNorm op, one log entry per conv
    assert _conv_of_groupnorm(rt, em, 17, 512, 128, 4, flags=lib.GEMM_OUT_F32) == ["lb_groupnorm_affine_from_stats", "lb_conv3x3_narrow_f16"]
    # fallbacks: exactly the ops of ever
    assert _conv_of_groupnorm(rt, em, 17, 128, 512, 512) == PAIR                                   # outside the measured policy
    assert _conv_of_groupnorm(rt, em, 17, 512, 128, 128, stats=False) == ["lb_groupnorm_nhwc", "lb_conv3x3_halo_f16"]
    assert _conv_of_groupnorm(rt, em, 17, 512, 128, 128, x_dtype=torch.float32, flags=lib.GEMM_OUT_F32) == PAIR    # fp32 stream
    assert _conv_of_groupnorm(rt, em, 2, 32, 128, 128) == ["lb_groupnorm_from_stats", "lb_gemm_f16"]               # not a halo route
    assert [e["op"] for e in em.norm_log[n_norm:]] == ["lb_groupnorm_from_stats", "lb_groupnorm_nhwc", "lb_groupnorm_from_stats",
                                                      "lb_groupnorm_from_stats"]
    gn_a_switch(0, 0)
    assert _conv_of_groupnorm(rt, em, 17, 512, 128, 128) == PAIR
    assert _conv_of_groupnorm(rt, em, 17, 512, 128, 4, flags=lib.GEMM_OUT_F32) == ["lb_groupnorm_from_stats", "lb_conv3x3_narrow_f16"]
    gn_a_switch(2, 0)
    em.gn_a = False                                                                               # the emitter's own switch
    assert _conv_of_groupnorm(rt, em, 17, 512, 128, 128) == PAIR
    em.gn_a = True
    assert _conv_of_groupnorm(rt, em, 17, 128, 512, 512) == FOLD


def test_emitter_leaves_ksplit_and_ragged_launches_alone(cpu_emitter, gn_a_switch):
    rt, em = cpu_emitter
    gn_a_switch(2, 0)
    api.lb_conv_halo_set_ksplit(2, 0)
    try:        # every Cin >= 128 launch splits: the K-split form has no GroupNorm-on-A twin
        assert _conv_of_groupnorm(rt, em, 17, 512, 128, 128) == ["lb_groupnorm_from_stats", "lb_conv3x3_halo_f16"]
    finally:
        api.lb_conv_halo_set_ksplit(1, 0)
    em.ragged_halo = True
    assert _conv_of_groupnorm(rt, em, 17, 520, 128, 128) == ["lb_groupnorm_from_stats", "lb_conv3x3_halo_f16"]
    assert _conv_of_groupnorm(rt, em, 17, 512, 128, 128) == ["lb_groupnorm_affine_from_stats", "lb_conv3x3_halo_f16"]
