"""Shared by the tests of the GroupNorm-on-A form of the 3x3 convs (LB_GEMM_GN_A: conv3_halo.hip, conv3_narrow.hip): seeded stream
operands with the channel statistics a producing conv would have left, the two launch sequences (table kernel + flagged conv /
lb_groupnorm_from_stats + plain conv) and the switch fixture."""
import ctypes as C

import pytest
import torch

from _ksplit import DEV, F16, F32, conv_params, lib, nhwc_dev, stream
from _parity import rnd

STREAM = 2.0 ** -4          # the VAE's residual stream holds value * 2^-4
EPS = 1e-6 * STREAM * STREAM


def channel_stats(x_nhwc):
    """[C, B * rows, 2] fp32 (sum, sum of squares) per (channel, 64-pixel row block) of the fp16 tensor x [B, H, W, C] - what
    LB_GEMM_CH_STATS leaves for a stored tensor (any partition of a sample's pixels into blocks folds to the same statistics) - and
    rows per sample.  Computed in float64 from the stored values, rounded once to fp32."""
    B, H, W, Cc = x_nhwc.shape
    rows = H * W // 64
    v = x_nhwc.double().reshape(B, rows, 64, Cc)
    st = torch.stack([v.sum(2), (v * v).sum(2)], -1)             # [B, rows, C, 2]
    return st.permute(2, 0, 1, 3).reshape(Cc, B * rows, 2).float().contiguous(), rows


def stream_operand(B, H, W, Cin, seed, const=None):
    """A stream tensor [B, H, W, Cin] fp16 (CPU): seeded normal values carrying the 2^-4 scale around a per-channel offset a quarter of
    their size, or the constant ``const`` everywhere."""
    if const is not None:
        return torch.full((B, H, W, Cin), const, dtype=F16)
    off = rnd(1, 1, 1, Cin, seed=seed + 1, dtype=F32) * 0.25
    return ((rnd(B, H, W, Cin, seed=seed, dtype=F32) + off) * STREAM).to(F16)


def gn_params(p, table, silu):
    p.flags |= lib().GEMM_GN_A
    p.gn_table, p.gn_silu = table.data_ptr(), int(silu)
    return p


def entry_of(kind):
    api = lib().api
    return {"halo": api.lb_conv3x3_halo_f16, "narrow": api.lb_conv3x3_narrow_f16, "gemm": api.lb_gemm_f16}[kind]


def run_pair(x_dev, w, gamma, beta, groups, silu, st, rows, *, entry="halo", out_f32=False, ldx=None, **kw):
    """(fused, reference) outputs [M, N] of one conv of GroupNorm(x): the table kernel + the flagged conv reading x itself, against
    lb_groupnorm_from_stats into a fresh contiguous buffer + the unflagged conv.  ``kw`` goes to conv_params (bias, residual, alpha)."""
    from latentblending_amd.hip import ops as o
    B, H, W, Cin = x_dev.shape
    M, N = B * H * W, w.shape[0]
    flags = lib().GEMM_OUT_F32 if out_f32 else 0
    table = o.groupnorm_affine_from_stats(gamma, beta, groups, EPS, st, rows, B, H * W)
    fused = torch.full((M, N), float("nan"), dtype=F32 if out_f32 else F16, device=DEV)
    entry_of(entry)(C.byref(gn_params(conv_params(x_dev, w, fused, flags=flags, **kw), table, silu)), stream())
    n = o.groupnorm_from_stats(x_dev, gamma, beta, groups, EPS, silu, st, rows, ldx=ldx,
                               out=torch.empty(B, H, W, Cin, dtype=F16, device=DEV))
    ref = torch.full((M, N), float("nan"), dtype=F32 if out_f32 else F16, device=DEV)
    entry_of(entry)(C.byref(conv_params(n, w, ref, flags=flags, **kw)), stream())
    torch.cuda.synchronize()
    return fused, ref, n, table


def same_bits(a, b):
    idt = torch.int16 if a.dtype == F16 else torch.int32
    return bool(torch.equal(a.contiguous().view(idt), b.contiguous().view(idt)))


@pytest.fixture
def gn_a_switch():
    """set(mode, grid) for the test; back to the policy and the default grid afterwards."""
    api = lib().api
    yield api.lb_conv_halo_set_gn_a
    api.lb_conv_halo_set_gn_a(1, 0)


def gn_a_plan(p):
    fuse, kind = C.c_int(), C.c_int()
    lib().api.lb_conv_halo_gn_a_plan(C.byref(p), C.byref(fuse), C.byref(kind))
    return fuse.value, kind.value


def host_conv_params(B, H, W, Cin, N, flags=0, ks=3):
    """Parameter block of a 3x3 (ks = 3) or one-launch sub-pixel (ks = 2) conv for the host-side plan / refusal checks: every
    pointer a launch needs is a non-null dummy (nothing is launched with them)."""
    g = lib().ConvGeom.conv3x3(H, W, Cin) if ks == 3 else lib().ConvGeom.subpixel(H, W, Cin, "all")
    return lib().gemm_params(A=4096, W=4096, C=4096, zero_page=4096, M=g.M(B), N=N, K=g.K, ldw=g.K, ldc=N, conv=g, flags=flags)
