"""Wrap-around padding (LbGemmParams.wrap, ``NativeSDXLPipe(tileable=...)``) on a real MI355X: every conv route, then whole programs.

Per kernel, for wrap 1 (x), 2 (y) and 3 (both) and two DIFFERENT samples, each launch first proves through lb_conv_plan that it runs
where the case says, and is then held three ways:

1. float64: every element against ``_tileable_ref.circ_conv`` (F.pad circular on the wrapped axes, zeros on the other) inside
   ``_parity.contraction_bound`` - the bound the float64 tests of the same kernels use (test_gemm_epilogue_matrix_gpu.py,
   test_value_ranges_gpu.py); nothing here invents a tolerance;
2. tiled-image identity: the same launcher run UNWRAPPED on the input repeated three times along each wrapped axis, centre crop -
   bit for bit where lb_conv_plan names the same route, tile and split for both launches, inside the float64 bound otherwise;
3. memory: the input lies between guard bands of NaN (``_guard``), so a read outside the image - the element-offset neighbour a
   missing mask gives for free is inside the image and is caught by 1. and 2. instead - shows up as a NaN; the output's guard
   bands must stay intact and every element of the result must have been stored.

No real checkpoint is available to these tests: what is held is the mathematical property, not how good a tiled picture looks.
"""
import ctypes as C
import dataclasses
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _tileable_ref as T  # noqa: E402
from _guard import guarded  # noqa: E402
from _ksplit import guarded_workspace, nhwc_dev  # noqa: E402
from _parity import U16, U32, activation_bound, check_elementwise, contraction_bound, rnd  # noqa: E402
from _value_kinds import gemm_mode  # noqa: E402

DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
WRAPS = [1, 2, 3]


def lib():
    from latentblending_amd.hip import lib as l
    return l


def ops():
    from latentblending_amd.hip import ops as o
    return o


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


# ------------------------------------------------------------------------------------------------------------ one launch
def conv_block(x, w, out, *, wrap=0, stride=1, ups=0, parity=None, flags=0, bias=None, residual=None):
    """LbGemmParams of one conv over the device view x [B, H, W, Cin] (pixel stride = ldx): 3x3 / pad 1, or the sub-pixel form."""
    l = lib()
    B, H, W, Cin = x.shape
    if parity is None:
        g = l.ConvGeom.conv3x3(H, W, Cin, stride=stride, ups=ups, ldx=x.stride(2), wrap=wrap)
    else:
        g = l.ConvGeom.subpixel(H, W, Cin, parity, ldx=x.stride(2), wrap=wrap)
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    return l.gemm_params(A=x.data_ptr(), W=w.data_ptr(), C=out.data_ptr(), M=g.M(B), N=w.shape[-2], K=g.K, ldw=w.stride(-2),
                         ldc=out.stride(0), conv=g, bias=ptr(bias), residual=ptr(residual), ldr=0 if residual is None else residual.stride(0),
                         flags=flags, zero_page=ops().zero_page(DEV).data_ptr())


def plan_key(p):
    pl = lib().conv_plan(p)
    # (a K-split launch cuts its tiles where its unit count and grid put the cuts: two launches split alike only with the same units)
    return (pl.route, pl.tile, pl.splitk, pl.halo_kind, pl.halo_tile_w, pl.ksplit_split, pl.ksplit_units if pl.ksplit_split else 0)


def launch_guarded(x_cpu, w, *, rows, n, route, prepare=None, out_f32=False, **kw):
    """One launch through lb_gemm_f16 of the conv ``conv_block(x, w, out, **kw)`` with x between NaN guard bands and the output
    between sentinel guard bands -> (result [rows, n] on the CPU, plan key).  ``route``: what lb_conv_plan must answer first.
    ``prepare(p)``: last changes to the block (a workspace, a GroupNorm table) before it is planned and launched."""
    x, xg = nhwc_dev(x_cpu, ldx=x_cpu.shape[-1])            # (dense rows: the guards are the bands in front of and behind the image)
    out, og = guarded(rows, n, n, F32 if out_f32 else F16, DEV)
    p = conv_block(x, w, out, **kw)
    keep = prepare(p) if prepare is not None else None
    key = plan_key(p)
    assert key[0] == route, f"lb_conv_plan routes the launch to {key[0]}, the case is about route {route}"
    lib().api.lb_gemm_f16(C.byref(p), stream())
    torch.cuda.synchronize()
    del keep
    xg.assert_intact("input")
    og.assert_intact("output")
    og.assert_fully_written("output")
    return out.cpu().clone(), key


def hold(log, name, x, w, ref_fn, absref_fn, wrap, out_hw, *, terms, bias=None, tiled_hw=None, **kw):
    """The three checks of one case.  ``ref_fn(x64 NCHW, w64-ish) -> NCHW float64`` is the circular reference of the conv."""
    B, H, W, Cin = x.shape
    Ho, Wo = out_hw
    n = w.shape[-2]
    wd = w.to(DEV)
    bd = None if bias is None else bias.to(DEV)
    got, key = launch_guarded(x, wd, rows=B * Ho * Wo, n=n, wrap=wrap, bias=bd, **kw)
    got = got.view(B, Ho, Wo, n)
    x64 = x.double().permute(0, 3, 1, 2)
    ref = ref_fn(x64).permute(0, 2, 3, 1)
    ad = absref_fn(x64.abs()).permute(0, 2, 3, 1)
    if bias is not None:
        ref = ref + bias.double()
    bound = contraction_bound(None, None, terms, ref, out_f32=kw.get("out_f32", False), bias=bias, absdot64=ad)
    assert bool(torch.isfinite(got).all()), f"{name}: a NaN in the result: the kernel read outside the image"
    check_elementwise(log, name + "_f64", got, ref, bound)
    # the same launcher, unwrapped, on the tiled image
    xt = T.tile3(x, wrap, dims=(1, 2))
    Bt, Ht, Wt, _ = xt.shape
    Hto, Wto = (Ht * Ho) // H, (Wt * Wo) // W
    tiled, tkey = launch_guarded(xt, wd, rows=Bt * Hto * Wto, n=n, wrap=0, bias=bd, **kw)
    tiled = T.centre(tiled.view(Bt, Hto, Wto, n), wrap, Ho, Wo, dims=(1, 2))
    if tkey == key:
        assert torch.equal(bits(got), bits(tiled)), f"{name}: differs from the unwrapped launch on the tiled image (same plan {key}: bit for bit)"
    else:
        check_elementwise(log, name + "_tiled", tiled, ref, bound)
        check_elementwise(log, name + "_vs_tiled", got, tiled.double(), 2 * bound)


def operands(B, H, W, cin, n, seed, ks=3):
    x = rnd(B, H, W, cin, seed=seed)
    w = rnd(n, cin, ks, ks, seed=seed + 1, scale=(cin * ks * ks) ** -0.5)
    return x, w, rnd(n, seed=seed + 2, dtype=F32)


def conv3_refs(w, wrap, stride=1, ups=0):
    w64 = w.double()
    return (lambda x: T.circ_conv(x, w64, None, wrap, stride, ups)), (lambda x: T.circ_conv(x, w64.abs(), None, wrap, stride, ups))


@pytest.fixture
def halo_always():
    api = lib().api
    api.lb_gemm_set_halo(2)         # every eligible conv on its halo-style kernel, whatever the grid
    yield api
    api.lb_gemm_set_halo(1)
    api.lb_conv_halo_set_ksplit(1, 0)
    api.lb_conv_halo_set_gn_a(1, 0)


# ------------------------------------------------------------------------------------------------------------ halo, plain
# (B, H, W, Cin, N): one tile whose halo wraps onto itself, two tiles along x / y, four tiles; Cin 128 = a chunk change, N 128
HALO_PLAIN = [(2, 16, 16, 64, 64), (2, 16, 32, 128, 64), (2, 32, 16, 64, 128), (2, 32, 32, 128, 128)]


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("shape", HALO_PLAIN, ids=lambda s: "x".join(map(str, s)))
def test_halo_plain(shape, wrap, halo_always, results_log):
    B, H, W, cin, n = shape
    x, w, bias = operands(B, H, W, cin, n, 11 + H + W + cin)
    r, a = conv3_refs(w, wrap)
    hold(results_log, f"tile_halo_{'x'.join(map(str, shape))}_w{wrap}", x, ops().pack_conv_weight(w, cin), r, a, wrap, (H, W), terms=9 * cin,
         bias=bias, route=lib().ROUTE_HALO3)


@functools.lru_cache(maxsize=None)
def multi_tile_operands():
    return operands(2, 192, 192, 64, 64, 97)


@pytest.mark.parametrize("wrap", WRAPS)
def test_halo_block_walks_several_tiles(wrap, halo_always, results_log):
    """288 items on at most 256 persistent blocks: some blocks set the offsets of a SECOND tile, on the path inside the tile loop.
    All three checks, like every other case."""
    B, H, W, cin, n = 2, 192, 192, 64, 64
    x, w, bias = multi_tile_operands()
    pl = lib().conv_plan(lib().conv_probe(B, H, W, cin, n, 3, wrap=wrap, zero_page=ops().zero_page(DEV).data_ptr()))
    assert pl.route == lib().ROUTE_HALO3 and pl.halo_items > pl.halo_grid, (pl.halo_items, pl.halo_grid)
    r, a = conv3_refs(w, wrap)
    hold(results_log, f"tile_halo_multi_tile_w{wrap}", x, ops().pack_conv_weight(w, cin), r, a, wrap, (H, W), terms=9 * cin, bias=bias,
         route=lib().ROUTE_HALO3)


# ------------------------------------------------------------------------------------------------------------ halo, ragged
@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("hw", [(24, 40), (40, 24)], ids=lambda s: "x".join(map(str, s)))
def test_halo_ragged(hw, wrap, halo_always, results_log):
    H, W = hw
    B, cin, n = 2, 64, 64
    x, w, bias = operands(B, H, W, cin, n, 31 + H)
    r, a = conv3_refs(w, wrap)

    def check_ragged(p):
        assert lib().conv_plan(p).halo_kind == 3

    hold(results_log, f"tile_halo_ragged_{H}x{W}_w{wrap}", x, ops().pack_conv_weight(w, cin), r, a, wrap, (H, W), terms=9 * cin, bias=bias,
         route=lib().ROUTE_HALO3, flags=lib().GEMM_HALO_RAGGED, prepare=check_ragged)


# ------------------------------------------------------------------------------------------------------------ halo, K-split
@pytest.mark.parametrize("wrap", WRAPS)
def test_halo_ksplit(wrap, halo_always, results_log):
    """tests/_ksplit.py's smallest shape (4 x 16 x 32, Cin 128, 16 units on a forced grid of 3 blocks: cut tiles)."""
    B, H, W, cin, n = 4, 16, 32, 128, 128
    halo_always.lb_conv_halo_set_ksplit(2, 3)
    x, w, bias = operands(B, H, W, cin, n, 301)
    r, a = conv3_refs(w, wrap)
    state = {}

    def with_workspace(p):
        p.flags |= lib().GEMM_HALO_KSPLIT
        ws, guard, counters = guarded_workspace(p)
        p.partial = ws.data_ptr()
        assert lib().conv_plan(p).ksplit_split == 1
        state["ws"] = (ws, guard, counters)
        return ws

    hold(results_log, f"tile_halo_ksplit_w{wrap}", x, ops().pack_conv_weight(w, cin), r, a, wrap, (H, W), terms=9 * cin, bias=bias,
         route=lib().ROUTE_HALO3, prepare=with_workspace)
    ws, guard, counters = state["ws"]
    guard.assert_intact("K-split workspace")
    assert int(ws[0, :counters].view(torch.int32).abs().max()) == 0, "the kernel must leave its counters zero"


# ------------------------------------------------------------------------------------------------------------ GroupNorm on A
def gn_table(B, cin, seed):
    """A [B][Cin] float2 (scale, shift) table as lb_groupnorm_affine_from_stats leaves it (any affine map will do here)."""
    t = torch.stack([1.0 + 0.25 * rnd(B, cin, seed=seed, dtype=F32), 0.5 * rnd(B, cin, seed=seed + 1, dtype=F32)], -1)
    return t.contiguous()


def gn_operand64(x, table):
    """What the flagged kernels multiply, f16(silu(fma(x, scale, shift))), in float64 [B, H, W, C], and the bound ``dn`` of the
    kernel's fp16 operand against it, built as tests/test_halo_gn_gpu.py builds it (reference64): the error of the pre-activation
    value - here the table is GIVEN in fp32, so only the map's own fp32 roundings count: the product, the shift, the sum - through
    ``_parity.activation_bound`` (Lipschitz 1.13, exp / rcp, the fp16 store)."""
    sc, sh = table[:, None, None, :, 0].double(), table[:, None, None, :, 1].double()
    t = x.double() * sc + sh
    n = t * torch.sigmoid(t)
    pre = U32 * ((x.double() * sc).abs() + sh.abs() + t.abs())
    return n, activation_bound(pre, n)


def hold_gn(log, name, x, w, wrap, *, route, bias, out_f32=False, gn_grid=0):
    """A flagged (LB_GEMM_GN_A) wrapped launch: 2. and 3. as everywhere; 1. against the float64 conv of the float64 map inside the
    bound of the kernel's own float64 test (tests/test_halo_gn_gpu.py, the same assembly): ``contraction_bound`` with the operand's
    error ``dn`` inside |A| . |W|, plus sum_k dn_k |w_k| (1 + 2^-11)."""
    B, H, W, cin = x.shape
    n = w.shape[0]
    table = gn_table(B, cin, 555)
    td = table.to(DEV)
    wk = ops().pack_conv_weight(w, cin).to(DEV)
    bd = bias.to(DEV)

    def flag(p):
        p.flags |= lib().GEMM_GN_A
        p.gn_table, p.gn_silu = td.data_ptr(), 1
        return td

    lib().api.lb_conv_halo_set_gn_a(2, gn_grid)
    flags = lib().GEMM_OUT_F32 if out_f32 else 0
    got, key = launch_guarded(x, wk, rows=B * H * W, n=n, route=route, wrap=wrap, bias=bd, prepare=flag, out_f32=out_f32, flags=flags)
    n64, dn = gn_operand64(x, table)
    w64, nchw = w.double(), lambda t: t.permute(0, 3, 1, 2)
    ref = T.circ_conv(nchw(n64), w64, None, wrap).permute(0, 2, 3, 1) + bias.double()
    operand_err = T.circ_conv(nchw(dn), w64.abs(), None, wrap).permute(0, 2, 3, 1)
    ad = T.circ_conv(nchw(n64.abs() + dn), w64.abs(), None, wrap).permute(0, 2, 3, 1)
    bound = contraction_bound(None, None, 9 * cin, ref, out_f32=out_f32, bias=bias, absdot64=ad) + operand_err * (1 + U16)
    got = got.view(B, H, W, n)
    assert bool(torch.isfinite(got).all()), f"{name}: a NaN in the result: the kernel read outside the image"
    check_elementwise(log, name + "_f64", got, ref, bound)
    xt = T.tile3(x, wrap, dims=(1, 2))
    Bt, Ht, Wt, _ = xt.shape
    tiled, tkey = launch_guarded(xt, wk, rows=Bt * Ht * Wt, n=n, route=route, wrap=0, bias=bd, prepare=flag, out_f32=out_f32, flags=flags)
    tiled = T.centre(tiled.view(Bt, Ht, Wt, n), wrap, H, W, dims=(1, 2))
    if tkey == key:
        assert torch.equal(bits(got), bits(tiled)), f"{name}: differs from the unwrapped flagged launch on the tiled image (same plan: bit for bit)"
    else:
        check_elementwise(log, name + "_vs_tiled", got, tiled.double(), 2 * bound)


@pytest.mark.parametrize("wrap", WRAPS)
def test_halo_gn_a(wrap, halo_always, results_log):
    """Folded GroupNorm, whole tiles, with a forced grid of 2 blocks for 8 tiles: a wrapped halo piece is a real pixel and is mapped
    in LDS; the zero padding of the other axis stays zero (a mapped zero would be silu(shift) != 0 and break the float64 bound)."""
    B, H, W, cin, n = 2, 32, 32, 128, 128
    x, w, bias = operands(B, H, W, cin, n, 401)
    hold_gn(results_log, f"tile_halo_gn_a_w{wrap}", x, w, wrap, route=lib().ROUTE_HALO3, bias=bias, gn_grid=2)


# ------------------------------------------------------------------------------------------------------------ sub-pixel
@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("hw", [(16, 16), (16, 32)], ids=lambda s: "x".join(map(str, s)))
def test_subpixel_all_parities(hw, wrap, halo_always, results_log):
    H, W = hw
    B, cin, n = 2, 64, 64
    x, w3, bias = operands(B, H, W, cin, n, 61 + W)
    subs = ops().subpixel_upsample_weights(w3)
    w4 = torch.stack([subs[(0, 0)], subs[(0, 1)], subs[(1, 0)], subs[(1, 1)]]).contiguous()       # [4][N][4 Cin]

    def ref_of(fn):
        def f(x64):
            xp = T.circ_pad(x64, wrap)
            out = torch.zeros(B, n, 2 * H, 2 * W, dtype=F64)
            for i, (py, px) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
                k = fn(w4[i].double()).reshape(n, 2, 2, cin).permute(0, 3, 1, 2)
                out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], k)
            return out
        return f

    def is_upconv(p):
        assert lib().conv_plan(p).halo_kind == 2

    hold(results_log, f"tile_subpixel_{H}x{W}_w{wrap}", x, w4, ref_of(lambda t: t), ref_of(torch.abs), wrap, (2 * H, 2 * W), terms=4 * cin,
         bias=bias, route=lib().ROUTE_UPCONV_HALO, parity="all", prepare=is_upconv)


# ------------------------------------------------------------------------------------------------------------ narrow
@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("gna", [False, True], ids=["plain", "gn_a"])
@pytest.mark.parametrize("shape", [(2, 16, 16, 64, 4), (2, 32, 16, 128, 16)], ids=lambda s: "x".join(map(str, s)))
def test_narrow(shape, gna, wrap, halo_always, results_log):
    B, H, W, cin, n = shape
    x, w, bias = operands(B, H, W, cin, n, 71 + cin)
    name = f"tile_narrow_{'x'.join(map(str, shape))}_{'gna' if gna else 'plain'}_w{wrap}"
    if gna:
        hold_gn(results_log, name, x, w, wrap, route=lib().ROUTE_NARROW, bias=bias, out_f32=True)
    else:
        r, a = conv3_refs(w, wrap)
        hold(results_log, name, x, ops().pack_conv_weight(w, cin), r, a, wrap, (H, W), terms=9 * cin, bias=bias, route=lib().ROUTE_NARROW,
             flags=lib().GEMM_OUT_F32, out_f32=True)


# ------------------------------------------------------------------------------------------------------------ 64-channel
@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("case", [(16, 16, 0), (32, 16, 1), (24, 24, 0)], ids=["16x16", "32x16_ups", "24x24_overhang"])
def test_c64(case, wrap, results_log):
    H, W, ups = case
    B = 2
    x, w, bias = operands(B, H, W, 64, 64, 81 + H)
    r, a = conv3_refs(w, wrap, ups=ups)
    hold(results_log, f"tile_c64_{H}x{W}_ups{ups}_w{wrap}", x, ops().pack_conv_weight(w, 64), r, a, wrap, (H << ups, W << ups), terms=576, bias=bias,
         route=lib().ROUTE_C64, flags=lib().GEMM_C64, ups=ups)


# ------------------------------------------------------------------------------------------------------------ implicit GEMM
GEMM_CASES = {"8x8": (8, 8, 1, 0), "16x16_s2": (16, 16, 2, 0), "8x8_s2": (8, 8, 2, 0), "8x8_ups": (8, 8, 1, 1)}


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("variant", [1, 0], ids=["glds", "ring"])
@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_implicit_gemm(case, variant, wrap, results_log):
    """Both GEMM families, forced as test_gemm_epilogue_matrix_gpu.py forces them (64 x 64 tile, unsplit)."""
    H, W, stride, ups = GEMM_CASES[case]
    B, cin, n = 2, 64, 64
    x, w, bias = operands(B, H, W, cin, n, 91 + H + stride + ups)
    r, a = conv3_refs(w, wrap, stride=stride, ups=ups)
    Ho, Wo = ((H << ups) - 1) // stride + 1, ((W << ups) - 1) // stride + 1

    def forced(p):
        tile, sk = C.c_int(), C.c_int()
        lib().api.lb_gemm_plan(C.byref(p), C.byref(tile), C.byref(sk), None)
        assert (tile.value, sk.value) == (3, 1), (tile.value, sk.value)

    with gemm_mode(variant, 3, 1):
        hold(results_log, f"tile_gemm_{case}_v{variant}_w{wrap}", x, ops().pack_conv_weight(w, cin), r, a, wrap, (Ho, Wo), terms=9 * cin, bias=bias,
             route=lib().ROUTE_GEMM, stride=stride, ups=ups, prepare=forced)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_wrap_on_a_refusing_geometry_writes_nothing():
    l = lib()
    x, xg = nhwc_dev(rnd(2, 16, 16, 64, seed=5), ldx=64)
    w1 = rnd(64, 64, seed=6).to(DEV)
    out, og = guarded(2 * 16 * 16, 64, 64, F16, DEV)
    g = l.ConvGeom(16, 16, 64, 1, 1, ldx=64)
    p = l.gemm_params(A=x.data_ptr(), W=w1.data_ptr(), C=out.data_ptr(), M=g.M(2), N=64, K=g.K, ldw=64, ldc=64, conv=g,
                      zero_page=ops().zero_page(DEV).data_ptr())
    p.wrap = 1                                              # (ConvGeom refuses to build it: the block is forged)
    with pytest.raises(RuntimeError, match="wrap"):
        l.api.lb_gemm_f16(C.byref(p), stream())
    w3 = ops().pack_conv_weight(rnd(64, 64, 3, 3, seed=7), 64).to(DEV)
    for entry, wrap, flags in ((l.api.lb_conv3x3_halo_f16, 4, 0), (l.api.lb_conv3x3_narrow_f16, 8, 0), (l.api.lb_gemm_f16, 5, l.GEMM_C64)):
        q = conv_block(x, w3, out, flags=flags)
        q.wrap = wrap
        with pytest.raises(RuntimeError, match="wrap"):
            entry(C.byref(q), stream())
    torch.cuda.synchronize()
    og.assert_untouched("output of refused launches")
    xg.assert_intact("input")


# ============================================================================================================ whole programs
# Tiny configurations (oracle/sdxl_ref.py), latents 16 x 16 and 16 x 24, B = 2.  The yardstick of every property below is measured,
# never chosen: the error of the very program on the very input against the float64 circular model (``e``).  A property that
# compares two native runs (roll-equivariance) is allowed 2 e - it is the difference of two runs that each carry that error - and the
# same roll along a non-wrapped axis, or with wrap off, must exceed that allowance by a wide margin (MARGIN x), which shows that the
# test can fail: one zero-padded conv already misses by the size of its outputs (test_tileable_cpu.py).
import _model_units as MU  # noqa: E402
from oracle import sdxl_ref as R  # noqa: E402

LATENTS = [16, (16, 24)]
MARGIN = 4.0
VAE_CH = (64, 128, 128, 128)        # (as tests/test_model_units_gpu.py: 64-channel levels reach the halo-tile kernels)
AXIS = {1: 3, 2: 2}                 # wrap bit -> NCHW axis


def native():
    import latentblending_amd.native as n
    return n


def max_err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


@functools.lru_cache(maxsize=None)
def unet_net():
    n = native()
    return n.NativeUNet(n.UNetConfig(**dataclasses.asdict(R.tiny_unet_cfg())), n.SyntheticProvider(0), DEV)


@functools.lru_cache(maxsize=None)
def unet_inputs(L):
    cfg, B = R.tiny_unet_cfg(), 2
    H, W = (L, L) if isinstance(L, int) else L
    g = torch.Generator().manual_seed(2000 + H + W)
    return dict(x_in=torch.randn(B, 4, H, W, generator=g).half(), tvals=torch.full((B,), 499.0),
                ctx=torch.randn(B, 77, cfg.cross_dim, generator=g).half(), text_embeds=torch.randn(B, cfg.pooled_dim, generator=g).half(),
                time_ids=torch.tensor([[128.0, 128.0, 0.0, 0.0, 128.0, 128.0]] * B))


def unet_eps(prog, i, x=None):
    prog.set_conditioning(i["ctx"].to(DEV), i["text_embeds"].to(DEV), i["time_ids"].to(DEV))
    return prog.forward((i["x_in"] if x is None else x).to(DEV), i["tvals"]).clone().cpu()


@functools.lru_cache(maxsize=None)
def unet_run(L, wrap):
    """(program, native eps, float64 circular eps, e = their max-abs difference)."""
    i = unet_inputs(L)
    prog = unet_net().build(2, L, wrap=wrap)
    eps = unet_eps(prog, i)
    w = R.make_weights(R.unet_spec(R.tiny_unet_cfg()), 0)
    ref, _ = MU.evs(w)
    with T.circular_oracle(wrap):
        eps64 = R.unet_forward(R.tiny_unet_cfg(), ref.w, i["x_in"], torch.tensor(499.0), i["ctx"], i["text_embeds"], i["time_ids"], dtype=F64)
    return prog, eps, eps64, max_err(eps, eps64)


@pytest.mark.parametrize("wrap", [0] + WRAPS)
@pytest.mark.parametrize("L", LATENTS, ids=["16x16", "16x24"])
def test_unet_roll_equivariance(L, wrap, results_log):
    """eps(roll(x, s)) == roll(eps(x), s) on a wrapped axis for s a multiple of 2^(levels - 1) = 4, within 2 e; along every other
    axis (and on both with wrap off) the defect exceeds MARGIN x that allowance."""
    prog, eps, eps64, e = unet_run(L, wrap)
    assert rel_l2(eps, eps64) <= 1e-2, "the free-running bar of tests/test_model_units_gpu.py, against the circular float64 model"
    i = unet_inputs(L)
    figures = {"e": e}
    for bit, axis in AXIS.items():
        s = 4
        defect = max_err(unet_eps(prog, i, torch.roll(i["x_in"], s, axis)), torch.roll(eps, s, axis))
        figures[f"defect_axis{axis}"] = defect
        print(f"[tileable] unet L={L} wrap={wrap} axis={axis}: defect {defect:.3e}, e {e:.3e}, allowance {2 * e:.3e}")
        if wrap & bit:
            assert defect <= 2 * e, (L, wrap, axis, defect, e)
        else:
            assert defect > MARGIN * 2 * e, (L, wrap, axis, defect, e)
    results_log[f"tileable/unet_roll_{L}_w{wrap}"] = figures


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("L", LATENTS, ids=["16x16", "16x24"])
def test_unet_units_match_the_float64_circular_model(L, wrap, results_log):
    """Every unit with a 3x3 conv, teacher-forced with the native inputs of that unit, against the same unit in float64 with
    wrap-around padding, inside tests/_model_units.py's bound (FACTOR x the error of the storage model)."""
    prog, eps, _, _ = unet_run(L, wrap)
    cfg, i = R.tiny_unet_cfg(), unet_inputs(L)
    unet_eps(prog, i)
    taps = {k: v.cpu() if k == "eps" else (MU.nchw(v.detach().cpu()).contiguous() if v.dim() == 4 else v.detach().cpu()) for k, v in prog.capture().items()}
    torch.cuda.synchronize()
    ref, model = MU.evs(R.make_weights(R.unet_spec(cfg), 0))
    failed, seen = [], 0
    with T.circular_units(wrap):
        for name, kind, ins in MU.unet_units(cfg, False):
            if kind not in ("conv_in", "resnet", "downsample", "upsample", "out"):
                continue
            given = [i[k] if k in i else taps[k] for k in ins]
            ref64 = MU.unet_unit(ref, cfg, name, kind, given, prog.ln_mode is True)
            mod = MU.unet_unit(model, cfg, name, kind, given, prog.ln_mode is True)
            bad = MU.compare(results_log, f"tileable/unet_{L}_w{wrap}/{name}", taps[name], mod, ref64)
            seen += 1
            if bad:
                failed.append(bad)
    assert seen >= 10 and not failed, "\n".join(failed)
    assert torch.equal(taps["eps"], eps)


def test_unet_graph_replay_equals_eager():
    i = unet_inputs(16)
    prog = unet_net().build(2, 16, wrap=3)
    eager = unet_eps(prog, i)
    prog.enable_graphs()
    assert torch.equal(unet_eps(prog, i), eager) and torch.equal(eager, unet_run(16, 3)[1])


# ------------------------------------------------------------------------------------------------------------ decoders
@functools.lru_cache(maxsize=None)
def vae_run(L, wrap):
    n = native()
    cfg = R.VAECfg(block_channels=VAE_CH)
    net = n.NativeVAEDecoder(n.VAEConfig(**dataclasses.asdict(cfg)), n.SyntheticProvider(1), DEV)
    H, W = (L, L) if isinstance(L, int) else L
    z = torch.randn(2, 4, H, W, generator=torch.Generator().manual_seed(3000 + H + W)).half()
    prog = net.build(2, L, wrap=wrap)

    def image(zz):
        prog.decode(zz.to(DEV))
        return MU.nchw(prog.image_f32.detach().cpu())[:, :cfg.out_channels].contiguous().clone()
    ref, _ = MU.evs(R.make_weights(R.vae_decoder_spec(cfg), 1))
    with T.circular_oracle(wrap):
        img64 = R.vae_decode(cfg, ref.w, z.double() / cfg.scaling_factor, dtype=F64)
    img = image(z)
    return z, image, img, img64, max_err(img, img64), prog, cfg


@functools.lru_cache(maxsize=None)
def tiny_run(L, wrap):
    import _taesd_ref as TR
    n = native()
    sd = TR.synthetic_state_dict(0)
    net = n.NativeTinyVAEDecoder(n.TinyVAEConfig(), n.DictProvider(sd), DEV)
    H, W = (L, L) if isinstance(L, int) else L
    z = torch.randn(2, 4, H, W, generator=torch.Generator().manual_seed(4000 + H + W)).half()
    prog = net.build(2, L, wrap=wrap)

    def image(zz):
        prog.decode(zz.to(DEV))
        return MU.nchw(prog.image_f32.detach().cpu())[:, :3].contiguous().clone()
    with T.circular_taesd(wrap):
        img64 = TR.decode(sd, z)
    img = image(z)
    return z, image, img, img64, max_err(img, img64), prog.frames.cpu().numpy().copy(), TR.to_u8(img64).numpy()


@pytest.mark.parametrize("wrap", [0] + WRAPS)
@pytest.mark.parametrize("L", LATENTS, ids=["16x16", "16x24"])
@pytest.mark.parametrize("decoder", ["full", "tiny"])
def test_decoder_roll_equivariance(decoder, L, wrap, results_log, monkeypatch):
    """A latent rolled by ONE pixel on a wrapped axis decodes to the image rolled by 8, within 2 e; the decoded image itself lies
    at the free-running bar (rel-L2 <= 1e-2) from the float64 circular model."""
    if decoder == "tiny":           # (every 64 -> 64 conv on the LDS-resident-weights kernel, as tests/test_tiny_vae_gpu.py forces it)
        from latentblending_amd.native import tiny_vae
        monkeypatch.setattr(tiny_vae, "C64_MIN_TILES", 1)
    z, image, img, img64, e = (vae_run if decoder == "full" else tiny_run)(L, wrap)[:5]
    assert rel_l2(img, img64) <= 1e-2       # (the element-wise holds: test_vae_units_... / test_tiny_decoder_... below)
    figures = {"e": e}
    for bit, axis in AXIS.items():
        defect = max_err(image(torch.roll(z, 1, axis)), torch.roll(img, 8, axis))
        figures[f"defect_axis{axis}"] = defect
        print(f"[tileable] {decoder} decoder L={L} wrap={wrap} axis={axis}: defect {defect:.3e}, e {e:.3e}, allowance {2 * e:.3e}")
        if wrap & bit:
            assert defect <= 2 * e, (decoder, L, wrap, axis, defect, e)
        else:
            assert defect > MARGIN * 2 * e, (decoder, L, wrap, axis, defect, e)
    results_log[f"tileable/{decoder}_roll_{L}_w{wrap}"] = figures


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("L", LATENTS, ids=["16x16", "16x24"])
def test_vae_units_match_the_float64_circular_model(L, wrap, results_log):
    """Every unit of the decode program - the decoded image (``image_f32``, the ``out`` unit) included - teacher-forced with the
    native input of that unit, against the same unit in float64 with wrap-around padding, per element inside
    tests/_model_units.py's bound (FACTOR x the error of the storage model), as tests/test_model_units_gpu.py holds the
    zero-padded program."""
    z, _, img, _, _, prog, cfg = vae_run(L, wrap)
    prog.decode(z.to(DEV))
    taps = {k: (MU.nchw(v.detach().cpu()).contiguous() if v.dim() == 4 else v.detach().cpu()) for k, v in prog.capture().items()}
    torch.cuda.synchronize()
    taps["image_f32"] = taps["image_f32"][:, :cfg.out_channels].contiguous()
    assert torch.equal(taps["image_f32"], img)
    one = "lb_attn_fwd_d512" in prog.prog.op_names()
    ref, model = MU.evs(R.make_weights(R.vae_decoder_spec(cfg), 1))
    failed, seen = [], 0
    with T.circular_units(wrap):
        for name, kind, ins in MU.vae_units(cfg):
            given = [z if k == "z_in" else taps[k] for k in ins]
            ref64 = MU.vae_unit(ref, cfg, name, kind, given, True, one)
            mod = MU.vae_unit(model, cfg, name, kind, given, True, one)
            bad = MU.compare(results_log, f"tileable/vae_{L}_w{wrap}/{name}", taps[name], mod, ref64)
            seen += 1
            if bad:
                failed.append(bad)
    assert seen == len(MU.vae_units(cfg)) >= 15 and not failed, "\n".join(failed)


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("L", LATENTS, ids=["16x16", "16x24"])
def test_tiny_decoder_matches_the_float64_circular_restatement(L, wrap, results_log, monkeypatch):
    """The tiny decoder has no unit model; its float64 test (tests/test_tiny_vae_gpu.py) holds the decode to the float64 restatement
    at three bars - image rel-L2 <= 1e-2, mean |du8| <= 2, >= 99 % of the bytes within 4.  The same bars against the restatement
    with wrap-around padding."""
    import numpy as np
    from latentblending_amd.native import tiny_vae
    monkeypatch.setattr(tiny_vae, "C64_MIN_TILES", 1)
    _, _, img, img64, _, got_u8, ref_u8 = tiny_run(L, wrap)
    d = np.abs(got_u8.astype(np.int32) - ref_u8.astype(np.int32))
    r = rel_l2(img, img64)
    results_log[f"tileable/tiny_{L}_w{wrap}"] = {"rel_l2": r, "mean_abs_u8": float(d.mean()), "frac_within_4": float((d <= 4).mean())}
    print(f"[tileable] tiny decoder L={L} wrap={wrap}: rel_l2={r:.3e} mean|du8|={d.mean():.3f} within4={(d <= 4).mean():.4f}")
    assert r <= 1e-2 and d.mean() <= 2 and (d <= 4).mean() >= 0.99


# ------------------------------------------------------------------------------------------------------------ pipe, engine, replay
def make_pipe(**kw):
    n = native()
    return n.NativeSDXLPipe(turbo=True, unet_cfg=n.UNetConfig(**dataclasses.asdict(R.tiny_unet_cfg())),
                            vae_cfg=n.VAEConfig(**dataclasses.asdict(R.tiny_vae_cfg())), seed=0, allow_synthetic=True, **kw)


def pipe_outputs(p, L=16):
    i = unet_inputs(L)
    eps = unet_eps(p.unet_program(2, L), i)
    frames = p.vae_program(2, L).decode(i["x_in"].to(DEV)).clone().cpu()
    return eps, frames


def test_pipe_setting_switches_programs_and_back():
    fresh = pipe_outputs(make_pipe())
    p = make_pipe()
    assert p.tileable == "" and p.unet_program(2, 16).wrap == 0
    out = {}
    for setting in ("xy", "x", "y"):
        p.tileable = setting
        assert not p._unet_programs and not p._vae_programs and not p._tiny_vae_programs
        out[setting] = pipe_outputs(p)
        assert p.unet_program(2, 16).wrap == p.vae_program(2, 16).wrap == {"x": 1, "y": 2, "xy": 3}[setting]
        assert list(p._unet_programs) == [(2, 16)], "cache keys stay (B, L)"
    p.tileable = None
    back = pipe_outputs(p)
    assert torch.equal(back[0], fresh[0]) and torch.equal(back[1], fresh[1])
    for a, b in (("x", "y"), ("x", "xy"), ("y", "xy")):
        assert not torch.equal(out[a][0], out[b][0]) and not torch.equal(out[a][1], out[b][1])
    for setting in out:
        assert not torch.equal(out[setting][0], fresh[0]) and not torch.equal(out[setting][1], fresh[1])
    built = pipe_outputs(make_pipe(tileable="xy"))
    assert torch.equal(built[0], out["xy"][0]) and torch.equal(built[1], out["xy"][1])
    p.decoder = "tiny"
    p.tileable = True
    assert p.tileable == "xy" and p.vae_program(2, 16).wrap == 3 and isinstance(p.vae_program(2, 16), native().TinyVAEProgram)


def run_short_transition(p):
    import numpy as np
    from latentblending_amd import BlendingEngine
    np.random.seed(0)
    be = BlendingEngine(p, verbose=False)
    be.set_dimensions((64, 64))
    be.set_num_inference_steps(2)
    be.set_branching(depth_strength=0.5, nmb_max_branches=1)        # (turbo: one mid branch = 3 frames)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    return be, [np.asarray(f) for f in be.run_transition(fixed_seeds=[420, 421])]


def test_short_transition_and_replay_under_tileable():
    import numpy as np
    be0, plain = run_short_transition(make_pipe())
    p = make_pipe(tileable="xy")
    be, tiled = run_short_transition(p)
    assert set(be.get_state_dict()) == set(be0.get_state_dict()), "get_state_dict keeps its key set"
    assert len(tiled) == len(plain) == 3 and all(f.shape == (64, 64, 3) and f.dtype == np.uint8 for f in tiled)
    assert all(not np.array_equal(a, b) for a, b in zip(tiled, plain))
    assert all(prog.wrap == 3 for cache in (p._unet_programs, p._vae_programs) for prog in cache.values())
    # the replay driver takes the setting for the length of a chain and puts the pipe's own back
    from latentblending_amd import replay
    p.tileable = "y"
    seen = []
    segs = replay.run_multi_transition(be, ["photo of a reef", "rendering of an alien planet"], [420, 421], tileable="x",
                                       on_segment=lambda k, frames: seen.append(p.tileable))
    assert seen == ["x"] and p.tileable == "y" and len(segs) == 1 and len(segs[0]) == 3
    from latentblending_amd.utils import tile_preview
    mosaic = tile_preview(tiled[0])
    assert mosaic.shape == (128, 128, 3)
