"""Which VALUES go through the K-split form of the 3x3 halo-tile conv (LB_GEMM_HALO_KSPLIT, csrc/conv3_halo.hip), and through which
doors: every launch here runs under lb_conv_halo_set_ksplit(2, grid) and is held as tests/test_value_ranges_gpu.py holds the other
contractions - a float64 F.conv2d, element by element, under the derived bounds of tests/_parity.py (contraction_bound covers any
summation order, so the re-association of the chunk sums needs no allowance), or exact equality.

A  split launches against fp64: value kinds x shapes (up to 20 contributors to one tile; the default grid), the epilogues the models
   run split (fp32 residual stream, ReLU, padded leading dimensions), exact integers, the distance to the unsplit kernel (gated),
   the fp16 edge of the store, power-of-two rescaling (bitwise), the epilogue switches.
B  slabs rewritten between launches: two operand sets alternating on ONE workspace - a last arriver that summed a slab of the
   launch before would show.
C  the router: lb_gemm_f16 takes a flagged conv to the halo kernel as the direct entry does, and runs a flagged conv it routes
   elsewhere without ever touching ``partial``.

tests/test_halo_ksplit_cpu.py checks that the walks of the shapes have the features their names promise."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _guard import guarded  # noqa: E402
from _ksplit import (DEV, F16, F32, SHAPES, conv_params, counters_zero, forced_split, guarded_workspace, ksplit_plan, launch, lib,  # noqa: E402,F401
                     nhwc_dev, run_conv)
from _parity import accumulate_bound, activation_bound, check_elementwise, contraction_bound, epilogue_bound, rnd  # noqa: E402
from test_value_ranges_gpu import EDGE_HI, EDGE_LO, _assert_scaled, _check_edge, _conv_operands, _nchw64, _pow2, banded  # noqa: E402

F64 = torch.float64
NAN = float("nan")


def _pack(w):
    from latentblending_amd.hip import ops as o
    return o.pack_conv_weight(w, w.shape[1]).to(DEV)


def _conv64(x, w):
    """(fp64 conv, the same conv of the absolute values), NHWC, from the fp16 operands the kernel reads."""
    base = F.conv2d(_nchw64(x), w.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    ad = F.conv2d(_nchw64(x).abs(), w.double().abs(), padding=1).permute(0, 2, 3, 1).contiguous()
    return base, ad


def _shape(shape):
    B, H, W, Cin, N, _ = SHAPES[shape]
    return B, H, W, Cin, N, B * H * W


@functools.lru_cache(maxsize=None)
def value_case(shape, kind):
    """Operands of one (shape, value kind) as _conv_operands builds them, on the CPU and on the device, and their fp64 convs:
    computed once, shared, never modified."""
    B, H, W, Cin, N, M = _shape(shape)
    seed = 700 + 40 * sorted(SHAPES).index(shape)
    x, w = _conv_operands(kind, (B, H, W, Cin), N, seed)
    base, ad = _conv64(x, w)
    bias, res, rowvec = rnd(N, seed=seed + 10, dtype=F32), rnd(B, H, W, N, seed=seed + 11), rnd(B, N, seed=seed + 12)
    return dict(x=x, w=w, bias=bias, res=res, rowvec=rowvec, base=base, ad=ad, K=9 * Cin, xd=nhwc_dev(x)[0], wd=_pack(w), bd=bias.to(DEV),
                rd=res.reshape(M, N).to(DEV), rvd=rowvec.to(DEV))


# ------------------------------------------------------------------ A.1 / A.4 value kinds x shapes, against fp64 and against the unsplit kernel
VALUE_CASES = [(s, k) for s in ("tail_whole_head", "three_sharers", "one_unit_per_block") for k in ("normal", "outliers", "sub_a", "sub_w")]
VALUE_CASES += [("default_grid", "normal"), ("default_grid", "outliers")]


def _value_launch(shape, kind, split):
    """Subnormal operands run bare (as test_conv_elementwise), the others with bias + fp16 residual -> (result, reference, bound)."""
    c = value_case(shape, kind)
    B, H, W, Cin, N, M = _shape(shape)
    bare = kind.startswith("sub")
    bias, res = (torch.zeros_like(c["bias"]), None) if bare else (c["bias"], c["res"])
    ref = c["base"] + bias.double() + (0 if res is None else res.double())
    got = run_conv(c["xd"], c["wd"], split=split, bias=bias.to(DEV), residual=None if bare else c["rd"])
    bound = contraction_bound(None, None, c["K"], ref, bias=bias, residual=res, absdot64=c["ad"])
    return got.view(B, H, W, N), ref, bound


@pytest.mark.parametrize("shape,kind", VALUE_CASES)
def test_split_conv_elementwise(shape, kind, forced_split, results_log):
    forced_split(shape)
    B, H, W, Cin, N, M = _shape(shape)
    c = value_case(shape, kind)
    units, grid, split = ksplit_plan(conv_params(c["xd"], c["wd"], torch.empty(1, N, dtype=F16, device=DEV), ksplit=True))
    assert split == 1 and units == (M // 256) * ((N + 127) // 128) * (Cin // 64)
    if shape == "default_grid":                          # one block per CU, more units than blocks
        assert grid == torch.cuda.get_device_properties(0).multi_processor_count and units > grid
    else:
        assert grid == SHAPES[shape][5]
    got, ref, bound = _value_launch(shape, kind, True)
    check_elementwise(results_log, f"ksv_{shape}_{kind}", got, ref, bound)
    if kind.startswith("sub"):                           # a flushed input would store zeros the reference does not have
        assert int((got.cpu() == 0).sum()) == int((ref.half() == 0).sum())


@pytest.mark.parametrize("shape", ["tail_whole_head", "three_sharers", "one_unit_per_block", "default_grid"])
def test_split_against_unsplit(shape, forced_split, results_log):
    """Both kernels lie within ``bound`` of the fp64 value, so within 2 * bound of each other, element by element."""
    forced_split(shape)
    got, ref, bound = _value_launch(shape, "normal", True)
    plain, _, _ = _value_launch(shape, "normal", False)
    d = (got.double() - plain.double()).abs().cpu()
    name = f"ksv_{shape}_normal_vs_unsplit"
    results_log[name] = {"max_abs": float(d.max()), "differing": int((d != 0).sum()), "elements": d.numel(),
                         "worst_diff_over_2bound": float((d / (2 * bound)).max())}
    print(f"[parity] {name}: max_abs={float(d.max()):.3e}, {int((d != 0).sum())} of {d.numel()} elements differ, "
          f"worst diff / (2 bound) = {float((d / (2 * bound)).max()):.3f}")
    assert bool(torch.isfinite(plain).all()) and bool((d <= 2 * bound).all())


# ------------------------------------------------------------------ A.2 the epilogues the models run split
@pytest.mark.parametrize("epi", ["res_alpha", "rowvec", "f32", "relu", "padded"])
@pytest.mark.parametrize("shape", ["tail_whole_whole", "three_sharers"])
def test_split_epilogues_elementwise(shape, epi, forced_split, results_log):
    """res_alpha: bias + fp16 residual + alpha 0.5; rowvec: bias + row vector; f32: LB_GEMM_OUT_F32 | LB_GEMM_RES_F32 with an fp32
    residual of scale 100 (the VAE's residual stream); relu: LB_GEMM_RELU; padded: ldc = ldr = N + 8, ldx = Cin + 8, all three
    inside guarded buffers."""
    forced_split(shape)
    l = lib()
    B, H, W, Cin, N, M = _shape(shape)
    c = value_case(shape, "normal")
    x, w, bias, base, ad, K = c["xd"], c["wd"], c["bias"], c["base"], c["ad"], c["K"]
    name = f"ksv_epi_{shape}_{epi}"
    if epi == "res_alpha":
        got = run_conv(x, w, bias=c["bd"], residual=c["rd"], alpha=0.5)
        ref = 0.5 * base + bias.double() + c["res"].double()
        bound = contraction_bound(None, None, K, ref, alpha=0.5, bias=bias, residual=c["res"], absdot64=ad)
    elif epi == "rowvec":
        rows = c["rowvec"].double()[:, None, None, :].expand(B, H, W, N)
        got = run_conv(x, w, bias=c["bd"], rowvec=c["rvd"])
        ref = base + bias.double() + rows
        bound = contraction_bound(None, None, K, ref, bias=bias, rowvec=rows, absdot64=ad)
    elif epi == "f32":
        res32 = rnd(B, H, W, N, seed=741, dtype=F32, scale=100.0)
        got = run_conv(x, w, bias=c["bd"], residual=res32.reshape(M, N).to(DEV), flags=l.GEMM_OUT_F32 | l.GEMM_RES_F32)
        assert got.dtype == F32
        ref = base + bias.double() + res32.double()
        bound = contraction_bound(None, None, K, ref, out_f32=True, bias=bias, residual=res32, absdot64=ad)
    elif epi == "relu":
        got = run_conv(x, w, bias=c["bd"], flags=l.GEMM_RELU)
        y = base + bias.double()
        ref = F.relu(y)
        bound = activation_bound(accumulate_bound(ad, K) + epilogue_bound(y, bias), ref)
    else:
        xp, x_guard = nhwc_dev(c["x"], ldx=Cin + 8)
        rp, r_guard = guarded(M, N, N + 8, F16, DEV)
        rp.copy_(c["rd"])
        out, out_guard = guarded(M, N, N + 8, F16, DEV)
        got = run_conv(xp, w, out=out, bias=c["bd"], residual=rp)
        out_guard.assert_intact(name + " output")
        out_guard.assert_fully_written(name + " output")
        x_guard.assert_intact(name + " input")
        r_guard.assert_intact(name + " residual")
        assert torch.equal(xp, c["xd"]) and torch.equal(rp, c["rd"]), "an operand was written"
        ref = base + bias.double() + c["res"].double()
        bound = contraction_bound(None, None, K, ref, bias=bias, residual=c["res"], absdot64=ad)
    check_elementwise(results_log, name, got.reshape(B, H, W, N), ref, bound)


# ------------------------------------------------------------------ A.3 exact integers
@pytest.mark.parametrize("shape", ["three_sharers", "one_unit_per_block"])
def test_split_conv_of_small_integers_is_exact(shape, forced_split):
    """x in {-2 .. 2}, w in {-1, 0, 1}, zero bias: every partial sum is an integer far below 2^24, so every summation order gives
    the same fp32 value, and every result is exact in fp16: split, unsplit and the rounded reference agree bit for bit."""
    forced_split(shape)
    B, H, W, Cin, N, M = _shape(shape)
    g = torch.Generator().manual_seed(751)
    x = torch.randint(-2, 3, (B, H, W, Cin), generator=g).to(F16)
    w = torch.randint(-1, 2, (N, Cin, 3, 3), generator=g).to(F16)
    ref, ad = _conv64(x, w)
    # (what makes the test exact, asserted on the reference: three_sharers has max |ref| = 272, max |x| . |w| = 2528)
    assert float(ad.max()) < 2.0 ** 24 and torch.equal(ref.half().double(), ref) and float(ref.abs().max()) > 64
    xd, wd, bias = nhwc_dev(x)[0], _pack(w), torch.zeros(N, dtype=F32, device=DEV)
    want = ref.half().reshape(M, N)
    got, plain = run_conv(xd, wd, bias=bias).cpu(), run_conv(xd, wd, split=False, bias=bias).cpu()
    assert torch.equal(plain, want), f"unsplit: {int((plain != want).sum())} of {M * N} integer results are wrong"
    assert torch.equal(got, want), f"split: {int((got != want).sum())} of {M * N} integer results are wrong"


# ------------------------------------------------------------------ A.5 the fp16 edge of the store
def test_split_conv_store_at_the_fp16_edge(results_log):
    """The construction of test_halo_conv_store_at_the_fp16_edge on (4, 16, 32, 128, 128) over 3 blocks: channel 7 carries the
    outliers, its centre tap is +-29.297, image row 5 of sample 0 holds 2048 there (+-60000), row 9 of sample 1 holds 2390
    (+-70020)."""
    l = lib()
    x, _ = _conv_operands("outliers", (4, 16, 32, 128), 128, 543)
    w = rnd(128, 128, 3, 3, seed=544, scale=(9 * 128) ** -0.5)
    w[:, 7] = 0
    w[:, 7, 1, 1] = (29.297 * (1.0 - 2.0 * (torch.arange(128) % 2))).to(F16)
    x[0, 5, :, 7], x[1, 9, :, 7] = EDGE_LO, EDGE_HI
    ref, ad = _conv64(x, w)
    xd, wd, bias = nhwc_dev(x)[0], _pack(w), torch.zeros(128, dtype=F32, device=DEV)
    l.api.lb_conv_halo_set_ksplit(2, 3)
    try:
        got16 = run_conv(xd, wd, bias=bias).view(4, 16, 32, 128)
        got32 = run_conv(xd, wd, bias=bias, flags=l.GEMM_OUT_F32).view(4, 16, 32, 128)
    finally:
        l.api.lb_conv_halo_set_ksplit(1, 0)
    _check_edge(results_log, "ksv_edge", got16, got32, ref, contraction_bound(None, None, 1152, ref, absdot64=ad))
    check_elementwise(results_log, "ksv_edge_f32", got32, ref, contraction_bound(None, None, 1152, ref, out_f32=True, absdot64=ad))


# ------------------------------------------------------------------ A.6 exact rescaling, bitwise
@functools.lru_cache(maxsize=None)
def banded_case(shape):
    B, H, W, Cin, N, M = _shape(shape)
    x, w = _conv_operands("banded", (B, H, W, Cin), N, 760)
    bias, res = rnd(N, seed=761, dtype=F32), banded((B, H, W, N), -2, 2, 555)
    return dict(x=x, w=w, bias=bias, res=res, ref=_conv64(x, w)[0] + bias.double() + res.double())


@pytest.mark.parametrize("a,b", [(4, -4), (3, 3)])
@pytest.mark.parametrize("shape", ["tail_whole_whole", "three_sharers"])
def test_split_conv_pow2_rescale_bitwise(shape, a, b, forced_split, results_log):
    """C(2^a x, 2^b w, 2^(a+b) bias, 2^(a+b) residual) == 2^(a+b) C(x, w, bias, residual) bit for bit: the slabs are summed in a
    fixed order, so the split kernel commutes with a power of two as the unsplit one does."""
    forced_split(shape)
    B, H, W, Cin, N, M = _shape(shape)
    c = banded_case(shape)
    assert float(c["ref"].abs().max()) * 2.0 ** (a + b) < 60000

    def run(x, w, bias, res):
        return run_conv(nhwc_dev(x)[0], _pack(w), bias=bias.to(DEV), residual=res.reshape(M, N).to(DEV))

    base = run(c["x"], c["w"], c["bias"], c["res"])
    scaled = run(_pow2(c["x"], a), _pow2(c["w"], b), _pow2(c["bias"], a + b), _pow2(c["res"], a + b))
    _assert_scaled(f"ksv_pow2_{shape}_a{a}b{b}", base, scaled, 2.0 ** (a + b), c["ref"].reshape(M, N), a + b == 0, results_log)


# ------------------------------------------------------------------ A.7 the epilogue switches
@pytest.mark.parametrize("switch", ["lb_gemm_set_lean_epilogue", "lb_gemm_set_wide_store"])
@pytest.mark.parametrize("epi", ["plain", "res"])
def test_split_conv_under_the_epilogue_switches(epi, switch, forced_split):
    """The per-row epilogue and the 8-byte stores give the bits of the defaults, split as unsplit."""
    shape = "tail_whole_head"
    forced_split(shape)
    c = value_case(shape, "normal")
    kw = dict(bias=c["bd"]) if epi == "plain" else dict(bias=c["bd"], residual=c["rd"], alpha=0.5)
    want = run_conv(c["xd"], c["wd"], **kw)
    try:
        getattr(lib().api, switch)(0)
        got = run_conv(c["xd"], c["wd"], **kw)
    finally:
        lib().api.lb_gemm_set_lean_epilogue(1)
        lib().api.lb_gemm_set_wide_store(1)
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want)


# ------------------------------------------------------------------ B. slabs rewritten between launches
@functools.lru_cache(maxsize=None)
def second_case(shape):
    """Q: other operands at three times the scale of P = value_case(shape, "normal")."""
    B, H, W, Cin, N, M = _shape(shape)
    x, w = rnd(B, H, W, Cin, seed=771, scale=3.0), rnd(N, Cin, 3, 3, seed=772, scale=(9 * Cin) ** -0.5)
    base, ad = _conv64(x, w)
    return dict(x=x, w=w, base=base, ad=ad, xd=nhwc_dev(x)[0], wd=_pack(w))


@pytest.mark.parametrize("shape", ["three_sharers", "one_unit_per_block"])
def test_slabs_are_rewritten_between_launches(shape, forced_split, results_log):
    """In a program the slabs are shared by different convs, launch after launch.  P, Q, P, Q, P, Q on one workspace and one
    stream without a host synchronisation in between, then a recorded launch whose operands are overwritten in place between graph
    launches: every result equals the one its operands give on a fresh workspace - which is held to fp64 first."""
    from latentblending_amd.native.runtime import Program
    forced_split(shape)
    B, H, W, Cin, N, M = _shape(shape)
    P, Q = value_case(shape, "normal"), second_case(shape)
    bias_cpu, bias = P["bias"], P["bd"]
    fresh = {}
    for tag, c in (("P", P), ("Q", Q)):
        fresh[tag] = run_conv(c["xd"], c["wd"], bias=bias)
        ref = c["base"] + bias_cpu.double()
        check_elementwise(results_log, f"ksv_slabs_{shape}_{tag}", fresh[tag].view(B, H, W, N), ref,
                          contraction_bound(None, None, 9 * Cin, ref, bias=bias_cpu, absdot64=c["ad"]))
    assert not torch.equal(fresh["P"], fresh["Q"])

    ws, ws_guard, counter_floats = guarded_workspace(conv_params(P["xd"], P["wd"], fresh["P"], bias=bias, ksplit=True))
    outs = [torch.full((M, N), NAN, dtype=F16, device=DEV) for _ in range(6)]
    for i, out in enumerate(outs):                       # (nothing here synchronises: six launches back to back)
        c = (P, Q)[i % 2]
        run_conv(c["xd"], c["wd"], ws=ws, out=out, bias=bias)
    torch.cuda.synchronize()
    for i, out in enumerate(outs):
        assert torch.equal(out, fresh["PQ"[i % 2]]), f"launch {i} ({'PQ'[i % 2]}) on the shared workspace differs from its fresh-workspace result"
    ws_guard.assert_intact("shared workspace")
    assert counters_zero(ws, counter_floats)

    xb, wb = P["xd"].clone(), P["wd"].clone()
    rec = torch.full((M, N), NAN, dtype=F16, device=DEV)
    prog = Program(f"ksv_slabs_{shape}")
    with prog.record():
        run_conv(xb, wb, ws=ws, out=rec, bias=bias)
    assert prog.num_ops == 1 and bool(torch.isnan(rec).all()), "a recording launches nothing"
    prog.instantiate()
    seen = []
    for tag in "PQP":                                    # (stream-ordered copies and clones: no host synchronisation either)
        c = P if tag == "P" else Q
        xb.copy_(c["xd"])
        wb.copy_(c["wd"])
        prog.launch()
        seen.append(rec.clone())
    torch.cuda.synchronize()
    for tag, got in zip("PQP", seen):
        assert torch.equal(got, fresh[tag]), f"graph launch on operands {tag} differs from their fresh-workspace result"
    ws_guard.assert_intact("shared workspace")
    assert counters_zero(ws, counter_floats)


# ------------------------------------------------------------------ C. the router
@pytest.fixture
def halo_mode():
    yield lib().api.lb_gemm_set_halo
    lib().api.lb_gemm_set_halo(1)


def test_router_takes_a_flagged_conv_to_the_split_kernel(forced_split, halo_mode):
    from latentblending_amd.native.runtime import Program
    shape = "tail_whole_whole"
    forced_split(shape)
    halo_mode(2)
    B, H, W, Cin, N, M = _shape(shape)
    c = value_case(shape, "normal")
    kw = dict(bias=c["bd"], residual=c["rd"])
    ws, ws_guard, counter_floats = guarded_workspace(conv_params(c["xd"], c["wd"], c["rd"], ksplit=True, **kw))
    assert bool(torch.isnan(ws[0, counter_floats:]).all())
    routed = run_conv(c["xd"], c["wd"], ws=ws, entry="gemm", **kw)
    assert bool(torch.isfinite(ws[0, counter_floats:]).any()), "the routed launch wrote no slab: it did not split"
    direct = run_conv(c["xd"], c["wd"], ws=ws, **kw)
    assert bool(torch.isfinite(direct).all()) and torch.equal(routed, direct)
    rec = torch.full((M, N), NAN, dtype=F16, device=DEV)
    prog = Program("ksv_router")
    with prog.record():
        run_conv(c["xd"], c["wd"], ws=ws, out=rec, entry="gemm", **kw)
    assert prog.op_names() == ["lb_conv3x3_halo_f16"]
    prog.run()
    assert torch.equal(rec, direct)
    ws_guard.assert_intact("workspace")
    assert counters_zero(ws, counter_floats)


@pytest.mark.parametrize("route", ["igemm", "stride2", "narrow"])
def test_router_runs_a_flagged_conv_elsewhere_without_its_workspace(route, forced_split, halo_mode):
    """include/lb_hip.h: "A flagged conv that lb_gemm_f16 routes to another kernel runs there without split-K workspace".  The same
    3x3 conv under lb_gemm_set_halo(0) (implicit GEMM), a stride-2 conv (implicit GEMM) and an N = 4 conv (narrow-N kernel), flagged
    and with ``partial`` on a sentinel-filled buffer of the size the halo-eligible twin would need: the bits of the unflagged launch
    without ``partial``, and not one byte of the buffer touched."""
    shape = "tail_whole_whole"
    forced_split(shape)
    B, H, W, Cin, N, M = _shape(shape)
    c = value_case(shape, "normal")
    x, w, bias = c["xd"], c["wd"], c["bd"]
    stride = 2 if route == "stride2" else 1
    if route == "narrow":
        w, bias = w[:4].contiguous(), bias[:4].contiguous()
    if route == "igemm":
        halo_mode(0)
    twin = conv_params(x, w, torch.empty(1, w.shape[0], dtype=F16, device=DEV), bias=bias, ksplit=True)
    need = lib().api.lb_conv_halo_ksplit_workspace_bytes(twin)
    assert need > 0
    sentinel, guard = guarded(1, need // 4, need // 4, F32, DEV, back_rows=0)
    want = run_conv(x, w, split=False, entry="gemm", bias=bias, stride=stride)
    got = run_conv(x, w, ws=sentinel, entry="gemm", bias=bias, stride=stride)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want)
    guard.assert_untouched("the buffer behind `partial`")
    from latentblending_amd.native.runtime import Program
    prog = Program("ksv_route_" + route)
    with prog.record():
        run_conv(x, w, ws=sentinel, entry="gemm", bias=bias, stride=stride)
    assert prog.op_names() == ["lb_conv3x3_narrow_f16" if route == "narrow" else "lb_gemm_f16"]


def test_c64_refuses_a_flagged_problem_with_a_workspace(forced_split):
    """LB_GEMM_C64 | LB_GEMM_HALO_KSPLIT with ``partial`` set: that kernel or a refusal - refused, before any store."""
    forced_split("tail_whole_whole")
    x, w = rnd(1, 16, 16, 64, seed=781), rnd(64, 64, 3, 3, seed=782, scale=576 ** -0.5)
    out, out_guard = guarded(256, 64, 64, F16, DEV)
    ws, ws_guard = guarded(1, 1 << 16, 1 << 16, F32, DEV, back_rows=0)
    p = conv_params(nhwc_dev(x)[0], _pack(w), out, flags=lib().GEMM_C64, ksplit=True, ws=ws[0])
    with pytest.raises(RuntimeError):
        launch(p, "gemm")
    torch.cuda.synchronize()
    out_guard.assert_untouched("output of the refused launch")
    ws_guard.assert_untouched("workspace of the refused launch")
