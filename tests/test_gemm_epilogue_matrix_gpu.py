"""The product the other GEMM tests leave out: every epilogue of lb_gemm_f16 on every forced tile, unsplit and through split-K, and
the implicit-conv gather forms, against float64, ELEMENT BY ELEMENT, with the derived bounds of tests/_parity.py.

The tile epilogue (csrc/lb_gemm.h: lb_gemm_tile_epilogue<TM, TN> / the lean form) and the split-K reduce (lb_gemm_store4) are two
hand-maintained copies of the same arithmetic; tests/test_gemm_epilogue_matrix_cpu.py shows that the bounds used here admit a correct
fp32 implementation and reject each way the two can drift apart.  Forced tiles fall back silently (an ineligible tile 9 becomes the
automatic choice, tile >= 4 outside the direct-to-LDS family becomes tile 1), so every launch here goes through ``_launch``: it asks
lb_gemm_plan about the very parameter block it then launches and fails unless the answer is the (tile, splitk) the case names."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _gemm_epilogue_model as E  # noqa: E402
from _parity import check_elementwise, contraction_bound, rnd  # noqa: E402
from _value_kinds import DEV, _conv_operands, _nchw64, _subpixel_ref, gemm_mode, lib  # noqa: E402

F16, F32, F64 = torch.float16, torch.float32, torch.float64
M, N, K = E.M, E.N, E.K
SENTINEL = 777.0            # pre-fill of every output buffer: exact in fp16, far outside every bound of a result that was not stored

UNSPLIT, SPLIT = E.UNSPLIT, E.SPLIT        # (variant, tile, splitk)
KINDS = ["normal", "outliers"]


def ops():
    from latentblending_amd.hip import ops as o
    return o


@functools.lru_cache(maxsize=None)
def dev_case(kind):
    """The operands of E.matrix_case(kind) on the device: uploaded once, never modified."""
    c = E.matrix_case(kind)
    return {k: c[k].to(DEV) for k in ("A", "W", "bias", "res", "rv", "res32")}


@functools.lru_cache(maxsize=None)
def workspace(m, n):
    """ONE split-K workspace per problem size for the whole file, NaN once and never cleared: every split launch finds the slabs of
    the launch before it - another epilogue, another split count."""
    return torch.full((lib().api.lb_gemm_workspace_bytes(m, n) // 4,), float("nan"), dtype=F32, device=DEV)


def _launch(expect, A, W, out, m, n, k, ldc, flags=0, alpha=1.0, bias=None, rowvec=None, rows_per_batch=0, residual=None, ldr=0, conv=None):
    """Build the parameter block, ask lb_gemm_plan (and lb_conv_plan) about it under the switches in force, require the answer
    ``expect`` = (tile, splitk) - tile None: whatever the automatic policy picks - and the implicit-GEMM route, then launch that very
    block.  Returns the tile code."""
    l = lib()
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    p = l.gemm_params(A=A.data_ptr(), W=W.data_ptr(), C=out.data_ptr(), M=m, N=n, K=k, lda=A.stride(0) if conv is None else 0,
                      ldw=W.stride(0), ldc=ldc, conv=conv, bias=ptr(bias), residual=ptr(residual), ldr=ldr if residual is not None else 0,
                      rowvec=ptr(rowvec), ld_rowvec=0 if rowvec is None else rowvec.stride(0), rows_per_batch=rows_per_batch, alpha=alpha,
                      flags=flags, partial=workspace(m, n).data_ptr(), zero_page=ops().zero_page(A.device).data_ptr())
    tile, sk = C.c_int(), C.c_int()
    l.api.lb_gemm_plan(C.byref(p), C.byref(tile), C.byref(sk), None)
    assert l.conv_plan(p).route == l.ROUTE_GEMM, f"routed to {l.conv_plan(p).route}, not to the implicit GEMM"
    want_tile, want_sk = expect
    assert (tile.value, sk.value) == (want_tile, want_sk) or (want_tile is None and tile.value > 0 and sk.value >= 1), \
        f"the launch would run on (tile {tile.value}, splitk {sk.value}), not on the forced {expect}"
    l.api.lb_gemm_f16(C.byref(p), ops().stream_ptr())
    return tile.value


def _out_buffer(epi, pad):
    """(buffer [rows, ldc] pre-filled with SENTINEL, columns that hold results)."""
    e = E.EPILOGUES[epi]
    rows, cols = (N, M) if e.get("trans") else (M, N // 2 if e.get("geglu") else N)
    ldc = cols + (3 if e.get("trans") else pad)
    return torch.full((rows, ldc), SENTINEL, dtype=F32 if e.get("out_f32") else F16, device=DEV), cols


def run_epilogue(kind, epi, expect, pad=0, inplace=False):
    """One launch of ``epi`` -> (the whole output buffer on the CPU, result columns).  ``inplace``: the residual IS the output."""
    d, e = dev_case(kind), E.EPILOGUES[epi]
    out, cols = _out_buffer(epi, pad)
    bias, rv, res = E.operands(d, epi)
    ldr = N
    if inplace:
        out[:, :cols] = res
        res, ldr = out, out.stride(0)
    _launch(expect, d["A"], d["W"], out, M, N, K, out.stride(0), flags=E.flags_of(epi), alpha=e.get("alpha", 1.0), bias=bias, rowvec=rv,
            rows_per_batch=E.ROWS_PER_SAMPLE, residual=res, ldr=ldr)
    return out.cpu(), cols


def _check_padding(name, buf, cols):
    assert bool((buf[:, cols:] == SENTINEL).all()), f"{name}: the padding columns {cols}.. of the output rows were written"


def _collect(failed, fn, *args):
    try:
        fn(*args)
    except AssertionError as exc:                   # (every cell of a case is measured and logged before the case fails)
        failed.append(str(exc).splitlines()[0])


def _matrix_cell(log, failed, variant, tile, splitk, kind, epi, pad):
    name = f"em_{epi}_{kind}_v{variant}_t{tile}_sk{splitk}_pad{pad}"
    ref, bound = E.reference(kind, epi)
    buf, cols = run_epilogue(kind, epi, (tile, splitk), pad)
    _collect(failed, check_elementwise, log, name, buf[:, :cols], ref, bound)
    _collect(failed, _check_padding, name, buf, cols)
    if epi in ("bias_rv_res", "silu"):              # in place: bit-identical to the out-of-place launch
        buf2, _ = run_epilogue(kind, epi, (tile, splitk), pad, inplace=True)
        if not torch.equal(buf2.view(torch.int16), buf.view(torch.int16)):
            failed.append(f"{name}: the in-place launch (residual is out) differs from the out-of-place one")


def _pads(epi):
    return (0,) if E.EPILOGUES[epi].get("trans") else (0, 4)       # (the transposed store has its own stride, ldc = M + 3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant,tile,splitk", UNSPLIT)
def test_epilogue_matrix_unsplit(variant, tile, splitk, kind, results_log):
    """Every epilogue of E.EPILOGUES on every tile code of both families, unsplit, at ldc = N (16-byte stores where the epilogue has
    them) and ldc = N + 4 (8-byte stores; the padding columns stay as pre-filled).  K = 320 is forceable on every tile code: the
    ping-pong kernel (tile 9) needs K % 64 == 0."""
    failed = []
    with gemm_mode(variant, tile, splitk):
        for epi in E.EPILOGUES:
            for pad in _pads(epi):
                _matrix_cell(results_log, failed, variant, tile, splitk, kind, epi, pad)
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant,tile,splitk", SPLIT)
def test_epilogue_matrix_splitk(variant, tile, splitk, kind, results_log):
    """The same through the split-K reduce (gemm_splitk_reduce_kernel -> lb_gemm_store4, the second copy of the epilogue), every
    epilogue but GEGLU.  A forced split of a GEGLU launch must be planned as splitk = 1 and give the bits of the unsplit launch."""
    failed = []
    with gemm_mode(variant, tile, splitk):
        for epi in E.EPILOGUES:
            if E.EPILOGUES[epi].get("geglu"):
                continue
            for pad in _pads(epi):
                _matrix_cell(results_log, failed, variant, tile, splitk, kind, epi, pad)
        geglu_forced, cols = run_epilogue(kind, "geglu", (tile, 1))
    with gemm_mode(variant, tile, 1):
        geglu_unsplit, _ = run_epilogue(kind, "geglu", (tile, 1))
    assert torch.equal(geglu_forced.view(torch.int16), geglu_unsplit.view(torch.int16)), "GEGLU under a forced split differs from the unsplit launch"
    ref, bound = E.reference(kind, "geglu")
    _collect(failed, check_elementwise, results_log, f"em_geglu_{kind}_v{variant}_t{tile}_sk{splitk}_forced", geglu_forced[:, :cols], ref, bound)
    assert not failed, "\n".join(failed)


def test_workspace_reused_across_epilogues_uncleared(results_log):
    """Two different epilogues with different split counts on ONE workspace that is not cleared in between (and starts as NaN): the
    reduce must read exactly the slabs its own launch wrote."""
    ws = workspace(M, N)
    ws.fill_(float("nan"))
    failed = []
    for epi, splitk in (("f32", 3), ("silu", 2), ("trans", 3), ("relu_f32", 2)):
        with gemm_mode(1, 3, splitk):
            buf, cols = run_epilogue("normal", epi, (3, splitk))
        ref, bound = E.reference("normal", epi)
        _collect(failed, check_elementwise, results_log, f"em_ws_reuse_{epi}_sk{splitk}", buf[:, :cols], ref, bound)
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------ implicit-conv gather forms
# name -> (B, H, W, Cin, Cin as stored, Cout, kernel, stride, pad, ups, scatter)
CONV_FORMS = {
    "3x3": (2, 12, 10, 72, 72, 96, 3, 1, 1, 0, 0),
    "3x3_s2": (2, 12, 12, 64, 64, 64, 3, 2, 1, 0, 0),
    "3x3_ups": (1, 6, 10, 64, 64, 72, 3, 1, 1, 1, 0),
    "3x3_cin4": (2, 9, 11, 4, 8, 64, 3, 1, 1, 0, 0),
    "1x1": (1, 12, 12, 192, 192, 64, 1, 1, 0, 0, 0),
    "11x11_s4": (1, 35, 35, 3, 8, 64, 11, 4, 2, 0, 0),
    "5x5": (1, 7, 7, 64, 64, 192, 5, 1, 2, 0, 0),
    "subpixel": (2, 10, 12, 64, 64, 64, 2, 1, 0, 0, 1),
}
FORMS_3X3 = ["3x3", "3x3_s2", "3x3_ups", "3x3_cin4"]
CONV_KINDS = ["normal", "outliers", "sub_a"]
# (variant, tile, splitk); tile None = the automatic policy with the halo / narrow kernels switched off (lb_gemm_set_halo(0))
CONV_TILES = [(1, t, 1) for t in (1, 2, 3, 4, 5)] + [(1, None, 0)] + [(0, 1, 1), (0, 3, 1)]
CONV_SPLITS = [(1, 3, 2), (1, 2, 3)]


@functools.lru_cache(maxsize=None)
def conv_form_case(form, kind):
    """Operands of one gather form (x zero-padded to the stored Cin, the packed weights), the float64 convolution of what the kernel
    reads and |x| * |w| from the same convolution of the absolute values; bias, residual and row vector for the epilogues."""
    B, H, Wd, cin, cin_p, cout, ks, stride, pad, ups, scatter = CONV_FORMS[form]
    seed = 800 + 20 * sorted(CONV_FORMS).index(form)
    if kind == "outliers" and cin <= 7:     # (no channel 7 to carry the outliers: the last real channel does, times 64 against weights / 8)
        x, w = rnd(B, H, Wd, cin, seed=seed + 2, dtype=F32), rnd(cout, cin, ks, ks, seed=seed + 3, scale=(cin * ks * ks) ** -0.5, dtype=F32)
        x[..., cin - 1] *= 64.0
        w[:, cin - 1] /= 8.0
        x, w = x.to(F16), w.to(F16)
    else:
        x, w = _conv_operands(kind, (B, H, Wd, cin), cout, seed, kh=3 if scatter else ks)
    xp = torch.zeros(B, H, Wd, cin_p, dtype=F16)
    xp[..., :cin] = x
    if scatter:
        if kind == "sub_a":     # a value kind is defined on the operand the kernel reads: four 2x2 kernels of its own
            w4 = torch.stack([_conv_operands(kind, (B, H, Wd, cin), cout, seed + 100 + i, kh=2)[1].permute(0, 2, 3, 1).reshape(cout, 4 * cin)
                              for i in range(4)])
        else:                   # the kernels a model would load: four 2x2 kernels summed from a 3x3 one
            subs = ops().subpixel_upsample_weights(w)
            w4 = torch.stack([subs[(0, 0)], subs[(0, 1)], subs[(1, 0)], subs[(1, 1)]])
        base, ad, wk = _subpixel_ref(x, w4), _subpixel_ref(x, w4, torch.abs), w4.contiguous()
    else:
        x64 = _nchw64(x)
        if ups:
            x64 = F.interpolate(x64, scale_factor=2, mode="nearest")
        base = F.conv2d(x64, w.double(), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
        ad = F.conv2d(x64.abs(), w.double().abs(), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
        wk = ops().pack_conv_weight(w, cin_p)
    return dict(x=xp, w=wk, base=base, ad=ad, terms=ks * ks * cin, bias=rnd(cout, seed=seed + 10, dtype=F32),
                res=rnd(*base.shape, seed=seed + 11), rv=rnd(B, cout, seed=seed + 12))


def _run_conv_form(form, c, expect, bias, rv, res):
    """Launch(es) of one form on CPU operands -> the NHWC output on the CPU (NaN-prefilled: every element must be stored)."""
    B, H, Wd, cin, cin_p, cout, ks, stride, pad, ups, scatter = CONV_FORMS[form]
    xd, wd = c["x"].to(DEV), c["w"].to(DEV)
    bd, rvd, rd = [None if t is None else t.to(DEV) for t in (bias, rv, res)]
    out = torch.full(tuple(c["base"].shape), float("nan"), dtype=F16, device=DEV)
    tiles = set()
    for par in ([(0, 0), (0, 1), (1, 0), (1, 1)] if scatter else [None]):
        g = lib().ConvGeom(H, Wd, cin_p, ks, ks, stride=stride, pad=pad, ups=ups, ldx=xd.stride(2), parity=par)
        wpar = wd if par is None else wd[2 * par[0] + par[1]]
        tiles.add(_launch(expect, xd, wpar, out, g.M(B), cout, g.K, cout, bias=bd, rowvec=rvd, rows_per_batch=g.Hout * g.Wout, residual=rd,
                          ldr=cout, conv=g))
    return out.cpu(), tiles


def _conv_cell(log, failed, form, kind, variant, tile, splitk, resnet):
    """One (form, kind, tile) cell.  ``resnet``: bias + per-sample row vector + residual (bias alone for the sub-pixel form, which
    takes no residual); otherwise bias + residual (bias alone for the sub-pixel form); the subnormal kind runs bare."""
    c = conv_form_case(form, kind)
    scatter = CONV_FORMS[form][-1]
    bare = kind == "sub_a"
    bias = None if bare else c["bias"]
    res = None if bare or scatter else c["res"]
    rv = c["rv"] if resnet and not bare and not scatter else None
    rows = None
    ref = c["base"]
    if bias is not None:
        ref = ref + bias.double()
    if res is not None:
        ref = ref + res.double()
    if rv is not None:
        rows = rv.double()[:, None, None, :].expand_as(ref)
        ref = ref + rows
    k_tiles = (CONV_FORMS[form][6] ** 2 * CONV_FORMS[form][4] + 63) // 64
    got, tiles = _run_conv_form(form, c, (tile, min(splitk, k_tiles)), bias, rv, res)
    name = f"em_conv_{form}_{kind}_v{variant}_t{tile if tile is not None else 'auto' + '_'.join(map(str, sorted(tiles)))}_sk{splitk}"
    assert bool(torch.isfinite(got).all()), f"{name}: an element of the NaN-prefilled output was not stored"
    bound = contraction_bound(None, None, c["terms"], ref, bias=bias, residual=res, rowvec=rows, absdot64=c["ad"])
    _collect(failed, check_elementwise, log, name, got, ref, bound)
    if bare:
        zeros, want = int((got == 0).sum()), int((ref.half() == 0).sum())
        if zeros != want:
            failed.append(f"{name}: {zeros} zeros stored, the reference has {want}: a subnormal operand was flushed")


@pytest.mark.parametrize("kind", CONV_KINDS)
@pytest.mark.parametrize("form", list(CONV_FORMS))
def test_conv_gather_forms_elementwise(form, kind, results_log):
    """Every gather form of the implicit-GEMM conv - 3x3, stride 2, the fused nearest-2x gather, Cin padded to 8, 1x1, 11x11 stride
    4, 5x5 pad 2 and the four single-parity sub-pixel launches into one NaN-prefilled output - on the 4-wave tiles of both families,
    the 256-wide tiles and the automatic policy, against F.conv2d in float64."""
    l = lib()
    failed = []
    l.api.lb_gemm_set_halo(0)       # (a forced tile keeps the conv on the implicit GEMM by itself; the automatic policy needs this)
    try:
        for variant, tile, splitk in CONV_TILES:
            with gemm_mode(variant, tile or 0, splitk):
                _conv_cell(results_log, failed, form, kind, variant, tile, splitk, resnet=False)
    finally:
        l.api.lb_gemm_set_halo(1)
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("kind", CONV_KINDS)
@pytest.mark.parametrize("form", FORMS_3X3 + ["subpixel"])
def test_conv_gather_forms_splitk(form, kind, results_log):
    """The 3x3 forms through split-K with the ResNet epilogue - bias + time-embedding row vector (rows_per_batch = Hout * Wout, no
    multiple of 16 for three of the four) + residual - and the sub-pixel scatter with bias: lb_gemm_store4 computes the scatter row and
    the sample index itself.  The Cin = 8 form has two K-tiles, so a forced split of 3 is planned - and asserted - as 2."""
    failed = []
    for variant, tile, splitk in CONV_SPLITS:
        with gemm_mode(variant, tile, splitk):
            _conv_cell(results_log, failed, form, kind, variant, tile, splitk, resnet=True)
    assert not failed, "\n".join(failed)
