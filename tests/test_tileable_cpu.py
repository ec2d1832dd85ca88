"""Wrap-around padding without a device: the float64 identities the GPU tests lean on, the geometry value and the parameter block,
the plans of every conv of tests/_conv_plan_grid.py under wrap, and the host surface (``tileable`` parsing, movie JSON, replay)."""
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_plan_grid as G
import _tileable_ref as T
from latentblending_amd import replay, utils
from latentblending_amd.hip import lib, ops
from latentblending_amd.native.geometry import TILEABLE_WRAP, check_tileable

F64 = torch.float64
WRAPS = [1, 2, 3]


def rnd64(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


# ------------------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("ups", [0, 1])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", [(8, 8), (16, 16), (16, 32), (48, 24)], ids=lambda s: "x".join(map(str, s)))
def test_tiled_image_identity_holds_to_the_last_bit(hw, stride, ups, wrap):
    """The wrapped conv of X is the centre crop of the zero-padded conv of X repeated three times along each wrapped axis."""
    H, W = hw
    x, w, b = rnd64(2, 5, H, W, seed=H + W), rnd64(7, 5, 3, 3, seed=1), rnd64(7, seed=2)
    wrapped = T.circ_conv(x, w, b, wrap, stride, ups)
    tiled = T.circ_conv(T.tile3(x, wrap), w, b, 0, stride, ups)
    Ho, Wo = ((H << ups) - 1) // stride + 1, ((W << ups) - 1) // stride + 1
    assert tuple(wrapped.shape) == (2, 7, Ho, Wo)
    assert torch.equal(wrapped, T.centre(tiled, wrap, Ho, Wo))
    assert not torch.equal(wrapped, T.circ_conv(x, w, b, 0, stride, ups)), "the zero-padded conv must differ: the test can fail"
    # and it is torch's own circular padding mode where both axes wrap
    if wrap == 3 and not ups:
        conv = torch.nn.Conv2d(5, 7, 3, stride=stride, padding=1, padding_mode="circular", dtype=F64)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
            assert torch.allclose(conv(x), wrapped, rtol=0, atol=1e-13)


@pytest.mark.parametrize("wrap", WRAPS)
def test_subpixel_packing_on_the_wrapped_low_res_grid(wrap):
    """The project's own sub-pixel weight packing applied on the wrapped LOW-resolution grid equals "nearest-2x, then circular 3x3":
    a nearest-upsampled periodic image is periodic, so the pre-summed parity kernels stay valid.  Weights are multiples of 2^-6 so
    that the packer's fp16 rounding of the sums is exact and the comparison is one of float64 sums."""
    H, W, cin, n = 8, 12, 8, 4
    g = torch.Generator().manual_seed(9)
    w3 = torch.randint(-16, 17, (n, cin, 3, 3), generator=g).double() / 64
    x = rnd64(2, cin, H, W, seed=10)
    want = T.circ_conv(x, w3, None, wrap, 1, 1)
    got = T.subpixel_on_wrapped_grid(x, w3, wrap, lambda w: ops.subpixel_upsample_weights(w.float(), cin))
    assert float((got - want).abs().max()) <= 1e-12
    zero = T.subpixel_on_wrapped_grid(x, w3, 0, lambda w: ops.subpixel_upsample_weights(w.float(), cin))
    assert float((zero - want).abs().max()) > 1e-3


def test_one_zero_padded_conv_is_not_roll_equivariant_and_a_wrapped_one_is():
    x, w = rnd64(1, 3, 8, 8, seed=3), rnd64(3, 3, 3, 3, seed=4)
    for wrap, dim in ((1, 3), (2, 2)):
        eq = T.circ_conv(torch.roll(x, 3, dim), w, None, wrap) - torch.roll(T.circ_conv(x, w, None, wrap), 3, dim)
        assert float(eq.abs().max()) <= 1e-13
        other = 2 if dim == 3 else 3
        miss = T.circ_conv(torch.roll(x, 3, other), w, None, wrap) - torch.roll(T.circ_conv(x, w, None, wrap), 3, other)
        assert float(miss.abs().max()) > 0.1 * float(T.circ_conv(x, w, None, wrap).abs().max())


# ------------------------------------------------------------------------------------------------------------ geometry, block
def test_geometry_carries_wrap_and_refuses_where_it_is_not_defined():
    plain = lib.ConvGeom.conv3x3(16, 24, 64)
    assert plain.wrap == 0 and len(plain) == 12 and plain == lib.ConvGeom(16, 24, 64, 3, 3, pad=1)
    for wrap in WRAPS:
        g = lib.ConvGeom.conv3x3(16, 24, 64, wrap=wrap)
        assert g.wrap == wrap and g != plain and hash(g) != hash(plain) and g == lib.ConvGeom(16, 24, 64, 3, 3, pad=1, wrap=wrap)
        assert (g.Hout, g.Wout, g.K, g.ldx, g.scatter) == (plain.Hout, plain.Wout, plain.K, plain.ldx, plain.scatter)
        assert g.with_wrap(0) == plain and plain.with_wrap(wrap) == g and f"wrap={wrap}" in repr(g)
        assert g._asdict() == dict(plain._asdict(), wrap=wrap) and "wrap" not in plain._asdict() and len(plain._asdict()) == 12
        assert g._replace(Hin=32) == lib.ConvGeom.conv3x3(32, 24, 64, wrap=wrap) and g._replace(wrap=0) == plain
        assert plain._replace(wrap=wrap) == g and plain._replace(stride=2).Hout == 8
        with pytest.raises(ValueError):
            g._replace(Hout=3)
        with pytest.raises(ValueError):
            lib.ConvGeom.down3x3(16, 24, 64)._replace(Cin=8)
        with pytest.raises(TypeError):
            lib.ConvGeom._make(tuple(g))
        assert lib.ConvGeom.conv3x3(16, 24, 64, stride=2, wrap=wrap).wrap == wrap
        assert lib.ConvGeom.conv3x3(16, 24, 64, ups=1, wrap=wrap).wrap == wrap
        for parity in ("all", (0, 1)):
            assert lib.ConvGeom.subpixel(16, 24, 64, parity, wrap=wrap).wrap == wrap
        for bad in (lambda: lib.ConvGeom(16, 24, 64, 1, 1, wrap=wrap), lambda: lib.ConvGeom(16, 24, 64, 3, 3, pad=0, wrap=wrap),
                    lambda: lib.ConvGeom(64, 64, 8, 11, 11, stride=4, pad=2, wrap=wrap), lambda: lib.ConvGeom.down3x3(16, 24, 64).with_wrap(wrap),
                    lambda: lib.ConvGeom.conv3x3(16, 24, 64, wrap=wrap | 4), lambda: lib.ConvGeom(16, 24, 64, 5, 5, pad=2, wrap=wrap)):
            with pytest.raises(ValueError, match="wrap"):
                bad()
    # stride 2: an even side on every WRAPPED axis
    assert lib.ConvGeom.conv3x3(15, 16, 64, stride=2, wrap=1).wrap == 1 and lib.ConvGeom.conv3x3(16, 15, 64, stride=2, wrap=2).wrap == 2
    for H, W, wrap in ((15, 16, 2), (16, 15, 1), (15, 15, 3)):
        with pytest.raises(ValueError, match="even"):
            lib.ConvGeom.conv3x3(H, W, 64, stride=2, wrap=wrap)


def _nonzero(p):
    return {name: getattr(p, name) for name, _ in lib.LbGemmParams._fields_ if getattr(p, name)}


def test_wrap_lands_in_the_block_and_nothing_else_moves():
    assert lib.LbGemmParams._fields_[-1] == ("wrap", C.c_int) and lib.api.lb_version() >= 10100
    for make in (lambda **k: lib.ConvGeom.conv3x3(16, 32, 64, **k), lambda **k: lib.ConvGeom.conv3x3(16, 32, 64, stride=2, **k),
                 lambda **k: lib.ConvGeom.subpixel(16, 32, 64, "all", **k), lambda **k: lib.ConvGeom.subpixel(16, 32, 64, (1, 0), **k)):
        g0 = make()
        base = _nonzero(lib.gemm_params(M=g0.M(2), N=128, K=g0.K, ldw=g0.K, ldc=128, conv=g0, zero_page=64))
        assert "wrap" not in base
        for wrap in WRAPS:
            g = make(wrap=wrap)
            got = _nonzero(lib.gemm_params(M=g.M(2), N=128, K=g.K, ldw=g.K, ldc=128, conv=g, zero_page=64))
            assert got == dict(base, wrap=wrap)
    # a block built without wrap: field by field what gemm_params built before (the literal of tests/test_gemm_params_cpu.py)
    assert _nonzero(lib.conv_probe(2, 16, 32, 256, 128, 3, flags=lib.GEMM_HALO_RAGGED)) == dict(
        M=1024, N=128, K=2304, flags=1024, conv=1, Hin=16, Win=32, Cin=256, Hout=16, Wout=32, KH=3, KW=3, stride=1, pad=1, ldx=256, zero_page=64)
    assert lib.conv_probe(2, 16, 32, 256, 128, 3, wrap=3).wrap == 3 and lib.conv_probe(2, 16, 32, 256, 128, 2, wrap=1).wrap == 1


# ------------------------------------------------------------------------------------------------------------ plans
def _row_block(row, flags, wrap):
    kind, B, H, W, cin, cout, opt = row
    ks, stride, pad, ups, scatter = G.KINDS[kind]
    parity = None if not scatter else ("all" if scatter == 2 else (0, 0))
    g = lib.ConvGeom(H, W, cin, ks, ks, stride=stride, pad=pad, ups=ups, parity=parity, wrap=wrap)
    M = g.M(B)
    partial = opt.get("partial", ((M + 63) // 64) * ((cout + 63) // 64) <= 640)
    return lib.gemm_params(M=M, N=cout, K=g.K, ldw=g.K, ldc=cout, conv=g, flags=opt.get("flags", 0) | flags, A=4096, W=4096, C=4096,
                           residual=4096 if opt.get("residual") else None, ldr=cout, rowvec=4096 if opt.get("rowvec") else None,
                           ld_rowvec=cout, rows_per_batch=g.Hout * g.Wout, partial=4096 if partial else None,
                           zero_page=4096 if opt.get("zero_page", True) else None, gn=(4096, 1) if flags & G.GN_A else None)


def _plan(p):
    pl = lib.LbConvPlan()
    rc = lib._lib.lb_conv_plan(C.byref(p), C.byref(pl))
    return rc, pl


CONV_ROWS = [r for r in G.rows() if r[0] in G.KINDS]
PLAN_FIELDS = [name for name, _ in lib.LbConvPlan._fields_]
# Wrap costs no route: every conv kernel implements it, so there is NO exception to list - the plan of a wrapped conv is, field by
# field, the plan of its zero-padded twin (and a conv the unwrapped plan refuses - LB_GEMM_C64 on a non-64-channel conv, LB_GEMM_GN_A
# where nothing implements it at launch - is refused alike, with the same fields filled).
PLAN_EXCEPTIONS = {}


def test_plans_of_the_grid_do_not_move_under_wrap():
    assert len(CONV_ROWS) > 100
    checked = 0
    for row in CONV_ROWS:
        for flags in G.FLAG_SETS:
            rc0, want = _plan(_row_block(row, flags, 0))
            for wrap in WRAPS:
                if row[0] == "c3s2" and ((wrap & 2 and row[2] % 2) or (wrap & 1 and row[3] % 2)):
                    continue
                rc, got = _plan(_row_block(row, flags, wrap))
                assert rc == rc0, (row, flags, wrap, lib.api.lb_last_error_string())
                a, b = [getattr(got, f) for f in PLAN_FIELDS], [getattr(want, f) for f in PLAN_FIELDS]
                assert a == b or (row, flags, wrap) in PLAN_EXCEPTIONS, (row, flags, wrap, dict(zip(PLAN_FIELDS, zip(a, b))))
                checked += 1
    assert checked > 1500 and not PLAN_EXCEPTIONS


def test_plan_calls_refuse_a_wrap_that_is_not_defined():
    g = lib.ConvGeom(32, 32, 128, 1, 1)
    p = lib.gemm_params(M=g.M(2), N=128, K=g.K, ldw=g.K, ldc=128, conv=g, zero_page=64)
    assert _plan(p)[0] == 0
    p.wrap = 1
    rc, pl = _plan(p)
    assert rc != 0 and b"wrap" in lib.api.lb_last_error_string() and pl.tile == 0
    with pytest.raises(RuntimeError, match="wrap"):
        lib.api.lb_gemm_plan(C.byref(p), None, None, None)
    q = lib.conv_probe(2, 32, 32, 128, 128, 3)
    for bad in (4, 7, -1):
        q.wrap = bad
        assert _plan(q)[0] != 0
        kind = C.c_int(-1)
        lib.api.lb_conv_halo_plan(C.byref(q), C.byref(kind), None, None, None)
        assert kind.value == 0
    plain = lib.gemm_params(M=64, N=64, K=64, lda=64, ldw=64, ldc=64, zero_page=64)
    plain.wrap = 1
    assert _plan(plain)[0] != 0, "a plain GEMM has nothing to wrap"


# ------------------------------------------------------------------------------------------------------------ emitter
def test_emitter_applies_wrap_to_same_convs_only():
    import latentblending_amd.native.runtime as rt
    em = rt.Emitter(rt.Arena("cpu"))
    geoms = [lib.ConvGeom.conv3x3(16, 16, 64), lib.ConvGeom.conv3x3(16, 16, 64, stride=2), lib.ConvGeom.conv3x3(16, 16, 64, ups=1),
             lib.ConvGeom.subpixel(16, 16, 64, "all"), lib.ConvGeom.subpixel(16, 16, 64, (1, 1))]
    others = [lib.ConvGeom(16, 16, 64, 1, 1), lib.ConvGeom.down3x3(16, 16, 64), lib.ConvGeom(64, 64, 8, 11, 11, stride=4, pad=2), None]
    assert em.wrap == 0 and all(em._geom(g) is g for g in geoms + others)
    for wrap in WRAPS:
        em.wrap = wrap
        assert [em._geom(g).wrap for g in geoms] == [wrap] * len(geoms)
        assert all(em._geom(g) is g for g in others)
    em.wrap = 1
    assert em._geom(lib.ConvGeom.conv3x3(15, 16, 64, stride=2)).wrap == 1
    with pytest.raises(ValueError, match="even"):          # a same conv that cannot wrap is an error, never a zero-padded conv
        em._geom(lib.ConvGeom.conv3x3(16, 15, 64, stride=2))
    with pytest.raises(ValueError, match="wrap"):
        rt.RecordedProgram(types.SimpleNamespace(device="cpu"), 1, 16, wrap=4)


# ------------------------------------------------------------------------------------------------------------ host surface
def test_check_tileable_table():
    from latentblending_amd.native.pipe import NativeSDXLPipe
    table = {None: "", False: "", "": "", "x": "x", "y": "y", "xy": "xy", True: "xy", " XY ": "xy", "X": "x"}
    for value, want in table.items():
        assert NativeSDXLPipe._check_tileable(value) == want == check_tileable(value)
    assert TILEABLE_WRAP == {"": 0, "x": 1, "y": 2, "xy": 3}
    for bad in ("yx", "both", 1, 3, "z", ("x",), 0.0):
        with pytest.raises(ValueError, match="'x', 'y', 'xy'"):
            NativeSDXLPipe._check_tileable(bad)
    with pytest.raises(ValueError, match="tileable"):
        NativeSDXLPipe(tileable="diagonal")             # refused before anything needs a device


def _engine(pipe):
    return types.SimpleNamespace(dh=types.SimpleNamespace(pipe=pipe, width_img=64, height_img=48, num_inference_steps=2))


def test_movie_json_header_carries_tileable_only_when_on(tmp_path):
    items = [{"iteration": 0, "seed": 1, "prompt": "a", "negative_prompt": ""}, {"iteration": 1, "seed": 2, "prompt": "b", "negative_prompt": ""}]
    fp = str(tmp_path / "m.json")
    replay.save_movie_json(fp, _engine(object()), items)
    default = open(fp).read()
    assert "tileable" not in default and set(json.loads(default)[0]) == {"settings", "width", "height", "num_inference_steps"}
    for off in (None, False, ""):
        replay.save_movie_json(fp, _engine(types.SimpleNamespace(tileable="")), items, tileable=off)
        assert open(fp).read() == default
    for given, want in (("x", "x"), ("y", "y"), ("XY", "xy"), (True, "xy")):
        replay.save_movie_json(fp, _engine(object()), items, tileable=given)
        header, got = replay.load_movie_json(fp)
        assert header["tileable"] == want and got == items
    replay.save_movie_json(fp, _engine(types.SimpleNamespace(tileable="y")), items)          # (None: the pipe as it stands)
    assert replay.load_movie_json(fp)[0]["tileable"] == "y"
    with pytest.raises(ValueError, match="tileable"):
        replay.save_movie_json(fp, _engine(object()), items, tileable="sideways")


def test_tileable_needs_a_pipe_with_the_setting_and_is_restored():
    oracle_like = _engine(object())
    with pytest.raises(ValueError, match="tileable"):
        replay.run_multi_transition(oracle_like, ["a", "b"], [1, 2], tileable="x")

    class Pipe:
        def __init__(self):
            self._t, self.seen = "y", []

        @property
        def tileable(self):
            return self._t

        @tileable.setter
        def tileable(self, v):
            self._t = check_tileable(v)
            self.seen.append(self._t)
    pipe = Pipe()
    with replay._tileable_as(_engine(pipe), "x"):
        assert pipe.tileable == "x"
    assert pipe.tileable == "y" and pipe.seen == ["x", "y"]
    with pytest.raises(RuntimeError):
        with replay._tileable_as(_engine(pipe), True):
            assert pipe.tileable == "xy"
            raise RuntimeError("a chain that fails")
    assert pipe.tileable == "y"
    with replay._tileable_as(_engine(pipe), None):
        pass
    assert pipe.seen == ["x", "y", "xy", "y"]


def test_run_movie_json_hands_the_header_setting_on(tmp_path, monkeypatch):
    items = [{"iteration": 0, "seed": 1, "prompt": "a", "negative_prompt": ""}, {"iteration": 1, "seed": 2, "prompt": "b", "negative_prompt": ""}]
    fp = str(tmp_path / "m.json")
    be = _engine(object())
    be.set_dimensions = be.set_num_inference_steps = lambda *a: None
    seen = []
    monkeypatch.setattr(replay, "run_multi_transition", lambda *a, **k: seen.append(k.get("tileable")) or [])
    replay.save_movie_json(fp, be, items, tileable="x")
    replay.run_movie_json(be, fp)
    replay.run_movie_json(be, fp, tileable="xy")
    replay.save_movie_json(fp, be, items)
    replay.run_movie_json(be, fp)
    assert seen == ["x", "xy", None]


def test_tile_preview():
    a = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    m = utils.tile_preview(a)
    assert m.shape == (4, 6, 3) and all(np.array_equal(m[y:y + 2, x:x + 3], a) for y in (0, 2) for x in (0, 3))
    assert utils.tile_preview(a, 3, 1).shape == (2, 9, 3) and utils.tile_preview(a[..., 0], 1, 2).shape == (4, 3)
    t = utils.tile_preview(torch.from_numpy(a), 2, 3)
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == (6, 6, 3) and torch.equal(t[4:, 3:], torch.from_numpy(a))
    from PIL import Image
    im = utils.tile_preview(Image.fromarray(a), nx=2, ny=2)
    assert isinstance(im, Image.Image) and im.size == (6, 4) and np.array_equal(np.asarray(im), m)
    with pytest.raises(ValueError):
        utils.tile_preview(a, 0, 2)
