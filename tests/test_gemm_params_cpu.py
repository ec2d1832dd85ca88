"""The one builder of the GEMM / conv parameter block (lib.gemm_params), the conv geometry value (lib.ConvGeom) and their three
product callers - ops.gemm, Emitter._gemm_params, lib.conv_probe - held to literal blocks.

The tables below were recorded ONCE from the constructors of the commit before the builder existed (ops.gemm with the launch
entry patched as here, Emitter._gemm_params with the hand-written 11-key conv dicts, lib.conv_probe), never from the builder: a
table lists every field that is not zero / null, a pointer as the name of the tensor it must point at ("?" = some other address:
a workspace the wrapper allocated itself).  No device, no device tensor, no launch."""
import ctypes as C
import os
import re

import pytest
import torch

import latentblending_amd.native.runtime as rt
from latentblending_amd.hip import lib, ops

F16, F32 = torch.float16, torch.float32
GEGLU, TRANS_OUT, RELU, OUT_F32 = lib.GEMM_GEGLU, lib.GEMM_TRANS_OUT, lib.GEMM_RELU, lib.GEMM_OUT_F32


def t(*shape, dtype=F16):
    return torch.zeros(*shape, dtype=dtype)


def f32(x):
    return C.c_float(x).value


def block(p, tensors):
    """The fields of ``p`` that are not zero / null; a pointer as the name of the tensor in ``tensors`` it points at."""
    names = {v.data_ptr(): k for k, v in tensors.items()}
    out = {}
    for name, ctype in lib.LbGemmParams._fields_:
        v = getattr(p, name)
        if ctype is C.c_void_p:
            v = names.get(v, "?") if v else None
        if v:
            out[name] = v
    return out


# ------------------------------------------------------------------------------ the geometry value
GEOMETRIES = {
    # name: (geometry, B, (Hout, Wout, K, M(B), scatter))
    "3x3 s1 p1": (lambda: lib.ConvGeom.conv3x3(64, 48, 320), 2, (64, 48, 2880, 6144, 0)),
    "3x3 s2 p1 odd": (lambda: lib.ConvGeom.conv3x3(15, 15, 64, stride=2), 3, (8, 8, 576, 192, 0)),
    "3x3 ups": (lambda: lib.ConvGeom.conv3x3(16, 24, 64, ups=1), 1, (32, 48, 576, 1536, 0)),
    "1x1 p0": (lambda: lib.ConvGeom(32, 32, 128, 1, 1), 2, (32, 32, 128, 2048, 0)),
    "11x11 s4 p2": (lambda: lib.ConvGeom(64, 64, 8, 11, 11, stride=4, pad=2), 2, (15, 15, 968, 450, 0)),
    "2x2 parity (1, 0)": (lambda: lib.ConvGeom.subpixel(16, 32, 256, (1, 0)), 2, (16, 32, 1024, 1024, 1)),
    "2x2 parity all": (lambda: lib.ConvGeom.subpixel(16, 32, 256, "all"), 2, (16, 32, 1024, 1024, 2)),
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry_derives_the_literal_sizes(name):
    make, B, want = GEOMETRIES[name]
    g = make()
    assert (g.Hout, g.Wout, g.K, g.M(B), g.scatter) == want
    assert g.ldx == g.Cin                                   # (ldx=None: dense)


def test_geometry_is_a_frozen_value():
    g = lib.ConvGeom.conv3x3(8, 8, 16, ldx=24)
    assert (g.KH, g.KW, g.stride, g.pad, g.ups, g.ldx, g.parity) == (3, 3, 1, 1, 0, 24, None)
    assert g == lib.ConvGeom(8, 8, 16, 3, 3, pad=1, ldx=24) and hash(g) == hash(lib.ConvGeom(8, 8, 16, 3, 3, pad=1, ldx=24))
    with pytest.raises(Exception):
        g.pad = 0
    s = lib.ConvGeom.subpixel(8, 8, 16, (0, 1))
    assert (s.KH, s.KW, s.stride, s.pad, s.ups, s.ldx, s.parity) == (2, 2, 1, 0, 0, 16, (0, 1))


# ------------------------------------------------------------------------------ ops.gemm
def _ws(M, N):
    return t(lib.api.lb_gemm_workspace_bytes(M, N) // 4, dtype=F32)


def _ops_cases():
    """name -> (tensors by name, keyword arguments of ops.gemm)."""
    c = {}
    x = dict(A=t(40, 72)[:, :64], W=t(48, 64))
    c["strided_A"] = (x, dict(x))
    x = dict(A=t(40, 64), W=t(48, 64), bias=t(48, dtype=F32), residual=t(40, 56)[:, :48], rowvec=t(2, 1280)[:, 100:148], C=t(40, 48),
             partial=_ws(40, 48))
    c["bias_residual_rowvec"] = (x, dict(A=x["A"], W=x["W"], bias=x["bias"], residual=x["residual"], rowvec=x["rowvec"], rows_per_batch=20,
                                         alpha=0.25, out=x["C"], workspace=x["partial"]))
    x = dict(A=t(40, 64), W=t(96, 64))
    c["geglu"] = (x, dict(x, flags=GEGLU))
    x = dict(A=t(40, 64), W=t(48, 64), C=t(48, 50)[:, :40])
    c["trans_out"] = (x, dict(A=x["A"], W=x["W"], out=x["C"], flags=TRANS_OUT))
    x = dict(A=t(40, 64), W=t(48, 64), bias=t(48, dtype=F32), ln_colsum=t(48, dtype=F32))
    c["ln"] = (x, dict(A=x["A"], W=x["W"], bias=x["bias"], ln=(x["ln_colsum"], 1e-5)))
    x = dict(A=t(2, 8, 8, 16), W=t(32, 144), bias=t(32, dtype=F32), ch_stats=t(32, 2, 2, dtype=F32))
    c["conv3_ch_stats"] = (x, dict(A=x["A"], W=x["W"], bias=x["bias"], ch_stats=x["ch_stats"], flags=RELU, conv=dict(KH=3, KW=3, pad=1)))
    x = dict(A=t(1, 15, 15, 24)[..., :16], W=t(32, 144))
    c["conv3_s2_padded_ldx"] = (x, dict(x, conv=dict(KH=3, KW=3, stride=2, pad=1)))
    x = dict(A=t(1, 8, 8, 64), W=t(64, 576))
    c["conv3_ups_halo_entry"] = (x, dict(x, flags=OUT_F32, conv=dict(KH=3, KW=3, pad=1, ups=1, halo=True)))
    x = dict(A=t(1, 8, 8, 16), W=t(32, 64), C=t(1, 16, 16, 32))
    c["parity_10"] = (x, dict(A=x["A"], W=x["W"], out=x["C"], conv=dict(KH=2, KW=2, parity=(1, 0))))
    x = dict(A=t(1, 8, 8, 16), W=t(4, 32, 64)[0], C=t(1, 16, 16, 32))
    c["parity_all"] = (x, dict(A=x["A"], W=x["W"], out=x["C"], conv=dict(KH=2, KW=2, parity="all")))
    x = dict(A=t(40, 64), W=t(48, 64))
    c["no_workspace"] = (x, dict(x, splitk_ws=False))
    return c


OPS_WANT = {
    "strided_A": ("lb_gemm_f16", dict(
        A="A", W="W", C="C", partial="?", M=40, N=48, K=64, lda=72, ldw=64, ldc=48, alpha=1.0, zero_page="zero_page")),
    "bias_residual_rowvec": ("lb_gemm_f16", dict(
        A="A", W="W", C="C", bias="bias", residual="residual", rowvec="rowvec", partial="partial", M=40, N=48, K=64, lda=64, ldw=64,
        ldc=48, ldr=56, ld_rowvec=1280, rows_per_batch=20, alpha=0.25, zero_page="zero_page")),
    "geglu": ("lb_gemm_f16", dict(
        A="A", W="W", C="C", M=40, N=96, K=64, lda=64, ldw=64, ldc=48, alpha=1.0, flags=4, zero_page="zero_page")),
    "trans_out": ("lb_gemm_f16", dict(
        A="A", W="W", C="C", partial="?", M=40, N=48, K=64, lda=64, ldw=64, ldc=50, alpha=1.0, flags=8, zero_page="zero_page")),
    "ln": ("lb_gemm_f16", dict(
        A="A", W="W", C="C", bias="bias", M=40, N=48, K=64, lda=64, ldw=64, ldc=48, alpha=1.0, flags=64, zero_page="zero_page",
        ln_colsum="ln_colsum", ln_eps=f32(1e-5))),
    "conv3_ch_stats": ("lb_gemm_f16", dict(
        A="A", W="W", C="C", bias="bias", partial="?", M=128, N=32, K=144, ldw=144, ldc=32, alpha=1.0, flags=32 | 512, conv=1, Hin=8,
        Win=8, Cin=16, Hout=8, Wout=8, KH=3, KW=3, stride=1, pad=1, ldx=16, zero_page="zero_page", ch_stats="ch_stats",
        ch_stats_rows=2)),
    "conv3_s2_padded_ldx": ("lb_gemm_f16", dict(
        A="A", W="W", C="C", partial="?", M=64, N=32, K=144, ldw=144, ldc=32, alpha=1.0, conv=1, Hin=15, Win=15, Cin=16, Hout=8,
        Wout=8, KH=3, KW=3, stride=2, pad=1, ldx=24, zero_page="zero_page")),
    "conv3_ups_halo_entry": ("lb_conv3x3_halo_f16", dict(
        A="A", W="W", C="C", partial="?", M=256, N=64, K=576, ldw=576, ldc=64, alpha=1.0, flags=1, conv=1, Hin=8, Win=8, Cin=64,
        Hout=16, Wout=16, KH=3, KW=3, stride=1, pad=1, ups=1, ldx=64, zero_page="zero_page")),
    "parity_10": ("lb_gemm_f16", dict(
        A="A", W="W", C="C", partial="?", M=64, N=32, K=64, ldw=64, ldc=32, alpha=1.0, conv=1, Hin=8, Win=8, Cin=16, Hout=8, Wout=8,
        KH=2, KW=2, stride=1, ldx=16, zero_page="zero_page", scatter=1, sc_py=1)),
    "parity_all": ("lb_gemm_f16", dict(
        A="A", W="W", C="C", partial="?", M=64, N=32, K=64, ldw=64, ldc=32, alpha=1.0, conv=1, Hin=8, Win=8, Cin=16, Hout=8, Wout=8,
        KH=2, KW=2, stride=1, ldx=16, zero_page="zero_page", scatter=2)),
    "no_workspace": ("lb_gemm_f16", dict(
        A="A", W="W", C="C", M=40, N=48, K=64, lda=64, ldw=64, ldc=48, alpha=1.0, zero_page="zero_page")),
}


def run_ops_case(monkeypatch, name):
    """(entry point launched, block it was handed) for one ops.gemm case, launching nothing."""
    got = []
    for entry in ("lb_gemm_f16", "lb_conv3x3_halo_f16"):
        monkeypatch.setattr(lib.api, entry, lambda pp, stream, entry=entry: got.append((entry, pp._obj)))
    monkeypatch.setattr(ops, "stream_ptr", lambda: None)
    tensors, kwargs = _ops_cases()[name]
    out = ops.gemm(**kwargs)
    tensors = dict(tensors, zero_page=ops.zero_page(out.device))
    tensors.setdefault("C", out)
    (entry, p), = got
    return entry, block(p, tensors)


@pytest.mark.parametrize("name", list(OPS_WANT))
def test_ops_gemm_hands_the_launcher_the_literal_block(name, monkeypatch):
    assert run_ops_case(monkeypatch, name) == OPS_WANT[name]


def test_every_ops_case_has_a_table():
    assert set(_ops_cases()) == set(OPS_WANT)


# ------------------------------------------------------------------------------ Emitter._gemm_params
def _emitter_cases(geom):
    """name -> (tensors by name, keyword arguments of Emitter._gemm_params); ``geom``: the constructor of a conv geometry."""
    c = {}
    x = dict(A=t(40, 64), W=t(48, 64), C=t(40, 48), bias=t(48, dtype=F32))
    c["dense_defaults"] = (x, dict(M=40, bias=x["bias"]))
    x = dict(A=t(40, 72), W=t(48, 64), C=t(40, 56), residual=t(40, 60), rowvec=t(2, 1280))
    c["explicit_lds"] = (x, dict(M=40, residual=x["residual"], rowvec=x["rowvec"], rows_per_batch=20, alpha=0.25, lda=72, ldc=56, ldr=60,
                                 ld_rowvec=1280))
    x = dict(A=t(40, 64), W=t(96, 64), C=t(40, 48), rowvec=t(2, 96))
    c["geglu_rowvec_default_ld"] = (x, dict(M=40, rowvec=x["rowvec"], rows_per_batch=20, flags=GEGLU))
    x = dict(A=t(40, 64), W=t(48, 64), C=t(48, 40))
    c["trans_out"] = (x, dict(M=40, flags=TRANS_OUT))
    x = dict(A=t(2, 8, 8, 24), W=t(32, 144), C=t(2, 8, 8, 32), bias=t(32, dtype=F32))
    c["conv_padded_ldx"] = (x, dict(M=128, bias=x["bias"], rows_per_batch=64, flags=RELU, conv=geom(8, 8, 16, 3, 3, pad=1, ldx=24)))
    x = dict(A=t(1, 15, 15, 64), W=t(64, 576), C=t(1, 8, 8, 64))
    c["conv_s2"] = (x, dict(M=64, ldc=64, conv=geom(15, 15, 64, 3, 3, stride=2, pad=1)))
    x = dict(A=t(40, 64), W=t(48, 64), C=t(40, 48), ln_colsum=t(48, dtype=F32))
    c["ln"] = (x, dict(M=40, ln=(x["ln_colsum"], 1e-5)))
    x = dict(A=t(2, 8, 8, 16), W=t(32, 144), C=t(2, 8, 8, 32), ch_stats=t(32, 2, 2, dtype=F32))
    c["conv_ch_stats"] = (x, dict(M=128, ch_stats=x["ch_stats"], alpha=0.0625, conv=geom(8, 8, 16, 3, 3, pad=1)))
    x = dict(A=t(1, 8, 8, 16), W=t(32, 64), C=t(1, 16, 16, 32))
    c["parity_01"] = (x, dict(M=64, ldc=32, conv=geom(8, 8, 16, 2, 2, parity=(0, 1))))
    x = dict(A=t(1, 8, 8, 16), W=t(4, 32, 64)[0], C=t(1, 16, 16, 32))
    c["parity_all"] = (x, dict(M=64, ldc=32, conv=geom(8, 8, 16, 2, 2, parity="all")))
    return c


EMITTER_WANT = {
    "dense_defaults": dict(
        A="A", W="W", C="C", bias="bias", M=40, N=48, K=64, lda=64, ldw=64, ldc=48, ldr=48, alpha=1.0, zero_page="zero_page"),
    "explicit_lds": dict(
        A="A", W="W", C="C", residual="residual", rowvec="rowvec", M=40, N=48, K=64, lda=72, ldw=64, ldc=56, ldr=60, ld_rowvec=1280,
        rows_per_batch=20, alpha=0.25, zero_page="zero_page"),
    "geglu_rowvec_default_ld": dict(
        A="A", W="W", C="C", rowvec="rowvec", M=40, N=96, K=64, lda=64, ldw=64, ldc=48, ldr=48, ld_rowvec=96, rows_per_batch=20,
        alpha=1.0, flags=4, zero_page="zero_page"),
    "trans_out": dict(
        A="A", W="W", C="C", M=40, N=48, K=64, lda=64, ldw=64, ldc=40, ldr=48, alpha=1.0, flags=8, zero_page="zero_page"),
    "conv_padded_ldx": dict(          # (rows_per_batch given without a rowvec: stays zero)
        A="A", W="W", C="C", bias="bias", M=128, N=32, K=144, ldw=144, ldc=32, ldr=32, alpha=1.0, flags=32, conv=1, Hin=8, Win=8,
        Cin=16, Hout=8, Wout=8, KH=3, KW=3, stride=1, pad=1, ldx=24, zero_page="zero_page"),
    "conv_s2": dict(
        A="A", W="W", C="C", M=64, N=64, K=576, ldw=576, ldc=64, ldr=64, alpha=1.0, conv=1, Hin=15, Win=15, Cin=64, Hout=8, Wout=8,
        KH=3, KW=3, stride=2, pad=1, ldx=64, zero_page="zero_page"),
    "ln": dict(
        A="A", W="W", C="C", M=40, N=48, K=64, lda=64, ldw=64, ldc=48, ldr=48, alpha=1.0, flags=64, zero_page="zero_page",
        ln_colsum="ln_colsum", ln_eps=f32(1e-5)),
    "conv_ch_stats": dict(
        A="A", W="W", C="C", M=128, N=32, K=144, ldw=144, ldc=32, ldr=32, alpha=0.0625, flags=512, conv=1, Hin=8, Win=8, Cin=16,
        Hout=8, Wout=8, KH=3, KW=3, stride=1, pad=1, ldx=16, zero_page="zero_page", ch_stats="ch_stats", ch_stats_rows=2),
    "parity_01": dict(
        A="A", W="W", C="C", M=64, N=32, K=64, ldw=64, ldc=32, ldr=32, alpha=1.0, conv=1, Hin=8, Win=8, Cin=16, Hout=8, Wout=8,
        KH=2, KW=2, stride=1, ldx=16, zero_page="zero_page", scatter=1, sc_px=1),
    "parity_all": dict(
        A="A", W="W", C="C", M=64, N=32, K=64, ldw=64, ldc=32, ldr=32, alpha=1.0, conv=1, Hin=8, Win=8, Cin=16, Hout=8, Wout=8,
        KH=2, KW=2, stride=1, ldx=16, zero_page="zero_page", scatter=2),
}


def run_emitter_case(name, geom):
    em = rt.Emitter(rt.Arena("cpu"))
    tensors, kwargs = _emitter_cases(geom)[name]
    p = em._gemm_params(tensors["A"], tensors["W"], tensors["C"], **kwargs)
    return block(p, dict(tensors, zero_page=em.zero_page))


@pytest.mark.parametrize("name", list(EMITTER_WANT))
def test_emitter_builds_the_literal_block(name):
    assert run_emitter_case(name, lib.ConvGeom) == EMITTER_WANT[name]


def test_every_emitter_case_has_a_table():
    assert set(_emitter_cases(lib.ConvGeom)) == set(EMITTER_WANT)


# ------------------------------------------------------------------------------ lib.conv_probe
PROBE_WANT = {      # (no ldw / ldc / alpha: the plan calls read none of them)
    3: dict(M=1024, N=128, K=2304, flags=1024, conv=1, Hin=16, Win=32, Cin=256, Hout=16, Wout=32, KH=3, KW=3, stride=1, pad=1, ldx=256,
            zero_page=64),
    2: dict(M=1024, N=128, K=1024, conv=1, Hin=16, Win=32, Cin=256, Hout=16, Wout=32, KH=2, KW=2, stride=1, ldx=256, zero_page=64,
            scatter=2),
}


def _nonzero(p):
    return {name: getattr(p, name) for name, _ in lib.LbGemmParams._fields_ if getattr(p, name)}


@pytest.mark.parametrize("ks", [3, 2])
def test_conv_probe_returns_the_literal_block(ks):
    assert _nonzero(lib.conv_probe(2, 16, 32, 256, 128, ks, flags=lib.GEMM_HALO_RAGGED if ks == 3 else 0)) == PROBE_WANT[ks]
    bare = {k: v for k, v in PROBE_WANT[ks].items() if k not in ("zero_page", "flags")}
    assert _nonzero(lib.conv_probe(2, 16, 32, 256, 128, ks, zero_page=0)) == bare


# ------------------------------------------------------------------------------ one constructor
PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "latentblending_amd")
BUILDER = os.path.join("hip", "lib.py")
PLANNING = {os.path.join("native", "runtime.py"): {"flags", "partial"}}        # the emitter's opt-in bits and its workspaces


def test_only_the_builder_assigns_fields_of_the_block():
    """Plain-text scan of the package: outside the builder's module no statement assigns ``p.<field>`` (``=``, ``|=``, ``&=``, tuple
    targets) over the field names of LbGemmParams, but for the planning fields the emitter sets on a built block.  A function that
    fills an LbAttnParams (which shares the field name K) is told apart by the constructor it calls."""
    names = {name for name, _ in lib.LbGemmParams._fields_}
    assign = re.compile(r"\s*((?:p\.\w+\s*,\s*)*p\.\w+)\s*[|&]?=(?!=)")
    scanned = 0
    for root, _, files in os.walk(PACKAGE):
        for fn in files:
            rel = os.path.relpath(os.path.join(root, fn), PACKAGE)
            if not fn.endswith(".py") or rel == BUILDER:
                continue
            scanned += 1
            with open(os.path.join(root, fn)) as fh:
                src = fh.read()
            assert "LbGemmParams()" not in src, rel
            for fun in re.split(r"\n(?=\s*def )", src):
                if "LbAttnParams()" in fun:
                    continue
                for line in fun.splitlines():
                    lhs = assign.match(line.split("#")[0])
                    if lhs:
                        fields = set(re.findall(r"p\.(\w+)", lhs.group(1))) & names
                        assert fields <= PLANNING.get(rel, set()), f"{rel}: {line.strip()}"
    assert scanned > 10
    with open(os.path.join(PACKAGE, BUILDER)) as fh:
        assert "LbGemmParams()" not in fh.read() and lib.gemm_params.__kwdefaults__["make"] is lib.LbGemmParams
