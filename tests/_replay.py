"""The replay protocol of test_program_replay_gpu.py and the registry of launcher cases it is applied to.

A *case* owns every device buffer a launcher call touches (inputs with their snapshots, outputs inside ``_guard.guarded`` buffers,
scratch workspaces), a thunk that makes the call(s), and the op names the program must report.  ``run_protocol`` holds the case to
one rule: whatever way the recorded closure is replayed - eagerly, in every ``run_range`` split, as a hipGraph on two streams, under
``time_ops`` - the bytes of every output buffer, guard bands included, equal the bytes of a direct launch.  No tolerance anywhere.

The protocol talks to the device only through a *driver* (``GpuDriver`` below), so that a CPU test can run it on fake cases and prove
that it fails when a replay differs by one bit or a recording writes (test_program_cpu.py).

The registry is importable without a GPU: an entry is (case id, launcher names, builder); builders run on the GPU tier only.
"""
import contextlib
import ctypes as C
import functools
import math

import torch

DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
U8, I16, I32 = torch.uint8, torch.int16, torch.int32
NAN = float("nan")

# every switch include/lb_hip.h documents as "same results": name -> (default, another legal value)
KNOBS = {
    "lb_gemm_set_wide_store": (1, 0),
    "lb_gemm_set_lean_epilogue": (1, 0),
    "lb_conv_halo_set_persistent": (1, 0),
    "lb_gemm_set_t192_waves8": (1, 0),
    "lb_gemm_set_kgroups": (1, 0),
    "lb_gemm_set_pp_auto": (1, 0),
    "lb_gemm_set_depth": (0, 2),
    "lb_layernorm_set_form": (1, 0),
    "lb_groupnorm_set_fused": (1, 0),
    "lb_attn_set_tuning": (0, 128),          # bit 7: 8-byte output stores
}


def is_program_api(name):
    return name.startswith("lb_program_")


def table_launchers():
    """What a program can record: the entries of lib.SIGNATURES whose role is ``launcher`` (one replay case each, at least)."""
    return {name for name, sig in _lib().SIGNATURES.items() if sig[2] == "launcher"}


# ====================================================================== cases ==================
class Out:
    """One output (or in-out) buffer: ``bits`` is the whole allocation (guards, pad columns), ``init`` its state before a run -
    the sentinel everywhere for a pure output, the operand inside the guards for an in-out buffer."""

    def __init__(self, name, bits, chk=None, full=True, inout=False):
        self.name, self.bits, self.chk, self.full, self.inout = name, bits, chk, full, inout
        self.init = None

    def reset(self):
        self.bits.copy_(self.init)


class Case:
    def __init__(self, name, ops):
        self.name, self.ops = name, list(ops)
        self.outs, self.inputs, self.keep, self.host = [], [], [], []
        self.knobs = {}              # "same results" switches this case records under (others: defaults)
        self.thunk = None
        self.mutate = None           # optional: writes new values into input buffers (params_dev) between replays
        self.decoy = None            # valid device memory the host pointer arrays are pointed at after recording
        self.operands = {}           # optional: the builder's tensors by name, for a test that checks the results against a reference

    # -- building ---------------------------------------------------------------------------
    def guarded(self, name, rows, cols, ld, dtype, back_rows=256, full=True, fill=None, sentinel=None):
        """A guarded output; ``fill`` [rows, cols] makes it an in-out buffer that starts as that operand."""
        from _guard import guarded
        view, chk = guarded(rows, cols, ld, dtype, DEV, back_rows=back_rows, sentinel=sentinel)
        if fill is not None:
            view.copy_(fill.to(DEV))
        self.outs.append(Out(name, chk.bits, chk, full=full and dtype != U8, inout=fill is not None))
        return view

    def plain_out(self, name, shape, dtype):
        """An output of a dtype ``_guard`` has no sentinel for (int32 frame sizes): poisoned with 0xA5 bytes, compared whole."""
        t = torch.full((math.prod(shape) * torch.empty((), dtype=dtype).element_size(),), 0xA5, dtype=U8, device=DEV)
        self.outs.append(Out(name, t, None, full=False))
        return t.view(dtype).view(*shape)

    def inp(self, t):
        """Register a device input (restored from its snapshot before every run); returns it."""
        self.inputs.append([t, None])
        return t

    def dev(self, t):
        return self.inp(t.to(DEV))

    def scratch(self, n, dtype):
        t = torch.empty(n, dtype=dtype, device=DEV)
        self.keep.append(t)
        return t

    def freeze(self):
        for o in self.outs:
            o.init = o.bits.clone()
        for pair in self.inputs:
            pair[1] = pair[0].clone()
        return self

    # -- running ----------------------------------------------------------------------------
    def restore(self):
        for t, snap in self.inputs:
            t.copy_(snap)
        for o in self.outs:
            o.reset()

    def snapshot(self):
        return [o.bits.clone() for o in self.outs]

    def differs(self, want):
        """Names of the outputs whose bytes differ from ``want`` (a snapshot)."""
        return [o.name for o, w in zip(self.outs, want) if not torch.equal(o.bits, w)]

    def destroy_host(self):
        """Zero the parameter structs, point the host pointer arrays at the decoy buffer, overwrite the fraction arrays, and drop
        every reference.  (Pointer arrays get VALID decoy pointers rather than random bits: a closure that wrongly read them at replay
        must produce a wrong result the comparison sees, not a wild store on a shared machine.)"""
        n = len(self.host)
        for obj in self.host:
            if isinstance(obj, C.Structure):
                C.memset(C.addressof(obj), 0, C.sizeof(obj))
            elif isinstance(obj, C.Array) and obj._type_ is C.c_void_p:
                for i in range(len(obj)):
                    obj[i] = self.decoy
            elif isinstance(obj, C.Array):
                for i in range(len(obj)):
                    obj[i] = 0.123456789
            else:                                   # a scalar passed by value (the ``double fract`` of lb_lerp_*)
                obj.value = 0.123456789
        self.host.clear()
        return n


@contextlib.contextmanager
def track_host(case):
    """While a thunk runs, every LbGemmParams / LbAttnParams / host pointer array the ops.py wrappers build is registered with the
    case, so that the protocol can destroy them after the recording."""
    from latentblending_amd.hip import lib, ops

    def tracked(cls):
        def make(*a, **k):
            obj = cls(*a, **k)
            case.host.append(obj)
            return obj
        return make

    saved = ops.LbGemmParams, ops.LbAttnParams, ops._ptr_array

    def ptr_array(tensors):
        cast, arr = saved[2](tensors)
        case.host.append(arr)
        return cast, arr
    ops.LbGemmParams, ops.LbAttnParams, ops._ptr_array = tracked(lib.LbGemmParams), tracked(lib.LbAttnParams), ptr_array
    try:
        yield
    finally:
        ops.LbGemmParams, ops.LbAttnParams, ops._ptr_array = saved


# ====================================================================== the protocol ===========
class ProtocolFailure(AssertionError):
    pass


def _require(cond, case, step, what):
    if not cond:
        raise ProtocolFailure(f"[{case.name}] {step}: {what}")


def run_protocol(case, drv):
    """Steps 1-8 of the replay protocol (see the module docstring of test_program_replay_gpu.py); returns the record line."""
    rec = {"case": case.name, "ops": len(case.ops)}
    record_knobs = {k: case.knobs.get(k, d) for k, (d, _) in KNOBS.items()}
    other_knobs = {k: (a if record_knobs[k] != a else d) for k, (d, a) in KNOBS.items()}
    try:
        drv.set_knobs(record_knobs)
        # 1. two direct launches on restored inputs and poisoned outputs
        case.restore()
        drv.direct(case)
        D = case.snapshot()
        case.restore()
        drv.direct(case)
        _require(not case.differs(D), case, "direct x2", f"two direct launches differ in {case.differs(D)}: the kernel is not deterministic")
        rec["direct2"] = "equal"
        # 2. D is a real result: written, guards intact
        for o in case.outs:
            if o.chk is not None:
                o.chk.assert_intact(f"{case.name} {o.name}")
                if o.full and not o.inout:
                    o.chk.assert_fully_written(f"{case.name} {o.name}")
            _require(not torch.equal(o.bits, o.init), case, "direct", f"output {o.name} is unchanged by a direct launch")
        # 3. record: launches nothing, reports the ops
        case.restore()
        case.host.clear()
        prog = drv.record(case)
        _require(not case.differs([o.init for o in case.outs]), case, "record",
                 f"recording wrote {case.differs([o.init for o in case.outs])}: a recording must launch nothing")
        _require(prog.num_ops == len(case.ops) and prog.op_names() == case.ops, case, "record",
                 f"program reports {prog.op_names()}, expected {case.ops}")
        rec["record"] = "clean"
        # 4. destroy what the caller owned, move every "same results" switch
        rec["host_objects"] = case.destroy_host()
        drv.set_knobs(other_knobs)
        # 5. eager replay
        case.restore()
        prog.run()
        drv.sync()
        _require(not case.differs(D), case, "eager", f"eager replay differs from the direct launch in {case.differs(D)}")
        rec["eager"] = "equal"
        # 6. every run_range split
        n = prog.num_ops
        for k in range(1, n):
            case.restore()
            prog.run_range(0, k)
            prog.run_range(k, n)
            drv.sync()
            _require(not case.differs(D), case, f"run_range split {k}", f"differs in {case.differs(D)}")
        rec["ranges"] = f"equal({max(n - 1, 0)})"
        # 7. graph, on the current stream and on a second non-default stream
        prog.instantiate()
        case.restore()
        drv.sync()
        prog.launch()
        drv.sync()
        _require(not case.differs(D), case, "graph", f"graph launch differs in {case.differs(D)}")
        case.restore()
        drv.launch_on_second_stream(prog)
        _require(not case.differs(D), case, "graph, second stream", f"differs in {case.differs(D)}")
        rec["graph"] = rec["graph_s2"] = "equal"
        # 8. time_ops
        case.restore()
        drv.sync()
        times = prog.time_ops()
        drv.sync()
        _require(len(times) == n and all(math.isfinite(t) and t >= 0 for t in times), case, "time_ops", f"times {times}")
        _require(not case.differs(D), case, "time_ops", f"differs in {case.differs(D)}")
        rec["time_ops"] = "equal"
        # new values in the same device buffers (scheduler parameter rows): a replay must see them
        if case.mutate is not None:
            case.mutate()
            for pair in case.inputs:
                pair[1] = pair[0].clone()
            drv.set_knobs(record_knobs)
            case.restore()
            drv.direct(case)
            D2 = case.snapshot()
            case.host.clear()
            _require(case.differs(D), case, "mutate", "the new parameter values do not change the direct result: the case proves nothing")
            drv.set_knobs(other_knobs)
            for mode, go in (("eager", prog.run), ("graph", prog.launch)):
                case.restore()
                drv.sync()
                go()
                drv.sync()
                _require(not case.differs(D2), case, f"new values, {mode}", f"replay does not see the rewritten device buffers: {case.differs(D2)}")
            rec["new_values"] = "equal"
    finally:
        drv.set_knobs({k: d for k, (d, _) in KNOBS.items()})
    return rec


def format_record(rec):
    keys = ("direct2", "record", "eager", "ranges", "graph", "graph_s2", "time_ops", "new_values")
    return f"{rec['case']:<44} ops {rec['ops']:>2}  " + "  ".join(f"{k} {rec[k]}" for k in keys if k in rec)


class GpuDriver:
    def sync(self):
        torch.cuda.synchronize()

    def set_knobs(self, values):
        from latentblending_amd.hip import lib
        for name, v in values.items():
            getattr(lib.api, name)(v)

    def direct(self, case):
        with track_host(case):
            case.thunk()
        torch.cuda.synchronize()

    def record(self, case):
        from latentblending_amd.native.runtime import Program
        prog = Program(case.name)
        with track_host(case), prog.record():
            case.thunk()
        torch.cuda.synchronize()
        return prog

    def launch_on_second_stream(self, prog):
        torch.cuda.synchronize()
        s2 = torch.cuda.Stream()
        prog.launch(s2.cuda_stream)
        s2.synchronize()
        torch.cuda.synchronize()


# ====================================================================== the registry ===========
REGISTRY = []           # (case id, launcher names, builder)


def case(case_id, *launchers):
    def deco(fn):
        REGISTRY.append((case_id, launchers, fn))
        return fn
    return deco


def registered_launchers():
    return {name for _, launchers, _ in REGISTRY for name in launchers}


def _api():
    from latentblending_amd.hip import lib
    return lib.api


def _lib():
    from latentblending_amd.hip import lib
    return lib


def _ops():
    from latentblending_amd.hip import ops
    return ops


def _kb():
    import test_kernel_bounds_gpu as KB          # its operand builders (poisoned pads, NaN rows behind every operand)
    return KB


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rnd(*shape, **kw):
    from _parity import rnd
    return rnd(*shape, **kw)


def _decoy(c, nbytes=1 << 22):
    t = torch.full((nbytes,), 0x3C, dtype=U8, device=DEV)
    c.keep.append(t)
    c.decoy = t.data_ptr()
    return t


def _tracked_array(c, ctype, values):
    arr = (ctype * len(values))(*values)
    c.host.append(arr)
    return arr


def _reg(c, *tensors):
    """Register operands that other helpers built (views into poisoned buffers) as inputs of the case."""
    for t in tensors:
        c.inp(t)
    return tensors[0] if len(tensors) == 1 else tensors


# ---------------------------------------------------------------------- GEMM --------------------
GEMM_REPLAY_SHAPES = [(65, 132, 72), (300, 260, 128)]
# (variant, forced tile): the register ring has tiles 1-3; the direct-to-LDS family all of 1-5, 7, 10, 11; 9 = the ping-pong loop
GEMM_REPLAY_CONFIGS = [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (1, 7), (1, 10), (1, 11), (-1, 9)]


def _gemm_case(variant, tile, M, N, K):
    def build():
        KB, o, l = _kb(), _ops(), _lib()
        api = l.api
        d, dk, g = KB._gemm_operands(M, N, K), KB._gemm_operands(M, N, 512), KB._geglu_operands(M, K)
        ln = KB._ln_operands(M, N, K) if variant != 0 else None
        n_ops = 8 if variant != 0 else 7
        c = Case(f"gemm_v{variant}t{tile}_{M}x{N}x{K}", ["lb_gemm_f16"] * n_ops)
        for dd in (d, dk):
            _reg(c, dd["A_d"], dd["W_d"], dd["bias_d"], dd["res_d"], dd["res32_d"], dd["rv_d"])
        _reg(c, g["A_d"], g["W_d"], g["bias_d"])
        if ln:
            _reg(c, ln["A_d"], ln["W_d"], ln["bias_d"], ln["colsum_d"])
        ws = c.scratch(api.lb_gemm_workspace_bytes(M, N) // 4, F32)          # the split-K slabs, owned by the test
        rpb = KB._rpb(M)
        # in place: residual == C (what unet.py / clip.py emit), the buffer starts as the residual
        c_res = c.guarded("inplace_residual", M, N, N + 12, F16, fill=d["res"])
        c_geglu = c.guarded("geglu", M, 132, 132 + 4, F16)
        c_ln = c.guarded("ln_fold", M, N, N + 8, F16) if ln else None
        c_tr = c.guarded("trans_out", N, M, M + 3, F16)
        c_f32 = c.guarded("f32_out_f32_residual", M, N, N + 4, F32)
        c_rv = c.guarded("rowvec", M, N, N + 12, F16)
        c_sk2 = c.guarded("splitk2_inplace_residual", M, N, N + 12, F16, fill=dk["res"])
        c_sk5 = c.guarded("splitk5_inplace_residual", M, N, N + 4, F16, fill=dk["res"])

        def thunk():
            api.lb_gemm_set_variant(variant, 0)
            api.lb_gemm_set_tuning(tile, 0)
            try:
                o.gemm(d["A_d"], d["W_d"], bias=d["bias_d"], residual=c_res, out=c_res, workspace=ws)
                o.gemm(g["A_d"], g["W_d"], bias=g["bias_d"], flags=l.GEMM_GEGLU, out=c_geglu)
                if ln:
                    o.gemm(ln["A_d"], ln["W_d"], bias=ln["bias_d"], ln=(ln["colsum_d"], 1e-5), out=c_ln)
                o.gemm(d["A_d"], d["W_d"], flags=l.GEMM_TRANS_OUT, out=c_tr, workspace=ws)
                o.gemm(d["A_d"], d["W_d"], bias=d["bias_d"], residual=d["res32_d"], alpha=0.5,
                       flags=l.GEMM_OUT_F32 | l.GEMM_RES_F32, out=c_f32, workspace=ws)
                o.gemm(d["A_d"], d["W_d"], rowvec=d["rv_d"], rows_per_batch=rpb, out=c_rv, workspace=ws)
                api.lb_gemm_set_tuning(tile, 2)
                o.gemm(dk["A_d"], dk["W_d"], bias=dk["bias_d"], residual=c_sk2, out=c_sk2, workspace=ws)
                api.lb_gemm_set_tuning(tile, 5)
                o.gemm(dk["A_d"], dk["W_d"], bias=dk["bias_d"], residual=c_sk5, out=c_sk5, workspace=ws)
            finally:
                api.lb_gemm_set_variant(-1, 0)
                api.lb_gemm_set_tuning(0, 0)
        c.thunk = thunk
        return c.freeze()
    return build


for _cfg in GEMM_REPLAY_CONFIGS:
    for _shape in GEMM_REPLAY_SHAPES:
        case(f"gemm_v{_cfg[0]}t{_cfg[1]}_{'x'.join(map(str, _shape))}", "lb_gemm_f16")(_gemm_case(*_cfg, *_shape))


# ---------------------------------------------------------------------- convolutions ------------
def _conv_params(x, w, bias, out, B, H, Wd, Cin, N, ks, ldc, ldx, zero_page, flags=0, scatter=0):
    """LbGemmParams of a 3x3 / pad 1 (ks = 3) or one-launch sub-pixel 2x2 (ks = 2, scatter = 2) conv on NHWC x."""
    l = _lib()
    g = l.ConvGeom.conv3x3(H, Wd, Cin, ldx=ldx) if ks == 3 else l.ConvGeom(H, Wd, Cin, ks, ks, ldx=ldx, parity="all" if scatter else None)
    return l.gemm_params(A=x.data_ptr(), W=w.data_ptr(), C=out.data_ptr(), bias=bias.data_ptr(), M=B * H * Wd, N=N, K=g.K, ldw=w.stride(0),
                         ldc=ldc, conv=g, flags=flags, zero_page=zero_page.data_ptr())


def _halo_operands(c, B, H, Wd, Cin, Cout, ldx_pad=8, seed=90):
    KB, o = _kb(), _ops()
    from _guard import poisoned
    x, w = _rnd(B, Cin, H, Wd, seed=seed), _rnd(Cout, Cin, 3, 3, seed=seed + 1, scale=(Cin * 9) ** -0.5)
    b = _rnd(Cout, seed=seed + 2, dtype=F32)
    x_d = c.inp(KB._nhwc_poisoned(x, Cin, Cin + ldx_pad))
    w_d = c.inp(poisoned(o.pack_conv_weight(w, Cin), Cout, 9 * Cin, 9 * Cin, NAN, DEV))
    return x_d, w_d, c.dev(b)


@case("conv_routing", "lb_gemm_f16")
def _conv_routing():
    """Convs through lb_gemm_f16 that land on the halo, narrow and upconv kernels, and one that stays an implicit GEMM: the
    recorded op name is the routed one."""
    KB, o, l = _kb(), _ops(), _lib()
    from _guard import poisoned
    c = Case("conv_routing", ["lb_conv3x3_halo_f16", "lb_conv3x3_narrow_f16", "lb_upconv2x_halo_f16", "lb_gemm_f16"])
    # halo: (1, 8, 96, 64, 64) of the bounds test, bias + residual
    B, H, Wd, Cin, Cout = 1, 8, 96, 64, 64
    hx, hw, hb = _halo_operands(c, B, H, Wd, Cin, Cout)
    hres = c.inp(poisoned(_rnd(B * H * Wd, Cout, seed=93), B * H * Wd, Cout, Cout + 12, NAN, DEV).unflatten(0, (B, H, Wd)))
    hout = c.guarded("halo", B * H * Wd, Cout, Cout + 8, F16).unflatten(0, (B, H, Wd))
    # narrow: (3, 16, 64, 7) of the bounds test, fp32 output
    nB, nH, nCin, nCout = 3, 16, 64, 7
    nx, nw = _rnd(nB, nCin, nH, nH, seed=201), _rnd(nCout, nCin, 3, 3, seed=202, scale=(9 * nCin) ** -0.5)
    wp = torch.zeros(8, 9 * nCin, dtype=F16)
    wp[:nCout] = o.pack_conv_weight(nw, nCin)
    bp = torch.zeros(8, dtype=F32)
    bp[:nCout] = _rnd(nCout, seed=203, dtype=F32)
    nx_d, nw_d, nb_d = c.inp(KB._nhwc_poisoned(nx, nCin, nCin + 8)), c.inp(poisoned(wp, 8, 9 * nCin, 9 * nCin, NAN, DEV)), c.dev(bp)
    nout = c.guarded("narrow", nB * nH * nH, 8, 8 + 4, F32).unflatten(0, (nB, nH, nH))
    # upconv: the case of the bounds test (N = 200: a last channel block that overhangs N)
    uB, uH, uCin, uCout = 2, 16, 64, 200
    ux, uw = _rnd(uB, uCin, uH, uH, seed=190), _rnd(uCout, uCin, 3, 3, seed=191, scale=(9 * uCin) ** -0.5)
    subs = o.subpixel_upsample_weights(uw)
    w4 = torch.stack([subs[(0, 0)], subs[(0, 1)], subs[(1, 0)], subs[(1, 1)]]).reshape(4 * uCout, 4 * uCin)
    uw_d, ux_d = c.inp(poisoned(w4, 4 * uCout, 4 * uCin, 4 * uCin, NAN, DEV)), c.inp(KB._nhwc_poisoned(ux, uCin, uCin + 8))
    ub_d = c.dev(_rnd(uCout, seed=192, dtype=F32))
    uout = c.guarded("upconv", uB * 4 * uH * uH, uCout, uCout + 8, F16).unflatten(0, (uB, 2 * uH, 2 * uH))
    # implicit GEMM: stride 2 is no halo / narrow shape
    ic = KB.CONV_ROWS[1]
    d = KB._conv_operands(ic)
    _reg(c, d["x_d"], d["w_d"], d["b_d"])
    iB, ho, wo = ic[0], d["ref"].shape[1], d["ref"].shape[2]
    iout = c.guarded("implicit", iB * ho * wo, d["cout_p"], d["cout_p"] + 8, F16).unflatten(0, (iB, ho, wo))
    ws = c.scratch(l.api.lb_gemm_workspace_bytes(uB * 4 * uH * uH, 256) // 4, F32)

    def thunk():
        l.api.lb_gemm_set_halo(2)
        try:
            o.gemm(hx, hw, bias=hb, residual=hres, out=hout, conv=dict(KH=3, KW=3, stride=1, pad=1), workspace=ws)
            o.gemm(nx_d, nw_d, bias=nb_d, flags=l.GEMM_OUT_F32, out=nout, conv=dict(KH=3, KW=3, stride=1, pad=1), workspace=ws)
            o.gemm(ux_d, uw_d[:uCout], bias=ub_d, out=uout, conv=dict(KH=2, KW=2, stride=1, pad=0, parity="all"), workspace=ws)
            o.gemm(d["x_d"], d["w_d"], bias=d["b_d"], out=iout, conv=dict(KH=ic[5], KW=ic[5], stride=ic[6], pad=ic[7], ups=ic[8]),
                   workspace=ws)
        finally:
            l.api.lb_gemm_set_halo(1)
    c.thunk = thunk
    return c.freeze()


@case("conv_direct_launchers", "lb_conv3x3_halo_f16", "lb_conv3x3_narrow_f16", "lb_upconv2x_halo_f16")
def _conv_direct():
    """The three conv launchers called by name (TW = 16 halo tiling, ragged N = 132), parameter structs owned by the test."""
    KB, o, l = _kb(), _ops(), _lib()
    from _guard import poisoned
    c = Case("conv_direct_launchers", ["lb_conv3x3_halo_f16", "lb_conv3x3_narrow_f16", "lb_upconv2x_halo_f16"])
    zp = o.zero_page(DEV)
    B, H, Wd, Cin, Cout = 3, 16, 16, 192, 132
    hx, hw, hb = _halo_operands(c, B, H, Wd, Cin, Cout, ldx_pad=0)
    hout = c.guarded("halo", B * H * Wd, Cout, Cout + 4, F16)
    nB, nH, nCin = 3, 16, 64
    nx = _rnd(nB, nCin, nH, nH, seed=201)
    wp = torch.zeros(8, 9 * nCin, dtype=F16)
    wp[:7] = o.pack_conv_weight(_rnd(7, nCin, 3, 3, seed=202, scale=(9 * nCin) ** -0.5), nCin)
    nx_d, nw_d = c.inp(KB._nhwc_poisoned(nx, nCin, nCin)), c.inp(poisoned(wp, 8, 9 * nCin, 9 * nCin, NAN, DEV))
    nb_d = c.dev(_rnd(8, seed=203, dtype=F32))
    nout = c.guarded("narrow", nB * nH * nH, 8, 8, F16)
    uB, uH, uCin, uCout = 2, 16, 64, 200
    subs = o.subpixel_upsample_weights(_rnd(uCout, uCin, 3, 3, seed=191, scale=(9 * uCin) ** -0.5))
    w4 = torch.stack([subs[(0, 0)], subs[(0, 1)], subs[(1, 0)], subs[(1, 1)]]).reshape(4 * uCout, 4 * uCin)
    uw_d = c.inp(poisoned(w4, 4 * uCout, 4 * uCin, 4 * uCin, NAN, DEV))
    ux_d = c.inp(KB._nhwc_poisoned(_rnd(uB, uCin, uH, uH, seed=190), uCin, uCin))
    ub_d = c.dev(_rnd(uCout, seed=192, dtype=F32))
    uout = c.guarded("upconv", uB * 4 * uH * uH, uCout, uCout + 4, F16)

    def thunk():
        ph = _conv_params(hx, hw, hb, hout, B, H, Wd, Cin, Cout, 3, Cout + 4, Cin, zp)
        pn = _conv_params(nx_d, nw_d, nb_d, nout, nB, nH, nH, nCin, 8, 3, 8, nCin, zp)
        pu = _conv_params(ux_d, uw_d, ub_d, uout, uB, uH, uH, uCin, uCout, 2, uCout + 4, uCin, zp, scatter=2)
        c.host.extend([ph, pn, pu])
        l.api.lb_conv3x3_halo_f16(C.byref(ph), _stream())
        l.api.lb_conv3x3_narrow_f16(C.byref(pn), _stream())
        l.api.lb_upconv2x_halo_f16(C.byref(pu), _stream())
    c.thunk = thunk
    return c.freeze()


@case("halo_ch_stats_groupnorm_from_stats", "lb_gemm_f16", "lb_groupnorm_from_stats")
def _halo_stats():
    """A routed halo conv that leaves its channel statistics, and lb_groupnorm_from_stats consuming them."""
    o, l = _ops(), _lib()
    c = Case("halo_ch_stats_groupnorm_from_stats", ["lb_conv3x3_halo_f16", "lb_groupnorm_from_stats"])
    B, H, Wd, Cin, Cout = 1, 8, 96, 64, 64
    x_d, w_d, b_d = _halo_operands(c, B, H, Wd, Cin, Cout, seed=211)
    l.api.lb_gemm_set_halo(2)
    try:
        rows = o.conv_ch_stat_rows(B, H, Wd, Cin, Cout)
    finally:
        l.api.lb_gemm_set_halo(1)
    assert rows > 0
    st = c.guarded("ch_stats", Cout, B * rows * 2, B * rows * 2, F32).view(Cout, B * rows, 2)
    y = c.guarded("conv_out", B * H * Wd, Cout, Cout + 8, F16).unflatten(0, (B, H, Wd))
    out = c.guarded("normalised", B * H * Wd, Cout, Cout + 16, F16)
    gamma, beta = c.dev(1 + 0.1 * _rnd(Cout, seed=215, dtype=F32)), c.dev(0.1 * _rnd(Cout, seed=216, dtype=F32))
    ws = c.scratch(l.api.lb_groupnorm_workspace_bytes(B, 32) // 8, F64)

    def thunk():
        l.api.lb_gemm_set_halo(2)
        try:
            o.gemm(x_d, w_d, bias=b_d, alpha=0.5, out=y, conv=dict(KH=3, KW=3, stride=1, pad=1), ch_stats=st, splitk_ws=False)
        finally:
            l.api.lb_gemm_set_halo(1)
        o.groupnorm_from_stats(y, gamma, beta, 32, 1e-6, True, st, rows, ldx=Cout + 8, ldy=Cout + 16, out=out, workspace=ws)
    c.thunk = thunk
    return c.freeze()


@case("halo_ch_stats_groupnorm_affine_from_stats", "lb_gemm_f16", "lb_groupnorm_affine_from_stats")
def _halo_stats_affine():
    """The same producer, and lb_groupnorm_affine_from_stats turning its statistics into the [B][C] (scale, shift) table of a conv
    flagged LB_GEMM_GN_A.  Two samples: the smallest batch at which the per-sample indexing of the table can go wrong."""
    o, l = _ops(), _lib()
    c = Case("halo_ch_stats_groupnorm_affine_from_stats", ["lb_conv3x3_halo_f16", "lb_groupnorm_affine_from_stats"])
    B, H, Wd, Cin, Cout = 2, 8, 96, 64, 64
    x_d, w_d, b_d = _halo_operands(c, B, H, Wd, Cin, Cout, seed=221)
    l.api.lb_gemm_set_halo(2)
    try:
        rows = o.conv_ch_stat_rows(B, H, Wd, Cin, Cout)
    finally:
        l.api.lb_gemm_set_halo(1)
    assert rows > 0
    st = c.guarded("ch_stats", Cout, B * rows * 2, B * rows * 2, F32).view(Cout, B * rows, 2)
    y = c.guarded("conv_out", B * H * Wd, Cout, Cout + 8, F16).unflatten(0, (B, H, Wd))
    table = c.guarded("table", B, Cout * 2, Cout * 2, F32, back_rows=2)
    gamma, beta = c.dev(1 + 0.1 * _rnd(Cout, seed=225, dtype=F32)), c.dev(0.1 * _rnd(Cout, seed=226, dtype=F32))

    def thunk():
        l.api.lb_gemm_set_halo(2)
        try:
            o.gemm(x_d, w_d, bias=b_d, alpha=0.5, out=y, conv=dict(KH=3, KW=3, stride=1, pad=1), ch_stats=st, splitk_ws=False)
        finally:
            l.api.lb_gemm_set_halo(1)
        o.groupnorm_affine_from_stats(gamma, beta, 32, 1e-6, st, rows, B, H * Wd, out=table)
    c.thunk = thunk
    return c.freeze()


# ---------------------------------------------------------------------- norms -------------------
def _groupnorm_case(name, B, HW, Cc, f32_in, fused):
    def build():
        o, l = _ops(), _lib()
        from _guard import poisoned
        c = Case(name, ["lb_groupnorm_nhwc"])
        c.knobs["lb_groupnorm_set_fused"] = fused
        l.api.lb_groupnorm_set_fused(fused)
        try:
            assert l.api.lb_groupnorm_plan(HW, Cc, 32, int(f32_in)) == (1 if fused and not f32_in else 0), "case no longer takes its form"
        finally:
            l.api.lb_groupnorm_set_fused(1)
        x = _rnd(B * HW, Cc, seed=45, scale=2.0, dtype=F32 if f32_in else F16) + 0.5
        x_d = c.inp(poisoned(x, B * HW, Cc, Cc + 32, NAN, DEV).unflatten(0, (B, HW)))
        gamma, beta = c.dev(_rnd(Cc, seed=46, dtype=F32) * 0.1 + 1), c.dev(_rnd(Cc, seed=47, dtype=F32) * 0.1)
        out = c.guarded("y", B * HW, Cc, Cc + 8, F16)
        ws = c.scratch(l.api.lb_groupnorm_workspace_bytes(B, 32) // 8, F64)
        c.thunk = lambda: o.groupnorm_nhwc(x_d, gamma, beta, 32, 1e-5, True, ldx=Cc + 32, ldy=Cc + 8, out=out, workspace=ws)
        return c.freeze()
    return build


case("groupnorm_one_launch_f16", "lb_groupnorm_nhwc")(_groupnorm_case("groupnorm_one_launch_f16", 2, 250, 640, False, 1))
case("groupnorm_two_launch_f16", "lb_groupnorm_nhwc")(_groupnorm_case("groupnorm_two_launch_f16", 2, 64, 32, False, 0))
case("groupnorm_two_launch_f32", "lb_groupnorm_nhwc")(_groupnorm_case("groupnorm_two_launch_f32", 1, 250, 128, True, 1))


def _layernorm_case(name, M, Cc, form):
    def build():
        l = _lib()
        from _guard import poisoned
        c = Case(name, ["lb_layernorm_f16"])
        c.knobs["lb_layernorm_set_form"] = form
        x_d = c.inp(poisoned(_rnd(M, Cc, seed=48, scale=3.0) + 1, M, Cc, Cc + 8, NAN, DEV))
        g_d, b_d = c.dev(_rnd(Cc, seed=49, dtype=F32) * 0.1 + 1), c.dev(_rnd(Cc, seed=50, dtype=F32) * 0.1)
        out = c.guarded("y", M, Cc, Cc + 16, F16)
        c.thunk = lambda: l.api.lb_layernorm_f16(x_d.data_ptr(), out.data_ptr(), g_d.data_ptr(), b_d.data_ptr(), M, Cc, Cc + 8,
                                                 Cc + 16, 1e-5, _stream())
        return c.freeze()
    return build


for _form in (1, 0):
    for _m, _c in ((9, 1032), (5, 64)):
        case(f"layernorm_form{_form}_{_m}x{_c}", "lb_layernorm_f16")(_layernorm_case(f"layernorm_form{_form}_{_m}x{_c}", _m, _c, _form))


# ---------------------------------------------------------------------- attention ---------------
ATTN_ONE_TILE, ATTN_LONG, ATTN_CAUSAL = (2, 2, 130, 80, 77), (2, 3, 300, 300, 300), (2, 12, 77, 77, 77)
# (id, shape, causal, force): force bits 0..1 = query groups per block, 32 = the 5-stage ring, 512 = the ping-pong form
ATTN_REPLAY = [("one_tile_qg1_valid77of80", ATTN_ONE_TILE, False, 1), ("one_tile_qg2_valid77of80", ATTN_ONE_TILE, False, 2),
               ("streaming_qg1", ATTN_LONG, False, 1), ("streaming_qg2", ATTN_LONG, False, 2),
               ("pingpong_qg1", ATTN_LONG, False, 513), ("pingpong_qg2", ATTN_LONG, False, 514),
               ("ring5_qg1", ATTN_LONG, False, 33), ("causal_auto", ATTN_CAUSAL, True, 0)]


def _attn_case(name, shape, causal, force):
    def build():
        KB, o, l = _kb(), _ops(), _lib()
        B, H, Sq, Skv, valid = shape
        Cc = H * 64
        _, q, k, v = KB._attn_operands(B, H, Sq, Skv, valid, 64, causal)
        c = Case(name, ["lb_attn_fwd_d64"])
        _reg(c, q, k, v)
        out = c.guarded("o", B * Sq, Cc, Cc + 64, F16)

        def thunk():
            l.api.lb_attn_set_tuning(force)           # (read when the launcher is called: the closure carries it)
            try:
                o.attention_d64(q, k, v, B, H, Sq, Skv, valid, out=out, causal=causal)
            finally:
                l.api.lb_attn_set_tuning(0)
        c.thunk = thunk
        return c.freeze()
    return build


for _id, _shape, _causal, _force in ATTN_REPLAY:
    case(f"attn_d64_{_id}", "lb_attn_fwd_d64")(_attn_case(f"attn_d64_{_id}", _shape, _causal, _force))


@case("attn_d512", "lb_attn_fwd_d512")
def _attn512():
    KB, o = _kb(), _ops()
    B, H, Sq, Skv, valid = 2, 1, 100, 77, 70
    _, q, k, v = KB._attn_operands(B, H, Sq, Skv, valid, 512, False)
    c = Case("attn_d512", ["lb_attn_fwd_d512"])
    _reg(c, q, k, v)
    out = c.guarded("o", B * Sq, 512, 512 + 8, F16)
    c.thunk = lambda: o.attention_d512(q, k, v, B, H, Sq, Skv, valid, out=out)
    return c.freeze()


@case("softmax_rows_in_place", "lb_softmax_rows_f16")
def _softmax():
    o = _ops()
    c = Case("softmax_rows_in_place", ["lb_softmax_rows_f16"])
    buf = c.guarded("x", 7, 304, 312, F16, fill=_rnd(7, 304, seed=57, scale=4.0))
    c.thunk = lambda: o.softmax_rows_(buf, 0.3)
    return c.freeze()


# ---------------------------------------------------------------------- mixing ------------------
def _slerp_pairs_case(name, launcher, dtype):
    def build():
        l = _lib()
        c = Case(name, [launcher])
        _decoy(c)
        G, n = 17, 8 * 37                 # more than one LB_MAX_PAIRS chunk; pair 16 starts one element off 16-byte alignment, so
        a = c.dev(_rnd(G, n + 8, seed=71, dtype=dtype))       # its chunk takes the scalar kernel while the first stays vectorised
        b = c.dev(_rnd(G, n + 8, seed=72, dtype=dtype))
        fr = [0.0, 1.0, 0.5, 0.37, 0.8] + [0.05 * g for g in range(5, G)]
        odt = F16 if dtype == F16 else F32
        outs = [c.guarded(f"pair{g}", 1, n, n, odt, back_rows=1) for g in range(G)]
        off = lambda g: 1 if g == G - 1 else 0          # noqa: E731
        pa = [a[g, off(g):off(g) + n].data_ptr() for g in range(G)]
        pb = [b[g, off(g):off(g) + n].data_ptr() for g in range(G)]
        po = [t.data_ptr() for t in outs]

        def thunk():
            arrs = [_tracked_array(c, C.c_void_p, p) for p in (pa, pb, po)]
            frh = _tracked_array(c, C.c_double, fr)
            getattr(l.api, launcher)(*[C.cast(x, l.c_void_pp) for x in arrs], frh, G, n, _stream())
        c.thunk = thunk
        return c.freeze()
    return build


for _sfx, _dt in (("f16", F16), ("f32", F32), ("f64", F64)):
    case(f"slerp_pairs_{_sfx}", f"lb_slerp_pairs_{_sfx}")(_slerp_pairs_case(f"slerp_pairs_{_sfx}", f"lb_slerp_pairs_{_sfx}", _dt))


@case("slerp_batched_and_strided", "lb_slerp_batched_f16", "lb_slerp_strided_f16")
def _slerp_dev():
    """Device-fraction slerps: n = 296 (register-staged) and n = 32776 (> 32768: the two-pass / LDS-staged forms), strided with
    stride n and with stride 0 (broadcast)."""
    l = _lib()
    G = 5
    c = Case("slerp_batched_and_strided", ["lb_slerp_batched_f16", "lb_slerp_strided_f16", "lb_slerp_strided_f16"] * 2)
    frd = c.dev(torch.tensor([0.0, 1.0, 0.5, 0.37, 0.8], dtype=F64))
    calls = []
    for n in (8 * 37, 32768 + 8):
        a, b = c.dev(_rnd(G, n, seed=71)), c.dev(_rnd(G, n, seed=72))
        ob, os_, o0 = [c.guarded(f"{k}_n{n}", G, n, n, F16, back_rows=2) for k in ("batched", "strided", "broadcast")]
        calls.append((a, b, ob, os_, o0, n))

    def thunk():
        for a, b, ob, os_, o0, n in calls:
            l.api.lb_slerp_batched_f16(a.data_ptr(), b.data_ptr(), ob.data_ptr(), frd.data_ptr(), G, n, _stream())
            l.api.lb_slerp_strided_f16(a.data_ptr(), n, b.data_ptr(), n, os_.data_ptr(), frd.data_ptr(), G, n, _stream())
            l.api.lb_slerp_strided_f16(a.data_ptr(), 0, b.data_ptr(), 0, o0.data_ptr(), frd.data_ptr(), G, n, _stream())
    c.thunk = thunk
    return c.freeze()


@case("lerp", "lb_lerp_f16", "lb_lerp_f32")
def _lerp():
    """The ``double fract`` argument is captured by value (a scalar tail: n = 8 * 37 + 3)."""
    l = _lib()
    n = 8 * 37 + 3
    c = Case("lerp", ["lb_lerp_f16", "lb_lerp_f32"])
    a16, b16, a32, b32 = (c.dev(_rnd(1, n, seed=s, dtype=dt)) for s, dt in ((11, F16), (12, F16), (11, F32), (12, F32)))
    o16, o32 = c.guarded("f16", 1, n, n, F16, back_rows=1), c.guarded("f32", 1, n, n, F32, back_rows=1)

    def thunk():
        f = C.c_double(0.7321)
        c.host.append(f)
        l.api.lb_lerp_f16(a16.data_ptr(), b16.data_ptr(), o16.data_ptr(), n, f, _stream())
        l.api.lb_lerp_f32(a32.data_ptr(), b32.data_ptr(), o32.data_ptr(), n, f, _stream())
    c.thunk = thunk
    return c.freeze()


@case("scheduler_steps", "lb_scale_model_input_f16", "lb_euler_step_f16", "lb_ddim_step_f16")
def _scheduler():
    """The three scheduler steps read their sigma / dt / guidance rows from ``params_dev`` at replay: the protocol rewrites the rows
    after the recording and requires every replay to follow."""
    o, l = _ops(), _lib()
    B, n, g = 2, 8 * 37 + 3, 3.5
    c = Case("scheduler_steps", ["lb_scale_model_input_f16", "lb_scale_model_input_f16", "lb_euler_step_f16", "lb_euler_step_f16",
                                 "lb_euler_step_f16", "lb_ddim_step_f16", "lb_ddim_step_f16"])
    x, eps, noise = c.dev(_rnd(B, n, seed=15, scale=5.0)), c.dev(_rnd(2 * B, n, seed=16)), c.dev(_rnd(B, n, seed=17))
    params = c.inp(o.step_params([(4.2, 3.1, 0.0, g, -1.1)] * B, DEV))
    params_anc = c.inp(o.step_params([(4.2, 2.6, 1.7, g, -1.6)] * B, DEV))
    from latentblending_amd.native.scheduler import NativeDDIMScheduler
    nd = NativeDDIMScheduler(device=DEV)
    nd.set_timesteps(30)
    params_ddim = c.inp(o.step_params([nd.step_row(13, g)] * B, DEV))
    outs = {k: c.guarded(k, rows, n, n, F16, back_rows=2) for k, rows in
            (("scale", B), ("scale_dup", 2 * B), ("euler", B), ("euler_ancestral", B), ("euler_cfg", B), ("ddim", B), ("ddim_cfg", B))}
    P = lambda t: t.data_ptr()      # noqa: E731

    def thunk():
        a, s = l.api, _stream()
        a.lb_scale_model_input_f16(P(x), P(outs["scale"]), P(params), n, B, 0, s)
        a.lb_scale_model_input_f16(P(x), P(outs["scale_dup"]), P(params), n, B, 1, s)
        a.lb_euler_step_f16(P(x), P(eps), P(noise), P(outs["euler"]), P(params), n, B, 0, 0, s)
        a.lb_euler_step_f16(P(x), P(eps), P(noise), P(outs["euler_ancestral"]), P(params_anc), n, B, 0, 1, s)
        a.lb_euler_step_f16(P(x), P(eps), None, P(outs["euler_cfg"]), P(params), n, B, 1, 0, s)
        a.lb_ddim_step_f16(P(x), P(eps), P(outs["ddim"]), P(params_ddim), n, B, 0, s)
        a.lb_ddim_step_f16(P(x), P(eps), P(outs["ddim_cfg"]), P(params_ddim), n, B, 1, s)
    c.thunk = thunk

    def mutate():
        params.copy_(o.step_params([(2.9, 1.8, 0.0, 5.0, -1.1)] * B, DEV))
        params_anc.copy_(o.step_params([(2.9, 1.3, 1.2, 5.0, -1.6)] * B, DEV))
        params_ddim.copy_(o.step_params([nd.step_row(7, 5.0)] * B, DEV))
    c.mutate = mutate
    return c.freeze()


# per sample (schedule length, step index, guidance): the rows the LCM case records under, and the ones the protocol rewrites them to
LCM_PLANS = {"recorded": [(4, 2, 3.0), (8, 4, 3.5)], "recorded_last": [(4, 3, 3.0), (8, 7, 3.5)],
             "rewritten": [(4, 0, 3.0), (8, 0, 3.5)], "rewritten_last": [(8, 7, 2.0), (3, 2, 2.0)]}
# per sample (schedule length, Karras?, step index, first step of its run?, guidance): a first-order row, a second-order row and a
# schedule's last row in one batch; rewritten to second-order rows throughout
DPMPP_PLANS = {"recorded": [(8, True, 3, True, 3.3), (20, True, 7, False, 4.0), (6, False, 5, False, 2.7)],
               "rewritten": [(8, True, 3, False, 3.0), (20, True, 7, False, 3.3), (6, False, 2, False, 2.5)]}


def _lcm_rows(plan):
    from latentblending_amd.native.scheduler import NativeLCMScheduler
    rows = []
    for n, i, g in plan:
        s = NativeLCMScheduler(device="cpu")
        s.set_timesteps(n)
        rows.append(s.step_row(i, g))
    return rows


def _dpmpp_rows(plan):
    from latentblending_amd.native.scheduler import NativeDPMSolverPP2MScheduler
    rows = []
    for n, karras, i, first, g in plan:
        s = NativeDPMSolverPP2MScheduler(use_karras_sigmas=karras, device="cpu")
        s.set_timesteps(n)
        rows.append(s.step_row(i, g, first=first))
    return rows


@case("lcm_steps", "lb_lcm_step_f16")
def _lcm_steps():
    """The latent-consistency step plain, under CFG, and on last-step rows with a null noise pointer (``all_last`` was recorded:
    the rewritten rows of that launch stay last-step rows).  tests/test_lcm_gpu.py checks the direct launch against the
    restatement; ``operands`` is what it needs for that."""
    o, l = _ops(), _lib()
    B, n = 2, 8 * 37 + 3
    c = Case("lcm_steps", ["lb_lcm_step_f16"] * 3)
    x, eps, noise = c.dev(_rnd(B, n, seed=15, scale=4.0)), c.dev(_rnd(2 * B, n, seed=16)), c.dev(_rnd(B, n, seed=17))
    params = c.inp(o.step_params(_lcm_rows(LCM_PLANS["recorded"]), DEV))
    params_last = c.inp(o.step_params(_lcm_rows(LCM_PLANS["recorded_last"]), DEV))
    outs = {k: c.guarded(k, B, n, n, F16, back_rows=2) for k in ("lcm", "lcm_cfg", "lcm_last_null_noise")}
    c.operands = dict(B=B, n=n, x=x, eps=eps, noise=noise, outs=outs)
    P = lambda t: t.data_ptr()      # noqa: E731

    def thunk():
        a, s = l.api, _stream()
        a.lb_lcm_step_f16(P(x), P(eps), P(noise), P(outs["lcm"]), P(params), n, B, 0, 0, s)
        a.lb_lcm_step_f16(P(x), P(eps), P(noise), P(outs["lcm_cfg"]), P(params), n, B, 1, 0, s)
        a.lb_lcm_step_f16(P(x), P(eps), None, P(outs["lcm_last_null_noise"]), P(params_last), n, B, 0, 1, s)
    c.thunk = thunk

    def mutate():
        params.copy_(o.step_params(_lcm_rows(LCM_PLANS["rewritten"]), DEV))
        params_last.copy_(o.step_params(_lcm_rows(LCM_PLANS["rewritten_last"]), DEV))
    c.mutate = mutate
    return c.freeze()


@case("dpmpp_steps", "lb_dpmpp2m_step_f16")
def _dpmpp_steps():
    """The DPM-Solver++ 2M step on two-plane buffers: plain, under CFG, and chained (``out`` of op 0 is ``state`` of op 2).
    tests/test_dpmpp_gpu.py checks the direct launches against the restatement; ``operands`` is what it needs for that."""
    o, l = _ops(), _lib()
    B, n = 3, 8 * 37
    c = Case("dpmpp_steps", ["lb_dpmpp2m_step_f16"] * 3)
    latents, m1 = _rnd(B, n, seed=15, scale=4.0).clamp(-15, 15), _rnd(B, n, seed=16, scale=1.5)
    x, e = c.dev(torch.stack([latents, m1])), c.dev(_rnd(2 * B, n, seed=17))
    params = c.inp(o.step_params(_dpmpp_rows(DPMPP_PLANS["recorded"]), DEV))
    outs = {k: c.guarded(k, 2 * B, n, n, F16, back_rows=2) for k in ("dpmpp", "dpmpp_cfg", "dpmpp_chained")}
    c.operands = dict(B=B, n=n, state=x, eps=e, outs=outs)
    P = lambda t: t.data_ptr()      # noqa: E731

    def thunk():
        a, s = l.api, _stream()
        a.lb_dpmpp2m_step_f16(P(x), P(e), P(outs["dpmpp"]), P(params), n, B, 0, s)
        a.lb_dpmpp2m_step_f16(P(x), P(e), P(outs["dpmpp_cfg"]), P(params), n, B, 1, s)
        a.lb_dpmpp2m_step_f16(P(outs["dpmpp"]), P(e), P(outs["dpmpp_chained"]), P(params), n, B, 0, s)
    c.thunk = thunk

    def mutate():
        params.copy_(o.step_params(_dpmpp_rows(DPMPP_PLANS["rewritten"]), DEV))
    c.mutate = mutate
    return c.freeze()


@case("counter_noise", "lb_counter_noise_f16")
def _counter_noise():
    """fp16 normals and the raw Philox words of the same rows.  3 x 2056 values are 771 sixteen-byte work items (1542 raw): no
    multiple of a wave or a block.  The key / counter rows are read when the kernel RUNS (include/lb_hip.h): the protocol rewrites
    them after the recording and requires every replay to draw the other noise."""
    o = _ops()
    n, per = 3, 2056
    c = Case("counter_noise", ["lb_counter_noise_f16", "lb_counter_noise_f16"])
    rows = c.inp(o.noise_rows([(0x243F6A88, 0x85A308D3, 7, 0, 0), (0x13198A2E, 0x03707344, 7, 0, 0), (0xA4093822, 0x299F31D0, 0, 1, 5)], DEV))
    z = c.guarded("normals", n, per, per, F16, back_rows=2)
    words = c.guarded("words", n, per, per, F32, back_rows=2)        # 32-bit words: compared as bits, never read as floats

    def thunk():
        o.counter_noise(rows, (n, per), out=z)
        o.counter_noise(rows, (n, per), raw=True, out=words.view(I32))
    c.thunk = thunk

    def mutate():
        rows.copy_(o.noise_rows([(0x243F6A88, 0x85A308D3, 8, 0, 0), (0x082EFA98, 0xEC4E6C89, 7, 0, 0), (0xA4093822, 0x299F31D0, 0, 1, 6)], DEV))
    c.mutate = mutate
    return c.freeze()


# ---------------------------------------------------------------------- LPIPS / small kernels ---
@case("lpips_tap_16_pairs", "lb_lpips_tap")
def _lpips_tap():
    """Accumulates into ``acc``: an in-out buffer that the protocol resets (to zeros) before every run."""
    o = _ops()
    import torch.nn.functional as F
    HW, Cc, npairs = 1089, 100, 16
    c = Case("lpips_tap_16_pairs", ["lb_lpips_tap"])
    _decoy(c)
    fa = [c.dev(F.relu(_rnd(HW, Cc, seed=500 + i))) for i in range(npairs)]
    fb = [c.dev(F.relu(_rnd(HW, Cc, seed=600 + i))) for i in range(npairs)]
    lin = c.dev(_rnd(Cc, seed=700, dtype=F32).abs())
    acc = c.guarded("acc", 1, npairs, npairs, F32, back_rows=1, fill=torch.zeros(1, npairs))
    ws = c.scratch(16 * 128, F32)
    c.thunk = lambda: o.lpips_tap(fa, fb, lin, acc[0], workspace=ws)
    return c.freeze()


CAP = 2048 * 256          # misc.hip launches at most 2048 blocks of 256 threads: every case below goes round the grid-stride loop twice


@case("misc_copy_cast_fill", "lb_copy_cols_f16", "lb_cast_f16_to_f32", "lb_cast_f32_to_f16", "lb_fill_f32", "lb_copy_d2d")
def _misc_copies():
    o, l = _ops(), _lib()
    from _guard import poisoned
    c = Case("misc_copy_cast_fill", ["lb_copy_cols_f16", "lb_cast_f16_to_f32", "lb_cast_f32_to_f16", "lb_fill_f32", "lb_copy_d2d"])
    rows, cols = 4100, 1032
    assert rows * (cols // 8) > CAP
    src = c.inp(poisoned(_rnd(rows, cols, seed=58), rows, cols, 1040, NAN, DEV, extra_rows=2))
    dst = c.guarded("copy_cols", rows, 2080, 2080, F16, back_rows=2, full=False)
    n = CAP + 3
    h, f = c.dev(_rnd(n, seed=301, scale=30.0)), c.dev(_rnd(n, seed=302, dtype=F32, scale=3e4))
    o32 = c.guarded("cast_f16_to_f32", 1, n, n, F32, back_rows=1)
    o16 = c.guarded("cast_f32_to_f16", 1, n, n, F16, back_rows=1)
    ofill = c.guarded("fill_f32", 1, n, n, F32, back_rows=1)
    ocopy = c.guarded("copy_d2d", 1, n, n, F16, back_rows=1)

    def thunk():
        o.copy_cols(src, dst, 1040)
        o.cast_f16_to_f32(h, out=o32[0])
        o.cast_f32_to_f16(f, 2.0 ** -3, out=o16[0])
        o.fill_f32_(ofill[0], -2.5)
        l.api.lb_copy_d2d(ocopy.data_ptr(), h.data_ptr(), n * 2, _stream())
    c.thunk = thunk
    return c.freeze()


@case("misc_layouts", "lb_nchw_to_nhwc_f16", "lb_nhwc_to_nchw_f16", "lb_maxpool3s2_nhwc_f16", "lb_sinusoid_f16")
def _misc_layouts():
    o, l = _ops(), _lib()
    from _guard import poisoned
    c = Case("misc_layouts", ["lb_nchw_to_nhwc_f16", "lb_nhwc_to_nchw_f16", "lb_maxpool3s2_nhwc_f16", "lb_sinusoid_f16"])
    B, Cc, HW, ld = 2, 4, 33000, 8
    assert B * HW * ld > CAP
    z = c.dev(_rnd(B, Cc, HW, seed=60))
    o_nhwc = c.guarded("nchw_to_nhwc", B * HW, ld, ld, F16, back_rows=2)
    HW2 = 66001
    assert B * Cc * HW2 > CAP
    nh = c.dev(_rnd(B * HW2, ld, seed=61))
    o_nchw = c.guarded("nhwc_to_nchw", B * Cc, HW2, HW2, F16, back_rows=1)
    N, H, Cp = 2, 131, 512
    Ho = (H - 3) // 2 + 1
    assert N * Ho * Ho * (Cp // 8) > CAP
    f = c.inp(poisoned(_rnd(N * H * H, Cp, seed=62), N * H * H, Cp, Cp, NAN, DEV, extra_rows=4))
    o_pool = c.guarded("maxpool", N * Ho * Ho, Cp, Cp, F16, back_rows=4)
    rows, dim, col_off, lds = 2100, 256, 24, 256 + 24 + 40
    assert rows * dim > CAP
    vals = c.inp(poisoned((torch.arange(rows, dtype=F32) * 0.4763).reshape(rows, 1), rows, 1, 3, NAN, DEV, extra_rows=2))
    o_sin = c.guarded("sinusoid", rows, lds, lds, F16, back_rows=2, full=False)

    def thunk():
        s = _stream()
        l.api.lb_nchw_to_nhwc_f16(z.data_ptr(), o_nhwc.data_ptr(), B, Cc, HW, ld, 1 / 0.13025, s)
        l.api.lb_nhwc_to_nchw_f16(nh.data_ptr(), o_nchw.data_ptr(), B, Cc, HW2, ld, s)
        l.api.lb_maxpool3s2_nhwc_f16(f.data_ptr(), o_pool.data_ptr(), N, H, H, Cp, s)
        o.sinusoid(vals, dim, out=o_sin, col_off=col_off)
    c.thunk = thunk
    return c.freeze()


@case("misc_images_and_tokens", "lb_postprocess_u8", "lb_lpips_prep_u8", "lb_embed_tokens_f16", "lb_gather_rows_f16",
      "lb_frames_lerp_u8")
def _misc_images():
    o, l = _ops(), _lib()
    from _guard import poisoned
    c = Case("misc_images_and_tokens", ["lb_postprocess_u8", "lb_postprocess_u8", "lb_lpips_prep_u8", "lb_embed_tokens_f16",
                                        "lb_gather_rows_f16", "lb_frames_lerp_u8"])
    H = 420
    assert H * H * 3 > CAP
    px16, px32 = c.dev(_rnd(H * H, 4, seed=61)), c.dev(_rnd(H * H, 4, seed=61, dtype=F32))
    o_pp16 = c.guarded("postprocess_f16", H * H, 3, 3, U8, back_rows=2)
    o_pp32 = c.guarded("postprocess_f32", H * H, 3, 3, U8, back_rows=2, sentinel=0x5A)
    Hp = 730
    assert Hp * Hp > CAP
    g = torch.Generator().manual_seed(9)
    img = c.dev((torch.rand(Hp * Hp, 3, generator=g) * 256).to(U8))
    o_prep = c.guarded("lpips_prep", Hp * Hp, 8, 8, F16, back_rows=2)
    rows, seq, Cc, vocab = 4200, 77, 1024, 1000
    assert rows * (Cc // 8) > CAP
    tok = c.inp(poisoned(_rnd(vocab, Cc, seed=401), vocab, Cc, Cc, NAN, DEV, extra_rows=2))
    pos = c.inp(poisoned(_rnd(seq, Cc, seed=402), seq, Cc, Cc, NAN, DEV, extra_rows=2))
    ids = torch.randint(0, vocab, (rows,), generator=g, dtype=I32)
    ids[0], ids[1], ids[-1], ids[-2] = -1, 1005, 1005, -1
    ids_d = c.dev(ids)
    o_emb = c.guarded("embed_tokens", rows, Cc, Cc, F16, back_rows=2)
    src = c.inp(poisoned(_rnd(300, Cc, seed=404), 300, Cc, 1032, NAN, DEV, extra_rows=2))
    idx_d = c.dev(torch.randint(0, 300, (rows,), generator=g, dtype=I32))
    o_gat = c.guarded("gather_rows", rows, Cc, Cc, F16, back_rows=2)
    frames = c.dev((torch.rand(3, 840, 840, 3, generator=g) * 256).to(U8))
    fb = frames[0].numel()
    assert fb // 16 > 512 * 256 and fb % 16 == 0
    left, wts = [0, 1, 1, 0], [0.25, 0.5, 0.999, 0.0]
    tables = (c.dev(torch.tensor(left, dtype=I32)), c.dev(torch.tensor(wts, dtype=F64)))
    o_fl = c.guarded("frames_lerp", len(left), fb, fb, U8, back_rows=1)

    def thunk():
        s = _stream()
        l.api.lb_postprocess_u8(px16.data_ptr(), o_pp16.data_ptr(), H * H, 4, 0, s)
        l.api.lb_postprocess_u8(px32.data_ptr(), o_pp32.data_ptr(), H * H, 4, 1, s)
        o.lpips_prep_u8(img, out=o_prep)
        o.embed_tokens(ids_d, tok, pos, seq, out=o_emb)
        o.gather_rows(src, idx_d, out=o_gat)
        o.frames_lerp_u8(frames, left, wts, out=o_fl.reshape(len(left), 840, 840, 3), tables=tables)
    c.thunk = thunk
    return c.freeze()


# ---------------------------------------------------------------------- movie frames ------------
@case("jpeg_both_stages", "lb_jpeg_dct_quant_u8", "lb_jpeg_entropy")
def _jpeg():
    o = _ops()
    n, h, w, code = 2, 64, 96, 0
    c = Case("jpeg_both_stages", ["lb_jpeg_dct_quant_u8", "lb_jpeg_entropy"])
    g = torch.Generator().manual_seed(5)
    base = torch.rand(n, h // 8, w // 8, 3, generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    frames = c.dev(((base * 200 + torch.rand(n, h, w, 3, generator=g) * 55)).to(U8))
    qt = c.inp(o._jpeg_qtables(92, torch.device(DEV, torch.cuda.current_device())).clone())
    count = o.api.lb_jpeg_coefficient_count(n, h, w, code)
    coef = c.guarded("coefficients", 1, count, count, I16, back_rows=1, full=False)
    ws = c.scratch(o.api.lb_jpeg_workspace_bytes(n, h, w, code), U8)
    out = c.guarded("scan_bytes", 1, n * (h * w + 4096), n * (h * w + 4096), U8, back_rows=1)
    fbytes = c.plain_out("frame_bytes", (n,), I32)

    def thunk():
        o.jpeg_dct_quant_into(frames, qt, coef.view(n, -1, 64), code)
        o.jpeg_entropy_into(coef.view(-1), ws, out.view(-1), fbytes, n, h, w, code)
    c.thunk = thunk
    return c.freeze()


@case("resample_u8", "lb_resample_u8")
def _resample():
    """Two passes, each single pass, and the copy (both axes unchanged)."""
    o = _ops()
    n, hin, win = 3, 40, 56
    c = Case("resample_u8", ["lb_resample_u8"] * 4)
    g = torch.Generator().manual_seed(6)
    frames = c.dev((torch.rand(n, hin, win, 3, generator=g) * 256).to(U8))
    dev = frames.device
    jobs = []
    for name, (hout, wout) in (("two_pass", (24, 32)), ("horizontal", (40, 32)), ("vertical", (24, 56)), ("copy", (40, 56))):
        tx, ty = o._resample_tables(hin, win, hout, wout, "bicubic", dev)
        for t in (tx, ty):
            if t is not None:
                c.keep.append(t)
        tmp = c.scratch(n * hin * wout * 3, U8).view(n, hin, wout, 3) if tx is not None and ty is not None else None
        dst = c.guarded(name, 1, n * hout * wout * 3, n * hout * wout * 3, U8, back_rows=1)
        jobs.append((tmp, dst.view(n, hout, wout, 3), tx, ty))

    def thunk():
        for tmp, dst, tx, ty in jobs:
            o.resample_u8_into(frames, tmp, dst, tx, ty)
    c.thunk = thunk
    return c.freeze()


@functools.lru_cache(maxsize=None)
def case_ids():
    return [cid for cid, _, _ in REGISTRY]


def build_case(case_id):
    for cid, _, builder in REGISTRY:
        if cid == case_id:
            c = builder()
            assert c.name == cid, (c.name, cid)
            return c
    raise KeyError(case_id)
