"""The program layer on a real MI355X: recorded, replayed and graph launches of every launcher, compared bit for bit.

Production never calls a launcher directly: the UNet / VAE / CLIP / LPIPS forwards are recorded once into an ``LbProgram``
(csrc/program.hip, ``LB_DISPATCH`` in csrc/lb_common.h, native/runtime.py:Program) and then run as closures replayed from C++ or
as one instantiated hipGraph.  The other GPU files test the launchers by direct calls; this one tests what a closure captured.

**The protocol** (``_replay.run_protocol``, applied to every case of the registry in ``_replay.py``; every comparison is
``torch.equal`` on the raw bytes of the whole output allocations, guard bands and pad columns included - no tolerance anywhere):

1. two direct launches on freshly restored inputs and poisoned outputs must agree (determinism is the premise of the rest);
2. the first result D must be fully written with its guards intact (two unwritten buffers must not pass as equal);
3. the thunk is recorded into a fresh ``Program``: the outputs must still hold the poison (a recording launches nothing), and
   ``num_ops`` / ``op_names()`` must be the case's;
4. the caller's side is destroyed: parameter structs zeroed, host pointer / fraction arrays overwritten, references dropped, and
   every "same results" switch (``_replay.KNOBS``) set to a legal value other than the one at record time;
5. an eager replay must give D; 6. so must ``run_range(0, k)`` + ``run_range(k, n)`` for every k; 7. so must the instantiated
   graph on the current stream and on a second, non-default stream; 8. so must ``time_ops()``, which returns ``num_ops`` finite,
   non-negative times.  Cases with device-resident parameters (the scheduler steps) then get new values in the same buffers and
   every replay must follow them.

Then a composite program with real data dependencies and arena buffers reused inside it, the life cycle (re-recording,
destroying, misuse, exceptions, threads), and - in a fresh child process - a graph instantiated before any eager run.
"""
import os
import subprocess
import sys
import threading
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import _replay as RP  # noqa: E402
from _guard import guarded  # noqa: E402
from _parity import rnd  # noqa: E402

DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RECORDS, _TIMES = [], {}


def lib():
    from latentblending_amd.hip import lib as l
    return l


def ops():
    from latentblending_amd.hip import ops as o
    return o


def Program(name="test"):
    from latentblending_amd.native.runtime import Program as P
    return P(name)


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module", autouse=True)
def replay_record():
    """The per-case lines (case, ops, equal or not per mode) and the run times are written to the file that the environment variable
    LB_REPLAY_RECORD names (profiles/program_replay.txt is such a record); without it they are only printed."""
    t0 = time.time()
    yield
    path = os.environ.get("LB_REPLAY_RECORD")
    if not _RECORDS or not path:
        return
    slow = max(_TIMES, key=_TIMES.get)
    with open(path, "w") as fh:
        fh.write(f"# program replay protocol: {len(_RECORDS)} registry cases, file wall time {time.time() - t0:.1f} s, "
                 f"slowest case {slow} {_TIMES[slow]:.2f} s\n")
        fh.write("\n".join(_RECORDS) + "\n")


# ====================================================================== every launcher ========
@pytest.mark.parametrize("case_id", RP.case_ids())
def test_replay_equals_direct_launch(case_id):
    t0 = time.time()
    case = RP.build_case(case_id)
    rec = RP.run_protocol(case, RP.GpuDriver())
    _TIMES[case_id] = time.time() - t0
    line = RP.format_record(rec)
    _RECORDS.append(line)
    print("[replay] " + line)


# ====================================================================== a composite program ===
class Composite:
    """About a dozen ops with real data dependencies on a 16 x 32 latent with 64 channels, 2 samples, one head of 64: halo conv
    with channel statistics -> groupnorm_from_stats -> copy_cols -> LayerNorm-folded q|k|v GEMM -> attention on column slices of
    it -> out-projection with in-place residual -> GEGLU GEMM -> forced split-K GEMM -> cast to fp32 and back -> euler_step.
    Intermediates come from a ``runtime.Arena`` and are released (and reused) inside the sequence; the inputs, the parameter rows
    and the final output belong to the test."""
    B, H, W, Cc = 2, 16, 32, 64

    def __init__(self, seed, ws):
        from latentblending_amd.native.runtime import Arena
        o, l = ops(), lib()
        B, H, W, Cc = self.B, self.H, self.W, self.Cc
        self.M, self.n = B * H * W, H * W * Cc
        self.arena, self.ws = Arena(torch.device(DEV)), ws
        self.x = rnd(B, H, W, Cc, seed=seed).to(DEV)
        self.params = o.step_params([(4.2, 3.1, 0.0, 1.0, -1.1)] * B, DEV)
        wc = rnd(Cc, Cc, 3, 3, seed=seed + 1, scale=(9 * Cc) ** -0.5)
        self.wc, self.bc = o.pack_conv_weight(wc, Cc).to(DEV), rnd(Cc, seed=seed + 2, dtype=F32).to(DEV)
        self.gamma, self.beta = (1 + 0.1 * rnd(Cc, seed=seed + 3, dtype=F32)).to(DEV), (0.1 * rnd(Cc, seed=seed + 4, dtype=F32)).to(DEV)
        wf, colsum, b2 = o.fold_layernorm(rnd(3 * Cc, Cc, seed=seed + 5, scale=Cc ** -0.5), rnd(3 * Cc, seed=seed + 6, dtype=F32),
                                          1.0 + 0.2 * rnd(Cc, seed=seed + 7, dtype=F32), 0.1 * rnd(Cc, seed=seed + 8, dtype=F32))
        self.wqkv, self.colsum, self.bqkv = wf.to(DEV), colsum.to(DEV), b2.to(DEV)
        self.wo, self.bo = rnd(Cc, Cc, seed=seed + 9, scale=Cc ** -0.5).to(DEV), rnd(Cc, seed=seed + 10, dtype=F32).to(DEV)
        self.wg, self.bg = rnd(4 * Cc, Cc, seed=seed + 11, scale=Cc ** -0.5).to(DEV), rnd(4 * Cc, seed=seed + 12, dtype=F32, scale=0.1).to(DEV)
        self.w2 = rnd(Cc, 2 * Cc, seed=seed + 13, scale=(2 * Cc) ** -0.5).to(DEV)
        self.gn_ws = torch.empty(l.api.lb_groupnorm_workspace_bytes(B, 32) // 8, dtype=F64, device=DEV)
        l.api.lb_gemm_set_halo(2)
        try:
            self.rows = o.conv_ch_stat_rows(B, H, W, Cc, Cc)
        finally:
            l.api.lb_gemm_set_halo(1)
        assert self.rows > 0
        self.out, self.chk = guarded(B, self.n, self.n, F16, DEV, back_rows=2)
        self.n_ops = 11
        self.names = ["lb_conv3x3_halo_f16", "lb_groupnorm_from_stats", "lb_copy_cols_f16", "lb_gemm_f16", "lb_attn_fwd_d64",
                      "lb_gemm_f16", "lb_gemm_f16", "lb_gemm_f16", "lb_cast_f16_to_f32", "lb_cast_f32_to_f16", "lb_euler_step_f16"]

    def new_values(self, seed):
        """New contents in the SAME input buffers and parameter rows."""
        self.x.copy_(rnd(self.B, self.H, self.W, self.Cc, seed=seed, scale=1.5).to(DEV))
        self.params.copy_(ops().step_params([(2.9, 1.8, 0.0, 1.0, -0.7)] * self.B, DEV))

    def emit(self):
        o, l, ar = ops(), lib(), self.arena
        B, H, W, Cc, M = self.B, self.H, self.W, self.Cc, self.M
        y, st = ar.alloc((B, H, W, Cc)), ar.alloc((Cc, B * self.rows, 2), F32)
        l.api.lb_gemm_set_halo(2)
        try:
            o.gemm(self.x, self.wc, bias=self.bc, out=y, conv=dict(KH=3, KW=3, stride=1, pad=1), ch_stats=st, splitk_ws=False)
        finally:
            l.api.lb_gemm_set_halo(1)
        h = ar.alloc((B, H, W, Cc))
        o.groupnorm_from_stats(y, self.gamma, self.beta, 32, 1e-6, False, st, self.rows, out=h, workspace=self.gn_ws)
        ar.release(y), ar.release(st)
        tok = ar.alloc((M, Cc))
        o.copy_cols(h.view(M, Cc), tok, 0)
        ar.release(h)
        qkv = ar.alloc((M, 3 * Cc))                                   # (reuses nothing of its size yet: a fresh class)
        o.gemm(tok, self.wqkv, bias=self.bqkv, ln=(self.colsum, 1e-5), out=qkv)
        att = ar.alloc((M, Cc))                                       # (the size class of y / h: one of their buffers comes back)
        o.attention_d64(qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:], B, 1, H * W, H * W, out=att)
        ar.release(qkv)
        o.gemm(att, self.wo, bias=self.bo, residual=tok, out=tok, workspace=self.ws)        # in place: residual == C
        ar.release(att)
        ff = ar.alloc((M, 2 * Cc))
        o.gemm(tok, self.wg, bias=self.bg, flags=l.GEMM_GEGLU, out=ff)
        ar.release(tok)
        o2 = ar.alloc((M, Cc))
        l.api.lb_gemm_set_tuning(0, 2)                                # split-K forced: the slabs go through the shared workspace
        try:
            o.gemm(ff, self.w2, out=o2, workspace=self.ws)
        finally:
            l.api.lb_gemm_set_tuning(0, 0)
        ar.release(ff)
        f32 = ar.alloc((M * Cc,), F32)
        o.cast_f16_to_f32(o2.view(-1), out=f32)
        ar.release(o2)
        eps = ar.alloc((B, self.n))
        o.cast_f32_to_f16(f32, 0.5, out=eps.view(-1))
        ar.release(f32)
        l.api.lb_euler_step_f16(self.x.data_ptr(), eps.data_ptr(), None, self.out.data_ptr(), self.params.data_ptr(), self.n, B, 0, 0,
                                stream())
        ar.release(eps)

    def poison(self):
        self.chk.bits.fill_(self.chk.sentinel)

    def direct(self):
        self.poison()
        self.emit()
        torch.cuda.synchronize()
        self.chk.assert_intact("composite output")
        self.chk.assert_fully_written("composite output")
        return self.chk.bits.clone()

    def record(self):
        self.poison()
        prog = Program("composite")
        prog.keep.append(self)
        with prog.record():
            self.emit()
        torch.cuda.synchronize()
        assert bool((self.chk.bits == self.chk.sentinel).all()), "recording the composite program wrote its output"
        assert prog.op_names() == self.names
        return prog

    def replayed(self, go):
        self.poison()
        torch.cuda.synchronize()
        go()
        torch.cuda.synchronize()
        return self.chk.bits


def _shared_ws():
    return torch.empty(lib().api.lb_gemm_workspace_bytes(Composite.B * Composite.H * Composite.W, 4 * Composite.Cc) // 4, dtype=F32,
                       device=DEV)


def test_composite_program_four_ways_and_new_values():
    cp = Composite(900, _shared_ws())
    D = cp.direct()
    assert torch.equal(cp.direct(), D), "two direct runs of the composite sequence differ"
    prog = cp.record()
    n = prog.num_ops
    assert n == cp.n_ops

    def check(want, what):
        assert torch.equal(cp.replayed(prog.run), want), f"eager replay, {what}"
        for k in range(1, n):
            assert torch.equal(cp.replayed(lambda: (prog.run_range(0, k), prog.run_range(k, n))), want), f"run_range split {k}, {what}"
        assert torch.equal(cp.replayed(prog.launch), want), f"graph, {what}"
    prog.instantiate()
    check(D, "recorded values")
    cp.new_values(901)
    D2 = cp.direct()
    assert not torch.equal(D2, D)
    check(D2, "new values in the same input buffers and parameter rows")


def test_two_graphs_share_the_splitk_workspace():
    ws = _shared_ws()
    a, b = Composite(910, ws), Composite(920, ws)
    Da, Db = a.direct(), b.direct()
    assert not torch.equal(Da, Db)
    pa, pb = a.record(), b.record()
    pa.instantiate(), pb.instantiate()
    for rnd_ in range(2):
        a.poison(), b.poison()
        pa.launch(), pb.launch(), pa.launch(), pb.launch()           # alternately, on one stream
        torch.cuda.synchronize()
        assert torch.equal(a.chk.bits, Da) and torch.equal(b.chk.bits, Db), f"round {rnd_}: a graph lost its result to the other"


# ====================================================================== life cycle and misuse ==
def _fill_target():
    return guarded(1, 1000, 1000, F32, DEV, back_rows=1)


def _fill(t, v, s=None):
    lib().api.lb_fill_f32(t.data_ptr(), t.numel(), v, s if s is not None else stream())


def test_rerecording_an_instantiated_program_drops_its_graph():
    (a, _), (b, _), (c, chk_c) = _fill_target(), _fill_target(), _fill_target()
    prog = Program()
    with prog.record():
        _fill(a, 1.0), _fill(b, 2.0)
    prog.instantiate()
    prog.launch()
    torch.cuda.synchronize()
    assert bool((a == 1.0).all()) and bool((b == 2.0).all())
    with prog.record():
        _fill(c, 3.0)
    assert prog.num_ops == 3 and not prog.graph_ready
    prog.launch()                       # no graph any more: all three ops, eagerly
    torch.cuda.synchronize()
    chk_c.assert_fully_written("third op after re-recording")
    assert bool((c == 3.0).all()), "launch() replayed the stale two-op graph"
    prog.instantiate()
    c.fill_(0.0)
    prog.launch()
    torch.cuda.synchronize()
    assert bool((c == 3.0).all())


def test_destroying_the_recording_program_ends_the_recording():
    api = lib().api
    t, chk = _fill_target()
    h = api.lb_program_create()
    api.lb_program_begin_record(h)
    assert api.lb_program_recording() == 1
    api.lb_program_destroy(h)
    assert api.lb_program_recording() == 0
    _fill(t, 4.0)                       # executes directly (before the fix: pushed into freed memory)
    torch.cuda.synchronize()
    assert bool((t == 4.0).all())
    chk.assert_intact("fill after destroy")


def test_bad_calls_raise_and_change_nothing():
    api = lib().api
    t, chk = _fill_target()
    p, q = Program("p"), Program("q")
    with pytest.raises(RuntimeError, match="empty program"):
        p.instantiate()
    assert p.num_ops == 0
    api.lb_program_begin_record(p.handle)
    try:
        with pytest.raises(RuntimeError, match="not recording this program"):
            api.lb_program_end_record(q.handle)
        with pytest.raises(RuntimeError, match="already recording"):
            api.lb_program_begin_record(q.handle)
        with pytest.raises(RuntimeError, match="already recording"):
            api.lb_program_begin_record(p.handle)
        assert api.lb_program_recording() == 1
        _fill(t, 5.0)                   # still recorded into p
    finally:
        api.lb_program_end_record(p.handle)
    torch.cuda.synchronize()
    chk.assert_untouched("fill recorded into p")
    assert p.num_ops == 1 and q.num_ops == 0 and api.lb_program_recording() == 0


def test_exception_inside_record_leaves_the_thread_not_recording():
    t, chk = _fill_target()
    prog = Program()
    with pytest.raises(ZeroDivisionError):
        with prog.record():
            1 / 0
    assert lib().api.lb_program_recording() == 0
    _fill(t, 6.0)
    torch.cuda.synchronize()
    assert bool((t == 6.0).all()) and prog.num_ops == 0


def test_recording_is_per_thread():
    """Thread A holds a recording open; thread B launches the same kernel directly on its own stream: B's output is written, A's
    program holds only A's ops."""
    api = lib().api
    (ta, chk_a), (tb, chk_b) = _fill_target(), _fill_target()
    a_recording, b_done, res = threading.Event(), threading.Event(), {}
    prog = Program("thread A")

    def thread_a():
        try:
            with prog.record():
                _fill(ta, 7.0)
                a_recording.set()
                assert b_done.wait(30)
                _fill(ta, 7.5)
            res["a"] = "ok"
        except BaseException as e:      # noqa: BLE001
            res["a"] = repr(e)
            a_recording.set()

    def thread_b():
        try:
            assert a_recording.wait(30)
            res["b_recording"] = api.lb_program_recording()
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                _fill(tb, 8.0, s.cuda_stream)
            s.synchronize()
            res["b"] = "ok"
        except BaseException as e:      # noqa: BLE001
            res["b"] = repr(e)
        finally:
            b_done.set()
    A, B = threading.Thread(target=thread_a), threading.Thread(target=thread_b)
    A.start(), B.start()
    A.join(60), B.join(60)
    torch.cuda.synchronize()
    assert res == {"a": "ok", "b": "ok", "b_recording": 0}, res
    assert bool((tb == 8.0).all()), "thread B's direct launch was swallowed by thread A's recording"
    chk_a.assert_untouched("thread A's recorded fills")
    assert prog.op_names() == ["lb_fill_f32", "lb_fill_f32"]


def test_wrappers_that_allocate_refuse_while_recording():
    """On the device as on the CPU tier: no op is added and nothing runs."""
    o = ops()
    x, g = torch.zeros(1, 64, 64, dtype=F16, device=DEV), torch.ones(64, dtype=F32, device=DEV)
    prog = Program()
    with prog.record():
        with pytest.raises(RuntimeError, match="while a program is recording"):
            o.groupnorm_nhwc(x, g, g, 32, 1e-5, False)
    assert prog.num_ops == 0


# ====================================================================== graph before any eager run
def test_graph_instantiated_before_any_eager_run():
    """What a caller gets from ``Program.instantiate()`` straight after ``record()``, in a process that has launched none of the
    kernels before: the first replay of every kernel family that asks for its dynamic-LDS limit on first use (halo conv and upconv,
    the direct-to-LDS GEMM tiles 4 / 9 / 10, the ping-pong and the 5-stage attention) happens inside the stream capture."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_graph_first_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and "VERDICT equal" in r.stdout, f"exit {r.returncode}: {r.stdout[-1500:]} {r.stderr[-1500:]}"
