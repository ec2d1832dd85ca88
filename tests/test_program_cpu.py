"""The program layer without a GPU.  A recording never launches, so with the built library and fake, suitably aligned pointers the
host half of csrc/program.hip and of every launcher runs here: registry completeness, op names and routing, refusals at record
time, the life cycle, thread-local recording, the ops.py wrappers that must not hand a temporary buffer to a closure - and a
self-test of the replay protocol itself on fake cases (test_program_replay_gpu.py is the device half)."""
import contextlib
import ctypes as C
import threading

import pytest
import torch

import _replay as RP
from latentblending_amd.hip import lib, ops

api = lib.api
P = [0x100000 * (k + 1) for k in range(16)]         # fake device pointers, 1 MiB apart, 16-byte aligned: never dereferenced


@contextlib.contextmanager
def recording():
    h = api.lb_program_create()
    api.lb_program_begin_record(h)
    try:
        yield h
    finally:
        if api.lb_program_recording():
            api.lb_program_end_record(h)
        api.lb_program_destroy(h)


def names(h):
    return [api.lb_program_op_name(h, i).decode() for i in range(api.lb_program_num_ops(h))]


# ---------------------------------------------------------------- registry completeness
def test_every_stream_launcher_has_a_replay_case():
    """A new launcher in lib.SIGNATURES without a case in tests/_replay.py fails here, and so does a role that the signature's
    shape contradicts."""
    launchers = RP.table_launchers()
    missing = sorted(launchers - RP.registered_launchers())
    assert not missing, f"launchers without a replay case: {missing}"
    assert not RP.registered_launchers() - launchers, sorted(RP.registered_launchers() - launchers)
    # a role is what the signature says: outside the program API, "int status, stream last" is a launcher and nothing else is
    for n, (res, args, role) in lib.SIGNATURES.items():
        assert role in ("launcher", "status", "value"), (n, role)
        if not RP.is_program_api(n):
            assert (role == "launcher") == (res is C.c_int and bool(args) and args[-1] is C.c_void_p), (n, role)
    assert not any(RP.is_program_api(n) for n in launchers)
    assert len(RP.case_ids()) == len(set(RP.case_ids()))
    for n in RP.KNOBS:
        assert lib.SIGNATURES[n][2] == "value" and lib.SIGNATURES[n][0] is None, n


# ---------------------------------------------------------------- fake calls of every launcher
def conv_params(B=1, H=16, W=32, Cin=64, N=128, ks=3, flags=0, scatter=0, ldc=None):
    g = lib.ConvGeom.conv3x3(H, W, Cin) if ks == 3 else lib.ConvGeom(H, W, Cin, ks, ks, parity="all" if scatter == 2 else None)
    return lib.gemm_params(A=P[0], W=P[1], C=P[2], zero_page=P[3], M=g.M(B), N=N, K=g.K, ldw=g.K, ldc=N if ldc is None else ldc, conv=g,
                           flags=flags)


def gemm_params(M=64, N=64, K=64, flags=0):
    return lib.gemm_params(A=P[0], W=P[1], C=P[2], zero_page=P[3], M=M, N=N, K=K, lda=K, ldw=K, ldc=N, flags=flags)


def attn_params(D=64, causal=0, Sq=128, Skv=128):
    p = lib.LbAttnParams()
    p.Q, p.K, p.V, p.O, p.zero_page = P[0], P[1], P[2], P[3], P[4]
    p.B, p.H, p.Sq, p.Skv, p.Skv_valid = 1, 1, Sq, Skv, Skv
    p.ldq = p.ldk = p.ldv = p.ldo = D
    p.scale, p.causal = D ** -0.5, causal
    return p


def ptrs(n, base):
    arr = (C.c_void_p * n)(*[base + 4096 * i for i in range(n)])
    return C.cast(arr, lib.c_void_pp), arr


def slerp_pairs(fn):
    def call():
        (a, ka), (b, kb), (o, ko) = ptrs(17, P[0]), ptrs(17, P[1]), ptrs(17, P[2])
        fn(a, b, o, (C.c_double * 17)(*[0.5] * 17), 17, 64, None)
    return call


def lpips_tap():
    (a, ka), (b, kb) = ptrs(16, P[0]), ptrs(16, P[1])
    api.lb_lpips_tap(a, b, P[2], P[3], P[4], 16, 64, 64, None)


FAKE_CALLS = {
    "lb_slerp_pairs_f16": slerp_pairs(api.lb_slerp_pairs_f16),
    "lb_slerp_pairs_f32": slerp_pairs(api.lb_slerp_pairs_f32),
    "lb_slerp_pairs_f64": slerp_pairs(api.lb_slerp_pairs_f64),
    "lb_slerp_batched_f16": lambda: api.lb_slerp_batched_f16(P[0], P[1], P[2], P[3], 2, 64, None),
    "lb_slerp_strided_f16": lambda: api.lb_slerp_strided_f16(P[0], 0, P[1], 64, P[2], P[3], 2, 64, None),
    "lb_lerp_f16": lambda: api.lb_lerp_f16(P[0], P[1], P[2], 64, 0.25, None),
    "lb_lerp_f32": lambda: api.lb_lerp_f32(P[0], P[1], P[2], 64, 0.25, None),
    "lb_scale_model_input_f16": lambda: api.lb_scale_model_input_f16(P[0], P[1], P[2], 64, 2, 0, None),
    "lb_euler_step_f16": lambda: api.lb_euler_step_f16(P[0], P[1], None, P[2], P[3], 64, 2, 0, 0, None),
    "lb_ddim_step_f16": lambda: api.lb_ddim_step_f16(P[0], P[1], P[2], P[3], 64, 2, 0, None),
    "lb_lcm_step_f16": lambda: api.lb_lcm_step_f16(P[0], P[1], None, P[2], P[3], 64, 2, 0, 1, None),
    "lb_dpmpp2m_step_f16": lambda: api.lb_dpmpp2m_step_f16(P[0], P[1], P[2], P[3], 64, 2, 1, None),
    "lb_counter_noise_f16": lambda: api.lb_counter_noise_f16(P[0], P[1], 64, 2, 0, None),
    "lb_gemm_f16": lambda: api.lb_gemm_f16(C.byref(gemm_params()), None),
    "lb_conv3x3_halo_f16": lambda: api.lb_conv3x3_halo_f16(C.byref(conv_params()), None),
    "lb_conv3x3_narrow_f16": lambda: api.lb_conv3x3_narrow_f16(C.byref(conv_params(N=8)), None),
    "lb_upconv2x_halo_f16": lambda: api.lb_upconv2x_halo_f16(C.byref(conv_params(ks=2, scatter=2)), None),
    "lb_groupnorm_nhwc": lambda: api.lb_groupnorm_nhwc(P[0], P[1], P[2], P[3], P[4], 1, 64, 64, 64, 64, 32, 1e-5, 0, 0, None),
    "lb_groupnorm_from_stats": lambda: api.lb_groupnorm_from_stats(P[0], P[1], P[2], P[3], P[4], P[5], 1, 64, 64, 64, 64, 32, 1e-5, 0, 0,
                                                                   4, None),
    "lb_groupnorm_affine_from_stats": lambda: api.lb_groupnorm_affine_from_stats(P[0], P[1], P[2], P[3], 2, 64, 64, 32, 1e-5, 4, None),
    "lb_layernorm_f16": lambda: api.lb_layernorm_f16(P[0], P[1], P[2], P[3], 4, 64, 64, 64, 1e-5, None),
    "lb_attn_fwd_d64": lambda: api.lb_attn_fwd_d64(C.byref(attn_params()), None),
    "lb_attn_fwd_d512": lambda: api.lb_attn_fwd_d512(C.byref(attn_params(D=512)), None),
    "lb_softmax_rows_f16": lambda: api.lb_softmax_rows_f16(P[0], 4, 64, 64, 1.0, None),
    "lb_sinusoid_f16": lambda: api.lb_sinusoid_f16(P[0], 4, 1, 1, 64, P[1], 64, 0, None),
    "lb_copy_cols_f16": lambda: api.lb_copy_cols_f16(P[0], P[1], 4, 64, 64, 64, 0, None),
    "lb_cast_f16_to_f32": lambda: api.lb_cast_f16_to_f32(P[0], P[1], 64, None),
    "lb_cast_f32_to_f16": lambda: api.lb_cast_f32_to_f16(P[0], P[1], 64, 1.0, None),
    "lb_nchw_to_nhwc_f16": lambda: api.lb_nchw_to_nhwc_f16(P[0], P[1], 1, 4, 64, 8, 1.0, None),
    "lb_nhwc_to_nchw_f16": lambda: api.lb_nhwc_to_nchw_f16(P[0], P[1], 1, 4, 64, 8, None),
    "lb_postprocess_u8": lambda: api.lb_postprocess_u8(P[0], P[1], 64, 4, 0, None),
    "lb_lpips_prep_u8": lambda: api.lb_lpips_prep_u8(P[0], P[1], 64, None),
    "lb_maxpool3s2_nhwc_f16": lambda: api.lb_maxpool3s2_nhwc_f16(P[0], P[1], 1, 8, 8, 64, None),
    "lb_lpips_tap": lpips_tap,
    "lb_fill_f32": lambda: api.lb_fill_f32(P[0], 64, 1.0, None),
    "lb_embed_tokens_f16": lambda: api.lb_embed_tokens_f16(P[0], P[1], P[2], P[3], 4, 4, 64, 100, None),
    "lb_frames_lerp_u8": lambda: api.lb_frames_lerp_u8(P[0], P[1], P[2], P[3], 2, 256, None),
    "lb_gather_rows_f16": lambda: api.lb_gather_rows_f16(P[0], P[1], P[2], 4, 64, 64, None),
    "lb_copy_d2d": lambda: api.lb_copy_d2d(P[0], P[1], 64, None),
    "lb_jpeg_dct_quant_u8": lambda: api.lb_jpeg_dct_quant_u8(P[0], P[1], P[2], 1, 16, 16, 0, None),
    "lb_jpeg_entropy": lambda: api.lb_jpeg_entropy(P[0], P[1], P[2], 4096, P[3], 1, 16, 16, 0, None),
    "lb_resample_u8": lambda: api.lb_resample_u8(P[0], P[1], P[2], 1, 8, 8, 12, 12, P[3], P[4], P[5], 4, P[6], P[7], P[8], 4, None),
}
# launchers that make a HIP call when they are CALLED (not when they are replayed) and therefore could not be recorded without a
# device.  lb_gemm_f16 calls lb_gemm_glds_init() (hipFuncSetAttribute) at record time: without a device those calls fail and are
# ignored, the op is recorded all the same - so the list is empty, and test_every_launcher_records_under_its_own_name proves it.
NEEDS_A_DEVICE_TO_RECORD = []


def test_every_launcher_records_under_its_own_name():
    assert set(FAKE_CALLS) == RP.registered_launchers() - set(NEEDS_A_DEVICE_TO_RECORD)
    for name, call in FAKE_CALLS.items():
        with recording() as h:
            call()
            assert names(h) == [name], (name, names(h))
    assert api.lb_program_recording() == 0


def test_routing_is_decided_at_record_time_and_names_the_routed_kernel():
    api.lb_gemm_set_halo(2)
    try:
        with recording() as h:
            api.lb_gemm_f16(C.byref(conv_params()), None)                              # 3x3, Cin 64, W 32: halo
            api.lb_gemm_f16(C.byref(conv_params(N=8)), None)                           # N <= 16: narrow
            api.lb_gemm_f16(C.byref(conv_params(ks=2, scatter=2)), None)               # four parities in one launch: upconv
            p = conv_params()
            p.stride, p.Hout, p.Wout, p.M = 2, 8, 16, 8 * 16                           # stride 2: implicit GEMM
            api.lb_gemm_f16(C.byref(p), None)
            api.lb_gemm_f16(C.byref(gemm_params()), None)
            got = names(h)
        assert got == ["lb_conv3x3_halo_f16", "lb_conv3x3_narrow_f16", "lb_upconv2x_halo_f16", "lb_gemm_f16", "lb_gemm_f16"]
        api.lb_gemm_set_halo(0)                                                        # halo kernels off: the same convs stay GEMMs
        with recording() as h:
            api.lb_gemm_f16(C.byref(conv_params()), None)
            api.lb_gemm_f16(C.byref(conv_params(N=8)), None)
            assert names(h) == ["lb_gemm_f16", "lb_gemm_f16"]
    finally:
        api.lb_gemm_set_halo(1)


# ---------------------------------------------------------------- refusals at record time
def _stats(p, rows, ptr=P[5]):
    p.flags |= lib.GEMM_CH_STATS
    p.ch_stats, p.ch_stats_rows = ptr, rows
    return p


def _too_many_tiles():
    # 2^22 tiles of 256 pixels x 256 channel blocks = 2^30 work items: one more than a launch takes
    return conv_params(B=1024, H=1024, W=1024, N=32768)


def _ln_on_the_register_ring():
    api.lb_gemm_set_variant(0, 0)
    try:
        p = gemm_params(flags=lib.GEMM_LN_A)
        p.ln_colsum = P[6]
        api.lb_gemm_f16(C.byref(p), None)
    finally:
        api.lb_gemm_set_variant(-1, 0)


def _routed(p):
    api.lb_gemm_set_halo(2)
    try:
        api.lb_gemm_f16(C.byref(p), None)
    finally:
        api.lb_gemm_set_halo(1)


def _resample(tmp=P[1], sx=P[3], sy=P[6], n=1, hout=12):
    api.lb_resample_u8(P[0], tmp, P[2], n, 8, 8, hout, 12, sx, P[4], P[5], 4, sy, P[7], P[8], 4, None)


def _softmax_300():
    api.lb_softmax_rows_f16(P[0], 7, 300, 312, 0.3, None)


GOOD_ROWS = 1 * (16 * 32 // 256) * 4            # conv_params(): B * (tiles per sample) * 4 wave rows

# (id, call, message): everything test_kernel_bounds_gpu.py / test_host_cpu.py / test_resample_gpu.py assert a DIRECT call refuses,
# and the checks that used to sit inside the closures (LB_GEMM_CH_STATS, "too many tiles")
REFUSALS = [
    ("halo ch_stats_rows wrong", lambda: api.lb_conv3x3_halo_f16(C.byref(_stats(conv_params(), 3)), None), "ch_stats_rows must be"),
    ("halo ch_stats null", lambda: api.lb_conv3x3_halo_f16(C.byref(_stats(conv_params(), GOOD_ROWS, None)), None), "needs ch_stats"),
    ("routed halo ch_stats_rows wrong", lambda: _routed(_stats(conv_params(), GOOD_ROWS + 4)), "ch_stats_rows must be"),
    ("upconv ch_stats_rows wrong", lambda: api.lb_upconv2x_halo_f16(C.byref(_stats(conv_params(ks=2, scatter=2), 3)), None),
     "halo upconv: LB_GEMM_CH_STATS"),
    ("routed upconv ch_stats_rows wrong", lambda: _routed(_stats(conv_params(ks=2, scatter=2), 3)), "halo upconv: LB_GEMM_CH_STATS"),
    ("halo too many tiles", lambda: api.lb_conv3x3_halo_f16(C.byref(_too_many_tiles()), None), "too many tiles"),
    ("routed halo too many tiles", lambda: _routed(_too_many_tiles()), "too many tiles"),
    ("ch_stats on a plain gemm", lambda: api.lb_gemm_f16(C.byref(_stats(gemm_params(), 4)), None), "halo-tile conv kernels only"),
    ("gemm N % 4", lambda: api.lb_gemm_f16(C.byref(gemm_params(N=6)), None), "multiple of 4"),
    ("gemm LN fold on the register ring", _ln_on_the_register_ring, "LB_GEMM_LN_A"),
    ("narrow conv ldc % 4 (routed)", lambda: _routed(conv_params(N=8, ldc=10)), "ldc must be a multiple of 4"),
    ("narrow conv ldc % 4", lambda: api.lb_conv3x3_narrow_f16(C.byref(conv_params(N=8, ldc=10)), None), "ldc multiple of 4"),
    ("slerp_batched n % 8", lambda: api.lb_slerp_batched_f16(16, 16, 16, 16, 2, 12, None), "n must be a multiple of 8"),
    ("softmax N % 8", _softmax_300, "multiples of 8"),
    ("attention causal Sq != Skv", lambda: api.lb_attn_fwd_d64(C.byref(attn_params(causal=1, Sq=64)), None), "causal"),
    ("attention d512 causal", lambda: api.lb_attn_fwd_d512(C.byref(attn_params(D=512, causal=1)), None), "no causal form"),
    ("groupnorm groups", lambda: api.lb_groupnorm_nhwc(P[0], P[1], P[2], P[3], P[4], 1, 64, 64, 64, 64, 24, 1e-5, 0, 0, None), "groups"),
    ("resample without tmp", lambda: _resample(tmp=None), "tmp"),
    ("resample without horizontal tables", lambda: _resample(sx=None), "horizontal tables"),
    ("resample without vertical tables", lambda: _resample(sy=None), "vertical tables"),
    ("resample n = 0", lambda: _resample(n=0), "positive"),
    ("resample Hout < 0", lambda: _resample(hout=-1), "positive"),
    ("copy_d2d 0 bytes", lambda: api.lb_copy_d2d(P[0], P[1], 0, None), "arguments"),
]
# Audit of the other LB_REQUIREs that sit behind an LB_DISPATCH: groupnorm_impl repeats two checks lb_groupnorm_nhwc has already made;
# the narrow conv's "too many tiles" needs M >= 2^39, which an int M cannot hold; gemm_launch_impl, attn_dispatch, the slerp, jpeg,
# resample and lpips implementations contain none.


@pytest.mark.parametrize("what,call,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_a_recording_refuses_what_a_direct_call_refuses(what, call, message):
    with pytest.raises(RuntimeError, match=message):
        call()                                              # direct: refused before anything is launched (no GPU here)
    with recording() as h:
        FAKE_CALLS["lb_fill_f32"]()
        with pytest.raises(RuntimeError, match=message):
            call()
        assert names(h) == ["lb_fill_f32"], f"{what}: the refused call left an op behind"
        FAKE_CALLS["lb_fill_f32"]()                         # the recording goes on
        assert api.lb_program_num_ops(h) == 2


def test_good_ch_stats_rows_are_accepted_while_recording():
    assert api.lb_gemm_ch_stat_rows(C.byref(conv_params())) == 0          # (default routing: 8 halo blocks are too few)
    with recording() as h:
        api.lb_conv3x3_halo_f16(C.byref(_stats(conv_params(), GOOD_ROWS)), None)
        _routed(_stats(conv_params(), GOOD_ROWS))
        assert names(h) == ["lb_conv3x3_halo_f16"] * 2


# ---------------------------------------------------------------- life cycle
def test_life_cycle_errors_raise_and_change_nothing():
    p, q = api.lb_program_create(), api.lb_program_create()
    try:
        with pytest.raises(RuntimeError, match="empty program"):
            api.lb_program_instantiate(p)
        assert api.lb_program_num_ops(p) == 0 and api.lb_program_recording() == 0
        with pytest.raises(RuntimeError, match="not recording this program"):
            api.lb_program_end_record(p)
        api.lb_program_begin_record(p)
        with pytest.raises(RuntimeError, match="not recording this program"):
            api.lb_program_end_record(q)
        for again in (q, p):
            with pytest.raises(RuntimeError, match="already recording"):
                api.lb_program_begin_record(again)
        assert api.lb_program_recording() == 1
        FAKE_CALLS["lb_fill_f32"]()
        assert (api.lb_program_num_ops(p), api.lb_program_num_ops(q)) == (1, 0)      # still recording p, nothing went to q
        with pytest.raises(RuntimeError, match="arguments"):
            api.lb_program_time_ops(p, None, (C.c_float * 1)())                      # synchronises: never while recording
        api.lb_program_end_record(p)
        assert api.lb_program_recording() == 0
        with pytest.raises(RuntimeError, match="range"):
            api.lb_program_run_range(p, 0, 2, None)
    finally:
        api.lb_program_destroy(p)
        api.lb_program_destroy(q)


def test_destroying_the_recording_program_ends_the_recording():
    p = api.lb_program_create()
    api.lb_program_begin_record(p)
    FAKE_CALLS["lb_fill_f32"]()
    api.lb_program_destroy(p)                    # (before the fix: the next launcher call pushed into the freed program)
    assert api.lb_program_recording() == 0
    with recording() as h:                       # and this thread can record again
        FAKE_CALLS["lb_fill_f32"]()
        assert names(h) == ["lb_fill_f32"]
    q = api.lb_program_create()
    api.lb_program_begin_record(q)
    other = api.lb_program_create()
    api.lb_program_destroy(other)                # destroying ANOTHER program leaves the recording alone
    assert api.lb_program_recording() == 1
    api.lb_program_end_record(q)
    api.lb_program_destroy(q)
    api.lb_program_destroy(None)


def test_exception_inside_record_ends_the_recording():
    from latentblending_amd.native.runtime import Program
    prog = Program()
    with pytest.raises(ZeroDivisionError):
        with prog.record():
            FAKE_CALLS["lb_fill_f32"]()
            1 / 0
    assert api.lb_program_recording() == 0 and prog.num_ops == 1
    with prog.record():                          # recording again appends, and marks the graph as gone
        FAKE_CALLS["lb_cast_f16_to_f32"]()
    assert prog.op_names() == ["lb_fill_f32", "lb_cast_f16_to_f32"] and not prog.graph_ready


def test_recording_is_thread_local():
    res = {}
    with recording() as h:
        def other():
            res["recording"] = api.lb_program_recording()
            q = api.lb_program_create()
            try:
                api.lb_program_begin_record(q)           # a second recording, on another thread, at the same time
                FAKE_CALLS["lb_cast_f16_to_f32"]()
                res["mid"] = api.lb_program_recording()
                api.lb_program_end_record(q)
                res["names"] = names(q)
            except RuntimeError as e:
                res["error"] = str(e)
            finally:
                api.lb_program_destroy(q)
        FAKE_CALLS["lb_fill_f32"]()
        t = threading.Thread(target=other)
        t.start()
        t.join()
        FAKE_CALLS["lb_fill_f32"]()
        assert names(h) == ["lb_fill_f32", "lb_fill_f32"]
    assert res == {"recording": 0, "mid": 1, "names": ["lb_cast_f16_to_f32"]}, res


# ---------------------------------------------------------------- ops.py wrappers
def test_wrappers_refuse_to_record_a_buffer_they_would_free(monkeypatch):
    """Every ops.py wrapper that allocates a device buffer it does not return raises while the calling thread records, unless the
    caller passed that buffer in; with the buffer, the same call records.  (CPU tensors and a null stream: nothing here is ever
    launched.)"""
    monkeypatch.setattr(ops, "stream_ptr", lambda: None)
    F16, F32, F64 = torch.float16, torch.float32, torch.float64
    A, W, out = torch.zeros(64, 64, dtype=F16), torch.zeros(64, 64, dtype=F16), torch.zeros(64, 64, dtype=F16)
    x, y, g = torch.zeros(1, 64, 64, dtype=F16), torch.zeros(1, 64, 64, dtype=F16), torch.ones(64, dtype=F32)
    st = torch.zeros(64, 4, 2, dtype=F32)
    fa, acc = [torch.zeros(64, 64, dtype=F16)], torch.zeros(1, dtype=F32)
    frames, fout = torch.zeros(2, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    ws_gemm = torch.zeros(api.lb_gemm_workspace_bytes(64, 64) // 4, dtype=F32)
    ws_gn = torch.zeros(api.lb_groupnorm_workspace_bytes(1, 32) // 8, dtype=F64)
    tables = (torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=F64))
    calls = [
        ("lb_gemm_f16", lambda **k: ops.gemm(A, W, out=out, **k), dict(workspace=ws_gemm)),
        ("lb_groupnorm_nhwc", lambda **k: ops.groupnorm_nhwc(x, g, g, 32, 1e-5, False, out=y, **k), dict(workspace=ws_gn)),
        ("lb_groupnorm_from_stats", lambda **k: ops.groupnorm_from_stats(x, g, g, 32, 1e-5, False, st, 4, out=y, **k), dict(workspace=ws_gn)),
        ("lb_lpips_tap", lambda **k: ops.lpips_tap(fa, fa, g, acc, **k), dict(workspace=torch.zeros(16 * 128, dtype=F32))),
        ("lb_frames_lerp_u8", lambda **k: ops.frames_lerp_u8(frames, [0], [0.5], out=fout, **k), dict(tables=tables)),
    ]
    for name, call, owned in calls:
        with recording() as h:
            with pytest.raises(RuntimeError, match="while a program is recording"):
                call()
            assert api.lb_program_num_ops(h) == 0, name
            call(**owned)
            assert names(h) == [name]
    # a temporary copy of a non-contiguous / wrongly typed operand is such a buffer too; a usable operand records
    nchw, lat = torch.zeros(1, 4, 8, 8, dtype=F16), torch.zeros(2, 64, dtype=F16)
    copies = [
        ("lb_nchw_to_nhwc_f16", lambda t: ops.nchw_to_nhwc(t, 8), nchw.permute(0, 1, 3, 2), nchw),
        ("lb_euler_step_f16", lambda t: ops.euler_step(lat, lat, g, noise=t, ancestral=True), torch.zeros(64, 2, dtype=F16).t(), lat),
        ("lb_lerp_f16", lambda t: ops.lerp(t, lat, 0.5), torch.zeros(64, 2, dtype=F16).t(), lat),
        ("lb_lerp_f32", lambda t: ops.lerp(t, lat.float(), 0.5), lat, lat.float()),
    ]
    for name, call, needs_copy, usable in copies:
        with recording() as h:
            with pytest.raises(RuntimeError, match="while a program is recording"):
                call(needs_copy)
            assert api.lb_program_num_ops(h) == 0, name
            call(usable)
            assert names(h) == [name]
    with recording() as h:                      # a GEMM that cannot split needs no workspace
        ops.gemm(A, W, out=out, splitk_ws=False)
        assert names(h) == ["lb_gemm_f16"]


# ---------------------------------------------------------------- the protocol can fail
class FakeProgram:
    def __init__(self, drv):
        self.drv, self.ops, self.graph = drv, [], False

    @contextlib.contextmanager
    def record(self):
        self.drv.recording = self
        try:
            yield self
        finally:
            self.drv.recording = None

    num_ops = property(lambda s: len(s.ops))

    def op_names(self):
        return [n for n, _ in self.ops]

    def run_range(self, a, b):
        for _, fn in self.ops[a:b]:
            fn(self.drv.flaw if self.drv.flaw_in in ("eager", "all") else None)

    def run(self):
        self.run_range(0, len(self.ops))

    def instantiate(self):
        self.graph = True

    def launch(self, stream=None):
        assert self.graph
        for _, fn in self.ops:
            fn(self.drv.flaw if self.drv.flaw_in in ("graph", "all") else None)

    def time_ops(self):
        self.run()
        return [0.0] * len(self.ops)


class FakeDriver:
    """Stands in for the GPU: a "launcher" adds 1 to its input; a flawed replay flips the lowest bit of one element."""

    def __init__(self, flaw_in=None, record_writes=False, nondeterministic=False, writes=True):
        self.flaw_in, self.flaw, self.recording = flaw_in, 1, None
        self.record_writes, self.nondeterministic, self.writes, self.calls, self.knobs = record_writes, nondeterministic, writes, 0, []

    def make_case(self):
        c = RP.Case("fake", ["fake_add_one"])
        x, y = torch.arange(64, dtype=torch.int32), torch.full((64,), 0x7FC5A5A5, dtype=torch.int32)
        c.inputs.append([x, None])
        c.outs.append(RP.Out("y", y))

        def kernel(flaw=None):
            if not self.writes:
                return
            y.copy_(x + 1)
            if flaw:
                y[17] ^= flaw

        def thunk():
            self.calls += 1
            if self.recording is not None:
                self.recording.ops.append(("fake_add_one", kernel))
                if self.record_writes:
                    kernel()
                return
            kernel(1 if self.nondeterministic and self.calls == 2 else None)
        c.thunk = thunk
        return c.freeze()

    def sync(self):
        pass

    def set_knobs(self, values):
        self.knobs.append(dict(values))

    def direct(self, case):
        case.thunk()

    def record(self, case):
        prog = FakeProgram(self)
        with prog.record():
            case.thunk()
        return prog

    def launch_on_second_stream(self, prog):
        prog.launch()


def test_protocol_passes_a_faithful_replay_and_moves_every_knob():
    drv = FakeDriver()
    rec = RP.run_protocol(drv.make_case(), drv)
    assert rec["eager"] == rec["graph"] == rec["time_ops"] == "equal" and rec["record"] == "clean"
    at_record, at_replay, at_exit = drv.knobs[0], drv.knobs[1], drv.knobs[-1]
    assert set(at_record) == set(at_replay) == set(RP.KNOBS)
    assert all(at_record[k] != at_replay[k] for k in RP.KNOBS), "a switch kept its record-time value for the replays"
    assert at_exit == {k: d for k, (d, _) in RP.KNOBS.items()}, "the defaults are not restored"
    assert "ops  1" in RP.format_record(rec)


@pytest.mark.parametrize("kwargs,step", [(dict(flaw_in="eager"), "eager"), (dict(flaw_in="graph"), "graph"),
                                         (dict(record_writes=True), "record"), (dict(nondeterministic=True), "direct x2"),
                                         (dict(writes=False), "direct")],
                         ids=["replay_off_by_one_bit", "graph_off_by_one_bit", "recording_writes", "direct_runs_differ", "nothing_written"])
def test_protocol_fails_where_it_must(kwargs, step):
    """In the style of the _guard self-test (test_host_cpu.py): a replay that differs from the direct result by ONE bit, a graph
    that does, a recording that writes the output, two direct launches that differ and an output nobody wrote each fail - at the
    step that is there to catch them - and the defaults are restored on the way out."""
    drv = FakeDriver(**kwargs)
    with pytest.raises(RP.ProtocolFailure, match=r"\] " + step + ":"):
        RP.run_protocol(drv.make_case(), drv)
    assert drv.knobs[-1] == {k: d for k, (d, _) in RP.KNOBS.items()}
