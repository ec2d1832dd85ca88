"""``lb_counter_noise_f16`` on the device (csrc/noise.hip; contract: include/lb_hip.h) and counter-based noise through the
native loops.  The reference is tests/_counter_noise_ref.py - an independent restatement in Python integers and float64 - never
native/noise.py.  Words must match exactly; values must equal ``fp16(float64 restatement)``, with the one allowance the float64
evaluation leaves (device and host libm each within an ulp of float64: a value that close to an fp16 rounding boundary): at most
1 element in 10^5 may differ, and then only to the neighbouring fp16 value.  The observed count (expected 0) is written to the file
the environment variable LB_COUNTER_NOISE_RECORD names (profiles/counter_noise.txt holds such a record), else printed."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from oracle import sdxl_ref as R  # noqa: E402  (tiny configs only)
import _counter_noise_ref as REF  # noqa: E402
from _guard import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16 = torch.float16
_RECORD = []


def ops_mod():
    from latentblending_amd.hip import ops
    return ops


def api():
    from latentblending_amd.hip import lib
    return lib.api


def stream():
    return torch.cuda.current_stream().cuda_stream


def rows_for(n):
    """n rows: the all-zero row and the all-ones row first, then (trajectory id, step) rows as the engine builds them."""
    rows = [(0, 0, 0, 0, 0), (REF.MASK32,) * 5]
    rows += [REF.row_of(REF.fold(REF.TAG_ANCHOR, 420 + k), k % 4) for k in range(n)]
    return rows[:n] if n > 1 else rows[1:2]


@pytest.fixture(scope="module", autouse=True)
def record_file():
    yield
    path = os.environ.get("LB_COUNTER_NOISE_RECORD")
    if _RECORD and path:
        with open(path, "w") as fh:
            fh.write("\n".join(_RECORD) + "\n")


# ================================================================== words and values
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("per_sample", [8, 64, 2880])
def test_raw_words_are_the_restatements(per_sample, n):
    rows = rows_for(n)
    got = ops_mod().counter_noise(rows, (n, per_sample), raw=True, device=DEV)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, per_sample)
    want = REF.words(rows, per_sample)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    if per_sample == 8:             # ... and the restatement's vectorised form is its scalar definition
        assert [int(v) for v in want[-1]] == REF.words_scalar(rows[-1], per_sample)


@pytest.mark.parametrize("per_sample", [8, 64, 2880, 16384])
def test_values_equal_fp16_of_the_float64_restatement(per_sample):
    n = 5
    rows = rows_for(n)
    got = ops_mod().counter_noise(rows, (n, per_sample), device=DEV)
    assert got.dtype == F16 and tuple(got.shape) == (n, per_sample)
    g = got.cpu().numpy()
    want = REF.normals_f16(rows, per_sample)
    assert np.isfinite(g).all() and np.abs(g.astype(np.float64)).max() <= 5.89
    gb, wb = g.view(np.uint16).astype(np.int32), want.view(np.uint16).astype(np.int32)
    differ = gb != wb
    count = int(differ.sum())
    line = f"values n={n} per_sample={per_sample}: {count} of {g.size} elements differ from fp16(float64 restatement)"
    print("[counter-noise] " + line)
    _RECORD.append(line)
    # the cap (a condition, not a measurement): <= 1 in 10^5, and a differing element is the neighbouring fp16 value
    assert count <= g.size // 100000, line
    if count:
        same_sign = (gb[differ] >> 15) == (wb[differ] >> 15)
        assert same_sign.all() and np.abs(gb[differ] - wb[differ]).max() == 1


# ================================================================== position independence
def test_a_row_gives_the_same_bytes_wherever_it_is_served():
    """Device against device, bit for bit: alone; as row 0 and as row 16 of 17; into a buffer at a 16-byte offset; on a second
    stream; with raw words likewise."""
    ops = ops_mod()
    per = 2880
    row = REF.row_of(REF.fold(REF.TAG_MID, 420, 421, REF.f64_bits(0.375), 2), 3)
    others = rows_for(16)
    for raw in (False, True):
        alone = ops.counter_noise([row], (1, per), raw=raw, device=DEV)[0]
        first = ops.counter_noise([row] + others, (17, per), raw=raw, device=DEV)
        last = ops.counter_noise(others + [row], (17, per), raw=raw, device=DEV)
        assert torch.equal(first[0], alone) and torch.equal(last[16], alone)
        assert torch.equal(first[1:], last[:16])
        width = 4 if raw else 2
        buf = torch.zeros(per + 16 // width, dtype=alone.dtype, device=DEV)
        off = buf[16 // width:]
        assert off.data_ptr() % 16 == 0 and off.data_ptr() == buf.data_ptr() + 16
        ops.counter_noise([row], (1, per), raw=raw, out=off.view(1, per))
        assert torch.equal(off, alone) and int(buf[:16 // width].abs().sum()) == 0
        s2 = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s2):
            second = ops.counter_noise(others[:3] + [row], (4, per), raw=raw, device=DEV)
        s2.synchronize()
        assert torch.equal(second[3], alone)


def test_recorded_replayed_in_halves_and_graph_launched():
    """The whole replay protocol of tests/_replay.py, used as a library (the case never enters its registry): two direct launches,
    a recording that launches nothing and reports the op under its own name, eager replay, the run_range halves, hipGraph on two
    streams, time_ops - and new rows in the same device buffer.  The header's contract: ``rows_dev`` is read when the kernel
    runs, the caller keeps it alive, and rewriting it between replays draws other noise.  The values each mode reproduces are
    the direct launch's, which the tests above hold to the restatement."""
    import _replay as RP
    ops = ops_mod()
    n, per = 3, 296
    c = RP.Case("counter_noise", ["lb_counter_noise_f16"] * 2)
    rows_host = rows_for(5)[2:]
    rows = c.inp(ops.noise_rows(rows_host, DEV))
    out = c.guarded("values", n, per, per, F16, back_rows=2)
    words = c.plain_out("words", (n, per), torch.int32)

    def thunk():
        api().lb_counter_noise_f16(rows.data_ptr(), out.data_ptr(), per, n, 0, stream())
        api().lb_counter_noise_f16(rows.data_ptr(), words.data_ptr(), per, n, 1, stream())
    c.thunk = thunk
    other = [REF.row_of(REF.fold(REF.TAG_ANCHOR, 7 + k), 1) for k in range(n)]
    c.mutate = lambda: rows.copy_(ops.noise_rows(other, DEV))
    c.freeze()
    rec = RP.run_protocol(c, RP.GpuDriver())
    print("[counter-noise] " + RP.format_record(rec))
    assert rec["eager"] == rec["graph"] == rec["graph_s2"] == rec["new_values"] == "equal" and rec["ranges"] == "equal(1)"
    c.restore()
    c.thunk()
    torch.cuda.synchronize()
    assert np.array_equal(words.cpu().numpy().view(np.uint32), REF.words(other, per))
    assert np.array_equal(out.contiguous().cpu().numpy().view(np.uint16), REF.normals_f16(other, per).view(np.uint16))
    # the wrapper holds a recording caller to that contract: host rows would be uploaded into a buffer that dies with the call
    from latentblending_amd.native.runtime import Program
    prog = Program("refuse")
    with prog.record():
        with pytest.raises(RuntimeError, match="while a program is recording"):
            ops.counter_noise(rows_host, (n, per), out=out.contiguous())
        ops.counter_noise(rows, (n, per), out=torch.empty(n, per, dtype=F16, device=DEV))        # caller-owned device rows: fine
    assert prog.op_names() == ["lb_counter_noise_f16"]


# ================================================================== memory contract, refusals
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("n,per_sample", [(1, 8), (5, 8), (3, 296), (2, 2880)])
def test_memory_contract(n, per_sample, raw):
    """Guard bands in front of and behind ``out`` stay untouched, every element is written (the last row's tail too, at
    per_sample = 8: one 16-byte store per row), and ``rows_dev`` - with poisoned rows behind the last one - is unchanged."""
    ops = ops_mod()
    rows = rows_for(n)
    padded = torch.full((n + 64, 8), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    padded[:n] = ops.noise_rows(rows, DEV)
    before = padded.clone()
    if raw:
        view, chk = guarded(n, per_sample, per_sample, torch.float32, DEV, back_rows=4)
        api().lb_counter_noise_f16(padded.data_ptr(), view.data_ptr(), per_sample, n, 1, stream())
        torch.cuda.synchronize()
        chk.assert_intact("raw words")
        got = chk.bits[chk.front:chk.front + n * per_sample].view(n, per_sample).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, REF.words(rows, per_sample))                 # (complete: every word is the restatement's)
    else:
        view, chk = guarded(n, per_sample, per_sample, F16, DEV, back_rows=4)
        api().lb_counter_noise_f16(padded.data_ptr(), view.data_ptr(), per_sample, n, 0, stream())
        torch.cuda.synchronize()
        chk.assert_intact("values")
        chk.assert_fully_written("values")
    assert torch.equal(padded, before)


def test_refusals_raise_and_leave_out_untouched():
    ops = ops_mod()
    rows = ops.noise_rows(rows_for(2), DEV)
    view, chk = guarded(2, 64, 64, F16, DEV, back_rows=4)
    R_, O_ = rows.data_ptr(), view.data_ptr()
    assert R_ % 16 == 0 and O_ % 16 == 0
    bad = {"n = 0": (R_, O_, 64, 0, 0), "n < 0": (R_, O_, 64, -2, 0), "per_sample = 0": (R_, O_, 0, 2, 0),
           "per_sample % 8": (R_, O_, 60, 2, 0), "per_sample % 8 (raw)": (R_, O_, 4, 2, 1), "null rows": (None, O_, 64, 2, 0),
           "null out": (R_, None, 64, 2, 0), "misaligned rows": (R_ + 4, O_, 64, 2, 0), "misaligned out": (R_, O_ + 2, 64, 2, 0),
           "misaligned out by 8": (R_, O_ + 8, 56, 2, 0)}
    for name, args in bad.items():
        with pytest.raises(RuntimeError, match=r"lb_counter_noise_f16: \w"):
            api().lb_counter_noise_f16(*args, stream())
        torch.cuda.synchronize()
        chk.assert_untouched(name)
    with pytest.raises(ValueError):
        ops.counter_noise(rows_for(2), (3, 64), device=DEV)
    with pytest.raises(ValueError):
        ops.counter_noise(rows_for(2), (2, 64), out=torch.empty(2, 64, dtype=torch.float32, device=DEV))
    chk.assert_untouched("wrapper refusals")


# ================================================================== through the pipe
STEPS, INJ = 4, 2


def tiny_pipe(noise):
    import latentblending_amd.native as n
    return n.NativeSDXLPipe(turbo=True, unet_cfg=n.UNetConfig(**dataclasses.asdict(R.tiny_unet_cfg())),
                            vae_cfg=n.VAEConfig(**dataclasses.asdict(R.tiny_vae_cfg())), seed=0, allow_synthetic=True, noise=noise)


def engine(pipe, frontier):
    from latentblending_amd import BlendingEngine
    np.random.seed(0)
    be = BlendingEngine(pipe, verbose=False, do_compile=True, frontier_width=frontier)
    be.set_dimensions((128, 128))
    be.set_branching(nmb_max_branches=5)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    return be


class StepSpy:
    """Wraps ``scheduler.device_step``: the noise tensor of every call, in call order."""

    def __init__(self, sched):
        self.sched, self.inner, self.calls = sched, sched.device_step, []

    def __enter__(self):
        def spy(x, eps, params, noise=None, cfg=False, **kw):
            self.calls.append(None if noise is None else noise.detach().clone())
            return self.inner(x, eps, params, noise=noise, cfg=cfg, **kw)
        self.sched.device_step = spy
        return self

    def __exit__(self, *exc):
        del self.sched.device_step

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def test_the_native_loops_hand_device_step_the_same_noise():
    """Sample by sample and step by step the noise ``device_step`` receives is the same bytes - and the restatement's - whether
    a branch runs alone (G = 1), in a batch of 3 in permuted order, or in the fused wavefront, with and without a known anchor.
    The NOISE is compared, not the latents: the GEMM tile policy depends on the batch, so latents are not bit-stable across
    batch sizes."""
    from latentblending_amd.native import noise as N
    p = tiny_pipe("counter")
    assert p.noise == "counter" and isinstance(p.scheduler.noise_source, N.CounterNoise)
    be = engine(p, 8)
    assert be.num_inference_steps == STEPS
    emb = [be.dh.get_text_embedding(t) for t in ("photo of a reef", "rendering of an alien planet")]
    starts = {s: be.get_noise(s) for s in (420, 421, 1, 2, 3)}
    a_ids = [N.anchor_id(420), N.anchor_id(421)]
    fr = [0.25, 0.5, 0.75]
    m_ids = [N.mid_id(420, 421, f, INJ) for f in fr]
    zeros = [0.0] * STEPS
    shape = tuple(starts[420].shape)
    per = int(np.prod(shape[1:]))

    def want(tid, step):
        return REF.normals_f16([REF.row_of(tid, step)], per).view(np.uint16).reshape(shape[1:])

    def as_bits(t):
        return t.cpu().numpy().view(np.uint16)
    with StepSpy(p.scheduler) as spy:
        # G = 1 per branch
        alone = {}
        for tid, seed, idx in [(a_ids[0], 420, 0), (a_ids[1], 421, 0)] + [(m, s, INJ) for m, s in zip(m_ids, (1, 2, 3))]:
            p.native_run_diffusion_batch([emb[0]], [starts[seed]], idx, [None], [zeros], STEPS, [0.0], noise_ids=[tid])
            calls = spy.take()
            assert len(calls) == STEPS - idx and all(c is not None and tuple(c.shape) == shape for c in calls)
            for k, c in enumerate(calls):
                alone[(tid, idx + k)] = as_bits(c[0])
                assert np.array_equal(alone[(tid, idx + k)], want(tid, idx + k))
        assert len(alone) == 2 * STEPS + 3 * (STEPS - INJ)
        # the generic single-branch entry under a bound id (what the engine's sequential path does)
        p.scheduler.noise_source.bind(m_ids[1])
        p.native_run_diffusion(emb[0], starts[2], INJ, None, zeros, STEPS, 0.0)
        p.scheduler.noise_source.bind(None)
        for k, c in enumerate(spy.take()):
            assert np.array_equal(as_bits(c[0]), alone[(m_ids[1], INJ + k)])
        # the generic loop: scheduler.step() draws under the bound id at the scheduler's own step index
        sched, src, drawn = p.scheduler, p.scheduler.noise_source, []
        inner_draw = sched.draw_noise
        sched.draw_noise = lambda shp, device: (drawn.append(inner_draw(shp, device)), drawn[-1])[1]
        try:
            sched.set_timesteps(STEPS)
            src.bind(a_ids[1])
            x = starts[421].to(DEV, F16).contiguous()
            for t in sched.timesteps:
                x = sched.step(torch.zeros_like(x), t, x)[0]
        finally:
            del sched.draw_noise
            src.bind(None)
            sched.set_timesteps(STEPS)
        assert len(drawn) == STEPS and not spy.take()
        for i, z in enumerate(drawn):
            assert np.array_equal(as_bits(z[0]), alone[(a_ids[1], i)])
        # G = 3, permuted
        perm = [2, 0, 1]
        p.native_run_diffusion_batch([emb[0]] * 3, [starts[1 + g] for g in perm], INJ, [None] * 3, [zeros] * 3, STEPS, [0.0] * 3,
                                     noise_ids=[m_ids[g] for g in perm])
        calls = spy.take()
        assert len(calls) == STEPS - INJ
        for k, c in enumerate(calls):
            assert tuple(c.shape) == (3,) + shape[1:]
            for slot, g in enumerate(perm):
                assert np.array_equal(as_bits(c[slot]), alone[(m_ids[g], INJ + k)])
        # counter-based loops refuse to guess an identity
        with pytest.raises(ValueError, match="noise_ids"):
            p.native_run_diffusion_batch([emb[0]] * 2, [starts[1], starts[2]], INJ, [None] * 2, [zeros] * 2, STEPS, [0.0] * 2)
        spy.take()

        # the fused wavefront: both anchors from step 0, the mids join at INJ
        def wavefront(known, elide=False):
            coeffs = [[0.0, 0.0, 0.0, 1.0]] * 3 if elide else [zeros] * 3
            out = p.native_run_wavefront([emb[0], emb[1]], [starts[420], starts[421]], [emb[0]] * 3, fr, coeffs, INJ, STEPS, 0.0,
                                         [0.0] * 3, known_anchors=known, noise_ids=(a_ids, m_ids), elide_dead_steps=elide)
            return out, spy.take()
        (t1, t2, _), calls = wavefront((None, None))
        assert len(calls) == STEPS
        for i, c in enumerate(calls):
            ids = a_ids + (m_ids if i >= INJ else [])
            assert c.shape[0] == len(ids)
            for slot, tid in enumerate(ids):
                assert np.array_equal(as_bits(c[slot]), alone[(tid, i)])
        _, calls = wavefront((t1, None))                           # anchor 1 known: only anchor 2 and the mids draw
        assert len(calls) == STEPS
        for i, c in enumerate(calls):
            ids = a_ids[1:] + (m_ids if i >= INJ else [])
            assert c.shape[0] == len(ids)
            for slot, tid in enumerate(ids):
                assert np.array_equal(as_bits(c[slot]), alone[(tid, i)])
        _, calls = wavefront((t1, t2))                             # both known: the mids alone, from INJ
        assert len(calls) == STEPS - INJ
        for k, c in enumerate(calls):
            assert all(np.array_equal(as_bits(c[g]), alone[(m_ids[g], INJ + k)]) for g in range(3))
        # a dead step (the next step's crossfeed coefficient is exactly 1) runs the anchors only: the mids' row of that step is
        # not even asked for, and every other row is what it was
        asked = []
        keyed = p.scheduler.noise_source.keyed
        p.scheduler.noise_source.keyed = lambda pairs, shp: (asked.extend(pairs), keyed(pairs, shp))[1]
        try:
            _, calls = wavefront((None, None), elide=True)
        finally:
            del p.scheduler.noise_source.keyed
        assert sorted(asked) == sorted([(t, i) for t in a_ids for i in range(STEPS)] + [(t, STEPS - 1) for t in m_ids])
        assert [c.shape[0] for c in calls] == [2, 2, 2, 5]
        for slot, tid in enumerate(a_ids + m_ids):
            assert np.array_equal(as_bits(calls[-1][slot]), alone[(tid, STEPS - 1)])


def frames_u8(frames):
    return np.stack([np.asarray(f) for f in frames])


def test_counter_transition_is_reproducible_and_close_across_frontier_widths():
    """One full ``run_transition`` under noise="counter": the same bits when run twice; at frontier width 1 against 8 the same tree
    and frames within the tolerance the cross-path GPU tests use for a whole transition (mean |du8| <= 2, 99 % within 4) - the
    noise is identical, the latents are not bit-stable across batch sizes."""
    p = tiny_pipe("counter")
    runs = {}
    for key, width in (("w8", 8), ("w8 again", 8), ("w1", 1)):
        be = engine(p, width)
        runs[key] = (frames_u8(be.run_transition(fixed_seeds=[420, 421])), list(be.tree_fracts))
    assert len(runs["w8"][0]) == len(runs["w8"][1]) >= 5
    assert np.array_equal(runs["w8"][0], runs["w8 again"][0]) and runs["w8"][1] == runs["w8 again"][1]
    assert runs["w1"][1] == runs["w8"][1]
    d = np.abs(runs["w1"][0].astype(np.int32) - runs["w8"][0].astype(np.int32))
    line = f"transition frontier 1 vs 8 under counter noise: mean|du8|={d.mean():.3f} within4={(d <= 4).mean():.4f}"
    print("[counter-noise] " + line)
    _RECORD.append(line)
    assert d.mean() <= 2 and (d <= 4).mean() >= 0.99


def test_stream_is_the_default_and_unchanged():
    """noise="stream": no source is installed, the wavefront serves a round with ONE ``draw_noise_many`` call of 2 x steps +
    G x (steps - injection) latents - the parent commit's sequence - and a Turbo transition is bit-identical to itself."""
    p = tiny_pipe("stream")
    assert p.noise == "stream" and p.scheduler.noise_source is None
    inner, calls = p.scheduler.draw_noise_many, []

    def spy(n, shape, device):
        calls.append((int(n), tuple(shape)))
        return inner(n, shape, device)
    p.scheduler.draw_noise_many = spy
    out = []
    for _ in range(2):
        be = engine(p, 8)
        calls.clear()
        torch.manual_seed(1234)
        out.append(frames_u8(be.run_transition(fixed_seeds=[420, 421])))
        assert p.scheduler.noise_source is None
        assert [int(v) for v in be.list_idx_injection] == [INJ] and be.num_inference_steps == STEPS
        stems, dropped = int(be.list_nmb_stems[0]), be.stats.get("speculation_dropped", 0)
        assert stems >= 3 and len(out[-1]) == stems + 2
        assert calls[0] == (2 * STEPS + min(stems, 8) * (STEPS - INJ), (1, 4, 16, 16))
        assert all(s == (1, 4, 16, 16) and n % (STEPS - INJ) == 0 for n, s in calls[1:])
        assert sum(n for n, _ in calls) == 2 * STEPS + (stems + dropped) * (STEPS - INJ)
    assert np.array_equal(out[0], out[1])
    with pytest.raises(ValueError, match="noise must be one of"):
        p.noise = "philox"
    p.noise = "counter"
    assert type(p.scheduler.noise_source).__name__ == "CounterNoise"
    p.noise = "stream"
    assert p.scheduler.noise_source is None
