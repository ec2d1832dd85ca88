"""Counter-based sampler noise without a GPU: the stream's definition (Philox4x32-10 known answers, native/noise.py against the
independent restatement of tests/_counter_noise_ref.py bit for bit, moments, range), the trajectory ids, the launcher's refusals
and its recorded name, and path independence of the draws on the CPU oracle pipe: whatever frontier width, speculation prior,
``elide_dead_steps`` setting or farm serves a transition, trajectory ``id`` gets the same bytes at step ``i`` - and nobody asks
for a row it does not use.  (The batched native loops exist on the GPU only: tests/test_counter_noise_gpu.py holds them to the
same map.)"""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch

import _counter_noise_ref as REF
from latentblending_amd.native import noise as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ---------------------------------------------------------------- the stream
def test_philox_known_answers():
    for ctr, key, want in REF.KNOWN_ANSWERS:
        assert REF.philox_scalar(ctr, key) == want
        assert tuple(int(v) for v in N.philox4x32_10(ctr, key)) == want
        row = (key[0], key[1], ctr[1], ctr[2], ctr[3])               # element 4 q + k of a row is word k at counter word 0 = q
        q = ctr[0]
        if q < 8:
            assert tuple(int(v) for v in N.counter_words([row], 32)[0, 4 * q:4 * q + 4]) == want
    assert (N.PHILOX_M0, N.PHILOX_M1, N.PHILOX_W0, N.PHILOX_W1) == (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85)


@pytest.mark.parametrize("per_sample", [8, 64, 2880])
def test_native_restatement_equals_the_test_restatement_bit_for_bit(per_sample):
    rows = REF.mixed_rows()
    w = REF.words(rows, per_sample)
    for j in (0, 1, len(rows) - 1):                                   # (the vectorised twin against the scalar definition)
        assert [int(v) for v in w[j]] == REF.words_scalar(rows[j], per_sample)
    assert np.array_equal(N.counter_words(rows, per_sample), w)
    got, want = N.counter_normal_f16(rows, per_sample), REF.normals_f16(rows, per_sample)
    assert got.dtype == np.float16 and got.shape == (len(rows), per_sample)
    assert np.array_equal(bits(got), bits(want))
    z = REF.normals_from_words(w)
    for j, e in ((0, 0), (1, 2), (len(rows) - 1, per_sample - 2)):    # ... and the transform against ``math``, pair by pair
        a, b = REF.normal_pair_scalar(int(w[j, e]), int(w[j, e + 1]))
        assert abs(z[j, e] - a) <= 1e-15 * max(1.0, abs(a)) and abs(z[j, e + 1] - b) <= 1e-15 * max(1.0, abs(b))


def test_moments_and_range():
    """131 072 values: standard errors are 1 / sqrt(n) = 0.0028 (mean) and sqrt(2 / n) = 0.0039 (variance) - 0.02 is five of them."""
    rows = [REF.row_of(REF.fold(REF.TAG_ANCHOR, 420), s) for s in range(8)]
    for z in (N.counter_normal_f16(rows, 16384).astype(np.float64), REF.normals_f64(rows, 16384)):
        assert z.size == 131072 and np.isfinite(z).all()
        assert abs(z.mean()) < 0.02 and abs(z.var() - 1.0) < 0.02
        assert np.abs(z).max() <= 5.89
    # the extreme words: u1 at both ends, t at both ends - finite, inside the bound, and the bound is reached
    ext = np.array([[0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF]], dtype=np.uint32)
    for fn in (N.normals_from_words, REF.normals_from_words):
        z = fn(ext)
        assert np.isfinite(z).all() and np.abs(z).max() <= 5.89
        assert np.isfinite(z.astype(np.float16)).all()
        assert abs(abs(z[0, 0]) - (50 * np.log(2.0)) ** 0.5) < 1e-6           # u1 = 2^-25, cospi(2^-24) ~ 1
        assert np.abs(z[0, 4:6]).max() < 3e-4                                  # u1 = 1 - 2^-25: r ~ 2.4e-4
    assert np.array_equal(bits(N.normals_from_words(ext).astype(np.float16)), bits(REF.normals_from_words(ext).astype(np.float16)))


# ---------------------------------------------------------------- identities
def test_trajectory_ids():
    assert N.trajectory_id(0) == 0xE220A8397B1DCDAF                 # SplitMix64's first output from state 0 (its published vector)
    assert N.anchor_id(420) == REF.fold(REF.TAG_ANCHOR, 420) == 0x8B3185B8685E9F64
    assert N.mid_id(420, 421, 0.5, 2) == REF.fold(REF.TAG_MID, 420, 421, REF.f64_bits(0.5), 2) == 0x725D31D5498528AD
    assert N.free_id(0, 0) == REF.fold(REF.TAG_FREE, 0, 0) == 0x546F36061B6B1313
    assert (N.TAG_ANCHOR, N.TAG_MID, N.TAG_FREE, N.DRAW_STEP) == (1, 2, 3, 0)
    fracts = [i / 64 for i in range(1, 64)] + [0.5 + 2.0 ** -50, 0.1 + 0.2, 0.3]
    ids = {N.mid_id(420, 421, f, lvl) for f in fracts for lvl in (1, 2, 3)}
    assert len(ids) == 3 * len(fracts)                              # fracts (to the last bit) and levels
    ids |= {N.mid_id(s1, s2, 0.5, 2) for s1, s2 in ((421, 420), (420, 422), (0, 0), (1, 0), (0, 1))}
    ids |= {N.anchor_id(s) for s in range(200)} | {N.free_id(0, k) for k in range(200)} | {N.free_id(1, k) for k in range(200)}
    assert len(ids) == 3 * len(fracts) + 5 + 600
    assert all(0 <= i < 2 ** 64 for i in ids)
    assert N.anchor_id(np.int32(420)) == N.anchor_id(420)           # ('randomize' leaves numpy integers on the engine)
    # a row: key = id (low word first), ctr1 = step, ctr2 = draw kind, ctr3 = 0
    tid = N.anchor_id(7)
    assert N.noise_row(tid, 3) == (tid & 0xFFFFFFFF, tid >> 32, 3, 0, 0) == REF.row_of(tid, 3)


class Recording(N.CounterNoise):
    """CounterNoise that keeps {(id, step): bytes} of everything it was asked for (and how often)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.seen, self.requests = {}, 0

    def keyed(self, ids_and_steps, shape):
        out = super().keyed(ids_and_steps, shape)
        for (tid, step), z in zip(ids_and_steps, out):
            raw = z.numpy().tobytes()
            assert self.seen.setdefault((int(tid), int(step)), raw) == raw
            self.requests += 1
        return out


def test_counter_noise_source_on_cpu():
    src = N.CounterNoise("cpu", seed=5)
    a = src.keyed([(N.anchor_id(1), 0), (N.anchor_id(2), 3)], (2, 4, 4, 4))
    assert a.dtype == torch.float16 and tuple(a.shape) == (2, 4, 4, 4) and a.device.type == "cpu"
    rows = [REF.row_of(REF.fold(1, 1), 0), REF.row_of(REF.fold(1, 2), 3)]
    assert np.array_equal(bits(a.numpy().reshape(2, 64)), bits(REF.normals_f16(rows, 64)))
    # position independence of the host implementation: alone == as row 1 of 2
    assert torch.equal(src.keyed([(N.anchor_id(2), 3)], (1, 4, 4, 4))[0], a[1])
    # bound draws: the bound id and the scheduler's step index; a list binds one id per sample

    class Sched:
        _step_index = 3
    src.scheduler = Sched()
    assert src.bind(N.anchor_id(2)) is None
    assert torch.equal(src((1, 4, 4, 4))[0], a[1])
    assert src.bind([N.anchor_id(1), N.anchor_id(2)]) == N.anchor_id(2)
    Sched._step_index = 0
    assert torch.equal(src((2, 4, 4, 4))[0], a[0])
    src.bind(None)
    # unbound: TAG_FREE ids from the source's seed and its running call count (foreign code keeps working)
    f0, f1 = src((1, 4, 4, 4)), src.many(2, (1, 4, 4, 4))
    want = REF.normals_f16([REF.row_of(REF.fold(3, 5, k), 0) for k in range(3)], 64)
    assert np.array_equal(bits(torch.cat([f0, f1]).numpy().reshape(3, 64)), bits(want))
    with pytest.raises(ValueError):
        src.keyed([(1, 0)], (2, 4, 4, 4))
    Sched._step_index = None
    src.bind(7)
    with pytest.raises(RuntimeError, match="step"):
        src((1, 4, 4, 4))


# ---------------------------------------------------------------- path independence (CPU oracle pipe)
def _engine(width, farm=None, counter=True, **attrs):
    from oracle import pipe as OP, sdxl_ref as R
    from latentblending_amd import BlendingEngine
    p = OP.StableDiffusionXLPipeline(turbo=True, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg())
    if counter:
        p.scheduler.noise_source = Recording("cpu", scheduler=p.scheduler)
    np.random.seed(0)
    be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False, frontier_width=width, farm=farm)
    for k, v in attrs.items():
        assert hasattr(be, k)
        setattr(be, k, v)
    be.set_dimensions((128, 128))
    be.set_branching(nmb_max_branches=7)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    if counter:         # the engine's speed benchmark (set_dimensions) denoises unbound: TAG_FREE rows, which no transition shares
        src = p.scheduler.noise_source
        assert src.seen and all(t in {N.free_id(0, k) for k in range(src.requests)} for t, _ in src.seen)
        src.seen.clear()
        src.requests = 0
    return be, p


def _expected_keys(be):
    """The rows a transition USES: every committed branch at every step it ran (Euler-ancestral draws at each)."""
    steps = be.num_inference_steps
    keys = set()
    for f, idx in zip(be.tree_fracts, be.tree_idx_injection):
        tid = N.anchor_id(be.seed1) if f == 0.0 else N.anchor_id(be.seed2) if f == 1.0 else N.mid_id(be.seed1, be.seed2, f, idx)
        keys |= {(tid, i) for i in range(int(idx) if 0.0 < f < 1.0 else 0, steps)}
    return keys


@pytest.fixture(scope="module")
def sequential():
    from oracle import sdxl_ref as R
    from latentblending_amd.backend import set_backend
    set_backend(R.TorchCpuBackend())
    try:
        be, p = _engine(1)
        be.run_transition(fixed_seeds=[420, 421])
        src = p.scheduler.noise_source
        assert set(src.seen) == _expected_keys(be) and src.requests == len(src.seen)       # each row asked for once, none unused
        yield dict(seen=dict(src.seen), fracts=list(be.tree_fracts), idx=list(be.tree_idx_injection),
                   last=[t[-1].clone() for t in be.tree_latents])
    finally:
        set_backend(None)


@pytest.mark.parametrize("width,attrs", [(8, {}), (8, dict(speculate_virtual=False)), (8, dict(speculate_from_previous_tree=True)),
                                         (4, dict(speculation_oversubscribe=2.0)), (8, dict(elide_dead_steps=True)),
                                         (1, dict(elide_dead_steps=True))])
def test_draws_do_not_depend_on_the_path(width, attrs, sequential):
    from oracle import sdxl_ref as R
    from latentblending_amd.backend import set_backend
    set_backend(R.TorchCpuBackend())
    try:
        be, p = _engine(width, **attrs)
        be.run_transition(fixed_seeds=[420, 421])
        if attrs.get("speculate_from_previous_tree"):               # the second transition speculates from the first one's commit order
            p.scheduler.noise_source.seen.clear()
            be.run_transition(fixed_seeds=[420, 421])
    finally:
        set_backend(None)
    seen = p.scheduler.noise_source.seen
    assert be.tree_fracts == sequential["fracts"] and list(be.tree_idx_injection) == sequential["idx"]
    used = _expected_keys(be)
    assert used == set(sequential["seen"])
    # the same bytes for every row the tree uses; whatever else was asked for belongs to speculation that was dropped
    assert {k: seen[k] for k in used} == sequential["seen"]
    dropped = be.stats.get("speculation_dropped", 0)
    extra = set(seen) - used
    assert len({tid for tid, _ in extra}) <= dropped
    if dropped == 0:
        assert seen == sequential["seen"]
    # on the CPU the arithmetic is the same on every path too: the latents agree to the bit
    for a, b in zip(be.tree_latents, sequential["last"]):
        assert torch.equal(a[-1], b)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _farm_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import sdxl_ref as R
    from latentblending_amd.backend import set_backend
    from latentblending_amd.dist import BranchFarm
    import test_counter_noise_cpu as T
    set_backend(R.TorchCpuBackend())
    be, p = T._engine(8, farm=BranchFarm())
    be.run_transition(fixed_seeds=[420, 421])
    src = p.scheduler.noise_source
    json.dump({"seen": [[str(t), s, v.hex()] for (t, s), v in src.seen.items()], "requests": src.requests,
               "fracts": [float(f) for f in be.tree_fracts], "dropped": be.stats.get("speculation_dropped", 0),
               "last": [t[-1].numpy().tobytes().hex() for t in be.tree_latents]}, open(os.path.join(out_dir, f"rank{rank}.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()


def test_a_farm_draws_what_one_process_draws(sequential, tmp_path):
    """world 2 over gloo: each rank asks only for rows of branches it denoises itself (a subset, each row once), together they
    ask for exactly the rows the tree uses, and both end with the sequential engine's latents."""
    import torch.multiprocessing as mp
    mp.spawn(_farm_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    res = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(2)]
    whole = {(str(t), s): v.hex() for (t, s), v in sequential["seen"].items()}
    maps = [{(t, s): v for t, s, v in r["seen"]} for r in res]
    union = {}
    for r, m in zip(res, maps):
        assert r["fracts"] == sequential["fracts"]
        assert r["requests"] == len(m)
        assert r["last"] == [t.numpy().tobytes().hex() for t in sequential["last"]]
        if r["dropped"] == 0:
            assert set(m) < set(whole)                         # a proper subset: no rank does everything, none asks beyond the tree
        assert all(whole.get(k, v) == v for k, v in m.items())
        union.update(m)
    assert not set(maps[0]) & set(maps[1])                     # no row is drawn twice anywhere
    assert {k: union[k] for k in whole} == whole
    if all(r["dropped"] == 0 for r in res):
        assert union == whole


def test_stream_noise_is_left_alone(sequential):
    """Default settings: the engine neither installs nor binds anything - the pipe's own tape is the source before and after, and is
    called once per executed step, in the order of the sequential engine (2 anchors x steps, then each mid's steps from its
    injection), exactly as before counter-based noise existed."""
    from oracle import sdxl_ref as R
    from latentblending_amd.backend import set_backend
    set_backend(R.TorchCpuBackend())
    try:
        be, p = _engine(1, counter=False)
        tape, calls = p.noise, []
        inner = type(tape).__call__

        class Spy(type(tape)):
            def __call__(self, shape):
                calls.append(tuple(shape))
                return inner(self, shape)
        tape.__class__ = Spy
        assert p.scheduler.noise_source is tape and be._counter_source() is None
        be.run_transition(fixed_seeds=[420, 421])
    finally:
        set_backend(None)
    assert p.scheduler.noise_source is tape and not hasattr(tape, "bind")
    steps = be.num_inference_steps
    runs = 2 * steps + sum(steps - int(i) for f, i in zip(be.tree_fracts, be.tree_idx_injection) if 0.0 < f < 1.0)
    assert calls == [(1, 4, 16, 16)] * runs
    assert be.tree_fracts == sequential["fracts"]               # (same policy; other noise, so the latents differ)
    assert not any(torch.equal(a[-1], b) for a, b in zip(be.tree_latents, sequential["last"]))


# ---------------------------------------------------------------- launcher, host half
def test_launcher_refusals_and_recorded_name():
    import contextlib
    from latentblending_amd.hip import lib, ops
    api = lib.api
    assert lib.SIGNATURES["lb_counter_noise_f16"][2] == "launcher"
    P0, P1 = 0x100000, 0x200000                                 # fake, 16-byte aligned device pointers: a recording never launches

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

    bad = {"n = 0": (P0, P1, 64, 0, 0), "n < 0": (P0, P1, 64, -1, 0), "per_sample = 0": (P0, P1, 0, 2, 0),
           "per_sample < 0": (P0, P1, -8, 2, 0), "per_sample % 8": (P0, P1, 12, 2, 0), "per_sample % 8 (raw)": (P0, P1, 4, 2, 1),
           "null rows": (None, P1, 64, 2, 0), "null out": (P0, None, 64, 2, 0), "misaligned rows": (P0 + 8, P1, 64, 2, 0),
           "misaligned out": (P0, P1 + 2, 64, 2, 0), "misaligned out (raw)": (P0, P1 + 4, 64, 2, 1),
           "counter overflow": (P0, P1, 4 * 2 ** 32, 1, 0)}
    with recording() as h:
        for name, args in bad.items():
            with pytest.raises(RuntimeError, match=r"lb_counter_noise_f16 failed.*lb_counter_noise_f16: \w") as e:
                api.lb_counter_noise_f16(*args, None)
            assert api.lb_program_num_ops(h) == 0, name
            assert len(str(e.value)) > 40, name
        api.lb_counter_noise_f16(P0, P1, 64, 2, 0, None)
        api.lb_counter_noise_f16(P0, P1, 4 * (2 ** 32 - 2), 1, 1, None)          # the largest per_sample the counter takes
        assert [api.lb_program_op_name(h, i).decode() for i in range(api.lb_program_num_ops(h))] == ["lb_counter_noise_f16"] * 2
        # the wrapper: host rows would be uploaded into a buffer nobody owns once it returns - refused while recording
        with pytest.raises(RuntimeError, match="counter_noise: called while a program is recording"):
            ops.counter_noise([(1, 2, 3, 0, 0)], (1, 64), out=torch.empty(1, 64, dtype=torch.float16))
        assert api.lb_program_num_ops(h) == 2
    rows = ops.noise_rows([(1, 2, 3, 4, 5), (0xFFFFFFFF, 0, 0, 0, 2 ** 32 + 7)], "cpu")
    assert rows.dtype == torch.int32 and rows.tolist() == [[1, 2, 3, 4, 5, 0, 0, 0], [-1, 0, 0, 0, 7, 0, 0, 0]]
