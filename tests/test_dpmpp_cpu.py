"""CPU tests of the second-order sampler: the DPM-Solver++ 2M scheduler's tables against float64 closed forms, its order of
convergence on the one model where the probability-flow ODE has a closed form, exactness on a point mass, the refusals of the
launcher and the wrapper, the pipe's scheduler names, and the restart rule under the generic loop.  No kernel is launched here
(``NativeDPMSolverPP2MScheduler(device="cpu")`` only builds tables and rows)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import pipe as OP
from oracle import sdxl_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dpmpp_ref as DR  # noqa: E402

F16 = torch.float16


@pytest.fixture()
def cpu_backend():
    from latentblending_amd.backend import set_backend
    set_backend(R.TorchCpuBackend())
    yield
    set_backend(None)


def native_sched(karras):
    from latentblending_amd.native.scheduler import NativeDPMSolverPP2MScheduler
    return NativeDPMSolverPP2MScheduler(use_karras_sigmas=karras, device="cpu")


# ---------------------------------------------------------------- tables
def test_class_attributes_and_identity_scale():
    s = native_sched(True)
    assert s.kind == "dpmpp_2m" and s.order == 1 and s.solver_order == 2 and s.multistep is True and s.ancestral is False
    assert s.init_noise_sigma == 1.0 and s.noise_draws(20, 0) == 0 and s.noise_draws(20, 7) == 0
    x = torch.randn(1, 4, 8, 8)
    assert s.scale_model_input(x, 999) is x


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 6, 20, 30])
def test_rows_match_float64_closed_forms(n, karras):
    """Every slot of every row, as a second-order row and as a first-order one, against tests/_dpmpp_ref.py's float64 forms (an
    independent restatement: its own table, ramp and interpolation), to fp32 rounding - the rows are float64 on the host and
    rounded once on upload, so the two float64 computations may differ by a few float64 ulps and nothing more."""
    from latentblending_amd.hip import ops
    s = native_sched(karras)
    s.set_timesteps(n)
    sig = DR.sigmas_f64(n, karras)
    assert s.num_inference_steps == n and len(s.sigmas_np) == n + 1 and s.sigmas_np[-1] == 0.0
    np.testing.assert_allclose(s.sigmas_np, sig, rtol=1e-12, atol=0)
    assert [int(t) for t in s.timesteps.tolist()] == DR.timesteps_of(sig)
    assert [s.index_of(t) for t in s.timesteps.tolist()] == list(range(n))
    ts = s.timesteps_np
    assert np.all(np.diff(ts) < 0) and ts[0] <= 999 and ts[-1] >= 0
    table = DR.sigma_table_f64()
    if karras:
        assert s.sigmas_np[0] == table[999] and (n == 1 or s.sigmas_np[n - 1] == table[0])
        assert int(ts[0]) == 999 and (n == 1 or int(ts[-1]) == 0)
    else:
        assert int(ts[-1]) == 1 and s.sigmas_np[n - 1] == table[1]
    for i in range(n):
        for first in (False, True):
            got = s.step_row(i, 3.5, first=first)
            want = DR.row_f64(sig, i, 3.5, first=first)
            assert len(got) == 8 and got[0] == 0.0 and got[3] == 3.5
            np.testing.assert_allclose(np.array(got, dtype=np.float64), np.array(want), rtol=1e-10, atol=0)
            up = ops.step_params([got], "cpu")[0].numpy()
            assert up.dtype == np.float32 and np.all(np.abs(up.astype(np.float64) - np.array(want)) <= np.abs(want) * 2.0 ** -24 * 1.001)
            if first or i == 0 or i == n - 1:
                assert got[5] == 0.0 and got[7] == 0.0, "first-order rows carry c1 == 0"
            else:
                assert got[5] == 0.5 * got[4] and got[5] != 0.0 and got[7] > 0.0
    last = s.step_row(n - 1, 2.0)
    assert last[2] == 0.0 and last[4] == -1.0 and last[5] == 0.0


def test_row_closed_forms_by_hand():
    """One second-order row written out from the paper's formulas, independent of both implementations' helpers."""
    s = native_sched(True)
    s.set_timesteps(20)
    i = 7
    sg = s.sigmas_np
    al = 1 / np.sqrt(sg ** 2 + 1)
    sp = sg * al
    lam = np.log(al[:-1] / sp[:-1])
    h, h0 = lam[i + 1] - lam[i], lam[i] - lam[i - 1]
    want = [0.0, sp[i], sp[i + 1] / sp[i], 1.5, al[i + 1] * (math.exp(-h) - 1), 0.5 * al[i + 1] * (math.exp(-h) - 1), 1 / al[i], h / h0]
    np.testing.assert_allclose(np.array(s.step_row(i, 1.5)), np.array(want), rtol=1e-9)


def test_timesteps_that_repeat_are_refused_with_the_largest_valid_count():
    s = native_sched(True)
    with pytest.raises(ValueError, match="strictly decreasing") as e:
        s.set_timesteps(200)
    best = int(str(e.value).rsplit(" ", 1)[-1])
    assert 20 < best < 200
    s.set_timesteps(best)                   # what it names is valid ...
    assert np.all(np.diff(s.timesteps_np) < 0)
    bad = best + 1
    with pytest.raises(ValueError, match=f"largest valid step count here is {best}"):
        s.set_timesteps(bad)                # ... and the next one is not
    assert s.num_inference_steps == best    # a refused call leaves the schedule as it was
    u = native_sched(False)
    u.set_timesteps(999)
    assert int(u.timesteps_np[0]) == 999
    with pytest.raises(ValueError, match="largest valid step count here is 999"):
        u.set_timesteps(1000)               # ("leading" with steps_offset 1 would start at t = 1000, outside the training range)
    with pytest.raises(ValueError, match="strictly decreasing"):
        u.set_timesteps(1001)
    for n in (0, -3):
        with pytest.raises(ValueError):
            s.set_timesteps(n)


# ---------------------------------------------------------------- convergence
def gaussian_flow_error(n, s_data, second_order, through_last_step, karras=True):
    """Gaussian data x0 ~ N(0, s^2): the ideal eps-predictor is eps = sigma' x / (alpha^2 s^2 + sigma'^2) and the probability-flow
    solution is x proportional to sqrt(alpha^2 s^2 + sigma'^2).  Relative error of the sampler's latent against it, float64, over
    the scheduler's own rows (``dpmpp_schedule`` / ``dpmpp_2m_row`` are what ``set_timesteps`` / ``step_row`` call; taken directly
    because n = 160 Karras timesteps repeat after rounding, which matters to a UNet and not to the sigmas)."""
    from latentblending_amd.native.scheduler import dpmpp_2m_row, dpmpp_schedule
    sig, _ = dpmpp_schedule(n, karras)
    al = 1 / np.sqrt(sig ** 2 + 1)
    sp = sig * al
    scale = lambda k: math.sqrt(al[k] ** 2 * s_data ** 2 + sp[k] ** 2)        # noqa: E731
    x, m1 = scale(0), None
    stop = n if through_last_step else n - 1
    for i in range(stop):
        row = dpmpp_2m_row(sig, i, 0.0, first=not second_order)
        e = sp[i] * x / (al[i] ** 2 * s_data ** 2 + sp[i] ** 2)
        x, m1 = DR.dpmpp_step_f64(row, x, e, m1)
    return abs(x - scale(stop)) / scale(stop)


def test_order_of_convergence_on_the_gaussian_model():
    """The latent entering the last step (at sigma = table[0]), n = 20, 40, 80, 160 on Karras sigmas, s = 0.5: the error falls
    >= 3.5x per doubling with the second-order rows (measured 4.38, 4.22, 4.11: order 2 in the limit) and 1.8x .. 2.2x with every
    row forced first order (2.01, 2.00, 2.00)."""
    e2 = [gaussian_flow_error(n, 0.5, True, False) for n in (20, 40, 80, 160)]
    e1 = [gaussian_flow_error(n, 0.5, False, False) for n in (20, 40, 80, 160)]
    r2 = [a / b for a, b in zip(e2[:-1], e2[1:])]
    r1 = [a / b for a, b in zip(e1[:-1], e1[1:])]
    print(f"[dpmpp] order 2: errors {e2} ratios {r2}; order 1: errors {e1} ratios {r1}")
    assert all(r >= 3.5 for r in r2), r2
    assert all(1.8 <= r <= 2.2 for r in r1), r1


@pytest.mark.parametrize("s_data", [0.25, 0.5, 1.0, 2.0])
def test_twenty_second_order_steps_beat_forty_first_order_steps(s_data):
    """End to end, last step included (measured: about 1e-2 against 3.4e-2 .. 5.2e-2)."""
    e2, e1 = gaussian_flow_error(20, s_data, True, True), gaussian_flow_error(40, s_data, False, True)
    print(f"[dpmpp] s={s_data}: 2M at 20 steps {e2:.3e}, first order at 40 steps {e1:.3e}")
    assert e2 < e1


@pytest.mark.parametrize("karras", [False, True])
def test_point_mass_is_returned_by_every_step(karras):
    """Data concentrated on one point c: the ideal predictor is eps = (x - alpha c) / sigma', so m0 = c at every step, the
    difference term vanishes and every step lands on alpha' c + sigma' z for the z it started with - at the end on c itself."""
    n = 8
    s = native_sched(karras)
    s.set_timesteps(n)
    sg = s.sigmas_np
    al = 1 / np.sqrt(sg ** 2 + 1)
    sp = sg * al
    g = torch.Generator().manual_seed(3)
    c, z = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    x, m1 = al[0] * c + sp[0] * z, None
    for i in range(n):
        e = (x - al[i] * c) / sp[i]
        x, m1 = DR.dpmpp_step_f64(s.step_row(i, 0.0), x, e, m1)
        assert torch.allclose(m1, c, rtol=0, atol=1e-9)
        assert torch.allclose(x, al[i + 1] * c + sp[i + 1] * z, rtol=0, atol=1e-9)
    assert torch.allclose(x, c, rtol=0, atol=1e-9)


def test_reference_scheduler_last_step_returns_m0_bit_for_bit():
    """The last row (ratio 0, c0 -1): 0 * x = 0 and 0 - (-m0) is exact in fp16."""
    g = torch.Generator().manual_seed(5)
    x, e = (torch.randn(2, 300, generator=g) * 3).to(F16), torch.randn(2, 300, generator=g).to(F16)
    sig = DR.sigmas_f64(6, True)
    y, m0 = DR.dpmpp_step_f16(DR.row_f64(sig, 5), x, e, None)
    assert torch.equal(y.view(torch.int16), m0.view(torch.int16))


# ---------------------------------------------------------------- refusals that need no GPU
def test_launcher_refuses_unknown_cfg_bits_and_bad_sizes():
    """Argument errors come back through the C-ABI error channel before anything is launched (fake aligned pointers)."""
    from latentblending_amd.hip import lib
    for bad in (4, 5, 8, -1):
        with pytest.raises(RuntimeError, match="lb_ddim_step_f16: cfg bits"):
            lib.api.lb_ddim_step_f16(16, 16, 16, 16, 8, 1, bad, None)
        with pytest.raises(RuntimeError, match="lb_dpmpp2m_step_f16: cfg bits"):
            lib.api.lb_dpmpp2m_step_f16(16, 16, 16, 16, 8, 1, bad, None)
    for bad in (2, 3):
        with pytest.raises(RuntimeError, match="lb_dpmpp2m_step_f16: cfg bits"):
            lib.api.lb_dpmpp2m_step_f16(16, 16, 16, 16, 8, 1, bad, None)
        # the overloading is gone: what used to select the DPM-Solver++ 2M step is refused, and the message says where it went
        with pytest.raises(RuntimeError, match="lb_ddim_step_f16: .*lb_dpmpp2m_step_f16"):
            lib.api.lb_ddim_step_f16(16, 16, 16, 16, 8, 1, bad, None)
    for per_sample, batch in ((0, 1), (8, 0), (-8, 1)):
        for cfg in (0, 2, 3):
            with pytest.raises(RuntimeError, match="lb_ddim_step_f16: sizes"):
                lib.api.lb_ddim_step_f16(16, 16, 16, 16, per_sample, batch, cfg, None)
        for cfg in (0, 1):
            with pytest.raises(RuntimeError, match="lb_dpmpp2m_step_f16: sizes"):
                lib.api.lb_dpmpp2m_step_f16(16, 16, 16, 16, per_sample, batch, cfg, None)


def test_wrapper_refuses_one_plane_state_aliasing_out_and_a_missing_out_while_recording():
    from latentblending_amd.hip import lib, ops
    s = native_sched(True)
    s.set_timesteps(6)
    params = ops.step_params([s.step_row(2, 0.0)] * 2, "cpu")
    eps = torch.zeros(2, 8, dtype=F16)
    with pytest.raises(ValueError, match="two planes"):
        ops.dpmpp2m_step(torch.zeros(2, 8, dtype=F16), eps, params)
    with pytest.raises(ValueError, match="two planes"):
        ops.dpmpp2m_step(torch.zeros(1, 2, 8, dtype=F16), eps, params)
    state = torch.zeros(2, 2, 8, dtype=F16)
    with pytest.raises(ValueError, match="two planes"):
        ops.dpmpp2m_step(state, eps, params, out=torch.zeros(2, 8, dtype=F16))
    with pytest.raises(ValueError, match="aliases"):
        ops.dpmpp2m_step(state, eps, params, out=state)
    big = torch.zeros(3, 2, 8, dtype=F16)
    with pytest.raises(ValueError, match="aliases"):
        ops.dpmpp2m_step(big[:2], eps, params, out=big[1:])           # (overlapping by one plane)
    with pytest.raises(ValueError, match="eps"):
        ops.dpmpp2m_step(state, eps, params, cfg=True)                # CFG needs 2 B samples of eps
    prog = lib.api.lb_program_create()
    lib.api.lb_program_begin_record(prog)
    try:
        with pytest.raises(RuntimeError, match="caller-owned out"):
            ops.dpmpp2m_step(state, eps, params)
    finally:
        lib.api.lb_program_end_record(prog)
    assert lib.api.lb_program_num_ops(prog) == 0
    lib.api.lb_program_destroy(prog)


def test_pipe_accepts_the_new_names_and_still_refuses_near_misses():
    """Without a device the constructor gets past its name check and stops at "needs an MI355X"; a refused name never gets there."""
    from latentblending_amd.native.pipe import NativeSDXLPipe
    for name in ("dpm", "dpmpp", "dpmpp_2m_sde", "dpmpp2m"):
        with pytest.raises(ValueError, match="'euler', 'ddim' or 'lcm'; also 'dpmpp_2m', 'dpmpp_2m_karras'"):
            NativeSDXLPipe(turbo=False, scheduler=name)
    with pytest.raises(ValueError, match="'euler', 'ddim' or 'lcm'; also 'dpmpp_2m', 'dpmpp_2m_karras'"):
        NativeSDXLPipe(turbo=False, scheduler=object())
    if not torch.cuda.is_available():
        for name in ("dpmpp_2m", "dpmpp_2m_karras", " DPMPP_2M_Karras "):
            with pytest.raises(RuntimeError, match="MI355X"):
                NativeSDXLPipe(turbo=False, scheduler=name)


# ---------------------------------------------------------------- restart rule under the generic loop
class _TappedUNet:
    """The oracle pipe's UNet, with every call's input latent and output kept."""

    def __init__(self, inner):
        self.inner, self.config, self.seen = inner, inner.config, []

    def __call__(self, sample, timestep, **kw):
        out = self.inner(sample, timestep, **kw)
        self.seen.append((int(timestep), sample.clone(), out[0].clone()))
        return out


def test_a_run_entering_at_idx_start_2_starts_first_order_under_the_generic_loop(cpu_backend):
    """The restartable loop calls ``set_timesteps`` at the start of every run, so a multistep scheduler starts each run - also
    one entering at ``idx_start`` = 2 - without history: its first executed step is the first-order formula, its second one the
    second-order formula over the first one's x0 prediction, and a second run right after repeats the first bit for bit."""
    from latentblending_amd import DiffusersHolder
    p = OP.StableDiffusionXLPipeline(turbo=True, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg())
    p.scheduler = DR.DPMPPRefScheduler(use_karras_sigmas=True)
    p.unet = _TappedUNet(p.unet)
    dh = DiffusersHolder(p)
    dh.set_dimensions((128, 128))
    dh.set_num_inference_steps(5)
    dh.guidance_scale = 1.0                  # (no CFG: the UNet's output IS the eps the scheduler gets)
    emb = dh.get_text_embedding("a reef")
    z = dh.get_noise(11)
    full = dh.run_diffusion(emb, z, idx_start=0)
    assert len(p.unet.seen) == 5
    p.unet.seen.clear()
    start = full[1]
    traj = dh.run_diffusion(emb, start, idx_start=2)
    assert traj[:2] == [None, None] and len(p.unet.seen) == 3
    sig = DR.sigmas_f64(5, True)
    assert [t for t, _, _ in p.unet.seen] == DR.timesteps_of(sig)[2:]
    (_, x2, e2), (_, x3, e3), _ = p.unet.seen
    assert x2.dtype == F16 and torch.equal(x2, start)
    y2, m2 = DR.dpmpp_step_f16(DR.row_f64(sig, 2, first=True), x2, e2, None)
    assert torch.equal(traj[2].view(torch.int16), y2.view(torch.int16))
    y2_second, _ = DR.dpmpp_step_f16(DR.row_f64(sig, 2), x2, e2, torch.zeros_like(x2))
    assert not torch.equal(traj[2], y2_second)
    assert not torch.equal(traj[2], full[2]), "the run from step 0 took step 2 with history: the case proves nothing"
    y3, _ = DR.dpmpp_step_f16(DR.row_f64(sig, 3), x3, e3, m2)
    assert torch.equal(x3, traj[2]) and torch.equal(traj[3].view(torch.int16), y3.view(torch.int16))
    again = dh.run_diffusion(emb, start, idx_start=2)
    assert all(torch.equal(a, b) for a, b in zip(traj[2:], again[2:]))


# ---------------------------------------------------------------- host layer around a sampler with history and no noise
def _engine(frontier, elide=False):
    from latentblending_amd import BlendingEngine
    p = OP.StableDiffusionXLPipeline(turbo=True, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg())
    p.scheduler = DR.DPMPPRefScheduler(use_karras_sigmas=False)
    np.random.seed(0)
    be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False, frontier_width=frontier)
    be.elide_dead_steps = elide
    be.set_dimensions((128, 128))
    be.set_num_inference_steps(4)
    be.set_branching(nmb_max_branches=4)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    return be, p


def test_engine_draws_no_noise_and_session_and_state_dict_carry_nothing_of_the_sampler(cpu_backend):
    """The engine's noise accounting sees a sampler that draws nothing (so a farm skips nothing for other ranks' runs), the
    speculative frontier commits the sequential tree with the same frames (every run starts its own history: the order of
    evaluation does not reach a result), and neither the state dict nor an ``EngineSession`` holds anything of the scheduler -
    it lives on the pipe - so a transition inside a bound session is the transition outside it."""
    from latentblending_amd import EngineSession
    from latentblending_amd.native.scheduler import noise_draws_per_run
    seq, p1 = _engine(1)
    assert not seq._draws_noise(p1.scheduler) and seq._run_noise_draws(0) == 0 and seq._run_noise_draws(2) == 0
    assert noise_draws_per_run(native_sched(True), 20, 0) == 0 and noise_draws_per_run(native_sched(False), 20, 5) == 0
    a = [np.asarray(f) for f in seq.run_transition(fixed_seeds=[420, 421])]
    assert p1.noise.draws == 0
    spec, _ = _engine(8)
    b = [np.asarray(f) for f in spec.run_transition(fixed_seeds=[420, 421])]
    assert seq.tree_fracts == spec.tree_fracts and seq.tree_idx_injection == spec.tree_idx_injection
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not any("sched" in k.lower() or "m1" == k for k in seq.get_state_dict())
    be, _ = _engine(1)
    with EngineSession(be).bound() as bound:
        c = [np.asarray(f) for f in bound.run_transition(fixed_seeds=[420, 421])]
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
