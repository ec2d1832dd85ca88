"""CPU tests of the few-step path: the latent-consistency scheduler's tables, scalings and step against float64 closed forms, the
guidance-scale embedding, and the host layer's noise accounting under a sampler that draws at every step but the last.  No
kernel is launched here (``NativeLCMScheduler(device="cpu")`` only builds tables and rows)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import pipe as OP
from oracle import sdxl_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lcm_ref as LR  # noqa: E402

U16 = 2.0 ** -11            # unit round-off of fp16 (round to nearest)


@pytest.fixture()
def cpu_backend():
    from latentblending_amd.backend import set_backend
    set_backend(R.TorchCpuBackend())
    yield
    set_backend(None)


def native_sched():
    from latentblending_amd.native.scheduler import NativeLCMScheduler
    return NativeLCMScheduler(device="cpu")


# ---------------------------------------------------------------- timesteps and scalings
KNOWN_TIMESTEPS = {1: [999], 2: [999, 499], 3: [999, 679, 359], 4: [999, 759, 519, 279],
                   8: [999, 879, 759, 639, 519, 399, 279, 159]}


@pytest.mark.parametrize("n", sorted(KNOWN_TIMESTEPS))
def test_lcm_timesteps_known_answers(n):
    s, r = native_sched(), LR.LCMRefScheduler()
    s.set_timesteps(n)
    r.set_timesteps(n)
    assert [int(t) for t in s.timesteps.tolist()] == KNOWN_TIMESTEPS[n]
    assert r.timesteps.tolist() == KNOWN_TIMESTEPS[n]
    assert s.num_inference_steps == n and [s.index_of(t) for t in KNOWN_TIMESTEPS[n]] == list(range(n))
    assert s.kind == "lcm" and s.order == 1 and s.init_noise_sigma == 1.0
    x = torch.randn(1, 4, 8, 8)
    assert s.scale_model_input(x, 999) is x


@pytest.mark.parametrize("n", [0, 51, -3])
def test_lcm_timesteps_out_of_range_raise(n):
    with pytest.raises(ValueError):
        native_sched().set_timesteps(n)
    with pytest.raises(ValueError):
        LR.LCMRefScheduler().set_timesteps(n)


def test_lcm_boundary_scalings():
    from latentblending_amd.native.scheduler import lcm_boundary_scalings
    for t in (999, 759, 519, 279, 19):
        c_skip, c_out = lcm_boundary_scalings(t)
        s2 = np.float64(t * 10.0) ** 2
        want = (0.25 / (s2 + 0.25)) ** 2 + s2 / (s2 + 0.25)            # c_skip^2 + c_out^2 in float64
        assert abs(c_skip ** 2 + c_out ** 2 - float(want)) <= 4 * np.finfo(np.float64).eps
        assert (c_skip, c_out) == LR.boundary_scalings(t)
    assert lcm_boundary_scalings(999)[0] == 0.25 / (9990.0 ** 2 + 0.25)


# ---------------------------------------------------------------- the step
def test_lcm_step_is_exact_on_a_point_mass_and_fp16_stays_within_its_bound():
    """Data distribution = one point x*: x_t = sqrt(abar) x* + sqrt(1 - abar) n and the perfect model returns eps = n, so the
    float64 step must recover denoised = c_out x* + c_skip x_t.  The fp16 restatement rounds six times on the way to `denoised`;
    the bound below carries each rounding (relative 2^-11 of that intermediate) through the remaining operations, evaluated on the
    float64 intermediates (+1 % for second-order terms and the fp32 coefficient round-off, which is 2^-13 of one fp16 rounding)."""
    abar = LR.abar_f64()
    g = torch.Generator().manual_seed(11)
    xs = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    nz = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    ref = LR.LCMRefScheduler()
    ref.set_timesteps(4)
    for i, t in enumerate(LR.lcm_timesteps(4)):
        a_t = float(abar[t])
        x_t = a_t ** 0.5 * xs + (1 - a_t) ** 0.5 * nz
        c_skip, c_out = LR.boundary_scalings(t)
        _, den = LR.lcm_step_f64(x_t, nz, None, a_t, None, t)
        assert torch.allclose(den, c_out * xs + c_skip * x_t, rtol=0, atol=1e-11 * float(x_t.abs().max()) / a_t ** 0.5)
        # fp16: the same fp16 inputs on both sides
        x16, e16 = x_t.to(torch.float16), nz.to(torch.float16)
        a32 = float(ref.alphas_cumprod[t])                                   # (the table the fp16 side reads)
        _, den64 = LR.lcm_step_f64(x16, e16, None, a32, None, t)
        den16 = ref.denoised(i, e16, x16)
        x, e = x16.double(), e16.double()
        inv = 1 / a32 ** 0.5
        t1 = (1 - a32) ** 0.5 * e
        t2 = x - t1
        x0 = t2 * inv
        d1, d2 = c_out * x0, c_skip * x
        e_t2 = U16 * t1.abs() + U16 * t2.abs()
        e_x0 = inv * e_t2 + U16 * x0.abs()
        bound = 1.01 * (c_out * e_x0 + U16 * d1.abs() + U16 * d2.abs() + U16 * (d1 + d2).abs()) + 2.0 ** -24       # (+ half the smallest subnormal)
        err = (den16.double() - den64).abs()
        assert bool((err <= bound).all()), (t, float((err / bound).max()))


@pytest.mark.parametrize("n", [4, 8])
def test_lcm_step_rows_match_float64(n):
    """Every step's row against float64.  Tolerances are those of test_ddim_tables_and_step_match_closed_form: the fp32 cumprod
    of 1000 factors is within 2e-6 (relative) of the float64 one; roots and reciprocals formed in fp32 from an fp32 table entry
    are within 1e-6 (relative) of the float64 functions of that same entry."""
    s = native_sched()
    s.set_timesteps(n)
    abar64 = LR.abar_f64()
    table = s.alphas_cumprod.double().numpy()
    ts = LR.lcm_timesteps(n)
    for t in ts:
        assert abs(table[t] - abar64[t]) <= 2e-6 * abar64[t]
    assert torch.equal(s.alphas_cumprod, LR.LCMRefScheduler().alphas_cumprod)
    ref = LR.LCMRefScheduler()
    ref.set_timesteps(n)
    for i in range(n):
        row = s.step_row(i, 2.5)
        want = LR.lcm_row_f64(n, i, 2.5, abar=table)
        assert len(row) == 8 and row[0] == 0.0 and row[3] == 2.5
        assert row[1] == want[1] and row[7] == want[7]                       # Python-float scalings: the same expression
        assert np.allclose([row[2], row[4], row[5], row[6]], [want[2], want[4], want[5], want[6]], rtol=1e-6, atol=0)
        assert (row[5] == 0.0 and row[2] == 0.0) == (i == n - 1)
        # ... and bit for bit the fp32 values the reference scheduler multiplies by
        c_skip, c_out, sb_t, inv, sa_p, sb_p = ref.coefficients(i)
        f32 = lambda v: float(np.float32(v))                                  # noqa: E731
        assert (f32(row[1]), f32(row[7]), row[4], row[6]) == (c_skip, c_out, sb_t, inv)
        assert (row[2], row[5]) == ((sa_p, sb_p) if i < n - 1 else (0.0, 0.0))
    assert s.noise_draws(n, 0) == n - 1 and s.noise_draws(n, n - 1) == 0 and s.noise_draws(1, 0) == 0


def test_lcm_ref_step_matches_float64_with_noise():
    ref = LR.LCMRefScheduler()
    ref.set_timesteps(4)
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(2, 4, 8, 8, generator=g) * 3).half()
    e, nz = torch.randn(2, 4, 8, 8, generator=g).half(), torch.randn(2, 4, 8, 8, generator=g).half()
    ts = LR.lcm_timesteps(4)
    for i, t in enumerate(ts):
        a_t = float(ref.alphas_cumprod[t])
        a_p = float(ref.alphas_cumprod[ts[i + 1]]) if i < 3 else None
        ref.noise_source = lambda shape: nz
        got = ref.step(e, t, x)[0]
        want, _ = LR.lcm_step_f64(x, e, nz, a_t, a_p, t)
        # nine fp16 roundings, each of a value no larger than the amplified intermediates: 1 / sqrt(abar_999) = 14.6 at most
        assert got.dtype == torch.float16 and torch.allclose(got.double(), want, rtol=0, atol=float(want.abs().max()) * 9 * U16 + 16 * 4 * U16)
        got32 = ref.step(e.float(), t, x.float())[0]
        assert torch.allclose(got32.double(), want, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------- guidance-scale embedding
@pytest.mark.parametrize("dim", [256, 32, 33])
def test_guidance_scale_embedding_matches_float64(dim):
    from latentblending_amd.native.pipe import NativeSDXLPipe
    w = [0.0, 0.5, 7.0]
    got = NativeSDXLPipe.get_guidance_scale_embedding(torch.tensor(w), embedding_dim=dim)
    want = LR.guidance_embedding_f64(w, dim)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, dim)
    # fp32 round-off, carried to the angle: the exponent e_i = i ln(10000) / (half - 1) <= 9.2 is a product of fp32 values
    # (ln 10000, its quotient, the product: relative 3 * 2^-24, i.e. absolute 3 e_i 2^-24, which exp turns into the same RELATIVE
    # error of f_i), exp rounds once more (2^-23 relative allowed), w * 1000 and the product w f round once each (2^-24): the
    # angle is off by at most |angle| (3 e_i + 4) 2^-24, and sin / cos move by no more than the angle does, plus their own
    # rounding (2^-23 absolute for values <= 1)
    half = dim // 2
    e_i = np.arange(half) * np.log(10000.0) / (half - 1)
    arg = np.abs(np.asarray(w)[:, None] * 1000.0 * np.exp(-e_i)[None, :])
    tol_half = arg * (3 * e_i[None, :] + 4) * 2.0 ** -24 + 2.0 ** -23
    tol = np.concatenate([tol_half, tol_half] + ([np.zeros((3, 1))] if dim % 2 else []), axis=1)
    assert bool((np.abs(got.double().numpy() - want) <= tol).all())
    # sin block first: w = 0 gives [0 ... 0 | 1 ... 1]
    assert torch.equal(got[0, :half], torch.zeros(half)) and torch.equal(got[0, half:2 * half], torch.ones(half))
    if dim % 2:
        assert torch.equal(got[:, -1], torch.zeros(3))
    # the first frequency is 1: column 0 is sin(1000 w), column `half` is cos(1000 w)
    assert abs(float(got[1, 0]) - np.sin(500.0)) < 1e-4 and abs(float(got[1, half]) - np.cos(500.0)) < 1e-4


# ---------------------------------------------------------------- host layer: noise accounting
def _lcm_engine(frontier):
    from latentblending_amd import BlendingEngine
    p = OP.StableDiffusionXLPipeline(turbo=True, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg())
    p.scheduler = LR.LCMRefScheduler(noise_source=p.noise)
    np.random.seed(0)
    be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False, frontier_width=frontier)
    be.set_dimensions((128, 128))
    be.set_num_inference_steps(4)
    be.set_branching(nmb_max_branches=5)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    runs = []
    inner = be.dh._denoise_generic

    def counted(text_embeddings, latents_start, idx_start, list_latents_mixing, coeffs):
        before = p.noise.draws
        out = inner(text_embeddings, latents_start, idx_start, list_latents_mixing, coeffs)
        runs.append((int(idx_start), p.noise.draws - before))
        return out
    be.dh._denoise_generic = counted
    p.noise.reset()
    be.run_transition(fixed_seeds=[420, 421])
    return be, p, runs


def test_lcm_noise_accounting_and_frontier_tree(cpu_backend):
    """The host layer driving the oracle pipe under the latent-consistency sampler: every denoising run from ``idx_start`` draws
    exactly steps - idx_start - 1 latents (none at the schedule's last step), and the speculative frontier commits the tree the
    sequential engine commits."""
    steps = 4
    seq, p1, runs1 = _lcm_engine(1)
    spec, p8, runs8 = _lcm_engine(8)
    for runs, pipe in ((runs1, p1), (runs8, p8)):
        assert len(runs) >= 2 + 3 and runs[0][0] == 0
        for idx_start, drawn in runs:
            assert drawn == steps - idx_start - 1, (idx_start, drawn)
        assert pipe.noise.draws == sum(steps - i - 1 for i, _ in runs)
    assert seq._run_noise_draws(0) == 3 and seq._run_noise_draws(3) == 0 and seq._draws_noise(p1.scheduler)
    assert seq.tree_fracts == spec.tree_fracts and seq.tree_idx_injection == spec.tree_idx_injection
    assert len(seq.tree_fracts) >= 5 and len(set(seq.tree_idx_injection)) >= 2      # (two injection levels were exercised)


# ---------------------------------------------------------------- refusals that need no GPU
def test_lcm_null_noise_and_unknown_modes_are_refused_before_any_launch():
    """``ops.lcm_step`` decides from the HOST rows whether a null noise pointer is legal, and the launcher refuses what the
    wrapper would have refused (argument errors come back through the C-ABI error channel before anything is launched)."""
    from latentblending_amd.hip import lib, ops
    s = native_sched()
    s.set_timesteps(4)
    x = torch.zeros(2, 8, dtype=torch.float16)
    mixed = ops.step_params([s.step_row(3), s.step_row(1)], "cpu")
    with pytest.raises(ValueError, match="last step"):
        ops.lcm_step(x, x, mixed, noise=None)
    with pytest.raises(ValueError, match="not the last"):
        ops.lcm_step(x, x, mixed, noise=None, all_last=True)
    with pytest.raises(ValueError, match="cannot be established"):
        ops.lcm_step(x, x, torch.zeros(2, 8), noise=None)
    with pytest.raises(RuntimeError, match="lb_lcm_step_f16: .*needs noise"):
        lib.api.lb_lcm_step_f16(16, 16, None, 16, 16, 8, 1, 0, 0, None)
    with pytest.raises(RuntimeError, match="ancestral step needs noise"):
        lib.api.lb_euler_step_f16(16, 16, None, 16, 16, 8, 1, 0, 1, None)
    with pytest.raises(RuntimeError, match="lb_euler_step_f16: ancestral is 0 or 1"):
        lib.api.lb_euler_step_f16(16, 16, 16, 16, 16, 8, 1, 0, 3, None)
    for bad in (2, 3, 4):           # (2 was "every row is a last step" when this was a mode of the Euler step: an argument now)
        with pytest.raises(RuntimeError, match="lb_lcm_step_f16: cfg bits"):
            lib.api.lb_lcm_step_f16(16, 16, 16, 16, 16, 8, 1, bad, 0, None)
    # the overloading is gone: what used to select the latent-consistency step is refused, and the message says where it went
    for noise in (None, 16):
        with pytest.raises(RuntimeError, match="lb_lcm_step_f16"):
            lib.api.lb_euler_step_f16(16, 16, noise, 16, 16, 8, 1, 0, 2, None)
    with pytest.raises(RuntimeError, match="lb_euler_step_f16: cfg is 0 or 1"):
        lib.api.lb_euler_step_f16(16, 16, 16, 16, 16, 8, 1, 2, 0, None)


def test_pipe_names_lcm_among_its_schedulers():
    from latentblending_amd.native.pipe import NativeSDXLPipe
    with pytest.raises(ValueError, match="'euler', 'ddim' or 'lcm'"):
        NativeSDXLPipe(turbo=True, scheduler="lcms")
    with pytest.raises(ValueError, match="'euler', 'ddim' or 'lcm'"):
        NativeSDXLPipe(turbo=True, scheduler=object())
