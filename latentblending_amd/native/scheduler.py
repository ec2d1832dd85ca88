"""Host side of the native samplers: Euler / Euler-ancestral (diffusers 0.25 semantics for SDXL base and SDXL-Turbo; SURVEY.md
Appendix B.2), DDIM (eta 0), the latent-consistency sampler (LCM) and DPM-Solver++ 2M on uniform or Karras sigmas.  Only the
sigma / abar / timestep tables and the per-step scalar coefficients live here (``step_row``: Python floats, float64 numpy or
0-dim fp32 tensors, as each sampler's diffusers counterpart forms them); the tensor work runs in ``lb_scale_model_input_f16``,
``lb_euler_step_f16``, ``lb_ddim_step_f16``, ``lb_lcm_step_f16`` and ``lb_dpmpp2m_step_f16`` - one entry point per sampler.

Every sampler derives from :class:`NativeScheduler`, which owns what they share - the schedule bookkeeping, the diffusers-style
``scale_model_input`` / ``step`` pair the generic holder loop drives, the noise draws and the questions the native loops
(native/pipe.py) ask: ``step_row``, ``device_step``, ``device_step_kwargs``, ``multistep``, ``noise_draws``.  A subclass adds
its tables, ``set_timesteps``, ``step_row`` and the two launches.  ``make_scheduler`` maps a pipe's ``scheduler=`` name to one.

Reference call sites: /root/reference/latentblending/diffusers_holder.py:42,53,247 (set_timesteps),
:301 (order), :330 (scale_model_input), :356 (step).  Known answers: tests/golden/scheduler.json, tests/golden/sampler_rows.json.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from ..hip import ops
from ..planner import noise_draws_per_run          # noqa: F401  (its home is the planner; importable from here as before)

NUM_TRAIN_TIMESTEPS = 1000


def _sigma_table() -> np.ndarray:
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, NUM_TRAIN_TIMESTEPS, dtype=np.float64) ** 2
    alphas_cumprod = np.cumprod(1.0 - betas)
    return ((1 - alphas_cumprod) / alphas_cumprod) ** 0.5


def _alphas_cumprod_f32() -> torch.Tensor:
    """The abar table in fp32, built exactly as diffusers builds it (``torch.cumprod`` of fp32 alphas): DDIM's and LCM's."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, NUM_TRAIN_TIMESTEPS, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


class SeededDeviceNoise:
    """Noise stream ``callable(shape) -> fp16 tensor`` from a device generator with an explicit seed: the same
    seed gives the same stream on every rank of a branch farm (same GPU model, same torch build), which is what
    lets ranks compute the anchor trajectories redundantly instead of exchanging them."""

    def __init__(self, seed: int, device):
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)

    def __call__(self, shape):
        return torch.randn(tuple(shape), generator=self.gen, device=self.device, dtype=torch.float16)

    def many(self, n: int, shape):
        """``n`` draws of ``shape`` ([1, ...]) stacked along dim 0 as ONE generator call (one launch instead of n; every rank of a
        farm makes the same call, so the streams stay aligned)."""
        return torch.randn((int(n),) + tuple(shape[1:]), generator=self.gen, device=self.device, dtype=torch.float16)


class NativeScheduler:
    """What every native sampler is to its two callers.  The native loops (native/pipe.py) upload ``step_row(i, guidance, first)``
    for every step of a run and call ``device_step(x, eps, params, noise=, cfg=, **device_step_kwargs(i))`` once per step for the
    whole batch; the generic diffusers-style loop calls ``scale_model_input`` / ``step`` with timesteps taken from ``timesteps``.
    A subclass sets its tables in ``__init__`` BEFORE calling this one's (which installs the default schedule) and provides
    ``set_timesteps`` (ending in ``_install``), ``step_row``, ``device_step`` and ``_step_tensors``."""
    order = 1                    # model evaluations per step (as diffusers reports it; the engine's loops read this)
    kind = ""
    multistep = False            # True: ``device_step`` takes and returns a two-plane state (latents, previous x0 prediction)
    ancestral = False            # the Euler-ancestral update (whether ANY per-step noise is drawn is ``draws_noise`` / ``noise_draws``)
    draws_noise = False
    init_noise_sigma = 1.0
    default_steps = 30

    def __init__(self, device="cuda"):
        self.device = device
        self.noise_source = None          # callable(shape) -> tensor; None = device RNG
        self._step_index = None
        self.set_timesteps(self.default_steps)

    # ---- schedule ---------------------------------------------------------------------------
    def _install(self, timesteps: np.ndarray, n: int):
        """The end of every ``set_timesteps``: the schedule's timesteps, and a fresh run (no step located, no history)."""
        self.timesteps_np = timesteps.astype(np.float32)
        self.timesteps = torch.from_numpy(self.timesteps_np)   # host tensor: iterating it never syncs
        self.num_inference_steps = n
        self._step_index = None
        self._reset_history()

    def _reset_history(self):
        self._m1 = None                   # (a multistep sampler's previous x0 prediction under ``step``; the others never set it)

    def index_of(self, t) -> int:
        return int(np.nonzero(self.timesteps_np == float(t))[0][0])

    def _locate(self, t) -> int:
        if self._step_index is None:
            self._step_index = self.index_of(float(t))
        return self._step_index

    def is_last(self, i: int) -> bool:
        return i == self.num_inference_steps - 1

    def step_row(self, i: int, guidance: float = 0.0, first: bool = False):
        """The scalar coefficients of step ``i`` for the sampler's step kernel.  ``first`` = this is the first step the sample
        executes: a multistep sampler has no history then; a single-step sampler returns the same row either way."""
        raise NotImplementedError

    def noise_level(self, i: int) -> Tuple[float, float]:
        """``(a, b)`` with which a sample ENTERING step ``i`` is ``a x0 + b eps`` in this sampler's own units (``0 <= i <
        num_inference_steps``); ``i = num_inference_steps`` is where the last step lands.  Read from the tables ``step_row``
        reads, so that a forward-noised picture (an image anchor of the engine) sits on the trajectory the step kernel walks."""
        n = self.num_inference_steps
        if not 0 <= int(i) <= n:
            raise ValueError(f"noise_level: step {i} outside 0..{n}")
        return self._noise_level(int(i))

    def _noise_level(self, i: int) -> Tuple[float, float]:
        raise NotImplementedError

    # ---- noise ------------------------------------------------------------------------------
    def noise_draws(self, steps: int, idx_start: int) -> int:
        """Latent-shaped noise draws one run from ``idx_start`` of a ``steps``-step schedule consumes."""
        return 0

    def draw_noise(self, shape, device) -> torch.Tensor:
        if self.noise_source is not None:
            return self.noise_source(tuple(shape)).to(device=device, dtype=torch.float16)
        return torch.randn(shape, device=device, dtype=torch.float16)

    def draw_noise_many(self, n: int, shape, device) -> torch.Tensor:
        """``n`` draws of ``shape`` ([1, C, L, L]) stacked along dim 0, in draw order.  The device RNG (and a noise source with a
        ``many`` method) serves them with ONE launch - a cfg-2 transition draws 38 latents' worth of ancestral noise, 38 launches of
        ~14 us each before round 6; a source without ``many`` (a recorded tape) is called once per draw, in the same order."""
        n = int(n)
        if n == 0:
            return torch.empty((0,) + tuple(shape[1:]), device=device, dtype=torch.float16)
        if self.noise_source is None:
            return torch.randn((n,) + tuple(shape[1:]), device=device, dtype=torch.float16)
        many = getattr(self.noise_source, "many", None)
        if many is not None:
            return many(n, tuple(shape)).to(device=device, dtype=torch.float16)
        return torch.cat([self.draw_noise(shape, device) for _ in range(n)])

    # ---- the native loops' batched step ------------------------------------------------------
    def device_step(self, x, eps, params, noise=None, cfg=False, **kw):
        """One launch for all samples of the batch, per-sample rows in ``params``."""
        raise NotImplementedError

    def device_step_kwargs(self, i: int) -> dict:
        """What ``device_step`` of step ``i`` takes beside the tensors (``params`` is usually a view of one upload of all steps'
        rows, which carries no host mirror: what the launcher must know about the step, the scheduler says here)."""
        return {}

    # ---- diffusers-style tensor API (generic holder loop / foreign callers) ------------------
    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def step(self, model_output, timestep, sample, generator=None, return_dict=False, **_):
        i = self._locate(timestep)
        first = self.multistep and self._m1 is None
        params = ops.step_params([self.step_row(i, first=first)] * sample.shape[0], sample.device)
        out = self._step_tensors(i, sample, model_output.contiguous(), params)
        self._step_index += 1
        return (out,)

    def _step_tensors(self, i: int, sample, eps, params) -> torch.Tensor:
        raise NotImplementedError


def _no_noise(self, shape, device) -> torch.Tensor:
    """``draw_noise`` of a deterministic sampler (never called; it must not consume the device RNG)."""
    return torch.zeros(shape, device=device, dtype=torch.float16)


class NativeEulerScheduler(NativeScheduler):
    kind = "euler"

    def __init__(self, ancestral: bool, timestep_spacing: Optional[str] = None, device="cuda"):
        self.ancestral = ancestral
        self.timestep_spacing = timestep_spacing or ("trailing" if ancestral else "leading")
        self._table = _sigma_table()
        super().__init__(device)

    draws_noise = property(lambda self: self.ancestral)

    # ---- tables -----------------------------------------------------------------------------
    def set_timesteps(self, num_inference_steps: int, device=None):
        n = int(num_inference_steps)
        if self.timestep_spacing == "trailing":
            ts = np.round(np.arange(NUM_TRAIN_TIMESTEPS, 0, -NUM_TRAIN_TIMESTEPS / n)) - 1
        elif self.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (NUM_TRAIN_TIMESTEPS // n)).round()[::-1].copy() + 1   # steps_offset = 1
        else:
            raise ValueError(f"unsupported timestep_spacing {self.timestep_spacing}")
        ts = ts.astype(np.float32)
        sig = np.interp(ts, np.arange(0, NUM_TRAIN_TIMESTEPS), self._table)
        self.sigmas_np = np.concatenate([sig, [0.0]]).astype(np.float32)
        self.sigmas = torch.from_numpy(self.sigmas_np)
        self._install(ts, n)

    @property
    def init_noise_sigma(self) -> float:
        m = float(self.sigmas_np.max())
        return m if self.timestep_spacing in ("linspace", "trailing") else (m * m + 1) ** 0.5

    def step_row(self, i: int, guidance: float = 0.0, first: bool = False) -> Tuple[float, float, float, float, float]:
        """(sigma_from, sigma_next, sigma_up, guidance, dt) for ``lb_euler_step_f16``; computed in
        Python floats exactly like the scheduler's own scalar arithmetic."""
        s_from, s_to = float(self.sigmas_np[i]), float(self.sigmas_np[i + 1])
        if self.ancestral:
            s_up = (s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) ** 0.5
            s_down = (s_to ** 2 - s_up ** 2) ** 0.5
            return (s_from, s_down, s_up, guidance, s_down - s_from)
        return (s_from, s_to, 0.0, guidance, s_to - s_from)

    def _noise_level(self, i: int) -> Tuple[float, float]:
        """Sigma space: the latent is ``x0 + sigma_i eps`` (``sigmas_np`` ends in 0)."""
        return 1.0, float(self.sigmas_np[i])

    def noise_draws(self, steps: int, idx_start: int) -> int:
        return max(0, int(steps) - int(idx_start)) if self.ancestral else 0

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        i = self._locate(timestep)
        params = ops.step_params([self.step_row(i)] * sample.shape[0], sample.device)
        return ops.scale_model_input(sample.contiguous(), params)

    def device_step(self, x, eps, params, noise=None, cfg=False, **kw):
        return ops.euler_step(x, eps, params, noise=noise, cfg=cfg, ancestral=self.ancestral)

    def _step_tensors(self, i, sample, eps, params):
        noise = self.draw_noise(sample.shape, sample.device) if self.ancestral else None
        return ops.euler_step(sample.contiguous(), eps, params, noise=noise, ancestral=self.ancestral)


class NativeDDIMScheduler(NativeScheduler):
    """DDIM (eta = 0, epsilon prediction) as diffusers configures it for SD / SDXL: scaled-linear betas, leading spacing,
    steps_offset = 1, set_alpha_to_one = False, clip_sample = False.  Host side = the fp32 abar table built exactly as
    diffusers builds it (``torch.cumprod`` of fp32 alphas) and the per-step coefficients; the tensor work is
    ``lb_ddim_step_f16``.  ``scale_model_input`` is the identity and ``init_noise_sigma`` is 1.  Reached from
    /root/reference/latentblending/diffusers_holder.py:330,356 when a pipe carries this scheduler
    (``NativeSDXLPipe(scheduler="ddim")``); the reference's own SDXL pipes carry Euler schedulers (:42)."""
    kind = "ddim"

    def __init__(self, device="cuda"):
        self.alphas_cumprod = _alphas_cumprod_f32()                         # fp32, as diffusers holds it
        self.final_alpha_cumprod = self.alphas_cumprod[0]                   # set_alpha_to_one = False
        super().__init__(device)

    def set_timesteps(self, num_inference_steps: int, device=None):
        n = int(num_inference_steps)
        ratio = NUM_TRAIN_TIMESTEPS // n
        ts = (np.arange(0, n) * ratio).round()[::-1].copy().astype(np.int64) + 1          # leading, steps_offset = 1
        self._ratio = ratio
        self._install(ts, n)

    def alpha_pair(self, i: int):
        """(abar_t, abar_prev) of step ``i`` as 0-dim fp32 tensors (prev_timestep = t - 1000 // n; below 0: final_alpha_cumprod)."""
        t = int(self.timesteps_np[i])
        prev = t - self._ratio
        return self.alphas_cumprod[t], (self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod)

    def step_row(self, i: int, guidance: float = 0.0, first: bool = False):
        """(0, sqrt(abar_t), sqrt(abar_prev), guidance, sqrt(1 - abar_t), sqrt(1 - abar_prev), 1 / sqrt(abar_t)) in fp32 tensor
        arithmetic, the scalars diffusers forms inside DDIMScheduler.step (beta_prod_t ** 0.5, alpha_prod_t ** 0.5, ...).  The last
        one is the fp32 reciprocal the device library forms when a tensor is divided by a 0-dim host tensor (its true-division
        kernel multiplies by ``1 / b`` for a CPU scalar ``b``): ``lb_ddim_step_f16`` multiplies by it instead of dividing."""
        a_t, a_p = self.alpha_pair(i)
        sa_t = a_t ** 0.5
        inv = torch.ones((), dtype=torch.float32) / sa_t.to(torch.float32)
        return (0.0, float(sa_t), float(a_p ** 0.5), guidance, float((1 - a_t) ** 0.5), float((1 - a_p) ** 0.5), float(inv))

    def _noise_level(self, i: int) -> Tuple[float, float]:
        """(sqrt(abar), sqrt(1 - abar)) in the fp32 tensor arithmetic of ``step_row``; the landing point of the last step is its
        ``abar_prev`` side - ``final_alpha_cumprod``, not 1 (set_alpha_to_one = False)."""
        n = self.num_inference_steps
        a = self.alpha_pair(i)[0] if i < n else self.alpha_pair(n - 1)[1]
        return float(a ** 0.5), float((1 - a) ** 0.5)

    draw_noise = _no_noise                                      # (eta = 0)

    def device_step(self, x, eps, params, noise=None, cfg=False, **kw):
        return ops.ddim_step(x, eps, params, cfg=cfg)

    def _step_tensors(self, i, sample, eps, params):
        return ops.ddim_step(sample.contiguous(), eps, params)


LCM_ORIGINAL_STEPS = 50          # diffusers 0.25.0 LCMScheduler: original_inference_steps
LCM_TIMESTEP_SCALING = 10.0      # timestep_scaling
LCM_SIGMA_DATA = 0.5


def lcm_boundary_scalings(t: int) -> Tuple[float, float]:
    """(c_skip, c_out) of the consistency parameterisation at timestep ``t``, in Python floats as diffusers'
    ``get_scalings_for_boundary_condition_discrete`` forms them: s = 10 t, c_skip = 0.25 / (s^2 + 0.25), c_out = s / sqrt(s^2 + 0.25)."""
    s = t * LCM_TIMESTEP_SCALING
    sd2 = LCM_SIGMA_DATA ** 2
    return sd2 / (s ** 2 + sd2), s / (s ** 2 + sd2) ** 0.5


class NativeLCMScheduler(NativeScheduler):
    """Latent-consistency multistep sampler (Luo et al. 2023, "Latent Consistency Models", algorithm 3) as diffusers 0.25.0's
    ``LCMScheduler`` configures it for SDXL: scaled-linear betas, original_inference_steps = 50, timestep_scaling = 10,
    sigma_data = 0.5, epsilon prediction, no thresholding / clipping.  Restated from the published algorithm and that class's
    documented behaviour - not checked against diffusers itself.  Host side = the fp32 abar table (DDIM's), the timestep
    selection and the per-step coefficients; the tensor work is ``lb_lcm_step_f16``.  ``scale_model_input`` is the
    identity and ``init_noise_sigma`` is 1.  Every step but the LAST of the schedule re-noises the denoised latent with one fresh
    fp16 draw (``noise_draws``)."""
    kind = "lcm"
    draws_noise = True           # (``ancestral`` stays False: this is not the Euler-ancestral update)
    default_steps = 4

    def __init__(self, device="cuda"):
        self.alphas_cumprod = _alphas_cumprod_f32()                         # fp32, as diffusers holds it
        super().__init__(device)

    def set_timesteps(self, num_inference_steps: int, device=None):
        n = int(num_inference_steps)
        if n < 1 or n > LCM_ORIGINAL_STEPS:
            raise ValueError(f"NativeLCMScheduler: num_inference_steps must be in 1..{LCM_ORIGINAL_STEPS} (got {n})")
        origin = np.arange(1, LCM_ORIGINAL_STEPS + 1) * (NUM_TRAIN_TIMESTEPS // LCM_ORIGINAL_STEPS) - 1
        skip = LCM_ORIGINAL_STEPS // n
        ts = origin[::-1][::skip][:n].copy().astype(np.int64)
        self._install(ts, n)

    def noise_draws(self, steps: int, idx_start: int) -> int:
        return max(0, int(steps) - int(idx_start) - 1)

    def _noise_level(self, i: int) -> Tuple[float, float]:
        """(sqrt(abar_t), sqrt(1 - abar_t)) as ``step_row`` forms them; the last step returns the denoised latent itself."""
        if i == self.num_inference_steps:
            return 1.0, 0.0
        a = self.alphas_cumprod[int(self.timesteps_np[i])]
        return float(a ** 0.5), float((1 - a) ** 0.5)

    def step_row(self, i: int, guidance: float = 0.0, first: bool = False):
        """(0, c_skip, sqrt(abar_prev), guidance, sqrt(1 - abar_t), sqrt(1 - abar_prev), 1 / sqrt(abar_t), c_out): the boundary
        scalings in Python floats, the roots and the reciprocal in 0-dim fp32 tensor arithmetic (as ``NativeDDIMScheduler.step_row``
        forms its own).  The last step of the schedule has no previous timestep: its slots 2 and 5 are 0, which is how the kernel
        knows to return the denoised latent itself and to leave the noise unread."""
        t = int(self.timesteps_np[i])
        a_t = self.alphas_cumprod[t]
        inv = torch.ones((), dtype=torch.float32) / (a_t ** 0.5).to(torch.float32)
        c_skip, c_out = lcm_boundary_scalings(t)
        if self.is_last(i):
            sa_p = sb_p = 0.0
        else:
            a_p = self.alphas_cumprod[int(self.timesteps_np[i + 1])]
            sa_p, sb_p = float(a_p ** 0.5), float((1 - a_p) ** 0.5)
        return (0.0, c_skip, sa_p, guidance, float((1 - a_t) ** 0.5), sb_p, float(inv), c_out)

    def device_step(self, x, eps, params, noise=None, cfg=False, last: Optional[bool] = None, **kw):
        """``last``: the loop's statement that this is the schedule's last step for every sample of the batch - only then may
        ``noise`` be None (the launcher never reads the device rows back)."""
        return ops.lcm_step(x, eps, params, noise=noise, cfg=cfg, all_last=last)

    def device_step_kwargs(self, i: int) -> dict:
        return {"last": self.is_last(i)}

    def _step_tensors(self, i, sample, eps, params):
        noise = None if self.is_last(i) else self.draw_noise(sample.shape, sample.device)
        return ops.lcm_step(sample.contiguous(), eps, params, noise=noise)


KARRAS_RHO = 7.0


def dpmpp_schedule(n: int, karras: bool, table: Optional[np.ndarray] = None):
    """(sigmas [n + 1] with sigma_n = 0 appended, integer timesteps [n]) of an ``n``-step schedule, float64.  Karras: the ramp of
    Karras et al. 2022, eq. 5 (rho = 7) from table[999] down to table[0], timesteps by linear interpolation in log sigma, rounded.
    Otherwise the sigmas at Euler's "leading" timesteps with steps_offset 1.  Nothing is refused here: whether the timesteps can be
    shown to a UNet (strictly decreasing) is ``set_timesteps``' business - the sigmas alone define the solver."""
    table = _sigma_table() if table is None else table
    if karras:
        s_max, s_min = table[-1], table[0]
        ramp = np.linspace(0.0, 1.0, n)
        sig = (s_max ** (1 / KARRAS_RHO) + ramp * (s_min ** (1 / KARRAS_RHO) - s_max ** (1 / KARRAS_RHO))) ** KARRAS_RHO
        sig[0] = s_max                      # (the ramp's ends are the table's ends exactly, not to a rounding of the 7th power)
        if n > 1:
            sig[-1] = s_min
        ts = np.round(np.interp(np.log(sig), np.log(table), np.arange(NUM_TRAIN_TIMESTEPS, dtype=np.float64)))
    else:
        ts = (np.arange(0, n) * (NUM_TRAIN_TIMESTEPS // n)).round()[::-1].copy().astype(np.float64) + 1      # leading, steps_offset = 1
        sig = np.interp(ts, np.arange(0, NUM_TRAIN_TIMESTEPS), table)
    return np.concatenate([sig, [0.0]]), ts


def dpmpp_2m_row(sigmas: np.ndarray, i: int, guidance: float = 0.0, first: bool = False):
    """(0, sigma'_i, ratio, guidance, c0, c1, 1 / alpha_i, 1 / r0) of step ``i`` over ``sigmas`` (float64, 0 appended), in float64 -
    rounded once to fp32 on upload.  Variance-preserving form of the table: alpha = 1 / sqrt(sigma^2 + 1), sigma' = sigma alpha,
    lambda = log(alpha / sigma') = -log(sigma); with h = lambda_{i+1} - lambda_i: ratio = sigma'_{i+1} / sigma'_i,
    c0 = alpha_{i+1} expm1(-h), c1 = c0 / 2, r0 = (lambda_i - lambda_{i-1}) / h.  A FIRST-ORDER row has c1 = 0 (which is how the
    kernel knows to leave the previous x0 prediction unread): ``first``, step 0, and the step onto sigma = 0, whose row is
    ratio 0, c0 -1 - the x0 prediction itself."""
    sig_i, sig_n = float(sigmas[i]), float(sigmas[i + 1])
    a_i, a_n = 1.0 / (sig_i ** 2 + 1.0) ** 0.5, 1.0 / (sig_n ** 2 + 1.0) ** 0.5
    s_i, s_n = sig_i * a_i, sig_n * a_n
    if sig_n == 0.0:
        return (0.0, s_i, 0.0, guidance, -1.0, 0.0, 1.0 / a_i, 0.0)
    h = float(np.log(sig_i) - np.log(sig_n))
    c0 = a_n * float(np.expm1(-h))
    if first or i == 0:
        return (0.0, s_i, s_n / s_i, guidance, c0, 0.0, 1.0 / a_i, 0.0)
    r0 = float(np.log(sigmas[i - 1]) - np.log(sig_i)) / h
    return (0.0, s_i, s_n / s_i, guidance, c0, 0.5 * c0, 1.0 / a_i, 1.0 / r0)


class NativeDPMSolverPP2MScheduler(NativeScheduler):
    """DPM-Solver++ 2M (Lu et al. 2022, "DPM-Solver++", algorithm 2: second-order multistep, data prediction) in the form diffusers'
    ``DPMSolverMultistepScheduler`` takes with algorithm_type "dpmsolver++", solver_type "midpoint", final_sigmas_type "zero" and
    epsilon prediction, over uniform ("leading", steps_offset 1) or Karras (Karras et al. 2022, eq. 5, rho = 7) sigmas - what user
    interfaces call "DPM++ 2M" / "DPM++ 2M Karras".  Restated from the paper and that class's documented behaviour - not checked
    against diffusers itself.  Host side = the float64 sigma table (``_sigma_table``, as for Euler), the schedule and the per-step
    coefficients, each rounded ONCE to fp32 on upload; the tensor work is ``lb_dpmpp2m_step_f16``.  The sampler
    has a history (``multistep``): ``device_step`` takes and returns a two-plane state (latents, previous x0 prediction), and
    ``step_row`` heeds ``first`` - the first step a sample executes has no history and is first order, like the schedule's last
    step (whose target sigma is 0).  The reference's restartable loop calls ``set_timesteps`` at the start of every run, which
    empties a multistep scheduler's history: a branch entering at ``idx_start > 0`` starts first order too."""
    solver_order = 2
    kind = "dpmpp_2m"
    multistep = True
    default_steps = 20

    def __init__(self, use_karras_sigmas: bool = False, device="cuda"):
        self.use_karras_sigmas = bool(use_karras_sigmas)
        self._table = _sigma_table()
        super().__init__(device)

    # ---- tables -----------------------------------------------------------------------------
    def _schedule(self, n: int):
        return dpmpp_schedule(n, self.use_karras_sigmas, self._table)

    @staticmethod
    def _valid(ts) -> bool:
        # (strictly decreasing, inside the training range: Euler's "leading" formula puts the first of 1000 steps at t = 1000)
        return bool(np.all(np.diff(ts) < 0)) and 0 <= ts[-1] and ts[0] <= NUM_TRAIN_TIMESTEPS - 1

    def set_timesteps(self, num_inference_steps: int, device=None):
        n = int(num_inference_steps)
        if n < 1:
            raise ValueError(f"NativeDPMSolverPP2MScheduler: num_inference_steps must be at least 1 (got {n})")
        sig, ts = self._schedule(n)
        if not self._valid(ts):
            best = next(m for m in range(min(n, NUM_TRAIN_TIMESTEPS) - 1, 0, -1) if self._valid(self._schedule(m)[1]))
            raise ValueError(f"NativeDPMSolverPP2MScheduler: the timesteps of a {n}-step schedule are not strictly decreasing "
                             f"inside 0..{NUM_TRAIN_TIMESTEPS - 1} (the UNet would see one timestep twice, or one it was never trained on); the largest valid step count here is {best}")
        self.sigmas_np = sig                                                # float64 [n + 1]; sigma_n = 0
        self.sigmas = torch.from_numpy(self.sigmas_np.astype(np.float32))
        self._install(ts, n)

    def step_row(self, i: int, guidance: float = 0.0, first: bool = False):
        """The row of step ``i`` (``dpmpp_2m_row`` over this schedule's sigmas).  ``first`` = the sample has no history at this
        step - the first step it executes: a first-order row."""
        return dpmpp_2m_row(self.sigmas_np, i, guidance, first)

    def _noise_level(self, i: int) -> Tuple[float, float]:
        """(alpha_i, sigma'_i) of ``dpmpp_2m_row``'s variance-preserving form over the same ``sigmas_np`` (sigma_n = 0 -> (1, 0))."""
        sig = float(self.sigmas_np[i])
        a = 1.0 / (sig ** 2 + 1.0) ** 0.5
        return a, sig * a

    draw_noise = _no_noise                                      # (the solver is deterministic)

    def device_step(self, x, eps, params, noise=None, cfg=False, out=None, **kw):
        """``x`` [2, B, ...] (latents, previous x0 prediction) -> the next state."""
        return ops.dpmpp2m_step(x, eps, params, cfg=cfg, out=out)

    def _step_tensors(self, i, sample, eps, params):
        """One step with the history kept HERE (``_m1``, the previous call's x0 prediction; ``set_timesteps`` drops it)."""
        state = torch.empty((2,) + tuple(sample.shape), dtype=torch.float16, device=sample.device)
        state[0].copy_(sample)
        if self._m1 is not None:
            state[1].copy_(self._m1)
        out = ops.dpmpp2m_step(state, eps, params)
        self._m1 = out[1]
        return out[0]


SCHEDULER_NAMES = ("euler", "ddim", "lcm", "dpmpp_2m", "dpmpp_2m_karras")
_NAMES_TEXT = "'euler', 'ddim' or 'lcm'; also 'dpmpp_2m', 'dpmpp_2m_karras'"


def make_scheduler(name, turbo: bool, device) -> NativeScheduler:
    """The sampler a pipe's ``scheduler=`` argument names (case-insensitive, surrounding blanks ignored).  None or "euler" = the
    reference pipes' choice: Euler-ancestral for Turbo, Euler for base.  Anything else raises ``ValueError`` (a misspelt
    "DDIM " or a scheduler object used to fall through to Euler silently)."""
    if name is not None and not isinstance(name, str):
        raise ValueError(f"NativeSDXLPipe: scheduler must be None, {_NAMES_TEXT} "
                         f"(got an object of type {type(name).__name__})")
    name = "euler" if name is None else name.strip().lower()
    if name not in SCHEDULER_NAMES:
        raise ValueError(f"NativeSDXLPipe: unknown scheduler {name!r} (None, {_NAMES_TEXT})")
    if name == "euler":
        return NativeEulerScheduler(ancestral=turbo, device=device)
    if name == "ddim":
        return NativeDDIMScheduler(device=device)
    if name == "lcm":
        return NativeLCMScheduler(device=device)
    return NativeDPMSolverPP2MScheduler(use_karras_sigmas=name.endswith("karras"), device=device)
