"""Host side of the Euler / Euler-ancestral schedulers (diffusers 0.25 semantics for SDXL base
and SDXL-Turbo).  Only the sigma / timestep tables and per-step scalar
coefficients live here (float64 numpy); the tensor work — ``x / sqrt(sigma^2+1)``, CFG combine
and the update — runs in ``lb_scale_model_input_f16`` / ``lb_euler_step_f16``.  ``NativeDDIMScheduler`` and
``NativeLCMScheduler`` (few-step sampling: diffusers' ``LCMScheduler``) keep the same interface over an fp32 abar table;
their tensor work is ``lb_ddim_step_f16`` and mode 2 of ``lb_euler_step_f16``.

Reference call sites: /root/reference/latentblending/diffusers_holder.py:42,53,247 (set_timesteps),
:301 (order), :330 (scale_model_input), :356 (step).  Known answers: tests/golden/scheduler.json.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from ..hip import ops

NUM_TRAIN_TIMESTEPS = 1000


def _sigma_table() -> np.ndarray:
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, NUM_TRAIN_TIMESTEPS, dtype=np.float64) ** 2
    alphas_cumprod = np.cumprod(1.0 - betas)
    return ((1 - alphas_cumprod) / alphas_cumprod) ** 0.5


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


class NativeEulerScheduler:
    order = 1
    kind = "euler"

    def __init__(self, ancestral: bool, timestep_spacing: Optional[str] = None, device="cuda"):
        self.ancestral = ancestral
        self.timestep_spacing = timestep_spacing or ("trailing" if ancestral else "leading")
        self.device = device
        self._table = _sigma_table()
        self.noise_source = None          # callable(shape) -> tensor; None = device RNG
        self._step_index = None
        self.set_timesteps(30)

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
        self.timesteps_np = ts
        self.timesteps = torch.from_numpy(ts)                  # host tensor: iterating it never syncs
        self.sigmas = torch.from_numpy(self.sigmas_np)
        self.num_inference_steps = n
        self._step_index = None

    @property
    def init_noise_sigma(self) -> float:
        m = float(self.sigmas_np.max())
        return m if self.timestep_spacing in ("linspace", "trailing") else (m * m + 1) ** 0.5

    def index_of(self, t) -> int:
        hits = np.nonzero(self.timesteps_np == float(t))[0]
        return int(hits[0])

    def step_row(self, i: int, guidance: float = 0.0) -> Tuple[float, float, float, float, float]:
        """(sigma_from, sigma_next, sigma_up, guidance, dt) for ``lb_euler_step_f16``; computed in
        Python floats exactly like the scheduler's own scalar arithmetic."""
        s_from, s_to = float(self.sigmas_np[i]), float(self.sigmas_np[i + 1])
        if self.ancestral:
            s_up = (s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) ** 0.5
            s_down = (s_to ** 2 - s_up ** 2) ** 0.5
            return (s_from, s_down, s_up, guidance, s_down - s_from)
        return (s_from, s_to, 0.0, guidance, s_to - s_from)

    # ---- diffusers-style tensor API (generic holder loop / foreign callers) ------------------
    def _locate(self, t) -> int:
        if self._step_index is None:
            self._step_index = self.index_of(float(t))
        return self._step_index

    def scale_model_input(self, sample: torch.Tensor, timestep) -> torch.Tensor:
        i = self._locate(timestep)
        params = ops.step_params([self.step_row(i)] * sample.shape[0], sample.device)
        return ops.scale_model_input(sample.contiguous(), params)

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

    def step(self, model_output, timestep, sample, generator=None, return_dict=False, **_):
        i = self._locate(timestep)
        B = sample.shape[0]
        params = ops.step_params([self.step_row(i)] * B, sample.device)
        noise = self.draw_noise(sample.shape, sample.device) if self.ancestral else None
        out = ops.euler_step(sample.contiguous(), model_output.contiguous(), params, noise=noise,
                             ancestral=self.ancestral)
        self._step_index += 1
        return (out,)

    def device_step(self, latents, eps, params, noise=None, cfg=False):
        """The batched step of the native loops (native/pipe.py): one launch for all samples, per-sample rows in ``params``."""
        return ops.euler_step(latents, eps, params, noise=noise, cfg=cfg, ancestral=self.ancestral)


class NativeDDIMScheduler:
    """DDIM (eta = 0, epsilon prediction) as diffusers configures it for SD / SDXL: scaled-linear betas, leading spacing,
    steps_offset = 1, set_alpha_to_one = False, clip_sample = False.  Host side = the fp32 abar table built exactly as
    diffusers builds it (``torch.cumprod`` of fp32 alphas) and the per-step coefficients; the tensor work is
    ``lb_ddim_step_f16``.  Same interface as :class:`NativeEulerScheduler` (``step_row`` / ``device_step`` for the native loops,
    ``scale_model_input`` / ``step`` for the generic diffusers-style loop); ``scale_model_input`` is the identity and
    ``init_noise_sigma`` is 1.  Reached from /root/reference/latentblending/diffusers_holder.py:330,356 when a pipe carries
    this scheduler (``NativeSDXLPipe(scheduler="ddim")``); the reference's own SDXL pipes carry Euler schedulers (:42)."""
    order = 1
    kind = "ddim"
    ancestral = False
    init_noise_sigma = 1.0

    def __init__(self, device="cuda"):
        self.device = device
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, NUM_TRAIN_TIMESTEPS, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)            # fp32, as diffusers holds it
        self.final_alpha_cumprod = self.alphas_cumprod[0]                   # set_alpha_to_one = False
        self.noise_source = None
        self._step_index = None
        self.set_timesteps(30)

    def set_timesteps(self, num_inference_steps: int, device=None):
        n = int(num_inference_steps)
        ratio = NUM_TRAIN_TIMESTEPS // n
        ts = (np.arange(0, n) * ratio).round()[::-1].copy().astype(np.int64) + 1          # leading, steps_offset = 1
        self.timesteps_np = ts.astype(np.float32)
        self.timesteps = torch.from_numpy(self.timesteps_np)
        self.num_inference_steps = n
        self._ratio = ratio
        self._step_index = None

    def index_of(self, t) -> int:
        return int(np.nonzero(self.timesteps_np == float(t))[0][0])

    def alpha_pair(self, i: int):
        """(abar_t, abar_prev) of step ``i`` as 0-dim fp32 tensors (prev_timestep = t - 1000 // n; below 0: final_alpha_cumprod)."""
        t = int(self.timesteps_np[i])
        prev = t - self._ratio
        return self.alphas_cumprod[t], (self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod)

    def step_row(self, i: int, guidance: float = 0.0):
        """(0, sqrt(abar_t), sqrt(abar_prev), guidance, sqrt(1 - abar_t), sqrt(1 - abar_prev), 1 / sqrt(abar_t)) in fp32 tensor
        arithmetic, the scalars diffusers forms inside DDIMScheduler.step (beta_prod_t ** 0.5, alpha_prod_t ** 0.5, ...).  The last
        one is the fp32 reciprocal the device library forms when a tensor is divided by a 0-dim host tensor (its true-division
        kernel multiplies by ``1 / b`` for a CPU scalar ``b``): ``lb_ddim_step_f16`` multiplies by it instead of dividing."""
        a_t, a_p = self.alpha_pair(i)
        sa_t = a_t ** 0.5
        inv = torch.ones((), dtype=torch.float32) / sa_t.to(torch.float32)
        return (0.0, float(sa_t), float(a_p ** 0.5), guidance, float((1 - a_t) ** 0.5), float((1 - a_p) ** 0.5), float(inv))

    def _locate(self, t) -> int:
        if self._step_index is None:
            self._step_index = self.index_of(float(t))
        return self._step_index

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def draw_noise(self, shape, device) -> torch.Tensor:        # (never used: eta = 0)
        return torch.zeros(shape, device=device, dtype=torch.float16)

    def device_step(self, latents, eps, params, noise=None, cfg=False):
        return ops.ddim_step(latents, eps, params, cfg=cfg)

    def step(self, model_output, timestep, sample, generator=None, return_dict=False, **_):
        i = self._locate(timestep)
        params = ops.step_params([self.step_row(i)] * sample.shape[0], sample.device)
        out = ops.ddim_step(sample.contiguous(), model_output.contiguous(), params)
        self._step_index += 1
        return (out,)


LCM_ORIGINAL_STEPS = 50          # diffusers 0.25.0 LCMScheduler: original_inference_steps
LCM_TIMESTEP_SCALING = 10.0      # timestep_scaling
LCM_SIGMA_DATA = 0.5


def lcm_boundary_scalings(t: int) -> Tuple[float, float]:
    """(c_skip, c_out) of the consistency parameterisation at timestep ``t``, in Python floats as diffusers'
    ``get_scalings_for_boundary_condition_discrete`` forms them: s = 10 t, c_skip = 0.25 / (s^2 + 0.25), c_out = s / sqrt(s^2 + 0.25)."""
    s = t * LCM_TIMESTEP_SCALING
    sd2 = LCM_SIGMA_DATA ** 2
    return sd2 / (s ** 2 + sd2), s / (s ** 2 + sd2) ** 0.5


def noise_draws_per_run(sched, steps: int, idx_start: int) -> int:
    """Latent-shaped noise draws one denoising run from ``idx_start`` consumes under ``sched``: a scheduler that knows says so
    itself (``noise_draws``: LCM draws at every step but the schedule's last); an ancestral one draws once per step; others none."""
    own = getattr(sched, "noise_draws", None)
    if own is not None:
        return int(own(steps, idx_start))
    return max(0, int(steps) - int(idx_start)) if getattr(sched, "ancestral", False) else 0


class NativeLCMScheduler:
    """Latent-consistency multistep sampler (Luo et al. 2023, "Latent Consistency Models", algorithm 3) as diffusers 0.25.0's
    ``LCMScheduler`` configures it for SDXL: scaled-linear betas, original_inference_steps = 50, timestep_scaling = 10,
    sigma_data = 0.5, epsilon prediction, no thresholding / clipping.  Restated from the published algorithm and that class's
    documented behaviour - not checked against diffusers itself.  Host side = the fp32 abar table (as the DDIM class builds it),
    the timestep selection and the per-step coefficients; the tensor work is mode 2 of ``lb_euler_step_f16``.  Same interface as
    :class:`NativeDDIMScheduler`; ``scale_model_input`` is the identity and ``init_noise_sigma`` is 1.  Every step but the LAST
    of the schedule re-noises the denoised latent with one fresh fp16 draw (``noise_draws``)."""
    order = 1
    kind = "lcm"
    ancestral = False            # (not the Euler-ancestral update; whether noise is drawn is ``draws_noise`` / ``noise_draws``)
    draws_noise = True
    init_noise_sigma = 1.0

    def __init__(self, device="cuda"):
        self.device = device
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, NUM_TRAIN_TIMESTEPS, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)            # fp32, as diffusers holds it
        self.noise_source = None
        self._step_index = None
        self.set_timesteps(4)

    def set_timesteps(self, num_inference_steps: int, device=None):
        n = int(num_inference_steps)
        if n < 1 or n > LCM_ORIGINAL_STEPS:
            raise ValueError(f"NativeLCMScheduler: num_inference_steps must be in 1..{LCM_ORIGINAL_STEPS} (got {n})")
        origin = np.arange(1, LCM_ORIGINAL_STEPS + 1) * (NUM_TRAIN_TIMESTEPS // LCM_ORIGINAL_STEPS) - 1
        skip = LCM_ORIGINAL_STEPS // n
        ts = origin[::-1][::skip][:n].copy().astype(np.int64)
        self.timesteps_np = ts.astype(np.float32)
        self.timesteps = torch.from_numpy(self.timesteps_np)
        self.num_inference_steps = n
        self._step_index = None

    def index_of(self, t) -> int:
        return int(np.nonzero(self.timesteps_np == float(t))[0][0])

    def noise_draws(self, steps: int, idx_start: int) -> int:
        return max(0, int(steps) - int(idx_start) - 1)

    def is_last(self, i: int) -> bool:
        return i == self.num_inference_steps - 1

    def step_row(self, i: int, guidance: float = 0.0):
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

    def _locate(self, t) -> int:
        if self._step_index is None:
            self._step_index = self.index_of(float(t))
        return self._step_index

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    draw_noise = NativeEulerScheduler.draw_noise
    draw_noise_many = NativeEulerScheduler.draw_noise_many

    def device_step(self, latents, eps, params, noise=None, cfg=False, last: Optional[bool] = None):
        """``last``: the loop's statement that this is the schedule's last step for every sample of the batch (``params`` is
        usually a view of one upload of all steps' rows, which carries no host mirror) - only then may ``noise`` be None."""
        return ops.lcm_step(latents, eps, params, noise=noise, cfg=cfg, all_last=last)

    def step(self, model_output, timestep, sample, generator=None, return_dict=False, **_):
        i = self._locate(timestep)
        params = ops.step_params([self.step_row(i)] * sample.shape[0], sample.device)
        noise = None if self.is_last(i) else self.draw_noise(sample.shape, sample.device)
        out = ops.lcm_step(sample.contiguous(), model_output.contiguous(), params, noise=noise)
        self._step_index += 1
        return (out,)


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


class NativeDPMSolverPP2MScheduler:
    """DPM-Solver++ 2M (Lu et al. 2022, "DPM-Solver++", algorithm 2: second-order multistep, data prediction) in the form diffusers'
    ``DPMSolverMultistepScheduler`` takes with algorithm_type "dpmsolver++", solver_type "midpoint", final_sigmas_type "zero" and
    epsilon prediction, over uniform ("leading", steps_offset 1) or Karras (Karras et al. 2022, eq. 5, rho = 7) sigmas - what user
    interfaces call "DPM++ 2M" / "DPM++ 2M Karras".  Restated from the paper and that class's documented behaviour - not checked
    against diffusers itself.  Host side = the float64 sigma table (``_sigma_table``, as for Euler), the schedule and the per-step
    coefficients, each rounded ONCE to fp32 on upload; the tensor work is bit 1 of ``cfg`` of ``lb_ddim_step_f16``.  Same interface
    as :class:`NativeDDIMScheduler`, except that the sampler has a history: ``device_step`` takes and returns a two-plane state
    (latents, previous x0 prediction), and ``step_row`` takes ``first`` - the first step a sample executes has no history and is
    first order, like the schedule's last step (whose target sigma is 0).  The reference's restartable loop calls
    ``set_timesteps`` at the start of every run, which empties a multistep scheduler's history: a branch entering at
    ``idx_start > 0`` starts first order too."""
    order = 1                    # model evaluations per step (as diffusers reports it; the engine's loops read this)
    solver_order = 2
    kind = "dpmpp_2m"
    multistep = True
    ancestral = False
    init_noise_sigma = 1.0

    def __init__(self, use_karras_sigmas: bool = False, device="cuda"):
        self.use_karras_sigmas = bool(use_karras_sigmas)
        self.device = device
        self._table = _sigma_table()
        self.noise_source = None
        self._step_index = None
        self._m1 = None
        self.set_timesteps(20)

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
        self.timesteps_np = ts.astype(np.float32)
        self.timesteps = torch.from_numpy(self.timesteps_np)
        self.sigmas = torch.from_numpy(self.sigmas_np.astype(np.float32))
        self.num_inference_steps = n
        self._step_index = None
        self._m1 = None

    def index_of(self, t) -> int:
        return int(np.nonzero(self.timesteps_np == float(t))[0][0])

    def noise_draws(self, steps: int, idx_start: int) -> int:
        return 0

    def is_last(self, i: int) -> bool:
        return i == self.num_inference_steps - 1

    def step_row(self, i: int, guidance: float = 0.0, first: bool = False):
        """The row of step ``i`` (``dpmpp_2m_row`` over this schedule's sigmas).  ``first`` = the sample has no history at this
        step - the first step it executes: a first-order row."""
        return dpmpp_2m_row(self.sigmas_np, i, guidance, first)

    # ---- diffusers-style tensor API (generic holder loop / foreign callers) ------------------
    def _locate(self, t) -> int:
        if self._step_index is None:
            self._step_index = self.index_of(float(t))
        return self._step_index

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def draw_noise(self, shape, device) -> torch.Tensor:        # (never used: the solver is deterministic)
        return torch.zeros(shape, device=device, dtype=torch.float16)

    def device_step(self, state, eps, params, noise=None, cfg=False, out=None):
        """The batched step of the native loops: ``state`` [2, B, ...] (latents, previous x0 prediction) -> the next state."""
        return ops.dpmpp2m_step(state, eps, params, cfg=cfg, out=out)

    def step(self, model_output, timestep, sample, generator=None, return_dict=False, **_):
        """One step with the history kept HERE (``_m1``, the previous call's x0 prediction; ``set_timesteps`` drops it)."""
        i = self._locate(timestep)
        first = self._m1 is None
        params = ops.step_params([self.step_row(i, first=first)] * sample.shape[0], sample.device)
        state = torch.empty((2,) + tuple(sample.shape), dtype=torch.float16, device=sample.device)
        state[0].copy_(sample)
        if not first:
            state[1].copy_(self._m1)
        out = ops.dpmpp2m_step(state, model_output.contiguous(), params)
        self._m1 = out[1]
        self._step_index += 1
        return (out[0],)
