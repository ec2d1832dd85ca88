"""References for the latent-consistency sampler and the guidance-scale embedding (test infrastructure, torch on the CPU).

The sampler restates the published algorithm (Luo et al. 2023, "Latent Consistency Models": multistep consistency sampling) as
diffusers 0.25.0's ``LCMScheduler`` configures it for SDXL - scaled-linear betas 0.00085 .. 0.012 over 1000 steps,
``original_inference_steps = 50``, ``timestep_scaling = 10``, ``sigma_data = 0.5``, epsilon prediction, no clipping - and is NOT
checked against diffusers itself (none is installed).  Three things live here:

* ``LCMRefScheduler``  - the diffusers-style tensor API (``set_timesteps`` / ``scale_model_input`` / ``step``).  On fp16 tensors
  its step is the op-by-op expression the device kernel restates: every tensor operation computes in fp32 with the fp32 value of
  its scalar coefficient and rounds its result to fp16.  (Written as ``(a.float() op c).half()`` rather than ``a op c`` on fp16
  CPU tensors: torch's CPU kernels round the scalar itself to fp16 first, which no GPU pipeline does - the same reason
  ``oracle/sdxl_ref.py``'s DDIM step is written this way.)
* ``lcm_step_f64`` / ``lcm_row_f64`` - the same step and its coefficients as float64 closed forms.
* ``guidance_embedding_f64`` - the guidance-scale embedding in float64.
"""
import math

import numpy as np
import torch

ORIGINAL_STEPS = 50
TIMESTEP_SCALING = 10.0
SIGMA_DATA = 0.5
F16 = torch.float16


def abar_f64() -> np.ndarray:
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas)


def lcm_timesteps(n: int):
    if n < 1 or n > ORIGINAL_STEPS:
        raise ValueError(f"LCM: 1 <= num_inference_steps <= {ORIGINAL_STEPS} (got {n})")
    origin = [k * (1000 // ORIGINAL_STEPS) - 1 for k in range(1, ORIGINAL_STEPS + 1)]
    return origin[::-1][::ORIGINAL_STEPS // n][:n]


def boundary_scalings(t: int):
    """(c_skip, c_out) in Python floats."""
    s = t * TIMESTEP_SCALING
    return SIGMA_DATA ** 2 / (s ** 2 + SIGMA_DATA ** 2), s / (s ** 2 + SIGMA_DATA ** 2) ** 0.5


def lcm_row_f64(n: int, i: int, guidance: float = 0.0, abar=None):
    """The parameter row of step ``i`` of an ``n``-step schedule in float64: {0, c_skip, sqrt(abar_prev), guidance, sqrt(1 - abar_t),
    sqrt(1 - abar_prev), 1 / sqrt(abar_t), c_out}; the last step has no previous timestep (slots 2 and 5 are 0).  ``abar``: the table
    to read (default: the float64 one)."""
    abar = abar_f64() if abar is None else abar
    ts = lcm_timesteps(n)
    a_t = float(abar[ts[i]])
    c_skip, c_out = boundary_scalings(ts[i])
    if i + 1 < n:
        a_p = float(abar[ts[i + 1]])
        sa_p, sb_p = a_p ** 0.5, (1 - a_p) ** 0.5
    else:
        sa_p = sb_p = 0.0
    return [0.0, c_skip, sa_p, float(guidance), (1 - a_t) ** 0.5, sb_p, 1.0 / a_t ** 0.5, c_out]


def lcm_step_f64(x, eps, noise, abar_t: float, abar_prev, t: int):
    """One step in float64: (prev_sample, denoised).  ``abar_prev`` None = the schedule's last step (prev_sample is denoised)."""
    x, eps = x.double(), eps.double()
    c_skip, c_out = boundary_scalings(t)
    x0 = (x - (1 - abar_t) ** 0.5 * eps) / abar_t ** 0.5
    den = c_out * x0 + c_skip * x
    if abar_prev is None:
        return den, den
    return abar_prev ** 0.5 * den + (1 - abar_prev) ** 0.5 * noise.double(), den


def cfg_combine_f16(eps_uncond, eps_text, guidance: float):
    """``eps_uncond + guidance * (eps_text - eps_uncond)`` on fp16 tensors: sub, scalar mul, add, each rounded to fp16."""
    rt = lambda v: v.to(F16).float()                                          # noqa: E731
    g = float(np.float32(guidance))
    diff = rt(eps_text.float() - eps_uncond.float())
    return rt(eps_uncond.float() + rt(g * diff)).to(F16)


def guidance_embedding_f64(w, dim: int) -> np.ndarray:
    """[len(w), dim]: [sin(1000 w f) | cos(1000 w f)], f_i = exp(-i ln(10000) / (dim // 2 - 1)); one zero column pads an odd dim."""
    w = np.asarray(w, dtype=np.float64).reshape(-1) * 1000.0
    half = dim // 2
    f = np.exp(-np.arange(half, dtype=np.float64) * math.log(10000.0) / (half - 1))
    ang = w[:, None] * f[None, :]
    out = np.concatenate([np.sin(ang), np.cos(ang)], axis=1)
    if dim % 2:
        out = np.concatenate([out, np.zeros((len(w), 1))], axis=1)
    return out


class LCMRefScheduler:
    order = 1
    init_noise_sigma = 1.0
    ancestral = False
    draws_noise = True          # (the engine's noise accounting: a sampler that consumes per-step noise ...)

    def __init__(self, noise_source=None):
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.noise_source = noise_source
        self.set_timesteps(4)

    def noise_draws(self, steps: int, idx_start: int) -> int:      # (... and how much of it one run from idx_start takes)
        return max(0, int(steps) - int(idx_start) - 1)

    def set_timesteps(self, n, device=None):
        self.num_inference_steps = int(n)
        self.timesteps = torch.tensor(lcm_timesteps(int(n)), dtype=torch.int64)

    def scale_model_input(self, sample, t=None):
        return sample

    def coefficients(self, i: int):
        """fp32 values as Python floats: (c_skip, c_out, sqrt(1 - abar_t), 1 / sqrt(abar_t), sqrt(abar_prev), sqrt(1 - abar_prev));
        the last two are None on the schedule's last step.  Roots and reciprocal are 0-dim fp32 tensor operations."""
        t = int(self.timesteps[i])
        a_t = self.alphas_cumprod[t]
        c_skip, c_out = boundary_scalings(t)
        f32 = lambda v: float(np.float32(v))                                  # noqa: E731  (a Python-float scalar reaches a device kernel as fp32)
        inv = float(torch.ones((), dtype=torch.float32) / (a_t ** 0.5))
        if i + 1 < self.num_inference_steps:
            a_p = self.alphas_cumprod[int(self.timesteps[i + 1])]
            sa_p, sb_p = float(a_p ** 0.5), float((1 - a_p) ** 0.5)
        else:
            sa_p = sb_p = None
        return f32(c_skip), f32(c_out), float((1 - a_t) ** 0.5), inv, sa_p, sb_p

    def denoised(self, i: int, model_output, sample):
        """The consistency model's output at step ``i``: c_out x0 + c_skip x (six roundings on fp16 tensors)."""
        c_skip, c_out, sb_t, inv, _, _ = self.coefficients(i)
        if sample.dtype != F16:
            x0 = (sample - sb_t * model_output) * inv
            return c_out * x0 + c_skip * sample
        rt = lambda v: v.to(F16).float()                                      # noqa: E731
        x, e = sample.float(), model_output.float()
        t1 = rt(sb_t * e)
        t2 = rt(x - t1)
        x0 = rt(t2 * inv)
        d1 = rt(c_out * x0)
        d2 = rt(c_skip * x)
        return rt(d1 + d2).to(F16)

    def denoise_and_renoise(self, i: int, model_output, sample, noise):
        """prev_sample of step ``i``: the denoised latent itself on the schedule's last step (``noise`` is not touched), else
        sqrt(abar_prev) denoised + sqrt(1 - abar_prev) noise (three more roundings on fp16 tensors)."""
        den = self.denoised(i, model_output, sample)
        _, _, _, _, sa_p, sb_p = self.coefficients(i)
        if sa_p is None:
            return den
        if sample.dtype != F16:
            return sa_p * den + sb_p * noise.to(sample.dtype)
        rt = lambda v: v.to(F16).float()                                      # noqa: E731
        a = rt(sa_p * den.float())
        b = rt(sb_p * noise.float())
        return rt(a + b).to(F16)

    def step(self, model_output, t, sample, generator=None, return_dict=False, **_):
        i = int((self.timesteps == int(t)).nonzero()[0])
        noise = None
        if i + 1 < self.num_inference_steps:
            if self.noise_source is not None:
                noise = self.noise_source(tuple(model_output.shape)).to(model_output.dtype)
            else:
                noise = torch.randn(model_output.shape, dtype=model_output.dtype, generator=generator)
        return (self.denoise_and_renoise(i, model_output, sample, noise),)
