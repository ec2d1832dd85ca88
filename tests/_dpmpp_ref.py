"""Reference for the DPM-Solver++ 2M sampler (test infrastructure, torch on the CPU).

The sampler restates the published algorithm (Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion
Probabilistic Models", algorithm 2: multistep, second order, data prediction) in the form diffusers'
``DPMSolverMultistepScheduler`` takes with ``algorithm_type="dpmsolver++"``, ``solver_type="midpoint"``,
``final_sigmas_type="zero"`` and epsilon prediction, over scaled-linear betas 0.00085 .. 0.012 (1000 steps) with uniform
("leading", steps_offset 1) or Karras (Karras et al. 2022, eq. 5, rho = 7) sigmas.  It is NOT checked against diffusers itself
(none is installed).  Three things live here:

* ``dpmpp_step_f16``     - one step on fp16 tensors, the op-by-op expression the device kernel restates: every tensor operation
  computes in fp32 with the fp32 value of its scalar coefficient and rounds its result to fp16.  (Written as
  ``(a.float() * c).half()`` with a Python float ``c`` rather than ``a * c`` on fp16 CPU tensors: torch's CPU kernels round the
  scalar itself to fp16 first, which no GPU pipeline does - the reason ``tests/_lcm_ref.py`` is written this way.)
* ``row_f64`` / ``sigmas_f64`` / ``timesteps_of`` - the schedule and the coefficients as float64 closed forms.
* ``DPMPPRefScheduler`` - the diffusers-style tensor API (``set_timesteps`` / ``scale_model_input`` / ``step`` / ``timesteps`` /
  ``init_noise_sigma`` / ``order``) for the oracle pipe under the generic loop.  Its history (the previous x0 prediction) is
  dropped by ``set_timesteps``, which the loop calls at the start of every run.
"""
import math

import numpy as np
import torch

F16 = torch.float16
RHO = 7.0


def sigma_table_f64() -> np.ndarray:
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    abar = np.cumprod(1.0 - betas)
    return np.sqrt((1.0 - abar) / abar)


def sigmas_f64(n: int, karras: bool) -> np.ndarray:
    """n sigmas, largest first, and a final 0."""
    table = sigma_table_f64()
    if karras:
        lo, hi = table[0] ** (1 / RHO), table[999] ** (1 / RHO)
        sig = [table[999] if k == 0 else table[0] if k == n - 1 else (hi + k / (n - 1) * (lo - hi)) ** RHO for k in range(n)]
    else:
        sig = [table[k * (1000 // n) + 1] for k in range(n - 1, -1, -1)]
    return np.array(list(sig) + [0.0], dtype=np.float64)


def timesteps_of(sigmas) -> list:
    """The integer timestep of each non-zero sigma: linear interpolation in log sigma over the table, rounded (half to even)."""
    logt = np.log(sigma_table_f64())
    out = []
    for s in sigmas:
        if s == 0:
            continue
        ls = math.log(s)
        k = int(np.searchsorted(logt, ls, side="right")) - 1
        k = min(max(k, 0), 998)
        w = min(max((ls - logt[k]) / (logt[k + 1] - logt[k]), 0.0), 1.0)
        out.append(int(round(k + w)))
    return out


def row_f64(sigmas, i: int, guidance: float = 0.0, first: bool = False):
    """{0, sigma'_i, ratio, guidance, c0, c1, 1 / alpha_i, 1 / r0} in float64.  alpha = 1 / sqrt(sigma^2 + 1), sigma' = sigma alpha,
    lambda = log(alpha / sigma').  The step onto sigma 0, step 0 and a ``first`` step are first order (c1 = 0)."""
    al = lambda s: 1.0 / math.sqrt(s * s + 1.0)                                # noqa: E731
    lam = lambda s: math.log(al(s) / (s * al(s)))                              # noqa: E731
    s0, s1 = float(sigmas[i]), float(sigmas[i + 1])
    if s1 == 0.0:
        return [0.0, s0 * al(s0), 0.0, float(guidance), -1.0, 0.0, 1.0 / al(s0), 0.0]
    h = lam(s1) - lam(s0)
    c0 = al(s1) * math.expm1(-h)
    ratio = (s1 * al(s1)) / (s0 * al(s0))
    if first or i == 0:
        return [0.0, s0 * al(s0), ratio, float(guidance), c0, 0.0, 1.0 / al(s0), 0.0]
    r0 = (lam(s0) - lam(float(sigmas[i - 1]))) / h
    return [0.0, s0 * al(s0), ratio, float(guidance), c0, 0.5 * c0, 1.0 / al(s0), 1.0 / r0]


def f32(v) -> float:
    """A row scalar as the kernel sees it: rounded once to fp32."""
    return float(np.float32(v))


def cfg_combine_f16(eps_uncond, eps_text, guidance: float):
    """``eps_uncond + guidance * (eps_text - eps_uncond)`` on fp16 tensors: sub, scalar mul, add, each rounded to fp16."""
    g = f32(guidance)
    diff = (eps_text.float() - eps_uncond.float()).to(F16)
    sc = (diff.float() * g).to(F16)
    return (eps_uncond.float() + sc.float()).to(F16)


def dpmpp_step_f16(row, x, e, m1):
    """(next latent, m0) on fp16 tensors; ``row`` as ``row_f64`` gives it (rounded to fp32 here).  ``m1`` is not touched on a
    first-order row (c1 == 0)."""
    _, sig, ratio, _, c0, c1, inv_alpha, inv_r0 = [f32(v) for v in row]
    assert x.dtype == F16 and e.dtype == F16
    t1 = (e.float() * sig).to(F16)
    t2 = (x.float() - t1.float()).to(F16)
    m0 = (t2.float() * inv_alpha).to(F16)
    a = (x.float() * ratio).to(F16)
    b = (m0.float() * c0).to(F16)
    y = (a.float() - b.float()).to(F16)
    if c1 != 0.0:
        dm = (m0.float() - m1.float()).to(F16)
        d1 = (dm.float() * inv_r0).to(F16)
        c = (d1.float() * c1).to(F16)
        y = (y.float() - c.float()).to(F16)
    return y, m0


def dpmpp_step_f64(row, x, e, m1):
    """The same step in float64 (tensors or numpy / Python scalars)."""
    _, sig, ratio, _, c0, c1, inv_alpha, inv_r0 = row
    m0 = (x - sig * e) * inv_alpha
    y = ratio * x - c0 * m0
    if c1 != 0.0:
        y = y - c1 * (inv_r0 * (m0 - m1))
    return y, m0


class DPMPPRefScheduler:
    order = 1
    solver_order = 2
    init_noise_sigma = 1.0
    ancestral = False

    def __init__(self, use_karras_sigmas: bool = False, noise_source=None):
        self.karras = bool(use_karras_sigmas)
        self.noise_source = noise_source            # (unused: the solver draws nothing)
        self.set_timesteps(20)

    def set_timesteps(self, n, device=None):
        self.num_inference_steps = int(n)
        self.sigmas_f64 = sigmas_f64(int(n), self.karras)
        ts = timesteps_of(self.sigmas_f64)
        assert all(a > b for a, b in zip(ts[:-1], ts[1:])), "timesteps must be strictly decreasing"
        self.timesteps = torch.tensor(ts, dtype=torch.int64)
        self.m1 = None                              # every run starts without history

    def scale_model_input(self, sample, t=None):
        return sample

    def step(self, model_output, t, sample, generator=None, return_dict=False, **_):
        i = int((self.timesteps == int(t)).nonzero()[0])
        row = row_f64(self.sigmas_f64, i, first=self.m1 is None)
        if sample.dtype == F16:
            y, m0 = dpmpp_step_f16(row, sample, model_output.to(F16), self.m1)
        else:
            y, m0 = dpmpp_step_f64(row, sample, model_output.to(sample.dtype), self.m1)
        self.m1 = m0
        return (y,)
