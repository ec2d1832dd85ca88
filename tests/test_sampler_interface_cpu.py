"""The native samplers' one interface (``NativeScheduler``, ``make_scheduler``) and the one home of the noise-accounting rule
(``planner.noise_draws_per_run``).  ``tests/golden/sampler_rows.json`` was recorded by ``sampler_tables`` below from the commit
BEFORE the samplers got their common base class: every schedule, every step row and every noise count is compared for equality
(floats as ``float.hex()``), so moving the code moved no bit."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import pipe as OP
from oracle import sdxl_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dpmpp_ref as DR  # noqa: E402
import _lcm_ref as LR  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_rows.json")
STEPS = (1, 4, 5, 20, 30)
# sampler -> (class, constructor arguments, step counts); the pipe's name and ``turbo`` that select it are in NAMES below
SAMPLERS = {
    "euler": ("NativeEulerScheduler", {"ancestral": False}, STEPS),
    "euler_ancestral": ("NativeEulerScheduler", {"ancestral": True}, STEPS),
    "ddim": ("NativeDDIMScheduler", {}, STEPS),
    "lcm": ("NativeLCMScheduler", {}, STEPS + (2, 8, 50)),
    "dpmpp_2m": ("NativeDPMSolverPP2MScheduler", {"use_karras_sigmas": False}, STEPS),
    "dpmpp_2m_karras": ("NativeDPMSolverPP2MScheduler", {"use_karras_sigmas": True}, STEPS),       # (Karras sigmas: at most 44)
}
NAMES = {"euler": ("euler", False), "euler_ancestral": ("euler", True), "ddim": ("ddim", True), "lcm": ("lcm", False),
         "dpmpp_2m": ("dpmpp_2m", True), "dpmpp_2m_karras": ("dpmpp_2m_karras", False)}


def _hex(values):
    return [float(v).hex() for v in values]


def sampler_tables(S) -> dict:
    """Everything the native loops read from the samplers of scheduler module ``S``, as JSON: per sampler and step count the
    timesteps, ``init_noise_sigma``, the sigmas where the class has them, every ``step_row(i, 2.5)`` (DPM-Solver: also with
    ``first=True``) and ``noise_draws_per_run`` from every start index.  Uses only what the module offered before the common
    base class, so the same function recorded the fixture."""
    out = {}
    for key, (cls, kwargs, counts) in SAMPLERS.items():
        sched = getattr(S, cls)(device="cpu", **kwargs)
        for n in counts:
            sched.set_timesteps(n)
            e = {"timesteps": _hex(sched.timesteps_np), "init_noise_sigma": float(sched.init_noise_sigma).hex(),
                 "rows": [_hex(sched.step_row(i, 2.5)) for i in range(n)],
                 "noise_draws": [S.noise_draws_per_run(sched, n, k) for k in range(n + 1)]}
            if hasattr(sched, "sigmas_np"):
                e["sigmas"] = _hex(sched.sigmas_np)
            if key.startswith("dpmpp"):
                e["rows_first"] = [_hex(sched.step_row(i, 2.5, first=True)) for i in range(n)]
            out[f"{key}/{n}"] = e
    return out


@pytest.fixture(scope="module")
def S():
    from latentblending_amd.native import scheduler
    return scheduler


def test_every_schedule_row_and_noise_count_equals_the_parent_commits(S):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = sampler_tables(S)
    assert sorted(got) == sorted(want) and len(want) == 6 * len(STEPS) + 3
    for case in want:
        assert sorted(got[case]) == sorted(want[case]), case
        for field in want[case]:
            assert got[case][field] == want[case][field], (case, field)


def _make(S, key):
    name, turbo = NAMES[key]
    return S.make_scheduler(name, turbo, "cpu")


@pytest.mark.parametrize("key", sorted(SAMPLERS))
def test_every_sampler_answers_the_whole_interface(S, key):
    s = _make(S, key)
    assert isinstance(s, S.NativeScheduler) and issubclass(getattr(S, SAMPLERS[key][0]), S.NativeScheduler)
    n = 5
    s.set_timesteps(n)
    assert s.multistep is key.startswith("dpmpp")
    assert bool(s.draws_noise) is (key in ("euler_ancestral", "lcm"))
    assert [s.is_last(i) for i in range(n)] == [False] * (n - 1) + [True]
    want_draws = {"euler_ancestral": lambda k: n - k, "lcm": lambda k: max(0, n - k - 1)}.get(key, lambda k: 0)
    assert [s.noise_draws(n, k) for k in range(n + 1)] == [want_draws(k) for k in range(n + 1)]
    for i in range(n):
        assert s.device_step_kwargs(i) == ({"last": i == n - 1} if key == "lcm" else {})
        if not s.multistep:         # a single-step sampler has no history: ``first`` changes nothing
            assert s.step_row(i, 2.5, first=True) == s.step_row(i, 2.5, first=False) == s.step_row(i, 2.5)
    if s.multistep:
        assert s.step_row(2, 2.5, first=True) != s.step_row(2, 2.5) and s.step_row(0, 2.5, first=True) == s.step_row(0, 2.5)
    x = np.zeros(1)
    assert key.startswith("euler") or s.scale_model_input(x, s.timesteps[0]) is x


def test_make_scheduler_maps_each_name_as_the_pipe_constructor_did(S):
    assert S.SCHEDULER_NAMES == ("euler", "ddim", "lcm", "dpmpp_2m", "dpmpp_2m_karras")
    classes = {"euler": S.NativeEulerScheduler, "ddim": S.NativeDDIMScheduler, "lcm": S.NativeLCMScheduler,
               "dpmpp_2m": S.NativeDPMSolverPP2MScheduler, "dpmpp_2m_karras": S.NativeDPMSolverPP2MScheduler}
    for name in S.SCHEDULER_NAMES + (None,):
        for turbo in (False, True):
            for spelt in ([None] if name is None else [name, name.upper(), f"  {name.title()}\t"]):
                s = S.make_scheduler(spelt, turbo, "cpu")
                assert type(s) is classes[name or "euler"] and s.device == "cpu" and s.noise_source is None
                assert s.ancestral is (turbo and name in (None, "euler"))
                assert getattr(s, "use_karras_sigmas", None) == {"dpmpp_2m": False, "dpmpp_2m_karras": True}.get(name)
                assert s.kind == {None: "euler", "dpmpp_2m_karras": "dpmpp_2m"}.get(name, name)
    accepted = "'euler', 'ddim' or 'lcm'; also 'dpmpp_2m', 'dpmpp_2m_karras'"
    for bad in ("dpm", "euler_a", "dpmpp_2m karras", ""):
        with pytest.raises(ValueError) as err:
            S.make_scheduler(bad, True, "cpu")
        assert str(err.value) == f"NativeSDXLPipe: unknown scheduler {bad!r} (None, {accepted})"
    with pytest.raises(ValueError) as err:
        S.make_scheduler(S.NativeDDIMScheduler(device="cpu"), True, "cpu")
    assert str(err.value) == f"NativeSDXLPipe: scheduler must be None, {accepted} (got an object of type NativeDDIMScheduler)"


def test_the_engine_counts_noise_by_the_planners_rule(S):
    from latentblending_amd import BlendingEngine, planner
    assert S.noise_draws_per_run is planner.noise_draws_per_run
    refs = {"oracle euler-ancestral": lambda p: p.scheduler, "oracle euler": lambda p: R.EulerScheduler(ancestral=False, noise_source=p.noise),
            "lcm reference": lambda p: LR.LCMRefScheduler(noise_source=p.noise), "dpmpp reference": lambda p: DR.DPMPPRefScheduler(use_karras_sigmas=True)}
    for what, sched_of in refs.items():
        p = OP.StableDiffusionXLPipeline(turbo=True, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg())
        p.scheduler = sched_of(p)
        be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False)
        be.set_num_inference_steps(4)
        want = {"oracle euler-ancestral": [4, 3, 2, 1, 0], "lcm reference": [3, 2, 1, 0, 0]}.get(what, [0] * 5)
        assert [be._run_noise_draws(k) for k in range(5)] == [planner.noise_draws_per_run(p.scheduler, 4, k) for k in range(5)] == want, what
        assert be._draws_noise(p.scheduler) is planner.draws_noise(p.scheduler) is (want[0] > 0), what
