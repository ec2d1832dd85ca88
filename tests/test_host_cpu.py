"""CPU-only tests (`-m "not gpu"`): the oracle against the golden vectors frozen from the unchanged
reference, the host logic (planner / tree / engine / holder) against the same vectors, the C-ABI
export surface, and fail-loud behaviour.  No kernel is launched here.
"""
import ctypes
import dataclasses
import json
import os
import re

import zlib

import numpy as np
import pytest
import torch

from oracle import pipe as OP
from oracle import ref_harness as H
from oracle import sdxl_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def gold(name):
    with open(os.path.join(GOLD, name + ".json")) as fh:
        return json.load(fh)


def seeded(n, seed, dtype=torch.float16, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(dtype)


DT = {"torch.float16": torch.float16, "torch.float32": torch.float32, "torch.float64": torch.float64}


@pytest.fixture()
def cpu_backend():
    from latentblending_amd.backend import set_backend
    set_backend(R.TorchCpuBackend())
    yield
    set_backend(None)


def check_against_golden_run(be, imgs, c, rtol=2e-3):
    """Numeric comparison with a frozen reference run (CPU summation order varies with thread count
    and ISA, so hashes are informational only)."""
    assert np.allclose([float(s) for s in be.tree_similarities], c["tree_similarities"], rtol=rtol)
    for lat, head, norm in zip(be.tree_latents, c["final_latent_head"], c["final_latent_norm"]):
        z = lat[-1].float().flatten()
        assert abs(float(z.norm()) - norm) <= rtol * norm
        assert np.allclose(z[:24].numpy(), head, rtol=5e-3, atol=5e-3 * norm / z.numel() ** 0.5)
    for img, mean, head in zip(imgs, c["frame_mean"], c["frame_head"]):
        a = np.asarray(img)
        assert abs(float(a.mean()) - mean) <= 0.25
        assert np.abs(a.flatten()[:24].astype(int) - np.array(head)).max() <= 2


def tiny_pipe(turbo=True):
    return OP.StableDiffusionXLPipeline(turbo=turbo, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg())


# ---------------------------------------------------------------- oracle pinned by the reference
def test_oracle_slerp_matches_reference_golden():
    for c in gold("slerp")["slerp"]:
        dt = DT[c["in_dtype"]]
        if c["name"] == "identical":
            p0 = seeded(c["n"], c["seed0"]); p1 = p0.clone()
        elif c["name"] == "antipodal":
            p0 = seeded(c["n"], c["seed0"]); p1 = -p0
        elif c["name"] == "zero_norm":
            p0 = torch.zeros(c["n"], dtype=torch.float16); p1 = seeded(c["n"], c["seed0"])
        else:
            p0, p1 = seeded(c["n"], c["seed0"], dt, c["scale"]), seeded(c["n"], c["seed1"], dt, c["scale"])
        out = R.slerp(p0, p1, c["fract"])
        assert str(out.dtype) == c["out_dtype"], c["name"]
        if c["nan"]:
            assert torch.isnan(out).all()
        elif out.dtype == torch.float16:
            assert out.view(torch.int16).tolist() == c["out_bits"], (c["name"], c["fract"])
        else:
            assert out.tolist() == c["out_f32"], c["name"]


def test_oracle_lerp_matches_reference_golden():
    from latentblending_amd.utils import interpolate_linear
    for c in gold("slerp")["lerp"]:
        if c.get("uint8"):
            a = np.array(c["a"], dtype=np.uint8).reshape(4, 4, 3)
            b = np.array(c["b"], dtype=np.uint8).reshape(4, 4, 3)
            assert interpolate_linear(a, b, c["fract"]).flatten().tolist() == c["out"]   # host path of utils
            continue
        x, y = seeded(c["n"], c["seed0"]), seeded(c["n"], c["seed1"])
        assert R.lerp(x, y, c["fract"]).view(torch.int16).tolist() == c["out_bits"]


def test_scheduler_tables_match_closed_form():
    g = gold("scheduler")
    for make in (lambda a: R.EulerScheduler(ancestral=a),):
        s = make(True); s.set_timesteps(4)
        assert s.timesteps.tolist() == g["trailing4_timesteps"]
        assert np.allclose(s.sigmas.numpy(), g["trailing4_sigmas"], atol=2e-5)
        assert abs(s.init_noise_sigma - g["sigma_999"]) < 1e-4
        for i, (up, down) in enumerate(g["trailing4_ancestral"]):
            u, d = R.ancestral_sigmas(float(s.sigmas[i]), float(s.sigmas[i + 1]))
            assert abs(u - up) < 2e-5 and abs(d - down) < 2e-5
        s = make(False); s.set_timesteps(30)
        assert int(s.timesteps[0]) == g["leading30_first"] and int(s.timesteps[-1]) == g["leading30_last"]
        assert abs(float(s.sigmas[0]) - g["leading30_sigma0"]) < 2e-4
        assert abs(s.init_noise_sigma - g["leading30_init_noise_sigma"]) < 2e-4


def test_ddim_tables_and_step_match_closed_form():
    """DDIM (north_star: "the Euler/DDIM step"): the abar table and leading-spaced timesteps of the oracle restatement against
    float64 closed-form known answers (tests/golden/scheduler.json), the native host scheduler equal to the oracle's, and the
    oracle's step against the DDIM paper's formula evaluated in float64."""
    from latentblending_amd.native.scheduler import NativeDDIMScheduler
    g = gold("scheduler")
    o, n = R.DDIMScheduler(), NativeDDIMScheduler(device="cpu")
    for t, want in g["ddim_alphas_cumprod"].items():
        assert abs(float(o.alphas_cumprod[int(t)]) - want) <= 2e-6 * want          # (fp32 cumprod of 1000 factors)
    assert abs(float(o.final_alpha_cumprod) - g["ddim_final_alpha_cumprod"]) < 1e-7
    for k in (30, 6, 50, 4):
        o.set_timesteps(k); n.set_timesteps(k)
        assert o.timesteps.tolist() == [int(t) for t in n.timesteps.tolist()]
    o.set_timesteps(30); n.set_timesteps(30)
    assert o.timesteps[:4].tolist() == g["ddim_leading30_timesteps_head"] and o.timesteps[-3:].tolist() == g["ddim_leading30_timesteps_tail"]
    assert torch.equal(o.alphas_cumprod, n.alphas_cumprod) and n.init_noise_sigma == 1.0
    x, e = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(5)), torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(6))
    assert n.scale_model_input(x, 958) is x
    for i in (0, 7, 29):                                    # (29: prev_timestep < 0 -> final_alpha_cumprod)
        t = int(o.timesteps[i])
        a_t, a_p = n.alpha_pair(i)
        prev = t - 1000 // 30
        assert float(a_t) == float(o.alphas_cumprod[t]) and float(a_p) == float(o.alphas_cumprod[prev] if prev >= 0 else o.final_alpha_cumprod)
        row = n.step_row(i, 2.5)
        at, ap = float(a_t), float(a_p)
        assert row[0] == 0.0 and row[3] == 2.5 and np.allclose(row[1:3] + row[4:6], [at ** 0.5, ap ** 0.5, (1 - at) ** 0.5, (1 - ap) ** 0.5], rtol=1e-6)
        assert row[6] == float(np.float32(1.0) / np.float32(row[1]))       # the fp32 reciprocal the step multiplies by (host-scalar division)
        got = o.step(e, t, x)[0].double()
        want = ap ** 0.5 * (x.double() - (1 - at) ** 0.5 * e.double()) / at ** 0.5 + (1 - ap) ** 0.5 * e.double()
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)


def test_native_scheduler_tables_equal_oracle():
    from latentblending_amd.native.scheduler import NativeEulerScheduler
    for anc, n in [(True, 4), (True, 2), (False, 30), (False, 6), (False, 50)]:
        a, b = NativeEulerScheduler(anc, device="cpu"), R.EulerScheduler(anc)
        a.set_timesteps(n); b.set_timesteps(n)
        assert a.timesteps.tolist() == b.timesteps.tolist()
        assert a.sigmas.tolist() == b.sigmas.tolist()
        assert a.init_noise_sigma == b.init_noise_sigma
        for i in range(n):
            row = a.step_row(i, 2.5)
            s_from, s_to = float(b.sigmas[i]), float(b.sigmas[i + 1])
            if anc:
                up, down = R.ancestral_sigmas(s_from, s_to)
                assert row == (s_from, down, up, 2.5, down - s_from)
            else:
                assert row == (s_from, s_to, 0.0, 2.5, s_to - s_from)


def test_unet_and_vae_parameter_counts():
    assert R.count_params(R.unet_spec(R.UNetCfg())) == 2_567_463_684
    assert R.count_params(R.vae_decoder_spec(R.VAECfg())) == 49_490_199


# ---------------------------------------------------------------- host logic vs the reference's vectors
def test_planner_matches_reference_golden():
    from latentblending_amd import planner
    g = gold("planner")
    for c in g["time_based"]:
        idx, stems = planner.time_based_branching(c["steps"], c["depth"], c.get("dt_unet", 0.0), c.get("dt_vae", 0.0),
                                                  c.get("tmax"), c.get("nmb"))
        assert [int(i) for i in idx] == c["idx"] and [int(s) for s in stems] == c["stems"], c
    for c in g["turbo"]:
        idx, stems = planner.turbo_branching(c["steps"], c["depth"], c["nmb"])
        assert idx == c["idx"] and stems == c["stems"], c
    for c in g["parental_coeffs"]:
        got = planner.parental_crossfeed_coeffs(c["steps"], c["idx_injection"], c["power"], c["range"], c["decay"])
        assert [float(x) for x in got] == c["coeffs"], c
    for c in g["anchor_coeffs"]:
        got = planner.anchor_crossfeed_coeffs(c["steps"], c["power"], c["range"], c["decay"])
        assert [float(x) for x in got] == c["coeffs"], c
    for c in g["guidance"]:
        got = [float(planner.damped_guidance(c["base"], c["damper"], f)) for f in c["fracts"]]
        assert got == c["values"], c


def test_tree_policy_units():
    from latentblending_amd.tree import TransitionTree, UNSCORED
    t = TransitionTree()
    t.reset(["a"], ["b"], "fa", "fb")
    assert t.similarities == [UNSCORED] and t.widest_gap() == 0          # reference quirk: first split w/o metric
    assert t.next_split(2) == (0.5, 0, 1)
    t.commit(0.5, 2, ["m"], "fm", 0.3, 0.7)
    assert t.fracts == [0.0, 0.5, 1.0] and t.similarities == [0.3, 0.7] and t.idx_injection == [0, 2, 0]
    assert t.next_split(2) == (0.75, 0, 2)                                 # parents skip the same-level branch
    t.commit(0.75, 2, ["n"], "fn", 0.7, 0.7)                               # tie -> first maximum
    assert t.widest_gap() == 1
    for c in gold("planner")["closest_idx"]:
        t.fracts = list(c["fracts"])
        assert list(t.neighbours(c["q"])) == c["result"]


@pytest.mark.parametrize("run", range(3))
def test_engine_reproduces_reference_transition(run, cpu_backend):
    """Our host layer, driving the same tiny CPU pipe, reproduces the reference run frozen in
    tests/golden/tree.json: census, tree, similarities (exact floats), latents and frames (hashes)."""
    from latentblending_amd import BlendingEngine
    import hashlib
    c = gold("tree")[run]
    cfgd = c["config"]
    p = tiny_pipe(turbo=c["turbo"])
    np.random.seed(0)
    be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False)
    be.set_dimensions((128, 128))
    if "steps" in cfgd:
        be.set_num_inference_steps(cfgd["steps"])
    if "gs" in cfgd:
        be.set_guidance_scale(cfgd["gs"])
    be.set_branching(depth_strength=cfgd.get("depth"), nmb_max_branches=cfgd["nmb"])
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    p.noise.reset()
    p.unet.calls = p.vae.calls = 0
    imgs = be.run_transition(fixed_seeds=[420, 421])
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).tobytes()).hexdigest()[:16]
    assert len(imgs) == c["frames"] and p.unet.calls == c["unet_calls"] and p.vae.calls == c["vae_calls"]
    assert p.noise.draws == c["noise_draws"]
    assert [int(i) for i in be.list_idx_injection] == c["list_idx_injection"]
    assert [int(s) for s in be.list_nmb_stems] == c["list_nmb_stems"]
    assert [float(f) for f in be.tree_fracts] == c["tree_fracts"]
    assert [int(i) for i in be.tree_idx_injection] == c["tree_idx_injection"]
    assert [[x is None for x in l] for l in be.tree_latents] == c["none_pattern"]
    check_against_golden_run(be, imgs, c)


@pytest.mark.parametrize("frontier", [1, 8])
def test_guidance_left_behind_is_the_last_committed_branchs(frontier, cpu_backend):
    """Round-5 review, parity bug 1: a frontier round stored the guidance of the last spec EVALUATED; the reference leaves the
    dampened scale of the last branch COMMITTED (blending_engine.py:155-164, 358-362) and computes the next transition's new
    anchor under it (:370-423).  Fixture: the unchanged reference's chain (tests/golden/guidance_chain.json): 3.25 after both
    transitions (round 5 at frontier 8: 3.75, and a different second transition)."""
    from latentblending_amd import BlendingEngine
    sys_path_tests = os.path.join(ROOT, "tests")
    import sys
    if sys_path_tests not in sys.path:
        sys.path.insert(0, sys_path_tests)
    from _baseline_cfgs import check_guidance_chain, run_guidance_chain
    p = tiny_pipe(turbo=False)
    np.random.seed(0)
    be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False, frontier_width=frontier)
    p.noise.reset()
    runs = run_guidance_chain(be)
    assert [r[1] for r in runs] == [3.25, 3.25]
    check_guidance_chain(be, runs, sim_rtol=2e-3, norm_rtol=2e-3, mean_tol=0.25, head_tol=2, ds_tol=0.5)


def test_live_differential_against_unchanged_reference(cpu_backend):
    """Our engine against the unchanged reference's run of the same chain, including branch-1 crossfeed, swap_forward +
    recycle (multi-transition chain, example_multi_trans.py:39-58): the reference's run is frozen in
    tests/golden/crossfeed_chain.{json,npz} (oracle/make_golden.py::crossfeed_chain_fixture) - identical tree, call census
    and noise draws, every frame within one grey level (CPU summation order varies with thread count and ISA).  Where the
    reference itself is importable, both engines also run side by side here and must agree bit for bit."""
    from latentblending_amd import BlendingEngine
    c = gold("crossfeed_chain")
    want = np.load(os.path.join(GOLD, "crossfeed_chain.npz"))["frames"]
    ref = H.load_reference() if H.reference_available() else None
    outs = []
    for which in (("ref", "ours") if ref is not None else ("ours",)):
        p = tiny_pipe(True)
        np.random.seed(0)
        with H.cuda_is_identity():
            be = ref.BlendingEngine(p) if which == "ref" else BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False)
            be.set_dimensions((128, 128))
            be.set_branching(nmb_max_branches=3)
            be.set_branch1_crossfeed(0.3, 0.5, 0.5)
            frames = []
            prompts = ["a", "b", "c"]
            for i in range(2):
                if i == 0:
                    be.set_prompt1(prompts[0]); be.set_prompt2(prompts[1])
                else:
                    be.swap_forward(); be.set_prompt2(prompts[i + 1])
                p.noise.reset()
                frames.append([np.asarray(f) for f in be.run_transition(recycle_img1=i > 0, fixed_seeds=[5 + i, 6 + i])])
            outs.append((frames, [float(f) for f in be.tree_fracts], p.unet.calls, p.noise.draws))
    fb, tb, cb, db = outs[-1]
    assert tb == c["tree_fracts"] and cb == c["unet_calls"] and db == c["noise_draws"]
    assert [len(x) for x in fb] == c["frames_per_transition"]
    got = np.stack([np.stack(x) for x in fb]).astype(np.int16)
    assert got.shape == want.shape
    d = np.abs(got - want.astype(np.int16))
    assert d.max() <= 1 and (d == 0).mean() >= 0.99, (int(d.max()), float((d == 0).mean()))
    if ref is not None:
        (fa, ta, ca, _), _ = outs
        assert ta == tb and ca == cb
        for x, y in zip(fa, fb):
            assert len(x) == len(y) and all(np.array_equal(a, b) for a, b in zip(x, y))


@pytest.mark.parametrize("turbo,seed", [(True, 420), (True, 421), (False, 7)])
def test_get_noise_is_diffusers_prepare_latents(turbo, seed, cpu_backend):
    """``DiffusersHolder.get_noise`` -> ``pipe.prepare_latents(1, 4, H, W, torch.float16, device, Generator.manual_seed(seed))``
    (/root/reference/latentblending/diffusers_holder.py:98-111); diffusers' randn_tensor draws IN the requested dtype
     - on the CPU generator an fp16 draw is a different stream from an fp32 draw cast to fp16
    (seed 420: first value 0.9907 vs -0.0070), which is what rounds 1-3 shipped."""
    from latentblending_amd import DiffusersHolder
    p = tiny_pipe(turbo)
    dh = DiffusersHolder(p)
    dh.set_dimensions((128, 128))
    z = dh.get_noise(seed)
    want = torch.randn((1, 4, 16, 16), generator=torch.Generator().manual_seed(seed), dtype=torch.float16) * p.scheduler.init_noise_sigma
    assert z.dtype == torch.float16 and z.shape == (1, 4, 16, 16) and torch.equal(z, want)
    wrong = torch.randn((1, 4, 16, 16), generator=torch.Generator().manual_seed(seed), dtype=torch.float32).to(torch.float16)
    assert not torch.equal(z, wrong * p.scheduler.init_noise_sigma)


def test_reference_error_behaviour_is_kept(cpu_backend):
    from latentblending_amd import BlendingEngine
    p = tiny_pipe(True)
    with pytest.raises(AssertionError):
        BlendingEngine(p, guidance_scale_mid_damper=0.0, metric=R.OracleLPIPS(7), verbose=False)
    be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False)
    with pytest.raises(AssertionError):
        be.set_branching(t_compute_max_allowed=3)                 # turbo: time budget unsupported
    with pytest.raises(AssertionError):
        be.run_transition(fixed_seeds=[1, 2, 3])
    with pytest.raises(AssertionError):
        be.dh.prepare_mixing([0.1, 0.2], None)                     # wrong coefficient count
    with pytest.raises(ValueError):
        be.dh.prepare_mixing((0.1,), None)
    with pytest.raises(AssertionError):
        be.run_diffusion(("not", "a", "list"))
    # cfg-1 as written (num_inference_steps=1) cannot build a tree in the reference either
    be.set_num_inference_steps(1)
    be.set_branching(nmb_max_branches=3)
    be.set_prompt1("a"); be.set_prompt2("b")
    with pytest.raises((IndexError, TypeError)):
        be.run_transition(fixed_seeds=[1, 2])
    base = BlendingEngine(tiny_pipe(False), metric=R.OracleLPIPS(7), verbose=False)
    with pytest.raises(ValueError):
        base.set_branching(t_compute_max_allowed=5, nmb_max_branches=5)
    assert (base.parental_crossfeed_power, base.parental_crossfeed_range, base.parental_crossfeed_decay) == (0.3, 0.6, 0.9)


# ---------------------------------------------------------------- boundary
def test_c_abi_exports_every_declared_symbol():
    from latentblending_amd.hip import lib
    header = open(os.path.join(ROOT, "include", "lb_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    study = re.search(r"#ifdef LB_STUDY_BUILD(.*?)#endif", header, flags=re.S)
    header = header.replace(study.group(0), "")                     # study-build-only switches: must NOT be in the product library
    assert set(re.findall(r"\b(lb_[a-z0-9_]+)\s*\(", study.group(1))) == set(lib.STUDY_SIGNATURES)
    declared = set(re.findall(r"\b(lb_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 40
    cdll = ctypes.CDLL(lib.LIB_PATH)
    missing = [n for n in declared if not hasattr(cdll, n)]
    assert not missing, f"declared in include/lb_hip.h but not exported: {missing}"
    unbound = sorted(declared - set(lib.SIGNATURES))
    assert not unbound, f"declared but not bound in hip/lib.py: {unbound}"
    undeclared = sorted(set(lib.SIGNATURES) - declared)
    assert not undeclared, f"bound in hip/lib.py but not declared in include/lb_hip.h: {undeclared}"
    assert lib.api.lb_version() >= 10000
    # struct layout guard: ctypes mirror == what a C compiler makes of the header
    import shutil
    import subprocess
    import tempfile
    if shutil.which("gcc"):
        with tempfile.TemporaryDirectory() as td:
            src = os.path.join(td, "t.c")
            with open(src, "w") as fh:
                fh.write('#include <stdio.h>\n#include <stddef.h>\n#include "lb_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",'
                         'sizeof(LbGemmParams), offsetof(LbGemmParams, splitk), sizeof(LbAttnParams), offsetof(LbAttnParams, scale), '
                         'sizeof(LbConvPlan), offsetof(LbConvPlan, ragged_kind));return 0;}\n')
            exe = os.path.join(td, "t")
            subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
            sizes = [int(x) for x in subprocess.check_output([exe]).split()]
        assert sizes == [ctypes.sizeof(lib.LbGemmParams), lib.LbGemmParams.splitk.offset,
                         ctypes.sizeof(lib.LbAttnParams), lib.LbAttnParams.scale.offset,
                         ctypes.sizeof(lib.LbConvPlan), lib.LbConvPlan.ragged_kind.offset]


def test_product_path_has_no_cpu_fallback():
    from latentblending_amd.backend import HipBackend
    be = HipBackend()
    a = torch.zeros(8, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU"):
        be.slerp(a, a, 0.5)
    with pytest.raises(RuntimeError, match="no CPU"):
        be.lerp(a, a, 0.5)
    if not torch.cuda.is_available():
        import latentblending_amd.native as N
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            N.NativeSDXLPipe(turbo=True, unet_cfg=N.UNetConfig(**dataclasses.asdict(R.tiny_unet_cfg())))
    # a scheduler name the pipe does not know is an error, not a silent Euler pipe (round-5 advice); checked before any device work
    import latentblending_amd.native as N
    for bad in ("dpm", "DDIM2", object()):
        with pytest.raises(ValueError, match="scheduler"):
            N.NativeSDXLPipe(turbo=True, scheduler=bad)
    # product modules never import the oracle
    for dirpath, _, files in os.walk(os.path.join(ROOT, "latentblending_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{f} imports the oracle"


def test_launchers_validate_arguments_without_a_gpu():
    """Argument errors are reported through the C-ABI error channel before anything is launched."""
    from latentblending_amd.hip import lib
    p = lib.LbGemmParams()
    p.M, p.N, p.K, p.lda, p.ldw, p.ldc = 16, 6, 64, 64, 64, 8      # N not a multiple of 4
    with pytest.raises(RuntimeError, match="multiple of 4"):
        lib.api.lb_gemm_f16(ctypes.byref(p), None)
    with pytest.raises(RuntimeError, match="n must be a multiple of 8"):
        lib.api.lb_slerp_batched_f16(16, 16, 16, 16, 2, 12, None)


def test_synthetic_provider_equals_oracle_weights():
    import latentblending_amd.native as N

    class Rec(N.SyntheticProvider):
        def __init__(self, seed):
            super().__init__(seed); self.got = {}

        def weight(self, n, *a, **k):
            self.got[n] = super().weight(n, *a, **k); return self.got[n]

        def bias(self, n, *a):
            self.got[n] = super().bias(n, *a); return self.got[n]

        def norm_weight(self, n, *a):
            self.got[n] = super().norm_weight(n, *a); return self.got[n]

        def positive(self, n, *a):
            self.got[n] = super().positive(n, *a); return self.got[n]

    def same(got, ref):
        assert set(got) == set(ref)
        assert all(torch.equal(got[k].reshape(ref[k].shape), ref[k]) for k in ref)
    oc, vc = R.tiny_unet_cfg(), R.tiny_vae_cfg()
    rec = Rec(0); N.NativeUNet(N.UNetConfig(**dataclasses.asdict(oc)), rec, "cpu"); same(rec.got, R.make_weights(R.unet_spec(oc), 0))
    rec = Rec(1); N.NativeVAEDecoder(N.VAEConfig(**dataclasses.asdict(vc)), rec, "cpu"); same(rec.got, R.make_weights(R.vae_decoder_spec(vc), 1))
    from latentblending_amd.native.lpips import NativeLPIPS
    rec = Rec(7); NativeLPIPS(rec, "cpu"); same(rec.got, R.make_weights(R.lpips_spec(), 7))


def test_host_utilities_and_movie_writer(tmp_path):
    from latentblending_amd import utils
    from latentblending_amd.movie import MovieSaver, fill_up_frames_linear_interpolation
    from latentblending_amd.native.frames import DeviceImage
    imgs = [np.full((8, 8, 3), v, dtype=np.uint8) for v in (0, 100, 200)]
    np.random.seed(1)
    out = utils.add_frames_linear_interp(imgs, nmb_frames_target=10)
    assert len(out) == 10 and out[0].mean() == 0 and out[-1].mean() == 200
    assert utils.add_frames_linear_interp(imgs, nmb_frames_target=2) is imgs
    with pytest.raises(ValueError):
        utils.add_frames_linear_interp(imgs, fps_target=3, nmb_frames_target=4)
    assert len(utils.get_spacing(7, 1.0)) == 7 and len(utils.get_spacing(8, 2.0)) == 8 and len(utils.get_spacing(9, 2.0)) == 9
    assert utils.compare_dicts({"a": 1, "b": 2}, {"a": 1, "b": 3, "c": 4}) == {"b": [2, 3]}
    assert re.fullmatch(r"\d{6}_\d{6}_\d{3}", utils.get_time("millisecond"))
    fp = tmp_path / "s.yml"
    utils.yml_save(str(fp), {"x": 1, "y": [1, 2]})
    assert utils.yml_load(str(fp)) == {"x": 1, "y": [1, 2]}
    frames = fill_up_frames_linear_interpolation([DeviceImage(torch.from_numpy(i)) for i in imgs], 2, 5)
    assert len(frames) == 10
    saver = MovieSaver(str(tmp_path / "m.avi"), fps=5, shape_hw=[8, 8])
    for f in frames:
        saver.write_frame(f)
    saver.finalize()
    blob = open(tmp_path / "m.avi", "rb").read()
    assert blob[:4] == b"RIFF" and blob[8:12] == b"AVI " and blob.count(b"00dc") >= 10


def golden_key_frames(seed, n, h, w):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for _ in range(n)]


def frame_sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a)).tobytes()).hexdigest()[:16]


def test_frame_inbetweening_matches_reference_golden():
    """add_frames_linear_interp (host path) against tests/golden/frames.json = the unchanged reference's
    utils.add_frames_linear_interp on the same seeded key frames and numpy RNG (oracle/make_golden.py frames_fixture)."""
    from latentblending_amd import utils
    for c in json.load(open(os.path.join(GOLD, "frames.json"))):
        imgs = golden_key_frames(c["seed"], c["n"], c["h"], c["w"])
        np.random.seed(c["rng_seed"])
        out = utils.add_frames_linear_interp(imgs, nmb_frames_target=c["target"])
        assert len(out) == c["count"]
        assert [frame_sha(o) for o in out] == c["sha"]


def test_movie_concatenation_and_lunar_tools_facade(tmp_path):
    """lunar_tools.concatenate_movies stand-in (example_multi_trans.py:62): parts back to back, payloads kept."""
    import lunar_tools
    from latentblending_amd import movie
    assert lunar_tools.MovieSaver is movie.MovieSaver and lunar_tools.concatenate_movies is movie.concatenate_movies
    with pytest.raises(AttributeError):
        lunar_tools.SomethingElse
    parts = []
    for k, n in enumerate((3, 5)):
        fp = str(tmp_path / f"p{k}.mp4")
        s = movie.MovieSaver(fp, fps=7, shape_hw=[16, 24])
        for i in range(n):
            s.write_frame(np.full((16, 24, 3), 40 * k + 10 * i, dtype=np.uint8))
        s.finalize()
        parts.append(fp)
        assert movie.read_movie_header(fp) == (7, 16, 24, n)
    fp_all = str(tmp_path / "all.mp4")
    lunar_tools.concatenate_movies(fp_all, parts)
    assert movie.read_movie_header(fp_all) == (7, 16, 24, 8)
    jp = movie.read_movie_jpegs(fp_all)
    assert jp == movie.read_movie_jpegs(parts[0]) + movie.read_movie_jpegs(parts[1])
    from PIL import Image
    import io
    means = [float(np.asarray(Image.open(io.BytesIO(j))).mean()) for j in jp]
    assert np.allclose(means, [0, 10, 20, 40, 50, 60, 70, 80], atol=1.5)
    bad = str(tmp_path / "other.mp4")
    with pytest.warns(UserWarning, match="Motion-JPEG AVI"):          # the fallback writer says what the file really holds
        s = movie.MovieSaver(bad, fps=9, shape_hw=[16, 24])
    assert s.container == "avi-mjpeg"
    s.write_frame(np.zeros((16, 24, 3), np.uint8)); s.finalize()
    with pytest.raises(AssertionError):
        movie.concatenate_movies(fp_all, [parts[0], bad])


def test_multi_transition_driver_and_movie_json(tmp_path, cpu_backend):
    """replay.run_movie_json == the loop of example_multi_trans_json.py:47-71 written out by hand: same
    engine calls, same frames, every shared key frame diffused once, one part per segment + the final movie."""
    from latentblending_amd import BlendingEngine, replay
    from latentblending_amd import movie

    def engine():
        p = tiny_pipe(turbo=True)
        np.random.seed(0)
        be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False)
        be.set_branching(nmb_max_branches=3)
        return p, be

    prompts = ["a reef", "an alien planet", "a city at night"]
    negs = ["blurry", "pale", "lofi"]
    seeds = [11, 12, 13]
    # the file the UI would have written (gradio_ui.py:168-190)
    p0, be0 = engine()
    be0.set_dimensions((128, 128)); be0.set_num_inference_steps(4)
    fp_json = str(tmp_path / "movie.json")
    replay.save_movie_json(fp_json, be0, [{"iteration": i, "seed": seeds[i], "prompt": prompts[i],
                                           "negative_prompt": negs[i], "preview_image": None} for i in range(3)])
    header, items = replay.load_movie_json(fp_json)
    assert header == {"settings": "sdxl", "width": 128, "height": 128, "num_inference_steps": 4} and len(items) == 3
    # by hand, as the reference script does it
    p1, be1 = engine()
    be1.set_dimensions((128, 128)); be1.set_num_inference_steps(4)
    hand = []
    for i in range(2):
        if i == 0:
            be1.set_prompt1(prompts[0]); be1.set_negative_prompt(negs[0]); be1.set_prompt2(prompts[1])
        else:
            be1.swap_forward(); be1.set_negative_prompt(negs[i + 1]); be1.set_prompt2(prompts[i + 1])
        hand.append([np.asarray(f) for f in be1.run_transition(recycle_img1=i > 0, fixed_seeds=seeds[i:i + 2])])
    # through the driver
    p2, be2 = engine()
    fp_movie = str(tmp_path / "out.mp4")
    segs = replay.run_movie_json(be2, fp_json, fp_movie, duration_single_trans=1, fps=6, dp_parts=str(tmp_path))
    assert len(segs) == 2 and p2.unet.calls == p1.unet.calls and p2.vae.calls == p1.vae.calls
    for a, b in zip(hand, segs):
        assert len(a) == len(b) == 5
        for x, y in zip(a, b):
            assert np.array_equal(x, np.asarray(y))
    assert np.array_equal(np.asarray(segs[0][-1]), np.asarray(segs[1][0]))          # shared key frame, recycled
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("tmp_part_")) == ["tmp_part_000.mp4", "tmp_part_001.mp4"]
    assert movie.read_movie_header(fp_movie) == (6, 128, 128, 12)
    # argument checking
    with pytest.raises(ValueError):
        replay.run_multi_transition(be2, ["only one"], [1])
    with pytest.raises(ValueError):
        replay.run_multi_transition(be2, prompts, [1, 2])
    bad = str(tmp_path / "bad.json")
    json.dump([{"foo": 1}], open(bad, "w"))
    with pytest.raises(ValueError):
        replay.load_movie_json(bad)


def test_pipelined_keyframes_chain_equals_the_sequential_chain(cpu_backend):
    """replay.run_multi_transition(pipeline_keyframes=True): all key frames denoised ahead of the transitions
    (BlendingEngine.precompute_keyframes), every transition with both anchors recycled.  On a deterministic sampler
    (SDXL-base config: Euler, CFG) the frames must be bit-identical to the sequential loop of example_multi_trans.py:39-58
    written out by hand - once that loop's one quirk is removed: it denoises key frame k+1 with the mid-dampened guidance
    scale the previous transition's last branch left behind; the pipelined form uses the scale current at the start."""
    from latentblending_amd import BlendingEngine, replay

    def engine():
        p = tiny_pipe(turbo=False)
        np.random.seed(0)
        be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False)
        be.set_dimensions((128, 128)); be.set_num_inference_steps(4); be.set_guidance_scale(3.0)
        be.set_branching(depth_strength=0.5, nmb_max_branches=3)
        return p, be

    prompts = ["a reef", "an alien planet", "a city at night"]
    negs = ["blurry", "pale", "lofi"]
    seeds = [11, 12, 13]
    p1, be1 = engine()
    hand = []
    for i in range(2):
        if i == 0:
            be1.set_prompt1(prompts[0]); be1.set_negative_prompt(negs[0]); be1.set_prompt2(prompts[1])
        else:
            be1.guidance_scale = be1.dh.guidance_scale = 3.0         # (the quirk, removed)
            be1.swap_forward(); be1.set_negative_prompt(negs[i + 1]); be1.set_prompt2(prompts[i + 1])
        hand.append([np.asarray(f) for f in be1.run_transition(recycle_img1=i > 0, fixed_seeds=seeds[i:i + 2])])
    p2, be2 = engine()
    seen = []
    segs = replay.run_multi_transition(be2, prompts, seeds, None, list_negative_prompts=negs, pipeline_keyframes=True,
                                       on_segment=lambda i, fr: seen.append(i))
    assert seen == [0, 1] and be2.stats["keyframes_precomputed"] == 3
    assert p2.unet.calls == p1.unet.calls                  # the same trajectories, only earlier
    assert p2.vae.calls < p1.vae.calls                     # every key frame decoded once (the loop decodes a recycled anchor again)
    for a, b in zip(hand, segs):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x, np.asarray(y))
    assert np.array_equal(np.asarray(segs[0][-1]), np.asarray(segs[1][0]))
    assert be2.negative_prompt == be1.negative_prompt and be2.prompt2 == be1.prompt2
    # key frames depend on each other under branch1 crossfeed: refused
    be2.set_branch1_crossfeed(0.3, 0.5, 0.5)
    with pytest.raises(AssertionError):
        replay.run_multi_transition(be2, prompts, seeds, None, pipeline_keyframes=True)


def test_synthetic_weight_streams_are_the_same_on_both_sides():
    """The product's SyntheticProvider and the oracle's make_weights must draw the same values for the same (name, seed) - tiny
    tensors from the single torch stream the golden fixtures were made with, big ones (> 1.5 * 2^20 elements) from the chunked
    numpy streams - whatever the thread count."""
    from latentblending_amd.native import weights as W
    for shape in [(7,), (64, 64), (256, 512, 3, 3), (1280, 1280), (1280, 1280, 3, 3)]:
        a, b = R._gen("mid_block.x.weight", shape, 0.03, 5, 0.5), W._seeded("mid_block.x.weight", shape, 0.03, 5, 0.5)
        assert torch.equal(a, b) and a.shape == tuple(shape)
        if a.numel() >= 4096:
            assert abs(float(a.mean()) - 0.5) < 0.005 and abs(float(a.std()) - 0.03) < 0.002
    g = torch.Generator().manual_seed((zlib.crc32(b"mid_block.x.weight") ^ (5 * 0x9E3779B1)) & 0x7FFFFFFF)
    assert torch.equal(W._seeded("mid_block.x.weight", (64, 64), 0.03, 5), torch.randn((64, 64), generator=g) * 0.03)    # the legacy stream
    big = W._seeded("a", (1280, 1280), 1.0, 0)
    assert not torch.equal(big, W._seeded("a", (1280, 1280), 1.0, 1)) and not torch.equal(big, W._seeded("b", (1280, 1280), 1.0, 0))
    assert abs(float((big[:640] * big[640:]).mean())) < 0.01                      # chunks are independent streams


def test_gemm_tile_policy_is_pinned():
    """lb_gemm_plan (pure host arithmetic of the launcher): the tile / split-K choices the MI355X sweeps led to
    (profiles/r01_gemm_*.txt, tools/ab_policy.py, profiles/r04_gemm_bench_call*.txt) for the shapes the SDXL programs launch.
    Tiles: 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 256x128 (8 waves), 5 = 256x256 (8 waves, lock-step), 7 = 192x128 (6 waves, rounds 2-5),
    9 = 256x256 ping-pong (gemm_pp.hip), 10 = 192x128 as 8 waves of 48x64 (round 6: every SIMD issues the same number of MFMAs),
    11 = 64x64 with two K-groups of 4 waves per block (round 6: small unsplit grids)."""
    from latentblending_amd.hip import lib

    def plan(M, N, K, conv=False, geglu=False, ws=None, zero_page=True):
        if ws is None:                  # the emitter's rule (native/runtime.py _gemm_ws): slabs only for <= 640 64x64 tiles
            ws = ((M + 63) // 64) * ((N + 63) // 64) <= 640
        p = lib.LbGemmParams()
        p.M, p.N, p.K, p.conv = M, N, K, int(conv)
        p.flags = lib.GEMM_GEGLU if geglu else 0
        p.partial = 64 if ws else None                # (never dereferenced by the planner)
        p.zero_page = 64 if zero_page else None
        t, sk, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
        lib.api.lb_gemm_plan(ctypes.byref(p), ctypes.byref(t), ctypes.byref(sk), ctypes.byref(nb))
        return t.value, sk.value, nb.value

    # UNet at B=17 (M = 17*256 / 17*1024)
    assert plan(4352, 10240, 1280, geglu=True)[:2] == (9, 1)            # GEGLU: 256x256 ping-pong, 680 blocks
    assert plan(4352, 10240, 1280, geglu=True)[2] == 17 * 40
    assert plan(4352, 1280, 1280) == (10, 1, 230)                       # short K, 170 blocks of 256x128 = 2/3 of the chip: 230 of 192x128
    assert plan(4352, 1280, 5120) == (10, 1, 230)                       # ... at every K (round 5: 71.9 vs 73.7 us at K = 5120)
    assert plan(4352, 2560, 1280)[:2] == (5, 1)                         # one round of 256x256 beats two of 256x128 (170 tiles: lock-step form)
    assert plan(4352, 3840, 1280) == (9, 1, 255)                        # fused q|k|v: one round of ping-pong tiles
    assert plan(17408, 5120, 640, geglu=True)[0] == 9                   # K = 640 pays only over several rounds (1360 tiles) ...
    assert plan(17408, 1920, 640)[0] != 9 and plan(17408, 640, 640)[0] != 9     # ... not over one or two
    assert plan(17408, 640, 2560) == (9, 1, 204)                        # (no automatic split-K on the ping-pong kernel)
    assert plan(1360, 166400, 2048)[0] == 9                             # per-branch context K|V projection
    assert plan(17408, 640, 640)[0] in (1, 2)                           # short K: 4-wave tiles
    assert plan(17408, 640, 5760, conv=True)[0] == 5
    assert plan(69632, 320, 2880, conv=True)[0] == 1                    # N = 320 pads badly to 256-wide tiles
    # VAE at B=17
    assert plan(4456448, 128, 1152, conv=True)[0] == 4                  # N = 128: 256x128
    assert plan(1114112, 256, 2304, conv=True)[0] == 5
    assert plan(4456448, 4, 1152, conv=True)[0] == 3                    # conv_out: 3 real columns (this bare plan describes no 3x3 geometry)

    def conv_plan(B, H, Cin, N, flags=0):
        p = lib.conv_probe(B, H, H, Cin, N, flags=flags)
        t, sk, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
        lib.api.lb_gemm_plan(ctypes.byref(p), ctypes.byref(t), ctypes.byref(sk), ctypes.byref(nb))
        return t.value, nb.value
    assert conv_plan(17, 512, 128, 4, lib.GEMM_OUT_F32) == (8, 17 * 1024)   # VAE conv_out: narrow-N kernel, 16x16-pixel tiles
    assert conv_plan(17, 64, 320, 4) == (8, 17 * 16)                        # UNet conv_out
    assert conv_plan(17, 64, 320, 320)[0] == 6                              # ordinary widths: halo-tile kernel
    # UNet at B=2 (M = 512 / 2048): small tiles, split-K where K is long
    assert plan(512, 1280, 1280) == (11, 1, 160)                        # round 6: two K-groups per 64x64 block where the grid leaves one wave per SIMD
    assert plan(512, 1280, 5120) == (3, 4, 160)
    assert plan(512, 1280, 11520, conv=True) == (3, 4, 160)
    assert plan(2048, 640, 5760, conv=True) == (2, 4, 160)              # 128x64 + split instead of 320 unsplittable blocks
    assert plan(2048, 640, 640) == (3, 1, 320)
    assert plan(512, 10240, 1280, geglu=True) == (10, 1, 240) and plan(2048, 5120, 640, geglu=True)[0] == 10      # round 6: small-batch GEGLU on the 8-wave 192x128 tile
    assert plan(512, 1280, 5120, ws=False)[1] == 1                      # no slab workspace -> never splits
    # without the zero page the direct-to-LDS family (and its 8-wave tiles) is not available
    assert plan(4352, 1280, 5120, zero_page=False)[0] in (1, 2) and plan(4456448, 128, 1152, conv=True, zero_page=False)[0] == 1
    assert plan(4352, 10240, 1280, geglu=True, zero_page=False)[0] == 9      # (the ping-pong kernel masks nothing: no zero page needed)
    # the study switches (arithmetic / policy A/B) are NOT part of the product library
    for name in ("lb_gemm_set_policy", "lb_slerp_set_study", "lb_conv_halo_set_study"):
        assert not hasattr(ctypes.CDLL(lib.LIB_PATH), name), f"{name} must only exist in -DLB_STUDY_BUILD libraries"


@pytest.mark.parametrize("TW,H,W", [(32, 16, 64), (16, 16, 16), (32, 8, 32)])
def test_halo_conv_index_math(TW, H, W):
    """Row-level emulation of csrc/conv3_halo.hip's address arithmetic (the kernel itself could not be run
    before the round's GPU budget ended): the loader's (wave, instruction, lane) -> halo row -> pixel mapping
    covers the halo exactly once, zero-fills out-of-image pixels, and `hbase + ky*(TW+2) + kx` reads the input
    pixel each tap needs; the result at `mrow` equals conv2d."""
    import torch.nn.functional as F
    TH, HWP = 256 // TW, TW + 2
    HR = (TH + 2) * HWP
    HRG = (HR + 7) // 8
    EXTRA = HRG - 40
    assert 1 <= EXTRA <= 8
    B, Cin, N = 2, 64, 8
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64)
    wt = torch.randn(N, 3, 3, Cin, generator=g, dtype=torch.float64)
    ref = F.conv2d(x.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(B * H * W, N)
    out = torch.full((B * H * W, N), float("nan"), dtype=torch.float64)
    tiles_x, tiles_y = W // TW, H // TH
    for tile in range(B * tiles_y * tiles_x):
        tx, rest = tile % tiles_x, tile // tiles_x
        ty, b = rest % tiles_y, rest // tiles_y
        y0, x0 = ty * TH, tx * TW
        halo = torch.full((HRG * 8, Cin), float("nan"), dtype=torch.float64)
        written = np.zeros(HRG * 8, dtype=int)
        for wave in range(8):
            for j in range(6):
                if not (j < 5 or wave < EXTRA):
                    continue                              # (the kernel does not issue this instruction)
                gidx = j * 8 + wave if j < 5 else 40 + wave
                for r8 in range(8):
                    row = gidx * 8 + r8
                    hy, hx = divmod(row, HWP)
                    y, xx = y0 + hy - 1, x0 + hx - 1
                    ok = row < HR and 0 <= y < H and 0 <= xx < W
                    halo[row] = x[b, y, xx] if ok else 0.0
                    written[row] += 1
        assert (written[:HR] == 1).all() and written.max() == 1
        for wave_m in range(4):
            for i in range(4):
                for l16 in range(16):
                    m = wave_m * 64 + i * 16 + l16
                    py, px = divmod(m, TW)
                    hbase = py * HWP + px
                    mrow = (b * H + y0 + py) * W + x0 + px
                    acc = torch.zeros(N, dtype=torch.float64)
                    for tap in range(9):
                        ky, kx = divmod(tap, 3)
                        acc += wt[:, ky, kx] @ halo[hbase + ky * HWP + kx]
                    assert torch.isnan(out[mrow]).all()
                    out[mrow] = acc
    assert torch.allclose(out, ref, rtol=1e-12, atol=1e-12)
    # request accounting of one step: [halo?] + 2 weight loads; wait constant = loads of the two previous steps
    cnt = lambda tap: 2 + (1 if tap % 9 <= 4 else 0)
    assert [cnt(t - 1) + cnt(t - 2) for t in range(9)] == [4, 5, 6, 6, 6, 6, 5, 4, 4]


# ---------------------------------------------------------------- speculation under a skewed metric
@pytest.mark.parametrize("skew", [3.0, -4.0])
def test_speculative_frontier_equals_sequential_under_skewed_metric(skew, cpu_backend):
    """With a flat similarity landscape the level-order guess of the frontier is consumed completely; with a metric
    that grows (or shrinks) exponentially along the transition the reference's greedy order leaves the balanced tree.
    The speculative engine must still commit exactly the sequential tree (policy of
    latentblending/blending_engine.py:531-588), merely in more rounds and with dropped speculation - both reported."""
    import math
    from latentblending_amd import BlendingEngine

    def run(width):
        p = tiny_pipe(turbo=True)
        np.random.seed(0)
        be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False, frontier_width=width)
        base = be.get_lpips_similarity

        def skewed(a, b, fa, fb):
            be.pair_metric = None
            try:
                d = base(a, b)
            finally:
                be.pair_metric = skewed
            return d * math.exp(skew * 0.5 * (fa + fb))
        be.pair_metric = skewed
        be.set_dimensions((128, 128))
        be.set_branching(nmb_max_branches=9)
        be.set_prompt1("photo of a reef")
        be.set_prompt2("rendering of an alien planet")
        p.noise.reset()
        be.run_transition(fixed_seeds=[420, 421])
        return be
    seq, spec = run(1), run(4)
    assert seq.tree_fracts == spec.tree_fracts and seq.tree_idx_injection == spec.tree_idx_injection
    assert np.allclose([float(x) for x in seq.tree_similarities], [float(x) for x in spec.tree_similarities], rtol=1e-6)
    balanced = [i / 10 for i in range(11)]
    assert seq.tree_fracts != balanced                      # the skew really bends the tree
    assert spec.stats["frontier_rounds"] >= 3               # ... which costs the frontier several rounds
    assert spec.stats["speculation_evaluated"] >= 9
    assert spec.stats["speculation_evaluated"] - spec.stats.get("speculation_dropped", 0) == 9


@pytest.mark.parametrize("skew,power", [(3.0, 2.0), (-4.0, 2.0), (6.0, 1.0)])
def test_frontier_second_round_walks_the_predicted_greedy_order(skew, power, cpu_backend):
    """cfg-2-shaped tree (15 branches, frontier 16) under a metric that depends on the fractions only (|df|^power x exp(skew x
    position): power 2 x skew 3 reproduces the rounds / evaluated counts the MI355X bench measured with the skewed LPIPS).
    After the blind first round the engine walks the reference's greedy order forward on exact + predicted distances
    (children already evaluated are consumed virtually; a virtual gap's halves are predicted from the child / parent ratios
    measured so far): the level finishes in TWO rounds where the round-3 budget rule (branches missing minus evaluated
    children, whether or not the greedy order would ever ask for them) crawled one candidate per round (4 - 9 rounds).
    The tree is the sequential one under every setting of the two knobs."""
    import math
    from latentblending_amd import BlendingEngine

    def run(width, **attrs):
        p = tiny_pipe(turbo=True)
        np.random.seed(0)
        be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False, frontier_width=width)
        for k, v in attrs.items():
            setattr(be, k, v)
        be.pair_metric = lambda a, b, fa, fb: abs(fa - fb) ** power * math.exp(skew * 0.5 * (fa + fb))
        be.set_dimensions((64, 64))
        be.set_branching(nmb_max_branches=15)
        be.set_prompt1("photo of a reef")
        be.set_prompt2("rendering of an alien planet")
        p.noise.reset()
        be.run_transition(fixed_seeds=[420, 421])
        return be
    seq = run(1)
    assert seq.tree_fracts != [i / 16 for i in range(17)]                  # the metric really bends the tree
    spec = run(16)
    assert spec.tree_fracts == seq.tree_fracts and spec.tree_idx_injection == seq.tree_idx_injection
    assert spec.stats["frontier_rounds"] <= 3 and spec.stats["speculation_evaluated"] <= 24
    if (skew, power) == (3.0, 2.0):
        assert spec.stats["frontier_rounds"] == 2 and spec.stats["speculation_evaluated"] == 18
    assert spec.stats["speculation_evaluated"] - spec.stats.get("speculation_dropped", 0) == 15
    for attrs in (dict(learn_child_ratio=False), dict(speculation_oversubscribe=2.0), dict(speculate_virtual=False)):
        other = run(16, **attrs)
        assert other.tree_fracts == seq.tree_fracts, attrs
        assert other.stats["speculation_evaluated"] - other.stats.get("speculation_dropped", 0) == 15


@pytest.mark.parametrize("skew", [3.0, -4.0])
def test_previous_tree_as_speculation_prior(skew, cpu_backend):
    """``speculate_from_previous_tree`` (opt-in, round 6): the blind first round of a level takes its candidates from the commit
    order of the previous transition instead of the level order of the binary splitting.  Under a metric that bends the tree the
    first transition needs two rounds (18 evaluated, 3 dropped); the second one - same metric - needs ONE (15 evaluated, none
    dropped) and commits the identical (sequential) tree.  A prior from a DIFFERENT metric is only a worse guess: the tree is
    still exact.  Off (default): every transition speculates blind."""
    import math
    from latentblending_amd import BlendingEngine

    def metric(k):
        return lambda a, b, fa, fb: abs(fa - fb) ** 2.0 * math.exp(k * 0.5 * (fa + fb))

    def engine(width, prior):
        p = tiny_pipe(turbo=True)
        np.random.seed(0)
        be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False, frontier_width=width)
        be.speculate_from_previous_tree = prior
        be.pair_metric = metric(skew)
        be.set_dimensions((64, 64))
        be.set_branching(nmb_max_branches=15)
        be.set_prompt1("photo of a reef")
        be.set_prompt2("rendering of an alien planet")
        return be, p

    def transition(be, p):
        p.noise.reset()
        be.stats.clear()
        be.run_transition(fixed_seeds=[420, 421])
        return list(be.tree_fracts), dict(be.stats)

    seq, _ = transition(*engine(1, False))
    be, p = engine(16, True)
    first, st1 = transition(be, p)
    second, st2 = transition(be, p)
    assert first == seq and second == seq
    assert st1["frontier_rounds"] >= 2 and st1["speculation_evaluated"] > 15
    assert st2["frontier_rounds"] == 1 and st2["speculation_evaluated"] == 15 and st2.get("speculation_dropped", 0) == 0
    be.pair_metric = metric(-skew)                  # the prior now points the wrong way: more rounds, the same exact tree
    third, st3 = transition(be, p)
    be1, p1 = engine(1, False)
    be1.pair_metric = metric(-skew)
    assert third == transition(be1, p1)[0] and st3["frontier_rounds"] >= 2
    off, poff = engine(16, False)
    transition(off, poff)
    assert transition(off, poff)[1]["frontier_rounds"] == st1["frontier_rounds"]      # default: no memory between transitions


@pytest.mark.parametrize("B,H,W,Cin,N,ks", [(17, 512, 512, 128, 128, 3), (17, 64, 64, 320, 320, 3), (17, 16, 16, 1280, 1280, 3),
                                            (2, 64, 64, 640, 320, 3), (17, 256, 256, 256, 256, 2), (3, 32, 32, 192, 640, 2),
                                            (1, 16, 16, 64, 64, 3)])
def test_halo_conv_persistent_work_split(B, H, W, Cin, N, ks):
    """lb_conv_halo_plan + an emulation of the kernel's block -> work-item walk (csrc/conv3_halo.hip: XCD remap of the
    block id, items bid, bid + G, ...): every (image, tile[, parity], channel block) item is processed exactly once and a
    block keeps ONE channel block (and parity) for its whole life - what lets it keep its weight stream running across
    tile boundaries."""
    from latentblending_amd.hip import lib
    p = lib.conv_probe(B, H, W, Cin, N, ks)              # (zero_page: never dereferenced by the planner)
    kind, tw, items, grid = ctypes.c_int(), ctypes.c_int(), ctypes.c_long(), ctypes.c_long()
    lib.api.lb_conv_halo_plan(ctypes.byref(p), ctypes.byref(kind), ctypes.byref(tw), ctypes.byref(items), ctypes.byref(grid))
    assert kind.value == ks and tw.value in (16, 32)
    th = 256 // tw.value
    n_blocks = (N + 127) // 128
    par = 4 if ks == 2 else 1
    assert items.value == B * (H // th) * (W // tw.value) * par * n_blocks
    G = grid.value
    assert 0 < G <= items.value and (G == items.value or (G <= 256 and G % (n_blocks * par) == 0))
    seen = set()
    for blk in range(G):
        q, r, xcd, idx = G // 8, G % 8, blk % 8, blk // 8
        bid = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx
        keys = set()
        item = bid
        while item < items.value:
            block_n = item % n_blocks
            tile = item // n_blocks
            parity = tile & 3 if ks == 2 else 0
            keys.add((block_n, parity))
            assert item not in seen
            seen.add(item)
            item += G
        assert len(keys) <= 1, "a persistent block changed its weight slab"
        # the kernel derives (block_n, parity) once, from the block id: same thing as from any of its items
        if keys:
            assert keys == {(bid % n_blocks, (bid // n_blocks) & 3 if ks == 2 else 0)}
    assert len(seen) == items.value
    # LB_GEMM_CH_STATS: the statistics rows per sample come from the library (its routing + its tile constants), never from a
    # host-side restatement: (items / channel blocks) * 4 wave rows over the samples when lb_gemm_f16 would route the conv to
    # the halo kernel (3x3: only chip-filling grids under the default lb_gemm_set_halo(1)), else 0
    rows = lib.api.lb_gemm_ch_stat_rows(ctypes.byref(p))
    tile = ctypes.c_int()
    lib.api.lb_gemm_plan(ctypes.byref(p), ctypes.byref(tile), None, None)
    if ks == 2 or tile.value == 6:
        assert rows == items.value // n_blocks * 4 // B > 0
    else:
        assert rows == 0
    p.KH = p.KW = 1                                      # not a halo conv at all
    p.K, p.pad, p.scatter = Cin, 0, 0
    assert lib.api.lb_gemm_ch_stat_rows(ctypes.byref(p)) == 0


def test_negative_prompt_semantics_follow_diffusers(cpu_backend):
    """diffusers' encode_prompt zeroes the negative embeddings only for ``negative_prompt is None``; the reference holder
    passes its default "" (diffusers_holder.py:23,87), which is therefore ENCODED.  Both the oracle pipe and the holder on
    top of it must behave that way (the native pipe has the same logic: tests/test_native_gpu.py)."""
    from latentblending_amd import DiffusersHolder
    p = tiny_pipe(turbo=False)
    pe, npe, pooled, npooled = p.encode_prompt("a reef", negative_prompt=None)
    assert float(npe.abs().max()) == 0 and float(npooled.abs().max()) == 0
    for neg in ("", "blurry", ["blurry"]):
        _, npe, _, npooled = p.encode_prompt("a reef", negative_prompt=neg)
        assert float(npe.abs().max()) > 0 and float(npooled.abs().max()) > 0
    e1 = p.encode_prompt("a reef", negative_prompt="blurry")[1]
    e2 = p.encode_prompt("a reef", negative_prompt=["blurry"])[1]
    assert torch.equal(e1, e2) and not torch.equal(e1, p.encode_prompt("a reef", negative_prompt="")[1])
    dh = DiffusersHolder(p)
    dh.guidance_scale = 4.0
    emb = dh.get_text_embedding("a reef")
    assert torch.equal(emb[1], p.encode_prompt("x", negative_prompt="")[1])          # holder default "" -> encoded ""
    dh.set_negative_prompt(["ugly", "ignored second entry"])
    assert torch.equal(dh.get_text_embedding("a reef")[1], p.encode_prompt("x", negative_prompt="ugly")[1])


# ------------------------------------------------------------------ the guarded-buffer helper of the memory-contract tests
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64, torch.uint8, torch.int16])
def test_guard_helper_detects_every_kind_of_stray_or_missing_write(dtype):
    """tests/_guard.py on CPU tensors: a clean write passes; one element in a pad column, one in each guard and one valid element
    left unwritten each make the matching assertion raise (a checker that cannot fail checks nothing)."""
    from _guard import FRONT, guarded, poisoned
    rows, cols, ld = 5, 12, 20

    def fresh():
        view, chk = guarded(rows, cols, ld, dtype, "cpu", back_rows=3)
        assert view.shape == (rows, cols) and view.stride() == (ld, 1) and view.dtype == dtype
        assert chk.bits.numel() * chk.bits.element_size() % 256 == 0 and FRONT * chk.bits.element_size() % 256 == 0
        assert chk.bits.numel() - FRONT - rows * ld >= 3 * ld + 4096
        return view, chk, chk.bits.view(dtype)

    one = torch.ones((), dtype=dtype)
    view, chk, flat = fresh()
    chk.assert_intact("empty")
    chk.assert_untouched("empty")
    with pytest.raises(AssertionError, match="never written"):
        chk.assert_fully_written("empty")
    view.copy_(torch.arange(rows * cols).reshape(rows, cols).to(dtype))          # a clean write
    chk.assert_intact("clean")
    chk.assert_fully_written("clean")
    with pytest.raises(AssertionError, match="refused"):
        chk.assert_untouched("clean")
    # one valid element left unwritten
    view, chk, flat = fresh()
    view.fill_(1)
    flat[FRONT + 3 * ld + 7] = chk.bits.view(dtype)[0]
    with pytest.raises(AssertionError, match=r"1 element\(s\).*row 3, column 7"):
        chk.assert_fully_written("hole")
    chk.assert_intact("hole")
    # one element into a pad column, one into each guard
    for where, index, told in (("pad", FRONT + 2 * ld + cols, "row 2, column 12 (pad columns)"),
                               ("front", FRONT - 1, "row -1, column 19 (front guard)"),
                               ("back", FRONT + rows * ld, "row 5, column 0 (back guard)"),
                               ("back end", None, "back guard")):
        view, chk, flat = fresh()
        view.fill_(1)
        flat[flat.numel() - 1 if index is None else index] = one
        with pytest.raises(AssertionError) as err:
            chk.assert_intact(where)
        assert "1 element(s)" in str(err.value) and told in str(err.value), str(err.value)
        chk.assert_fully_written(where)
    # a second sentinel (uint8 outputs, where 0xA5 is a legal value)
    view, chk = guarded(rows, cols, ld, torch.uint8, "cpu", sentinel=0x5A)
    assert int(chk.bits[0]) == 0x5A and int(view[0, 0]) == 0x5A
    # poisoned operands: data inside, the pad value in the pad columns and in the rows behind
    if dtype.is_floating_point:
        t = torch.arange(rows * cols).reshape(rows, cols).to(dtype)
        v = poisoned(t, rows, cols, ld, float("nan"), extra_rows=4)
        assert v.stride() == (ld, 1) and torch.equal(v, t)
        whole = torch.as_strided(v, (rows + 4, ld), (ld, 1))
        assert torch.isnan(whole[:rows, cols:]).all() and torch.isnan(whole[rows:]).all()


# ------------------------------------------------------------------ the element-wise bound helper of the value-range tests
def test_elementwise_bound_sees_what_check_close_cannot():
    """tests/_parity.py: an error of twice the derived bound planted in ONE small element (|ref| < 1e-3) makes check_elementwise raise -
    naming the element - while the suite's check_close (2^-8 * max|ref| + floor) still passes: the gap the value-range tests close.
    An exact fp16 rounding of the reference passes both; a zero where the reference is a non-zero fp16 subnormal fails."""
    from _parity import absdot, check_close, check_elementwise, contraction_bound, norm_bound, store_bound
    g = torch.Generator().manual_seed(7)
    A = torch.randn(40, 64, generator=g).half().double()
    W = (torch.randn(24, 64, generator=g) * 64 ** -0.5).half().double()
    ref = A @ W.t()
    k = int(ref.abs().argmin())
    i, j = k // 24, k % 24
    ref[i, j] = 5e-4 if abs(float(ref[i, j])) >= 1e-3 else ref[i, j]
    assert abs(float(ref[i, j])) < 1e-3
    bound = contraction_bound(A, W, 64, ref)
    assert torch.equal(bound, contraction_bound(A, W, 64, ref, absdot64=absdot(A, W)))
    assert float(bound[i, j]) < 1e-4 and bool((bound > 0).all())
    log = {}
    exact = ref.half()
    assert check_elementwise(log, "exact", exact, ref, store_bound(ref)) <= 1.0          # round-to-nearest alone is inside its own term
    check_elementwise(log, "exact_full", exact, ref, bound)
    check_close(log, "exact_cc", exact, ref.float())
    planted = ref.clone()
    planted[i, j] += 2 * bound[i, j]
    check_close(log, "planted_cc", planted, ref.float())                                  # today's check cannot see it
    with pytest.raises(AssertionError, match=rf"1 of 960 elements.*\({i}, {j}\)"):
        check_elementwise(log, "planted", planted, ref, bound)
    assert log["planted"]["bad"] == 1 and 1.9 < log["planted"]["worst_err_over_bound"] < 2.1
    # a flushed subnormal: the reference is a non-zero fp16 subnormal, the output exactly zero
    sub = torch.full((4, 4), 3 * 2.0 ** -24, dtype=torch.float64)
    check_elementwise(log, "sub_exact", sub.half(), sub, store_bound(sub))
    with pytest.raises(AssertionError):
        check_elementwise(log, "sub_flushed", torch.zeros(4, 4, dtype=torch.float16), sub, store_bound(sub))
    # non-finite outputs fail; the norm bound is relative for large outputs and 2^-10 max|gamma| for small ones
    bad = exact.clone()
    bad[0, 0] = float("inf")
    with pytest.raises(AssertionError):
        check_elementwise(log, "inf", bad, ref, bound)
    nb = norm_bound(torch.tensor([0.0, 8.0], dtype=torch.float64), torch.tensor([0.5, -2.0]))
    assert torch.equal(nb, torch.tensor([2.0 ** -9, 2.0 ** -7 + 2.0 ** -9], dtype=torch.float64))
