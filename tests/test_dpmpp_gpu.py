"""The second-order sampler on a real MI355X: the DPM-Solver++ 2M step kernel (lb_dpmpp2m_step_f16) bit for bit
against the torch restatement in tests/_dpmpp_ref.py, its memory contract, a chain of steps, the unchanged DDIM bits of cfg 0 and
1, recorded / replayed / graph launches, and whole branched transitions under ``scheduler="dpmpp_2m"`` / ``"dpmpp_2m_karras"``.

Bars: the kernel's rounding sequence is the contract, so it is held to the restatement BIT FOR BIT; frames mean |du8| <= 2 and
>= 99 % within +-4; identical trees.
"""
import dataclasses
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pipe as OP  # noqa: E402  (checker only)
from oracle import sdxl_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _dpmpp_ref as DR  # noqa: E402
from _guard import guarded  # noqa: E402
from _parity import rnd  # noqa: E402

DEV = "cuda"
F16 = torch.float16
GOLD = os.path.join(HERE, "golden")
NAN = float("nan")

# per sample: (schedule length, Karras?, step index, first step of its run?, guidance) - a batch mixes a first-order row (a run
# entering at step 3), a second-order row and a schedule's last row; every sample under its own schedule and guidance
# (guidance 3.3 and 2.7: not exactly representable, so their product with an fp16 difference is inexact in fp32 and a CFG combine that
# rounded it once instead of twice would show - the pipe's mid-dampened guidances are such values)
MIXED = [(8, True, 3, True, 3.3), (20, True, 7, False, 4.0), (6, False, 5, False, 2.7)]
ALL_SECOND = [(8, True, 3, False, 3.0), (20, True, 7, False, 3.3), (6, False, 2, False, 2.5)]


def native():
    import latentblending_amd.native as n
    return n


def ops_mod():
    from latentblending_amd.hip import ops
    return ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def misaligned(t):
    """The same values behind a pointer that is off 16-byte alignment by 2 bytes (still contiguous)."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 2 and view.is_contiguous()
    return view


def native_rows(plan):
    from latentblending_amd.native.scheduler import NativeDPMSolverPP2MScheduler
    rows = []
    for n, karras, i, first, g in plan:
        s = NativeDPMSolverPP2MScheduler(use_karras_sigmas=karras, device="cpu")
        s.set_timesteps(n)
        rows.append(s.step_row(i, g, first=first))
    return rows


def reference(plan, state, eps, cfg):
    """Per sample: tests/_dpmpp_ref.py's fp16 step on the CPU, over ITS OWN float64 rows -> the [2, B, n] state after the step."""
    B = len(plan)
    ys, ms = [], []
    for b, (n, karras, i, first, g) in enumerate(plan):
        row = DR.row_f64(DR.sigmas_f64(n, karras), i, g, first=first)
        e = DR.cfg_combine_f16(eps[b:b + 1], eps[B + b:B + b + 1], g) if cfg else eps[b:b + 1]
        y, m0 = DR.dpmpp_step_f16(row, state[0, b:b + 1], e, state[1, b:b + 1])
        ys.append(y)
        ms.append(m0)
    return torch.stack([torch.cat(ys), torch.cat(ms)])


def inputs(batch, per_sample, seed):
    # latents as at a large sigma (magnitudes up to ~15), the previous x0 prediction of unit scale, eps N(0, 1)
    x = rnd(batch, per_sample, seed=seed, scale=4.0).clamp(-15, 15)
    m1 = rnd(batch, per_sample, seed=seed + 1, scale=1.5)
    return torch.stack([x, m1]), rnd(2 * batch, per_sample, seed=seed + 2)


def first_order_rows(plan):
    return [b for b, (n, _, i, first, _) in enumerate(plan) if first or i == 0 or i == n - 1]


# ================================================================== kernel bits and memory contract
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("per_sample,off16", [(256, False), (100, False), (8 * 33, True)])
def test_dpmpp_step_kernel_matches_the_restatement_bit_for_bit(per_sample, off16, cfg):
    """256: the vector body (32 lanes of 16 bytes); 100: the scalar form (100 % 8 != 0); 264 behind pointers misaligned by 2 bytes:
    the scalar form again, chosen by the pointers.  B = 3 with a first-order row, a second-order row and a schedule's last row in
    ONE batch; plane 1 of ``x`` is NaN for the first-order rows (not read); ``out`` sits between guard bands - front of plane 0,
    back of plane 1, the planes themselves adjoin by contract - and every element of both planes is written."""
    from latentblending_amd.hip import lib
    ops = ops_mod()
    B = 3
    for plan in (MIXED, ALL_SECOND):
        state, eps = inputs(B, per_sample, seed=2000 + per_sample)
        e = eps if cfg else eps[:B].contiguous()
        want = reference(plan, state, e, cfg)
        poisoned = state.clone()
        for b in first_order_rows(plan):
            poisoned[1, b] = NAN
        put = misaligned if off16 else (lambda t: t.to(DEV).contiguous())
        xd, ed = put(poisoned), put(e)
        out, chk = guarded(2 * B, per_sample, per_sample, F16, DEV, back_rows=4)
        params = ops.step_params(native_rows(plan), DEV)
        lib.api.lb_dpmpp2m_step_f16(xd.data_ptr(), ed.data_ptr(), out.data_ptr(), params.data_ptr(), per_sample, B,
                                    int(cfg), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        chk.assert_intact("dpmpp out")
        chk.assert_fully_written("dpmpp out")
        got = out.contiguous().view(2, B, per_sample)
        assert torch.isfinite(got).all()
        assert torch.equal(bits(got[1]), bits(want[1])), "x0 prediction (plane 1)"
        assert torch.equal(bits(got[0]), bits(want[0])), "next latent (plane 0)"
        # the wrapper makes the same launch
        got_w = ops.dpmpp2m_step(xd, ed, params, cfg=cfg)
        assert torch.equal(bits(got_w), bits(got))
        if plan is MIXED:                     # the last row returns its x0 prediction in both planes
            assert torch.equal(bits(got[0, 2]), bits(got[1, 2]))


@pytest.mark.parametrize("cfg", [False, True])
def test_misaligned_out_alone_selects_the_scalar_form(cfg):
    """``x`` and ``eps`` aligned, ``out`` 2 bytes off: the third term of the launcher's vector predicate.  (No guard bands here: the
    guarded view is always aligned; the scalar form's stores are under guard in the test above.)"""
    ops = ops_mod()
    B, n = 3, 8 * 33
    state, eps = inputs(B, n, seed=77)
    e = eps if cfg else eps[:B].contiguous()
    out = misaligned(torch.zeros(2, B, n, dtype=F16))
    got = ops.dpmpp2m_step(state.to(DEV), e.to(DEV), ops.step_params(native_rows(ALL_SECOND), DEV), cfg=cfg, out=out)
    assert got.data_ptr() == out.data_ptr() and out.data_ptr() % 16 == 2
    assert torch.equal(bits(got), bits(reference(ALL_SECOND, state, e, cfg)))


@pytest.mark.parametrize("cfg", [False, True])
def test_three_step_chain_feeding_out_back_as_x(cfg):
    """Steps 0, 1, 2 of a 3-step Karras schedule - first order, second order, last - with ``out`` of one step as ``x`` of the
    next, bit for bit against the restatement chained the same way (per-sample guidance; 8 * 37 + 3 elements: vector body never
    runs, 296: it does)."""
    ops = ops_mod()
    B = 2
    for per_sample in (296, 8 * 37 + 3):
        state, _ = inputs(B, per_sample, seed=31)
        state[1] = NAN                                          # no history yet
        want, got = state.clone(), state.to(DEV)
        for i in range(3):
            plan = [(3, True, i, False, 3.3), (3, True, i, False, 1.7)]
            eps = rnd(2 * B, per_sample, seed=40 + i)
            e = eps if cfg else eps[:B].contiguous()
            want = reference(plan, want, e, cfg)
            got = ops.dpmpp2m_step(got, e.to(DEV), ops.step_params(native_rows(plan), DEV), cfg=cfg)
            assert torch.isfinite(got).all()
            assert torch.equal(bits(got), bits(want)), f"step {i}"
        assert torch.equal(bits(got[0]), bits(got[1]))


def test_ddim_cfg_0_and_1_keep_the_parent_commits_bits():
    """tests/golden/dpmpp_ddim_parent_bits.json: lb_ddim_step_f16 with cfg 0 and 1 (vector and scalar form) as the commit before
    the DPM-Solver++ 2M step existed computed them on an MI355X, on one fixed seeded input."""
    ops = ops_mod()
    with open(os.path.join(GOLD, "dpmpp_ddim_parent_bits.json")) as fh:
        gold = json.load(fh)
    inp = gold["input"]
    B = inp["B"]
    for n in inp["sizes"]:
        x, eps = rnd(B, n, seed=inp["seed_x"], scale=inp["scale_x"]).to(DEV), rnd(2 * B, n, seed=inp["seed_eps"]).to(DEV)
        p = ops.step_params(inp["rows"], DEV)
        for cfg in (0, 1):
            e = eps if cfg else eps[:B].contiguous()
            o = ops.ddim_step(x, e, p, cfg=bool(cfg))
            assert bits(o).flatten().tolist() == gold["cases"][f"n{n}_cfg{cfg}"]


def test_unknown_cfg_bits_are_refused_before_any_launch():
    from latentblending_amd.hip import lib
    ops = ops_mod()
    B, n = 3, 256
    state, eps = inputs(B, n, seed=9)
    xd, ed = state.to(DEV), eps[:B].contiguous().to(DEV)
    params = ops.step_params(native_rows(MIXED), DEV)
    out, chk = guarded(2 * B, n, n, F16, DEV, back_rows=2)
    s = torch.cuda.current_stream().cuda_stream
    for bad in (4, 6, 7):
        with pytest.raises(RuntimeError, match="lb_ddim_step_f16: cfg bits"):
            lib.api.lb_ddim_step_f16(xd.data_ptr(), ed.data_ptr(), out.data_ptr(), params.data_ptr(), n, B, bad, s)
        with pytest.raises(RuntimeError, match="lb_dpmpp2m_step_f16: cfg bits"):
            lib.api.lb_dpmpp2m_step_f16(xd.data_ptr(), ed.data_ptr(), out.data_ptr(), params.data_ptr(), n, B, bad, s)
    for bad in (2, 3):              # what used to select this step on the DDIM symbol: refused there, and no CFG value here
        with pytest.raises(RuntimeError, match="lb_dpmpp2m_step_f16"):
            lib.api.lb_ddim_step_f16(xd.data_ptr(), ed.data_ptr(), out.data_ptr(), params.data_ptr(), n, B, bad, s)
        with pytest.raises(RuntimeError, match="lb_dpmpp2m_step_f16: cfg bits"):
            lib.api.lb_dpmpp2m_step_f16(xd.data_ptr(), ed.data_ptr(), out.data_ptr(), params.data_ptr(), n, B, bad, s)
    with pytest.raises(ValueError, match="aliases"):
        ops.dpmpp2m_step(xd, ed, params, out=xd)
    torch.cuda.synchronize()
    chk.assert_untouched("out of the refused calls")


# ================================================================== program layer
def test_dpmpp_step_recorded_replayed_and_graph_launched():
    """The ``dpmpp_steps`` case of the registry in tests/_replay.py (plain, CFG, and ``out`` of op 0 as ``state`` of op 2) through
    the whole replay protocol (two direct launches, a recording that launches nothing, eager replay, every run_range split,
    hipGraph on two streams, time_ops, and new parameter rows in the same device buffers), recorded under the launcher's own
    name - and then this file's own check: the direct launches the protocol compared everything with are the right answer."""
    import _replay as RP
    c = RP.build_case("dpmpp_steps")
    assert c.ops == ["lb_dpmpp2m_step_f16"] * 3
    B, n, x, e, outs = (c.operands[k] for k in ("B", "n", "state", "eps", "outs"))
    assert (B, n) == (3, 8 * 37) and sorted(outs) == ["dpmpp", "dpmpp_cfg", "dpmpp_chained"]
    # (recorded on a mixed batch; rewritten to other steps of the schedules: every row second order then)
    assert RP.DPMPP_PLANS["recorded"] == MIXED and RP.DPMPP_PLANS["rewritten"] == ALL_SECOND
    state, eps = inputs(B, n, seed=15)
    assert torch.equal(bits(x), bits(state)) and torch.equal(bits(e), bits(eps))
    rec = RP.run_protocol(c, RP.GpuDriver())
    print("[dpmpp] " + RP.format_record(rec))
    assert rec["eager"] == rec["graph"] == rec["graph_s2"] == rec["new_values"] == "equal"
    # ... and the direct launch the protocol compared everything with is the right answer (the protocol leaves the rows of its
    # last stage, the rewritten ones, in the parameter buffer)
    c.restore()
    c.thunk()
    torch.cuda.synchronize()
    want = reference(ALL_SECOND, x.cpu(), e.cpu()[:B], False)
    assert torch.equal(bits(outs["dpmpp"].contiguous().view(2, B, n)), bits(want))
    want_cfg = reference(ALL_SECOND, x.cpu(), e.cpu(), True)
    assert torch.equal(bits(outs["dpmpp_cfg"].contiguous().view(2, B, n)), bits(want_cfg))
    want_chained = reference(ALL_SECOND, want, e.cpu()[:B], False)
    assert torch.equal(bits(outs["dpmpp_chained"].contiguous().view(2, B, n)), bits(want_chained))


# ================================================================== whole transitions
def tiny_cfgs():
    n = native()
    return dict(unet_cfg=n.UNetConfig(**dataclasses.asdict(R.tiny_unet_cfg())), vae_cfg=n.VAEConfig(**dataclasses.asdict(R.tiny_vae_cfg())))


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def frame_diff(a, b):
    return np.stack([np.abs(np.asarray(x).astype(np.int32) - np.asarray(y).astype(np.int32)) for x, y in zip(a, b)])


def within_frame_bar(d):
    return d.mean() <= 2 and (d <= 4).mean() >= 0.99


@pytest.fixture(scope="module")
def oracle_base_transition():
    """The CPU side of the base-model transition, computed once for both frontiers (the sampler is deterministic: the order in
    which an engine evaluates its branches does not reach the result)."""
    from latentblending_amd import BlendingEngine
    from latentblending_amd.backend import set_backend
    o = OP.StableDiffusionXLPipeline(turbo=False, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg(), seed=0)
    o.scheduler = DR.DPMPPRefScheduler(use_karras_sigmas=True)
    np.random.seed(0)
    set_backend(R.TorchCpuBackend())
    be = BlendingEngine(o, metric=R.OracleLPIPS(7), verbose=False)
    _setup_base(be)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(os.cpu_count() or 1, 8))          # (tiny-width CPU oracle)
    try:
        imgs = be.run_transition(fixed_seeds=[420, 421])
    finally:
        torch.set_num_threads(threads)
        set_backend(None)
    return be, [np.asarray(i) for i in imgs]


def _setup_base(be):
    be.set_dimensions((128, 128))
    be.set_num_inference_steps(6)
    be.set_guidance_scale(3.0)
    be.set_branching(depth_strength=0.5, nmb_max_branches=5)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")


@pytest.mark.parametrize("frontier", [1, 8])
def test_transition_with_dpmpp_2m_karras_matches_oracle(frontier, oracle_base_transition, results_log):
    """The whole branched transition under DPM-Solver++ 2M on Karras sigmas: NativeSDXLPipe(scheduler="dpmpp_2m_karras") through
    the native batched loops against the engine on the CPU oracle pipe carrying DPMPPRefScheduler under the generic step-by-step
    loop.  Base model, 6 steps, guidance 3.0 (CFG; mid-dampened per branch), two injection levels: every branch entering at
    ``idx_start > 0`` starts first order on both sides."""
    from latentblending_amd import BlendingEngine
    from latentblending_amd.backend import set_backend
    n = native()
    be_o, imgs_o = oracle_base_transition
    p = n.NativeSDXLPipe(turbo=False, seed=0, scheduler="dpmpp_2m_karras", allow_synthetic=True, **tiny_cfgs())
    assert p.scheduler.kind == "dpmpp_2m" and p.scheduler.use_karras_sigmas and p.scheduler.init_noise_sigma == 1.0
    set_backend(None)
    np.random.seed(0)
    be_p = BlendingEngine(p, verbose=False, do_compile=True, frontier_width=frontier)
    _setup_base(be_p)
    imgs_p = be_p.run_transition(fixed_seeds=[420, 421])
    assert len(imgs_o) == len(imgs_p) and be_o.tree_fracts == be_p.tree_fracts and be_o.tree_idx_injection == be_p.tree_idx_injection
    assert len(set(be_p.tree_idx_injection)) >= 3, "anchors plus two injection levels"
    assert all(t[-1].shape == (1, 4, 16, 16) for t in be_p.tree_latents), "stored trajectories are latents only"
    lat_err = max(rel_l2(a[-1], b[-1]) for a, b in zip(be_p.tree_latents, be_o.tree_latents))
    d = frame_diff(imgs_p, imgs_o)
    results_log[f"transition_dpmpp_karras_frontier{frontier}"] = {"frames": len(imgs_p), "final_latent_rel_l2": lat_err,
                                                                 "mean_abs_u8": float(d.mean()), "frac_within_4": float((d <= 4).mean()),
                                                                 "same_tree": True}
    print(f"[parity] DPM++ 2M Karras transition frontier {frontier}: frames={len(imgs_p)} levels={sorted(set(be_p.tree_idx_injection))} "
          f"latent rel_l2={lat_err:.3e} mean|du8|={d.mean():.3f} within4={(d <= 4).mean():.4f}")
    assert within_frame_bar(d)


def test_turbo_defaults_through_the_fused_wavefront_and_ignored_elision(results_log):
    """Turbo branching defaults (injection at step 2 of 4) under ``scheduler="dpmpp_2m"``: at frontier 8 the fused wavefront's
    batch grows at ``idx_injection`` - the anchors carry their histories over (second-order rows), the mids enter without
    (first-order rows), in ONE launch - against the same run at frontier 1, where every branch is a run of its own.  Then
    ``elide_dead_steps``: a skipped step would leave no x0 prediction behind, so it is ignored with one warning - same bits, same
    number of UNet samples."""
    from latentblending_amd import BlendingEngine
    from latentblending_amd.backend import set_backend
    n = native()
    set_backend(None)
    p = n.NativeSDXLPipe(turbo=True, seed=0, scheduler="dpmpp_2m", allow_synthetic=True, **tiny_cfgs())
    assert p.scheduler.kind == "dpmpp_2m" and not p.scheduler.use_karras_sigmas

    def run(frontier, elide=False):
        np.random.seed(0)
        be = BlendingEngine(p, verbose=False, do_compile=True, frontier_width=frontier)
        be.elide_dead_steps = elide
        be.set_dimensions((128, 128))
        be.set_num_inference_steps(4)
        be.set_branching(nmb_max_branches=5)
        be.set_prompt1("photo of a reef")
        be.set_prompt2("rendering of an alien planet")
        p.stats["unet_samples"] = 0
        frames = [np.asarray(f) for f in be.run_transition(fixed_seeds=[420, 421])]
        return be, frames, p.stats["unet_samples"]
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="elide_dead_steps")          # (nothing of the kind without the switch)
        be1, seq, _ = run(1)
        be8, fused, samples = run(8)
    assert sorted(set(be8.tree_idx_injection)) == [0, 2]
    assert be1.tree_fracts == be8.tree_fracts and be1.tree_idx_injection == be8.tree_idx_injection
    d = frame_diff(fused, seq)
    results_log["transition_dpmpp_wavefront_vs_sequential"] = {"mean_abs_u8": float(d.mean()), "frac_within_4": float((d <= 4).mean())}
    print(f"[parity] DPM++ 2M fused wavefront vs frontier 1: mean|du8|={d.mean():.3f} within4={(d <= 4).mean():.4f}")
    assert within_frame_bar(d)
    with pytest.warns(UserWarning, match="elide_dead_steps is ignored under the multistep sampler"):
        _, elided, samples_elided = run(8, elide=True)
    assert samples_elided == samples
    assert len(elided) == len(fused) and all(np.array_equal(a, b) for a, b in zip(fused, elided))
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="elide_dead_steps")          # (once per pipe)
        run(8, elide=True)


def test_recycled_anchor_and_precomputed_keyframes_under_dpmpp(results_log):
    """A chain of two transitions under ``scheduler="dpmpp_2m_karras"`` (base config: CFG, deterministic): the loop of the
    reference's multi-transition example written out by hand at frontier 1 (every run on its own), the same loop at frontier 4
    (the fused wavefront takes the recycled anchor's stored trajectory as ``known_anchors`` and carries only the new anchor's
    history), and replay.run_multi_transition(pipeline_keyframes=True) (all key frames denoised ahead as one lock-step batch, both
    anchors of every transition known: the wavefront's big batches hold first-order mids only at the injection step).  Same
    trees, the shared key frame handed through bit for bit, frames inside the frame bar (batch composition rounds differently)."""
    from latentblending_amd import BlendingEngine, replay
    from latentblending_amd.backend import set_backend
    n = native()
    set_backend(None)
    p = n.NativeSDXLPipe(turbo=False, seed=0, scheduler="dpmpp_2m_karras", allow_synthetic=True, **tiny_cfgs())
    prompts = ["a reef", "an alien planet", "a city at night"]
    seeds = [11, 12, 13]

    def engine(frontier):
        np.random.seed(0)
        be = BlendingEngine(p, verbose=False, do_compile=True, frontier_width=frontier)
        be.set_dimensions((128, 128))
        be.set_num_inference_steps(4)
        be.set_guidance_scale(3.0)
        be.set_branching(depth_strength=0.5, nmb_max_branches=3)
        return be

    def by_hand(frontier):
        be = engine(frontier)
        segs, trees = [], []
        for i in range(2):
            if i == 0:
                be.set_prompt1(prompts[0])
                be.set_prompt2(prompts[1])
            else:
                be.guidance_scale = be.dh.guidance_scale = 3.0       # (the loop's quirk, removed: see test_host_cpu.py)
                be.swap_forward()
                be.set_prompt2(prompts[i + 1])
            segs.append([np.asarray(f) for f in be.run_transition(recycle_img1=i > 0, fixed_seeds=seeds[i:i + 2])])
            trees.append((list(be.tree_fracts), list(be.tree_idx_injection)))
        return segs, trees
    hand, trees = by_hand(1)
    fused, trees_f = by_hand(4)
    be = engine(4)
    piped = [[np.asarray(f) for f in seg] for seg in replay.run_multi_transition(be, prompts, seeds, None, pipeline_keyframes=True)]
    assert be.stats["keyframes_precomputed"] == 3 and trees == trees_f
    for name, segs in (("recycled anchor, fused", fused), ("precomputed key frames", piped)):
        assert len(segs) == 2 and [len(s) for s in segs] == [len(s) for s in hand]
        assert np.array_equal(segs[0][-1], segs[1][0]), "the shared key frame"
        d = frame_diff(segs[0] + segs[1], hand[0] + hand[1])
        results_log[f"dpmpp_chain_{name.split(',')[0].replace(' ', '_')}"] = {"mean_abs_u8": float(d.mean()), "frac_within_4": float((d <= 4).mean())}
        print(f"[parity] DPM++ 2M chain, {name} vs hand-written loop: mean|du8|={d.mean():.3f} within4={(d <= 4).mean():.4f}")
        assert within_frame_bar(d)


def test_native_run_entering_at_idx_start_2_starts_first_order_and_carries_its_history():
    """The restart rule in the native loop itself (``native_run_diffusion_batch``), seen at the scheduler's ``device_step``: a run
    entering at step 2 of 5 launches a first-order row, then a second-order row whose history plane is the x0 prediction the
    step before left (``out`` of step i IS ``x`` of step i + 1), then the schedule's last row; a crossfeed mix in between changes
    the latent plane only; and a second run starts without history again."""
    from latentblending_amd import DiffusersHolder
    from latentblending_amd.backend import set_backend
    n = native()
    set_backend(None)
    p = n.NativeSDXLPipe(turbo=True, seed=0, scheduler="dpmpp_2m_karras", allow_synthetic=True, **tiny_cfgs())
    dh = DiffusersHolder(p)
    dh.set_dimensions((128, 128))
    dh.set_num_inference_steps(5)
    emb = dh.get_text_embedding("a reef")
    full = dh.run_diffusion(emb, dh.get_noise(11), idx_start=0)
    other = dh.run_diffusion(dh.get_text_embedding("an alien planet"), dh.get_noise(12), idx_start=0)
    calls = []
    inner = p.scheduler.device_step

    def spy(state, eps, params, noise=None, cfg=False, out=None):
        got = inner(state, eps, params, noise=noise, cfg=cfg, out=out)
        calls.append((state.clone(), params.cpu().clone(), got.clone()))
        return got
    p.scheduler.device_step = spy
    try:
        for coeffs in ([0.0] * 5, [0.0, 0.0, 0.0, 0.5, 0.0]):
            calls.clear()
            traj = dh.run_diffusion(emb, full[1], idx_start=2, list_latents_mixing=other, mixing_coeffs=coeffs)
            assert traj[:2] == [None, None] and len(calls) == 3
            (s2, r2, o2), (s3, r3, o3), (s4, r4, o4) = calls
            assert r2[0, 5] == 0 and r2[0, 7] == 0 and r2[0, 2] != 0, "first executed step: a first-order row"
            assert r3[0, 5] != 0 and r3[0, 5] == 0.5 * r3[0, 4] and r3[0, 7] > 0, "then a second-order row"
            assert r4[0, 2] == 0 and r4[0, 4] == -1 and r4[0, 5] == 0, "then the schedule's last row"
            assert torch.equal(bits(s2[0]), bits(full[1]))
            assert torch.equal(bits(s3[1]), bits(o2[1])) and torch.equal(bits(s4[1]), bits(o3[1])), "history = the previous x0 prediction"
            assert torch.equal(bits(s4[0]), bits(o3[0]))
            if coeffs[3] == 0:
                assert torch.equal(bits(s3[0]), bits(o2[0]))
            else:
                assert not torch.equal(bits(s3[0]), bits(o2[0])), "the mix reached the latent plane"
            for i, o in zip((2, 3, 4), (o2, o3, o4)):
                assert traj[i].shape == (1, 4, 16, 16) and torch.equal(bits(traj[i]), bits(o[0]))
                assert traj[i].untyped_storage().nbytes() == traj[i].numel() * 2, "a stored latent pins no x0-prediction plane"
            # the same step taken with history gives another result: the rule is visible in the bits
            assert not torch.equal(bits(traj[2]), bits(full[2]))
    finally:
        p.scheduler.device_step = inner
