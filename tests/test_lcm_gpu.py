"""The few-step path on a real MI355X: the latent-consistency step kernel (lb_lcm_step_f16) bit for bit against the
torch restatement in tests/_lcm_ref.py, its memory contract, recorded / replayed / graph launches, the refusal of a null noise
pointer, the guidance-embedded UNet against the unchanged oracle, and the whole branched transition under ``scheduler="lcm"``.

Bars: DESIGN.md section 1 parity bar for a restated fp16 step (<= 1 fp16 ulp; the rounding sequence is the same on both sides, so
bit equality is what is expected and the observed maximum is printed); UNet forward rel-L2 <= 1e-2; frames mean |du8| <= 2 and
>= 99 % within +-4; identical trees.
"""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pipe as OP  # noqa: E402  (checker only)
from oracle import sdxl_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _lcm_ref as LR  # noqa: E402
from _guard import guarded, poisoned  # noqa: E402
from _parity import rnd, ulp_diff_f16  # noqa: E402

DEV = "cuda"
F16 = torch.float16
GOLD = os.path.join(HERE, "golden")
NAN = float("nan")

# (schedule length, guidance) per sample: every sample of a batch runs under its own schedule, so that its row differs from the
# others' in every slot that matters (abar_prev at the first step, everything at the later ones)
SAMPLES = [(4, 3.0), (8, 3.5), (3, 4.0)]
WHICH = {"first": lambda n: 0, "middle": lambda n: n // 2, "last": lambda n: n - 1}


def native():
    import latentblending_amd.native as n
    return n


def ops_mod():
    from latentblending_amd.hip import ops
    return ops


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def misaligned(t):
    """The same values behind a pointer that is off 16-byte alignment by 2 bytes (still contiguous)."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 2 and view.is_contiguous()
    return view


def step_indices(batch, which):
    """[(schedule length, step index, guidance)] per sample; ``which`` is "first" / "middle" / "last" or one such word per sample."""
    words = [which] * batch if isinstance(which, str) else list(which)
    return [(n, WHICH[w](n), g) for (n, g), w in zip(SAMPLES[:batch], words)]


def native_rows(plan):
    from latentblending_amd.native.scheduler import NativeLCMScheduler
    rows = []
    for n, i, g in plan:
        s = NativeLCMScheduler(device="cpu")
        s.set_timesteps(n)
        rows.append(s.step_row(i, g))
    return rows


def reference(plan, x, eps, noise, cfg):
    """Per sample: LCMRefScheduler's step on the CPU (fp16 tensors); ``noise`` None = not needed (last steps only)."""
    B = len(plan)
    outs = []
    for b, (n, i, g) in enumerate(plan):
        ref = LR.LCMRefScheduler()
        ref.set_timesteps(n)
        e = LR.cfg_combine_f16(eps[b:b + 1], eps[B + b:B + b + 1], g) if cfg else eps[b:b + 1]
        outs.append(ref.denoise_and_renoise(i, e, x[b:b + 1], None if noise is None else noise[b:b + 1]))
    return torch.cat(outs)


def inputs(batch, per_sample, seed):
    # x as a latent at t = 999 under a large start value: magnitudes up to ~15; eps and noise N(0, 1)
    x = rnd(batch, per_sample, seed=seed, scale=4.0).clamp(-15, 15)
    return x, rnd(2 * batch, per_sample, seed=seed + 1), rnd(batch, per_sample, seed=seed + 2)


# ================================================================== kernel bits
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("per_sample,off16", [(8, False), (296, False), (4 * 8 * 8 + 3, True)])
def test_lcm_step_kernel_matches_the_restatement_bit_for_bit(per_sample, off16, batch, cfg, results_log):
    """8: one lane of the vector body; 296: 37 lanes of it (the vector form needs per_sample % 8 == 0, so its scalar tail loop runs
    zero times in both); 259 through pointers misaligned by 2 bytes: the scalar loop alone.  First, middle and last steps of
    per-sample schedules; the last step also with ``noise=None``."""
    ops = ops_mod()
    worst = 0
    for which in ("first", "middle", "last"):
        plan = step_indices(batch, which)
        x, eps, noise = inputs(batch, per_sample, seed=1000 + per_sample + 7 * batch)
        e = eps if cfg else eps[:batch]
        want = reference(plan, x, e, noise, cfg)
        put = misaligned if off16 else (lambda t: t.to(DEV).contiguous())
        xd, ed, nd = put(x), put(e.contiguous()), put(noise)
        params = ops.step_params(native_rows(plan), DEV)
        got = ops.lcm_step(xd, ed, params, noise=nd, cfg=cfg)
        d = ulp_diff_f16(got, want)
        worst = max(worst, d)
        print(f"[lcm] per_sample={per_sample} batch={batch} cfg={int(cfg)} step={which}: max ulp diff {d}")
        assert torch.isfinite(got).all() and d <= 1
        if which == "last":
            got_null = ops.lcm_step(xd, ed, params, noise=None, cfg=cfg)
            assert torch.equal(got_null.cpu().view(torch.int16), got.cpu().view(torch.int16))
    results_log[f"lcm_step_ulp_n{per_sample}_B{batch}_cfg{int(cfg)}"] = worst


def test_lcm_last_step_rows_return_the_denoised_latent_bit_for_bit(results_log):
    """A batch that mixes last and non-last rows: the last-step rows are `den` bit for bit - a negative zero included - and do not
    read their noise (NaN there); the other row takes its noise."""
    ops = ops_mod()
    B, n = 3, 296
    plan = step_indices(B, ["last", "middle", "last"])
    x, eps, noise = inputs(B, n, seed=77)
    x[2, :4], eps[2, :4] = -0.0, 0.0                       # t1 = +0, t2 = -0 - +0 = -0, x0 = d1 = d2 = -0, den = -0 + -0 = -0
    eps = eps[:B].contiguous()
    noise[0], noise[2] = NAN, NAN
    want = reference(plan, x, eps, noise, False)
    for b in (0, 2):
        ref = LR.LCMRefScheduler()
        ref.set_timesteps(plan[b][0])
        den = ref.denoised(plan[b][1], eps[b:b + 1], x[b:b + 1])
        assert torch.equal(want[b:b + 1].view(torch.int16), den.view(torch.int16))
    assert want[2, :4].view(torch.int16).tolist() == [-32768] * 4            # 0x8000: the reference itself yields -0 there
    got = ops.lcm_step(x.to(DEV), eps.to(DEV), ops.step_params(native_rows(plan), DEV), noise=noise.to(DEV)).cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16))
    assert torch.equal(got[2].view(torch.int16), want[2].view(torch.int16))
    d = ulp_diff_f16(got[1], want[1])
    results_log["lcm_step_mixed_rows_ulp"] = d
    print(f"[lcm] mixed last / non-last batch: non-last row max ulp diff {d}")
    assert d <= 1


# ================================================================== memory contract
@pytest.mark.parametrize("per_sample", [296, 4 * 8 * 8 + 3])
@pytest.mark.parametrize("cfg", [False, True])
def test_lcm_step_memory_contract(per_sample, cfg):
    """Guard bands around ``out``, NaN rows behind every operand, NaN noise for the last-step rows: everything inside ``out`` is
    written, nothing outside is, and no NaN reaches the result."""
    from latentblending_amd.hip import lib
    ops = ops_mod()
    B = 3
    plan = step_indices(B, ["last", "first", "last"])
    x, eps, noise = inputs(B, per_sample, seed=5)
    e = eps if cfg else eps[:B].contiguous()
    noise[0], noise[2] = NAN, NAN
    want = reference(plan, x, e, noise, cfg)
    xd = poisoned(x, B, per_sample, per_sample, NAN, DEV, extra_rows=4)
    ed = poisoned(e, e.shape[0], per_sample, per_sample, NAN, DEV, extra_rows=4)
    nd = poisoned(noise, B, per_sample, per_sample, NAN, DEV, extra_rows=4)
    out, chk = guarded(B, per_sample, per_sample, F16, DEV, back_rows=4)
    params = ops.step_params(native_rows(plan), DEV)
    lib.api.lb_lcm_step_f16(xd.data_ptr(), ed.data_ptr(), nd.data_ptr(), out.data_ptr(), params.data_ptr(), per_sample, B,
                            int(cfg), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    chk.assert_intact("lcm out")
    chk.assert_fully_written("lcm out")
    assert torch.isfinite(out).all()
    assert ulp_diff_f16(out.contiguous(), want) <= 1


# ================================================================== program layer
def test_lcm_step_recorded_replayed_and_graph_launched():
    """The ``lcm_steps`` case of the registry in tests/_replay.py (plain, CFG, last-step rows with a null noise pointer) through the
    whole replay protocol (two direct launches, a recording that launches nothing, eager replay, every run_range split, hipGraph
    on two streams, time_ops, and new parameter rows in the same device buffers), recorded under the launcher's own name - and
    then this file's own check: the direct launch the protocol compared everything with is the right answer."""
    import _replay as RP
    c = RP.build_case("lcm_steps")
    assert c.ops == ["lb_lcm_step_f16"] * 3
    B, n, x, eps, noise, outs = (c.operands[k] for k in ("B", "n", "x", "eps", "noise", "outs"))
    assert (B, n) == (2, 8 * 37 + 3) and sorted(outs) == ["lcm", "lcm_cfg", "lcm_last_null_noise"]
    assert RP.LCM_PLANS["recorded"] == step_indices(B, "middle") and RP.LCM_PLANS["recorded_last"] == step_indices(B, "last")
    # (rewritten to another step of each schedule; the null-noise launch keeps last-step rows: ``all_last`` was recorded)
    assert RP.LCM_PLANS["rewritten"] == step_indices(B, "first") and RP.LCM_PLANS["rewritten_last"] == [(8, 7, 2.0), (3, 2, 2.0)]
    rec = RP.run_protocol(c, RP.GpuDriver())
    print("[lcm] " + RP.format_record(rec))
    assert rec["eager"] == rec["graph"] == rec["graph_s2"] == rec["new_values"] == "equal"
    # ... and the direct launch the protocol compared everything with is the right answer
    c.restore()
    c.thunk()
    torch.cuda.synchronize()
    want = reference(step_indices(B, "first"), x.cpu(), eps.cpu()[:B], noise.cpu(), False)
    assert ulp_diff_f16(outs["lcm"].contiguous(), want) <= 1


# ================================================================== refusal, and the Euler step's bits
def test_lcm_null_noise_with_a_non_last_row_is_refused_before_any_launch():
    from latentblending_amd.hip import lib
    from latentblending_amd.native.runtime import Program
    ops = ops_mod()
    B, n = 3, 296
    x, eps, _ = inputs(B, n, seed=9)
    xd, ed = x.to(DEV), eps[:B].contiguous().to(DEV)
    params = ops.step_params(native_rows(step_indices(B, ["last", "middle", "last"])), DEV)
    prog = Program("lcm-refusal")
    with prog.record():             # (a launcher that got as far as its dispatch would leave an op in the recording)
        with pytest.raises(ValueError, match="last step"):
            ops.lcm_step(xd, ed, params, noise=None)
        with pytest.raises(ValueError, match="host rows hold a step that is not the last"):
            ops.lcm_step(xd, ed, params, noise=None, all_last=True)
        with pytest.raises(ValueError, match="cannot be established"):
            ops.lcm_step(xd, ed, params.view(B, 8)[:], noise=None)          # a view: no host mirror, no statement
    assert prog.num_ops == 0
    out, chk = guarded(B, n, n, F16, DEV, back_rows=2)
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="lb_lcm_step_f16: .*needs noise"):
        lib.api.lb_lcm_step_f16(xd.data_ptr(), ed.data_ptr(), None, out.data_ptr(), params.data_ptr(), n, B, 0, 0, s)
    with pytest.raises(RuntimeError, match="ancestral step needs noise"):
        lib.api.lb_euler_step_f16(xd.data_ptr(), ed.data_ptr(), None, out.data_ptr(), params.data_ptr(), n, B, 0, 1, s)
    with pytest.raises(RuntimeError, match="lb_euler_step_f16: ancestral is 0 or 1"):
        lib.api.lb_euler_step_f16(xd.data_ptr(), ed.data_ptr(), None, out.data_ptr(), params.data_ptr(), n, B, 0, 3, s)
    with pytest.raises(RuntimeError, match="lb_lcm_step_f16"):         # what used to select this step on the Euler symbol
        lib.api.lb_euler_step_f16(xd.data_ptr(), ed.data_ptr(), None, out.data_ptr(), params.data_ptr(), n, B, 0, 2, s)
    torch.cuda.synchronize()
    chk.assert_untouched("out of the refused calls")


def test_euler_modes_0_and_1_keep_the_parent_commits_bits():
    """tests/golden/lcm_euler_modes.json: lb_euler_step_f16 plain and ancestral (vector and scalar form, with and without CFG) as the
    commit before the latent-consistency step existed computed them on an MI355X, on one fixed input."""
    ops = ops_mod()
    with open(os.path.join(GOLD, "lcm_euler_modes.json")) as fh:
        gold = json.load(fh)
    B = gold["input"]["B"]
    for n in (296, 299):
        x, eps, noise = rnd(B, n, seed=151, scale=5.0).to(DEV), rnd(2 * B, n, seed=152).to(DEV), rnd(B, n, seed=153).to(DEV)
        pe = ops.step_params(gold["input"]["rows_euler"], DEV)
        pa = ops.step_params(gold["input"]["rows_ancestral"], DEV)
        for cfg in (False, True):
            e = eps if cfg else eps[:B].contiguous()
            o0 = ops.euler_step(x, e, pe, noise=None, cfg=cfg, ancestral=False)
            o1 = ops.euler_step(x, e, pa, noise=noise, cfg=cfg, ancestral=True)
            assert o0.cpu().view(torch.int16).flatten().tolist() == gold["cases"][f"n{n}_cfg{int(cfg)}_mode0"]
            assert o1.cpu().view(torch.int16).flatten().tolist() == gold["cases"][f"n{n}_cfg{int(cfg)}_mode1"]


# ================================================================== guidance-embedded UNet
TCOND = 32


def guided_cfg():
    return dataclasses.replace(R.tiny_unet_cfg(), time_cond_proj_dim=TCOND)


def cond_proj_weight(seed=0):
    """Wc as the native UNet draws it (SyntheticProvider: values depend on (name, seed) only), fp32 [C0, TCOND]."""
    cfg = R.tiny_unet_cfg()
    return native().SyntheticProvider(seed).weight("time_embedding.cond_proj.weight", (cfg.block_channels[0], TCOND), TCOND)


def weights_with_guidance(w, wc, guidance):
    """The identity linear_1(tsin + c) = linear_1(tsin) + W1 c: the UNCHANGED oracle computes the guidance-embedded UNet when
    linear_1's bias is replaced by b1 + W1 (Wc emb(w)), in fp32.  emb is rounded to fp16 first: that is the input the UNet gets
    (diffusers_holder.py casts it to the latents' dtype)."""
    emb = torch.from_numpy(LR.guidance_embedding_f64([guidance - 1.0], TCOND)).float().half().float()[0]
    w2 = dict(w)
    w2["time_embedding.linear_1.bias"] = w["time_embedding.linear_1.bias"].float() + w["time_embedding.linear_1.weight"].float() @ (wc @ emb)
    return w2


@pytest.mark.parametrize("B", [1, 3])
def test_guidance_embedded_unet_matches_oracle_through_the_bias_identity(B, results_log):
    n = native()
    L = 8
    plain, guided = R.tiny_unet_cfg(), guided_cfg()
    w = R.make_weights(R.unet_spec(plain), 0)
    wc = cond_proj_weight(0)
    net_g = n.NativeUNet(n.UNetConfig(**dataclasses.asdict(guided)), n.SyntheticProvider(0), DEV)
    net_p = n.NativeUNet(n.UNetConfig(**dataclasses.asdict(plain)), n.SyntheticProvider(0), DEV)
    assert tuple(net_g.w["time_embedding.cond_proj.weight"].shape) == (plain.block_channels[0], TCOND)
    assert "time_embedding.cond_proj.weight" not in net_p.w
    g = torch.Generator().manual_seed(B * 10 + L)
    x = torch.randn(B, 4, L, L, generator=g).half()
    ctx = torch.randn(B, 77, plain.cross_dim, generator=g).half()
    te = torch.randn(B, plain.pooled_dim, generator=g).half()
    ids = torch.tensor([[128.0, 128.0, 0.0, 0.0, 128.0, 128.0]] * B)
    guidance = [3.0, 1.0, 8.0][:B]
    ref = torch.cat([R.unet_forward(plain, weights_with_guidance(w, wc, guidance[b]), x[b:b + 1], torch.tensor(499.0),
                                    ctx[b:b + 1], te[b:b + 1], ids[b:b + 1]) for b in range(B)])
    ref_plain = R.unet_forward(plain, w, x, torch.tensor(499.0), ctx, te, ids)
    prog = net_g.build(B, L)
    emb = n.NativeSDXLPipe.get_guidance_scale_embedding([v - 1.0 for v in guidance], embedding_dim=TCOND).to(DEV, F16)
    prog.set_conditioning(ctx.to(DEV), te.to(DEV), ids.to(DEV), timestep_cond=emb)
    got = prog.forward(x.to(DEV), torch.full((B,), 499.0)).clone()
    r = rel_l2(got, ref)
    moved = rel_l2(ref, ref_plain)
    results_log[f"unet_guided_B{B}_rel_l2"] = r
    print(f"[lcm] guidance-embedded unet B={B}: rel_l2={r:.3e} (the embedding moves the output by rel_l2={moved:.3e})")
    assert torch.isfinite(got).all() and r <= 1e-2
    assert moved > 5 * 1e-2, "the guidance embedding does not move the oracle's output: the case proves nothing"
    # eager == graph
    prog.enable_graphs()
    assert torch.equal(prog.forward(x.to(DEV), torch.full((B,), 499.0)), got)
    # all-zero timestep_cond: the plain config's output, bit for bit
    prog_p = net_p.build(B, L)
    prog_p.set_conditioning(ctx.to(DEV), te.to(DEV), ids.to(DEV))
    plain_out = prog_p.forward(x.to(DEV), torch.full((B,), 499.0)).clone()
    prog.set_conditioning(ctx.to(DEV), te.to(DEV), ids.to(DEV), timestep_cond=torch.zeros(B, TCOND, dtype=F16, device=DEV))
    assert torch.equal(prog.forward(x.to(DEV), torch.full((B,), 499.0)), plain_out)
    # the plain config records op for op what the parent commit recorded; the guided one exactly one GEMM more
    with open(os.path.join(GOLD, "lcm_unet_tiny_plain_ops.json")) as fh:
        gold = json.load(fh)[f"B{B}_L8"]
    assert prog_p.prog_step.op_names() == gold["step"] and prog_p.prog_cond.op_names() == gold["cond"]
    names = prog.prog_step.op_names()
    assert names == gold["step"][:1] + ["lb_gemm_f16"] + gold["step"][1:] and prog.prog_cond.op_names() == gold["cond"]
    # required / refused
    with pytest.raises(ValueError, match="timestep_cond is required"):
        prog.set_conditioning(ctx.to(DEV), te.to(DEV), ids.to(DEV))
    with pytest.raises(ValueError, match="no time_cond_proj_dim"):
        prog_p.set_conditioning(ctx.to(DEV), te.to(DEV), ids.to(DEV), timestep_cond=emb)


def test_unet_facade_requires_timestep_cond_on_a_guidance_embedded_config():
    n = native()
    p = n.NativeSDXLPipe(turbo=True, unet_cfg=n.UNetConfig(**dataclasses.asdict(guided_cfg())),
                         vae_cfg=n.VAEConfig(**dataclasses.asdict(R.tiny_vae_cfg())), seed=0)
    cfg = R.tiny_unet_cfg()
    x = torch.zeros(1, 4, 8, 8, dtype=F16, device=DEV)
    kw = dict(encoder_hidden_states=torch.zeros(1, 77, cfg.cross_dim, dtype=F16, device=DEV),
              added_cond_kwargs={"text_embeds": torch.zeros(1, cfg.pooled_dim, dtype=F16, device=DEV),
                                 "time_ids": torch.tensor([[128.0, 128.0, 0.0, 0.0, 128.0, 128.0]], device=DEV)})
    with pytest.raises(ValueError, match="timestep_cond is required"):
        p.unet(x, 499.0, **kw)
    assert not p.do_classifier_free_guidance and not p.uses_cfg(5.0)
    emb = p.get_guidance_scale_embedding(torch.tensor([2.0]), embedding_dim=TCOND)
    a = p.unet(x, 499.0, timestep_cond=emb, **kw)[0]
    b = p.unet(x, 499.0, timestep_cond=p.get_guidance_scale_embedding(torch.tensor([6.0]), embedding_dim=TCOND), **kw)[0]
    assert torch.isfinite(a).all() and not torch.equal(a, b)
    for name in ("LCM", " lcm "):
        q = n.NativeSDXLPipe(turbo=True, unet_native=p.unet_native, vae_native=p.vae_native, scheduler=name)
        assert q.scheduler.kind == "lcm"
    with pytest.raises(ValueError, match="'euler', 'ddim' or 'lcm'"):
        n.NativeSDXLPipe(turbo=True, unet_native=p.unet_native, vae_native=p.vae_native, scheduler="lcms")


# ================================================================== whole transition
class _GuidedOracleUNet:
    """The oracle pipe's UNet with ``timestep_cond`` honoured through the bias identity (the oracle itself is unchanged)."""

    def __init__(self, inner, wc):
        self.inner, self.wc, self.config, self.calls = inner, wc, inner.config, 0

    def __call__(self, sample, timestep, encoder_hidden_states=None, timestep_cond=None, cross_attention_kwargs=None,
                 added_cond_kwargs=None, return_dict=False):
        self.calls += 1
        assert timestep_cond is not None and timestep_cond.shape[0] == 1 and sample.shape[0] == 1
        w = self.inner.w
        w2 = dict(w)
        w2["time_embedding.linear_1.bias"] = w["time_embedding.linear_1.bias"].float() + \
            w["time_embedding.linear_1.weight"].float() @ (self.wc @ timestep_cond[0].float())
        out = R.unet_forward(self.inner.cfg, w2, sample, timestep, encoder_hidden_states, added_cond_kwargs["text_embeds"],
                             added_cond_kwargs["time_ids"])
        return (out.to(sample.dtype),)


def _embedding_f64_as_pipe_method(w, embedding_dim=512, dtype=torch.float32):
    return torch.from_numpy(LR.guidance_embedding_f64(torch.as_tensor(w).reshape(-1).tolist(), embedding_dim)).to(dtype)


def _lcm_transition(frontier, turbo, guided, steps, results_log, key, guidance=None, turbo_depth=None):
    from latentblending_amd import BlendingEngine
    from latentblending_amd.backend import set_backend
    n = native()
    ucfg, vcfg = (guided_cfg() if guided else R.tiny_unet_cfg()), R.tiny_vae_cfg()
    o = OP.StableDiffusionXLPipeline(turbo=turbo, unet_cfg=ucfg, vae_cfg=vcfg, seed=0)
    o.scheduler = LR.LCMRefScheduler(noise_source=o.noise)
    if guided:
        o.unet = _GuidedOracleUNet(o.unet, cond_proj_weight(0))
        o.get_guidance_scale_embedding = _embedding_f64_as_pipe_method
    p = n.NativeSDXLPipe(turbo=turbo, unet_cfg=n.UNetConfig(**dataclasses.asdict(ucfg)), vae_cfg=n.VAEConfig(**dataclasses.asdict(vcfg)),
                         seed=0, scheduler="lcm")
    assert p.scheduler.kind == "lcm" and p.scheduler.init_noise_sigma == 1.0
    tape = OP.NoiseTape(12345)              # (the oracle pipe's own tape has the same seed: one recorded stream, read by both sides)
    p.scheduler.noise_source = tape
    np.random.seed(0)
    set_backend(R.TorchCpuBackend())
    be_o = BlendingEngine(o, metric=R.OracleLPIPS(7), verbose=False, frontier_width=frontier)
    set_backend(None)
    be_p = BlendingEngine(p, verbose=False, do_compile=True, frontier_width=frontier)
    for be in (be_o, be_p):
        be.set_dimensions((128, 128))
        be.set_num_inference_steps(steps)
        if turbo:
            if guidance is not None:
                be.set_guidance_scale(guidance)
            be.set_branching(depth_strength=turbo_depth, nmb_max_branches=5)
        else:
            be.set_guidance_scale(3.0)
            be.set_branching(depth_strength=0.5, nmb_max_branches=5)
        be.set_prompt1("photo of a reef")
        be.set_prompt2("rendering of an alien planet")
    set_backend(R.TorchCpuBackend())
    threads = torch.get_num_threads()
    torch.set_num_threads(min(os.cpu_count() or 1, 8))          # (tiny-width CPU oracle)
    try:
        o.noise.reset()
        imgs_o = be_o.run_transition(fixed_seeds=[420, 421])
    finally:
        torch.set_num_threads(threads)
        set_backend(None)
    tape.reset()
    imgs_p = be_p.run_transition(fixed_seeds=[420, 421])
    assert tape.draws == o.noise.draws and tape.draws > 0
    assert len(imgs_o) == len(imgs_p) and be_o.tree_fracts == be_p.tree_fracts and be_o.tree_idx_injection == be_p.tree_idx_injection
    lat_err = max(rel_l2(a[-1], b[-1]) for a, b in zip(be_p.tree_latents, be_o.tree_latents))
    d = np.stack([np.abs(np.asarray(a).astype(np.int32) - np.asarray(b).astype(np.int32)) for a, b in zip(imgs_p, imgs_o)])
    results_log[key] = {"frames": len(imgs_p), "final_latent_rel_l2": lat_err, "mean_abs_u8": float(d.mean()),
                        "frac_within_4": float((d <= 4).mean()), "same_tree": True, "noise_draws": tape.draws}
    print(f"[parity] LCM transition {key}: frames={len(imgs_p)} levels={sorted(set(be_p.tree_idx_injection))} latent rel_l2={lat_err:.3e} "
          f"mean|du8|={d.mean():.3f} within4={(d <= 4).mean():.4f} draws={tape.draws}")
    assert d.mean() <= 2 and (d <= 4).mean() >= 0.99
    return be_p, imgs_p, tape


@pytest.mark.parametrize("frontier", [1, 8])
def test_transition_with_lcm_scheduler_matches_oracle(frontier, results_log):
    """The whole branched transition under the latent-consistency sampler on a guidance-embedded UNet: NativeSDXLPipe(scheduler=
    "lcm") through the native batched loops against the engine on the CPU oracle pipe carrying LCMRefScheduler under the generic
    step-by-step loop, both at the same frontier and on one noise tape.  Base model, 4 steps, guidance 3.0 (embedded, so no CFG;
    mid-dampened per branch), two injection levels."""
    be, _, _ = _lcm_transition(frontier, turbo=False, guided=True, steps=4, results_log=results_log, key=f"transition_lcm_frontier{frontier}")
    assert len(set(be.tree_idx_injection)) >= 2


def test_turbo_transition_with_lcm_scheduler_matches_oracle(results_log):
    """``turbo=True``: no cond_proj, CFG off, 2 steps (the Turbo default injects at step 2, which a 2-step schedule does not have:
    depth_strength 0.5 injects at step 1, where a mid branch runs the schedule's last step only and draws nothing)."""
    _lcm_transition(8, turbo=True, guided=False, steps=2, results_log=results_log, key="transition_lcm_turbo_2steps", turbo_depth=0.5)


def test_lcm_through_the_fused_wavefront_and_dead_step_elision(results_log):
    """A single-level tree at frontier 8 goes through ``native_run_wavefront``: anchors and mids share the big batches, with the
    anchors' noise (three draws each) and the mids' (one each, at the injection step) concatenated per step, the last step without
    any, and one guidance embedding per sample (the mids run under mid-dampened guidance).  Turbo branching defaults (injection at
    step 2 of 4), guidance-embedded UNet at guidance 3.0.  Then the same transition with ``elide_dead_steps``: the overwrite
    argument holds under this sampler, so the frames are the same bits from fewer UNet samples."""
    from latentblending_amd import BlendingEngine
    be, imgs, tape = _lcm_transition(8, turbo=True, guided=True, steps=4, results_log=results_log, key="transition_lcm_wavefront",
                                     guidance=3.0)
    assert sorted(set(be.tree_idx_injection)) == [0, 2]
    pipe = be.dh.pipe
    draws = tape.draws

    def fresh_run(elide):       # (a fresh engine each time: a transition leaves its last branch's dampened guidance behind)
        np.random.seed(0)
        b = BlendingEngine(pipe, verbose=False, do_compile=True, frontier_width=8)
        b.elide_dead_steps = elide
        b.set_dimensions((128, 128))
        b.set_num_inference_steps(4)
        b.set_guidance_scale(3.0)
        b.set_branching(nmb_max_branches=5)
        b.set_prompt1("photo of a reef")
        b.set_prompt2("rendering of an alien planet")
        tape.reset()
        pipe.stats["unet_samples"] = 0
        frames = b.run_transition(fixed_seeds=[420, 421])
        assert tape.draws == draws and b.tree_fracts == be.tree_fracts
        return [np.asarray(f) for f in frames], pipe.stats["unet_samples"]
    plain, samples = fresh_run(False)
    elided, samples_elided = fresh_run(True)
    assert all(np.array_equal(np.asarray(x), y) for x, y in zip(imgs, plain))            # the parity run, reproduced
    print(f"[lcm] elide_dead_steps: unet samples {samples} -> {samples_elided}")
    assert samples_elided < samples, "no step was dead: the case proves nothing"
    assert len(plain) == len(elided) and all(np.array_equal(x, y) for x, y in zip(plain, elided))
