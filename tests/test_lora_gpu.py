"""LoRA adapters on a real MI355X: load, rescale, stack and unload on the native pipe, with every packed tensor held to a fresh build
from pre-merged weights (tests/_lora_ref.py: an independent float64 merge), recorded programs and graphs kept across the in-place
reload, and the merged models held to the CPU oracle at the bars of the existing parity tests.

Tiny configurations throughout (``R.tiny_unet_cfg()``, two 2-layer text towers of width 128, 128^2 renders, 4 steps, 5 branches).
The adapters are synthetic: they show that the arithmetic is the merged model's, not what a trained adapter does to a picture."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import _lora_ref as LR
import _model_units as MU
import _text_lpips_units as TL
from oracle import sdxl_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
UNET_BAR = 1e-2              # tests/test_native_gpu.py::test_unet_tiny_matches_oracle: rel-L2 of a tiny UNet forward against the oracle
UCFG = R.tiny_unet_cfg()
B, L = 2, 16


def native():
    import latentblending_amd.native as n
    return n


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def clip_cfgs():
    n = native()
    base = dict(vocab_size=2000, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, bos_token_id=1998,
                eos_token_id=1999)
    return n.CLIPTextConfig(pad_token_id=1999, **base), n.CLIPTextConfig(hidden_act="gelu", projection_dim=128, pad_token_id=0, **base)


@functools.lru_cache(maxsize=None)
def base_states():
    """(UNet, tower 1, tower 2) base state dicts: fp16-representable fp32, the values ``SyntheticProvider(0)`` gives the UNet."""
    c1, c2 = clip_cfgs()
    return R.make_weights(R.unet_spec(UCFG), 0), TL.clip_weights(c1, 3), TL.clip_weights(c2, 4)


@functools.lru_cache(maxsize=None)
def adapter(kind, seed=5, rank=4, alpha=6.0):
    """(unet, te1, te2) adapters of ``make_adapter``.  "all": attention / feed-forward linears, resnet convs, shortcuts, time projections,
    down- and upsampler convs, and the projections of both towers; "unet": the same without the towers; "lcm": the resnet convs,
    time projections and sampler convs only - with the attention linears the target set of the published LCM-LoRA."""
    su, s1, s2 = (LR.unet_weight_shapes(s) for s in base_states())
    pick_u = LR.pick(su, LR.RESNET if kind == "lcm" else LR.ATTN_FF + LR.RESNET)
    a_u = LR.make_adapter(pick_u, rank, alpha, seed)
    if kind != "all":
        return a_u, {}, {}
    return a_u, LR.make_adapter(LR.pick(s1, LR.CLIP_LINEARS), rank, alpha, seed + 1), LR.make_adapter(LR.pick(s2, LR.CLIP_LINEARS), rank, None, seed + 2)


def as_file(ad, naming="kohya"):
    out = {}
    for comp, a in zip(("unet", "te1", "te2"), ad):
        out.update(LR.write(a, naming, comp, UCFG))
    return out


def merged(stack):
    """``stack`` = [(adapter triple, scale), ...] -> the three pre-merged state dicts."""
    return tuple(LR.merged_state(s, [(ad[i], scale) for ad, scale in stack]) for i, s in enumerate(base_states()))


def make_pipe(states=None, scheduler="ddim", **kw):
    n = native()
    su, s1, s2 = states or base_states()
    c1, c2 = clip_cfgs()
    p1, p2 = n.DictProvider(s1), n.DictProvider(s2)
    enc = n.NativeTextEncoders(n.NativeCLIPText(c1, p1, DEV), n.NativeCLIPText(c2, p2, DEV), allow_synthetic=True, providers=(p1, p2))
    return n.NativeSDXLPipe(turbo=True, unet_cfg=n.UNetConfig(**dataclasses.asdict(UCFG)), vae_cfg=n.VAEConfig(**dataclasses.asdict(R.tiny_vae_cfg())),
                            unet_provider=n.DictProvider(su), encoders=enc, seed=0, scheduler=scheduler, allow_synthetic=True, **kw)


def fresh_unet(states):
    n = native()
    return n.NativeUNet(n.UNetConfig(**dataclasses.asdict(UCFG)), n.DictProvider(states[0]), DEV)


@functools.lru_cache(maxsize=None)
def step_inputs():
    g = torch.Generator().manual_seed(B * 100 + L)
    x = torch.randn(B, 4, L, L, generator=g).half()
    ctx = torch.randn(B, 77, UCFG.cross_dim, generator=g).half()
    te = torch.randn(B, UCFG.pooled_dim, generator=g).half()
    ids = torch.tensor([[128.0, 128.0, 0.0, 0.0, 128.0, 128.0]] * B)
    return x, ctx, te, ids


def run_step(prog, t=499.0):
    x, ctx, te, ids = step_inputs()
    prog.set_conditioning(ctx.to(DEV), te.to(DEV), ids.to(DEV))
    out = prog.forward(x.to(DEV), torch.full((B,), t)).clone()
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def shared():
    """One pipe (graphs on) for the tests that load and unload: each starts from ``clean()``; the base packed tensors and the base
    UNet step are taken once, before any adapter."""
    pipe = make_pipe()
    pipe.enable_graphs(True)
    base_w = {k: t.clone() for k, t in pipe.unet_native.w.items()}
    base_t = [{k: t.clone() for k, t in tw.w.items()} for tw in (pipe.encoders.enc1, pipe.encoders.enc2)]
    base_out = run_step(pipe.unet_program(B, L))
    return pipe, base_w, base_t, base_out


def clean():
    pipe, base_w, base_t, base_out = shared()
    pipe.unload_lora()
    assert not pipe.loras
    return pipe, base_w, base_t, base_out


def same_tensors(got, want):
    assert list(got) == list(want)
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    assert not bad, bad[:6]


# ---------------------------------------------------------------------------------------------------------------- packed tensors
def test_packed_tensors_are_those_of_a_fresh_build_from_merged_weights():
    pipe, base_w, base_t, _ = clean()
    n = native()
    ad = adapter("all")
    ptrs = [{k: t.data_ptr() for k, t in net.w.items()} for net in (pipe.unet_native, pipe.encoders.enc1, pipe.encoders.enc2)]
    name = pipe.load_lora(as_file(ad), name="style")
    assert name == "style" and dict(pipe.loras) == {"style": 1.0}
    want = merged([(ad, 1.0)])
    same_tensors(pipe.unet_native.w, fresh_unet(want).w)
    c1, c2 = clip_cfgs()
    same_tensors(pipe.encoders.enc1.w, n.NativeCLIPText(c1, n.DictProvider(want[1]), DEV).w)
    same_tensors(pipe.encoders.enc2.w, n.NativeCLIPText(c2, n.DictProvider(want[2]), DEV).w)
    assert ptrs == [{k: t.data_ptr() for k, t in net.w.items()} for net in (pipe.unet_native, pipe.encoders.enc1, pipe.encoders.enc2)]
    # what the adapter reaches did change - every derived layout among it - and what it does not reach kept its bits
    w = pipe.unet_native.w
    changed = {k for k in w if not torch.equal(w[k], base_w[k])}
    blk = "down_blocks.1.attentions.0.transformer_blocks.0"
    for k in (f"{blk}.attn1.qkv", f"{blk}.attn1.qkv_ln.weight", f"{blk}.attn1.qkv_ln.colsum", f"{blk}.attn1.qkv_ln.bias",
              f"{blk}.attn2.to_q_ln.weight", f"{blk}.ff.net.0.proj_ln.bias", "ctx_kv.weight", "temb_proj.weight",
              "down_blocks.0.resnets.0.conv1.weight", "down_blocks.1.resnets.0.conv_shortcut.weight", "down_blocks.0.downsamplers.0.conv.weight",
              "up_blocks.0.upsamplers.0.conv.weight.sub4", "up_blocks.0.upsamplers.0.conv.weight.sub01"):
        assert k in changed, k
    untouched = [k for k in w if k.startswith(("conv_in.", "conv_out.", "time_embedding.", "add_embedding.", "conv_norm_out.", "temb_proj.bias"))
                 or (k.endswith(".bias") and "_ln." not in k) or ".norm" in k]
    assert len(untouched) > 100 and not changed & set(untouched)
    for tw, base in zip((pipe.encoders.enc1, pipe.encoders.enc2), base_t):
        moved = {k for k in tw.w if not torch.equal(tw.w[k], base[k])}
        assert moved == {f"{i}.{m}.w" for i in range(2) for m in ("qkv", "out", "fc1", "fc2")}, moved


def test_pipe_without_base_providers_says_what_to_pass():
    n = native()
    pipe, _, _, _ = clean()
    bare = n.NativeSDXLPipe(turbo=True, unet_native=pipe.unet_native, vae_native=pipe.vae_native, allow_synthetic=True)
    with pytest.raises(ValueError, match="unet_provider="):
        bare.load_lora(as_file(adapter("unet")))
    with pytest.raises(ValueError, match="encoders="):
        bare_ok = n.NativeSDXLPipe(turbo=True, unet_native=pipe.unet_native, unet_provider=n.DictProvider(base_states()[0]),
                                   vae_native=pipe.vae_native, allow_synthetic=True)
        bare_ok.load_lora(as_file(adapter("all")))
    assert not bare.loras and not bare_ok.loras
    same_tensors(pipe.unet_native.w, shared()[1])           # a refused load wrote nothing


# ---------------------------------------------------------------------------------------------------------------- programs survive
def test_programs_and_graphs_survive_a_load():
    pipe, _, _, base_out = clean()
    prog = pipe.unet_program(B, L)
    assert prog.prog_step.graph_ready and prog.prog_cond.graph_ready
    handles, ops = (prog.prog_step.handle, prog.prog_cond.handle), (prog.prog_step.num_ops, prog.prog_cond.num_ops)
    cached = dict(pipe._unet_programs)
    assert torch.equal(run_step(prog), base_out)
    ad = adapter("all")
    pipe.load_lora(as_file(ad, "sgm"))
    assert dict(pipe._unet_programs) == cached and pipe.unet_program(B, L) is prog
    assert (prog.prog_step.handle, prog.prog_cond.handle) == handles and (prog.prog_step.num_ops, prog.prog_cond.num_ops) == ops
    assert prog.prog_step.graph_ready and prog.prog_cond.graph_ready
    got = run_step(prog)
    fresh = make_pipe(merged([(ad, 1.0)]))
    fresh.enable_graphs(True)
    assert torch.equal(got, run_step(fresh.unet_program(B, L)))
    moved = rel_l2(got, base_out)
    print(f"[lora] UNet step with the adapter against the base step: rel_l2={moved:.3e}")
    assert torch.isfinite(got).all() and moved >= 10 * UNET_BAR          # a merge that does nothing must not pass


# ---------------------------------------------------------------------------------------------------------------- against the oracle
def test_merged_unet_matches_the_oracle(results_log):
    pipe, _, _, _ = clean()
    ad = adapter("all")
    pipe.load_lora(as_file(ad, "peft"))
    x, ctx, te, ids = step_inputs()
    ref = R.unet_forward(UCFG, merged([(ad, 1.0)])[0], x, torch.tensor(499.0), ctx, te, ids)
    r = rel_l2(run_step(pipe.unet_program(B, L)), ref)
    results_log["lora_unet_tiny_rel_l2"] = r
    print(f"[lora] merged tiny UNet B={B} L={L} against the oracle: rel_l2={r:.3e}")
    assert r <= UNET_BAR


def test_merged_text_tower_matches_float64(results_log):
    """One prompt through the LoRA'd second tower against the float64 forward of tests/_text_lpips_units.py on the merged weights, at
    that file's bar: FACTOR x the storage model (``MU.compare``).  The storage model rounds where the program stores; a merged
    projection is no longer fp16-representable and the tower stores it as fp16, so the model's matrices are the fp16-rounded ones
    (the base suite's weights are fp16-representable, where this rounding is the identity).  REF sees the unrounded merge."""
    pipe, _, base_t, _ = clean()
    ad = adapter("all")
    pipe.load_lora(as_file(ad))
    cfg = clip_cfgs()[1]
    w = merged([(ad, 1.0)])[2]
    ref = MU.Ev(MU.F64, w, False)
    model = MU.Ev(MU.F32, {k: (v.half().float() if v.ndim == 2 else v) for k, v in w.items()}, True)
    ids = TL.make_ids(cfg, (9,), seed=20)
    pen, pooled = pipe.encoders.enc2.forward(ids)
    torch.cuda.synchronize()
    want, mod = TL.clip_forward(ref, cfg, ids), TL.clip_forward(model, cfg, ids)
    fails = [MU.compare(results_log, "lora_clip_te2/penultimate", pen, mod["penultimate"], want["penultimate"]),
             MU.compare(results_log, "lora_clip_te2/pooled", pooled, mod["pooled"], want["pooled"])]
    assert not [f for f in fails if f], fails
    base = TL.clip_forward(MU.Ev(MU.F64, base_states()[2], False), cfg, ids)
    assert MU.errors(pen, base["penultimate"].reshape(pen.shape))[0] > 0.1       # ... and it is not the base tower's answer


# ---------------------------------------------------------------------------------------------------------------- scale, stack, unload
def test_scale_stack_and_unload():
    pipe, base_w, base_t, base_out = clean()
    prog = pipe.unet_program(B, L)
    a, b = adapter("all"), adapter("unet", seed=31, rank=3, alpha=2.0)

    def is_base():
        same_tensors(pipe.unet_native.w, base_w)
        same_tensors(pipe.encoders.enc1.w, base_t[0])
        same_tensors(pipe.encoders.enc2.w, base_t[1])
        assert torch.equal(run_step(prog), base_out)

    def is_fresh(stack):
        net = fresh_unet(merged(stack))
        same_tensors(pipe.unet_native.w, net.w)
        assert torch.equal(run_step(prog), run_step(net.build(B, L)))

    na = pipe.load_lora(as_file(a), name="a")
    assert not torch.equal(run_step(prog), base_out)
    pipe.set_lora_scale(na, 0.0)
    assert dict(pipe.loras) == {"a": 0.0}
    is_base()
    pipe.set_lora_scale(na, 0.5)
    is_fresh([(a, 0.5)])
    pipe.unload_lora()
    assert not pipe.loras
    is_base()
    pipe.load_lora(as_file(a), scale=0.75, name="a")
    nb = pipe.load_lora(as_file(b, "sgm"), scale=-0.5)
    assert list(pipe.loras.items()) == [("a", 0.75), (nb, -0.5)]
    is_fresh([(a, 0.75), (b, -0.5)])
    pipe.unload_lora("a")
    assert list(pipe.loras.items()) == [(nb, -0.5)]
    is_fresh([(b, -0.5)])
    same_tensors(pipe.encoders.enc2.w, base_t[1])
    with pytest.raises(KeyError, match="nope"):
        pipe.unload_lora("nope")
    pipe.unload_lora()
    is_base()


def test_reload_leaves_no_second_copy_behind():
    pipe, _, _, _ = clean()
    pipe._embed_cache.clear()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    pipe.load_lora(as_file(adapter("all")))
    torch.cuda.synchronize()
    weights = pipe.unet_native.weight_bytes()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"[lora] reload: peak {peak} bytes over the resident set, UNet weights {weights} bytes")
    # one scratch copy of the packed weights while it is written over the live ones (plus the upload of one tensor at a time, which
    # is never a second scratch copy) - and nothing of it afterwards
    assert torch.cuda.memory_allocated() == before and peak <= 2 * weights


# ---------------------------------------------------------------------------------------------------------------- text cache
def test_embed_cache_follows_the_text_towers():
    pipe, _, _, _ = clean()
    pe0 = pipe.encode_prompt("photo of a reef", do_classifier_free_guidance=False)[0]
    assert "photo of a reef" in pipe._embed_cache
    pipe.load_lora(as_file(adapter("unet")), name="u")
    assert "photo of a reef" in pipe._embed_cache                        # a UNet-only adapter leaves the embeddings alone
    assert torch.equal(pipe.encode_prompt("photo of a reef", do_classifier_free_guidance=False)[0], pe0)
    pipe.load_lora(as_file(adapter("all")), name="t")
    assert not pipe._embed_cache
    pe1 = pipe.encode_prompt("photo of a reef", do_classifier_free_guidance=False)[0]
    fresh = make_pipe(merged([(adapter("all"), 1.0)]))
    assert not torch.equal(pe1, pe0) and torch.equal(pe1, fresh.encode_prompt("photo of a reef", do_classifier_free_guidance=False)[0])
    pipe.unload_lora("t")
    assert torch.equal(pipe.encode_prompt("photo of a reef", do_classifier_free_guidance=False)[0], pe0)


# ---------------------------------------------------------------------------------------------------------------- through the engine
def transition(pipe):
    from latentblending_amd import BlendingEngine
    np.random.seed(0)
    be = BlendingEngine(pipe, verbose=False)
    be.set_dimensions((128, 128))
    be.set_num_inference_steps(4)
    be.set_branching(depth_strength=0.5, nmb_max_branches=5)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    s0 = pipe.stats["unet_samples"]
    frames = [np.asarray(f) for f in be.run_transition(fixed_seeds=[420, 421])]
    return frames, pipe.stats["unet_samples"] - s0, be


def test_transition_with_scale_zero_and_unloaded_equals_the_base():
    pipe, _, _, _ = clean()
    base, n_base, _ = transition(pipe)
    name = pipe.load_lora(as_file(adapter("all")))
    with_lora, n_lora, _ = transition(pipe)
    pipe.set_lora_scale(name, 0.0)
    zero, n_zero, _ = transition(pipe)
    pipe.unload_lora()
    gone, n_gone, _ = transition(pipe)
    assert len(base) == len(with_lora) == len(zero) == len(gone) >= 3
    assert any(not np.array_equal(a, b) for a, b in zip(base, with_lora))
    assert all(np.array_equal(a, b) for a, b in zip(base, zero)) and all(np.array_equal(a, b) for a, b in zip(base, gone))
    assert n_base == n_lora == n_zero == n_gone > 0


def test_lcm_sampler_with_an_adapter_over_the_resnet_convs():
    """The LCM-LoRA way: ``scheduler="lcm"`` plus an adapter over the resnets' convs and time projections.  Counter-based sampler
    noise, so that two pipes draw the same values for the same seeds."""
    ad = adapter("lcm")
    assert any(m.endswith(".time_emb_proj") for m in ad[0]) and any(m.endswith(".conv1") for m in ad[0])
    pipe = make_pipe(scheduler="lcm", noise="counter", loras=[(as_file(ad), 1.0)])
    assert list(pipe.loras.values()) == [1.0]
    frames, _, be = transition(pipe)
    fresh = make_pipe(merged([(ad, 1.0)]), scheduler="lcm", noise="counter")
    frames2, _, be2 = transition(fresh)
    finals, finals2 = [t[-1] for t in be.tree_latents], [t[-1] for t in be2.tree_latents]
    assert len(finals) == len(finals2) >= 3 and all(torch.isfinite(t.float()).all() for t in finals)
    assert all(torch.equal(a, b) for a, b in zip(finals, finals2))
    assert all(np.array_equal(a, b) for a, b in zip(frames, frames2))
    plain, _, _ = transition(make_pipe(scheduler="lcm", noise="counter"))
    assert any(not np.array_equal(a, b) for a, b in zip(frames, plain))


# ---------------------------------------------------------------------------------------------------------------- diffusers' names
def test_diffusers_names_forward_to_the_pipe_methods():
    pipe, base_w, _, _ = clean()
    a, b = adapter("all"), adapter("unet", seed=31, rank=3, alpha=2.0)
    pipe.load_lora_weights(as_file(a), adapter_name="a")
    pipe.load_lora_weights(as_file(b), adapter_name="b")
    assert dict(pipe.loras) == {"a": 1.0, "b": 1.0}
    pipe.set_adapters(["a", "b"], adapter_weights=[0.5, 0.25])
    assert dict(pipe.loras) == {"a": 0.5, "b": 0.25}
    other = make_pipe()
    other.load_lora(as_file(a), scale=0.5)
    other.load_lora(as_file(b), scale=0.25)
    same_tensors(pipe.unet_native.w, other.unet_native.w)
    same_tensors(pipe.encoders.enc2.w, other.encoders.enc2.w)
    pipe.set_adapters("b")                                  # diffusers: the named adapters are active, the others are not
    assert dict(pipe.loras) == {"a": 0.0, "b": 1.0}
    same_tensors(pipe.unet_native.w, fresh_unet(merged([(b, 1.0)])).w)
    pipe.fuse_lora()
    pipe.unfuse_lora()
    same_tensors(pipe.unet_native.w, fresh_unet(merged([(b, 1.0)])).w)
    pipe.unload_lora_weights()
    assert not pipe.loras
    same_tensors(pipe.unet_native.w, base_w)
