"""ControlNet without a GPU: the reference (tests/_controlnet_ref.py) is pinned to the untouched oracle and shown to bite, the key
list of the published format is checked, and the engine / replay logic runs on the oracle's tiny CPU pipe through the generic
loop, with a test-side ``controlnet`` and a kwargs-accepting ``unet`` attached here."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _controlnet_ref as CR  # noqa: E402
import _model_units as MU  # noqa: E402
from oracle import pipe as OP  # noqa: E402
from oracle import sdxl_ref as R  # noqa: E402

F32, F64 = torch.float32, torch.float64
DEPTHS = ((0, 1, 2), (0, 0, 1))          # the ControlNet with the UNet's depths, and the shallow one


def inputs(B=2, L=16, seed=5):
    cfg = R.tiny_unet_cfg()
    g = torch.Generator().manual_seed(seed)
    return dict(sample=torch.randn(B, 4, L, L, generator=g).half().float(), t=torch.tensor(499.0),
                ctx=torch.randn(B, 77, cfg.cross_dim, generator=g).half().float(),
                text_embeds=torch.randn(B, cfg.pooled_dim, generator=g).half().float(),
                time_ids=torch.tensor([[128.0, 128.0, 0.0, 0.0, 128.0, 128.0]] * B),
                hint=torch.rand(1, 3, 8 * L, 8 * L, generator=g))


@pytest.fixture(scope="module")
def world():
    """Weights and one float64 / float32 pair of controlled forwards per ControlNet depth, computed once."""
    ucfg = R.tiny_unet_cfg()
    uw = R.make_weights(R.unet_spec(ucfg), 0)
    x = inputs()
    out = {}
    for depth in DEPTHS:
        ccfg = CR.control_cfg(ucfg, depth)
        cw = CR.control_weights(ccfg)
        taps = {}
        eps64 = CR.controlled_eps(ucfg, CR.cast(uw, F64), ccfg, CR.cast(cw, F64), **x, dtype=F64, taps=taps)
        eps32 = CR.controlled_eps(ucfg, uw, ccfg, cw, **x, dtype=F32)
        out[depth] = SimpleNamespace(ccfg=ccfg, cw=cw, eps64=eps64, eps32=eps32, taps=taps)
    return SimpleNamespace(ucfg=ucfg, uw=uw, x=x, by_depth=out)


# ====================================================================== the restatement is pinned to the untouched oracle
def test_zero_residuals_give_the_oracles_unet_bit_for_bit(world):
    ucfg, uw, x = world.ucfg, world.uw, {k: v for k, v in world.x.items() if k != "hint"}
    taps_o, taps_c = {}, {}
    want = R.unet_forward(ucfg, uw, x["sample"], x["t"], x["ctx"], x["text_embeds"], x["time_ids"], taps=taps_o)
    skips = R.unet_skip_channels(ucfg)
    sizes, s = [], 16
    for bi in range(len(ucfg.block_channels)):
        sizes += [s] * ucfg.layers_per_block
        if bi < len(ucfg.block_channels) - 1:
            s //= 2
            sizes.append(s)
    sizes = [16] + sizes
    zeros = [torch.zeros(2, c, n, n) for c, n in zip(skips, sizes)]
    got = CR.unet_forward_controlled(ucfg, uw, **x, down_res=zeros, mid_res=torch.zeros(2, skips[-1], sizes[-1], sizes[-1]), taps=taps_c)
    assert torch.equal(got, want)
    for k, v in taps_o.items():
        assert torch.equal(taps_c[k], v), k


# ====================================================================== the published key list
def test_sdxl_key_list_count_and_shapes():
    import latentblending_amd.native.controlnet as C
    cfg = C.ControlNetConfig()
    keys = C.expected_keys(cfg)
    # the same enumeration, made by the oracle's spec helpers
    ocfg = R.UNetCfg()
    spec = {name: tuple(shape) for name, shape, _, _ in CR.controlnet_spec(ocfg).items}
    assert keys == spec and list(keys) != [] and len(keys) == len(spec)
    zero = [k for k in keys if k.startswith("controlnet_down_blocks.") and k.endswith(".weight")]
    assert [keys[k] for k in zero] == [(c, c, 1, 1) for c in [320] * 4 + [640] * 3 + [1280] * 2], "nine zero convs in skip order"
    assert keys["controlnet_mid_block.weight"] == (1280, 1280, 1, 1) and keys["controlnet_mid_block.bias"] == (1280,)
    hint = [(k, v) for k, v in keys.items() if k.startswith("controlnet_cond_embedding.") and k.endswith(".weight")]
    assert hint == [("controlnet_cond_embedding.conv_in.weight", (16, 3, 3, 3)), ("controlnet_cond_embedding.blocks.0.weight", (16, 16, 3, 3)),
                    ("controlnet_cond_embedding.blocks.1.weight", (32, 16, 3, 3)), ("controlnet_cond_embedding.blocks.2.weight", (32, 32, 3, 3)),
                    ("controlnet_cond_embedding.blocks.3.weight", (96, 32, 3, 3)), ("controlnet_cond_embedding.blocks.4.weight", (96, 96, 3, 3)),
                    ("controlnet_cond_embedding.blocks.5.weight", (256, 96, 3, 3)), ("controlnet_cond_embedding.conv_out.weight", (320, 256, 3, 3))]
    assert not any(k.startswith(("up_blocks.", "conv_out", "conv_norm_out")) for k in keys)
    # the encoder's keys are the UNet's encoder keys, shape for shape
    unet = {name: tuple(shape) for name, shape, _, _ in R.unet_spec(ocfg).items}
    enc = {k: v for k, v in keys.items() if not k.startswith(("controlnet_",))}
    assert enc == {k: v for k, v in unet.items() if k in enc} and len(enc) == sum(1 for k in unet if not k.startswith(("up_blocks.", "conv_out", "conv_norm_out")))
    assert sum(int(np.prod(v)) for v in keys.values()) == 1_251_014_160        # 1.25 G parameters: the size the SDXL ControlNets are published at


def test_tiny_key_list_follows_skip_channels():
    import latentblending_amd.native.controlnet as C
    ucfg = R.tiny_unet_cfg()
    for depth in DEPTHS:
        cfg = C.ControlNetConfig.for_unet(ucfg, transformer_depth=depth)
        keys = C.expected_keys(cfg)
        assert keys == {name: tuple(shape) for name, shape, _, _ in CR.controlnet_spec(CR.control_cfg(ucfg, depth)).items}
        skips = R.unet_skip_channels(ucfg)
        assert C.skip_channels(cfg) == skips == [64, 64, 64, 64, 128, 128, 128, 256, 256]
        assert [keys[f"controlnet_down_blocks.{k}.weight"] for k in range(len(skips))] == [(c, c, 1, 1) for c in skips]
        assert f"controlnet_down_blocks.{len(skips)}.weight" not in keys and keys["controlnet_cond_embedding.conv_out.weight"] == (64, 256, 3, 3)


def test_unknown_keys_and_misfit_shapes_are_refused():
    import latentblending_amd.native.controlnet as C
    ucfg = R.tiny_unet_cfg()
    cfg = C.ControlNetConfig.for_unet(ucfg, transformer_depth=(0, 0, 1))
    state = CR.control_weights(CR.control_cfg(ucfg, (0, 0, 1)))
    C.check_state(cfg, state)
    with pytest.raises(KeyError, match="does not have"):
        C.check_state(cfg, {**state, "up_blocks.0.resnets.0.conv1.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="does not have"):       # the deeper ControlNet's state in the shallow config
        C.check_state(cfg, CR.control_weights(CR.control_cfg(ucfg, (0, 1, 2))))
    with pytest.raises(KeyError, match="missing"):
        C.check_state(cfg, {k: v for k, v in state.items() if k != "controlnet_mid_block.bias"})
    with pytest.raises(ValueError, match="controlnet_down_blocks.4.weight"):
        C.check_state(cfg, {**state, "controlnet_down_blocks.4.weight": torch.zeros(64, 64, 1, 1)})
    with pytest.raises(ValueError, match="conv_in.weight"):
        C.check_state(cfg, {**state, "controlnet_cond_embedding.conv_in.weight": torch.zeros(16, 4, 3, 3)})


def test_config_from_the_published_json():
    import latentblending_amd.native.controlnet as C
    published = {"block_out_channels": [320, 640, 1280], "layers_per_block": 2, "transformer_layers_per_block": [1, 2, 10],
                 "down_block_types": ["DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"], "attention_head_dim": [5, 10, 20],
                 "cross_attention_dim": 2048, "projection_class_embeddings_input_dim": 2816, "addition_time_embed_dim": 256,
                 "addition_embed_type": "text_time", "conditioning_embedding_out_channels": [16, 32, 96, 256], "use_linear_projection": True,
                 "in_channels": 4, "norm_num_groups": 32, "conditioning_channels": 3, "global_pool_conditions": False}
    assert C.ControlNetConfig.from_diffusers(published) == C.ControlNetConfig()
    small = C.ControlNetConfig.from_diffusers({**published, "transformer_layers_per_block": [0, 0, 1]})
    assert small.transformer_depth == (0, 0, 1)
    with pytest.raises(ValueError, match="global_pool_conditions"):
        C.ControlNetConfig.from_diffusers({**published, "global_pool_conditions": True})


# ====================================================================== the reference bites
def rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("depth", DEPTHS)
def test_residuals_are_a_real_fraction_of_the_skips(world, depth):
    s = world.by_depth[depth]
    plain = {}
    x = {k: v for k, v in world.x.items() if k != "hint"}
    zeros = [torch.zeros_like(r) for r in s.taps["down_res"]]
    CR.unet_forward_controlled(world.ucfg, CR.cast(world.uw, F64), **x, down_res=zeros, mid_res=torch.zeros_like(s.taps["mid_res"]),
                               taps=plain, dtype=F64)
    for k, (res, skip) in enumerate(zip(s.taps["down_res"], plain["skips"])):
        ratio = rms(res) / rms(skip)
        print(f"[controlnet] depth {depth} skip {k}: rms(residual) / rms(skip) = {ratio:.3f}")
        assert ratio >= 0.1, (k, ratio)
    ratio = rms(s.taps["mid_res"]) / rms(plain["mid"])
    print(f"[controlnet] depth {depth} mid: rms(residual) / rms(mid) = {ratio:.3f}")
    assert ratio >= 0.1, ratio


MUTANTS = [("drop_zero", 0), ("drop_zero", 4), ("drop_zero", 8), "drop_mid", "drop_hint", "hidden"]


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: m if isinstance(m, str) else f"{m[0]}{m[1]}")
def test_mutants_move_eps_by_more_than_the_gpu_bound(world, depth, mutant):
    """The GPU test holds eps to ``MU.FACTOR`` times the error of a lower-precision evaluation against float64; here that yardstick
    is fp32 against float64 of the unmutated reference.  Every wrong variant must miss it, in rel-L2 and in max-abs."""
    s = world.by_depth[depth]
    m_l2, m_max = MU.errors(s.eps32, s.eps64)
    got = CR.controlled_eps(world.ucfg, CR.cast(world.uw, F64), s.ccfg, CR.cast(s.cw, F64), **world.x, dtype=F64, mutant=mutant)
    e_l2, e_max = MU.errors(got, s.eps64)
    print(f"[controlnet] depth {depth} mutant {mutant}: rel-L2 {e_l2:.3e} max {e_max:.3e} | bound {MU.FACTOR * m_l2:.3e} / {MU.FACTOR * m_max:.3e}")
    assert e_l2 > MU.FACTOR * m_l2 and e_max > MU.FACTOR * m_max


def test_wrapped_hint_embedding_is_equivariant_under_rolls(world):
    s = world.by_depth[DEPTHS[1]]
    w64 = CR.cast(s.cw, F64)
    hint = world.x["hint"].double()
    e = CR.hint_embedding(s.ccfg, w64, hint, wrap=3)
    e_rolled = CR.hint_embedding(s.ccfg, w64, torch.roll(hint, (16, 24), (2, 3)), wrap=3)
    assert torch.allclose(e_rolled, torch.roll(e, (2, 3), (2, 3)), atol=1e-12)
    assert not torch.allclose(CR.hint_embedding(s.ccfg, w64, hint), e, atol=1e-6)


# ====================================================================== engine logic on the oracle's tiny CPU pipe
class KwargsUNet:
    """The oracle pipe's UNet taking diffusers' two residual keywords (``CR.unet_forward_controlled``)."""

    def __init__(self, inner):
        self.inner, self.config, self.controlled = inner, inner.config, 0

    @property
    def calls(self):
        return self.inner.calls

    def __call__(self, sample, timestep, encoder_hidden_states=None, timestep_cond=None, cross_attention_kwargs=None,
                 added_cond_kwargs=None, return_dict=False, down_block_additional_residuals=None, mid_block_additional_residual=None):
        if down_block_additional_residuals is None:
            return self.inner(sample, timestep, encoder_hidden_states, timestep_cond, cross_attention_kwargs, added_cond_kwargs, return_dict)
        self.inner.calls += 1
        self.controlled += 1
        out = CR.unet_forward_controlled(self.inner.cfg, self.inner.w, sample, timestep, encoder_hidden_states, added_cond_kwargs["text_embeds"],
                                         added_cond_kwargs["time_ids"], down_block_additional_residuals, mid_block_additional_residual)
        return (out.to(sample.dtype),)


class RefControlNet:
    def __init__(self, ucfg, depth=(0, 0, 1)):
        self.cfg = CR.control_cfg(ucfg, depth)
        self.w = CR.control_weights(self.cfg)
        self.seen = []

    def __call__(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale=1.0,
                 added_cond_kwargs=None, return_dict=False):
        assert controlnet_cond.shape[0] == sample.shape[0] and controlnet_cond.shape[1] == 3
        assert float(controlnet_cond.min()) >= 0.0 and float(controlnet_cond.max()) <= 1.0, "the hint is in [0, 1], not normalised to +-1"
        self.seen.append((tuple(controlnet_cond.shape), float(conditioning_scale), controlnet_cond[0].clone()))
        down, mid = CR.controlnet_forward(self.cfg, self.w, sample, timestep, encoder_hidden_states, added_cond_kwargs["text_embeds"],
                                          added_cond_kwargs["time_ids"], controlnet_cond, conditioning_scale)
        return down, mid


def tiny_pipe():
    p = OP.StableDiffusionXLPipeline(turbo=True, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg())
    p.unet = KwargsUNet(p.unet)
    p.controlnet = RefControlNet(p.unet_cfg)
    return p


def engine(p):
    from latentblending_amd import BlendingEngine
    np.random.seed(0)
    be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False)
    be.set_dimensions((128, 128))
    be.set_num_inference_steps(4)
    be.set_branching(depth_strength=0.5, nmb_max_branches=3)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    return be


def hint_picture(size=(128, 128), seed=3):
    g = torch.Generator().manual_seed(seed)
    return Image.fromarray((torch.rand(size[1], size[0], 3, generator=g) * 255).to(torch.uint8).numpy())


@pytest.fixture(scope="module", autouse=True)
def cpu_backend():
    from latentblending_amd.backend import set_backend
    set_backend(R.TorchCpuBackend())
    yield
    set_backend(None)


@pytest.fixture(scope="module")
def shared(cpu_backend):
    p = tiny_pipe()
    return p, engine(p)


def run(p, be, seeds=(11, 12), **kw):
    p.noise.reset()
    return [np.asarray(f).copy() for f in be.run_transition(fixed_seeds=list(seeds), **kw)]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_control_image_changes_the_transition_and_clearing_restores_it(shared):
    p, be = shared
    plain = run(p, be)
    assert p.unet.controlled == 0 and not p.controlnet.seen
    hint = hint_picture()
    be.set_control_image(hint, 0.8)
    controlled = run(p, be)
    assert not same(controlled, plain) and p.unet.controlled > 0
    assert all(shape == (1, 3, 128, 128) and scale == 0.8 for shape, scale, _ in p.controlnet.seen)
    want = torch.from_numpy(np.asarray(hint).copy()).permute(2, 0, 1).float() / 255.0
    assert torch.equal(p.controlnet.seen[0][2], want.to(p.controlnet.seen[0][2].dtype)), "fp16(u8 / 255): the pipe's dtype"
    assert same(run(p, be), controlled), "the hint is held: the same transition again"
    be.clear_control_image()
    n = p.unet.controlled
    assert same(run(p, be), plain), "clear_control_image restores the uncontrolled frames bit for bit"
    assert p.unet.controlled == n


def test_a_hint_of_another_size_is_resized_with_lanczos(shared):
    p, be = shared
    big = hint_picture((200, 152))
    be.set_control_image(big)
    try:
        p.controlnet.seen.clear()
        run(p, be)
        want = torch.from_numpy(np.asarray(big.resize((128, 128), Image.LANCZOS)).copy()).permute(2, 0, 1).float() / 255.0
        assert torch.equal(p.controlnet.seen[0][2], want.to(p.controlnet.seen[0][2].dtype)), "fp16(u8 / 255): the pipe's dtype"
    finally:
        be.clear_control_image()
    with pytest.raises(ValueError, match="control image"):
        be.set_control_image(np.zeros((8, 8), dtype=np.uint8))


def test_state_dict_round_trip_keeps_the_hint_and_the_scale(shared):
    p, be = shared
    keys = set(be.get_state_dict())
    hint = hint_picture(seed=4)
    be.set_control_image(hint, 0.6)
    try:
        state = be.get_state_dict()
        assert set(state) == keys | {"control_image", "control_scale"} and state["control_scale"] == 0.6
        json.dumps(state["control_image"])                 # plain data: survives a yml / json file
        want = run(p, be)
        be2 = engine(p)
        be2.load_state_dict(json.loads(json.dumps(state)))
        assert be2.control_scale == 0.6 and np.array_equal(np.asarray(be2.control_image), np.asarray(hint))
        assert same(run(p, be2), want)
        be2.load_state_dict({k: v for k, v in state.items() if not k.startswith("control_")})
        assert be2.control_image is None and be2.control_scale == 1.0, "a state without a hint clears the hint"
    finally:
        be.clear_control_image()
    assert set(be.get_state_dict()) == keys


def test_swap_forward_keeps_the_hint_and_sessions_do_not_share_it(shared):
    from latentblending_amd import session
    p, be = shared
    hint = hint_picture(seed=6)
    be.set_control_image(hint, 0.7)
    try:
        run(p, be)
        be.swap_forward()
        assert be.control_image is hint and be.control_scale == 0.7
    finally:
        be.clear_control_image()
    assert "control_image" in session._ENGINE_FIELDS and "control_scale" in session._ENGINE_FIELDS
    assert "control_image" in session._TRANSIENT_FIELDS
    defaults = session._snapshot(be)[:2]
    a, b = session.EngineSession(be, defaults=defaults), session.EngineSession(be, defaults=defaults)
    with a.bound() as e:
        e.set_control_image(hint, 0.5)
    with b.bound() as e:
        assert e.control_image is None
    with a.bound() as e:
        assert e.control_image is hint and e.control_scale == 0.5
    assert be.control_image is None


def test_replay_with_the_json_keys_equals_the_hand_written_calls(shared, tmp_path):
    from latentblending_amd import replay
    p, be = shared
    hint = hint_picture(seed=8)
    hint.save(tmp_path / "hint.png")
    prompts, seeds = ["a reef", "a photo", "a city"], [21, 22, 23]
    # by hand
    be.set_control_image(hint, 0.9)
    try:
        p.noise.reset()
        be.set_prompt1(prompts[0])
        be.set_negative_prompt("")
        be.set_prompt2(prompts[1])
        want = [[np.asarray(f).copy() for f in be.run_transition(fixed_seeds=seeds[0:2])]]
        be.swap_forward()
        be.set_negative_prompt("")
        be.set_prompt2(prompts[2])
        want.append([np.asarray(f).copy() for f in be.run_transition(recycle_img1=True, fixed_seeds=seeds[1:3])])
    finally:
        be.clear_control_image()
    # through the movie JSON
    header = {"settings": "sdxl", "width": 128, "height": 128, "num_inference_steps": 4, "control_image": "hint.png", "control_scale": 0.9}
    items = [{"iteration": i, "prompt": pr, "negative_prompt": "", "seed": s} for i, (pr, s) in enumerate(zip(prompts, seeds))]
    with open(tmp_path / "movie.json", "w") as fh:
        json.dump([header] + items, fh)
    p.noise.reset()
    got = replay.run_movie_json(be, str(tmp_path / "movie.json"), None)
    assert len(got) == 2 and all(same([np.asarray(f) for f in g], w) for g, w in zip(got, want))
    assert be.control_image is None, "the chain puts the engine's own (absent) hint back"
    # ... and through the keyword arguments
    p.noise.reset()
    got = replay.run_multi_transition(be, prompts, seeds, None, list_negative_prompts=[""] * 3, control_image=hint, control_scale=0.9)
    assert all(same([np.asarray(f) for f in g], w) for g, w in zip(got, want))
    # without the keys: another movie
    p.noise.reset()
    plain = replay.run_multi_transition(be, prompts, seeds, None, list_negative_prompts=[""] * 3)
    assert not same([np.asarray(f) for f in plain[0]], want[0])
    with pytest.raises(ValueError, match="control_scale"):
        replay.run_multi_transition(be, prompts, seeds, None, control_scale=0.5)


def test_a_pipe_without_a_controlnet_is_refused_when_the_run_starts():
    p = OP.StableDiffusionXLPipeline(turbo=True, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg())
    be = engine(p)
    be.set_control_image(hint_picture())
    with pytest.raises(ValueError, match="no controlnet"):
        be.run_transition(fixed_seeds=[1, 2])


# ====================================================================== the loader consumes exactly the published keys
def test_from_dir_reads_a_diffusers_folder_and_consumes_every_key(tmp_path):
    import latentblending_amd.native.controlnet as C
    from latentblending_amd.native.weights import DictProvider
    from safetensors.torch import save_file
    ucfg = R.tiny_unet_cfg()
    state = CR.control_weights(CR.control_cfg(ucfg, (0, 0, 1)))
    save_file({k: v.half().contiguous() for k, v in state.items()}, str(tmp_path / "diffusion_pytorch_model.fp16.safetensors"))
    with open(tmp_path / "config.json", "w") as fh:
        json.dump({"_class_name": "ControlNetModel", "block_out_channels": [64, 128, 256], "layers_per_block": 2,
                   "transformer_layers_per_block": [1, 1, 1], "down_block_types": ["DownBlock2D", "DownBlock2D", "CrossAttnDownBlock2D"],
                   "attention_head_dim": [1, 2, 4], "cross_attention_dim": 256, "projection_class_embeddings_input_dim": 128 + 6 * 32,
                   "addition_time_embed_dim": 32, "addition_embed_type": "text_time", "use_linear_projection": True,
                   "conditioning_embedding_out_channels": [16, 32, 96, 256]}, fh)
    net = C.NativeControlNet.from_dir(str(tmp_path), device="cpu", scale=0.5)
    assert net.cfg == C.ControlNetConfig.for_unet(ucfg, transformer_depth=(0, 0, 1)) and net.skip_channels() == R.unet_skip_channels(ucfg)

    asked = []

    class Tracking(DictProvider):
        def _get(self, name, shape):
            asked.append(name)
            return super()._get(name, shape)
    C.NativeControlNet(net.cfg, Tracking(state), device="cpu")
    assert set(asked) == set(C.expected_keys(net.cfg)) == set(state), "the packing asks for every published key and for nothing else"
    # the conditioning scale is baked into the packed zero convs, formed in float64, and rewritten in place
    w0 = state["controlnet_down_blocks.4.weight"].reshape(128, 128)
    assert torch.equal(net.w["controlnet_down_blocks.4.weight"], (0.5 * w0.double()).half())
    assert torch.equal(net.w["controlnet_mid_block.bias"], (0.5 * state["controlnet_mid_block.bias"].double()).float())
    ptr = net.w["controlnet_down_blocks.4.weight"].data_ptr()
    net.set_scale(0.3)
    assert net.w["controlnet_down_blocks.4.weight"].data_ptr() == ptr and net.scale == 0.3
    assert torch.equal(net.w["controlnet_down_blocks.4.weight"], (0.3 * w0.double()).half())
    with pytest.raises(KeyError, match="does not have"):
        C.NativeControlNet.from_state_dict({**state, "stray.weight": torch.zeros(1)}, net.cfg, device="cpu")
