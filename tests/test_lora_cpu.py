"""LoRA adapters without a device: key resolution in the three namings, the float64 merge of ``LoRAProvider``, the refusals, the
in-place reload of a model packed on the CPU, and the drivers' ``loras`` keywords (a stub pipe records the calls).

No real LoRA file exists here: the literal keys below are written from the published formats."""
import dataclasses
import json
import types

import pytest
import torch
import torch.nn.functional as F

import _lora_ref as LR
import _text_lpips_units as TL
from oracle import sdxl_ref as R

F32, F64 = torch.float32, torch.float64


def native():
    import latentblending_amd.native as n
    return n


def lora():
    import latentblending_amd.native.lora as L
    return L


def tiny_ucfg():
    return native().UNetConfig(**dataclasses.asdict(R.tiny_unet_cfg()))


def tiny_clip(proj):
    return native().CLIPTextConfig(vocab_size=1000, bos_token_id=998, eos_token_id=999, pad_token_id=999, num_hidden_layers=2,
                                   hidden_size=128, num_attention_heads=2, intermediate_size=256, hidden_act="gelu", projection_dim=proj)


# ---------------------------------------------------------------------------------------------------------------- literal keys
LITERAL = [
    ("lora_unet_input_blocks_4_1_transformer_blocks_0_attn1_to_q", "unet", "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q"),
    ("lora_unet_input_blocks_3_0_op", "unet", "down_blocks.0.downsamplers.0.conv"),
    ("lora_unet_input_blocks_1_0_emb_layers_1", "unet", "down_blocks.0.resnets.0.time_emb_proj"),
    ("lora_unet_middle_block_1_proj_out", "unet", "mid_block.attentions.0.proj_out"),
    ("lora_unet_output_blocks_2_2_conv", "unet", "up_blocks.0.upsamplers.0.conv"),
    ("lora_unet_output_blocks_5_1_transformer_blocks_1_ff_net_0_proj", "unet", "up_blocks.1.attentions.2.transformer_blocks.1.ff.net.0.proj"),
    ("lora_te2_text_model_encoder_layers_31_mlp_fc1", "te2", "text_model.encoder.layers.31.mlp.fc1"),
    ("unet.mid_block.attentions.0.transformer_blocks.0.attn2.to_k.lora_A.weight", "unet", "mid_block.attentions.0.transformer_blocks.0.attn2.to_k"),
]


@pytest.mark.parametrize("key,comp,param", LITERAL, ids=[k[:48] for k, _, _ in LITERAL])
def test_literal_keys_resolve_for_sdxl(key, comp, param):
    L, n = lora(), native()
    shapes = {"unet": L.unet_modules(n.UNetConfig()), "te2": L.clip_modules(n.CLIPTextConfig.openclip_bigg())}[comp]
    shape = shapes[param]
    down, up = torch.zeros((2, shape[1]) + tuple(shape[2:])), torch.zeros((shape[0], 2) + ((1, 1) if len(shape) == 4 else ()))
    if key.endswith(".lora_A.weight"):
        state = {key: down, key.replace("lora_A", "lora_B"): up}
    else:
        state = {key + ".lora_down.weight": down, key + ".lora_up.weight": up}
    rec = L.read_lora(state)                       # (the default configurations are SDXL's)
    assert list(rec.components[comp]) == [param + ".weight"] and rec.touched() == (comp,)
    d, u, alpha = rec.components[comp][param + ".weight"]
    assert d.shape == down.shape and u.shape == up.shape and alpha == 2.0


def test_older_peft_forms_resolve():
    L = lora()
    cfg = tiny_ucfg()
    b = "down_blocks.1.attentions.0.transformer_blocks.0"
    state = {f"unet.{b}.attn1.processor.to_q_lora.down.weight": torch.zeros(2, 128), f"unet.{b}.attn1.processor.to_q_lora.up.weight": torch.zeros(128, 2),
             f"unet.{b}.attn2.processor.to_out_lora.down.weight": torch.zeros(2, 128), f"unet.{b}.attn2.processor.to_out_lora.up.weight": torch.zeros(128, 2),
             f"unet.{b}.ff.net.2.lora.down.weight": torch.zeros(3, 512), f"unet.{b}.ff.net.2.lora.up.weight": torch.zeros(128, 3),
             f"unet.{b}.ff.net.2.alpha": torch.tensor(1.5)}
    rec = L.read_lora(state, unet_cfg=cfg)
    assert sorted(rec.components["unet"]) == [f"{b}.attn1.to_q.weight", f"{b}.attn2.to_out.0.weight", f"{b}.ff.net.2.weight"]
    assert rec.components["unet"][f"{b}.ff.net.2.weight"][2] == 1.5 and rec.components["unet"][f"{b}.attn1.to_q.weight"][2] == 2.0


# ---------------------------------------------------------------------------------------------------------------- resolution tables
class Spy:
    """A provider that records what it is asked for and hands out zero-stride zeros (no memory behind them)."""

    def __init__(self):
        self.weights, self.others = {}, set()

    def weight(self, name, shape, fan_in=0, gain=1.0):
        self.weights[name] = tuple(int(v) for v in shape)
        return torch.zeros(1).expand(*shape)

    def bias(self, name, n):
        self.others.add(name)
        return torch.zeros(n)

    norm_weight = positive = bias


@pytest.fixture
def cheap_packing(monkeypatch):
    """Nothing is kept of what the full-size models pack: the walk and its requests are what the test is about."""
    import latentblending_amd.native.weights as W
    monkeypatch.setattr(W.Packer, "dev", lambda self, t, dtype: torch.empty(0))


def check_tables(tables, shapes, asked):
    for naming, table in tables.items():
        # every module (the original SDXL UNet has no name for the guidance projection of distilled UNets), and ...
        assert set(table.values()) == set(shapes) - ({"time_embedding.cond_proj"} if naming == "sgm" else set()), naming
        assert len(set(table.values())) == len(table), naming                 # ... no two file names for one parameter
        for fname, mod in table.items():
            assert asked.get(mod + ".weight") == shapes[mod], (naming, fname, mod)


@pytest.mark.parametrize("size", ["tiny", "tiny_guided", "sdxl"])
def test_unet_tables_name_what_the_model_loads(size, cheap_packing):
    n, L = native(), lora()
    cfg = {"tiny": tiny_ucfg(), "tiny_guided": dataclasses.replace(tiny_ucfg(), time_cond_proj_dim=32), "sdxl": n.UNetConfig()}[size]
    spy = Spy()
    n.NativeUNet(cfg, spy, "cpu", fuse_layernorm=False)
    shapes = L.unet_modules(cfg)
    assert {m + ".weight": s for m, s in shapes.items()} == spy.weights           # the tables cover every weight the UNet asks for
    check_tables(L.unet_tables(cfg), shapes, spy.weights)
    assert all(m + ".weight" in spy.others for m in L._unet_norm_modules(cfg))    # the "not a weight" list names real norms


@pytest.mark.parametrize("which", ["tiny", "clip_l", "bigg"])
def test_clip_tables_name_what_the_tower_loads(which, cheap_packing):
    n, L = native(), lora()
    cfg = {"tiny": tiny_clip(64), "clip_l": n.CLIPTextConfig.clip_l(), "bigg": n.CLIPTextConfig.openclip_bigg()}[which]
    spy = Spy()
    n.NativeCLIPText(cfg, spy, "cpu", prefix="text_model.")
    shapes = L.clip_modules(cfg)
    for comp in ("te1", "te2"):
        tables = L.clip_tables(cfg, comp)
        for naming, table in tables.items():
            assert set(table.values()) == set(shapes) and len(set(table.values())) == len(table)
            assert all(spy.weights.get(mod + ".weight") == shapes[mod] for mod in table.values()), naming
    assert not set(L.clip_tables(cfg, "te1")["kohya"]) & set(L.clip_tables(cfg, "te2")["kohya"])


# ---------------------------------------------------------------------------------------------------------------- round trip
def tiny_adapters(seed=5):
    """(unet adapter, te1 adapter, te2 adapter) over the tiny models: attention / feed-forward linears, resnet convs, samplers."""
    ucfg = R.tiny_unet_cfg()
    ushapes = LR.unet_weight_shapes(R.make_weights(R.unet_spec(ucfg), 0))
    c1, c2 = tiny_clip(None), tiny_clip(64)
    a_u = LR.make_adapter(LR.pick(ushapes, LR.ATTN_FF + LR.RESNET), 4, 6.0, seed)
    a_1 = LR.make_adapter(LR.pick(LR.unet_weight_shapes(TL.clip_weights(c1, 3)), LR.CLIP_LINEARS), 4, 6.0, seed + 1)
    a_2 = LR.make_adapter(LR.pick(LR.unet_weight_shapes(TL.clip_weights(c2, 4)), LR.CLIP_LINEARS), 4, None, seed + 2)
    return a_u, a_1, a_2


def same_record(a, b):
    for comp in ("unet", "te1", "te2"):
        assert sorted(a.components[comp]) == sorted(b.components[comp])
        for k, (d, u, alpha) in a.components[comp].items():
            d2, u2, alpha2 = b.components[comp][k]
            assert torch.equal(d, d2) and torch.equal(u, u2) and alpha == alpha2 and d.dtype == F32, (comp, k)


def test_three_namings_read_back_to_one_record():
    L = lora()
    a_u, a_1, a_2 = tiny_adapters()
    assert any(len(d.shape) == 4 and d.shape[-1] == 3 for d, _, _ in a_u.values()) and any(m.endswith("conv_shortcut") for m in a_u)
    ucfg, c1, c2 = tiny_ucfg(), tiny_clip(None), tiny_clip(64)
    recs = {}
    for naming in LR.NAMINGS:
        state = {}
        for comp, ad in (("unet", a_u), ("te1", a_1), ("te2", a_2)):
            state.update(LR.write(ad, naming, comp, R.tiny_unet_cfg(), conv_shaped_linears=naming == "kohya"))
        recs[naming] = L.read_lora(state, unet_cfg=ucfg, te_cfgs=(c1, c2))
        assert recs[naming].naming[0] == naming and not recs[naming].skipped
    for naming in LR.NAMINGS:
        same_record(recs[naming], recs["peft"])
    want = {"unet": LR.targets(a_u), "te1": LR.targets(a_1), "te2": LR.targets(a_2)}
    for comp, t in want.items():                    # ... and that record is the adapter: squeezed linears, alpha or the rank
        assert set(t) == set(recs["sgm"].components[comp])
        for k, (d, u, alpha) in t.items():
            d2, u2, alpha2 = recs["sgm"].components[comp][k]
            assert torch.equal(d, d2) and torch.equal(u, u2) and alpha == alpha2
    assert {v[2] for v in recs["sgm"].components["te2"].values()} == {4.0}       # no alpha in the file: the rank


def test_a_safetensors_file_and_its_directory_read_like_the_dict(tmp_path):
    from safetensors.torch import save_file
    L = lora()
    a_u, _, _ = tiny_adapters()
    state = LR.write(a_u, "kohya", "unet")
    fp = tmp_path / "style.safetensors"
    save_file({k: v.contiguous() for k, v in state.items()}, str(fp))
    same_record(L.read_lora(str(fp), unet_cfg=tiny_ucfg()), L.read_lora(state, unet_cfg=tiny_ucfg()))
    same_record(L.read_lora(str(tmp_path), unet_cfg=tiny_ucfg()), L.read_lora(state, unet_cfg=tiny_ucfg()))


# ---------------------------------------------------------------------------------------------------------------- merge arithmetic
def base_tensors():
    g = torch.Generator().manual_seed(1)
    return {"lin.weight": torch.randn(48, 40, generator=g) * 40 ** -0.5, "conv.weight": torch.randn(24, 16, 3, 3, generator=g) / 12,
            "short.weight": torch.randn(24, 16, 1, 1, generator=g) / 4, "lin.bias": torch.randn(48, generator=g)}


def test_provider_weight_is_the_float64_merge_rounded_once():
    n = native()
    base = base_tensors()
    shapes = {"lin": (48, 40), "conv": (24, 16, 3, 3), "short": (24, 16, 1, 1)}
    a = LR.make_adapter(shapes, 4, 6.0, 11)             # alpha given
    b = LR.make_adapter(shapes, 3, None, 12)            # alpha absent: the rank
    for stack in ([(a, 1.0)], [(b, 0.7)], [(a, 0.8), (b, -0.35)]):
        pv = n.LoRAProvider(n.DictProvider(base), [(LR.targets(ad), s) for ad, s in stack])
        want = LR.merged_state(base, stack)
        for mod, shape in shapes.items():
            got = pv.weight(mod + ".weight", shape)
            assert got.dtype == F32 and torch.equal(got, want[mod + ".weight"]), (mod, len(stack))
            assert not torch.equal(got, base[mod + ".weight"])
        assert torch.equal(pv.bias("lin.bias", 48), base["lin.bias"])


def test_scale_zero_and_untargeted_names_return_the_base_bits():
    n = native()
    base = base_tensors()
    a = LR.make_adapter({"lin": (48, 40)}, 4, 6.0, 11)
    b = LR.make_adapter({"lin": (48, 40)}, 4, 6.0, 13)
    off = n.LoRAProvider(n.DictProvider(base), [(LR.targets(a), 0.0)])
    assert torch.equal(off.weight("lin.weight", (48, 40)), base["lin.weight"])
    on = n.LoRAProvider(n.DictProvider(base), [(LR.targets(a), 1.0)])
    assert torch.equal(on.weight("conv.weight", (24, 16, 3, 3)), base["conv.weight"])
    mixed = n.LoRAProvider(n.DictProvider(base), [(LR.targets(a), 0.0), (LR.targets(b), 1.0)])
    assert torch.equal(mixed.weight("lin.weight", (48, 40)), LR.merged_state(base, [(b, 1.0)])["lin.weight"])
    # a -0.0 base element must not come back as +0.0, as "W + 0 * delta" would give
    z = dict(base, **{"lin.weight": base["lin.weight"].clone()})
    z["lin.weight"][0, 0] = -0.0
    got = n.LoRAProvider(n.DictProvider(z), [(LR.targets(a), 0.0)]).weight("lin.weight", (48, 40))
    assert torch.equal(got.view(torch.int32), z["lin.weight"].view(torch.int32))


def test_merged_layer_equals_base_layer_plus_low_rank_path():
    base = {k: v.to(F64) for k, v in base_tensors().items()}
    g = torch.Generator().manual_seed(2)
    s, alpha = 0.6, 6.0
    a = LR.make_adapter({"lin": (48, 40), "conv": (24, 16, 3, 3)}, 4, alpha, 21)
    x = torch.randn(5, 40, generator=g, dtype=F64)
    d, u, _ = a["lin"]
    W2 = base["lin.weight"] + (s * (alpha / 4)) * (u.to(F64) @ d.to(F64))
    want = x @ base["lin.weight"].T + s * (alpha / 4) * (x @ d.to(F64).T) @ u.to(F64).T
    assert float((x @ W2.T - want).norm() / want.norm()) <= 1e-12
    img = torch.randn(2, 16, 9, 7, generator=g, dtype=F64)
    d, u, _ = a["conv"]
    W2 = base["conv.weight"] + (s * (alpha / 4)) * (u.to(F64).reshape(24, 4) @ d.to(F64).reshape(4, -1)).reshape(24, 16, 3, 3)
    want = F.conv2d(img, base["conv.weight"], padding=1) + s * (alpha / 4) * F.conv2d(F.conv2d(img, d.to(F64), padding=1), u.to(F64))
    assert float((F.conv2d(img, W2, padding=1) - want).norm() / want.norm()) <= 1e-12
    # ... and W2 is what the helper's merge rounds to float32
    f32 = {k: v.to(F32) for k, v in base_tensors().items()}
    assert torch.equal(LR.merged_state(f32, [(a, s)])["conv.weight"], W2.to(F32))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_key():
    L = lora()
    cfg = tiny_ucfg()
    q = "lora_unet_down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_q"
    good = {q + ".lora_down.weight": torch.zeros(4, 128), q + ".lora_up.weight": torch.zeros(128, 4)}
    assert L.read_lora(good, unet_cfg=cfg).touched() == ("unet",)

    def refused(extra, exc, *words, drop=()):
        state = {k: v for k, v in dict(good, **extra).items() if k not in drop}
        with pytest.raises(exc) as e:
            L.read_lora(state, unet_cfg=cfg)
        assert all(w in str(e.value) for w in words), str(e.value)

    bogus = "lora_unet_down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_z.lora_down.weight"
    refused({bogus: torch.zeros(4, 128)}, KeyError, bogus, "lora_unet_down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_")
    refused({q + ".dora_scale": torch.zeros(1, 128)}, ValueError, q + ".dora_scale", "DoRA")
    refused({q + ".hada_w1_a": torch.zeros(4, 4)}, ValueError, q + ".hada_w1_a", "LoHa")
    refused({q + ".lokr_w1": torch.zeros(4, 4)}, ValueError, q + ".lokr_w1", "LoKr")
    refused({q + ".lora_down.weight": torch.zeros(4, 96)}, ValueError, q + ".lora_down.weight", "(4, 128)")
    refused({q + ".lora_up.weight": torch.zeros(64, 4)}, ValueError, q + ".lora_up.weight")
    refused({q + ".lora_up.weight": torch.zeros(128, 8)}, ValueError, q + ".lora_down.weight", q + ".lora_up.weight", "rank")
    refused({}, ValueError, q + ".lora_down.weight", drop=(q + ".lora_up.weight",))
    norm = "lora_unet_down_blocks_1_attentions_0_transformer_blocks_0_norm1.lora_down.weight"
    refused({norm: torch.zeros(4, 128)}, ValueError, norm, "does not load as a weight")
    conv = "lora_unet_down_blocks_0_resnets_0_conv1"
    refused({conv + ".lora_down.weight": torch.zeros(4, 64), conv + ".lora_up.weight": torch.zeros(64, 4)}, ValueError,
            conv + ".lora_down.weight", "(4, 64, 3, 3)")
    # strict=False: the unknown keys are skipped and reported, everything else still stands
    rec = L.read_lora(dict(good, **{bogus: torch.zeros(4, 128), "something.else": torch.zeros(1)}), unet_cfg=cfg, strict=False)
    assert rec.skipped == [bogus, "something.else"]
    assert list(rec.components["unet"]) == ["down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight"]
    with pytest.raises(ValueError):                 # ... but a refused adapter kind is refused in either mode
        L.read_lora(dict(good, **{q + ".dora_scale": torch.zeros(1, 128)}), unet_cfg=cfg, strict=False)


def test_provider_refuses_a_delta_that_does_not_fit():
    n = native()
    base = base_tensors()
    a = LR.make_adapter({"lin": (48, 32)}, 4, 6.0, 11)
    with pytest.raises(ValueError, match="lin.weight"):
        n.LoRAProvider(n.DictProvider(base), [(LR.targets(a), 1.0)]).weight("lin.weight", (48, 40))


# ---------------------------------------------------------------------------------------------------------------- in-place reload
def test_reload_rewrites_a_model_in_place_and_refuses_another_layout(monkeypatch):
    """On the CPU, where a packed model is ordinary tensors: reload(merged provider) gives the tensors of a model built from the merged
    state dict, in the SAME storage; reload(base) brings the first bits back; a provider of another architecture is refused."""
    n = native()
    cfg = R.tiny_unet_cfg()
    state = R.make_weights(R.unet_spec(cfg), 0)
    a_u, _, _ = tiny_adapters()
    net = n.NativeUNet(tiny_ucfg(), n.DictProvider(state), "cpu")
    before = {k: t.clone() for k, t in net.w.items()}
    ptrs = {k: t.data_ptr() for k, t in net.w.items()}
    net.reload(n.LoRAProvider(n.DictProvider(state), [(LR.targets(a_u), 1.0)]))
    fresh = n.NativeUNet(tiny_ucfg(), n.DictProvider(LR.merged_state(state, [(a_u, 1.0)])), "cpu")
    assert list(net.w) == list(fresh.w) and all(torch.equal(net.w[k], fresh.w[k]) for k in fresh.w)
    assert {k: t.data_ptr() for k, t in net.w.items()} == ptrs
    changed = {k for k in before if not torch.equal(before[k], net.w[k])}
    assert {"ctx_kv.weight", "temb_proj.weight", "down_blocks.0.resnets.0.conv1.weight", "up_blocks.0.upsamplers.0.conv.weight.sub4"} <= changed
    assert not any(k.endswith(".bias") and "_ln" not in k for k in changed) and "conv_in.weight" not in changed
    net.reload(n.DictProvider(state))
    assert all(torch.equal(before[k], net.w[k]) for k in before)
    real = net._load

    def another_layout(pv):
        real(pv)
        net.w["conv_in.bias"] = net.w["conv_in.bias"][:-1]
    monkeypatch.setattr(net, "_load", another_layout)
    with pytest.raises(ValueError, match="conv_in.bias"):
        net.reload(n.LoRAProvider(n.DictProvider(state), [(LR.targets(a_u), 1.0)]))
    assert all(torch.equal(before[k], net.w[k]) for k in before) and {k: t.data_ptr() for k, t in net.w.items()} == ptrs   # nothing changed


# ---------------------------------------------------------------------------------------------------------------- drivers
class StubPipe:
    def __init__(self):
        self.calls, self._n = [], 0

    def load_lora(self, src, scale=1.0, name=None, strict=True):
        self._n += 1
        self.calls.append(("load", src, scale))
        return f"a{self._n}"

    def unload_lora(self, name=None):
        self.calls.append(("unload", name))


class StubEngine:
    def __init__(self):
        self.dh = types.SimpleNamespace(pipe=StubPipe(), width_img=128, height_img=128, num_inference_steps=4)
        self.order = []

    def __getattr__(self, name):        # set_prompt1 / set_prompt2 / set_negative_prompt / swap_forward / set_dimensions ...
        def call(*a, **k):
            self.order.append(name)
            return []
        return call


def test_replay_loads_the_chain_s_adapters_once_before_the_first_key_frame(tmp_path):
    from latentblending_amd import replay
    be = StubEngine()
    replay.run_multi_transition(be, ["a", "b", "c"], [1, 2, 3], loras=[("x.safetensors", 0.8), {"path": "y.safetensors"}])
    pipe = be.dh.pipe
    assert pipe.calls == [("load", "x.safetensors", 0.8), ("load", "y.safetensors", 1.0), ("unload", "a2"), ("unload", "a1")]
    assert be.order.count("run_transition") == 2
    be = StubEngine()
    replay.run_multi_transition(be, ["a", "b"], [1, 2])
    assert be.dh.pipe.calls == []                   # no loras: the pipe's adapters are not touched
    with pytest.raises(ValueError, match="native pipe"):
        eng = StubEngine()
        eng.dh.pipe = object()
        replay.run_multi_transition(eng, ["a", "b"], [1, 2], loras=[("x", 1.0)])
    # the movie JSON: the header's "loras" round-trips through save / load and reaches the pipe, relative to the file
    be = StubEngine()
    items = [{"iteration": i, "seed": i, "prompt": f"p{i}", "negative_prompt": ""} for i in range(2)]
    fp = tmp_path / "movie.json"
    replay.save_movie_json(str(fp), be, items, loras=[("style.safetensors", 0.5)])
    assert json.load(open(fp))[0]["loras"] == [{"path": "style.safetensors", "scale": 0.5}]
    header, _ = replay.load_movie_json(str(fp))
    assert header["loras"] == [{"path": "style.safetensors", "scale": 0.5}]
    replay.run_movie_json(be, str(fp))
    assert be.dh.pipe.calls[0] == ("load", str(tmp_path / "style.safetensors"), 0.5) and be.dh.pipe.calls[-1] == ("unload", "a1")
    replay.save_movie_json(str(fp), be, items)
    assert "loras" not in json.load(open(fp))[0]


def test_frontend_passes_its_loras_on_and_writes_them(tmp_path, monkeypatch):
    import contextlib
    from latentblending_amd import frontend, replay
    be = StubEngine()
    session = types.SimpleNamespace(bound=lambda: contextlib.nullcontext(be))
    bv = frontend.BlendingVariableHolder(be, session, dp_out=str(tmp_path))
    bv.data = [{"iteration": i, "seed": i, "prompt": f"p{i}", "negative_prompt": "", "preview_image": ""} for i in range(2)]
    bv.loras = [("lcm.safetensors", 1.0)]
    seen = {}
    monkeypatch.setattr(replay, "run_multi_transition", lambda *a, **k: seen.update(k))
    bv.generate_movie()
    assert seen["loras"] == [("lcm.safetensors", 1.0)]
    bv.generate_movie(loras=[("other.safetensors", 0.3)])
    assert seen["loras"] == [("other.safetensors", 0.3)]
    bv.write_json()
    assert json.load(open(bv.fp_json))[0]["loras"] == [{"path": "lcm.safetensors", "scale": 1.0}]
