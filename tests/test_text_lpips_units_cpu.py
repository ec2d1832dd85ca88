"""The references of tests/_text_lpips_units.py, checked before any kernel is held to them (no GPU):

* the CLIP REF against ``transformers``' own text tower in float64, every hidden state, the penultimate state and ``text_embeds``;
* the LPIPS REF against the oracle's ``lpips_features`` / ``lpips_distance`` (fp32) on the same weights, a non-square frame included;
* the *yardstick window*: for every unit the storage MODEL's rel-L2 error against REF, on CPU-generated inputs, lies in (0, 2^-9] - a
  zero yardstick would fail every kernel, a larger one would pass any (an fp16 store is 2^-11 per element and a unit has a few
  rounding points in series).  ``penultimate`` is a copy (held bit-equal, no yardstick) and the distances have an fp32 result (held
  to a derived bound): both are exempt;
* that each mutation the GPU suite must catch moves the MODEL past ``FACTOR`` x the yardstick (the model is broken, not a kernel);
* the marks and the arena journal of a tower program recorded on the CPU (nothing is launched).
"""
import dataclasses
import functools

import pytest
import torch
import torch.nn.functional as F

import _model_units as MU
import _text_lpips_units as TL
from oracle import sdxl_ref as R

F64 = torch.float64


@dataclasses.dataclass
class Cfg:
    """The fields of ``CLIPTextConfig`` the references read (the CPU tests need no native package for them)."""
    vocab_size: int = 1000
    hidden_size: int = 128
    intermediate_size: int = 256
    num_hidden_layers: int = 3
    num_attention_heads: int = 2
    max_position_embeddings: int = 77
    hidden_act: str = "gelu"
    layer_norm_eps: float = 1e-5
    projection_dim: int = 64
    bos_token_id: int = 998
    eos_token_id: int = 999
    pad_token_id: int = 1


TINY = Cfg()
CLIP_L2 = Cfg(hidden_size=768, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=12, hidden_act="quick_gelu",
              projection_dim=None, pad_token_id=999)
WIDE = Cfg(hidden_size=256, intermediate_size=1024, num_attention_heads=4, hidden_act="quick_gelu", projection_dim=None, pad_token_id=999)


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


# ---------------------------------------------------------------------------------------------------------------- CLIP REF vs transformers
def _hf_clip(c, seed):
    """The recipe of tests/test_native_gpu.py: random init widened 2.5x, fp16-representable parameters; here moved to float64."""
    from transformers import CLIPTextConfig as HFConfig, CLIPTextModel, CLIPTextModelWithProjection
    hf = HFConfig(vocab_size=c.vocab_size, hidden_size=c.hidden_size, intermediate_size=c.intermediate_size,
                  num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
                  max_position_embeddings=c.max_position_embeddings, hidden_act=c.hidden_act,
                  layer_norm_eps=c.layer_norm_eps, projection_dim=c.projection_dim or 512,
                  bos_token_id=c.bos_token_id, eos_token_id=c.eos_token_id, pad_token_id=c.pad_token_id)
    torch.manual_seed(seed)
    model = (CLIPTextModelWithProjection if c.projection_dim else CLIPTextModel)(hf).eval()
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if prm.dim() == 2 and "embedding" not in name:
                prm.mul_(2.5)
        for prm in model.parameters():
            prm.copy_(prm.half().float())
    return model


@pytest.mark.parametrize("cfg", [TINY, CLIP_L2], ids=["w128_L3_gelu_proj", "w768_L2_quick_gelu"])
def test_clip_ref_matches_transformers_in_float64(cfg):
    """Every hidden state, the penultimate state and text_embeds of transformers' tower, run in double, against the free-running REF.
    Both sides are float64 evaluations of the same function: 1e-12 leaves four digits for the different summation orders."""
    hf = _hf_clip(cfg, 5)
    # (transformers nests the tower under "text_model." or not, depending on class and version)
    w = {k if k.startswith((TL.TM, "text_projection.")) else TL.TM + k: v.detach().clone()
         for k, v in hf.state_dict().items() if v.is_floating_point()}
    ids = TL.make_ids(cfg, (1, 9, 40, 76))
    with torch.no_grad():
        out = hf.double()(input_ids=ids, output_hidden_states=True)
    assert out.hidden_states[0].dtype == F64
    ref, _ = MU.evs(w)
    got = TL.clip_forward(ref, cfg, ids)
    n = cfg.num_hidden_layers
    states = [got["embed"]] + [got[f"L{i}.fc2"] for i in range(n)]
    assert len(out.hidden_states) == n + 1
    for i, (mine, theirs) in enumerate(zip(states, out.hidden_states)):
        assert rel_l2(mine.view_as(theirs), theirs) <= 1e-12, i
    assert rel_l2(got["penultimate"], out.hidden_states[-2]) <= 1e-12
    assert torch.equal(got["penultimate"].reshape(-1, cfg.hidden_size), states[-2])
    if cfg.projection_dim:
        assert rel_l2(got["pooled"], out.text_embeds) <= 1e-12
    else:       # the pooled row of a tower without projection: transformers' pooler_output is final_layer_norm(last)[EOS row]
        fin = F.layer_norm(states[-1], (cfg.hidden_size,), ref.w[TL.TM + "final_layer_norm.weight"], ref.w[TL.TM + "final_layer_norm.bias"],
                           cfg.layer_norm_eps)
        assert rel_l2(fin[TL.eos_rows(cfg, ids)], out.pooler_output) <= 1e-12


def test_eos_rule():
    ids = TL.make_ids(CLIP_L2, (1, 76))                 # pad id = eos id: the FIRST eos counts
    assert TL.eos_rows(CLIP_L2, ids).tolist() == [1, 77 + 76]
    legacy = dataclasses.replace(TINY, eos_token_id=2, bos_token_id=0)
    ids = torch.tensor([[0, 5, 900, 2, 1] + [1] * 72])  # legacy configs: the argmax of the ids, not the eos
    assert TL.eos_rows(legacy, ids).tolist() == [2]


# ---------------------------------------------------------------------------------------------------------------- CLIP yardsticks
@functools.lru_cache(maxsize=None)
def clip_case(which):
    cfg = {"tiny": TINY, "tiny_hot": TINY, "wide_quick": WIDE}[which]
    w = TL.clip_weights(cfg, 3)
    if which == "tiny_hot":
        w = TL.make_hot(w, cfg)
    ref, model = MU.evs(w)
    ids = TL.make_ids(cfg, (1, 40, 76))
    free = TL.clip_forward(model, cfg, ids)             # CPU-generated unit inputs: what a program would hand on
    free["ids"] = ids
    return cfg, ref, model, ids, free


def _unit_pair(which, name, kind, ins, ref=None, model=None, cfg2=None):
    cfg, r, m, _, free = clip_case(which)
    given = [free[i] for i in ins]
    return (TL.clip_unit(ref or r, cfg, name, kind, given), TL.clip_unit(model or m, cfg2 or cfg, name, kind, given))


@pytest.mark.parametrize("which", ["tiny", "tiny_hot", "wide_quick"])
def test_clip_yardstick_window(which):
    cfg = clip_case(which)[0]
    seen = {}
    for name, kind, ins in TL.clip_units(cfg):
        r, m = _unit_pair(which, name, kind, ins)
        assert torch.isfinite(r).all() and torch.isfinite(m).all(), name
        if kind == "penultimate":
            assert torch.equal(m.double(), r)           # a copy: no yardstick, the GPU suite asks for the same bits
            continue
        seen[name] = MU.errors(m, r)[0]
    print(which, {k: f"{v:.2e}" for k, v in seen.items()})
    bad = {k: v for k, v in seen.items() if not 0.0 < v <= TL.WINDOW}
    assert not bad, bad


def test_hot_case_carries_outliers():
    """The hot weights do what they are for: in the fp64 residual stream entering the last layer the two hot channels are about 100
    times the typical (median) magnitude, every value is finite and far inside fp16's range."""
    cfg, ref, _, ids, _ = clip_case("tiny_hot")
    x = TL.clip_forward(ref, cfg, ids)["penultimate"].reshape(-1, cfg.hidden_size).abs()
    typical = float(x.median())
    hot = float(x[:, list(TL.HOT_CHANNELS)].median())
    print(f"typical {typical:.3f} hot {hot:.3f} max {float(x.max()):.1f} ratio {hot / typical:.0f}")
    assert 50 <= hot / typical <= 200 and float(x.max()) < 6e3
    cold = TL.clip_forward(clip_case("tiny")[1], cfg, ids)["penultimate"].abs()
    assert float(cold.max() / cold.median()) < 12     # what the synthetic weights lack


# ---------------------------------------------------------------------------------------------------------------- CLIP mutations
def _broken(which, name, kind, ins, **change):
    """Is a MODEL broken by ``change`` (a config field, or a patched helper) over FACTOR x the sound MODEL's error on this unit?"""
    r, m = _unit_pair(which, name, kind, ins)
    good = MU.errors(m, r)
    _, b = _unit_pair(which, name, kind, ins, cfg2=dataclasses.replace(clip_case(which)[0], **change))
    bad = MU.errors(b, r)
    return bad[0] > MU.FACTOR * good[0] or bad[1] > MU.FACTOR * good[1], good, bad


def test_mutation_wrong_eos_row(monkeypatch):
    cfg = clip_case("tiny")[0]
    name, kind, ins = TL.clip_units(cfg)[-1]
    r, m = _unit_pair("tiny", name, kind, ins)
    rule = TL.eos_rows
    monkeypatch.setattr(TL, "eos_rows", lambda c, ids: rule(c, ids) - 1)        # the row in front of the EOS
    _, b = _unit_pair("tiny", name, kind, ins)
    assert MU.errors(b, r)[0] > 100 * MU.FACTOR * MU.errors(m, r)[0]


def test_mutation_causal_mask_off_by_one(monkeypatch):
    cfg = clip_case("tiny")[0]
    name, kind, ins = "L0.attn", "attn", ("L0.qkv",)
    r, m = _unit_pair("tiny", name, kind, ins)
    monkeypatch.setattr(TL, "CAUSAL_DIAGONAL", 1)                               # every query sees the key behind it
    _, b = _unit_pair("tiny", name, kind, ins)
    good, bad = MU.errors(m, r), MU.errors(b, r)
    assert bad[0] > 100 * MU.FACTOR * good[0] and bad[1] > 100 * MU.FACTOR * good[1]
    # ... and on the first row alone, which a global norm over 77 rows would drown
    row0 = (b[0].double() - r[0]).abs().max()
    assert float(row0) > 100 * MU.FACTOR * good[1]


def test_mutation_layernorm_eps():
    """eps 1e-6 for 1e-5: visible where the variance is small - the first LayerNorm reads the embedding sum, variance about 5e-4 -
    and invisible behind it (variance about 0.1): the census of units, not a global norm, is what catches it."""
    hit, good, bad = _broken("tiny", "L0.qkv", "qkv", ("embed",), layer_norm_eps=1e-6)
    assert hit and bad[0] > 5 * MU.FACTOR * good[0], (good, bad)
    assert not _broken("tiny", "L2.qkv", "qkv", ("L1.fc2",), layer_norm_eps=1e-6)[0]


def test_mutation_quick_gelu_constant(monkeypatch):
    """1.7 for 1.702 stays inside FACTOR x the yardstick of the fc1 unit (the docstring of ``quick_gelu_fit`` says why); the fitted
    constant is what catches it: the sound MODEL is inside the bound, the mutated one 10 times outside."""
    cfg, ref, model, _, free = clip_case("wide_quick")
    x = free["L1.out"]
    pre = TL.fc1_pre(ref, cfg, 1, x)
    r, m = _unit_pair("wide_quick", "L1.fc1", "fc1", ("L1.out",))
    monkeypatch.setattr(TL, "activation", lambda c, t: t * torch.sigmoid(1.7 * t))
    _, b = _unit_pair("wide_quick", "L1.fc1", "fc1", ("L1.out",))
    good, bad = MU.errors(m, r), MU.errors(b, r)
    assert bad[0] <= MU.FACTOR * good[0] and bad[1] <= MU.FACTOR * good[1]
    e_rms = MU.FACTOR * float((m.double() - r).pow(2).mean().sqrt())
    dk, bound = TL.quick_gelu_fit(m, pre, e_rms)
    dk_bad, _ = TL.quick_gelu_fit(b, pre, e_rms)
    print(f"dk model {dk:.2e} mutated {dk_bad:.2e} bound {bound:.2e}")
    assert abs(dk) <= bound and abs(dk_bad) > 10 * bound and abs(dk_bad + 0.002) < 2e-4


# ---------------------------------------------------------------------------------------------------------------- LPIPS
@functools.lru_cache(maxsize=None)
def lpips_case():
    w = R.make_weights(R.lpips_spec(), 7)
    ref, model = MU.evs(w)
    base = TL.smooth_frames(2, 131, 163, 21)
    frames = torch.stack([base[0], TL.lerp_u8(base[0], base[1], 0.25), base[1], TL.nudge(base[0])])
    return w, ref, model, frames


def _oracle_input(frames):
    return (2 * frames.float() / 255 - 1).permute(0, 3, 1, 2)


def test_lpips_ref_matches_oracle():
    """REF (float64) against the oracle (fp32) on a non-square frame set: features within 1e-5 rel-L2 (fp32 accumulation over at most
    3456 terms), every distance within 1e-4 relatively - the near-identical pair included, whose fp32 evaluation is the noisier."""
    w, ref, _, frames = lpips_case()
    mine = TL.lpips_forward(ref, frames)
    theirs = R.lpips_features(w, _oracle_input(frames))
    geo = TL.lpips_geometry(131, 163)
    for t, o, (_, _, ho, wo, c) in zip(mine, theirs, geo):
        assert tuple(t.shape) == tuple(o.shape) == (4, c, ho, wo)
        assert rel_l2(t, o) <= 1e-5
    for a, b in ((0, 1), (0, 2), (1, 2), (0, 3)):
        d = float(TL.lpips_tap_terms(ref, [t[a:a + 1] for t in mine], [t[b:b + 1] for t in mine]).sum())
        want = float(R.lpips_distance(w, _oracle_input(frames[a:a + 1]), _oracle_input(frames[b:b + 1])))
        assert d > 0 and abs(d - want) <= 1e-4 * want, (a, b, d, want)
    assert float(TL.lpips_tap_terms(ref, [t[1:2] for t in mine], [t[1:2] for t in mine]).sum()) == 0.0


def test_lpips_frames_are_smooth_and_pairs_ordered():
    """Neighbouring frames are close: d(0, lerp .25) < d(0, 2), and the nudged frame is nearer still, by orders of magnitude."""
    _, ref, _, frames = lpips_case()
    taps = TL.lpips_forward(ref, frames)

    def d(a, b):
        return float(TL.lpips_tap_terms(ref, [t[a:a + 1] for t in taps], [t[b:b + 1] for t in taps]).sum())
    assert 0 < d(0, 3) < 1e-2 * d(0, 1) < 1e-2 * d(0, 2)
    x = frames.float()
    assert float((x[:, 1:] - x[:, :-1]).abs().mean()) < 6.0          # white noise would be about 85


def test_lpips_yardstick_window():
    _, ref, model, frames = lpips_case()
    free = dict(zip(TL.LPIPS_TAPS, TL.lpips_forward(model, frames)))
    free["frames"] = frames
    seen = {}
    for name, ins in TL.lpips_units():
        r, m = TL.lpips_unit(ref, name, free[ins[0]]), TL.lpips_unit(model, name, free[ins[0]])
        seen[name] = MU.errors(m, r)[0]
    r, m = TL.lpips_prep(ref, frames), TL.lpips_prep(model, frames)
    seen["prep"] = MU.errors(m, r)[0]
    print({k: f"{v:.2e}" for k, v in seen.items()})
    bad = {k: v for k, v in seen.items() if not 0.0 < v <= TL.WINDOW}
    assert not bad, bad


def test_lpips_mutations():
    """A dropped ReLU, a pool window of 2 and ``lin`` weights of the wrong tap each move the MODEL far past FACTOR x the yardstick
    (a distance: past the derived bound)."""
    w, ref, model, frames = lpips_case()
    free = dict(zip(TL.LPIPS_TAPS, TL.lpips_forward(model, frames)))
    r, m = TL.lpips_unit(ref, "conv4", free["conv3"]), TL.lpips_unit(model, "conv4", free["conv3"])
    good = MU.errors(m, r)
    no_relu = model.q(R._conv(model.t(free["conv3"]), model.w, "net.conv4"))
    assert MU.errors(no_relu, r)[0] > 100 * MU.FACTOR * good[0]
    r, m = TL.lpips_unit(ref, "conv2", free["conv1"]), TL.lpips_unit(model, "conv2", free["conv1"])
    p2 = TL.lpips_unit(model, "conv2", free["conv1"], pool=2)
    p2 = p2[..., :r.shape[-2], :r.shape[-1]]
    assert MU.errors(p2, r[..., :p2.shape[-2], :p2.shape[-1]])[0] > 100 * MU.FACTOR * MU.errors(m, r)[0]
    ta, tb = [t[0:1] for t in free.values()], [t[1:2] for t in free.values()]
    terms = TL.lpips_tap_terms(ref, ta, tb)
    shapes = [(t.shape[-2] * t.shape[-1], t.shape[-3]) for t in ta]
    bound = TL.lpips_distance_bound(terms, shapes)
    swapped = MU.Ev(torch.float32, {**w, "lin3.weight": w["lin4.weight"], "lin4.weight": w["lin3.weight"]}, True)
    assert abs(float(TL.lpips_tap_terms(model, ta, tb).sum()) - float(terms.sum())) <= bound
    assert abs(float(TL.lpips_tap_terms(swapped, ta, tb).sum()) - float(terms.sum())) > 100 * bound


def test_lpips_chain_and_bound():
    assert TL.lpips_chain(63 * 63, 192) == 3 + 8 + 6 + 4 and TL.lpips_chain(5, 256) == 4 + 1 + 6 + 4
    assert TL.lpips_distance_bound([1.0], [(16, 64)]) == (1 + 1 + 6 + 4 + 16) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- the hook, recorded on the CPU
@pytest.fixture
def cpu_native(monkeypatch):
    """The native package with every launch stream replaced by None: a tower program records on the CPU."""
    import latentblending_amd.native as n
    import latentblending_amd.native.runtime as rt
    import latentblending_amd.native.clip as CL
    for mod in (rt, CL):
        monkeypatch.setattr(mod, "_stream", lambda: None)
    return n


@pytest.mark.parametrize("proj", [64, None])
def test_clip_journal_and_marks(cpu_native, proj):
    n = cpu_native
    c = dataclasses.replace(TINY, projection_dim=proj)
    cfg = n.CLIPTextConfig(**dataclasses.asdict(c))
    tower = n.NativeCLIPText(cfg, n.DictProvider(TL.clip_weights(c, 3)), "cpu")
    plain, prog = tower.build(2), tower.build(2, journal=True)
    assert plain.arena.journal is None and prog.arena.journal
    assert plain.prog.op_names() == prog.prog.op_names()                # the hook changes no op
    assert [len(t) for t in plain.arena.all] == [len(t) for t in prog.arena.all]
    names = prog.prog.op_names()
    assert names.count("lb_attn_fwd_d64") == 3 and names.count("lb_layernorm_f16") == 6 + (1 if proj else 0)
    for pr in (plain, prog):
        MU.check_marks(pr.marks, {pr.prog.name: pr.prog}, ("ids",))
        assert [(m.name, m.kind, m.inputs) for m in pr.marks] == TL.clip_units(c)
        assert pr.marks[-1].op_end == pr.prog.num_ops
    assert [m.op_end for m in plain.marks] == [m.op_end for m in prog.marks]
    by = {m.name: m for m in prog.marks}
    assert by["penultimate"].out is prog.penultimate and tuple(by["L0.qkv"].out.shape) == (154, 384)
    if proj:
        assert by["pooled"].out is prog.pooled
    live, _ = MU.journal_state(prog.arena.journal, len(prog.arena.all))
    assert not live                                                      # every arena buffer is back at the end of emission
    assert all(name == prog.prog.name and 0 <= op <= prog.prog.num_ops for _, _, name, op in prog.arena.journal)
    assert tower._programs == {}                                         # ``build`` is not ``forward``'s cache
