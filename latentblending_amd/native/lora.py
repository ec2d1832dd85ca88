"""Reading a LoRA file and resolving its keys to the parameters the native models load.

``read_lora(src)`` -> ``LoRARecord``: per component ("unet", "te1", "te2") a map from THE PARAMETER NAME THE PACKER ASKS ITS PROVIDER
FOR (``down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight``, ``text_model.encoder.layers.3.mlp.fc1.weight``) to
``(down, up, alpha)``: ``down`` [r, cin] or [r, cin, k, k], ``up`` [cout, r] or [cout, r, 1, 1] (fp32), ``alpha`` a float (the rank
when the file carries none).  ``weights.LoRAProvider`` merges such records into what a base provider yields; ``pipe.load_lora`` is the
user's entry.

Three namings are accepted (``unet_tables`` / ``clip_tables``), each resolved by BUILDING the table "file module name -> module name"
from the model's configuration - an underscore is never parsed back into a dot:

* ``peft``  - PEFT / diffusers: ``unet.<module>.lora_A.weight`` / ``.lora_B.weight``, the older ``.lora.down.weight`` / ``.lora.up.weight``
  and the attention-processor form ``unet.<block>.attn1.processor.to_q_lora.down.weight``; text towers under ``text_encoder.`` /
  ``text_encoder_2.``; optional ``<module>.alpha``;
* ``kohya`` - kohya-ss with diffusers block names: ``lora_unet_down_blocks_1_attentions_0_proj_in.lora_down.weight`` / ``.lora_up.weight``
  / ``.alpha`` (the published LCM-LoRA for SDXL), text towers ``lora_te1_...`` / ``lora_te2_...``;
* ``sgm``   - kohya-ss with the original SDXL block names (``input_blocks`` / ``middle_block`` / ``output_blocks``), derived from the
  ``UNetConfig``: levels, layers per block, which levels carry attention.

None of the three could be checked against a real file; the safety net is structural: every resolved name is a parameter
the model has, ``down`` / ``up`` have the shapes it implies, and an unknown key is an error under ``strict``.
"""
from __future__ import annotations

import difflib
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .clip import CLIPTextConfig
from .unet import UNetConfig

COMPONENTS = ("unet", "te1", "te2")
TEXT_KEY_PREFIXES = ("lora_te_", "lora_te1_", "lora_te2_", "text_encoder.", "text_encoder_2.")     # file keys of the text towers
Target = Tuple[torch.Tensor, torch.Tensor, float]

# (suffix of a file key, role); the longer forms first
_SUFFIXES = ((".lora_down.weight", "down"), (".lora_up.weight", "up"), (".lora_A.weight", "down"), (".lora_B.weight", "up"),
             ("_lora.down.weight", "down"), ("_lora.up.weight", "up"), (".lora.down.weight", "down"), (".lora.up.weight", "up"),
             (".alpha", "alpha"))
# adapter kinds that are not W + up * down: refused by the key that shows them
_REFUSED = (("dora_scale", "DoRA"), ("hada_w", "LoHa"), ("hada_t", "LoHa"), ("lokr_w", "LoKr"), ("lokr_t", "LoKr"),
            ("lora_mid", "Tucker-decomposed LoCon"))


# ---------------------------------------------------------------------------------------------------------------- the models' modules
def _transformer_modules(out, p, c, depth, cross):
    out[p + ".proj_in"] = (c, c)
    for d in range(depth):
        b = f"{p}.transformer_blocks.{d}"
        for n in ("to_q", "to_k", "to_v"):
            out[f"{b}.attn1.{n}"] = (c, c)
        out[b + ".attn1.to_out.0"] = (c, c)
        out[b + ".attn2.to_q"] = (c, c)
        out[b + ".attn2.to_k"] = out[b + ".attn2.to_v"] = (c, cross)
        out[b + ".attn2.to_out.0"] = (c, c)
        out[b + ".ff.net.0.proj"] = (8 * c, c)
        out[b + ".ff.net.2"] = (c, 4 * c)
    out[p + ".proj_out"] = (c, c)


def _resnet_modules(out, p, cin, cout, T):
    out[p + ".conv1"] = (cout, cin, 3, 3)
    out[p + ".time_emb_proj"] = (cout, T)
    out[p + ".conv2"] = (cout, cout, 3, 3)
    if cin != cout:
        out[p + ".conv_shortcut"] = (cout, cin, 1, 1)


def _unet_walk(cfg: UNetConfig):
    """(down blocks, up blocks) of the config as lists of (resnet (cin, cout), transformer depth) per layer - diffusers' layout."""
    ch = cfg.block_channels
    skips, prev, down = [ch[0]], ch[0], []
    for bi, c in enumerate(ch):
        down.append([((prev if li == 0 else c, c), cfg.transformer_depth[bi]) for li in range(cfg.layers_per_block)])
        skips += [c] * cfg.layers_per_block + ([c] if bi < len(ch) - 1 else [])
        prev = c
    up, hidden = [], ch[-1]
    for ui, c in enumerate(reversed(ch)):
        layers = []
        for _ in range(cfg.layers_per_block + 1):
            layers.append(((hidden + skips.pop(), c), cfg.transformer_depth[len(ch) - 1 - ui]))
            hidden = c
        up.append(layers)
    return down, up


def unet_modules(cfg: UNetConfig) -> Dict[str, Tuple[int, ...]]:
    """Module name (diffusers) -> weight shape, for every module whose ``.weight`` ``NativeUNet`` loads through ``provider.weight``."""
    ch, T, X = cfg.block_channels, cfg.time_embed_dim, cfg.cross_dim
    out: Dict[str, Tuple[int, ...]] = {"conv_in": (ch[0], cfg.in_channels, 3, 3)}
    if cfg.time_cond_proj_dim is not None:
        out["time_embedding.cond_proj"] = (ch[0], cfg.time_cond_proj_dim)
    out["time_embedding.linear_1"], out["time_embedding.linear_2"] = (T, ch[0]), (T, T)
    out["add_embedding.linear_1"], out["add_embedding.linear_2"] = (T, cfg.add_in_dim), (T, T)
    down, up = _unet_walk(cfg)
    for bi, layers in enumerate(down):
        for li, ((cin, cout), depth) in enumerate(layers):
            _resnet_modules(out, f"down_blocks.{bi}.resnets.{li}", cin, cout, T)
            if depth:
                _transformer_modules(out, f"down_blocks.{bi}.attentions.{li}", cout, depth, X)
        if bi < len(ch) - 1:
            out[f"down_blocks.{bi}.downsamplers.0.conv"] = (ch[bi], ch[bi], 3, 3)
    c = ch[-1]
    _resnet_modules(out, "mid_block.resnets.0", c, c, T)
    _transformer_modules(out, "mid_block.attentions.0", c, cfg.transformer_depth[-1], X)
    _resnet_modules(out, "mid_block.resnets.1", c, c, T)
    for ui, layers in enumerate(up):
        for li, ((cin, cout), depth) in enumerate(layers):
            _resnet_modules(out, f"up_blocks.{ui}.resnets.{li}", cin, cout, T)
            if depth:
                _transformer_modules(out, f"up_blocks.{ui}.attentions.{li}", cout, depth, X)
        if ui < len(ch) - 1:
            out[f"up_blocks.{ui}.upsamplers.0.conv"] = (layers[-1][0][1],) * 2 + (3, 3)
    out["conv_out"] = (cfg.out_channels, ch[0], 3, 3)
    return out


def _unet_norm_modules(cfg: UNetConfig) -> List[str]:
    """Modules the UNet has but does not load as a weight matrix (norms): a delta for one of them is refused, not unknown."""
    mods = unet_modules(cfg)
    out = ["conv_norm_out"]
    for m in mods:
        if m.endswith(".conv1"):
            out += [m[:-len("conv1")] + "norm1", m[:-len("conv1")] + "norm2"]
        elif m.endswith(".proj_in"):
            out.append(m[:-len("proj_in")] + "norm")
        elif m.endswith(".attn1.to_q"):
            out += [m[:-len("attn1.to_q")] + n for n in ("norm1", "norm2", "norm3")]
    return out


def clip_modules(cfg: CLIPTextConfig) -> Dict[str, Tuple[int, ...]]:
    """Module name (``transformers``, with the ``text_model.`` prefix) -> weight shape of a tower's projections."""
    c, m, out = cfg.hidden_size, cfg.intermediate_size, {}
    for i in range(cfg.num_hidden_layers):
        L = f"text_model.encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[L + "self_attn." + n] = (c, c)
        out[L + "mlp.fc1"], out[L + "mlp.fc2"] = (m, c), (c, m)
    return out


def _clip_norm_modules(cfg: CLIPTextConfig) -> List[str]:
    out = ["text_model.final_layer_norm", "text_model.embeddings.token_embedding", "text_model.embeddings.position_embedding"]
    for i in range(cfg.num_hidden_layers):
        out += [f"text_model.encoder.layers.{i}.layer_norm1", f"text_model.encoder.layers.{i}.layer_norm2"]
    return out


# ---------------------------------------------------------------------------------------------------------------- the three namings
def _sgm_blocks(cfg: UNetConfig) -> Dict[str, str]:
    """Original SDXL (SGM) block prefix -> diffusers block prefix, from the config."""
    ch, lpb = cfg.block_channels, cfg.layers_per_block
    blocks = {"input_blocks.0.0": "conv_in", "time_embed.0": "time_embedding.linear_1", "time_embed.2": "time_embedding.linear_2",
              "label_emb.0.0": "add_embedding.linear_1", "label_emb.0.2": "add_embedding.linear_2", "out.2": "conv_out"}
    n = 1
    for bi in range(len(ch)):
        for li in range(lpb):
            blocks[f"input_blocks.{n}.0"] = f"down_blocks.{bi}.resnets.{li}"
            if cfg.transformer_depth[bi]:
                blocks[f"input_blocks.{n}.1"] = f"down_blocks.{bi}.attentions.{li}"
            n += 1
        if bi < len(ch) - 1:
            blocks[f"input_blocks.{n}.0.op"] = f"down_blocks.{bi}.downsamplers.0.conv"
            n += 1
    blocks["middle_block.0"], blocks["middle_block.1"], blocks["middle_block.2"] = \
        "mid_block.resnets.0", "mid_block.attentions.0", "mid_block.resnets.1"
    for ui in range(len(ch)):
        depth = cfg.transformer_depth[len(ch) - 1 - ui]
        for li in range(lpb + 1):
            n = ui * (lpb + 1) + li
            blocks[f"output_blocks.{n}.0"] = f"up_blocks.{ui}.resnets.{li}"
            if depth:
                blocks[f"output_blocks.{n}.1"] = f"up_blocks.{ui}.attentions.{li}"
        if ui < len(ch) - 1:
            blocks[f"output_blocks.{n}.{2 if depth else 1}.conv"] = f"up_blocks.{ui}.upsamplers.0.conv"
    return blocks


_SGM_RESNET = {"conv1": "in_layers.2", "time_emb_proj": "emb_layers.1", "conv2": "out_layers.3", "conv_shortcut": "skip_connection"}


def _sgm_names(cfg: UNetConfig) -> Dict[str, str]:
    """SGM module name (dotted) -> diffusers module name, for every module of ``unet_modules``."""
    back = {v: k for k, v in _sgm_blocks(cfg).items()}
    out = {}
    for mod in unet_modules(cfg):
        if mod in back:
            out[back[mod]] = mod
            continue
        # the longest block prefix this module lies under (a resnet, a transformer), then the rest of its name
        prefix = max((b for b in back if mod.startswith(b + ".")), key=len, default=None)
        if prefix is None:          # (time_embedding.cond_proj: a diffusers-side module, the original UNet has no name for it)
            continue
        rest = mod[len(prefix) + 1:]
        out[back[prefix] + "." + _SGM_RESNET.get(rest, rest)] = mod
    return out


def unet_tables(cfg: UNetConfig) -> Dict[str, Dict[str, str]]:
    """naming -> {file module name (its component prefix included) -> module name}."""
    mods = unet_modules(cfg)
    return {"peft": {"unet." + m: m for m in mods},
            "kohya": {"lora_unet_" + m.replace(".", "_"): m for m in mods},
            "sgm": {"lora_unet_" + s.replace(".", "_"): m for s, m in _sgm_names(cfg).items()}}


def clip_tables(cfg: CLIPTextConfig, component: str) -> Dict[str, Dict[str, str]]:
    """The same for one text tower (``component``: "te1" / "te2"); the kohya and SGM forms of a tower are one and the same."""
    assert component in ("te1", "te2")
    mods = clip_modules(cfg)
    peft = "text_encoder." if component == "te1" else "text_encoder_2."
    kohya = {f"lora_{component}_" + m.replace(".", "_"): m for m in mods}
    return {"peft": {peft + m: m for m in mods}, "kohya": kohya, "sgm": dict(kohya)}


# ---------------------------------------------------------------------------------------------------------------- reading
@dataclass
class LoRARecord:
    """``components[c][parameter name] = (down, up, alpha)``; ``skipped``: file keys left out under ``strict=False``; ``naming``: the
    namings the file's keys were found in."""
    components: Dict[str, Dict[str, Target]] = field(default_factory=lambda: {c: {} for c in COMPONENTS})
    skipped: List[str] = field(default_factory=list)
    naming: Tuple[str, ...] = ()

    def touched(self) -> Tuple[str, ...]:
        return tuple(c for c in COMPONENTS if self.components[c])


def load_state(src) -> Dict[str, torch.Tensor]:
    if isinstance(src, dict):
        return src
    path = os.fspath(src)
    if os.path.isdir(path):
        files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
        if len(files) != 1:
            raise FileNotFoundError(f"read_lora: {path} holds {len(files)} .safetensors files; name the one to load")
        path = os.path.join(path, files[0])
    from safetensors.torch import load_file
    return load_file(path)


def _split(key: str) -> Optional[Tuple[str, str]]:
    """file key -> (file module name, role) or None.  The attention-processor form names its projection in the suffix:
    ``<block>.attn1.processor.to_q_lora.down.weight`` is the module ``<block>.attn1.to_q`` (``to_out`` -> ``to_out.0``)."""
    for suffix, role in _SUFFIXES:
        if key.endswith(suffix):
            stem = key[:-len(suffix)]
            if suffix.startswith("_lora."):
                head, sep, proj = stem.rpartition(".processor.")
                if not sep or proj not in ("to_q", "to_k", "to_v", "to_out"):
                    return None
                stem = head + "." + ("to_out.0" if proj == "to_out" else proj)
            return stem, role
    return None


def read_lora(src, unet_cfg: Optional[UNetConfig] = None, te_cfgs: Optional[Sequence[Optional[CLIPTextConfig]]] = None,
              strict: bool = True) -> LoRARecord:
    """``src``: a ``.safetensors`` file, a directory holding one, or a loaded ``dict[str, Tensor]``.  ``unet_cfg`` / ``te_cfgs`` = the
    configurations the names and shapes are resolved against (default: SDXL's UNet, CLIP-L/14 and OpenCLIP-bigG/14).
    ``strict`` (default): a key that resolves to nothing is a ``KeyError`` naming the key and the closest known module names; else
    such keys are left out and listed in ``.skipped``.  ``ValueError`` (always, naming the key): DoRA / LoHa / LoKr keys, ``down`` /
    ``up`` whose ranks differ or whose shapes do not fit the parameter, a delta for a parameter the model does not load as a weight."""
    state = load_state(src)
    unet_cfg = unet_cfg or UNetConfig()
    te_cfgs = tuple(te_cfgs) if te_cfgs is not None else (CLIPTextConfig.clip_l(), CLIPTextConfig.openclip_bigg())
    tables = {"unet": unet_tables(unet_cfg)}
    shapes = {"unet": unet_modules(unet_cfg)}
    others = {"unet." + m: m for m in _unet_norm_modules(unet_cfg)}
    others.update({"lora_unet_" + m.replace(".", "_"): m for m in _unet_norm_modules(unet_cfg)})
    for comp, cfg in zip(("te1", "te2"), te_cfgs):
        if cfg is not None:
            tables[comp], shapes[comp] = clip_tables(cfg, comp), clip_modules(cfg)
            peft = "text_encoder." if comp == "te1" else "text_encoder_2."
            for m in _clip_norm_modules(cfg):
                others[peft + m] = others[f"lora_{comp}_" + m.replace(".", "_")] = m
    lookup: Dict[str, Tuple[str, str, str]] = {}
    for comp, by_naming in tables.items():
        for naming, table in by_naming.items():
            for fname, mod in table.items():
                lookup.setdefault(fname, (comp, naming, mod))

    rec = LoRARecord()
    parts: Dict[Tuple[str, str], Dict[str, Tuple[str, torch.Tensor]]] = {}
    namings = []
    for key in state:
        for mark, kind in _REFUSED:
            if mark in key:
                raise ValueError(f"read_lora: key '{key}' belongs to a {kind} adapter; only plain LoRA (W + up * down) is merged")
        sp = _split(key)
        hit = lookup.get(sp[0]) if sp is not None else None
        if hit is None:
            stem = sp[0] if sp is not None else key
            if stem in others:
                raise ValueError(f"read_lora: key '{key}' is a delta for '{others[stem]}', which the native model does not load as a weight")
            if strict:
                near = difflib.get_close_matches(stem, list(lookup), n=3, cutoff=0.0)
                raise KeyError(f"read_lora: key '{key}' resolves to no parameter of the model (closest known module names: "
                               f"{', '.join(near)}); strict=False skips such keys")
            rec.skipped.append(key)
            continue
        comp, naming, mod = hit
        if naming not in namings:
            namings.append(naming)
        parts.setdefault((comp, mod), {})[sp[1]] = (key, state[key])
    rec.naming = tuple(namings)

    for (comp, mod), got in parts.items():
        keys = ", ".join(f"'{k}'" for k, _ in got.values())
        if "down" not in got or "up" not in got:
            raise ValueError(f"read_lora: module '{mod}' has {keys} but lacks its {'down' if 'down' not in got else 'up'} matrix")
        (kd, down), (ku, up) = got["down"], got["up"]
        shape = shapes[comp][mod]
        cout, cin, k = shape[0], shape[1], (shape[2] if len(shape) == 4 else 1)
        down, up = down.detach().to(torch.float32), up.detach().to(torch.float32)
        if down.ndim not in (2, 4) or up.ndim not in (2, 4) or any(int(s) != 1 for s in tuple(up.shape[2:])):
            raise ValueError(f"read_lora: '{kd}' {tuple(down.shape)} / '{ku}' {tuple(up.shape)}: not the matrices of a LoRA")
        r = int(down.shape[0])
        if int(up.shape[1]) != r:
            raise ValueError(f"read_lora: rank mismatch: '{kd}' has rank {r} but '{ku}' {tuple(up.shape)} has rank {int(up.shape[1])}")
        want_down = (r, cin, k, k) if len(shape) == 4 else (r, cin)
        if len(shape) == 2 and down.ndim == 4 and tuple(down.shape[2:]) == (1, 1):          # a linear stored 1x1-conv-shaped
            down = down.reshape(r, -1)
        if len(shape) == 4 and down.ndim == 2 and k == 1:
            down = down.reshape(r, -1, 1, 1)
        if tuple(down.shape) != want_down:
            raise ValueError(f"read_lora: '{kd}' has shape {tuple(down.shape)}; '{mod}.weight' {shape} needs {want_down}")
        if int(up.shape[0]) != cout:
            raise ValueError(f"read_lora: '{ku}' has shape {tuple(up.shape)}; '{mod}.weight' {shape} needs ({cout}, {r})")
        up = up.reshape((cout, r, 1, 1) if len(shape) == 4 else (cout, r))
        alpha = float(got["alpha"][1].detach().to(torch.float64).reshape(-1)[0]) if "alpha" in got else float(r)
        rec.components[comp][mod + ".weight"] = (down.contiguous(), up.contiguous(), alpha)
    return rec

