"""Parameter providers for the native SDXL modules.

The model builders walk their architecture and ask a provider for every parameter by its HF
diffusers state-dict name (``down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight``,
``decoder.up_blocks.2.resnets.0.conv1.weight`` ...; a guidance-distilled UNet config also asks for
``time_embedding.cond_proj.weight``), so the same walk serves

* ``DictProvider``      — a state dict: a real checkpoint's tensors (``from_safetensors``) or the
  seeded weights a test shares with the CPU oracle;
* ``SyntheticProvider`` — seeded random weights of the right shapes and scales, generated on the
  fly (no checkpoint on disk and no network here; ``bench.py`` says ``"data": "synthetic"``).
  Init: W ~ N(0, gain^2 / fan_in), b ~ N(0, 0.02^2), norm gamma ~ N(1, 0.05^2); residual-branch
  output projections use gain 0.5 so that 70 stacked transformer blocks stay tame in fp16.
  Values are rounded to fp16 so every consumer (fp16 device path, fp32 CPU oracle) sees
  bit-identical parameters.  Seeds depend only on (name, seed): order independent.
* ``LoRAProvider``      — wraps either and adds the low-rank deltas of loaded LoRA adapters to the weights it passes on
  (``native/lora.py`` reads the files); ``Reloadable.reload`` puts what such a provider packs into a live model in place.

``Packer`` turns what a provider yields into the device tensors of a model's ``w``; ``pad_to`` is the channel padding it and the
emitters share.
"""
from __future__ import annotations

import math
import os
import zlib
from typing import Dict, Optional, Sequence

import numpy as np
import torch


_BIG = 3 << 19        # tensors above this many elements (1.57 M: the 1280 x 1280 projections and up; the tiny test models
#                       stop at 1.18 M) take the chunked numpy path
_CHUNK = 1 << 18
_POOL = None


def _pool():
    global _POOL
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1)))
    return _POOL


def _seeded(name: str, shape: Sequence[int], std: float, seed: int, mean: float = 0.0) -> torch.Tensor:
    """N(mean, std^2) values from a seed that depends only on (name, seed).  Tensors up to 1.5 * 2^20 elements: one torch CPU
    generator (the scheme every golden fixture was made with).  Larger ones (only the full-size SDXL / CLIP models have them;
    2.6 G values took 76 s of one core per process): 2^18-element chunks, each from its own numpy PCG64 stream, filled by a
    small thread pool (numpy releases the GIL) - same values whatever the thread count."""
    base = (zlib.crc32(name.encode()) ^ (seed * 0x9E3779B1)) & 0x7FFFFFFF
    shape = tuple(int(v) for v in shape)
    n = 1
    for v in shape:
        n *= v
    if n <= _BIG:
        g = torch.Generator().manual_seed(base)
        return torch.randn(shape, generator=g, dtype=torch.float32) * std + mean
    buf = np.empty(n, dtype=np.float32)

    def fill(c):
        lo, hi = c * _CHUNK, min(n, (c + 1) * _CHUNK)
        np.random.Generator(np.random.PCG64([base, c])).standard_normal(hi - lo, dtype=np.float32, out=buf[lo:hi])
    list(_pool().map(fill, range((n + _CHUNK - 1) // _CHUNK)))
    return torch.from_numpy(buf).view(shape).mul_(std).add_(mean)


class SyntheticProvider:
    def __init__(self, seed: int = 0, keep: bool = False, cache_file: Optional[str] = None):
        """``keep``: remember every generated tensor in ``self.state`` (HF key -> fp32 tensor), e.g.
        so that a benchmark can time a CPU checker on exactly the weights the device path uses.
        ``cache_file``: a scratch file holding the generated tensors (fp16, exact: every value is rounded to fp16
        anyway).  Drawing 2.6 G normal deviates from one CPU generator takes about a minute per process; profiling
        sessions that start the same benchmark several times load the file instead (``save_cache`` writes it)."""
        self.seed = seed
        self.state: Optional[Dict[str, torch.Tensor]] = {} if keep else None
        self.cache_file = cache_file
        self._cache: Optional[Dict[str, torch.Tensor]] = None
        self._fresh: Dict[str, torch.Tensor] = {}
        if cache_file and os.path.isfile(cache_file):
            self._cache = torch.load(cache_file, map_location="cpu", mmap=True, weights_only=True)

    def save_cache(self) -> None:
        if self.cache_file and self._cache is None and self._fresh:
            tmp = self.cache_file + f".tmp{os.getpid()}"
            torch.save(self._fresh, tmp)
            os.replace(tmp, self.cache_file)
        self._fresh = {}

    def _out(self, name: str, shape: Sequence[int], make) -> torch.Tensor:
        shape = tuple(shape)
        if self._cache is not None and name in self._cache and tuple(self._cache[name].shape) == shape:
            t = self._cache[name].float()
        else:
            h = make().half()
            if self.cache_file and self._cache is None:
                self._fresh[name] = h
            t = h.float()
        if self.state is not None:
            self.state[name] = t
        return t

    def weight(self, name: str, shape: Sequence[int], fan_in: int, gain: float = 1.0) -> torch.Tensor:
        return self._out(name, shape, lambda: _seeded(name, shape, gain / math.sqrt(fan_in), self.seed))

    def bias(self, name: str, n: int) -> torch.Tensor:
        return self._out(name, (n,), lambda: _seeded(name, (n,), 0.02, self.seed))

    def norm_weight(self, name: str, n: int) -> torch.Tensor:
        return self._out(name, (n,), lambda: _seeded(name, (n,), 0.05, self.seed, mean=1.0))

    def positive(self, name: str, n: int) -> torch.Tensor:        # LPIPS lin layers (non-negative)
        return self._out(name, (n,), lambda: _seeded(name, (n,), 1.0, self.seed).abs() / n)


def pad_to(n: int, m: int) -> int:
    return (n + m - 1) // m * m


class Packer:
    """Packs what a provider yields into ``w`` (name -> tensor on ``device``) in the layouts the kernels read: the one place a
    model's ``_load`` gets its device tensors from.  fp16 for MFMA operands, fp32 for biases and norm parameters."""

    def __init__(self, provider, w: Dict[str, Optional[torch.Tensor]], device):
        self.pv, self.w, self.device = provider, w, torch.device(device)

    def dev(self, t: torch.Tensor, dtype) -> torch.Tensor:
        return t.to(device=self.device, dtype=dtype).contiguous()

    def linear(self, name, cin, cout, bias=True, gain=1.0, keep_host=False) -> torch.Tensor:
        """[cout][cin] fp16 + fp32 bias; returns the host weight (``keep_host``: the weight is NOT stored - the caller fuses it)."""
        w = self.pv.weight(name + ".weight", (cout, cin), cin, gain)
        if not keep_host:
            self.w[name + ".weight"] = self.dev(w, torch.float16)
        if bias:
            self.w[name + ".bias"] = self.dev(self.pv.bias(name + ".bias", cout), torch.float32)
        return w

    def norm(self, name, c, keep_host=False):
        g, b = self.pv.norm_weight(name + ".weight", c), self.pv.bias(name + ".bias", c)
        if not keep_host:
            self.w[name + ".weight"] = self.dev(g, torch.float32)
            self.w[name + ".bias"] = self.dev(b, torch.float32)
        return g, b

    def conv(self, name, cin, cout, k, gain=1.0, bias=True, bias_shift=0.0, fold=False) -> None:
        """[cout_p][k][k][cin_p] fp16 ((ky, kx, cin) order; cin padded to 8, cout to 4, with zeros) and an fp32 bias [cout_p].
        ``bias=False``: no bias parameter - ``None`` is stored.  ``fold``: y -> 2 y - 1 folded into the conv (``W * 2``: exact in
        fp16; ``b * 2 - 1``, also without a bias parameter)."""
        w = self.pv.weight(name + ".weight", (cout, cin, k, k), cin * k * k, gain)
        cin_p, cout_p = pad_to(cin, 8), pad_to(cout, 4)
        packed = torch.zeros(cout_p, k, k, cin_p, dtype=torch.float32)
        packed[:cout, :, :, :cin] = w.permute(0, 2, 3, 1)
        b = torch.zeros(cout_p, dtype=torch.float32)
        if bias:
            b[:cout] = self.pv.bias(name + ".bias", cout)
            if bias_shift:
                b[:cout] += bias_shift
        if fold:
            packed, b = packed * 2.0, b * 2.0
            b[:cout] -= 1.0
        self.w[name + ".weight"] = self.dev(packed.reshape(cout_p, k * k * cin_p), torch.float16)
        self.w[name + ".bias"] = self.dev(b, torch.float32) if (bias or fold) else None

    def upconv(self, name, c) -> None:
        """Upsampler conv (nearest-2x, then 3x3) stored as four 2x2 sub-pixel kernels (4/9 of the FLOPs)."""
        from ..hip.ops import subpixel_upsample_weights
        w = self.pv.weight(name + ".weight", (c, c, 3, 3), c * 9, 1.0)
        subs = subpixel_upsample_weights(w, pad_to(c, 8))
        for (py, px), k in subs.items():
            self.w[f"{name}.weight.sub{py}{px}"] = k.to(self.device)
        # the same four kernels stacked [4][N][4 Cin] (parity py*2+px) for the one-launch halo form
        self.w[f"{name}.weight.sub4"] = torch.stack([subs[(0, 0)], subs[(0, 1)], subs[(1, 0)], subs[(1, 1)]]).to(self.device).contiguous()
        self.w[name + ".bias"] = self.dev(self.pv.bias(name + ".bias", c), torch.float32)


class DictProvider:
    """State dict lookup; shapes are checked, scales/gains ignored."""

    def __init__(self, state: Dict[str, torch.Tensor], prefix: str = ""):
        self.state, self.prefix = state, prefix

    def _get(self, name: str, shape) -> torch.Tensor:
        key = self.prefix + name
        if key not in self.state:
            raise KeyError(f"parameter '{key}' missing from the state dict")
        t = self.state[key]
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"parameter '{key}': expected shape {tuple(shape)}, found {tuple(t.shape)}")
        return t.detach().to(torch.float32)

    def weight(self, name, shape, fan_in=0, gain=1.0):
        return self._get(name, shape)

    def bias(self, name, n):
        return self._get(name, (n,))

    def norm_weight(self, name, n):
        return self._get(name, (n,))

    def positive(self, name, n):
        t = self.state[self.prefix + name]
        return t.detach().to(torch.float32).reshape(n)


class LoRAProvider:
    """A provider that merges LoRA adapters into what ``base`` yields: ``weight(name, ...)`` returns

        W + sum_j  s_j * (alpha_j / r_j) * up_j @ down_j

    over the adapters that target ``name``, in load order, evaluated in float64 and rounded ONCE to float32 - so every layout the
    ``Packer`` derives (qkv, the gamma-folded copies and their colsum, ctx_kv, temb_proj, packed convs, the sub-pixel kernels) is
    that of the merged model.  ``adapters``: [(targets, scale), ...], ``targets`` = {parameter name: (down, up, alpha)} as
    ``lora.read_lora`` gives them per component; a conv's ``down`` [r, cin, k, k] is flattened to [r, cin k k] and the product
    reshaped to [cout, cin, k, k].  An adapter at scale 0 is SKIPPED, not multiplied by zero: the base tensor comes back bit for
    bit.  ``prefix``: what the adapters' names carry in front of the names this provider is asked for (a text tower loaded without
    its ``text_model.`` nesting).  ``bias``, ``norm_weight`` and ``positive`` pass through."""

    def __init__(self, base, adapters, prefix: str = ""):
        self.base, self.prefix = base, prefix
        self.adapters = [(targets, float(scale)) for targets, scale in adapters]

    def weight(self, name, shape, fan_in=0, gain=1.0):
        w = self.base.weight(name, shape, fan_in, gain)
        shape = tuple(int(v) for v in shape)
        acc = None
        for targets, scale in self.adapters:
            hit = targets.get(self.prefix + name) if scale != 0.0 else None
            if hit is None:
                continue
            down, up, alpha = hit
            r = int(down.shape[0])
            want = (r,) + shape[1:]
            if tuple(down.shape) != want or tuple(up.shape[:2]) != (shape[0], r) or up.numel() != shape[0] * r:
                raise ValueError(f"LoRA delta for '{self.prefix + name}' {shape}: down {tuple(down.shape)} / up {tuple(up.shape)} do not "
                                 f"fit (expected {want} and {(shape[0], r)})")
            if acc is None:
                acc = w.to(torch.float64)
            delta = up.to(torch.float64).reshape(shape[0], r) @ down.to(torch.float64).reshape(r, -1)
            acc = acc + (scale * (float(alpha) / r)) * delta.reshape(shape)
        return w if acc is None else acc.to(torch.float32)

    def bias(self, name, n):
        return self.base.bias(name, n)

    def norm_weight(self, name, n):
        return self.base.norm_weight(name, n)

    def positive(self, name, n):
        return self.base.positive(name, n)


class Reloadable:
    """In-place reload for a native model whose ``_load(provider)`` fills ``self.w``: recorded launch programs and their hipGraphs
    hold raw pointers into ``self.w``, so new weights are COPIED INTO the live tensors - none is replaced, no program is dropped, an
    instantiated graph replays against the new values."""

    def reload(self, provider) -> None:
        """Pack ``provider`` through the model's own ``_load`` into a scratch dict, refuse unless its keys, shapes and dtypes are
        those of the live ``w``, synchronise the device, ``copy_`` tensor by tensor.  Until it returns the device holds a second
        copy of the weights; it is freed (and handed back by the caching allocator) before the return."""
        live = self.w
        self.w = {}
        try:
            self._load(provider)
            fresh = self.w
        finally:
            self.w = live
        if list(fresh) != list(live):
            odd = sorted(set(fresh) ^ set(live))
            raise ValueError(f"{type(self).__name__}.reload: the provider packs other tensors than the live model holds ({odd[:4]} ...)")
        for k, t in fresh.items():
            have = live[k]
            if (t is None) != (have is None) or (t is not None and (t.shape != have.shape or t.dtype != have.dtype)):
                raise ValueError(f"{type(self).__name__}.reload: '{k}' is {None if t is None else (tuple(t.shape), t.dtype)} but the "
                                 f"live tensor is {None if have is None else (tuple(have.shape), have.dtype)}")
        self._write_live(fresh)
        fresh.clear()
        t = have = None
        if self.device.type == "cuda":
            torch.cuda.empty_cache()

    def _write_live(self, fresh) -> None:
        """``copy_`` every tensor of ``fresh`` (name -> tensor or None) into the live tensor of that name, between two synchronisations."""
        live = self.w
        cuda = self.device.type == "cuda"
        if cuda:
            torch.cuda.synchronize(self.device)         # launches that read the old weights may still be in flight
        with torch.no_grad():
            for k, t in fresh.items():
                if t is not None:
                    live[k].copy_(t)
        if cuda:
            torch.cuda.synchronize(self.device)


def from_safetensors(path: str, prefix: str = "") -> DictProvider:
    """HF-layout ``*.safetensors`` file or directory (e.g. ``unet/diffusion_pytorch_model.fp16.safetensors``)."""
    from safetensors.torch import load_file
    files = [path] if os.path.isfile(path) else sorted(
        os.path.join(path, f) for f in os.listdir(path) if f.endswith(".safetensors"))
    state: Dict[str, torch.Tensor] = {}
    for f in files:
        state.update(load_file(f))
    return DictProvider(state, prefix)


# AlexNet trunk conv indices inside torchvision's ``alexnet().features`` / the slices of ``lpips.pretrained_networks.alexnet``
_ALEX_FEATURE_IDX = (0, 3, 6, 8, 10)


def lpips_provider(alexnet_state: Dict[str, torch.Tensor], lin_state: Dict[str, torch.Tensor]) -> DictProvider:
    """Provider for ``NativeLPIPS`` from REAL checkpoints: the torchvision AlexNet trunk (keys ``features.N.weight`` /
    ``.bias``, or the ``net.sliceK.N.*`` names the same tensors carry inside a saved ``lpips.LPIPS`` module) and the
    learned linear layers of ``lpips`` v0.1 (``linK.model.1.weight``, shape [1, C, 1, 1]; the file
    ``lpips/weights/v0.1/alex.pth``).  The reference builds exactly this net with ``lpips.LPIPS(net='alex')``
    (/root/reference/latentblending/blending_engine.py:73-76)."""
    out: Dict[str, torch.Tensor] = {}
    for i, idx in enumerate(_ALEX_FEATURE_IDX):
        for kind in ("weight", "bias"):
            for key in (f"features.{idx}.{kind}", f"net.slice{i + 1}.{idx}.{kind}", f"net.features.{idx}.{kind}"):
                if key in alexnet_state:
                    out[f"net.conv{i + 1}.{kind}"] = alexnet_state[key]
                    break
            else:
                raise KeyError(f"AlexNet conv {i + 1} ({kind}): none of features.{idx}.{kind} / net.slice{i + 1}.{idx}.{kind} found")
        for key in (f"lin{i}.model.1.weight", f"lin{i}.weight", f"lins.{i}.model.1.weight"):
            if key in lin_state:
                out[f"lin{i}.weight"] = lin_state[key].reshape(-1)
                break
        else:
            raise KeyError(f"LPIPS linear layer {i}: lin{i}.model.1.weight not found")
    return DictProvider(out)
