"""Recorder of what the native models pack and emit: for a fixed list of cases, every program's op names, every mark, the arena's
totals, a digest of the arena journal, and one digest per packed weight (``compact`` is how the file holds them).  It reads nothing but the models' public surface
(``net.w``, ``net.build``, ``.prog`` / ``.prog_cond`` / ``.prog_step``, ``.marks``, ``.arena``, ``.c64_launches``), so the same file
runs on any commit; two commits that record the same thing pack the same bits and launch the same ops.

    python -m oracle.record_native_models --out tests/golden/native_models.json        # the tiny cases, recorded on the CPU
    python -m oracle.record_native_models --production --out <file>                    # the benchmark's shapes, on the device

``tests/golden/native_models.json`` was written by the first command at the commit BEFORE the packer and the program base were
shared (``tests/test_native_models_cpu.py`` holds every later commit to it).  The CPU recording launches nothing: every module's
``_stream`` is replaced by ``lambda: None``, as tests/test_model_units_cpu.py does."""
from __future__ import annotations

import argparse
import hashlib
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_MODULES = ("runtime", "unet", "vae", "tiny_vae", "clip", "lpips")

# the tiny configs of the test suite (oracle.sdxl_ref.tiny_unet_cfg, tests/test_model_units_cpu.py, tests/test_text_lpips_units_cpu.py)
TINY_UNET = dict(block_channels=(64, 128, 256), transformer_depth=(0, 1, 2), cross_dim=256, pooled_dim=128, add_time_dim=32,
                 sample_size=16)
TINY_VAE = (64, 128, 128, 128)
WIDE_VAE = (64, 128, 256, 512)          # a 512-channel top level: the only one that packs ``qkv.*``
TINY_CLIP = dict(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2,
                 bos_token_id=998, eos_token_id=999, pad_token_id=1)


class patched_streams:
    """Every native module's ``_stream`` replaced by ``lambda: None`` (nothing is launched while a program records)."""

    def __enter__(self):
        self.saved = []
        for name in _MODULES:
            mod = importlib.import_module("latentblending_amd.native." + name)
            if hasattr(mod, "_stream"):
                self.saved.append((mod, mod._stream))
                mod._stream = lambda: None
        return self

    def __exit__(self, *exc):
        for mod, fn in self.saved:
            mod._stream = fn


class ShapeProvider:
    """Parameters of the right shapes and no particular values (zeros; norm weights one): the production recording reads the
    programs, which do not depend on the values."""

    def weight(self, name, shape, fan_in=0, gain=1.0):
        return torch.zeros(tuple(shape))

    def bias(self, name, n):
        return torch.zeros(n)

    def norm_weight(self, name, n):
        return torch.ones(n)

    positive = norm_weight


def _sha(*parts) -> str:
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else repr(p).encode())
        h.update(b"\0")
    return h.hexdigest()


def weight_digests(net) -> dict:
    """One sha256 per ``net.w`` entry over (key, dtype, shape, contiguity, raw bytes), ``None`` for ``None``, in sorted key order."""
    out = {}
    for key in sorted(net.w):
        t = net.w[key]
        if t is None:
            out[key] = None
            continue
        raw = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
        out[key] = _sha(key, str(t.dtype), tuple(t.shape), bool(t.is_contiguous()), raw)
    return out


def _programs(p):
    return [q for q in (getattr(p, n, None) for n in ("prog", "prog_cond", "prog_step")) if q is not None]


def program_record(p) -> dict:
    """What one program object recorded."""
    rec = {"programs": {q.name: q.op_names() for q in _programs(p)},
           "marks": [[m.name, m.kind, m.program, int(m.op_end), list(m.inputs), list(m.out.shape), str(m.out.dtype)]
                     for m in getattr(p, "marks", [])],
           "tap_names": dict(getattr(p, "tap_names", {})),
           "arena": [int(p.arena.bytes_allocated), len(p.arena.all)],
           "journal": None if p.arena.journal is None else _sha(json.dumps([list(e) for e in p.arena.journal]))}
    if hasattr(p, "c64_launches"):
        rec["c64_launches"] = int(p.c64_launches)
    return rec


# ------------------------------------------------------------------------------------------------ the tiny cases (CPU)
def tiny_cases(n, device="cpu"):
    """-> (cases, weights): ``cases[name]`` = a program record, ``weights[net name]`` = the digests of that net's ``w``."""
    from latentblending_amd.native.lpips import NativeLPIPS
    cases, weights = {}, {}

    def unet(name, fuse="auto", **cfg):
        net = n.NativeUNet(n.UNetConfig(**{**TINY_UNET, **cfg}), n.SyntheticProvider(0), device, fuse_layernorm=fuse)
        weights[name] = weight_digests(net)
        return net

    for fuse in (False, True, "auto"):
        net = unet(f"unet.fuse_{fuse}", fuse)
        cases[f"unet.fuse_{fuse}.B2.L16"] = program_record(net.build(2, 16, journal=True))
    for ragged in (True, False):            # (``net``: the "auto" UNet)
        cases[f"unet.B2.16x24.ragged_{ragged}"] = program_record(net.build(2, (16, 24), ragged_halo=ragged, journal=True))
    cases["unet.B3.8x16"] = program_record(net.build(3, (8, 16), journal=True))
    cases["unet.guided.B2.L16"] = program_record(unet("unet.guided", time_cond_proj_dim=32).build(2, 16, journal=True))

    def vae(name, ch=TINY_VAE, **cfg):
        net = n.NativeVAEDecoder(n.VAEConfig(block_channels=ch, **cfg), n.SyntheticProvider(1), device)
        weights[name] = weight_digests(net)
        return net

    net = vae("vae.scaled")
    cases["vae.scaled.B2.L16"] = program_record(net.build(2, 16, journal=True))
    for ragged in (True, False):
        cases[f"vae.scaled.B3.16x24.ragged_{ragged}"] = program_record(net.build(3, (16, 24), ragged_halo=ragged, journal=True))
    net = vae("vae.f32", stream_fp16_scaled=False)
    cases["vae.f32.B2.L16"] = program_record(net.build(2, 16, journal=True))
    cases["vae.f32.B2.8x16"] = program_record(net.build(2, (8, 16), journal=True))
    cases["vae.unfused_attn.B2.L16"] = program_record(vae("vae.unfused_attn", fused_mid_attention=False).build(2, 16, journal=True))
    net = vae("vae.wide", WIDE_VAE)
    cases["vae.wide.B1.L8"] = program_record(net.build(1, 8, journal=True))
    cases["vae.wide.B2.8x12"] = program_record(net.build(2, (8, 12), journal=True))

    for half, cls in (("dec", n.NativeTinyVAEDecoder), ("enc", n.NativeTinyVAEEncoder)):
        net = cls(n.TinyVAEConfig(), n.SyntheticProvider(2), device)
        weights[f"tiny.{half}"] = weight_digests(net)
        for B, L in ((2, 8), (2, 16), (2, (16, 24)), (3, (8, 12))):      # (L = 8: no conv reaches the C64 threshold; the others do)
            for c64 in (True, False):
                size = f"L{L}" if isinstance(L, int) else f"{L[0]}x{L[1]}"
                cases[f"tiny.{half}.B{B}.{size}.c64_{c64}"] = program_record(net.build(B, L, c64=c64))

    for act in ("quick_gelu", "gelu"):
        for proj in (None, 64):
            name = f"clip.{act}.proj_{proj}"
            cfg = n.CLIPTextConfig(**TINY_CLIP, hidden_act=act, projection_dim=proj)
            net = n.NativeCLIPText(cfg, n.SyntheticProvider(3), device)
            weights[name] = weight_digests(net)
            for B in (1, 2):
                cases[f"{name}.B{B}"] = program_record(net.build(B, journal=True))

    weights["lpips"] = weight_digests(NativeLPIPS(n.SyntheticProvider(7), device))
    return cases, weights


# ------------------------------------------------------------------------------------------------ the benchmark's shapes (device)
def production_cases(n, device):
    pv, cases = ShapeProvider(), {}
    net = n.NativeUNet(n.UNetConfig(), pv, device)
    for B in (2, 17):
        cases[f"unet.B{B}.L64"] = program_record(net.build(B, 64, journal=True))
    del net
    cases["vae.B17.L64"] = program_record(n.NativeVAEDecoder(n.VAEConfig(), pv, device).build(17, 64, journal=True))
    cases["tiny.dec.B17.L64"] = program_record(n.NativeTinyVAEDecoder(n.TinyVAEConfig(), pv, device).build(17, 64))
    for name, cfg in (("clip_l", n.CLIPTextConfig.clip_l()), ("openclip_bigg", n.CLIPTextConfig.openclip_bigg())):
        cases[f"{name}.B2"] = program_record(n.NativeCLIPText(cfg, pv, device, prefix="").build(2, journal=True))
    return cases


def record(production: bool = False, device: str = None) -> dict:
    import latentblending_amd.native as n
    if production:
        return {"cases": production_cases(n, device or "cuda:0")}
    with patched_streams():
        cases, weights = tiny_cases(n, device or "cpu")
    return {"cases": cases, "weights": weights}


def compact(rec: dict) -> dict:
    """The file form of a record, lossless: every list of op names, of marks and of weight digests (in sorted key order - a digest
    covers its key) becomes a list of indices into ONE table of the distinct values.  The nets share most of their weights and the
    cases most of their marks, so the file holds each sha256 and each mark once."""
    table, index = [], {}

    def intern(values):
        out = []
        for v in values:
            k = json.dumps(v)
            if k not in index:
                index[k] = len(table)
                table.append(v)
            out.append(index[k])
        return out
    out = {"cases": {name: {**c, "programs": {p: intern(ops) for p, ops in sorted(c["programs"].items())}, "marks": intern(c["marks"])}
                     for name, c in sorted(rec["cases"].items())}}
    if "weights" in rec:
        out["weights"] = {net: intern(w[k] for k in sorted(w)) for net, w in sorted(rec["weights"].items())}
    out["table"] = table
    return out


def expand(filed: dict) -> dict:
    """``compact`` undone, but for the weights' keys: ``weights[net]`` = the digests in sorted key order."""
    t = filed["table"]
    out = {"cases": {name: {**c, "programs": {p: [t[i] for i in ops] for p, ops in c["programs"].items()}, "marks": [t[i] for i in c["marks"]]}
                     for name, c in filed["cases"].items()}}
    if "weights" in filed:
        out["weights"] = {net: [t[i] for i in w] for net, w in filed["weights"].items()}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--production", action="store_true", help="the benchmark's shapes on the device (programs only, no weight digests)")
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    rec = record(a.production, a.device)
    filed = compact(rec)
    one = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))          # noqa: E731
    with open(a.out, "w") as f:         # one line per case / per net, the table twelve entries to the line
        groups = [json.dumps(g) + ":{\n" + ",\n".join(json.dumps(k) + ":" + one(v) for k, v in filed[g].items()) + "\n}"
                  for g in ("cases", "weights") if g in filed]
        t = filed["table"]
        groups.append('"table":[\n' + ",\n".join(",".join(one(v) for v in t[i:i + 12]) for i in range(0, len(t), 12)) + "\n]")
        f.write("{" + ",\n".join(groups) + "}\n")
    ops = {k: {p: len(v) for p, v in c["programs"].items()} for k, c in rec["cases"].items()}
    print(json.dumps({"cases": len(rec["cases"]), "ops": ops}))


if __name__ == "__main__":
    main()
