"""LoRA adapters at full SDXL size: wall time of ``load_lora`` / ``set_lora_scale`` / ``unload_lora`` beside the construction of the
pipe, and the device memory a reload holds for a moment (profiles/lora.txt).

    python tools/lora_bench.py [--rank 64]

Synthetic weights and a synthetic adapter over the LCM-LoRA target set (every attention / feed-forward linear, proj_in / proj_out, the
resnets' conv1 / conv2 / conv_shortcut / time_emb_proj, the down- and upsampler convs).  The base provider keeps what it generated
(as a checkpoint read into host memory would be kept), so a reload pays for merging, packing and uploading, not for drawing the
weights again.  One B = 2 UNet step under a hipGraph before and after each call shows that the recorded program keeps working.
"""
import argparse
import os
import socket
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import latentblending_amd.native as N                        # noqa: E402
from latentblending_amd.native import lora as L              # noqa: E402


class Memo:
    """A provider that remembers what its base yielded, by name."""

    def __init__(self, base):
        self.base, self.kept = base, {}

    def _get(self, kind, name, *args):
        if name not in self.kept:
            self.kept[name] = getattr(self.base, kind)(name, *args)
        return self.kept[name]

    def weight(self, name, shape, fan_in=0, gain=1.0):
        return self._get("weight", name, shape, fan_in, gain)

    def bias(self, name, n):
        return self._get("bias", name, n)

    def norm_weight(self, name, n):
        return self._get("norm_weight", name, n)


TARGETS = (".to_q", ".to_k", ".to_v", ".to_out.0", ".ff.net.0.proj", ".ff.net.2", ".proj_in", ".proj_out", ".conv1", ".conv2", ".conv_shortcut",
           ".time_emb_proj", "samplers.0.conv")


def synthetic_adapter(cfg, rank, seed=1):
    """A kohya-named state dict: down ~ N(0, 1 / fan_in), up ~ N(0, 1 / r), alpha = r / 2, fp16 as published files are."""
    g = torch.Generator().manual_seed(seed)
    names = {m: f for f, m in L.unet_tables(cfg)["kohya"].items()}
    state = {}
    for mod, shape in L.unet_modules(cfg).items():
        if not mod.endswith(TARGETS):
            continue
        fan_in = shape[1] * (shape[2] * shape[3] if len(shape) == 4 else 1)
        stem = names[mod]
        state[stem + ".lora_down.weight"] = (torch.randn((rank, shape[1]) + tuple(shape[2:]), generator=g) * fan_in ** -0.5).half()
        state[stem + ".lora_up.weight"] = (torch.randn((shape[0], rank) + ((1, 1) if len(shape) == 4 else ()), generator=g) * rank ** -0.5).half()
        state[stem + ".alpha"] = torch.tensor(rank / 2.0)
    return state


def timed(what, fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    dt = time.time() - t0
    print(f"{what:<34s} {dt:8.2f} s   peak over the resident set {(torch.cuda.max_memory_allocated() - before) / 2 ** 30:6.2f} GiB   "
          f"resident afterwards {torch.cuda.memory_allocated() / 2 ** 30:6.2f} GiB", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=64)
    args = ap.parse_args()
    print(f"host {socket.gethostname()}, device {torch.cuda.get_device_name(0)}, torch {torch.__version__}", flush=True)
    base = Memo(N.SyntheticProvider(0))
    pipe = timed("construct the pipe (UNet, VAE, LPIPS)", lambda: N.NativeSDXLPipe(turbo=True, unet_provider=base, allow_synthetic=True))
    pipe.enable_graphs(True)
    cfg = pipe.unet_cfg
    t0 = time.time()
    adapter = synthetic_adapter(cfg, args.rank)
    print(f"adapter: rank {args.rank}, {len(adapter) // 3} modules, {sum(t.numel() * t.element_size() for t in adapter.values()) / 2 ** 20:.0f} MiB fp16 "
          f"(drawn in {time.time() - t0:.1f} s); UNet weights on the device {pipe.unet_native.weight_bytes() / 2 ** 30:.2f} GiB", flush=True)

    g = torch.Generator().manual_seed(3)
    Ls = cfg.sample_size
    x = torch.randn(2, 4, Ls, Ls, generator=g).half().cuda()
    prog = pipe.unet_program(2, Ls)
    prog.set_conditioning(torch.randn(2, 77, cfg.cross_dim, generator=g).half().cuda(), torch.randn(2, cfg.pooled_dim, generator=g).half().cuda(),
                          torch.tensor([[512.0, 512.0, 0.0, 0.0, 512.0, 512.0]] * 2).cuda())

    def step():
        out = prog.forward(x, torch.full((2,), 499.0)).float().clone()
        torch.cuda.synchronize()
        return out

    def moved(out):
        return float((out - first).norm() / first.norm())
    first = step()
    name = timed("load_lora (scale 1.0)", lambda: pipe.load_lora(adapter, 1.0, name="synthetic"))
    print(f"    same program object: {pipe.unet_program(2, Ls) is prog}; step output moved by rel-L2 {moved(step()):.3e}")
    timed("set_lora_scale (0.5)", lambda: pipe.set_lora_scale(name, 0.5))
    print(f"    step output moved by rel-L2 {moved(step()):.3e}")
    timed("unload_lora", lambda: pipe.unload_lora())
    print(f"    step output equals the first one bit for bit: {torch.equal(step(), first)}")


if __name__ == "__main__":
    main()
