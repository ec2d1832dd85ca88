"""The native TAESDXL encoder, measured per op; written to profiles/tiny_encoder.txt.

For B = 2 at 512 x 512, B = 2 at 1024 x 1024 and B = 17 at 512 x 512, flagged (``c64=True``: the shipped rule) and unflagged
(``c64=False``: the library's own routing everywhere): ``Program.time_ops`` per op (hipEvents between ops, eager replay; median of
5 passes), grouped as conv_in / block convs per level / stride-2 convs / conv_out / layout, and the whole encode as hipGraph
replays.  Beside them, for scale, the same process's B = 2 UNet step at 512 x 512 (``--skip-unet`` leaves it out: it needs the
full-size UNet weights).  No threshold is set on these numbers: the file is the evidence for whether the stride-2 and edge convs
deserve attention later.  ``--parity FILE`` appends the ``tiny_encoder_*`` entries of a parity_metrics.json (the GPU tests' log).

Usage (MI355X): python tools/tiny_encoder_bench.py [--out profiles/tiny_encoder.txt] [--skip-unet] [--parity <parity_metrics.json of the GPU tests' results log>]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import latentblending_amd.native as N  # noqa: E402
from latentblending_amd.native import tiny_vae as TV  # noqa: E402

DEV = "cuda:0"
SHAPES = [(2, 512), (2, 1024), (17, 512)]        # (batch, picture side)


def graph_ms(prog, iters):
    prog.instantiate()
    for _ in range(2):
        prog.launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(iters):
            prog.launch()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / iters)
    med = statistics.median(times)
    return med, (max(times) - min(times)) / med


def op_medians(prog, passes=5):
    prog.time_ops()                                  # warm-up pass
    runs = [prog.time_ops() for _ in range(passes)]
    return [statistics.median(r[i] for r in runs) for i in range(len(runs[0]))]


def encoder_rows(net, B, side, c64, lines):
    prog = net.build(B, side // 8, c64=c64)
    u8 = torch.randint(0, 256, (B, side, side, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(side + B)).to(DEV)
    prog.encode(u8)
    torch.cuda.synchronize()
    names, ms = prog.prog.op_names(), op_medians(prog.prog)
    groups, order = {}, []
    level, convs = side, 0
    for (kind, n), name, t in zip(TV.encoder_layer_plan() + [("layout", -1)],
                                  _per_layer(names), _per_layer(ms)):
        if kind == "down":
            level //= 2
        key = {"in": f"conv_in 3(8) -> 64 @ {level}", "block": f"block convs 64 -> 64 @ {level}", "down": f"stride-2 conv 64 -> 64 -> {level}",
               "out": f"conv_out 64 -> 4 @ {level}", "layout": "lb_nhwc_to_nchw_f16"}[kind]
        if key not in groups:
            groups[key] = [0.0, 0, set()]
            order.append(key)
        groups[key][0] += sum(t)
        groups[key][1] += len(t)
        groups[key][2].update(name)
        convs += len(t) if kind != "layout" else 0
    total = sum(ms)
    g_ms, g_spread = graph_ms(prog.prog, 20 if B * side * side <= 2 * 512 * 512 else 5)
    lines.append(f"   B={B:2d} {side}x{side}  c64={str(c64):5s}: {len(ms)} ops ({convs} convs, {prog.c64_launches} flagged), "
                 f"sum of ops {total:8.3f} ms, hipGraph replay {g_ms:8.3f} ms per encode (spread {g_spread:5.1%})")
    for key in order:
        t, c, kinds = groups[key]
        lines.append(f"      {key:34s} x{c:2d} {t:9.3f} ms  {100 * t / total:5.1f} %   avg {1e3 * t / c:8.1f} us   [{', '.join(sorted(kinds))}]")
    for line in lines[-len(order) - 1:]:
        print(line, flush=True)
    return g_ms


def _per_layer(seq):
    """Split the program's 36 per-op values by layer: 1 (conv_in), then per plan entry 3 (block) or 1, then the layout op."""
    out, i = [], 0
    for kind, _ in TV.encoder_layer_plan():
        n = 3 if kind == "block" else 1
        out.append(list(seq[i:i + n]))
        i += n
    out.append(list(seq[i:]))
    return out


def unet_step(lines):
    import bench
    unet = N.NativeUNet(N.UNetConfig(sample_size=64), bench.device_synthetic_provider(0, DEV), DEV)
    B = 2
    up = unet.build(B, 64)
    g = torch.Generator().manual_seed(0)
    up.set_conditioning(torch.randn(B, 77, 2048, generator=g).half().to(DEV), torch.randn(B, 1280, generator=g).half().to(DEV),
                        torch.tensor([[512.0, 512, 0, 0, 512, 512]] * B, device=DEV))
    up.forward(torch.randn(B, 4, 64, 64, generator=g).half().to(DEV), torch.full((B,), 499.0))
    torch.cuda.synchronize()
    eager = sum(op_medians(up.prog_step, passes=3))
    up.enable_graphs()
    g_ms, g_spread = graph_ms(up.prog_step, 10)
    lines.append(f"   UNet step program B=2 512x512 (SDXL, seeded synthetic weights): {up.prog_step.num_ops} ops, sum of ops {eager:8.3f} ms, "
                 f"hipGraph replay {g_ms:8.3f} ms per step (spread {g_spread:5.1%})")
    print(lines[-1], flush=True)
    return g_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiny_encoder.txt"))
    ap.add_argument("--skip-unet", action="store_true")
    ap.add_argument("--parity", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tiny_encoder_bench needs an MI355X"
    lines = [f"Native TAESDXL encoder ({torch.cuda.get_device_name(0)}; tools/tiny_encoder_bench.py)", "",
             "1. Per op: Program.time_ops (hipEvents between ops, eager replay), median of 5 passes, grouped by layer kind and level; the whole",
             "   encode as hipGraph replays (median of 5 windows).  Seeded synthetic weights; the uint8 -> fp16 staging (one torch elementwise) is",
             f"   outside the program.  c64=True is the shipped rule (LB_GEMM_C64 where the output map has >= {TV.C64_MIN_TILES} tiles), c64=False the",
             "   library's own routing for every conv.  No threshold is set on these numbers.", ""]
    net = N.NativeTinyVAEEncoder(N.TinyVAEConfig(), N.SyntheticProvider(2), DEV)
    whole = {}
    for B, side in SHAPES:
        for c64 in (True, False):
            whole[(B, side, c64)] = encoder_rows(net, B, side, c64, lines)
            torch.cuda.empty_cache()
        lines.append(f"   B={B:2d} {side}x{side}: unflagged / flagged = {whole[(B, side, False)] / whole[(B, side, True)]:.3f}")
        lines.append("")
    if not args.skip_unet:
        lines += ["2. For scale, the same process's UNet step:", ""]
        step = unet_step(lines)
        lines.append(f"   one B=2 512x512 encode (flagged) = {whole[(2, 512, True)] / step:.2f} UNet steps of the same batch")
        lines.append("")
    if args.parity and os.path.isfile(args.parity):
        with open(args.parity) as fh:
            metrics = json.load(fh)
        lines += ["3. Parity of the GPU tests (tests/test_image_anchor_gpu.py): latents rel-L2 against the float64 restatement, bar 1e-2:", ""]
        for k in sorted(metrics):
            if k.startswith("tiny_encoder_B"):
                lines.append(f"   {k:34s} rel_l2 {metrics[k]['rel_l2']:.3e}   (rms of the reference latents {metrics[k]['rms_ref']:.4f})")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"[tiny_encoder_bench] wrote {args.out}")


if __name__ == "__main__":
    main()
