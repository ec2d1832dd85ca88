"""The native SDXL VAE encoder, measured; written to profiles/vae_encoder.txt.

Per picture size (512 x 512, 1024 x 1024, 1344 x 768) and B = 1, 2: the whole encode as hipGraph replays, for the full encoder
(``native/vae.py``, scaled fp16 stream: the shipped default) and the TAESDXL encoder; for the full encoder at B = 2 the per-op split
from ``Program.time_ops`` (hipEvents between ops, eager replay; median of 5 passes) summed per unit kind, with the share of the three
stride-2 convs and of conv_in stated.  ``--unet``: one B = 2 UNet step at 512 x 512 from the same process, as the yardstick (needs the
full-size UNet weights).  No threshold is set on these numbers: the file is the evidence for whether the stride-2 convs deserve a
kernel of their own later.

A measurement run handles the sizes it is given and writes its numbers to a JSON file; ``--assemble`` reads such files and the GPU
tests' parity log and writes the text - so every size can run as a step of its own, under its own time limit:

    python tools/vae_encoder_bench.py --sizes 512x512 --unet --json out/enc_512.json
    python tools/vae_encoder_bench.py --sizes 1024x1024 --json out/enc_1024.json
    python tools/vae_encoder_bench.py --sizes 1344x768 --json out/enc_1344.json
    python tools/vae_encoder_bench.py --assemble out/enc_512.json out/enc_1024.json out/enc_1344.json [--parity parity_metrics.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
KINDS = ["conv_in", "resnet", "downsample", "mid_attention", "out", "tail"]
KIND_TEXT = {"conv_in": "conv_in 3(8) -> 128", "resnet": "resnets (14)", "downsample": "stride-2 convs (3)", "mid_attention": "mid attention",
             "out": "norm_out + moments conv", "tail": "cast + layout"}


def graph_ms(prog, iters):
    import torch
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


def measure_size(W, H, full, tiny):
    """{"full": {B: ms}, "tiny": {B: ms}, "split": per-kind ms of the full encoder at B = 2, "ops": ...} for W x H pictures."""
    import torch
    out = {"size": f"{W}x{H}", "full": {}, "tiny": {}, "spread": {}}
    for B in (1, 2):
        u8 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(W + B)).to(DEV)
        for name, net in (("full", full), ("tiny", tiny)):
            prog = net.build(B, (H // 8, W // 8))
            prog.encode(u8)
            torch.cuda.synchronize()
            if name == "full" and B == 2:
                ms, names = op_medians(prog.prog), prog.prog.op_names()
                split, at = {k: 0.0 for k in KINDS}, 0
                for m in prog.marks:
                    split[m.kind] += sum(ms[at:m.op_end])
                    at = m.op_end
                split["tail"] = sum(ms[at:])
                routes = {}
                for n, t in zip(names, ms):
                    routes[n] = routes.get(n, 0.0) + t
                out["split"], out["sum_of_ops"], out["num_ops"], out["by_launcher"] = split, sum(ms), len(ms), routes
            g, spread = graph_ms(prog.prog, 20 if B * H * W <= 2 * 512 * 512 else 5)
            out[name][str(B)], out["spread"][f"{name}{B}"] = g, spread
            print(f"[vae_encoder_bench] {W}x{H} B={B} {name}: {g:.3f} ms per encode (spread {spread:.1%})", flush=True)
            del prog
            torch.cuda.empty_cache()
    return out


def unet_step():
    import torch
    import bench
    import latentblending_amd.native as N
    unet = N.NativeUNet(N.UNetConfig(sample_size=64), bench.device_synthetic_provider(0, DEV), DEV)
    B = 2
    up = unet.build(B, 64)
    g = torch.Generator().manual_seed(0)
    up.set_conditioning(torch.randn(B, 77, 2048, generator=g).half().to(DEV), torch.randn(B, 1280, generator=g).half().to(DEV),
                        torch.tensor([[512.0, 512, 0, 0, 512, 512]] * B, device=DEV))
    up.forward(torch.randn(B, 4, 64, 64, generator=g).half().to(DEV), torch.full((B,), 499.0))
    torch.cuda.synchronize()
    up.enable_graphs()
    g_ms, spread = graph_ms(up.prog_step, 10)
    print(f"[vae_encoder_bench] UNet step B=2 512x512: {g_ms:.3f} ms (spread {spread:.1%})", flush=True)
    return {"ms": g_ms, "spread": spread, "num_ops": up.prog_step.num_ops}


def measure(args):
    import torch
    import latentblending_amd.native as N
    assert torch.cuda.is_available(), "vae_encoder_bench needs an MI355X"
    full = N.NativeVAEEncoder(N.VAEConfig(), N.SyntheticProvider(1), DEV)
    tiny = N.NativeTinyVAEEncoder(N.TinyVAEConfig(), N.SyntheticProvider(2), DEV)
    res = {"device": torch.cuda.get_device_name(0), "sizes": []}
    for size in args.sizes:
        W, H = (int(v) for v in size.lower().split("x"))
        res["sizes"].append(measure_size(W, H, full, tiny))
    if args.unet:
        del full, tiny
        torch.cuda.empty_cache()
        res["unet"] = unet_step()
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"[vae_encoder_bench] wrote {args.json}")


def assemble(args):
    parts = []
    for fp in args.assemble:
        with open(fp) as fh:
            parts.append(json.load(fh))
    sizes = [s for p in parts for s in p["sizes"]]
    unet = next((p["unet"] for p in parts if "unet" in p), None)
    lines = [f"Native SDXL VAE encoder ({parts[0]['device']}; tools/vae_encoder_bench.py)", "",
             "1. The whole encode as hipGraph replays (median of 5 windows), ms per encode.  Seeded synthetic weights; the uint8 -> fp16",
             "   staging (one torch elementwise) is outside the programs.  full = AutoencoderKL encoder (scaled fp16 stream), tiny = TAESDXL.", "",
             "   size         B   full ms   tiny ms   full / tiny"]
    for s in sizes:
        for B in ("1", "2"):
            lines.append(f"   {s['size']:10s} {B:>3s} {s['full'][B]:9.3f} {s['tiny'][B]:9.3f} {s['full'][B] / s['tiny'][B]:10.1f}"
                         f"   (spread {s['spread']['full' + B]:.1%} / {s['spread']['tiny' + B]:.1%})")
    if unet is not None:
        lines += ["", f"   For scale, the same process's UNet step program (SDXL, B = 2, 512 x 512, {unet['num_ops']} ops): {unet['ms']:.3f} ms "
                      f"(spread {unet['spread']:.1%})."]
        for s in sizes:
            lines.append(f"   one B = 2 {s['size']} full encode = {s['full']['2'] / unet['ms']:.2f} such UNet steps")
    lines += ["", "2. Per-op split of the full encoder at B = 2: Program.time_ops (hipEvents between ops, eager replay), median of 5 passes,",
              "   summed per unit kind; the share is of the sum of ops.", ""]
    for s in sizes:
        if "split" not in s:
            continue
        tot = s["sum_of_ops"]
        lines.append(f"   {s['size']}: {s['num_ops']} ops, sum of ops {tot:.3f} ms")
        for k in KINDS:
            lines.append(f"      {KIND_TEXT[k]:28s} {s['split'][k]:9.3f} ms  {100 * s['split'][k] / tot:5.1f} %")
        lines.append("      by launcher: " + ", ".join(f"{n} {t:.3f}" for n, t in sorted(s["by_launcher"].items(), key=lambda kv: -kv[1])))
        lines.append(f"      => the three stride-2 convs are {100 * s['split']['downsample'] / tot:.1f} % and conv_in is "
                     f"{100 * s['split']['conv_in'] / tot:.1f} % of this encode")
        lines.append("")
    if args.parity and os.path.isfile(args.parity):
        with open(args.parity) as fh:
            metrics = json.load(fh)
        units = {k: v for k, v in metrics.items() if k.startswith("vae_encoder_units/") and "ratio_l2" in v}
        if units:
            lines += ["3. Error ratios of the GPU tests (tests/test_vae_encoder_gpu.py): native error / storage-model error against float64, per unit,",
                      "   teacher-forced; the bar is 4.  case/unit: ratio of rel-L2, ratio of max-abs (native rel-L2).", ""]
            for k in sorted(units):
                v = units[k]
                lines.append(f"   {k[len('vae_encoder_units/'):]:72s} {v['ratio_l2']:5.2f} {v['ratio_max']:5.2f}   ({v['e_native_l2']:.2e})")
            lines.append("")
        free = {k: v for k, v in metrics.items() if k.startswith("vae_encoder_units/") and k.endswith("free_running_rel_l2")}
        for k in sorted(free):
            lines.append(f"   {k[len('vae_encoder_units/'):]}: " + " ".join(f"{t}={e:.2e}" for t, e in free[k].items()))
        for k in ("vae_encoder_full_width_B2_64", "vae_encoder_pipe_rel_l2"):
            if k in metrics:
                lines.append(f"   {k}: {metrics[k]}")
        worst = max((v["worst_err_over_bound"] for k, v in metrics.items() if k.startswith("vae_enc_edge_") and isinstance(v, dict)), default=None)
        if worst is not None:
            lines.append(f"   far-edge gather (lb_gemm_f16 on ConvGeom.down3x3, every forced tile): worst err / bound {worst:.3f}")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"[vae_encoder_bench] wrote {args.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["512x512", "1024x1024", "1344x768"], help="picture sizes, width x height")
    ap.add_argument("--unet", action="store_true", help="also time one B = 2 UNet step at 512 x 512 in this process")
    ap.add_argument("--json", default=os.path.join(ROOT, "build", "vae_encoder_bench.json"))
    ap.add_argument("--assemble", nargs="+", default=None, help="JSON files of measurement runs -> the text file (no device needed)")
    ap.add_argument("--parity", default=None, help="parity_metrics.json of the GPU tests' results log")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_encoder.txt"))
    args = ap.parse_args()
    if args.assemble:
        assemble(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
