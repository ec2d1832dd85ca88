"""The tiny decoder (TAESDXL) and its 64 -> 64 conv kernel (LB_GEMM_C64), measured; written to profiles/tiny_vae.txt.

1. Per level shape: the 64 -> 64 conv (bias + ReLU) of every level of a 512 x 512 decode - 64^2, 128^2, 256^2, 512^2 maps, plain
   and with ups = 1 (the stored map is then half the size) - at B = 17 and B = 2: the flagged launch against the SAME problem
   without the bit (the library's own route: the parent's kernels), one process, alternating windows, median of the window means.
   Time, algorithmic TFLOP/s and GB/s (input map + output map + weights, each once), spread = (max - min) / median over the
   windows, and the verdict: the flagged launch WINS a shape when it is faster by more than the larger of the two spreads.  This
   table is where ``native.tiny_vae.C64_MIN_TILES`` comes from.
2. Whole decodes at 512 x 512 (B = 17 and B = 2, hipGraph replays, seeded synthetic weights): the full VAE, the tiny decoder
   with c64 = False and with c64 = True (the shipped rule), interleaved.
3. A cfg-2 transition (bench.py's workload: SDXL-Turbo 512 x 512, 4 steps, 15 branches) with each decoder, alternating.
   ``--skip-transition`` leaves it out (it needs the full-size UNet weights: about a minute of set-up).

Usage (MI355X): python tools/tiny_vae_bench.py [--out profiles/tiny_vae.txt] [--skip-transition]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import latentblending_amd.native as N  # noqa: E402
from latentblending_amd.hip import lib, ops  # noqa: E402
from latentblending_amd.native import tiny_vae as TV  # noqa: E402

DEV = "cuda:0"
LEVELS = [(64, 0), (128, 0), (256, 0), (512, 0), (128, 1), (256, 1), (512, 1)]       # (output side, ups)


def window(launch, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3        # us


def plan_of(x, w, out, flags, ups):
    """(tile code, blocks) lb_gemm_f16 would use."""
    import ctypes as C
    B, H, W, _ = x.shape
    p = lib.LbGemmParams()
    p.conv, p.M, p.N, p.K, p.flags = 1, out.numel() // 64, 64, 576, flags
    p.Hin, p.Win, p.Hout, p.Wout, p.Cin, p.KH, p.KW, p.stride, p.pad, p.ups, p.ldx = H, W, H << ups, W << ups, 64, 3, 3, 1, 1, ups, 64
    p.ldw, p.ldc, p.zero_page = 576, 64, 64
    t, nb = C.c_int(), C.c_long()
    lib.api.lb_gemm_plan(C.byref(p), C.byref(t), None, C.byref(nb))
    return t.value, nb.value


def conv_row(B, side, ups):
    g = torch.Generator().manual_seed(side * 10 + ups + B)
    hin = side >> ups
    x = torch.randn(B, hin, hin, 64, generator=g).half().to(DEV)
    w = (torch.randn(64, 576, generator=g) * 576 ** -0.5).half().to(DEV)
    bias = torch.randn(64, generator=g).to(DEV)
    outs = [torch.empty(B, side, side, 64, dtype=torch.float16, device=DEV) for _ in range(2)]
    conv = dict(KH=3, KW=3, stride=1, pad=1, ups=ups)

    def flagged():
        ops.gemm(x, w, bias=bias, flags=lib.GEMM_C64 | lib.GEMM_RELU, out=outs[0], splitk_ws=False, conv=conv)

    def plain():
        ops.gemm(x, w, bias=bias, flags=lib.GEMM_RELU, out=outs[1], splitk_ws=False, conv=conv)
    for f in (flagged, plain):
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    err = (outs[0].float() - outs[1].float()).abs().max().item() / max(outs[1].float().abs().max().item(), 1e-30)
    iters = max(20, min(2000, int(2e5 / max(1.0, window(plain, 5)))))        # ~0.2 s of work per window
    t = {"c64": [], "plain": []}
    for _ in range(5):                               # alternating windows
        t["c64"].append(window(flagged, iters))
        t["plain"].append(window(plain, iters))
    c, p = statistics.median(t["c64"]), statistics.median(t["plain"])
    sc, sp = (max(t["c64"]) - min(t["c64"])) / c, (max(t["plain"]) - min(t["plain"])) / p
    flops = 2.0 * B * side * side * 64 * 576
    nbytes = 2.0 * (x.numel() + outs[0].numel() + w.numel())
    tile, blocks = plan_of(x, w, outs[1], lib.GEMM_RELU, ups)
    return dict(B=B, side=side, ups=ups, tiles=B * (-(-side // 16)) ** 2, grid=plan_of(x, w, outs[0], lib.GEMM_C64 | lib.GEMM_RELU, ups)[1],
                c64_us=c, plain_us=p, speedup=p / c, wins=p / c > 1.0 + max(sc, sp), spread_c64=sc, spread_plain=sp, plain_tile=tile,
                plain_blocks=blocks, c64_tflops=flops / c / 1e6, plain_tflops=flops / p / 1e6, c64_gbs=nbytes / c / 1e3, plain_gbs=nbytes / p / 1e3,
                max_rel_diff=err)


def timed_ms(launch, iters):
    return window(launch, iters) / 1e3


def decodes(lines):
    full = N.NativeVAEDecoder(N.VAEConfig(), N.SyntheticProvider(1), DEV)
    tiny = N.NativeTinyVAEDecoder(N.TinyVAEConfig(), N.SyntheticProvider(2), DEV)
    for B in (17, 2):
        z = torch.randn(B, 4, 64, 64, generator=torch.Generator().manual_seed(3)).half().to(DEV)
        progs = {"full VAE": full.build(B, 64), "tiny, c64=False": tiny.build(B, 64, c64=False), "tiny, c64=True": tiny.build(B, 64, c64=True)}
        frames = {}
        for name, p in progs.items():
            frames[name] = p.decode(z).clone()
            p.prog.instantiate()
            for _ in range(2):
                p.prog.launch()
        torch.cuda.synchronize()
        iters = 5 if B == 17 else 20
        t = {name: [] for name in progs}
        for _ in range(5):
            for name, p in progs.items():
                t[name].append(timed_ms(p.prog.launch, iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        d = (frames["tiny, c64=True"].int() - frames["tiny, c64=False"].int()).abs()
        for name in progs:
            extra = f"   {progs[name].c64_launches} of 33 convs flagged" if name.startswith("tiny") else ""
            lines.append(f"   B={B:2d} 512x512  {name:16s} {med[name]:8.3f} ms   spread {(max(t[name]) - min(t[name])) / med[name]:5.1%}{extra}")
            print(lines[-1], flush=True)
        lines.append(f"   B={B:2d} ratios: full / tiny(c64=True) = {med['full VAE'] / med['tiny, c64=True']:.2f}   "
                     f"tiny(c64=False) / tiny(c64=True) = {med['tiny, c64=False'] / med['tiny, c64=True']:.3f}   "
                     f"tiny frames, c64 on vs off: max |du8| {int(d.max())}, mean {d.float().mean().item():.4f}")
        print(lines[-1], flush=True)
        del progs
        torch.cuda.empty_cache()


def transition(lines):
    import numpy as np
    import bench
    from latentblending_amd import BlendingEngine
    from latentblending_amd.native.frames import materialise_frames
    np.random.seed(0)
    torch.manual_seed(0)
    pipe = N.NativeSDXLPipe(turbo=True, unet_provider=bench.device_synthetic_provider(0, DEV), vae_provider=N.SyntheticProvider(1), device=DEV,
                            allow_synthetic=True)
    be = BlendingEngine(pipe, do_compile=True, frontier_width=16, verbose=False)
    be.set_prompt1("photo of underwater landscape, fish, und the sea, incredible detail, high resolution")
    be.set_prompt2("rendering of an alien planet, strange plants, strange creatures, surreal")
    be.set_branching(nmb_max_branches=15)
    modes = [("full", True), ("tiny", False), ("tiny", True)]

    def run(dec, c64):
        pipe.decoder, pipe.tiny_conv_c64 = dec, c64
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        imgs = be.run_transition(fixed_seeds=[420, 421])
        materialise_frames(imgs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, len(imgs)
    for dec, c64 in modes:              # warm-up: programs recorded, graphs captured
        run(dec, c64)
        run(dec, c64)
    t = {m: [] for m in modes}
    frames = 0
    for _ in range(4):
        for m in modes:
            # (the c64 switch drops the cached tiny programs: rebuild outside the timed transition)
            pipe.decoder, pipe.tiny_conv_c64 = m
            if m[0] == "tiny":
                run(*m)
            ms, frames = run(*m)
            t[m].append(ms)
    for m in modes:
        med = statistics.median(t[m])
        lines.append(f"   decoder={m[0]:4s} c64={str(m[1]):5s}: {med:8.2f} ms per transition ({frames} frames, {frames / med * 1e3:6.1f} frames/s)   "
                     f"spread {(max(t[m]) - min(t[m])) / med:5.1%}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiny_vae.txt"))
    ap.add_argument("--skip-transition", action="store_true")
    ap.add_argument("--skip-decodes", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tiny_vae_bench needs an MI355X"
    lines = [f"Tiny decoder (TAESDXL) and LB_GEMM_C64 ({torch.cuda.get_device_name(0)}; tools/tiny_vae_bench.py)", "",
             "1. Per level shape: 64 -> 64 3x3 conv, bias + ReLU; flagged (conv3_c64.hip) against the same problem unflagged (the library's own route),",
             "   5 alternating windows of ~0.2 s each, median of the window means; spread = (max - min) / median; TFLOP/s and GB/s are algorithmic",
             "   (2 M N K; input + output + weights once); WINS = unflagged time / flagged time > 1 + the larger spread.", "",
             f"{'B':>2s} {'out map':>9s} {'ups':>3s} {'tiles':>6s} {'grid':>5s} {'c64 us':>9s} {'plain us':>9s} {'speedup':>8s} {'c64 TF/s':>9s} {'plain TF/s':>10s} "
             f"{'c64 GB/s':>9s} {'plain GB/s':>10s} {'spread c/p':>12s} {'plain route':>12s} {'max rel diff':>12s} {'verdict':>8s}"]
    rows = []
    for B in (17, 2):
        for side, ups in LEVELS:
            r = conv_row(B, side, ups)
            rows.append(r)
            lines.append(f"{r['B']:2d} {r['side']:4d}x{r['side']:<4d} {r['ups']:3d} {r['tiles']:6d} {r['grid']:5d} {r['c64_us']:9.1f} {r['plain_us']:9.1f} {r['speedup']:8.2f} "
                         f"{r['c64_tflops']:9.1f} {r['plain_tflops']:10.1f} {r['c64_gbs']:9.0f} {r['plain_gbs']:10.0f} {r['spread_c64']:5.1%}/{r['spread_plain']:5.1%} "
                         f"{'tile ' + str(r['plain_tile']) + ' x' + str(r['plain_blocks']):>12s} {r['max_rel_diff']:12.2e} {'WINS' if r['wins'] else 'no':>8s}")
            print(lines[-1], flush=True)
    wins = [r for r in rows if r["wins"]]
    lose = [r for r in rows if not r["wins"]]
    lines += ["", f"   flagged wins on {len(wins)} of {len(rows)} shapes" + (f"; fewest tiles among the wins: {min(r['tiles'] for r in wins)}" if wins else "")
              + (f"; most tiles among the shapes it does not win: {max(r['tiles'] for r in lose)}" if lose else ""),
              f"   native.tiny_vae.C64_MIN_TILES = {TV.C64_MIN_TILES} (the emitter sets the bit on a conv whose output map has at least that many 16 x 16 tiles)", ""]
    if not args.skip_decodes:
        lines += ["2. Whole decodes, 512 x 512, seeded synthetic weights, hipGraph replays, 5 alternating windows, median:", ""]
        decodes(lines)
        lines.append("")
    if not args.skip_transition:
        lines += ["3. cfg-2 transition (SDXL-Turbo 512 x 512, 4 steps, 15 branches: bench.py's workload), host frames materialised, 4 alternating runs, median:", ""]
        transition(lines)
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"[tiny_vae_bench] wrote {args.out}")


if __name__ == "__main__":
    main()
