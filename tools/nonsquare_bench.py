"""Non-square renders: what the ragged-tile form of the 3x3 halo conv (LB_GEMM_HALO_RAGGED) buys, written to profiles/nonsquare.txt.

1. Per-conv table: every UNet level of the 1344x768, 1024x576 and 768x448 renders (none divides into halo tiles), the level's
   resnet conv (Cin = Cout = level width, bias + residual) as a ragged halo launch against the implicit GEMM lb_gemm_f16 gives the
   same conv without the flag - alternating windows, median of the per-window means, same operands, outputs compared.  This table
   is where ``native.geometry.HALO_RAGGED_MIN_FILL`` comes from.
2. Programs: the full SDXL UNet step and VAE decode at 768x448 (Turbo, B = 17) and 1344x768 (base, B = 2), hipGraph replays with
   ``ragged_halo`` on and off (seeded synthetic weights).
3. ``--bench-lines FILE...``: result lines of bench.py (this commit and its parent, same box, alternating) quoted at the end.

Usage (MI355X): LB_SYNTH_CACHE=/tmp python tools/nonsquare_bench.py [--out profiles/nonsquare.txt] [--skip-programs] [--bench-lines a.json b.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import latentblending_amd.native as N  # noqa: E402
from latentblending_amd.hip import lib, ops  # noqa: E402
from latentblending_amd.native import geometry as G  # noqa: E402

DEV = "cuda:0"
RENDERS = [("1344x768", 2, (96, 168)), ("1024x576", 2, (72, 128)), ("768x448", 17, (56, 96))]      # (render, batch, latent (H, W))
LEVEL_CHANNELS = (320, 640, 1280)


def window(launch, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3        # us


def routed_to_halo(B, H, W, Cc):
    """lb_gemm_f16's own routing of the flagged conv (default mode: halo only when its grid has >= 96 blocks)."""
    p = lib.LbGemmParams()
    p.conv, p.M, p.N, p.K, p.flags = 1, B * H * W, Cc, 9 * Cc, lib.GEMM_HALO_RAGGED
    p.Hin, p.Win, p.Hout, p.Wout, p.Cin, p.KH, p.KW, p.stride, p.pad, p.ldx = H, W, H, W, Cc, 3, 3, 1, 1, Cc
    p.ldw, p.ldc, p.zero_page = 9 * Cc, Cc, 64
    t = C.c_int()
    lib.api.lb_gemm_plan(C.byref(p), C.byref(t), None, None)
    return t.value == 6


def conv_row(render, B, H, W, C):
    g = torch.Generator().manual_seed(H * 1000 + W + C)
    x = torch.randn(B, H, W, C, generator=g).half().to(DEV)
    w = (torch.randn(C, 9 * C, generator=g) * (9 * C) ** -0.5).half().to(DEV)
    bias, res = torch.randn(C, generator=g).to(DEV), torch.randn(B, H, W, C, generator=g).half().to(DEV)
    outs = [torch.empty(B, H, W, C, dtype=torch.float16, device=DEV) for _ in range(2)]
    ws = torch.empty(lib.api.lb_gemm_workspace_bytes(B * H * W, C) // 4, dtype=torch.float32, device=DEV)
    kind, tw, items, grid = ops.conv_halo_plan(B, H, W, C, C, flags=lib.GEMM_HALO_RAGGED)
    assert kind == 3
    if ops.conv_halo_plan(B, H, W, C, C)[0] == 3:       # the level divides into tiles: the shipped kernel takes it, nothing ragged to measure
        return None
    conv = dict(KH=3, KW=3, stride=1, pad=1)

    def ragged():
        ops.gemm(x, w, bias=bias, residual=res, flags=lib.GEMM_HALO_RAGGED, out=outs[0], splitk_ws=False, conv=dict(conv, halo=True))

    def igemm():
        ops.gemm(x, w, bias=bias, residual=res, out=outs[1], workspace=ws, conv=conv)
    for f in (ragged, igemm):
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    err = (outs[0].float() - outs[1].float()).abs().max().item() / outs[1].float().abs().max().item()
    iters = max(20, min(400, int(2e5 / max(1.0, window(igemm, 5)))))        # ~0.2 s of work per window
    t = {"ragged": [], "igemm": []}
    for _ in range(5):                               # alternating windows
        t["ragged"].append(window(ragged, iters))
        t["igemm"].append(window(igemm, iters))
    r, i = statistics.median(t["ragged"]), statistics.median(t["igemm"])
    flops = 2.0 * B * H * W * C * 9 * C
    return dict(render=render, B=B, H=H, W=W, C=C, tile=f"{tw}x{256 // tw}", items=items, grid=grid, fill=G.halo_ragged_fill(H, W, tw),
                ragged_us=r, igemm_us=i, speedup=i / r, routed=routed_to_halo(B, H, W, C), ragged_tflops=flops / r / 1e6, spread_ragged=(max(t["ragged"]) - min(t["ragged"])) / r,
                spread_igemm=(max(t["igemm"]) - min(t["igemm"])) / i, max_rel_diff=err)


def timed_program(launch, iters):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    return statistics.median(window(launch, iters) for _ in range(5)) / 1e3       # ms


def programs(lines):
    cdir = os.environ.get("LB_SYNTH_CACHE")
    cfile = (lambda s: os.path.join(cdir, f"lb_synth_seed{s}.pt")) if cdir else (lambda s: None)
    cases = [("768x448 Turbo", 17, (56, 96)), ("1344x768 base", 2, (96, 168))]
    vprov = N.SyntheticProvider(1, cache_file=cfile(1))
    vae = N.NativeVAEDecoder(N.VAEConfig(), vprov, DEV)
    vprov.save_cache()
    for name, B, (H, W) in cases:
        z = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(3)).half().to(DEV)
        res = {}
        for flag in (True, False):
            prog = vae.build(B, (H, W), ragged_halo=flag)
            out = prog.decode(z).clone()
            prog.prog.instantiate()
            names = prog.prog.op_names()
            res[flag] = (timed_program(prog.prog.launch, 5), names.count("lb_conv3x3_halo_f16"), names.count("lb_gemm_f16"), out)
            del prog
        d = (res[True][3].int() - res[False][3].int()).abs()
        lines.append(f"VAE decode  {name:14s} B={B:2d} latent {H}x{W}: ragged_halo on {res[True][0]:8.3f} ms ({res[True][1]} halo convs / {res[True][2]} GEMMs)"
                     f"   off {res[False][0]:8.3f} ms ({res[False][1]} / {res[False][2]})   on/off = {res[True][0] / res[False][0]:.3f}"
                     f"   frames: max |du8| {int(d.max())}, mean {d.float().mean().item():.4f}")
        print(lines[-1], flush=True)
    del vae
    torch.cuda.empty_cache()
    uprov = N.SyntheticProvider(0, cache_file=cfile(0))
    net = N.NativeUNet(N.UNetConfig(), uprov, DEV)
    uprov.save_cache()
    for name, B, (H, W) in cases:
        g = torch.Generator().manual_seed(B)
        ctx, te = torch.randn(B, 77, 2048, generator=g).half().to(DEV), torch.randn(B, 1280, generator=g).half().to(DEV)
        ids = torch.tensor([[512.0, 512.0, 0.0, 0.0, 512.0, 512.0]] * B).to(DEV)
        x = torch.randn(B, 4, H, W, generator=g).half().to(DEV)
        res = {}
        for flag in (True, False):
            prog = net.build(B, (H, W), ragged_halo=flag)
            prog.set_conditioning(ctx, te, ids)
            out = prog.forward(x, torch.full((B,), 499.0)).clone()
            prog.enable_graphs()
            names = prog.prog_step.op_names()
            res[flag] = (timed_program(prog.prog_step.launch, 10 if B == 2 else 5), names.count("lb_conv3x3_halo_f16"), names.count("lb_gemm_f16"), out)
            del prog
        rel = ((res[True][3].float() - res[False][3].float()).norm() / res[False][3].float().norm()).item()
        lines.append(f"UNet step   {name:14s} B={B:2d} latent {H}x{W}: ragged_halo on {res[True][0]:8.3f} ms ({res[True][1]} halo convs / {res[True][2]} GEMMs)"
                     f"   off {res[False][0]:8.3f} ms ({res[False][1]} / {res[False][2]})   on/off = {res[True][0] / res[False][0]:.3f}"
                     f"   eps rel-L2 on vs off {rel:.2e}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nonsquare.txt"))
    ap.add_argument("--skip-programs", action="store_true")
    ap.add_argument("--bench-lines", nargs="*", default=[], help="files holding bench.py result lines, quoted at the end (label = file name)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "nonsquare_bench needs an MI355X"
    lines = [f"Non-square renders: ragged halo-conv tiles against the implicit GEMM ({torch.cuda.get_device_name(0)}; tools/nonsquare_bench.py)", "",
             "1. Per-conv: the resnet conv of every UNet level (Cin = Cout, bias + fp16 residual), 5 alternating windows of ~0.2 s each, median of the window means;",
             "   spread = (max - min) / median over the windows; fill = valid pixels / tile pixels; speedup = implicit GEMM time / ragged halo time;",
             "   route = where lb_gemm_f16 sends the flagged conv in a program (the halo kernel only when its grid has >= 96 blocks, LB_HALO_MIN_BLOCKS).", "",
             f"{'render':9s} {'B':>2s} {'level HxW':>9s} {'C':>5s} {'tile':>5s} {'items':>6s} {'grid':>5s} {'fill':>6s} {'ragged us':>10s} {'igemm us':>10s} {'speedup':>8s} "
             f"{'TFLOP/s':>8s} {'spread r/i':>12s} {'max rel diff':>12s} {'route':>6s}"]
    rows = []
    for render, B, (H, W) in RENDERS:
        for lvl, C in enumerate(LEVEL_CHANNELS):
            r = conv_row(render, B, H >> lvl, W >> lvl, C)
            if r is None:
                lines.append(f"{render:9s} {B:2d} {H >> lvl:4d}x{W >> lvl:<4d} {C:5d}   divides into halo tiles: the shipped kernel runs it, with or without the flag")
                continue
            rows.append(r)
            lines.append(f"{r['render']:9s} {r['B']:2d} {r['H']:4d}x{r['W']:<4d} {r['C']:5d} {r['tile']:>5s} {r['items']:6d} {r['grid']:5d} {r['fill']:6.3f} {r['ragged_us']:10.1f} "
                         f"{r['igemm_us']:10.1f} {r['speedup']:8.2f} {r['ragged_tflops']:8.1f} {r['spread_ragged']:5.1%}/{r['spread_igemm']:5.1%} {r['max_rel_diff']:12.2e} {'halo' if r['routed'] else 'gemm':>6s}")
            print(lines[-1], flush=True)
    losers = [r for r in rows if r["speedup"] < 1.0]
    lines += ["", f"   ragged wins on {len(rows) - len(losers)} of {len(rows)} shapes; lowest fill measured {min(r['fill'] for r in rows):.3f}"
              + ("" if not losers else "; loses at " + ", ".join(f"{r['H']}x{r['W']} C{r['C']} (fill {r['fill']:.3f}, {r['items']} blocks, routed to the "
                                                                   f"{'halo kernel' if r['routed'] else 'implicit GEMM'})" for r in losers)),
              f"   losses among the shapes the router sends to the halo kernel: {sum(1 for r in losers if r['routed'])}",
              f"   native.geometry.HALO_RAGGED_MIN_FILL = {G.HALO_RAGGED_MIN_FILL}", ""]
    if not args.skip_programs:
        lines += ["2. Programs (full SDXL widths, seeded synthetic weights, hipGraph replays, median of 5 windows):", ""]
        programs(lines)
        lines.append("")
    if args.bench_lines:
        lines += ["3. bench.py --gpus 1 (headline: the square 512x512 workload), this commit beside its parent, same box, alternating:", ""]
        for path in args.bench_lines:
            for ln in open(path):
                ln = ln.strip()
                if not ln.startswith("{"):
                    continue
                try:
                    rec = json.loads(ln)
                except ValueError:
                    continue
                keep = {k: rec[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup") if k in rec}
                lines.append(f"   {os.path.basename(path):28s} {json.dumps(keep or {k: v for k, v in rec.items() if not isinstance(v, (dict, list))})}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"[nonsquare_bench] wrote {args.out}")


if __name__ == "__main__":
    main()
