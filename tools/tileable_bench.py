"""Wrap-around padding (``tileable``), measured: wrapped against unwrapped launches in ONE process, alternating, per conv route at the
programs' own shapes and for the whole UNet / decoder programs; written to profiles/tileable.txt.

The expectation is no difference: the halo-style kernels gain a few integer operations per TILE (where the halo offsets are set), the
implicit GEMM a conditional add per gathered request on the levels that run there.  No ratio is fixed in advance: a row whose
wrapped median lies outside the run-to-run spread of the unwrapped one is marked, and the text says which.

Method: per case both forms are warmed up, then WINDOWS alternate (unwrapped, wrapped, unwrapped, ...): a window is ``iters``
back-to-back launches between two hipEvents (at least ~20 ms of device work for the single convs), ``windows`` windows per form;
reported: the median window per form in us per launch, the spread (max - min) / median of the unwrapped windows, and wrapped /
unwrapped.  Programs replay as hipGraphs.

    python tools/tileable_bench.py --convs --json out/tile_convs.json
    python tools/tileable_bench.py --programs --json out/tile_programs.json
    python tools/tileable_bench.py --assemble out/tile_convs.json out/tile_programs.json > profiles/tileable.txt
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"

# name -> (B, H, W, Cin, N, ups, flags by name, fp32 output): the programs' own shapes at 512 x 512 renders (latent 64 x 64)
CONVS = {
    "unet 64^2 320->320 (halo)": (17, 64, 64, 320, 320, 0, (), False),
    "unet 32^2 640->640 (halo, K-split)": (17, 32, 32, 640, 640, 0, ("ksplit",), False),
    "unet 16^2 1280->1280 (halo, K-split)": (17, 16, 16, 1280, 1280, 0, ("ksplit",), False),
    "unet 16^2 1280->1280 B=2 (implicit GEMM)": (2, 16, 16, 1280, 1280, 0, (), False),
    "unet conv_out 64^2 320->4 (narrow)": (17, 64, 64, 320, 4, 0, (), False),
    "vae 128^2 512->512 (halo)": (17, 128, 128, 512, 512, 0, (), False),
    "vae 256^2 256->256 (halo)": (17, 256, 256, 256, 256, 0, (), False),
    "vae 512^2 128->128 (halo)": (17, 512, 512, 128, 128, 0, (), False),
    "vae conv_out 512^2 128->4 fp32 (narrow)": (17, 512, 512, 128, 4, 0, (), True),
    "taesdxl 512^2 64->64 (64-channel kernel)": (17, 512, 512, 64, 64, 0, ("c64", "relu"), False),
    "taesdxl 256^2 -> 512^2 64->64 ups (64-channel kernel)": (17, 256, 256, 64, 64, 1, ("c64",), False),
}
ROUTES = ["implicit GEMM", "64-channel kernel", "halo upconv", "narrow", "halo 3x3"]


def windows_ab(run_a, run_b, iters, windows):
    """Alternating windows of two launch closures -> (list of ms per window of a, of b)."""
    import torch
    for f in (run_a, run_b):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(windows):
        for f, acc in ((run_a, ta), (run_b, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1) / iters)
    return ta, tb


def row(name, ta, tb, extra=None):
    ma, mb = statistics.median(ta), statistics.median(tb)
    r = {"name": name, "unwrapped_us": ma * 1e3, "wrapped_us": mb * 1e3, "spread_unwrapped": (max(ta) - min(ta)) / ma,
         "spread_wrapped": (max(tb) - min(tb)) / mb, "ratio": mb / ma}
    r.update(extra or {})
    print(json.dumps(r), flush=True)
    return r


def measure_convs(windows):
    import torch
    from latentblending_amd.hip import lib, ops
    out = []
    stream = torch.cuda.current_stream().cuda_stream
    flagbits = {"ksplit": lib.GEMM_HALO_KSPLIT, "c64": lib.GEMM_C64, "relu": lib.GEMM_RELU}
    for name, (B, H, W, cin, n, ups, fl, f32) in CONVS.items():
        x = (torch.randn(B, H, W, cin, device=DEV) * 0.5).half()
        w = (torch.randn(n, 9 * cin, device=DEV) * (9 * cin) ** -0.5).half()
        bias = torch.randn(n, device=DEV)
        flags = sum(flagbits[f] for f in fl) | (lib.GEMM_OUT_F32 if f32 else 0)
        blocks, keep = [], []
        for wrap in (0, 3):
            g = lib.ConvGeom.conv3x3(H, W, cin, ups=ups, wrap=wrap)
            o = torch.empty(g.M(B), n, dtype=torch.float32 if f32 else torch.float16, device=DEV)
            p = lib.gemm_params(A=x.data_ptr(), W=w.data_ptr(), C=o.data_ptr(), M=g.M(B), N=n, K=g.K, ldw=9 * cin, ldc=n, conv=g,
                                bias=bias.data_ptr(), flags=flags, zero_page=ops.zero_page(DEV).data_ptr())
            pl = lib.conv_plan(p)
            if "ksplit" in fl:
                if pl.route == lib.ROUTE_HALO3 and pl.ksplit_split:
                    ws = torch.zeros(pl.ksplit_counter_bytes + pl.ksplit_slab_bytes, dtype=torch.uint8, device=DEV)
                    p.partial = ws.data_ptr()
                    keep.append(ws)
                else:
                    p.flags &= ~lib.GEMM_HALO_KSPLIT
                pl = lib.conv_plan(p)
            blocks.append((p, pl))
            keep.append(o)
        (p0, pl0), (p1, pl1) = blocks
        assert (pl0.route, pl0.tile, pl0.splitk, pl0.ksplit_split) == (pl1.route, pl1.tile, pl1.splitk, pl1.ksplit_split), name
        flops = 2.0 * p0.M * n * 9 * cin
        iters = max(3, min(200, int(20e-3 / max(flops / 400e12, 5e-6))))
        ta, tb = windows_ab(lambda: lib.api.lb_gemm_f16(C.byref(p0), stream), lambda: lib.api.lb_gemm_f16(C.byref(p1), stream), iters, windows)
        out.append(row(name, ta, tb, {"route": ROUTES[pl0.route], "tile": pl0.tile, "ksplit": pl0.ksplit_split, "iters": iters}))
        del keep
    return out


def measure_programs(windows):
    import torch
    import latentblending_amd.native as n
    out = []
    pipe = n.NativeSDXLPipe(turbo=True, allow_synthetic=True)
    L = 64

    def pair(build, feed):
        progs = []
        for wrap in (0, 3):
            prog = build(wrap)
            feed(prog)
            prog.enable_graphs()
            progs.append(prog)
        return progs

    for B in (17, 2):
        def feed(prog, B=B):
            cfg = pipe.unet_cfg
            prog.set_conditioning(torch.randn(B, 77, cfg.cross_dim, device=DEV).half(), torch.randn(B, cfg.pooled_dim, device=DEV).half(),
                                  torch.tensor([[512.0, 512.0, 0.0, 0.0, 512.0, 512.0]] * B, device=DEV))
            prog.forward(torch.randn(B, 4, L, L, device=DEV).half(), torch.full((B,), 499.0))
        a, b = pair(lambda wrap, B=B: pipe.unet_native.build(B, L, wrap=wrap), feed)
        ta, tb = windows_ab(a.prog_step.launch, b.prog_step.launch, 10 if B == 17 else 30, windows)
        out.append(row(f"UNet step B={B} 512^2", ta, tb))
        del a, b
        torch.cuda.empty_cache()
    z = torch.randn(17, 4, L, L, device=DEV).half()
    a, b = pair(lambda wrap: pipe.vae_native.build(17, L, wrap=wrap), lambda prog: prog.decode(z))
    ta, tb = windows_ab(a.prog.launch, b.prog.launch, 5, windows)
    out.append(row("VAE decode B=17 512^2", ta, tb))
    del a, b
    torch.cuda.empty_cache()
    a, b = pair(lambda wrap: pipe._tiny_net().build(17, L, wrap=wrap), lambda prog: prog.decode(z))
    ta, tb = windows_ab(a.prog.launch, b.prog.launch, 20, windows)
    out.append(row("tiny (TAESDXL) decode B=17 512^2", ta, tb))
    return out


def assemble(paths):
    rows = []
    for p in paths:
        with open(p) as fh:
            rows += json.load(fh)
    print(f"{'case':58s} {'route':18s} {'unwrapped us':>13s} {'wrapped us':>11s} {'w / u':>7s} {'spread u':>9s} {'spread w':>9s}  outside the spread")
    for r in rows:
        outside = abs(r["ratio"] - 1.0) > max(r["spread_unwrapped"], r["spread_wrapped"])
        print(f"{r['name']:58s} {r.get('route', 'program'):18s} {r['unwrapped_us']:13.1f} {r['wrapped_us']:11.1f} {r['ratio']:7.4f} "
              f"{r['spread_unwrapped']:9.4f} {r['spread_wrapped']:9.4f}  {'YES' if outside else 'no'}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--convs", action="store_true")
    ap.add_argument("--programs", action="store_true")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--assemble", nargs="*", default=None)
    a = ap.parse_args()
    if a.assemble is not None:
        return assemble(a.assemble)
    rows = []
    if a.convs:
        rows += measure_convs(a.windows)
    if a.programs:
        rows += measure_programs(a.windows)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
