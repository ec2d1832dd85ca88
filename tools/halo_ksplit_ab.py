"""A/B of the K-split form of the 3x3 halo-tile conv (LB_GEMM_HALO_KSPLIT, csrc/conv3_halo.hip), one process, one GPU.

  shapes    every split-eligible 3x3 conv shape of the B = 17 / B = 2 UNet step programs and of the B = 17 VAE decode at 512^2: the
            flagged launch under lb_conv_halo_set_ksplit mode 0 (never), 1 (the policy) and 2 (always), alternated REPS times; per
            mode the median and the spread (max - min) of its own repeats.  Weights stay warm in the Infinity Cache here, unlike
            inside a program: the program A/B below is the figure that counts, this one sets the policy's allowance and margin.
  programs  hipGraph replay of the whole UNet step (B = 17, B = 2) and of the VAE decode (B = 17), recorded with the switch off and
            on (the emitter asks the plan when it records), both programs alive, alternated REPS times.

  close     the shapes table for the four shapes whose gain is close to the spread, 15 repeats

Usage: LB_SYNTH_CACHE=/tmp python tools/halo_ksplit_ab.py shapes   > profiles/halo_ksplit_ab.txt
       LB_SYNTH_CACHE=/tmp python tools/halo_ksplit_ab.py programs > profiles/halo_ksplit_programs.txt"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from latentblending_amd.hip import lib, ops

DEV = "cuda:0"
REPS = 5
# (program, B, H = W, Cin, N): the stride-1 3x3 convs that run on the halo-tile kernel
SHAPES = ([("unet17", 17, 16, c, 1280) for c in (640, 1280, 1920, 2560)] + [("unet17", 17, 32, c, 640) for c in (320, 640, 960, 1280, 1920)] +
          [("unet17", 17, 64, c, 320) for c in (320, 640, 960)] + [("unet2", 2, 64, c, 320) for c in (320, 640, 960)] +
          [("vae17", 17, 64, 512, 512), ("vae17", 17, 128, 512, 512), ("vae17", 17, 256, 512, 256), ("vae17", 17, 256, 256, 256),
           ("vae17", 17, 512, 256, 128), ("vae17", 17, 512, 128, 128)])


def stream():
    return torch.cuda.current_stream().cuda_stream


def timed(launch, iters):
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summary(xs):
    return statistics.median(xs), max(xs) - min(xs)


def shapes(reps=REPS, only=None):
    """``only`` = a list of (program, H, Cin) to restrict the table to (more repeats of the close calls)."""
    REPS = reps
    api = lib.api
    zero = ops.zero_page(DEV)
    print(f"# per-shape A/B, us per launch: median of {REPS} alternated repeats (spread = max - min of the mode's own repeats)")
    print("# program B  HxW   Cin    N | items grid | units | policy |   mode 0 (spread) |   mode 1 (spread) |   mode 2 (spread) | gain of 2 | steps unsplit / split")
    for prog, B, H, Cin, N in SHAPES:
        if only is not None and (prog, H, Cin) not in only:
            continue
        torch.manual_seed(1)
        x = torch.randn(B, H, H, Cin, dtype=torch.float16, device=DEV) * 0.5
        w = torch.randn(N, 9 * Cin, dtype=torch.float16, device=DEV) * (9 * Cin) ** -0.5
        out = torch.empty(B * H * H, N, dtype=torch.float16, device=DEV)
        p = lib.LbGemmParams()
        p.A, p.W, p.C = x.data_ptr(), w.data_ptr(), out.data_ptr()
        p.M, p.N, p.K, p.ldw, p.ldc = B * H * H, N, 9 * Cin, 9 * Cin, N
        p.conv, p.Hin, p.Win, p.Hout, p.Wout = 1, H, H, H, H
        p.Cin, p.KH, p.KW, p.stride, p.pad, p.ldx = Cin, 3, 3, 1, 1, Cin
        p.alpha, p.zero_page, p.flags = 1.0, zero.data_ptr(), lib.GEMM_HALO_KSPLIT
        kind, tw, items, grid = C.c_int(), C.c_int(), C.c_long(), C.c_long()
        api.lb_conv_halo_plan(C.byref(p), C.byref(kind), C.byref(tw), C.byref(items), C.byref(grid))
        units, kgrid, split = C.c_long(), C.c_long(), C.c_int()
        api.lb_conv_halo_set_ksplit(1, 0)
        api.lb_conv_halo_ksplit_plan(C.byref(p), C.byref(units), C.byref(kgrid), C.byref(split))
        policy = split.value
        api.lb_conv_halo_set_ksplit(2, 0)
        api.lb_conv_halo_ksplit_plan(C.byref(p), C.byref(units), C.byref(kgrid), C.byref(split))
        ws = torch.zeros(max(int(api.lb_conv_halo_ksplit_workspace_bytes(C.byref(p))), 256), dtype=torch.uint8, device=DEV)
        p.partial = ws.data_ptr()
        iters = 20
        t = {0: [], 1: [], 2: []}
        for _ in range(REPS):
            for mode in (0, 1, 2):
                api.lb_conv_halo_set_ksplit(mode, 0)
                t[mode].append(1e3 * timed(lambda: api.lb_conv3x3_halo_f16(C.byref(p), stream()), iters))
        api.lb_conv_halo_set_ksplit(1, 0)
        (m0, s0), (m1, s1), (m2, s2) = summary(t[0]), summary(t[1]), summary(t[2])
        nch = Cin // 64
        un = -(-items.value // grid.value) * 9 * nch
        sp = -(-units.value // kgrid.value) * 9 if kgrid.value else 0
        print(f"{prog:7s} {B:2d} {H:3d}^2 {Cin:5d} {N:4d} | {items.value:5d} {grid.value:4d} | {units.value:5d} | {policy:6d} | "
              f"{m0:8.1f} ({s0:5.1f}) | {m1:8.1f} ({s1:5.1f}) | {m2:8.1f} ({s2:5.1f}) | {m0 - m2:+8.1f} | {un:4d} / {sp:4d}", flush=True)
        del x, w, out, ws


def programs():
    import latentblending_amd.native as N
    api = lib.api
    cdir = os.environ.get("LB_SYNTH_CACHE")
    prov = N.SyntheticProvider(0, cache_file=os.path.join(cdir, "lb_synth_seed0.pt") if cdir else None)
    unet = N.NativeUNet(N.UNetConfig(), prov, DEV)
    vae = N.NativeVAEDecoder(N.VAEConfig(), prov, DEV)
    prov.save_cache()
    print(f"# program A/B, ms per hipGraph launch: {REPS} alternated repeats per setting; a gain counts if it exceeds 3 x the larger spread")

    def report(name, runs, err):
        (moff, soff), (mon, son) = summary(runs[0]), summary(runs[1])
        gain, noise = moff - mon, 3 * max(soff, son)
        print(f"{name}: off {moff:8.3f} ms (spread {soff:.3f}: {' '.join(f'{v:.3f}' for v in runs[0])}) | on {mon:8.3f} ms (spread {son:.3f}: "
              f"{' '.join(f'{v:.3f}' for v in runs[1])}) | gain {gain:+.3f} ms, 3 x spread {noise:.3f}: {'COUNTS' if gain > noise else 'does not count'}"
              f" | rel-L2 on vs off {err:.2e}", flush=True)

    for B in (17, 2):
        g = torch.Generator().manual_seed(B)
        ctx, te = torch.randn(B, 77, 2048, generator=g).half().to(DEV), torch.randn(B, 1280, generator=g).half().to(DEV)
        ids = torch.tensor([[512.0, 512.0, 0.0, 0.0, 512.0, 512.0]] * B).to(DEV)
        x = torch.randn(B, 4, 64, 64, generator=g).half().to(DEV)
        progs, outs = [], []
        for mode in (0, 1):
            api.lb_conv_halo_set_ksplit(mode, 0)
            prog = unet.build(B, 64)
            prog.set_conditioning(ctx, te, ids)
            outs.append(prog.forward(x, torch.full((B,), 499.0)).float().clone())
            prog.enable_graphs()
            progs.append(prog)
        api.lb_conv_halo_set_ksplit(1, 0)
        runs = {0: [], 1: []}
        for _ in range(REPS):
            for k in (0, 1):
                runs[k].append(timed(progs[k].prog_step.launch, 10 if B == 2 else 5))
        report(f"UNet step B={B:2d}", runs, float((outs[1] - outs[0]).norm() / outs[0].norm()))
        del progs
    B = 17
    z = torch.randn(B, 4, 64, 64, generator=torch.Generator().manual_seed(3)).half().to(DEV)
    progs, outs = [], []
    for mode in (0, 1):
        api.lb_conv_halo_set_ksplit(mode, 0)
        prog = vae.build(B, 64)
        outs.append(prog.decode(z).float().clone())
        prog.prog.instantiate()
        progs.append(prog)
    api.lb_conv_halo_set_ksplit(1, 0)
    runs = {0: [], 1: []}
    for _ in range(REPS):
        for k in (0, 1):
            runs[k].append(timed(progs[k].prog.launch, 3))
    report(f"VAE decode B={B:2d}", runs, float((outs[1] - outs[0]).norm() / (outs[0].norm() + 1e-30)))


if __name__ == "__main__":
    CLOSE = [("unet17", 16, 640), ("unet17", 16, 1280), ("unet17", 64, 320), ("unet2", 64, 320)]
    {"shapes": shapes, "programs": programs, "close": lambda: shapes(15, CLOSE)}[sys.argv[1] if len(sys.argv) > 1 else "shapes"]()
