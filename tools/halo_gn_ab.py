"""A/B of the GroupNorm-on-A form of the 3x3 convs (LB_GEMM_GN_A, csrc/conv3_halo.hip + conv3_narrow.hip), one process, one GPU.

  shapes    every GroupNorm -> 3x3 conv pair of the B = 17 and B = 2 VAE decode programs at 512^2, launched through lb_gemm_f16 as
            the emitter launches them: (lb_groupnorm_affine_from_stats + the flagged conv reading the raw tensor) against
            (lb_groupnorm_from_stats + the plain conv), alternated REPS times; per side the median and the spread (max - min) of its
            own repeats.  A shape belongs in the policy (HALO_GN_A_MAX_BLOCKS, conv3_halo.hip) only where the gain exceeds 3 x the
            larger spread.  Weights stay warm in the Infinity Cache here, unlike inside a program: the program A/B is the figure
            that counts, this one sets the policy.
  programs  hipGraph replay of the VAE decode (B = 17, B = 2), recorded with lb_conv_halo_set_gn_a 0 (off) and 1 (the policy), both
            programs alive, alternated REPS times; also whether the uint8 frames are bit-identical.  `programs 2` records the "on"
            side with mode 2 (every eligible launch).

Usage: LB_SYNTH_CACHE=/tmp python tools/halo_gn_ab.py shapes   > profiles/halo_gn_ab.txt
       LB_SYNTH_CACHE=/tmp python tools/halo_gn_ab.py programs > profiles/halo_gn_programs.txt"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from latentblending_amd.hip import lib, ops

DEV = "cuda:0"
REPS = 5
# (H = W, Cin, N) of the decoder's GroupNorm -> conv pairs: resnets of the four levels, then conv_norm_out -> conv_out
PAIRS = [(64, 512, 512), (128, 512, 512), (256, 512, 256), (256, 256, 256), (512, 256, 128), (512, 128, 128), (512, 128, 4)]
STREAM = 2.0 ** -4


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


def shapes():
    api = lib.api
    zero = ops.zero_page(DEV)
    print(f"# per-shape A/B, us per (GroupNorm side + conv): median of {REPS} alternated repeats (spread = max - min of the side's own repeats)")
    print("# B  HxW   Cin    N | route  blocks | policy | apply + conv (spread) | table + fused conv (spread) |     gain | 3 x spread | verdict | bits")
    for B in (17, 2):
        for H, Cin, N in PAIRS:
            torch.manual_seed(1)
            x = (torch.randn(B, H, H, Cin, device=DEV) * STREAM).half()
            w = (torch.randn(N, 9 * Cin, device=DEV) * (9 * Cin) ** -0.5).half()
            gamma, beta = 1.0 + 0.1 * torch.randn(Cin, device=DEV), 0.1 * torch.randn(Cin, device=DEV)
            out_f32 = N <= 16
            out = [torch.empty(B * H * H, N, dtype=torch.float32 if out_f32 else torch.float16, device=DEV) for _ in range(2)]
            n = torch.empty_like(x)
            rows = H * H // 64
            v = x.float().reshape(B, rows, 64, Cin)
            st = torch.stack([v.sum(2), (v * v).sum(2)], -1).permute(2, 0, 1, 3).reshape(Cin, B * rows, 2).contiguous()
            del v
            table = torch.empty(B, Cin, 2, dtype=torch.float32, device=DEV)
            ws = torch.empty(int(api.lb_groupnorm_workspace_bytes(B, 32)) // 8, dtype=torch.float64, device=DEV)
            eps = 1e-6 * STREAM * STREAM

            def params(a, o, fused):
                p = lib.LbGemmParams()
                p.A, p.W, p.C = a.data_ptr(), w.data_ptr(), o.data_ptr()
                p.M, p.N, p.K, p.ldw, p.ldc = B * H * H, N, 9 * Cin, 9 * Cin, N
                p.conv, p.Hin, p.Win, p.Hout, p.Wout = 1, H, H, H, H
                p.Cin, p.KH, p.KW, p.stride, p.pad, p.ldx = Cin, 3, 3, 1, 1, Cin
                p.alpha, p.zero_page, p.flags = 1.0, zero.data_ptr(), lib.GEMM_OUT_F32 if out_f32 else 0
                if fused:
                    p.flags |= lib.GEMM_GN_A
                    p.gn_table, p.gn_silu = table.data_ptr(), 1
                return p

            p_plain, p_fused = params(n, out[0], False), params(x, out[1], True)
            tile, nb = C.c_int(), C.c_long()
            api.lb_gemm_plan(C.byref(p_plain), C.byref(tile), None, C.byref(nb))
            fuse, kind = C.c_int(), C.c_int()
            api.lb_conv_halo_set_gn_a(2, 0)
            api.lb_conv_halo_gn_a_plan(C.byref(p_plain), C.byref(fuse), C.byref(kind))
            able = fuse.value
            api.lb_conv_halo_set_gn_a(1, 0)
            api.lb_conv_halo_gn_a_plan(C.byref(p_plain), C.byref(fuse), C.byref(kind))
            head = f"{B:2d} {H:3d}^2 {Cin:5d} {N:4d} | {'halo' if tile.value == 6 else 'narrow' if tile.value == 8 else 'gemm':6s} {nb.value:6d} | {fuse.value:6d} |"
            if not able:
                print(head + "  (no kernel of this route applies the GroupNorm itself: the apply pass stays)", flush=True)
                continue

            def apply_then_conv():
                api.lb_groupnorm_from_stats(x.data_ptr(), n.data_ptr(), gamma.data_ptr(), beta.data_ptr(), st.data_ptr(), ws.data_ptr(),
                                            B, H * H, Cin, Cin, Cin, 32, eps, 1, 0, rows, stream())
                api.lb_gemm_f16(C.byref(p_plain), stream())

            def table_then_fused():
                api.lb_groupnorm_affine_from_stats(st.data_ptr(), gamma.data_ptr(), beta.data_ptr(), table.data_ptr(), B, H * H, Cin, 32,
                                                   eps, rows, stream())
                api.lb_gemm_f16(C.byref(p_fused), stream())

            iters = 5 if B == 17 else 20
            t = {0: [], 1: []}
            for _ in range(REPS):
                t[0].append(1e3 * timed(apply_then_conv, iters))
                t[1].append(1e3 * timed(table_then_fused, iters))
            (m0, s0), (m1, s1) = summary(t[0]), summary(t[1])
            gain, noise = m0 - m1, 3 * max(s0, s1)
            bits = torch.equal(out[0].view(torch.int32 if out_f32 else torch.int16), out[1].view(torch.int32 if out_f32 else torch.int16))
            print(head + f" {m0:12.1f} ({s0:6.1f}) | {m1:18.1f} ({s1:6.1f}) | {gain:+8.1f} | {noise:10.1f} | "
                  f"{'IN ' if gain > noise else 'out'} {100 * gain / m0:+5.1f} % | {'same' if bits else 'DIFFERENT'}", flush=True)
            del x, w, out, n, st, table


def programs(on_mode=1):
    import latentblending_amd.native as N
    api = lib.api
    cdir = os.environ.get("LB_SYNTH_CACHE")
    prov = N.SyntheticProvider(0, cache_file=os.path.join(cdir, "lb_synth_seed0.pt") if cdir else None)
    vae = N.NativeVAEDecoder(N.VAEConfig(), prov, DEV)
    prov.save_cache()
    print(f"# program A/B, ms per hipGraph launch of the VAE decode at 512^2: {REPS} alternated repeats per setting (off = lb_conv_halo_set_gn_a 0, "
          f"on = {on_mode}); a gain counts if it exceeds 3 x the larger spread")
    for B in (17, 2):
        z = torch.randn(B, 4, 64, 64, generator=torch.Generator().manual_seed(3)).half().to(DEV)
        progs, outs = [], []
        for mode in (0, on_mode):
            api.lb_conv_halo_set_gn_a(mode, 0)
            prog = vae.build(B, 64)
            outs.append(prog.decode(z).clone())
            prog.prog.instantiate()
            progs.append(prog)
        api.lb_conv_halo_set_gn_a(1, 0)
        names = [p.prog.op_names() for p in progs]
        runs = {0: [], 1: []}
        for _ in range(REPS):
            for k in (0, 1):
                runs[k].append(timed(progs[k].prog.launch, 3 if B == 17 else 10))
        (moff, soff), (mon, son) = summary(runs[0]), summary(runs[1])
        gain, noise = moff - mon, 3 * max(soff, son)
        print(f"VAE decode B={B:2d}: off {moff:8.3f} ms (spread {soff:.3f}: {' '.join(f'{v:.3f}' for v in runs[0])}) | on {mon:8.3f} ms (spread {son:.3f}: "
              f"{' '.join(f'{v:.3f}' for v in runs[1])}) | gain {gain:+.3f} ms, 3 x spread {noise:.3f}: {'COUNTS' if gain > noise else 'does not count'}"
              f" | frames {'bit-identical' if torch.equal(outs[0], outs[1]) else 'DIFFERENT'} | apply passes {names[0].count('lb_groupnorm_from_stats')} -> "
              f"{names[1].count('lb_groupnorm_from_stats')}, table kernels {names[1].count('lb_groupnorm_affine_from_stats')}", flush=True)
        del progs, outs


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "shapes"
    if what == "shapes":
        shapes()
    else:
        programs(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
