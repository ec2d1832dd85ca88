"""ControlNet, measured at full SDXL width with synthetic weights; the record is profiles/controlnet.txt.

1. The UNet step at 512 x 512, B = 2 and B = 17: the plain program (the program of ever, same process) against the controlled one -
   both networks in one step program -, alternating windows of hipGraph replays between hipEvents.  No bar is fixed: the
   ControlNet's encoder and mid block hold about half of the UNet's transformer layers, so a step of about 1.4 - 1.5x the plain one
   would be no surprise; the per-op split (``time_ops``) says where the time goes.
2. The hint embedding, once, at 512 x 512 and 1024 x 1024 (paid once per control image and render size).
3. A whole cfg-2 transition (bench.py's workload: SDXL-Turbo 512 x 512, 4 steps, 15 branches) with and without a control image.
4. The ControlNet's weight bytes.

With synthetic weights nothing can be said about how well structure is held: this measures cost only.

    python tools/controlnet_bench.py --steps --hint --transition > profiles/controlnet.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
L = 64


def windows_ab(run_a, run_b, iters, windows):
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


def say(lines, text=""):
    lines.append(text)
    print(text, flush=True)


def make_pipe():
    import bench
    import latentblending_amd.native as N
    pipe = N.NativeSDXLPipe(turbo=True, unet_provider=bench.device_synthetic_provider(0, DEV), vae_provider=N.SyntheticProvider(1), device=DEV,
                            allow_synthetic=True)
    pipe.load_controlnet((N.ControlNetConfig.for_unet(pipe.unet_cfg), bench.device_synthetic_provider(3, DEV)))
    return pipe


def hint_picture(size):
    import numpy as np
    rng = np.random.default_rng(0)
    return rng.integers(0, 256, (size, size, 3), dtype=np.uint8)


def split_by_unit(prog):
    """ms per kind of unit of the step program: the ControlNet's encoder, its ten fused adds, the UNet's own units."""
    import torch
    ms = prog.prog_step.time_ops()
    out, at = {"control encoder + mid": 0.0, "control zero convs + adds": 0.0, "unet": 0.0}, 0
    for m in prog.marks:
        if m.program != prog.prog_step.name:
            continue
        t = sum(ms[at:m.op_end])
        at = m.op_end
        key = "control zero convs + adds" if m.kind == "zero" else "control encoder + mid" if m.name.startswith("control.") else "unet"
        out[key] += t
    torch.cuda.synchronize()
    return out


def steps(pipe, lines, windows):
    import torch
    cfg = pipe.unet_cfg
    pipe.set_control_image(hint_picture(8 * L), 1.0)
    net = pipe.controlnet_native
    say(lines, f"4. weights: ControlNet {net.weight_bytes() / 2 ** 30:.2f} GiB packed (fp16 MFMA operands, both LayerNorm forms, fp32 biases and norms); "
               f"UNet {pipe.unet_native.weight_bytes() / 2 ** 30:.2f} GiB")
    say(lines)
    say(lines, "1. UNet step at 512 x 512 (latent 64 x 64), hipGraph replays, alternating windows, median window (spread = (max - min) / median):")
    for B, iters in ((2, 20), (17, 6)):
        progs = []
        for control in (False, True):
            prog = pipe.unet_program(B, L, control=control)
            prog.set_conditioning(torch.randn(B, 77, cfg.cross_dim, device=DEV).half(), torch.randn(B, cfg.pooled_dim, device=DEV).half(),
                                  torch.tensor([[512.0, 512.0, 0.0, 0.0, 512.0, 512.0]] * B, device=DEV))
            prog.forward(torch.randn(B, 4, L, L, device=DEV).half(), torch.full((B,), 499.0))
            prog.enable_graphs()
            progs.append(prog)
        plain, ctl = progs
        ta, tb = windows_ab(plain.prog_step.launch, ctl.prog_step.launch, iters, windows)
        ma, mb = statistics.median(ta), statistics.median(tb)
        say(lines, f"   B = {B:2d}: plain {ma:7.3f} ms ({plain.prog_step.num_ops} ops, spread {(max(ta) - min(ta)) / ma:5.1%})   controlled {mb:7.3f} ms "
                   f"({ctl.prog_step.num_ops} ops, spread {(max(tb) - min(tb)) / mb:5.1%})   controlled / plain = {mb / ma:.3f}")
        sp = split_by_unit(ctl)
        total = sum(sp.values())
        say(lines, "           eager per-op split of the controlled step (time_ops; launch gaps included): "
                   + ", ".join(f"{k} {v:.3f} ms ({v / total:4.0%})" for k, v in sp.items()))
        ca, cb = windows_ab(plain.prog_cond.launch, ctl.prog_cond.launch, 20, windows)
        say(lines, f"           conditioning program: plain {statistics.median(ca):.3f} ms, controlled {statistics.median(cb):.3f} ms (runs when the conditioning changes)")
    pipe.clear_control()
    say(lines)


def hint(pipe, lines, windows):
    from latentblending_amd.native.controlnet import hint_tensor
    say(lines, "2. hint embedding (8 convs at image resolution down to the latent grid; once per control image and render size):")
    for size in (512, 1024):
        prog = pipe._hint_program((size, size))
        prog.embed(hint_tensor(hint_picture(size)))
        prog.enable_graphs()
        ta, _ = windows_ab(prog.prog.launch, prog.prog.launch, 20, windows)
        ms = prog.prog.time_ops()
        say(lines, f"   {size} x {size}: {statistics.median(ta):.3f} ms per embedding; eager per conv (ms): " + " ".join(f"{v:.3f}" for v in ms))
    say(lines)


def transition(pipe, lines, runs):
    import numpy as np
    import torch
    from latentblending_amd import BlendingEngine
    from latentblending_amd.native.frames import materialise_frames
    np.random.seed(0)
    torch.manual_seed(0)
    be = BlendingEngine(pipe, do_compile=True, frontier_width=16, verbose=False)
    be.set_prompt1("photo of underwater landscape, fish, und the sea, incredible detail, high resolution")
    be.set_prompt2("rendering of an alien planet, strange plants, strange creatures, surreal")
    be.set_branching(nmb_max_branches=15)
    picture = hint_picture(512)

    def run(control):
        if control:
            be.set_control_image(picture, 1.0)
        else:
            be.clear_control_image()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        imgs = be.run_transition(fixed_seeds=[420, 421])
        materialise_frames(imgs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, len(imgs)
    for control in (False, True, False, True):      # warm-up: programs recorded, graphs captured
        run(control)
    t = {False: [], True: []}
    frames = {}
    for _ in range(runs):
        for control in (False, True):
            ms, frames[control] = run(control)
            t[control].append(ms)
    say(lines, f"3. cfg-2 transition (SDXL-Turbo 512 x 512, 4 steps, 15 branches: bench.py's workload), host frames materialised, {runs} alternating runs, median:")
    med = {c: statistics.median(t[c]) for c in t}
    for c in (False, True):
        say(lines, f"   {'with a control image' if c else 'without control     '}: {med[c]:8.2f} ms per transition ({frames[c]} frames, {frames[c] / med[c] * 1e3:6.1f} frames/s)   "
                   f"spread {(max(t[c]) - min(t[c])) / med[c]:5.1%}")
    say(lines, f"   controlled / plain = {med[True] / med[False]:.3f}")
    be.clear_control_image()
    say(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--hint", action="store_true")
    ap.add_argument("--transition", action="store_true")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    say(lines, "ControlNet at full SDXL width, synthetic weights (cost only: nothing can be said about how well structure is held)")
    say(lines)
    pipe = make_pipe()
    if a.steps:
        steps(pipe, lines, a.windows)
    if a.hint:
        hint(pipe, lines, a.windows)
    if a.transition:
        transition(pipe, lines, a.runs)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
