"""What the second-order sampler costs and buys on one MI355X (the figures of profiles/dpmpp.txt).

  python tools/sampler_bench.py --part kernel
      the DPM-Solver++ 2M step kernel (lb_dpmpp2m_step_f16) on a 1 GiB batch of latents, timed beside the plain DDIM step
      (lb_ddim_step_f16) and the latent-consistency step (lb_lcm_step_f16) in the same process: us per launch and GB/s over
      the algorithmic bytes (HIP events around ``--iters`` back-to-back launches, after a warm-up).
  python tools/sampler_bench.py --part transition --samplers euler:30,dpmpp_2m_karras:20
      one base-SDXL transition at full width (synthetic weights, 1024^2, guidance 4.0 with CFG, depth_strength 0.5, 15 branches:
      the cfg-3 branching of bench.py) under each ``sampler:steps`` pair: seconds and frames/s of the second run, UNet samples.
      ``euler:30`` alone also runs on a commit that has no second-order sampler (the comparison run on the parent).
One JSON line per measurement on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_launches(fn, iters: int, warmup: int = 3) -> float:
    """Microseconds per call of ``fn`` (which enqueues one launch), averaged over ``iters`` back-to-back calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def kernel_part(args) -> None:
    from latentblending_amd.hip import ops
    from latentblending_amd.native.scheduler import NativeDDIMScheduler, NativeDPMSolverPP2MScheduler, NativeLCMScheduler
    dev = "cuda"
    per_sample = 4 * 128 * 128                                  # one 1024^2 latent
    B = (args.gib << 30) // 2 // per_sample                     # latents in ``--gib`` GiB of fp16
    n = B * per_sample
    g = torch.Generator(device=dev).manual_seed(0)
    state = torch.randn(2, B, per_sample, generator=g, device=dev, dtype=torch.float16)
    eps = torch.randn(2 * B, per_sample, generator=g, device=dev, dtype=torch.float16)
    noise = torch.randn(B, per_sample, generator=g, device=dev, dtype=torch.float16)
    out2 = torch.empty_like(state)
    x, out1 = state[0], out2[0]
    s = torch.cuda.current_stream().cuda_stream
    dpm, ddim, lcm = NativeDPMSolverPP2MScheduler(True, device="cpu"), NativeDDIMScheduler(device="cpu"), NativeLCMScheduler(device="cpu")
    dpm.set_timesteps(20)
    ddim.set_timesteps(30)
    lcm.set_timesteps(4)
    rows = {"dpm2": ops.step_params([dpm.step_row(7, 4.0)] * B, dev), "dpm1": ops.step_params([dpm.step_row(7, 4.0, first=True)] * B, dev),
            "ddim": ops.step_params([ddim.step_row(7, 4.0)] * B, dev), "lcm": ops.step_params([lcm.step_row(1, 4.0)] * B, dev)}
    api = ops.api
    P = lambda t: t.data_ptr()      # noqa: E731
    cases = [
        ("lb_dpmpp2m_step_f16 cfg 0: second-order rows", 10, lambda: api.lb_dpmpp2m_step_f16(P(state), P(eps), P(out2), P(rows["dpm2"]), per_sample, B, 0, s)),
        ("lb_dpmpp2m_step_f16 cfg 0: first-order rows", 8, lambda: api.lb_dpmpp2m_step_f16(P(state), P(eps), P(out2), P(rows["dpm1"]), per_sample, B, 0, s)),
        ("lb_dpmpp2m_step_f16 cfg 1: second-order rows, CFG", 12, lambda: api.lb_dpmpp2m_step_f16(P(state), P(eps), P(out2), P(rows["dpm2"]), per_sample, B, 1, s)),
        ("lb_ddim_step_f16 cfg 0: DDIM", 6, lambda: api.lb_ddim_step_f16(P(x), P(eps), P(out1), P(rows["ddim"]), per_sample, B, 0, s)),
        ("lb_ddim_step_f16 cfg 1: DDIM, CFG", 8, lambda: api.lb_ddim_step_f16(P(x), P(eps), P(out1), P(rows["ddim"]), per_sample, B, 1, s)),
        ("lb_lcm_step_f16 cfg 0: latent-consistency step", 8, lambda: api.lb_lcm_step_f16(P(x), P(eps), P(noise), P(out1), P(rows["lcm"]), per_sample, B, 0, 0, s)),
    ]
    for rnd in range(args.rounds):
        for name, bytes_per_element, fn in cases:
            us = time_launches(fn, args.iters)
            print(json.dumps({"part": "kernel", "round": rnd, "name": name, "batch": B, "per_sample": per_sample, "us": round(us, 1),
                              "bytes_per_element": bytes_per_element, "GB_per_s": round(bytes_per_element * n / us * 1e-3, 1)}), flush=True)
    assert torch.isfinite(out2).all()


def transition_part(args) -> None:
    import numpy as np
    import bench                                                # (repository root: the benchmark's synthetic-weight provider)
    import latentblending_amd.native as N
    from latentblending_amd import BlendingEngine
    from latentblending_amd.native.frames import materialise_frames
    dev = "cuda:0"
    unet_prov = bench.device_synthetic_provider(0, dev)
    vae_prov = N.SyntheticProvider(1)
    base = N.NativeSDXLPipe(turbo=False, unet_provider=unet_prov, vae_provider=vae_prov, device=dev, allow_synthetic=True)
    for spec in args.samplers.split(","):
        name, steps = spec.split(":")
        steps = int(steps)
        pipe = base if name == "euler" else N.NativeSDXLPipe(turbo=False, unet_native=base.unet_native, vae_native=base.vae_native,
                                                             device=dev, allow_synthetic=True, scheduler=name)
        np.random.seed(0)
        be = BlendingEngine(pipe, do_compile=True, frontier_width=16, verbose=False)
        be.host_frames = True
        be.set_dimensions((1024, 1024))
        be.set_num_inference_steps(steps)
        be.set_guidance_scale(4.0)
        be.set_prompt1("photo of underwater landscape, fish, und the sea, incredible detail, high resolution")
        be.set_prompt2("rendering of an alien planet, strange plants, strange creatures, surreal")
        be.set_branching(depth_strength=0.5, nmb_max_branches=15)
        runs = []
        for _ in range(1 + args.repeats):                       # the first run records the programs and captures their graphs
            pipe.stats["unet_samples"] = pipe.stats["unet_forwards"] = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            imgs = be.run_transition(fixed_seeds=[420, 421])
            materialise_frames(imgs)
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
        best = min(runs[1:])
        print(json.dumps({"part": "transition", "sampler": name, "steps": steps, "frames": len(imgs), "seconds_first_run": round(runs[0], 3),
                          "seconds": round(best, 4), "all_seconds": [round(r, 4) for r in runs[1:]], "frames_per_s": round(len(imgs) / best, 3),
                          "unet_forwards": pipe.stats["unet_forwards"], "unet_samples": pipe.stats["unet_samples"],
                          "levels": [int(v) for v in be.list_idx_injection], "stems": [int(v) for v in be.list_nmb_stems]}), flush=True)
        del be


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("kernel", "transition"), required=True)
    ap.add_argument("--gib", type=int, default=1, help="kernel part: GiB of fp16 latents in the batch")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="kernel part: passes over all kernels (interleaved)")
    ap.add_argument("--samplers", default="euler:30,dpmpp_2m_karras:20", help="transition part: sampler:steps pairs")
    ap.add_argument("--repeats", type=int, default=2, help="transition part: timed runs after the recording one")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    import socket
    print(json.dumps({"part": "box", "host": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__}), flush=True)
    (kernel_part if args.part == "kernel" else transition_part)(args)


if __name__ == "__main__":
    main()
