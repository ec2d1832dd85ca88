"""Counter-based sampler noise against the generator call it replaces, same process, alternating.

    python tools/noise_bench.py [--repeats 200] [--rounds 5] [--transition] [--out profiles/counter_noise.txt]

Two shapes, each served (a) by ``CounterNoise.keyed`` as the native loops call it - rows built on the host, ONE upload, ONE
``lb_counter_noise_f16`` launch - (b) by that launch alone on rows already on the device, and (c) by the single ``torch.randn``
the stream path makes for the same draws:

* the cfg-2 transition's noise: 38 draws of 4 x 64 x 64 (2 anchors x 4 steps + 15 mids x 2 steps, SDXL-Turbo 512^2);
* one step of a B = 17 round at 1024^2: 17 draws of 4 x 128 x 128.

Times are host wall-clock around ``--repeats`` calls ending in a device synchronise (the cost a loop pays: host work, upload,
launch, kernel), best and median of ``--rounds`` alternating rounds.  ``--transition`` adds the cfg-2 transition itself (seeded
synthetic SDXL-Turbo weights, 512^2, 4 steps, 15 mid branches, frontier 16, graphs) under ``noise="stream"`` and ``"counter"``,
alternating, on one pipe.  No threshold is set: the file records what was measured.  ``--append FILE`` copies another record
(the value tests' mismatch counts) under the timings."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from latentblending_amd.hip import ops  # noqa: E402
from latentblending_amd.native.noise import CounterNoise, anchor_id, mid_id, noise_row  # noqa: E402

SHAPES = [("cfg-2 transition: 38 draws of 4x64x64", 38, (4, 64, 64)), ("B=17 step at 1024^2: 17 draws of 4x128x128", 17, (4, 128, 128))]


def pairs_for(n):
    ids = [anchor_id(420), anchor_id(421)] + [mid_id(420, 421, (k + 1) / 16, 2) for k in range(15)]
    return [(ids[k % len(ids)], k // len(ids)) for k in range(n)]


def timed(fn, repeats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeats * 1e6


def microbench(args, dev, lines):
    src = CounterNoise(dev)
    for label, n, chw in SHAPES:
        shape = (n,) + chw
        pairs = pairs_for(n)
        rows_dev = ops.noise_rows([noise_row(t, s) for t, s in pairs], dev)
        out = torch.empty(shape, dtype=torch.float16, device=dev)
        forms = {"keyed (rows + upload + launch)": lambda: src.keyed(pairs, shape),
                 "launch alone (device rows, own out)": lambda: ops.counter_noise(rows_dev, shape, out=out),
                 "torch.randn (one call)": lambda: torch.randn(shape, device=dev, dtype=torch.float16)}
        for fn in forms.values():               # warm every form at this shape
            for _ in range(10):
                fn()
        got = {k: [] for k in forms}
        for _ in range(args.rounds):            # alternating: one round = every form once
            for k, fn in forms.items():
                got[k].append(timed(fn, args.repeats))
        lines.append(f"{label}  ({n * int(np.prod(chw)) * 2 / 1024:.0f} KiB fp16)")
        for k, v in got.items():
            lines.append(f"    {k:<38} best {min(v):8.1f} us   median {statistics.median(v):8.1f} us   (rounds: {' '.join(f'{x:.1f}' for x in v)})")
        ratio = statistics.median(got["keyed (rows + upload + launch)"]) / statistics.median(got["torch.randn (one call)"])
        lines.append(f"    keyed / randn (medians): {ratio:.2f}x" + ("  - the counter-based draw COSTS MORE than the randn it replaces" if ratio > 1 else ""))


def transition_bench(args, dev, lines):
    import latentblending_amd.native as N
    from latentblending_amd import BlendingEngine
    np.random.seed(0)
    torch.manual_seed(0)
    from bench import device_synthetic_provider          # (the benchmark's own seeded weights, finished on the GPU)
    pipe = N.NativeSDXLPipe(turbo=True, unet_provider=device_synthetic_provider(0, str(dev)), vae_provider=N.SyntheticProvider(1), device=dev,
                            allow_synthetic=True)
    be = BlendingEngine(pipe, do_compile=True, frontier_width=16, verbose=False)
    be.host_frames = True
    be.set_prompt1("photo of underwater landscape, fish, und the sea, incredible detail, high resolution")
    be.set_prompt2("rendering of an alien planet, strange plants, strange creatures, surreal")
    be.set_branching(nmb_max_branches=15)
    got = {"stream": [], "counter": []}
    for mode in got:                            # warm both (programs, graphs, code objects)
        pipe.noise = mode
        be.run_transition(fixed_seeds=[420, 421])
    for _ in range(args.rounds):
        for mode in got:
            pipe.noise = mode
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frames = be.run_transition(fixed_seeds=[420, 421])
            torch.cuda.synchronize()
            got[mode].append((time.perf_counter() - t0) * 1e3)
    lines.append(f"cfg-2 transition (SDXL-Turbo 512^2, 4 steps, {len(frames)} frames, frontier 16, graphs, host frames), synthetic weights")
    for mode, v in got.items():
        lines.append(f"    noise={mode:<8} best {min(v):8.2f} ms   median {statistics.median(v):8.2f} ms   (rounds: {' '.join(f'{x:.2f}' for x in v)})")
    lines.append(f"    counter / stream (medians): {statistics.median(got['counter']) / statistics.median(got['stream']):.4f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--transition", action="store_true")
    ap.add_argument("--append", default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "counter_noise.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("noise_bench: needs the GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = [f"# counter-based sampler noise vs the generator call it replaces: {torch.cuda.get_device_name(dev)}, "
             f"{args.repeats} calls per timing, {args.rounds} alternating rounds, host wall-clock ending in a synchronise"]
    microbench(args, dev, lines)
    if args.transition:
        transition_bench(args, dev, lines)
    if args.append and os.path.isfile(args.append):
        lines.append("# value tests (tests/test_counter_noise_gpu.py): device against fp16(float64 restatement)")
        lines += [ln.rstrip() for ln in open(args.append) if ln.strip()]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
