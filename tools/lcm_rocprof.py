"""rocprofv3 kernel durations of the three sampler step kernels on the same >= 1 GiB batch: the latent-consistency step
(lb_lcm_step_f16), the DDIM step and the Euler-ancestral step - three instantiations of sampler_step_kernel (csrc/mix.hip),
told apart by the policy name in the kernel symbol.

  rocprofv3 --kernel-trace --stats --output-format csv -d lcm_rocprof_out -- python tools/lcm_rocprof.py run lcm_rocprof_out
  python tools/lcm_rocprof.py fold lcm_rocprof_out lcm_rocprof_out/summary.json

`run` launches each kernel ITER times on `pairs` latents of 4 x 64 x 64 fp16 (the batch of tools/mixing_rocprof.py) with per-sample
rows of a 4-step schedule's first step; `fold` divides the algorithmic byte counts (LCM and Euler-ancestral: x, eps, noise in, out
= 8 B / element; DDIM: 6) by the average durations in rocprofv3's kernel_stats.csv."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ITER = 10
META_NAME = "lcm_rocprof_meta.json"          # written by `run` into the trace directory, read back by `fold`


def run(out_dir):
    import torch
    from latentblending_amd.hip.lib import api
    from latentblending_amd.native.scheduler import NativeDDIMScheduler, NativeEulerScheduler, NativeLCMScheduler
    dev = "cuda"
    n = 4 * 64 * 64
    pairs = (1 << 30) // (n * 2 * 3)
    x, eps, noise = (torch.randn(pairs, n, device=dev).half() for _ in range(3))
    out = torch.empty_like(x)

    def rows(sched, steps):
        sched.set_timesteps(steps)
        row = [float(v) for v in sched.step_row(0, 0.0)]
        return torch.tensor([row + [0.0] * (8 - len(row))] * pairs, dtype=torch.float32, device=dev)
    p_lcm, p_ddim = rows(NativeLCMScheduler(device=dev), 4), rows(NativeDDIMScheduler(device=dev), 30)
    p_anc = rows(NativeEulerScheduler(True, device=dev), 4)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()      # noqa: E731
    for _ in range(ITER):
        api.lb_lcm_step_f16(P(x), P(eps), P(noise), P(out), P(p_lcm), n, pairs, 0, 0, st)
        api.lb_ddim_step_f16(P(x), P(eps), P(out), P(p_ddim), n, pairs, 0, st)
        api.lb_euler_step_f16(P(x), P(eps), P(noise), P(out), P(p_anc), n, pairs, 0, 1, st)
    torch.cuda.synchronize()
    os.makedirs(out_dir, exist_ok=True)
    json.dump({"pairs": pairs, "elements_per_pair": n, "iters": ITER,
               "bytes": {"LcmStep": pairs * n * 8, "DdimStep": pairs * n * 6, "EulerStep": pairs * n * 8}},      # (policy names)
              open(os.path.join(out_dir, META_NAME), "w"))


def fold(src, dst):
    meta = json.load(open(os.path.join(src, META_NAME)))
    files = glob.glob(os.path.join(src, "**", "*kernel_stats.csv"), recursive=True)
    rows = list(csv.DictReader(open(files[0])))
    out = {"command": "rocprofv3 --kernel-trace --stats -- python tools/lcm_rocprof.py run", "batch": meta, "kernels": []}
    for key, nbytes in meta["bytes"].items():
        for r in rows:
            if key in r["Name"]:
                avg_ns = float(r["AverageNs"])
                out["kernels"].append({"name": r["Name"][:120], "calls": int(r["Calls"]), "avg_us": avg_ns / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                                       "algorithmic_bytes": nbytes, "GB_per_s": nbytes / avg_ns if avg_ns else 0.0})
    json.dump(out, open(dst, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        fold(sys.argv[2], sys.argv[3])
