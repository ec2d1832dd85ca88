"""Recorder of the sampler step kernels' bits: every sampler (Euler, Euler-ancestral, DDIM, latent-consistency, DPM-Solver++ 2M),
with and without CFG, in the vector and in the scalar form, on seeded inputs under per-sample guidance values that are NOT
representable in fp16 - so that ``g * diff`` of the CFG combine is inexact in fp32 and a build that rounds it once (a fused
multiply-and-round) differs from one that rounds it twice.  It calls nothing but ``ops.*`` and the schedulers' ``step_row``, so
the same file runs on any commit; two commits that record the same thing compute the same bits.

    python -m oracle.record_sampler_bits --out tests/golden/sampler_step_parent_bits.json --commit <hash>     # on an MI355X

``tests/golden/sampler_step_parent_bits.json`` was written by this command at the commit BEFORE the step kernels were folded
into one skeleton (the hash is in the file); ``tests/test_sampler_bits_gpu.py`` holds every later commit to it.  The file stores
the seeds and the parameter rows, so a replay depends on the kernels alone, not on the host tables."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B = 2
SIZES = (40, 43)                       # 40: the vector form, 5 lanes of 16 bytes, empty tail; 43: the scalar form alone
GUIDANCE = (4.37, 2.718281828)         # per sample; neither is an fp16 value, nor is their product with one exact in fp32
SEEDS = {"x": 9101, "eps": 9102, "noise": 9103, "m1": 9104}
SCALES = {"x": 4.0, "eps": 1.0, "noise": 1.0, "m1": 1.5}


def build_rows() -> dict:
    """One list of B rows per case kind, from the native schedulers' ``step_row`` at middle steps (and the last / first-order
    rows the LCM and DPM-Solver++ cases are about)."""
    from latentblending_amd.native.scheduler import (NativeDDIMScheduler, NativeDPMSolverPP2MScheduler, NativeEulerScheduler,
                                                     NativeLCMScheduler)
    g0, g1 = GUIDANCE
    euler, anc = NativeEulerScheduler(False, device="cpu"), NativeEulerScheduler(True, device="cpu")
    ddim, lcm, dpm = NativeDDIMScheduler(device="cpu"), NativeLCMScheduler(device="cpu"), NativeDPMSolverPP2MScheduler(True, device="cpu")
    euler.set_timesteps(30)
    anc.set_timesteps(4)
    ddim.set_timesteps(30)
    lcm.set_timesteps(4)
    dpm.set_timesteps(20)
    rows = {"euler": [euler.step_row(14, g0), euler.step_row(15, g1)],
            "euler_ancestral": [anc.step_row(1, g0), anc.step_row(2, g1)],
            "ddim": [ddim.step_row(14, g0), ddim.step_row(15, g1)],
            "lcm": [lcm.step_row(1, g0), lcm.step_row(2, g1)],
            "lcm_mixed": [lcm.step_row(3, g0), lcm.step_row(1, g1)],                 # a last row and a non-last row
            "lcm_all_last_null_noise": [lcm.step_row(3, g0), lcm.step_row(3, g1)],
            "dpmpp2m": [dpm.step_row(7, g0), dpm.step_row(8, g1)],
            "dpmpp2m_mixed": [dpm.step_row(7, g0, first=True), dpm.step_row(7, g1)]}  # a first-order and a second-order row
    return {k: [[float(v) for v in r] for r in rs] for k, rs in rows.items()}


def _rnd(inp, name, n, rows):
    """A CPU-generator draw: seed ``seeds[name] + n``, N(0, 1) times ``scales[name]``, rounded to fp16."""
    g = torch.Generator().manual_seed(inp["seeds"][name] + n)
    return (torch.randn(rows, n, generator=g) * inp["scales"][name]).to(torch.float16)


def compute(inp: dict, device="cuda") -> dict:
    """``inp`` (the "input" entry of the file) -> {case name: int16 views of the output, flattened}; both planes for DPM-Solver++."""
    from latentblending_amd.hip import ops
    nb = inp["B"]
    out = {}
    for n in inp["sizes"]:
        x, eps, noise, m1 = (_rnd(inp, k, n, r).to(device) for k, r in (("x", nb), ("eps", 2 * nb), ("noise", nb), ("m1", nb)))
        state = torch.stack([x, m1]).contiguous()
        for cfg in (0, 1):
            e = eps if cfg else eps[:nb].contiguous()
            for kind, rows in inp["rows"].items():
                p = ops.step_params(rows, device)
                if kind == "euler":
                    o = ops.euler_step(x, e, p, cfg=bool(cfg))
                elif kind == "euler_ancestral":
                    o = ops.euler_step(x, e, p, noise=noise, cfg=bool(cfg), ancestral=True)
                elif kind == "ddim":
                    o = ops.ddim_step(x, e, p, cfg=bool(cfg))
                elif kind.startswith("lcm"):
                    o = ops.lcm_step(x, e, p, noise=None if kind.endswith("null_noise") else noise, cfg=bool(cfg))
                else:
                    o = ops.dpmpp2m_step(state, e, p, cfg=bool(cfg))
                torch.cuda.synchronize()
                out[f"{kind}_n{n}_cfg{cfg}"] = o.cpu().contiguous().view(torch.int16).flatten().tolist()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", required=True, help="the commit the library was built from (stored in the file)")
    a = ap.parse_args(argv)
    inp = {"B": B, "sizes": list(SIZES), "guidance": list(GUIDANCE), "seeds": dict(SEEDS), "scales": dict(SCALES), "rows": build_rows()}
    cases = compute(inp)
    with open(a.out, "w") as f:          # one line per case
        f.write('{"recorded_at": ' + json.dumps(a.commit) + ',\n"device": ' + json.dumps(torch.cuda.get_device_name(0)) + ',\n"input": '
                + json.dumps(inp) + ',\n"cases": {\n' + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":"))
                                                                    for k, v in cases.items()) + "\n}}\n")
    print(json.dumps({"cases": len(cases), "values": sum(len(v) for v in cases.values())}))


if __name__ == "__main__":
    main()
