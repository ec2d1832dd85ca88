"""Child process of test_graph_instantiated_before_any_eager_run (test_program_replay_gpu.py): record, instantiate WITHOUT any eager
run, launch the graph, then launch the same ops directly and compare the bytes.  Prints one ``VERDICT`` line; exit code 0 = equal."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import _replay as RP  # noqa: E402

# one op (at least) of each kernel family that sets a dynamic-LDS attribute on first use: halo conv (both tilings come with the
# routing case) and upconv, direct-to-LDS GEMM tiles 4 / 10 and the ping-pong tile 9, ping-pong and 5-stage attention
CASES = ["conv_direct_launchers", "conv_routing", "gemm_v1t4_300x260x128", "gemm_v-1t9_300x260x128", "gemm_v1t10_300x260x128",
         "attn_d64_pingpong_qg1", "attn_d64_ring5_qg1"]


def main():
    drv = RP.GpuDriver()
    cases = [RP.build_case(cid) for cid in CASES]
    progs = []
    for c in cases:
        c.restore()
        progs.append(drv.record(c))
    for p in progs:                     # nothing of the library has been launched in this process so far
        p.instantiate()
    for p in progs:
        p.launch()
    drv.sync()
    graph = [c.snapshot() for c in cases]
    bad = []
    for c, g in zip(cases, graph):
        c.restore()
        drv.direct(c)
        bad += [f"{c.name}: {name}" for name in c.differs(g)]
        if any(torch.equal(o.bits, o.init) for o in c.outs):
            bad.append(f"{c.name}: an output was never written")
    print("VERDICT " + ("equal" if not bad else "differ: " + "; ".join(bad)))
    return 0 if not bad else 1


if __name__ == "__main__":
    sys.exit(main())
