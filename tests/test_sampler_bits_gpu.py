"""Every sampler step kernel bit for bit against tests/golden/sampler_step_parent_bits.json: what the commit named in the file
computed on an MI355X for Euler, Euler-ancestral, DDIM, the latent-consistency step (non-last rows, a last row beside a non-last
one, all-last rows with a null noise pointer) and DPM-Solver++ 2M (second-order rows, a first-order row beside a second-order
one; both output planes), each with and without CFG, at per_sample 40 (vector form, 5 lanes, empty tail) and 43 (scalar form).

The per-sample guidance values (4.37, 2.718281828) are not fp16 values: ``g * diff`` of the CFG combine is inexact in fp32, so a
build that fuses "multiply, round to fp32, round to fp16" into one multiply-and-round differs from one that rounds twice.  The
other parent-bit fixtures (lcm_euler_modes.json, dpmpp_ddim_parent_bits.json) use guidances that are exact in fp16 and cannot
see that.  Recorder and replay are one function, oracle/record_sampler_bits.py::compute, over the seeds and rows in the file.
"""
import json
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import record_sampler_bits as REC  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_step_parent_bits.json")
KINDS = ("euler", "euler_ancestral", "ddim", "lcm", "lcm_mixed", "lcm_all_last_null_noise", "dpmpp2m", "dpmpp2m_mixed")


def test_every_sampler_step_keeps_the_recorded_bits():
    with open(GOLD) as fh:
        gold = json.load(fh)
    inp = gold["input"]
    assert inp["B"] == 2 and inp["sizes"] == [40, 43] and tuple(inp["rows"]) == KINDS
    for g in inp["guidance"]:                   # the fixture's point: guidance that fp16 cannot hold
        assert float(torch.tensor(g, dtype=torch.float32).half()) != float(torch.tensor(g, dtype=torch.float32))
    assert inp["rows"]["lcm_mixed"][0][5] == 0 and inp["rows"]["lcm_mixed"][1][5] != 0
    assert inp["rows"]["dpmpp2m_mixed"][0][5] == 0 and inp["rows"]["dpmpp2m_mixed"][1][5] != 0
    got = REC.compute(inp)
    assert sorted(got) == sorted(gold["cases"]) and len(got) == len(KINDS) * 2 * 2
    changed = []
    for name, want in gold["cases"].items():
        n = int(re.search(r"_n(\d+)_cfg[01]$", name).group(1))
        planes = 2 if name.startswith("dpmpp2m") else 1
        assert len(want) == planes * inp["B"] * n, name
        diff = sum(a != b for a, b in zip(got[name], want))
        print(f"[sampler bits] {name}: {diff} of {len(want)} values differ from {gold['recorded_at'][:7]}")
        if diff or len(got[name]) != len(want):
            changed.append((name, diff))
    assert not changed, changed
