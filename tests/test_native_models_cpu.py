"""Every native model packs the bits and records the ops it did before the packer (``native/weights.py: Packer``) and the program
base (``native/runtime.py: RecordedProgram``) were shared: ``tests/golden/native_models.json`` was written by
``oracle/record_native_models.py`` at the commit before that one, and the same recorder must reproduce it entry for entry."""
import json
import os

import pytest

from oracle import record_native_models as REC

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "native_models.json")


@pytest.fixture(scope="module")
def both():
    with open(GOLDEN) as f:
        want = REC.expand(json.load(f))                 # (``weights[net]``: the digests in sorted key order)
    got = json.loads(json.dumps(REC.record()))          # (tuples -> lists, as the fixture holds them)
    return want, got


def test_the_same_cases_and_nets(both):
    want, got = both
    assert sorted(got["cases"]) == sorted(want["cases"]) and sorted(got["weights"]) == sorted(want["weights"])
    assert len(want["cases"]) == 39 and len(want["weights"]) == 15


def test_every_weight_keeps_its_name_dtype_shape_and_bits(both):
    want, got = both
    for net, digests in want["weights"].items():
        mine = got["weights"][net]                      # key -> digest; a digest covers its key
        assert len(mine) == len(digests), (net, len(mine), len(digests))
        bad = [k for k, d in zip(sorted(mine), digests) if mine[k] != d]
        assert not bad, (net, bad[:8])
    # the bias-free convs of both TAESDXL halves store None, the folded last conv of the decoder does not
    mine = got["weights"]
    assert [k for k in sorted(mine["tiny.dec"]) if mine["tiny.dec"][k] is None] == [f"decoder.layers.{n}.bias" for n in (11, 16, 6)]
    assert [k for k in sorted(mine["tiny.enc"]) if mine["tiny.enc"][k] is None] == [f"encoder.layers.{n}.bias" for n in (10, 2, 6)]
    assert want["weights"]["tiny.dec"].count(None) == 3 and want["weights"]["tiny.enc"].count(None) == 3
    assert len(want["weights"]["vae.wide"]) == len(want["weights"]["vae.scaled"]) + 9          # (``qkv.*`` and their ``_s``)


def test_every_program_records_what_it_recorded(both):
    want, got = both
    for name, rec in want["cases"].items():
        mine = got["cases"][name]
        assert sorted(mine) == sorted(rec), name
        for field in ("programs", "marks", "tap_names", "arena", "journal", "c64_launches"):
            if field in rec:
                assert mine[field] == rec[field], (name, field)
        assert mine == rec, name
    # the cases bite where they are meant to: the C64 bit is recorded in some tiny programs and not in others
    c64 = {k: v["c64_launches"] for k, v in want["cases"].items() if k.startswith("tiny.")}
    assert len(c64) == 16 and any(c64.values()) and all(v == 0 for k, v in c64.items() if k.endswith("c64_False"))
    assert all(want["cases"][k]["journal"] for k in want["cases"] if not k.startswith("tiny."))
