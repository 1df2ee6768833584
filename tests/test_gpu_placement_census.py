"""Where every op runs, pinned: for one model per family and the row lengths that flip a placement
(placement_cases.py), the launches and FLOPs per profiling class of one forward over 8 windows, ``describe()``, the
placement statistics and the model's FLOPs per window equal golden/placement_census.json exactly.

The golden file is recorded by scripts/record_placement_census.py from a library built at the commit BEFORE a change to
the host code, never from the code under test.  Everything in it is host arithmetic - launch counts are integers, the
FLOPs are doubles computed on the host by fixed formulas - so equality is exact.  A placement regression (a conv off the
split-f16 kernels, a fused block or the small-window kernel no longer taken) passes every parity test and runs 4 - 5x
slower: this is the guard for it, and for the FLOP formulas of the profiling bracket (the x 2 of a fused block
included)."""
import json

import placement_cases as pc
import pytest
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "placement_census.json").read_text())


def test_golden_covers_the_cases(golden):
    assert sorted(golden) == sorted(pc.MODELS)


@pytest.mark.parametrize("name", sorted(pc.MODELS))
def test_placement_census(golden, name):
    got = json.loads(json.dumps(pc.census(name)))          # (through JSON: lists and float repr as recorded)
    want = golden[name]
    assert got["describe"] == want["describe"]
    assert got["stats"] == want["stats"]
    assert got["flops_per_window"] == want["flops_per_window"]
    assert sorted(got["runs"]) == sorted(want["runs"])
    for run, classes in want["runs"].items():
        assert got["runs"][run] == classes, (name, run)
