"""``attscan.traceback`` (the host half of the att-site alignment: aligned strings rebuilt inside the box a device
result row names) against the CPU reference of tests/alignpairs_reference.py on the fixed case table."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import alignpairs_cases as cases  # noqa: E402
import alignpairs_reference as ref  # noqa: E402


@pytest.fixture(scope="module")
def table():
    """(name, query, ref as the aligner sees it, reference alignment) per case - computed once."""
    out = []
    for name, q, r, rev in cases.all_cases():
        seen = ref.reverse_complement(r) if rev else r
        out.append((name, q, seen, ref.align(q, seen)))
    return out


def test_hand_made_cases_are_untied_and_fuzz_is_mostly(table):
    """With the helper alone: a tied case has co-optimal alignments, which pin nothing but score and end cell."""
    hand = [(n, a) for n, _, _, a in table if not n.startswith("fuzz_")]
    fuzz = [a for n, _, _, a in table if n.startswith("fuzz_")]
    assert len(fuzz) == 200 and len(hand) >= 14
    assert [n for n, a in hand if a["tied"]] == []
    assert all(a["score"] > 0 for _, a in hand)
    assert sum(a["tied"] for a in fuzz) <= 0.10 * len(fuzz)
    assert sum(a["score"] > 0 for a in fuzz) >= 150


def test_case_table_holds_what_it_says(table):
    by = {n: a for n, _, _, a in table}
    for L in (20, 33, 64, 120, 251, 600):
        a = by[f"exact_{L}"]
        assert (a["score"], a["cols"], a["fgaps"], a["rgaps"], a["idents"]) == (2 * L, L, 0, 0, L)
    assert (by["mismatch"]["cols"], by["mismatch"]["idents"], by["mismatch"]["score"]) == (150, 149, 2 * 149 - 100)
    assert (by["query_gap"]["fgaps"], by["query_gap"]["rgaps"], by["query_gap"]["score"]) == (1, 0, 2 * 159 - 100)
    assert (by["ref_gap3"]["fgaps"], by["ref_gap3"]["rgaps"], by["ref_gap3"]["score"]) == (0, 3, 2 * 167 - 110)
    assert by["lower_case"]["idents"] == 90 and any(c.islower() for c in by["lower_case"]["query"])
    a = by["n_in_repeat"]                                       # N against N is a mismatch, paid for by > 50 matches on both sides
    assert (a["cols"], a["idents"], a["score"]) == (180, 179, 2 * 179 - 100)
    assert by["revcomp_40"]["score"] == 80 and by["revcomp_130"]["score"] == 260
    assert (by["revcomp_ref_gap"]["rgaps"], by["revcomp_ref_gap"]["score"]) == (1, 2 * 139 - 100)


def test_traceback_reproduces_the_reference(table):
    from jaeger_amd import attscan
    for name, q, seen, a in table:
        got = attscan.traceback(q, seen, ref.result_row(a))
        if a["score"] == 0:
            assert got["query"] == got["ref"] == got["comp"] == "", name
            continue
        assert (got["score"], got["end_query"], got["end_ref"]) == (a["score"], a["end_q"], a["end_r"]), name
        if not a["tied"]:
            assert (got["query"], got["ref"], got["comp"]) == (a["query"], a["ref"], a["comp"]), name


def test_traceback_refuses_a_row_that_does_not_fit(table):
    from jaeger_amd import attscan
    name, q, seen, a = next(t for t in table if t[0] == "query_gap")
    row = ref.result_row(a)
    for col, delta in ((0, 2), (2, -1), (3, 1), (4, -1)):     # score, query gaps, reference gaps, identities
        bad = list(row)
        bad[col] += delta
        with pytest.raises(ValueError):
            attscan.traceback(q, seen, bad)


def test_reverse_complement_keeps_the_reference_table():
    from jaeger_amd import attscan
    assert attscan.reverse_complement("ACGTacgtNRYKMBVDHWSn-x") == "N-NSWDHBVKMRYNACGTACGT"
