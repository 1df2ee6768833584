#!/usr/bin/env python3
"""Golden vectors for the prophage segmentation and report, produced by IMPORTING the reference's
postprocess/prophages.py (``segment``, ``prophage_report``) with stub modules in place of what is not installed:

* ``ruptures.KernelCPD`` / ``kneed.KneeLocator`` replay RECORDED breakpoints and knees, so that ``segment`` pins the lines
  behind them (ranges, inclusive means, merge, fallback index, the except path);
* ``pyfastx.Fasta`` iterates the recorded contigs, ``parasail.sw_trace_scan_16`` answers with result objects filled from
  the alignments of tests/alignpairs_reference.py, so that ``prophage_report`` pins the coordinate arithmetic, the LTR_
  rule, the empty-flank row and the TSV text.

Build container only; outputs are data (no reference code is kept):

    python tests/golden/make_golden_prophage_report.py <reference>/src   ->  prophage_segment.json, prophage_report.json
"""
import json
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import pandas as pd

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))            # tests/: the alignment helper
sys.path.insert(0, str(HERE.parents[1]))        # the repository: oracle/
sys.path.insert(0, sys.argv[1])
import alignpairs_reference as helper  # noqa: E402

for name in ("pyfastx", "parasail", "ruptures", "matplotlib", "matplotlib.pyplot", "matplotlib.patches",
             "matplotlib.lines", "kneed", "pycirclize"):
    m = types.ModuleType(name)
    for attr in ("Patch", "Line2D", "KneeLocator", "Circos"):
        setattr(m, attr, object)
    sys.modules.setdefault(name, m)
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
from jaeger.postprocess import prophages as P  # noqa: E402

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def rand_seq(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes().decode()


# ---- segment ---------------------------------------------------------------------------------------------------------
def make_segment():
    rng = np.random.Generator(np.random.PCG64(524))
    replay = {}

    class KernelCPD:
        def __init__(self, **kw):
            assert kw == {"kernel": "linear", "min_size": 3, "jump": 1}

        def fit(self, x):
            self.table = replay["bkpts"]
            return self

        def predict(self, pen):
            if replay.get("raise_in_predict"):
                raise RuntimeError("replayed failure")
            return list(self.table[str(pen)])

    class KneeLocator:
        def __init__(self, x, y, curve, direction):
            assert (curve, direction) == ("convex", "decreasing")
            self.knee = replay["knee"]

    P.rpt = types.SimpleNamespace(KernelCPD=KernelCPD)
    P.KneeLocator = KneeLocator
    n = 60
    track = rng.normal(0.4, 0.15, n)
    track[20:32] += 2.2
    track[32:38] += 1.3
    track[50:54] += 2.6
    fine = [8, 20, 26, 32, 38, 50, 54, 60]
    mid = [20, 32, 38, 50, 54, 60]
    coarse = [20, 38, 60]
    cases = []

    def case(name, bkpts, knee, length=600_000, cutoff=500_000, sensitivity=1.5, **extra):
        cases.append(dict(name=name, bkpts={str(p): b for p, b in bkpts.items()}, knee=knee, length=length,
                          cutoff=cutoff, sensitivity=sensitivity, **extra))

    nine = {1: fine, 2: fine, 3: mid, 4: mid, 5: mid, 6: coarse, 7: coarse, 8: [60], 9: [60]}
    case("knee_picks_mid", nine, len(mid))
    case("knee_picks_coarse", nine, len(coarse))
    case("no_knee_takes_the_first", nine, None)
    case("touching_ranges_merge", nine, len(fine), sensitivity=1.0)
    case("nothing_above_sensitivity", nine, len(mid), sensitivity=9.0)
    case("knee_not_a_length", nine, 5)                                    # .index raises -> the except path
    case("one_segment_everywhere", {p: [60] for p in range(1, 10)}, None)
    case("predict_raises", nine, None, raise_in_predict=True)
    case("at_the_cutoff_is_skipped", nine, len(mid), length=500_000)
    out = []
    for c in cases:
        replay.clear()
        replay.update(bkpts=c["bkpts"], knee=c["knee"], raise_in_predict=c.get("raise_in_predict", False))
        frame = pd.DataFrame({"phage": track.copy(), "bacteria": 1 - track})
        got = P.segment({"ctg": [frame, "bacteria", c["length"]]}, outdir=None, cutoff_length=c["cutoff"],
                        sensitivity=c["sensitivity"], identifier="phage")
        if "ctg" in got:
            ranges, scores = got["ctg"]
            c["expected"] = {"ranges": np.asarray(ranges).tolist(), "scores": [float(s) for s in np.asarray(scores).tolist()]}
        else:
            c["expected"] = None
        out.append(c)
        print("segment", c["name"], c["expected"])
    (HERE / "prophage_segment.json").write_text(json.dumps({"track": track.tolist(), "cases": out}, indent=1) + "\n")


# ---- prophage_report -------------------------------------------------------------------------------------------------
class Contig:
    """A contig of N with stretches of real sequence, recorded as (start, text) pieces."""

    def __init__(self, name, length):
        self.name, self.length, self.pieces = name, length, {}

    def put(self, start, text):
        assert 0 <= start and start + len(text) <= self.length
        seq = self.sequence()
        seq = seq[:start] + text + seq[start + len(text):]
        # re-record as maximal non-N stretches
        self.pieces, at = {}, 0
        arr = np.frombuffer(seq.encode(), np.uint8)
        real = np.concatenate(([False], arr != ord("N"), [False]))
        edges = np.nonzero(real[1:] != real[:-1])[0]
        for a, b in zip(edges[::2], edges[1::2]):
            self.pieces[int(a)] = seq[a:b]

    def sequence(self):
        out = bytearray(b"N" * self.length)
        for start, text in self.pieces.items():
            out[start:start + len(text)] = text.encode()
        return out.decode()


def make_report():
    rng = np.random.Generator(np.random.PCG64(706))
    calls = []

    def sw_trace_scan_16(s1, s2, gap_open, gap_extend, matrix):
        assert (gap_open, gap_extend, matrix) == (100, 5, ("ACGT", 2, -100))
        a = helper.align(s1, s2)
        calls.append({"q_len": len(s1), "r_len": len(s2), "row": helper.result_row(a)})
        return types.SimpleNamespace(score=a["score"], end_query=a["end_q"], end_ref=a["end_r"], saturated=False,
                                     traceback=types.SimpleNamespace(query=a["query"], ref=a["ref"], comp=a["comp"]))

    P.parasail = types.SimpleNamespace(matrix_create=lambda alphabet, match, mismatch: (alphabet, match, mismatch),
                                       sw_trace_scan_16=sw_trace_scan_16)
    P.pyfastx = types.SimpleNamespace(Fasta=lambda records, build_index: iter(records))

    def flanks(ctg, raw_start, raw_end, inside=2000, outside=4000):
        """Real sequence over both flanks of a region (the interior beyond ``inside`` stays N)."""
        a, b = max(raw_start - outside, 0), min(raw_start + inside, ctg.length)
        ctg.put(a, rand_seq(rng, b - a))
        a, b = max(raw_end - inside, 0), min(raw_end + outside, ctg.length)
        if b > a:
            ctg.put(a, rand_seq(rng, b - a))

    runs = []
    # run 1: fsize 2000, stride 1500 - raw_start = 1500 start, raw_end = 1500 (end - 1) + 2000
    A = Contig("ctgA,1", 600_000)
    regions_a = []
    # region at the contig's start: search_start clamps to 0; a 30-base direct repeat
    flanks(A, 1500, 6500)
    rep = rand_seq(rng, 30)
    A.put(700, "N" + rep + "N"); A.put(7000, rep)
    regions_a.append(((1, 4), 2.4375))
    # DTR, region_len // 2 >= 14000: off_set 2000; 40-base direct repeat outside the region on both sides
    flanks(A, 150_000, 182_000)
    rep = rand_seq(rng, 40)
    A.put(149_600, "N" + rep + "N"); A.put(182_300, rep)
    regions_a.append(((100, 121), 3.0123456))
    # ITR, region_len // 2 < 14000: off_set = region_len // 4; lower case inside the repeat; the whole region is real
    flanks(A, 300_000, 308_000, inside=4000)
    rep = rand_seq(rng, 60)
    A.put(299_000, "N" + rep[:20] + rep[20:30].lower() + rep[30:] + "N"); A.put(309_100, helper.reverse_complement(rep))
    regions_a.append(((200, 205), 1.75))
    # neither: only 300 real bases in each flank - nothing of more than 12 columns
    A.put(449_800, rand_seq(rng, 300)); A.put(454_500 + 100, rand_seq(rng, 300))
    regions_a.append(((300, 303), 1.6))
    # LTR_DTR: a 300-base direct repeat with one base missing in the right copy (a gap in the reference row)
    flanks(A, 525_000, 561_000)
    rep = rand_seq(rng, 300)
    A.put(524_000, "N" + rep + "N"); A.put(561_500, rep[:140] + rep[141:])
    regions_a.append(((350, 374), 2.2))
    # the last window hangs over the contig's end: an empty right flank, no alignment at all
    A.put(598_000, rand_seq(rng, 2000))
    regions_a.append(((399, 400), 1.9))
    short = Contig("short", 3000)
    short.put(0, rand_seq(rng, 3000))
    runs.append(dict(fsize=2000, stride=1500, contigs=[short, A],
                     cords=[[[[0, 1]], [2.0]], [[list(c) for c, _ in regions_a], [s for _, s in regions_a]]]))
    # run 2: stride None (step = fsize); a name holding ___; a zero-width region (off_set 0) with a 25-base direct repeat;
    # a contig without regions between the two
    B = Contig("ctg___B", 510_000)
    flanks(B, 200_000, 200_000, inside=0)
    rep = rand_seq(rng, 25)
    B.put(199_000, "N" + rep + "N"); B.put(200_900, rep)
    # second region: ITR and DTR both there, the DTR scores higher
    flanks(B, 400_000, 406_000)
    rep, rep2 = rand_seq(rng, 50), rand_seq(rng, 35)
    B.put(399_500, "N" + rep + "N" + rep2 + "N"); B.put(406_400, rep + "N" + helper.reverse_complement(rep2))
    empty = Contig("no_regions", 505_000)
    runs.append(dict(fsize=2000, stride=None, contigs=[empty, B],
                     cords=[None, [[[100, 100], [200, 203]], [1.52, 4.25]]]))
    out = []
    for run in runs:
        calls.clear()
        records = [(c.name, c.sequence()) for c in run["contigs"]]
        by_name = {c.name.replace(",", "___"): cd for c, cd in zip(run["contigs"], run["cords"]) if cd is not None}
        cords = {k: [np.array(v[0]), np.array(v[1])] for k, v in by_name.items()}
        with tempfile.TemporaryDirectory() as tmp:
            P.prophage_report(run["fsize"], records, cords, Path(tmp), refined_boundaries=None, stride=run["stride"])
            tsv = (Path(tmp) / "prophages_jaeger.tsv").read_text()
        print(tsv)
        out.append(dict(fsize=run["fsize"], stride=run["stride"], cords=run["cords"], alignments=list(calls), tsv=tsv,
                        contigs=[dict(name=c.name, length=c.length, pieces=[[s, t] for s, t in sorted(c.pieces.items())])
                                 for c in run["contigs"]]))
    (HERE / "prophage_report.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    make_segment()
    make_report()
