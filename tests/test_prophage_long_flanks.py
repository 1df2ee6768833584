"""``-p`` on regions whose flanks exceed the 6 144 bases of ``jg_align_pairs``: the report at the longest flank its rule can
produce (4 000 + 6 999 = 10 999), a long and a short region in one call, the routing of ``attscan.align_flanks`` between
the two entry points, ``_write_side_outputs`` with a 20 000-base region, and the constants.  No GPU: the device call is the
CPU reference (tests/alignpairs_reference.py) or a recording fake."""
import logging
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

ROOT = Path(__file__).resolve().parents[1]


def _with_repeat(rng, n: int, left_at: int, right_at: int, rep: str, inverted: bool = False) -> str:
    """A random contig of ``n`` bases with ``N rep N`` at ``left_at - 1`` and ``rep`` (or its reverse complement) at
    ``right_at``."""
    from alignpairs_cases import rand_seq
    from alignpairs_reference import reverse_complement
    seq = rand_seq(rng, n)
    other = reverse_complement(rep) if inverted else rep
    seq = seq[:left_at - 1] + "N" + rep + "N" + seq[left_at + len(rep) + 1:]
    seq = seq[:right_at] + other + seq[right_at + len(other):]
    assert len(seq) == n
    return seq


def _recording(log):
    import alignpairs_reference as ref

    def align(bases, jobs):
        log.append([(int(j["q_len"]), int(j["r_len"]), int(j["flags"])) for j in jobs])
        return ref.align_jobs(bases, jobs)
    return align


def _rows(path):
    head, *rows = (line.split("\t") for line in path.read_text().splitlines())
    return [dict(zip(head, row)) for row in rows]


def test_report_at_the_longest_flank_the_rule_produces(tmp_path):
    """Windows of 9 333 bases, a region of three: region_len 27 999, region_len // 2 = 13 999 < 14 000, so off_set =
    27 999 // 4 = 6 999; the contig is 110 000 bases, scan_length = min(max(int(4 400), 400), 4 000) = 4 000: both flanks
    are 10 999 bases, the most the rule gives.  A 40-base direct repeat sits 52 bases left of the region's start and 10
    bases right of its end.  One call, two jobs of 10 999 x 10 999, one DTR row with the planted site."""
    from alignpairs_cases import rand_seq
    from jaeger_amd.prophage_report import prophage_report
    rng = np.random.Generator(np.random.PCG64(10999))
    fsize, (start, end) = 9333, (4, 7)
    raw_start, raw_end = start * fsize, end * fsize
    att = rand_seq(rng, 40)
    left_at, right_at = raw_start - 52, raw_end + 10
    seq = _with_repeat(rng, 110_000, left_at, right_at, att)
    log = []
    path = prophage_report(fsize, [("long", seq)], [[np.array([[start, end]]), np.array([2.5])]], tmp_path, _recording(log),
                           stride=fsize, min_len=50_000)
    assert log == [[(10_999, 10_999, 0), (10_999, 10_999, 1)]]
    rows = _rows(path)
    assert len(rows) == 1
    got = rows[0]
    assert (got["att_type"], got["attL"], got["attR"], got["att_score"]) == ("DTR", att, att, "80")
    assert (got["sstart"], got["send"], got["estart"], got["eend"]) == (str(left_at), str(left_at + 39), str(right_at),
                                                                        str(right_at + 39))
    assert (got["raw_start"], got["raw_end"]) == (str(raw_start), str(raw_end)) == ("37332", "65331")


def test_a_long_and_a_short_region_in_one_call(tmp_path):
    """Contig one (110 000 bases, 4 000-base scans): a one-window region, off_set 2 333, flanks of 6 333 - above the short
    entry point's 6 144.  Contig two (50 000 bases, 2 000-base scans): the same window size gives flanks of 4 333 and carries
    an inverted repeat.  One call of four jobs; the rows come back in report order."""
    from alignpairs_cases import rand_seq
    from jaeger_amd.prophage_report import prophage_report
    rng = np.random.Generator(np.random.PCG64(6333))
    fsize = 9333
    att, inv = rand_seq(rng, 40), rand_seq(rng, 36)
    one = _with_repeat(rng, 110_000, 5 * fsize - 30, 6 * fsize + 25, att)
    two = _with_repeat(rng, 50_000, 2 * fsize - 100, 3 * fsize + 200, inv, inverted=True)
    cords = [[np.array([[5, 6]]), np.array([2.0])], [np.array([[2, 3]]), np.array([3.0])]]
    log = []
    path = prophage_report(fsize, [("one", one), ("two", two)], cords, tmp_path, _recording(log), stride=fsize, min_len=20_000)
    assert log == [[(6333, 6333, 0), (6333, 6333, 1), (4333, 4333, 0), (4333, 4333, 1)]]
    first, second = _rows(path)
    assert (first["contig_id"], first["att_type"], first["attL"], first["attR"]) == ("one", "DTR", att, att)
    assert (first["sstart"], first["eend"]) == (str(5 * fsize - 30), str(6 * fsize + 25 + 39))
    assert (second["contig_id"], second["att_type"], second["attL"], second["attR"]) == ("two", "ITR", inv, inv)
    assert (second["sstart"], second["send"]) == (str(2 * fsize - 100), str(2 * fsize - 100 + 36))
    assert (second["estart"], second["eend"]) == (str(3 * fsize + 200), str(3 * fsize + 200 + 36))


def test_align_flanks_routes_by_the_longest_length(monkeypatch):
    """All jobs short: one call of ``align_pairs`` with all of them.  One length of 6 145 among short ones: one call of
    ``align_pairs_long`` with all of them.  No job: shape (0, 8)."""
    from jaeger_amd import attscan
    calls = {"short": [], "long": []}

    def fake(kind):
        def call(device, bases, jobs):
            calls[kind].append((device, len(bases), [(int(j["q_len"]), int(j["r_len"])) for j in jobs]))
            return np.full((len(jobs), 8), len(calls[kind]), np.int32)
        return call

    monkeypatch.setattr(attscan, "align_pairs", fake("short"))
    monkeypatch.setattr(attscan, "align_pairs_long", fake("long"))
    bases = np.zeros(20_000, np.uint8)
    short = [(0, 100, 50, 6144, 0), (0, 0, 6144, 10, 1), (5, 5, 1, 1, 0)]
    got = attscan.align_flanks("dev", bases, attscan.make_jobs(short))
    assert got.shape == (3, 8) and calls["long"] == []
    assert calls["short"] == [("dev", 20_000, [(50, 6144), (6144, 10), (1, 1)])]
    for odd in ((0, 0, 6145, 10, 0), (0, 0, 10, 6145, 1)):
        calls["short"].clear()
        calls["long"].clear()
        mixed = short[:2] + [odd] + short[2:]
        got = attscan.align_flanks("dev", bases, attscan.make_jobs(mixed))
        assert got.shape == (4, 8) and calls["short"] == []
        assert calls["long"] == [("dev", 20_000, [(50, 6144), (6144, 10), odd[2:4], (1, 1)])]
    empty = attscan.align_flanks("dev", bases, attscan.make_jobs([]))
    assert empty.shape == (0, 8) and empty.dtype == np.int32


def test_side_outputs_with_a_20_kb_region(tmp_path, monkeypatch, caplog):
    """``-p`` behind the tables with a 20 000-base island in a 520 kb contig (the pattern of
    tests/test_prophage_report.py::test_side_outputs_with_a_region): off_set = region_len // 4, flanks of about 9 000 bases.
    The TSV appears with the planted site, nothing is logged as an error, and the one call went to the long entry point."""
    import alignpairs_reference as ref
    from alignpairs_cases import rand_seq
    from jaeger_amd import attscan, predict
    rng = np.random.Generator(np.random.PCG64(20_000))
    att = rand_seq(rng, 44)
    big = _with_repeat(rng, 520_000, 199_901, 220_050, att)
    seqs = {"s0": rand_seq(rng, 3000), "big one": big, "s2": rand_seq(rng, 4000)}
    fasta = tmp_path / "in.fasta"
    fasta.write_text("".join(f">{n}\n" + "\n".join(s[i:i + 80] for i in range(0, len(s), 80)) + "\n" for n, s in seqs.items()))
    names = ["s0", "big", "s2"]
    lens = [len(s) for s in seqs.values()]
    n_win = [max(n // 2000, 1) for n in lens]
    preds = [np.tile(np.array([[3.0, -3.0, 0.0]], np.float32), (k, 1)) for k in n_win]
    preds[1][100:110] = [-3.0, 3.0, 0.0]                    # phage over 200 000 .. 220 000
    data_full = {"headers": np.array(names), "lengths": np.array(lens), "predictions": preds,
                 "gc_skews": [rng.normal(0, 0.1, k) for k in n_win], "gcs": [rng.uniform(0.4, 0.6, k) for k in n_win]}
    class_map = {"class": ["bacteria", "phage", "eukarya"], "index": [0, 1, 2]}
    opt = {"prophage": True, "lc": 500_000, "fsize": 2000, "stride": 2000, "sensitivity": 1.5}
    plan = SimpleNamespace(options=opt, out_dir=tmp_path, file_base="in", input_path=fasta, fsize=2000, local_rank=0)
    device = object()
    res = SimpleNamespace(class_map=class_map, engine=SimpleNamespace(device=device), y_pred=None)
    calls = {"short": [], "long": []}

    def fake(kind):
        def call(dev, bases, jobs):
            assert dev is device
            calls[kind].append([(int(j["q_len"]), int(j["r_len"])) for j in jobs])
            return ref.align_jobs(bases, jobs)
        return call

    monkeypatch.setattr(attscan, "align_pairs", fake("short"))
    monkeypatch.setattr(attscan, "align_pairs_long", fake("long"))
    with caplog.at_level(logging.INFO, logger="Jaeger"):
        predict._write_side_outputs(plan, res, data_full)
    messages = [r.getMessage() for r in caplog.records]
    assert not any("error" in m for m in messages), messages
    pro = tmp_path / "in_prophages"
    assert sorted(p.name for p in pro.iterdir()) == ["in_segmentation_inputs.npz", "prophages_jaeger.tsv"]
    assert calls["short"] == [] and len(calls["long"]) == 1 and len(calls["long"][0]) == 2
    (q_len, r_len), second = calls["long"][0]
    assert second == (q_len, r_len) and q_len == r_len and attscan.ALIGN_MAX < q_len <= attscan.ALIGN_LONG_MAX
    rows = _rows(pro / "prophages_jaeger.tsv")
    assert len(rows) == 1
    got = rows[0]
    assert (got["contig_id"], got["att_type"], got["attL"], got["attR"]) == ("big", "DTR", att, att)
    assert (got["sstart"], got["send"], got["estart"], got["eend"]) == ("199901", "199944", "220050", "220093")   # 44 bases
    # the frames are a width-4 box sum of the logits' softmax: each edge moves by at most two windows
    region_len = int(got["raw_end"]) - int(got["raw_start"])
    assert abs(int(got["raw_start"]) - 200_000) <= 4000 and abs(int(got["raw_end"]) - 220_000) <= 4000
    assert q_len == 4000 + region_len // 4


def test_constants():
    from jaeger_amd import _lib, attscan
    header = (ROOT / "include" / "jaeger_hip.h").read_text()
    defines = {name: int(value) for name, value in re.findall(r"^#define (JG_ALIGN\w*MAX) (\d+)\s*$", header, flags=re.M)}
    assert defines == {"JG_ALIGN_MAX": 6144, "JG_ALIGN_LONG_MAX": 24 * 512}
    assert (_lib.JG_ALIGN_MAX, _lib.JG_ALIGN_LONG_MAX) == (6144, defines["JG_ALIGN_LONG_MAX"])
    assert (attscan.ALIGN_MAX, attscan.ALIGN_LONG_MAX) == (_lib.JG_ALIGN_MAX, _lib.JG_ALIGN_LONG_MAX)
    assert _lib.SYMBOLS["jg_align_pairs_long"] == _lib.SYMBOLS["jg_align_pairs"]
