"""``prophages_jaeger.tsv`` (``jaeger_amd.prophage_report``) against the reference's own ``prophage_report`` run over
recorded contigs, regions and alignments (tests/golden/prophage_report.json, made by
tests/golden/make_golden_prophage_report.py), and the wiring behind ``-p`` when no contig has a region."""
import json
import logging
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"


def _contig(rec) -> str:
    out = bytearray(b"N" * rec["length"])
    for start, text in rec["pieces"]:
        out[start:start + len(text)] = text.encode()
    return out.decode()


@pytest.fixture(scope="module")
def runs():
    gold = json.loads((GOLDEN / "prophage_report.json").read_text())
    for run in gold:
        run["records"] = [(c["name"], _contig(c)) for c in run["contigs"]]
    return gold


def _replayed(run, log):
    """The device call's stand-in: answers the jobs with the recorded alignments, in the reference's call order (per
    region direct, then reverse-complemented), and checks that the jobs are the reference's flanks."""
    def align(bases, jobs):
        log.append(len(jobs))
        want = run["alignments"]
        assert len(jobs) == len(want)
        assert int(jobs["q_off"][0]) == 0 and len(bases) == sum(int(j["q_len"]) + int(j["r_len"]) for j in jobs[::2])
        for k, (job, rec) in enumerate(zip(jobs, want)):
            assert (int(job["q_len"]), int(job["r_len"]), int(job["flags"])) == (rec["q_len"], rec["r_len"], k % 2), k
            assert int(job["r_off"]) == int(job["q_off"]) + int(job["q_len"])
        return np.array([rec["row"] for rec in want], np.int32)
    return align


def test_report_equals_the_reference_text(runs, tmp_path):
    """DTR chosen, ITR chosen, neither, LTR_DTR with a gap, a region at the contig's start (search_start clamped to 0),
    region_len // 2 on both sides of 14 000, a zero-width region, an empty flank (no job), a contig at or below the length
    limit, a contig without regions, a name holding ``___``: the TSV text is the reference's, byte for byte - float
    formatting of the columns that hold None included.  One device call per report."""
    from jaeger_amd.prophage_report import prophage_report
    kinds = set()
    for k, run in enumerate(runs):
        out = tmp_path / f"run{k}"
        out.mkdir()
        log = []
        path = prophage_report(run["fsize"], run["records"], run["cords"], out, _replayed(run, log), stride=run["stride"])
        assert path == out / "prophages_jaeger.tsv" and log == [len(run["alignments"])]
        text = path.read_text()
        assert text == run["tsv"]
        kinds |= {line.split("\t")[15] for line in text.splitlines()[1:]}
    assert kinds == {"DTR", "ITR", "LTR_DTR", ""}


def test_report_without_regions_calls_nothing_and_writes_nothing(runs, tmp_path):
    from jaeger_amd.prophage_report import prophage_report

    def align(bases, jobs):
        raise AssertionError("device called")

    run = runs[1]
    assert prophage_report(2000, run["records"], [None, [[], []]], tmp_path, align) is None
    assert prophage_report(2000, run["records"], run["cords"], tmp_path, align, min_len=600_000) is None
    assert list(tmp_path.iterdir()) == []


def test_min_len_lets_small_contigs_through(tmp_path):
    """The reference's hard-coded 500 000 is the default of ``min_len``; below it a 9 kb contig with a planted direct
    repeat goes through the same code (scan length 400 = max(int(0.04 len), 400))."""
    import sys
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    import alignpairs_reference as ref
    from alignpairs_cases import rand_seq
    from jaeger_amd.prophage_report import prophage_report
    rng = np.random.Generator(np.random.PCG64(12))
    rep = rand_seq(rng, 31)
    seq = rand_seq(rng, 9000)
    seq = seq[:2890] + "N" + rep + "N" + seq[2923:6100] + rep + seq[6131:]
    assert len(seq) == 9000
    cords = [[np.array([[3, 6]]), np.array([2.5])]]
    assert prophage_report(1000, [("small", seq)], cords, tmp_path, ref.align_jobs) is None        # default limit
    path = prophage_report(1000, [("small", seq)], cords, tmp_path, ref.align_jobs, min_len=5000)
    head, row = (line.split("\t") for line in path.read_text().splitlines())
    got = dict(zip(head, row))
    assert (got["att_type"], got["attL"], got["attR"], got["sstart"], got["eend"]) == ("DTR", rep, rep, "2891", "6130")
    assert (got["raw_start"], got["raw_end"], got["att_score"]) == ("3000", "6000", "62")


def test_side_outputs_without_regions(tmp_path, monkeypatch, caplog):
    """``_write_side_outputs`` with ``-p`` on contigs whose phage track is flat: the segmentation-input ``.npz`` is what it
    always was, no device is touched (the run's engine is a stand-in without any entry point) and no TSV appears."""
    from jaeger_amd import predict
    from jaeger_amd.prophage_inputs import logits_to_df_v2
    rng = np.random.Generator(np.random.PCG64(77))
    lens = [7000, 2400, 6500]
    fasta = tmp_path / "in.fasta"
    names = ["c0", "c1", "c2"]
    seqs = ["".join(rng.choice(list("ACGT"), n)) for n in lens]
    fasta.write_text("".join(f">{n} x\n{s}\n" for n, s in zip(names, seqs)))
    n_win = [7, 2, 6]
    data_full = {"headers": np.array(names), "lengths": np.array(lens),
                 "predictions": [np.tile(np.array([[2.0, -1.0, 0.0]], np.float32), (k, 1)) for k in n_win],
                 "gc_skews": [rng.normal(0, 0.1, k) for k in n_win], "gcs": [rng.uniform(0.4, 0.6, k) for k in n_win]}
    class_map = {"class": ["bacteria", "phage", "eukarya"], "index": [0, 1, 2]}
    opt = {"prophage": True, "lc": 5000, "fsize": 1000, "stride": 1000, "sensitivity": 1.5}
    plan = SimpleNamespace(options=opt, out_dir=tmp_path, file_base="in", input_path=fasta, fsize=1000, local_rank=0)
    res = SimpleNamespace(class_map=class_map, engine=object(), y_pred=None)
    with caplog.at_level(logging.INFO, logger="Jaeger"):
        predict._write_side_outputs(plan, res, data_full)
    pro = tmp_path / "in_prophages"
    assert sorted(p.name for p in pro.iterdir()) == ["in_segmentation_inputs.npz"]
    got = np.load(pro / "in_segmentation_inputs.npz", allow_pickle=True)
    frames = logits_to_df_v2(class_map=class_map, cmdline_kwargs=opt, headers=np.array(names),
                             predictions=data_full["predictions"], lengths=data_full["lengths"],
                             gc_skews=data_full["gc_skews"], gcs=data_full["gcs"])
    assert list(got["contigs"]) == ["c0", "c2"] == list(frames)
    assert sorted(got.files) == ["columns", "contigs", "hosts", "lengths", "tracks"]
    for a, key in zip(got["tracks"], frames):
        np.testing.assert_array_equal(a, frames[key][0].to_numpy(np.float64))
    messages = [r.getMessage() for r in caplog.records]
    assert "identifying prophages" in messages and "no prophage regions found" in messages
    assert not any("error" in m for m in messages)


def test_side_outputs_with_a_region(tmp_path, monkeypatch, caplog):
    """``-p`` behind the tables when a contig HAS a region: the third record of the file (520 kb, between shorter ones) is
    found by record number, only it is read again from the input (as written: lower case kept), its flanks go through ONE
    alignment call and the TSV carries the planted att site.  The device call is replaced by the CPU reference; the run's
    engine is a stand-in that only hands out its device."""
    import sys
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    import alignpairs_reference as ref
    from alignpairs_cases import rand_seq
    from jaeger_amd import attscan, predict
    rng = np.random.Generator(np.random.PCG64(2024))
    att = rand_seq(rng, 44)
    att = att[:10] + att[10:20].lower() + att[20:]
    big = rand_seq(rng, 520_000)
    big = big[:199_900] + "N" + att + "N" + big[199_946:230_050] + att.upper() + big[230_094:]
    seqs = {"s0": rand_seq(rng, 3000), "s1": rand_seq(rng, 2500), "big one": big, "s3": rand_seq(rng, 4000)}
    fasta = tmp_path / "in.fasta"
    fasta.write_text("".join(f">{n}\n" + "\n".join(s[i:i + 80] for i in range(0, len(s), 80)) + "\n" for n, s in seqs.items()))
    names = ["s0", "s1", "big", "s3"]                       # the ingest keeps a header's first token
    lens = [len(s) for s in seqs.values()]
    n_win = [max(n // 2000, 1) for n in lens]
    preds = [np.tile(np.array([[3.0, -3.0, 0.0]], np.float32), (k, 1)) for k in n_win]
    preds[2][100:115] = [-3.0, 3.0, 0.0]                    # phage over 200 000 .. 230 000
    data_full = {"headers": np.array(names), "lengths": np.array(lens), "predictions": preds,
                 "gc_skews": [rng.normal(0, 0.1, k) for k in n_win], "gcs": [rng.uniform(0.4, 0.6, k) for k in n_win]}
    class_map = {"class": ["bacteria", "phage", "eukarya"], "index": [0, 1, 2]}
    opt = {"prophage": True, "lc": 500_000, "fsize": 2000, "stride": 2000, "sensitivity": 1.5}
    plan = SimpleNamespace(options=opt, out_dir=tmp_path, file_base="in", input_path=fasta, fsize=2000, local_rank=0)
    device = object()
    res = SimpleNamespace(class_map=class_map, engine=SimpleNamespace(device=device), y_pred=None)
    calls = []

    def fake(dev, bases, jobs):
        assert dev is device
        calls.append((len(bases), len(jobs)))
        return ref.align_jobs(bases, jobs)

    monkeypatch.setattr(attscan, "align_pairs", fake)
    with caplog.at_level(logging.INFO, logger="Jaeger"):
        predict._write_side_outputs(plan, res, data_full)
    messages = [r.getMessage() for r in caplog.records]
    assert not any("error" in m for m in messages), messages
    pro = tmp_path / "in_prophages"
    assert sorted(p.name for p in pro.iterdir()) == ["in_segmentation_inputs.npz", "prophages_jaeger.tsv"]
    assert calls == [(2 * 6000, 2)]
    assert f"prophage cordinates saved at {pro / 'prophages_jaeger.tsv'}" in messages
    head, *rows = (line.split("\t") for line in (pro / "prophages_jaeger.tsv").read_text().splitlines())
    assert len(rows) == 1
    got = dict(zip(head, rows[0]))
    assert (got["contig_id"], got["seq_len"], got["att_type"], got["attL"], got["attR"]) == ("big", "520000", "DTR", att, att.upper())
    assert (got["sstart"], got["send"], got["estart"], got["eend"]) == ("199901", "199944", "230050", "230093")
    assert (got["att_identities"], got["att_score"]) == ("44", "88")
    # the frames are the logits' softmax under a width-4 box sum: the island's edges move by at most two windows
    assert abs(int(got["raw_start"]) - 200_000) <= 4000 and abs(int(got["raw_end"]) - 230_000) <= 4000
