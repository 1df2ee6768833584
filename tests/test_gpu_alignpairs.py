"""``jg_align_pairs`` (the batched rectangular local alignment behind the att-site search) on the GPU: the fixed case
table against the CPU reference, the lengths at which the kernel's geometry changes against results known by
construction, the refused calls, the terminal-repeat kernel on the same spans, and the prophage report end to end."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

ROW_CLASSES = (1, 2, 4, 8, 16, 24)           # rows per thread of the kernel's instantiations; 256 threads per job
ALIGN_MAX = 6144


@pytest.fixture(scope="module")
def dev():
    from jaeger_amd.engine import HipDevice
    d = HipDevice(0)
    yield d
    d.close()


class _Buffer:
    """A compact base buffer with a little junk in front of and between the spans (so that no span starts at 0)."""

    def __init__(self):
        self.parts, self.at, self.rows = [b"TTGACA"], 6, []

    def add(self, q: str, r: str, flags: int):
        qb, rb = q.encode("latin-1"), r.encode("latin-1")
        self.rows.append((self.at, self.at + len(qb) + 3, len(qb), len(rb), flags))
        self.parts += [qb, b"GAT", rb, b"C"]
        self.at += len(qb) + 3 + len(rb) + 1

    def run(self, dev):
        from jaeger_amd import attscan
        return attscan.align_pairs(dev, np.frombuffer(b"".join(self.parts), np.uint8), attscan.make_jobs(self.rows))


def test_case_table_against_the_cpu_reference(dev):
    """Every case of tests/alignpairs_cases.py in ONE call (jobs of the row classes 1, 2 and 4 interleaved, spans at
    non-zero offsets, direct and reverse-complemented): all seven numbers equal the reference's; a case whose reference
    traceback met a tie is compared on score and end cell only."""
    import alignpairs_cases as cases
    import alignpairs_reference as ref
    table = cases.all_cases()
    buf = _Buffer()
    for _, q, r, rev in table:
        buf.add(q, r, 1 if rev else 0)
    assert {len(q) > 256 for _, q, _, _ in table} == {False, True} and max(len(q) for _, q, _, _ in table) > 512
    got = buf.run(dev)
    for (name, q, r, rev), row in zip(table, got.tolist()):
        a = ref.align(q, ref.reverse_complement(r) if rev else r)
        want = ref.result_row(a)
        if a["tied"]:
            assert (row[0], row[5], row[6], row[7]) == (want[0], want[5], want[6], 0), name
        else:
            assert row == want, name


def _planted(rng, q_len: int, r_len: int, L: int, q_at: int, r_at: int, q_drop: int = 0, r_drop: int = 0):
    """Random query / reference of exactly ``q_len`` / ``r_len`` bases sharing ONE repeat of ``L`` bases (fenced by N in the
    query so that it is exactly L long), the query's copy starting at ``q_at``, the reference's at ``r_at``;
    ``q_drop`` / ``r_drop`` bases are cut out of the middle of the query's / the reference's copy.  -> (q, r, row)."""
    from alignpairs_cases import rand_seq
    rep = rand_seq(rng, L)
    q_rep = rep[:L // 2] + rep[L // 2 + q_drop:]
    r_rep = rep[:L // 2] + rep[L // 2 + r_drop:]
    q = rand_seq(rng, q_at - 1) + "N" + q_rep + "N"
    q += rand_seq(rng, q_len - len(q))
    r = rand_seq(rng, r_at) + r_rep
    r += rand_seq(rng, r_len - len(r))
    assert len(q) == q_len and len(r) == r_len
    drop = q_drop + r_drop
    score = 2 * (L - drop) - (100 + 5 * (drop - 1) if drop else 0)
    row = [score, L, q_drop, r_drop, L - drop, q_at + len(q_rep) - 1, r_at + len(r_rep) - 1, 0]
    return q, r, row


def test_lengths_where_the_geometry_changes(dev):
    """q_len 1, 255, 256, 257, every class boundary 256 R and 256 R + 1, 6 144; r_len 1; 300 x 6 144 and 6 144 x 300;
    6 144 x 6 144.  Expectations by construction: ONE planted repeat of L bases in random background scores 2 L (a gap of
    k bases inside it: minus 100 + 5 (k - 1)) with known counts and end cell - the background's chance matches (at most
    ~20 bases in 6 144 x 6 144) stay far below.  Every repeat is longer than a thread's strip, so it crosses strip
    boundaries; the two gapped jobs (one gap in each row, above 600 bases) tell the two gap counts apart."""
    rng = np.random.Generator(np.random.PCG64(61440))
    buf, want, names = _Buffer(), [], []

    def add(name, q, r, row, flags=0):
        buf.add(q, r, flags)
        want.append(row)
        names.append(name)

    # one row / one column: the first matching letter in (column, row) order
    add("q1", "g", "TTNCAGTG", [2, 1, 0, 0, 1, 0, 5, 0])
    add("r1", "TTNCAtGA", "A", [2, 1, 0, 0, 1, 4, 0, 0])
    add("q1_nothing", "N", "ACGTN", [0, 0, 0, 0, 0, -1, -1, 0])
    for q_len in (255, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, ALIGN_MAX):
        L = 70
        add(f"q{q_len}_tail", *_planted(rng, q_len, 150, L, q_len - L - 1, 40))        # ends in the last row but one
        add(f"q{q_len}_head", *_planted(rng, q_len, 97, L, 1, 20))
    add("300x6144", *_planted(rng, 300, ALIGN_MAX, 90, 150, ALIGN_MAX - 90))            # ends in the last column
    add("6144x300", *_planted(rng, ALIGN_MAX, 300, 90, 3000, 5))
    add("6144x6144", *_planted(rng, ALIGN_MAX, ALIGN_MAX, 130, 6000, 77))
    add("query_gap", *_planted(rng, 4500, 700, 161, 2100, 300, q_drop=1))
    add("ref_gap3", *_planted(rng, 700, 5000, 170, 310, 4100, r_drop=3))
    # a reverse-complemented reference above 600: the repeat sits mirrored in the span
    from alignpairs_reference import reverse_complement
    q, r, row = _planted(rng, 1500, 900, 120, 700, 100)
    add("revcomp_1500x900", q, reverse_complement(r), row, flags=1)
    got = buf.run(dev)
    for name, g, w in zip(names, got.tolist(), want):
        assert g == w, name


def test_refused_calls_and_the_empty_call(dev):
    """A length above JG_ALIGN_MAX (or 0), a span past n_bases and n_jobs = 0 come back before anything is launched: the
    result rows keep their sentinel."""
    from jaeger_amd import _lib as L
    from jaeger_amd import attscan
    bases = np.frombuffer(b"ACGT" * 2000, np.uint8).copy()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(rows, n_bases=None):
        jobs = attscan.make_jobs(rows)
        res = np.full((max(len(rows), 1), 8), -7, np.int32)
        rc = dev.lib.jg_align_pairs(dev.handle, ptr(bases), bases.size if n_bases is None else n_bases, L.JG_PTR_HOST,
                                    ptr(jobs), len(rows), ptr(res))
        assert (res == -7).all()
        return rc

    good = (0, 100, 50, 60, 0)
    assert call([good, (0, 0, ALIGN_MAX + 1, 10, 0)]) == L.JG_ERR_UNSUPPORTED
    assert call([good, (0, 0, 10, ALIGN_MAX + 1, 0)]) == L.JG_ERR_UNSUPPORTED
    assert call([(0, 0, 0, 10, 0)]) == L.JG_ERR_UNSUPPORTED
    assert call([good, (7990, 0, 11, 10, 0)]) == L.JG_ERR_INVALID
    assert call([good, (0, 7000, 10, 1001, 1)]) == L.JG_ERR_INVALID
    assert call([(-1, 0, 10, 10, 0)]) == L.JG_ERR_INVALID
    assert call([good], n_bases=150) == L.JG_ERR_INVALID
    assert call([]) == L.JG_OK
    assert dev.lib.jg_align_pairs(dev.handle, None, 0, L.JG_PTR_HOST, None, 0, None) == L.JG_OK
    with pytest.raises(L.JaegerHipError, match="6145|6144"):
        attscan.align_pairs(dev, bases, attscan.make_jobs([(0, 0, ALIGN_MAX + 1, 10, 0)]))
    assert attscan.align_pairs(dev, bases, attscan.make_jobs([])).shape == (0, 8)


def test_square_jobs_equal_the_terminal_repeat_kernel(dev):
    """The same spans through both kernels: jobs cut from contig ends give the score, columns, query gaps and end cell
    jg_terminal_repeats reports with JG_OPT_TERMINI_EXACT."""
    from alignpairs_cases import rand_seq
    from alignpairs_reference import reverse_complement
    from jaeger_amd import _lib as L
    from jaeger_amd import attscan
    from jaeger_amd import fragment as frag
    from jaeger_amd.termini import terminal_repeat_table
    rng = np.random.Generator(np.random.PCG64(808))
    seqs = []
    for n, L_rep, kind in ((900, 0, "none"), (3000, 70, "dtr"), (12_000, 130, "dtr_gap"), (30_000, 160, "itr"),
                           (101_000, 300, "dtr"), (2500, 20, "itr")):
        s, scan = rand_seq(rng, n), min(max(int(n * 0.04), 400), 4000)
        rep = rand_seq(rng, L_rep)
        tail = {"none": "", "dtr": rep, "dtr_gap": rep[:60] + rep[62:], "itr": reverse_complement(rep)}[kind]
        a, b = scan // 3, n - scan + scan // 2
        s = s[:a] + rep + s[a + len(rep):b] + tail + s[b + len(tail):]
        s = s[:5] + s[5:9].lower() + s[9:]
        seqs.append(s.encode())
    bases, offsets = frag.concat_records(seqs)
    fa = frag.FastaBatch([f"r{i}" for i in range(len(seqs))], bases, offsets)
    L.check(dev.lib.jg_engine_set_option(dev.handle, L.JG_OPT_TERMINI_EXACT, 1))
    try:
        term = terminal_repeat_table(dev, fa, 500)
    finally:
        L.check(dev.lib.jg_engine_set_option(dev.handle, L.JG_OPT_TERMINI_EXACT, 0))
    rows = []
    for k, s in enumerate(seqs):
        n = len(s)
        scan = min(min(max(int(n * 0.04), 400), 4000), n)
        for flags in (0, 1):
            rows.append((int(offsets[k]), int(offsets[k + 1]) - scan, scan, scan, flags))
    got = attscan.align_pairs(dev, bases, attscan.make_jobs(rows)).reshape(len(seqs), 2, 8)
    assert (term[:, 0] > 100).sum() >= 3 and (term[:, 5] > 100).sum() >= 1
    for k in range(len(seqs)):
        for h in range(2):
            assert got[k, h, [0, 1, 2, 5, 6]].tolist() == term[k, 5 * h:5 * h + 5].tolist(), (k, h)
    assert got[2, 0, 3] == 2                   # the two bases missing at the contig's end: reference-row gaps


def _genome():
    """Two synthetic contigs (seeded): 520 kb with a 30 kb island at 200 000 .. 230 000 and a 40-base DIRECT repeat at its
    borders, 505 kb with an 8 kb island at 100 000 .. 108 000 and a 36-base INVERTED repeat at its borders; frames whose
    phage track is high over the islands (2 000-base windows, stride = window)."""
    import pandas as pd
    from alignpairs_cases import rand_seq
    from alignpairs_reference import reverse_complement
    rng = np.random.Generator(np.random.PCG64(520))
    att, inv = rand_seq(rng, 40), rand_seq(rng, 36)
    one = rand_seq(rng, 520_000)
    one = one[:199_900] + "N" + att + "N" + one[199_942:230_050] + att + one[230_090:]
    two = rand_seq(rng, 505_000)
    two = two[:99_000] + "N" + inv + "N" + two[99_038:108_700] + reverse_complement(inv) + two[108_736:]
    assert (len(one), len(two)) == (520_000, 505_000)
    frames = {}
    for name, seq, (a, b) in (("one", one, (100, 115)), ("two", two, (50, 54))):
        track = rng.normal(0.3, 0.05, len(seq) // 2000)
        track[a:b] += 3.0
        frames[name] = [pd.DataFrame({"phage": track}), "bacteria", len(seq)]
    return [("one", one), ("two", two)], frames, att, inv


def test_report_end_to_end_through_the_device(dev, tmp_path):
    """``segment`` over synthetic frames, then the report with the real device: the TSV is the one the same code writes
    with the CPU reference in the device's place, and its two rows carry the planted attL / attR."""
    import alignpairs_reference as ref
    from jaeger_amd import attscan
    from jaeger_amd.prophage_report import prophage_report
    from jaeger_amd.prophage_segment import segment
    records, frames, att, inv = _genome()
    cord = segment(frames, cutoff_length=500_000, sensitivity=1.5)
    assert np.asarray(cord["one"][0]).tolist() == [[100, 115]] and np.asarray(cord["two"][0]).tolist() == [[50, 54]]
    cords = [cord[name] for name, _ in records]
    calls = []

    def on_device(bases, jobs):
        calls.append((len(bases), len(jobs)))
        return attscan.align_pairs(dev, bases, jobs)

    (tmp_path / "gpu").mkdir()
    (tmp_path / "cpu").mkdir()
    got = prophage_report(2000, records, cords, tmp_path / "gpu", on_device).read_text()
    want = prophage_report(2000, records, cords, tmp_path / "cpu", ref.align_jobs).read_text()
    assert calls == [(4 * 6000, 4)]                          # one call, a buffer of nothing but the four flanks
    assert got == want
    head, *rows = (line.split("\t") for line in got.splitlines())
    one, two = (dict(zip(head, row)) for row in rows)
    assert (one["att_type"], one["attL"], one["attR"], one["sstart"], one["eend"]) == ("DTR", att, att, "199901", "230089")
    assert (two["att_type"], two["attL"], two["attR"]) == ("ITR", inv, inv)
    assert (two["sstart"], two["send"], two["estart"], two["eend"]) == ("99001", "99037", "108700", "108736")
