"""``jg_align_pairs_long`` (flanks of up to 12 288 bases: the 512-thread instantiations of ``align_kernel``) on the GPU:
the lengths at which the 512-thread geometry changes against results known by construction, short jobs against
``jg_align_pairs`` row for row (alone and mixed with long ones), seeded long pairs against the CPU reference, the refused
calls, and the prophage report end to end over 9 000-base flanks."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

ROW_CLASSES = (1, 2, 4, 8, 16, 24)           # rows per thread of the instantiations; 512 threads per long job
ALIGN_MAX, ALIGN_LONG_MAX = 6144, 12288


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

    def add(self, q: str, r: str, flags: int = 0):
        qb, rb = q.encode("latin-1"), r.encode("latin-1")
        self.rows.append((self.at, self.at + len(qb) + 3, len(qb), len(rb), flags))
        self.parts += [qb, b"GAT", rb, b"C"]
        self.at += len(qb) + 3 + len(rb) + 1

    def run(self, dev, call):
        from jaeger_amd import attscan
        return call(dev, np.frombuffer(b"".join(self.parts), np.uint8), attscan.make_jobs(self.rows))


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
    assert len(q) == q_len and len(r) == r_len and q_at >= 1
    drop = q_drop + r_drop
    score = 2 * (L - drop) - (100 + 5 * (drop - 1) if drop else 0)
    row = [score, L, q_drop, r_drop, L - drop, q_at + len(q_rep) - 1, r_at + len(r_rep) - 1, 0]
    return q, r, row


def _long_jobs(rng):
    """Three jobs only the 512-thread kernels take, with rows known by construction: (q, r, flags, row)."""
    from alignpairs_reference import reverse_complement
    a = _planted(rng, 700, 6145, 80, 300, 6000)
    b = _planted(rng, 6150, 90, 75, 6000, 3)
    q, r, row = _planted(rng, 513, 6500, 100, 200, 77)
    return [(a[0], a[1], 0, a[2]), (b[0], b[1], 0, b[2]), (q, reverse_complement(r), 1, row)]


def test_lengths_where_the_512_thread_geometry_changes(dev):
    """Every class boundary 512 R and 512 R + 1 beside a 6 145-base reference (which alone sends the job to the 512-thread
    kernels), q_len 6 145 and 12 287, 12 288 x 150 ending in thread 511's strip, 1 x 6 145, 300 x 12 288 ending in the last
    column, 12 288 x 300, 12 288 x 12 288, one gap in each row and a reverse-complemented reference above 6 144.
    Expectations by construction: ONE planted, N-fenced repeat of L >= 70 bases in random background scores 2 L (a gap of
    k bases inside it: minus 100 + 5 (k - 1)) with known counts and end cell; the background's chance matches (about 15
    bases in 12 288 x 12 288) stay far below."""
    from alignpairs_cases import rand_seq
    from alignpairs_reference import reverse_complement
    from jaeger_amd import attscan
    rng = np.random.Generator(np.random.PCG64(12288))
    buf, want, names = _Buffer(), [], []

    def add(name, q, r, row, flags=0):
        buf.add(q, r, flags)
        want.append(row)
        names.append(name)

    L = 70
    for q_len in (512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193):
        add(f"q{q_len}_tail", *_planted(rng, q_len, ALIGN_MAX + 1, L, q_len - L - 1, 40))   # ends in the last row but one
        add(f"q{q_len}_head", *_planted(rng, q_len, ALIGN_MAX + 1, L, 1, 6000))
    for q_len in (ALIGN_MAX + 1, ALIGN_LONG_MAX - 1):
        add(f"q{q_len}_tail", *_planted(rng, q_len, 150, L, q_len - L - 1, 40))
        add(f"q{q_len}_head", *_planted(rng, q_len, 97, L, 1, 20))
    add("12288x150", *_planted(rng, ALIGN_LONG_MAX, 150, L, ALIGN_LONG_MAX - L - 1, 33))   # rows 12 217 .. 12 286
    add("1x6145", "g", "TTNCAGTG" + rand_seq(rng, ALIGN_MAX + 1 - 8), [2, 1, 0, 0, 1, 0, 5, 0])
    add("300x12288", *_planted(rng, 300, ALIGN_LONG_MAX, 90, 150, ALIGN_LONG_MAX - 90))    # ends in the last column
    add("12288x300", *_planted(rng, ALIGN_LONG_MAX, 300, 90, 9000, 5))
    add("12288x12288", *_planted(rng, ALIGN_LONG_MAX, ALIGN_LONG_MAX, 130, 12_100, 12_150))
    add("query_gap", *_planted(rng, 9000, 700, 161, 4200, 300, q_drop=1))
    add("ref_gap3", *_planted(rng, 700, 10_000, 170, 310, 8200, r_drop=3))
    q, r, row = _planted(rng, 1500, 7000, 120, 700, 5100)
    add("revcomp_1500x7000", q, reverse_complement(r), row, flags=1)
    assert all(max(job[2], job[3]) > ALIGN_MAX for job in buf.rows)
    got = buf.run(dev, attscan.align_pairs_long)
    for name, g, w in zip(names, got.tolist(), want):
        assert g == w, name


def test_short_jobs_get_the_rows_of_jg_align_pairs(dev):
    """Every case of tests/alignpairs_cases.py through ``jg_align_pairs_long`` and through ``jg_align_pairs``: the same
    rows, element for element.  Then the same cases in ONE call with three long jobs in between (first, in the middle,
    last): every row comes back where its job stood."""
    import alignpairs_cases as cases
    from jaeger_amd import attscan
    table = cases.all_cases()
    buf = _Buffer()
    for _, q, r, rev in table:
        buf.add(q, r, 1 if rev else 0)
    short = buf.run(dev, attscan.align_pairs)
    assert short.shape == (len(table), 8) and (short[:, 0] > 0).sum() > len(table) // 2
    np.testing.assert_array_equal(buf.run(dev, attscan.align_pairs_long), short)
    rng = np.random.Generator(np.random.PCG64(513))
    extra = _long_jobs(rng)
    where = {0: extra[0], len(table) // 2: extra[1], len(table): extra[2]}
    mixed, want = _Buffer(), []
    for k in range(len(table) + 1):
        if k in where:
            q, r, flags, row = where[k]
            mixed.add(q, r, flags)
            want.append(row)
        if k < len(table):
            _, q, r, rev = table[k]
            mixed.add(q, r, 1 if rev else 0)
            want.append(short[k].tolist())
    got = mixed.run(dev, attscan.align_pairs_long)
    assert len(want) == len(table) + 3
    for k, (g, w) in enumerate(zip(got.tolist(), want)):
        assert g == w, k


def _pair(seed: int, q_len: int, r_len: int, L: int, kind: str):
    """A seeded pair sharing one repeat of ``L`` bases, NOT fenced: the bases next to it are the random background's (a
    mismatch, or a chance match that lengthens the alignment), and the repeat itself carries a mismatch, a missing base in
    the query, or two missing bases in a reference that is read reverse-complemented.  -> (query, ref, revcomp)."""
    from alignpairs_cases import _mutate, rand_seq
    from alignpairs_reference import reverse_complement
    rng = np.random.Generator(np.random.PCG64(seed))
    rep = rand_seq(rng, L)
    q_rep = rep[:L // 2] + rep[L // 2 + 1:] if kind == "query_gap" else rep
    r_rep = {"mismatch": _mutate(rep, L // 2), "query_gap": rep, "ref_gap2_revcomp": rep[:L // 2] + rep[L // 2 + 2:]}[kind]
    q, r = rand_seq(rng, q_len - len(q_rep)), rand_seq(rng, r_len - len(r_rep))
    q_at, r_at = (2 * len(q)) // 3, len(r) // 2
    q = q[:q_at] + q_rep + q[q_at:]
    r = r[:r_at] + r_rep + r[r_at:]
    assert (len(q), len(r)) == (q_len, r_len)
    rev = kind == "ref_gap2_revcomp"
    return q, reverse_complement(r) if rev else r, rev


# seeds chosen with the CPU reference alone, so that at most one pair's reference traceback meets a tie
REFERENCE_PAIRS = ((7001, 7000, 6500, 150, "mismatch"), (6205, 6200, 6150, 160, "query_gap"),
                   (9003, 2000, 9000, 170, "ref_gap2_revcomp"))


def test_long_pairs_against_the_cpu_reference(dev):
    """Not by construction: the seven numbers of three seeded long pairs equal the CPU reference's (matrices over the
    alignment's box); a pair whose reference traceback met a tie is compared on score and end cell only - at most one of
    the three, by the helper's own flag."""
    import alignpairs_reference as ref
    from jaeger_amd import attscan
    pairs = [(f"{kind}_{q_len}x{r_len}", *_pair(seed, q_len, r_len, L, kind)) for seed, q_len, r_len, L, kind in REFERENCE_PAIRS]
    buf = _Buffer()
    for _, q, r, rev in pairs:
        buf.add(q, r, 1 if rev else 0)
    assert all(ALIGN_MAX < max(job[2], job[3]) <= ALIGN_LONG_MAX for job in buf.rows)
    got = buf.run(dev, attscan.align_pairs_long)
    tied = 0
    for (name, q, r, rev), row in zip(pairs, got.tolist()):
        a = ref.align(q, ref.reverse_complement(r) if rev else r, box_only=True)
        want = ref.result_row(a)
        assert want[0] > 150 and want[2] + want[3] + (want[1] - want[4]) >= 1, name     # the repeat, with its flaw inside
        tied += bool(a["tied"])
        if a["tied"]:
            assert (row[0], row[5], row[6], row[7]) == (want[0], want[5], want[6], 0), name
        else:
            assert row == want, name
    assert tied <= 1


def test_refused_calls_and_the_empty_call(dev):
    """A length above JG_ALIGN_LONG_MAX (or 0), a span past n_bases and n_jobs = 0 come back before anything is launched:
    the result rows keep their sentinel."""
    from jaeger_amd import _lib as L
    from jaeger_amd import attscan
    bases = np.frombuffer(b"ACGT" * 4000, np.uint8).copy()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(rows, n_bases=None):
        jobs = attscan.make_jobs(rows)
        res = np.full((max(len(rows), 1), 8), -7, np.int32)
        rc = dev.lib.jg_align_pairs_long(dev.handle, ptr(bases), bases.size if n_bases is None else n_bases, L.JG_PTR_HOST,
                                         ptr(jobs), len(rows), ptr(res))
        assert (res == -7).all()
        return rc

    good = (0, 100, 50, 7000, 0)
    assert call([good, (0, 0, ALIGN_LONG_MAX + 1, 10, 0)]) == L.JG_ERR_UNSUPPORTED
    assert call([good, (0, 0, 10, ALIGN_LONG_MAX + 1, 0)]) == L.JG_ERR_UNSUPPORTED
    assert call([(0, 0, 0, 10, 0)]) == L.JG_ERR_UNSUPPORTED
    assert call([(0, 0, 10, 0, 0)]) == L.JG_ERR_UNSUPPORTED
    assert call([good, (15_990, 0, 11, 10, 0)]) == L.JG_ERR_INVALID
    assert call([good, (0, 9000, 10, 7001, 1)]) == L.JG_ERR_INVALID
    assert call([(-1, 0, 10, 10, 0)]) == L.JG_ERR_INVALID
    assert call([good], n_bases=7099) == L.JG_ERR_INVALID
    assert call([]) == L.JG_OK
    assert dev.lib.jg_align_pairs_long(dev.handle, None, 0, L.JG_PTR_HOST, None, 0, None) == L.JG_OK
    with pytest.raises(L.JaegerHipError, match="job 1 is 10 x 12289"):
        attscan.align_pairs_long(dev, bases, attscan.make_jobs([good, (0, 0, 10, ALIGN_LONG_MAX + 1, 0)]))
    assert attscan.align_pairs_long(dev, bases, attscan.make_jobs([])).shape == (0, 8)


def _genome():
    """A synthetic contig (seeded) of 520 kb with a 20 kb island at 200 000 .. 220 000 and a 40-base direct repeat at its
    borders; a frame whose phage track is high over the island (2 000-base windows, stride = window)."""
    import pandas as pd
    from alignpairs_cases import rand_seq
    rng = np.random.Generator(np.random.PCG64(20520))
    att = rand_seq(rng, 40)
    one = rand_seq(rng, 520_000)
    one = one[:199_900] + "N" + att + "N" + one[199_942:220_050] + att + one[220_090:]
    assert len(one) == 520_000
    track = rng.normal(0.3, 0.05, len(one) // 2000)
    track[100:110] += 3.0
    return [("one", one)], {"one": [pd.DataFrame({"phage": track}), "bacteria", len(one)]}, att


def test_report_end_to_end_over_9000_base_flanks(dev, tmp_path):
    """``segment`` over a synthetic frame, then the report through ``attscan.align_flanks`` on the device: region_len
    20 000, off_set 5 000, flanks of 9 000 - one call, and the TSV is the one the same code writes with the CPU reference in
    the device's place, with the planted attL / attR in its row."""
    import alignpairs_reference as ref
    from jaeger_amd import attscan
    from jaeger_amd.prophage_report import prophage_report
    from jaeger_amd.prophage_segment import segment
    records, frames, att = _genome()
    cord = segment(frames, cutoff_length=500_000, sensitivity=1.5)
    assert np.asarray(cord["one"][0]).tolist() == [[100, 110]]
    cords = [cord[name] for name, _ in records]
    calls = []

    def on_device(bases, jobs):
        calls.append((len(bases), len(jobs)))
        return attscan.align_flanks(dev, bases, jobs)

    (tmp_path / "gpu").mkdir()
    (tmp_path / "cpu").mkdir()
    got = prophage_report(2000, records, cords, tmp_path / "gpu", on_device).read_text()
    want = prophage_report(2000, records, cords, tmp_path / "cpu", ref.align_jobs).read_text()
    assert calls == [(2 * 9000, 2)]                          # one call, a buffer of nothing but the two flanks
    assert got == want
    head, *rows = (line.split("\t") for line in got.splitlines())
    assert len(rows) == 1
    one = dict(zip(head, rows[0]))
    assert (one["att_type"], one["attL"], one["attR"], one["sstart"], one["eend"]) == ("DTR", att, att, "199901", "220089")
