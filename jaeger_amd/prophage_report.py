"""``prophages_jaeger.tsv``: att-site search at the boundaries of the prophage regions and the report
(``postprocess/prophages.py:605-703`` ``get_prophage_alignment_summary``, ``:706-873`` ``prophage_report`` with
``refined_boundaries=None`` - gene-based boundary refinement is not built, so ``sstart`` / ``eend`` of a region without
repeat are the raw window boundaries and ``raw_start`` / ``raw_end`` repeat them).

Per region the reference aligns the flank left of it (``scan_length`` bases outside, ``off_set`` inside) against the flank
right of it with parasail, direct and reverse-complemented.  Here the flanks of ALL regions of ALL contigs are copied into
one compact buffer and go through ONE device call (:func:`jaeger_amd.attscan.align_flanks`: ``jg_align_pairs`` when no
flank exceeds 6 144 bases, else ``jg_align_pairs_long``, which takes 12 288 - a flank is at most 4 000 + 6 999 = 10 999);
the aligned strings of the chosen orientation are rebuilt on the host from the device's counts.  Which of several
co-optimal alignments parasail reports is unpinned.
"""

from __future__ import annotations

import logging
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pandas as pd

from . import attscan

logger = logging.getLogger("Jaeger")

LTR_CUTOFF = 250


def calculate_gc_content(sequence: str) -> float:
    """helpers.py:710-723: upper-case G and C over the characters as read."""
    return (sequence.count("G") + sequence.count("C")) / len(sequence)


def calculate_percentage_of_n(sequence: str) -> float:
    """helpers.py:726-739."""
    return sequence.count("N") / len(sequence)


def get_prophage_alignment_summary(result_object, seq_len, record, cordinates, phage_score, type_="DTR") -> dict:
    """prophages.py:605-703.  ``result_object``: None (no repeat) or an object with ``score``, ``end_query``, ``end_ref``
    and ``traceback.query`` / ``.ref`` / ``.comp``."""
    if result_object is None:
        s_alig_start = cordinates["start"][0]
        e_alig_end = cordinates["end"][0]
        sequence = record[1][s_alig_start:e_alig_end]
        gc_ = calculate_gc_content(sequence)
        return {
            "contig_id": record[0], "seq_len": seq_len, "region_len": e_alig_end - s_alig_start, "phage_score": phage_score,
            "n%": None, "gc%": gc_, "reject": None, "sstart": s_alig_start, "send": None, "estart": None,
            "eend": e_alig_end, "att_alignment_length": None, "att_identities": None, "att_identity": None,
            "att_score": None, "att_type": None, "att_fgaps": None, "att_rgaps": None, "attL": None, "attR": None,
        }
    alig_len = len(result_object.traceback.query)
    f_gaps = result_object.traceback.query.count("-")
    rc_gaps = result_object.traceback.ref.count("-")
    iden = result_object.traceback.comp.count("|")
    if type_ == "ITR":
        s_alig_end = cordinates["start"][0] + result_object.end_query + 1
        s_alig_start = s_alig_end - alig_len
        e_alig_start = cordinates["end"][1] - result_object.end_ref - 1
        e_alig_end = e_alig_start + alig_len
    elif type_ == "DTR":
        s_alig_end = cordinates["start"][0] + result_object.end_query
        s_alig_start = s_alig_end - alig_len + 1
        e_alig_end = cordinates["end"][0] + result_object.end_ref
        e_alig_start = e_alig_end - alig_len + 1
        if (s_alig_end - s_alig_start) >= LTR_CUTOFF:
            type_ = f"LTR_{type_}"
    sequence = record[1][s_alig_start:e_alig_end]
    percentage_of_n = calculate_percentage_of_n(sequence)
    gc_ = calculate_gc_content(sequence)
    return {
        "contig_id": record[0], "seq_len": seq_len, "region_len": e_alig_end - s_alig_start, "phage_score": phage_score,
        "n%": percentage_of_n, "gc%": gc_, "reject": percentage_of_n > 0.20, "sstart": s_alig_start, "send": s_alig_end,
        "estart": e_alig_start, "eend": e_alig_end, "att_alignment_length": alig_len, "att_identities": iden,
        "att_identity": round(iden / alig_len, 2), "att_score": result_object.score, "att_type": type_,
        "att_fgaps": f_gaps, "att_rgaps": rc_gaps, "attL": result_object.traceback.query,
        "attR": result_object.traceback.ref,
    }


def _result(query: str, ref: str, row):
    """A device result row as the object the summary reads (parasail's result: score, ends, traceback strings)."""
    tb = attscan.traceback(query, ref, row)
    return SimpleNamespace(score=tb["score"], end_query=tb["end_query"], end_ref=tb["end_ref"], saturated=False,
                           traceback=SimpleNamespace(query=tb["query"], ref=tb["ref"], comp=tb["comp"]))


def prophage_report(fsize: int, records, prophage_cordinates, outdir, align, stride: int | None = None,
                    min_len: int = 500_000):
    """``records``: (name, sequence as read) per contig; ``prophage_cordinates``: per contig - SAME position, contigs are
    matched by record number, not by name - ``[ranges, scores]`` of :func:`jaeger_amd.prophage_segment.segment` or None;
    ``align(bases, jobs) -> (n, 8)``: the device call (``attscan.align_flanks`` bound to a device) - called once, over a
    buffer that holds only the flanks, and not at all when no region has two non-empty flanks.  Contigs of at most
    ``min_len`` bases are skipped (the reference's hard-coded 500 000).  Writes ``outdir / "prophages_jaeger.tsv"`` when
    there is a row and returns its path, else None."""
    step = stride or fsize
    regions = []          # what the second pass needs, in report order
    parts, jobs, at = [], [], 0
    for rec_no, record in enumerate(records):
        seq_len = len(record[1])
        if not seq_len > min_len:
            continue
        entry = prophage_cordinates[rec_no] if rec_no < len(prophage_cordinates) else None
        cords, scores = entry if entry is not None else [[], []]
        if not (len(cords) > 0 and len(scores) > 0):
            continue
        for (start, end), j in zip(cords, scores):
            raw_start = int(start * step)                           # region spans [first window start, last window end]
            raw_end = int((end - 1) * step + fsize)
            region_len = raw_end - raw_start
            scan_length = min(max(int(seq_len * 0.04), 400), 4000)
            off_set = 2000 if region_len // 2 >= 14000 else region_len // 4
            search_start = max(raw_start - scan_length, 0)
            search_end = min(raw_end + scan_length, seq_len)
            left_seq = str(record[1][search_start:raw_start + off_set])
            right_seq = str(record[1][raw_end - off_set:search_end])
            reg = SimpleNamespace(record=record, seq_len=seq_len, score=j, raw_start=raw_start, raw_end=raw_end,
                                  off_set=off_set, search_start=search_start, search_end=search_end, left=left_seq,
                                  right=right_seq, job=-1)
            if left_seq and right_seq:
                # a guard the rule above cannot reach: scan_length <= 4 000, and off_set is region_len // 4 only while
                # region_len // 2 < 14 000, i.e. region_len <= 27 999 and off_set <= 6 999 (2 000 above) - a flank is at most
                # 4 000 + 6 999 = 10 999 bases, ALIGN_LONG_MAX is 12 288
                if max(len(left_seq), len(right_seq)) > attscan.ALIGN_LONG_MAX:
                    raise ValueError(f"{record[0]}: region {raw_start}..{raw_end} has flanks of {len(left_seq)} / "
                                     f"{len(right_seq)} bases, the alignment kernels take {attscan.ALIGN_LONG_MAX}")
                reg.job = len(jobs)
                for seq in (left_seq, right_seq):
                    parts.append(np.frombuffer(seq.encode("latin-1", "replace"), np.uint8))
                jobs.append((at, at + len(left_seq), len(left_seq), len(right_seq), 0))
                jobs.append((at, at + len(left_seq), len(left_seq), len(right_seq), attscan.REVCOMP))
                at += len(left_seq) + len(right_seq)
            regions.append(reg)
    rows = align(np.concatenate(parts), attscan.make_jobs(jobs)) if jobs else np.zeros((0, 8), np.int32)
    summaries = []
    for reg in regions:
        none_cords = {"start": [reg.raw_start, None], "end": [reg.raw_end, None]}
        att_cords = {"start": [reg.search_start, reg.search_start + reg.off_set],
                     "end": [reg.raw_end - reg.off_set, reg.search_end]}
        summary = None
        if reg.job >= 0:
            dtr, itr = rows[reg.job], rows[reg.job + 1]
            if itr[attscan.COLS] > 12 or dtr[attscan.COLS] > 12:
                if itr[attscan.SCORE] > dtr[attscan.SCORE]:
                    result = _result(reg.left, attscan.reverse_complement(reg.right), itr)
                    summary = get_prophage_alignment_summary(result, reg.seq_len, reg.record, att_cords, reg.score, "ITR")
                else:
                    result = _result(reg.left, reg.right, dtr)
                    summary = get_prophage_alignment_summary(result, reg.seq_len, reg.record, att_cords, reg.score, "DTR")
        if summary is None:                                          # an empty flank, or no repeat of more than 12 columns
            summary = get_prophage_alignment_summary(None, reg.seq_len, reg.record, none_cords, reg.score, None)
        summary["raw_start"] = reg.raw_start
        summary["raw_end"] = reg.raw_end
        summaries.append(summary)
    if not summaries:
        return None
    df = pd.DataFrame(summaries)
    df["contig_id"] = df["contig_id"].apply(lambda x: x.replace("___", ","))
    path = Path(outdir) / "prophages_jaeger.tsv"
    df.to_csv(path, sep="\t", index=False, float_format="%.3f")
    logger.info(f"prophage cordinates saved at {path}")
    return path
