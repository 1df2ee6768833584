"""``jaeger predict`` orchestration on the MI355X engine.

Mirrors ``commands/predict.py:488-861`` (``run_core``) for the conv model family: model
discovery, FASTA validation, output layout ``<output>/<model_id>/<stem>.tsv``, two-pass
short-contig mode, auxiliary npz writers - with the tf.data pipeline
(``_build_prediction_dataset`` :186-245) and ``InferModel.predict`` replaced by one window
table + ``JaegerHipEngine.predict_windows`` call per pass.  Under ``torchrun`` (WORLD_SIZE > 1)
contigs are sharded over the ranks and gathered on rank 0 (RCCL): ``sharded.py``, imported on that path only.

``run_core`` is a list of stages: :func:`plan_run` (one :class:`RunPlan`), the prediction (``_predict_pipelined``,
``_predict_sequential`` or ``sharded.predict_sharded``: one :class:`RunResult`), the tables, the side outputs, the summary
line and the release behind the return.
"""

from __future__ import annotations

import json
import logging
import os
import sys
import threading
import time
import traceback
from collections import defaultdict
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any

import numpy as np

from . import fragment as frag

logger = logging.getLogger("Jaeger")


# ---- model registry (utils/misc.py:334-396) ------------------------------------------------
class AvailableModels:
    """Scan ``model/`` directories for ``<name>_graph/``, ``<name>_classes.yaml``,
    ``<name>_project.yaml`` and ``<name>.weights.h5`` / ``<name>.npz`` entries."""

    def __init__(self, path):
        self.paths = [Path(path)] if isinstance(path, (str, Path)) else [Path(p) for p in path]
        self.info = self._scan()

    def _scan(self):
        models: dict[str, dict] = defaultdict(dict)
        for path in self.paths:
            dirs = [p for p in path.rglob("model") if p.is_dir()]
            if path.name == "model" and path.is_dir():
                dirs.append(path)
            for d in dirs:
                for e in d.iterdir():
                    if e.is_dir() and e.name.endswith("_graph"):
                        models[e.name.removesuffix("_graph")]["graph"] = e
                    elif e.is_file():
                        name = e.name
                        if "_classes.yaml" in name:
                            key = "classes"
                        elif "_project.yaml" in name:
                            key = "project"
                        elif e.suffix == ".h5" and ".weights" in e.stem:
                            key = "weights"
                        elif e.suffix == ".npz" and ".weights" in e.stem:
                            key = "weights_npz"           # canonical weights for the MI355X engine
                        else:
                            continue
                        base = (name.replace("_classes.yaml", "").replace("_project.yaml", "")
                                .replace(".weights.h5", "").replace(".weights.npz", ""))
                        models[base][key] = e
        return models


def get_model_id(model: str) -> str:
    """utils/misc.py:395-396: ``jaeger_38341_1.4M_fragment`` -> ``38341_1.4M``."""
    return model.split("_", 1)[1].rsplit("_", 1)[0]


def validate_fasta_entries(path, min_len: int) -> int:
    """utils/fs.py:99-115: record count; raises when no record reaches ``min_len``.  ``path`` may be
    an already loaded :class:`~jaeger_amd.fragment.FastaBatch` (one ingest pass instead of three)."""
    fa = path if isinstance(path, frag.FastaBatch) else frag.load_fasta(path)
    num, ok = len(fa), int((fa.lengths >= min_len).sum())
    logger.info(f"{ok}/{num} entries in {'input' if isinstance(path, frag.FastaBatch) else path}")
    if ok == 0:
        raise Exception(f"all records in {'input' if isinstance(path, frag.FastaBatch) else path} are < {min_len}bp")
    return num


def get_logger(out_dir: Path, log_file: Path, level: int = 1) -> logging.Logger:
    """utils/logging.py:30-75: console + DEBUG file handler."""
    lg = logging.getLogger("Jaeger")
    lg.setLevel(logging.DEBUG)
    for h in list(lg.handlers):
        lg.removeHandler(h)
    ch = logging.StreamHandler(sys.stderr)
    ch.setLevel(logging.DEBUG if level and level > 1 else logging.INFO)
    ch.setFormatter(logging.Formatter("%(asctime)s %(levelname)-8s [jaeger] %(message)s", "%Y-%m-%d %H:%M:%S"))
    lg.addHandler(ch)
    fh = logging.FileHandler(out_dir / f"{time.strftime('%m%d%Y_%H%M%S')}_{log_file}")
    fh.setLevel(logging.DEBUG)
    fh.setFormatter(ch.formatter)
    lg.addHandler(fh)
    return lg


def _crop_length_warning(trained_codons, trained_nt, fsize: int) -> str | None:
    """commands/predict.py:36-63."""
    if trained_codons is not None:
        runtime = (int(fsize) - 5) // 3
        if runtime == trained_codons:
            return None
        hint = f" ({trained_nt} nt)" if trained_nt is not None else ""
        return (f"runtime --fsize {fsize} maps to {runtime} codon frames, but the model was trained on "
                f"{trained_codons} codons{hint}; prefer --fsize "
                f"{trained_nt if trained_nt is not None else 'used at training'} for this model.")
    if trained_nt is not None and int(fsize) != int(trained_nt):
        return (f"runtime --fsize {fsize} differs from the model's trained fragment length ({trained_nt} nt).")
    return None


def _concat_predictions(a: dict, b: dict) -> dict:
    """commands/predict.py:248-258."""
    if not a:
        return b
    if not b:
        return a
    return {k: np.concatenate([a[k], b[k]], axis=0) for k in a}


# ---- one prediction pass --------------------------------------------------------------------
def predict_batch(engine, fa: "frag.FastaBatch", fsize: int, stride: int | None, min_len: int | None = None,
                  max_len: int | None = None, dynamic_stride: bool = False,
                  dynamic_stride_threshold: float = 10.0, batch: int = 96, padded: bool = False,
                  subset=None, pre_cased: bool = False,
                  want=("prediction", "reliability", "embedding", "nmd"), meta: bool = True,
                  dust_device: bool = False) -> dict[str, np.ndarray]:
    """Window table + GPU encode/forward for the records of ``fa`` (optionally only those listed in
    ``subset``, kept in that order); returns the dict ``InferModel.predict`` would (model outputs +
    ``meta_0..9``).  ``padded`` reproduces ``padded_batch`` of the short-contig pass: windows run in
    groups of ``batch`` padded to the longest frame of the group (commands/predict.py:236-245).  ``dust_device``: the
    bases are DUST soft-masked on the GPU after their upload (the host buffer stays as read) instead of ``pre_cased``
    by :func:`jaeger_amd.fragment.dust_mask`."""
    idx = np.arange(len(fa)) if subset is None else np.asarray(subset, np.int64)
    lengths = fa.lengths[idx]
    names = [fa.names[i] for i in idx.tolist()] if subset is not None else fa.names
    table = frag.build_window_table(lengths, fsize, stride, dynamic_stride, dynamic_stride_threshold,
                                    min_len, max_len)
    if len(table) == 0:
        return {}
    starts = fa.offsets[idx][table.contig] + table.start
    if not padded:
        out = engine.predict_windows(fa.bases, starts, table.length, fsize, pre_cased=pre_cased, want=want,
                                     dust_records=fa.offsets if dust_device else None)
    else:
        # the short-contig pass: one whole-contig window per record.  The selected records are compacted into a
        # buffer of their own once, so that a batch of 96 windows uploads the few hundred kB it covers and not the
        # whole FASTA image (a 2 Gbp assembly with 1 M short contigs would otherwise move 2 GB per batch)
        # (compacted batch by batch, run by run: records are in FASTA order, so adjacent short records merge into one
        # slice copy - no per-base index array over every short contig of the assembly)
        wl = table.length.astype(np.int64)
        cstart = np.cumsum(wl) - wl
        off3 = (-2, -1, 0)[fsize % 3]
        parts = []
        for i in range(0, len(table), batch):
            sl = slice(i, i + batch)
            lmax = int(max(0, -(-(int(table.length[sl].max()) - 5 + off3) // 3)))
            if getattr(engine.model, "strands", 1) > 1:                       # nucleotide rows hold bases
                lmax = int(table.length[sl].max())
            elif getattr(engine.model, "wide_ids", False):                    # dicodon rows: codon pairs six bases apart
                lmax = int(max(0, -(-(int(table.length[sl].max()) - 8 + off3) // 6)))
            c0, c1 = int(cstart[i]), int(cstart[sl][-1] + wl[sl][-1])
            s_b, l_b = starts[sl], wl[sl]
            cut = np.nonzero(s_b[1:] != s_b[:-1] + l_b[:-1])[0] + 1          # where a new run of adjacent records starts
            run_a = s_b[np.concatenate(([0], cut))]
            run_b = (s_b + l_b)[np.concatenate((cut - 1, [len(s_b) - 1]))]
            compact = np.concatenate([fa.bases[x:y] for x, y in zip(run_a.tolist(), run_b.tolist())]) \
                if len(run_a) > 1 else fa.bases[int(run_a[0]):int(run_b[0])]
            # (every window of this pass is a whole record: the compact buffer's record table is its window table)
            recs = np.append(cstart[sl] - c0, c1 - c0) if dust_device else None
            parts.append(engine.predict_windows(compact, cstart[sl] - c0, table.length[sl], fsize,
                                                l_pad=max(lmax, 1), pre_cased=pre_cased, want=want, dust_records=recs))
        out = {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}
    if not meta:                       # sharded runs: rank 0 rebuilds the metadata from its own window table
        return out
    counts = out.pop("counts")
    out.update(frag.window_metadata(table, names, counts))
    return out


def predict_records(engine, names: list[str], seqs: list[bytes], fsize: int, stride: int | None, **kw):
    """:func:`predict_batch` for records given as Python lists."""
    bases, offsets = frag.concat_records(seqs)
    return predict_batch(engine, frag.FastaBatch(list(names), bases, offsets), fsize, stride, **kw)


class _LazyTableWriter:
    """``postprocess.TableWriter`` created at its first batch: pandas is then imported beside the forward, not in front of it."""

    def __init__(self, class_map: dict, table_path, phage_path, reliability_cutoff, phage_score):
        self._args = (class_map.get("class"), class_map.get("index"), table_path, phage_path)
        self._kw = dict(reliability_cutoff=reliability_cutoff, phage_score=phage_score)
        self.w = None

    def append(self, data: dict) -> None:
        if self.w is None:
            from .postprocess import TableWriter
            self.w = TableWriter(*self._args, **self._kw)
        self.w.append(data)

    def close(self) -> int:
        return self.w.close() if self.w is not None else 0

    def abort(self) -> None:
        if self.w is not None:
            self.w.abort()


class _Aggregator:
    """Per-contig aggregation of the long pass BESIDE the forward: ``advance(done)`` is called with the engine's progress
    mark (output rows of windows [0, done) are final, ``HipDevice.windows_done``) and runs ``pred_to_dict`` on the contigs
    whose windows are all below it, batch by batch; the reference aggregates after ``InferModel.predict`` has returned
    (commands/predict.py:846).  Per-contig statistics do not depend on which other contigs share a batch, so the merged
    result equals one ``pred_to_dict`` call over everything (tests/test_postprocess.py)."""

    def __init__(self, table: "frag.WindowTable", names: list[str], out: dict, pred_kw: dict, min_batch: int, workers: int = 1):
        self.table, self.out, self.kw = table, out, pred_kw
        # workers > 1 (round 6): batches are aggregated on a small pool - ``parts`` then holds futures, in batch order - so
        # that on files of very many short contigs the aggregation keeps pace with the forward (numpy and the native
        # reductions run without the interpreter lock); consumers take the batches in order whatever finished first
        self.pool = None
        if workers > 1:
            from concurrent.futures import ThreadPoolExecutor
            self.pool = ThreadPoolExecutor(max_workers=int(workers), thread_name_prefix="jaeger-agg")
        # names straight from the native parser (fragment.Names) that io.py:109's normalisation leaves as they are stay BYTES
        # from the FASTA image to the table rows; anything else goes through the per-record strings as before
        self._names = names
        self.names_bytes = names if isinstance(names, frag.Names) and names.plain() else None
        self._hdr = None
        n_rec = len(names)
        per_rec = np.bincount(table.contig, minlength=n_rec).astype(np.int64) if len(table) else np.zeros(n_rec, np.int64)
        self.ends = np.cumsum(per_rec[per_rec > 0])              # window index one past each contig's last window
        self.w_done = 0                                           # windows aggregated so far (always a contig boundary)
        self.min_batch = max(1, int(min_batch))
        self.parts: list = []
        self.busy_s = 0.0
        self.flushed = 0                                          # parts already handed to the table writer
        self._unique = None

    @property
    def hdr(self) -> np.ndarray:
        """The records' normalised names as an object array of Python strings (made when something needs them)."""
        if self._hdr is None:
            self._hdr = frag.normalise_headers(self._names)
        return self._hdr

    def advance(self, done: int, final: bool = False) -> None:
        if len(self.ends) == 0:
            return
        k = int(np.searchsorted(self.ends, done, side="right"))
        w1 = int(self.ends[k - 1]) if k else 0
        if w1 <= self.w_done or (not final and w1 - self.w_done < self.min_batch):
            return
        w0, self.w_done = self.w_done, w1
        if self.pool is not None:
            self.parts.append(self.pool.submit(self._batch, w0, w1))
        else:
            part = self._batch(w0, w1)
            if part is not None:
                self.parts.append(part)

    def _batch(self, w0: int, w1: int):
        """(data, data_full) of the contigs whose windows are [w0, w1), or None."""
        t0 = time.time()
        rec = self.table.contig[w0:w1]
        first = np.ones(len(rec), dtype=bool)
        first[1:] = rec[1:] != rec[:-1]
        part = self._aggregate(self.slice(w0, w1, with_names=self.names_bytes is None), np.asarray(rec[first], dtype=np.int64))
        self.busy_s += time.time() - t0
        return part

    def _part(self, i: int, wait: bool = True):
        """Batch ``i`` as (data, data_full) (None: an empty one); with ``wait`` False, the string "pending" while a worker
        still has it."""
        item = self.parts[i]
        if hasattr(item, "result"):
            if not wait and not item.done():
                return "pending"
            item = self.parts[i] = item.result()          # (a worker's exception surfaces here, in the consumer)
        return item

    def close(self) -> None:
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None

    def names_unique(self) -> bool:
        """No record name twice (then a join by record number IS the reference's merge on the name).  One hash pass over
        the names, made once - the polling loop calls it beside the forward."""
        if self._unique is None:
            if self.names_bytes is not None:
                self._unique = self.names_bytes.is_unique()          # (jg_names_unique: no Python strings)
            else:
                import pandas as pd
                self._unique = bool(pd.Index(self.hdr).is_unique)
        return self._unique

    def slice(self, w0: int, w1: int, with_names: bool = True) -> dict:
        """Engine outputs + window metadata of windows [w0, w1) in ``InferModel.predict``'s dict form (``with_names`` False:
        without the per-window header array ``meta_0`` - the batch's contig names travel as bytes)."""
        t = self.table
        sub = frag.WindowTable(*(getattr(t, f)[w0:w1] for f in ("contig", "start", "length", "is_last", "ordinal", "seqlen")))
        y = {k: v[w0:w1] for k, v in self.out.items() if k != "counts"}
        y.update(frag.window_metadata(sub, self.hdr if with_names else None, self.out["counts"][w0:w1], normalised=True))
        return y

    def add(self, y_pred: dict, records: np.ndarray | None = None) -> None:
        part = self._aggregate(y_pred, records)
        if part is not None:
            self.parts.append(part)

    def _aggregate(self, y_pred: dict, records: np.ndarray | None = None):
        from .postprocess import SpanColumn, _Summaries, pred_to_dict, window_letters
        if y_pred and len(y_pred["meta_2"]):
            kw = self.kw
            if y_pred.get("meta_0") is None:                       # names as bytes: one span per contig of the batch
                kw = dict(kw, headers=SpanColumn(*self.names_bytes.spans(records), facts=self.names_bytes.facts))
            data, full = pred_to_dict(y_pred, **kw)
            # the run-length strings of the batch's contigs belong beside the forward too: the library's text as it comes
            runs, letters = data["frag_pred"], window_letters(self.kw["class_map"])
            blob = runs.summaries_blob(letters)
            data["frag_pred"] = _Summaries(blob=blob, n=len(runs)) if blob is not None else _Summaries(runs.summaries(letters))
            if records is not None and len(records) == len(data["headers"]):
                data["record_index"] = records        # FASTA record of every contig of the batch: the repeat table joins by it
            return data, full
        return None

    def flush(self, writer, term_repeats, wait: bool = True) -> None:
        """Hand the batches aggregated so far to the table writer, in order (needs the repeat table: the left merge of
        collect.py:527-532 is part of a row).  ``wait`` False: stop at the first batch a worker has not finished."""
        t0 = time.time()
        while self.flushed < len(self.parts):
            part = self._part(self.flushed, wait)
            if part == "pending":
                break
            if part is None:
                self.flushed += 1
                continue
            data = part[0]
            data["repeats"] = term_repeats
            row_of = getattr(term_repeats, "row_of_record", None)
            if row_of is None and term_repeats is not None and hasattr(term_repeats, "attrs"):
                row_of = term_repeats.attrs.get("_row_of_record")
            if row_of is not None and "record_index" in data and len(row_of) == len(self._names):
                data["repeat_rows"] = row_of[data["record_index"]]
                data["names_unique"] = self.names_unique()
            writer.append(data)
            self.flushed += 1
        self.busy_s += time.time() - t0

    def result_full(self):
        from .postprocess import merge_data
        parts = [self._part(i) for i in range(len(self.parts))]
        return merge_data([p[1] for p in parts if p is not None])


# ---- what outlives a run_core call ------------------------------------------------------------------------
SHARD_STATS: dict = {}        # filled by the sharded path (sharded.py; tests read it): local / total bases of this rank
LAST_RUN: dict = {}           # stage split of the last single-GPU run_core of this process (bench.py's e2e leg reads it)
_PENDING_RELEASE: list = []   # threads still releasing a finished run's engine / host buffers


def wait_for_release(timeout: float | None = 60.0) -> None:
    """Join the background release of earlier ``run_core`` calls (device memory and pinned staging are back when this
    returns).  ``run_core`` calls it on entry, so two runs never overlap one's teardown with the other's forward."""
    while _PENDING_RELEASE:
        _PENDING_RELEASE.pop().join(timeout)


def _mark(name: str) -> None:
    """(event, seconds since run_core was entered) onto the run's timeline: where the wall time of a short run goes."""
    LAST_RUN["timeline"].append((name, round(time.time() - LAST_RUN["t_start_epoch"], 4)))


# ---- the run description ------------------------------------------------------------------------------------
@dataclass(frozen=True)
class RunPlan:
    """What one ``run_core`` call is to do: decided once by :func:`plan_run`, read by every stage on either path."""
    options: dict                   # the caller's keywords, for what one stage alone reads (engine options, side outputs)
    model_name: str
    model_info: dict
    model_id: str
    input_path: Path
    file_base: str
    out_dir: Path
    table_path: Path
    phage_path: Path
    fsize: int
    stride: int | None
    user_min_len: int | None
    min_len: int
    passes: tuple                   # (min_len, max_len, padded) per prediction pass, in the order their rows are reported
    want: tuple
    want_full: bool
    pred_kw: dict                   # pred_to_dict's keywords, but for class_map and term_repeats (known after the run)
    dust: str                       # "none" | "host" (fragment.dust_mask over the FASTA image) | "device" (in the fused calls)
    common: dict                    # predict_batch's keywords
    rank: int
    world: int
    local_rank: int
    sharded: bool
    piped: bool
    rc: float
    pc: int


def find_model(kwargs: dict) -> tuple[str, dict]:
    """(name, files) of the model to run: ``--model_path``'s first classification model, or ``--model`` under ``--config``."""
    model_path = kwargs.get("model_path")
    if model_path:
        info = AvailableModels(path=model_path).info
        if not info:
            print(f"No model found in {model_path}", file=sys.stderr)
            sys.exit(1)
        cands = {n: m for n, m in info.items() if m.get("project") is not None and m.get("classes") is not None}
        if not cands:
            print(f"No classification model found in {model_path}. Expected *_classes.yaml, *_project.yaml "
                  "and *.weights.h5 / *.weights.npz files.", file=sys.stderr)
            sys.exit(1)
        cands = {n: m for n, m in cands.items() if not n.endswith("_embedding")} or cands
        model_name = next(iter(cands))
        return model_name, cands[model_name]
    cfg_path = kwargs.get("config")
    if not cfg_path:
        print("jaeger_amd: pass --model_path <dir with model/> or --config <json with model_paths>", file=sys.stderr)
        sys.exit(1)
    paths = json.loads(Path(cfg_path).read_text()).get("model_paths", [])
    info = AvailableModels(path=paths).info
    model_name = kwargs.get("model")
    if model_name not in info:
        print(f"model {model_name!r} not found under {paths}", file=sys.stderr)
        sys.exit(1)
    return model_name, info[model_name]


def plan_run(kwargs: dict) -> RunPlan:
    """The run description from ``run_core``'s keywords and torchrun's environment."""
    # (makes the output directory and the run's logger on the way, and refuses - exit 1 - what this path cannot do)
    model_name, model_info = find_model(kwargs)
    model_id = get_model_id(model_name)
    input_path = Path(kwargs.get("input"))
    file_base = input_path.stem
    out_dir = Path(kwargs.get("output")) / model_id
    out_dir.mkdir(parents=True, exist_ok=True)
    lg = get_logger(out_dir, Path(f"{file_base}_jaeger.log"), kwargs.get("verbose", 1))
    fsize, user_min_len = kwargs.get("fsize", 2000), kwargs.get("min_len")
    min_len = user_min_len or fsize
    table_path = out_dir / f"{file_base}.tsv"
    if table_path.exists() and not kwargs.get("overwrite"):
        lg.error("output file exists. enable --overwrite option to overwrite the output file.")
        sys.exit(1)
    for flag in ("refine", "quantized", "onnx", "int8", "cpu"):
        if kwargs.get(flag):
            lg.error(f"--{flag} is not available on the MI355X predict path (jaeger_amd has no CPU / "
                     "alternative-backend fallback; refinement post-processing is out of scope)")
            sys.exit(1)
    # experimental CRF (Viterbi) window decoding (commands/predict.py:288-307)
    crf_kw = {}
    if kwargs.get("crf"):
        lg.warning("CRF window decoding is experimental; results may change between releases")
        crf_kw = {"crf_switch_cost": kwargs.get("crf_switch_cost", 2.0), "crf_prior": kwargs.get("crf_prior", "biological")}
        matrix_path = kwargs.get("crf_transition_matrix")
        if matrix_path:
            crf_kw["crf_transition_matrix"] = json.loads(Path(matrix_path).read_text())
    # DUST soft-masking (on by default like the reference): on the GPU, on the uploaded copy of the bases inside the
    # fused call; --dust-host runs the host scan over the FASTA image instead (same masks bit for bit)
    dust = "none" if not kwargs.get("dustmask", True) else "host" if kwargs.get("dust_host", False) else "device"
    # the long pass, and with --min-len below --fsize the short contigs behind it, one whole-contig window each (padded)
    two_pass = user_min_len is not None and user_min_len < fsize
    passes = ((fsize, None, False), (user_min_len, fsize - 1, True)) if two_pass else ((min_len, None, False),)
    want = ("prediction", "reliability") + (("embedding",) if kwargs.get("save_embedding") else ()) \
        + (("nmd",) if kwargs.get("save_nmd") else ())
    want_full = bool(kwargs.get("window_scores") or kwargs.get("prophage"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    common = dict(dynamic_stride=kwargs.get("dynamic_stride", False),
                  dynamic_stride_threshold=kwargs.get("dynamic_stride_threshold", 10.0),
                  batch=kwargs.get("batch", 96), pre_cased=dust == "host", want=want, dust_device=dust == "device")
    # JAEGER_SHARDED=1: take the sharded path whatever the world size - with ONE rank under torchrun every collective of the
    # 8-GPU run (init over RCCL, broadcasts, the error all_reduce, both padded gathers, barrier) executes on the one GPU
    return RunPlan(options=kwargs, model_name=model_name, model_info=model_info, model_id=model_id, input_path=input_path,
                   file_base=file_base, out_dir=out_dir, table_path=table_path, phage_path=out_dir / f"{file_base}_phages.tsv",
                   fsize=fsize, stride=kwargs.get("stride", 1500), user_min_len=user_min_len, min_len=min_len, passes=passes,
                   want=want, want_full=want_full, pred_kw=dict(fsize=fsize, want_full=want_full, **crf_kw), dust=dust,
                   common=common, rank=int(os.environ.get("RANK", "0")), world=world,
                   local_rank=int(os.environ.get("LOCAL_RANK", str(kwargs.get("physicalid", 0)))),
                   sharded=world > 1 or os.environ.get("JAEGER_SHARDED") == "1", piped=not kwargs.get("no_pipeline"),
                   rc=kwargs.get("rc", 0.5), pc=kwargs.get("pc", 1))


@dataclass
class RunResult:
    """What the prediction stage (either path) hands to the tail of ``run_core``."""
    class_map: dict
    term_repeats: Any
    num: int                        # records of the input
    n_windows: int
    n_bp: float
    t_ingest: float
    t_predict: float
    engine: Any = None              # (the sharded path has closed its engine behind the gathers)
    agg: Any = None                 # one GPU: the aggregator and the writer that has the rows flushed so far
    writer: Any = None
    y_pred: dict | None = None      # sharded: every window's outputs; one GPU: only for the embedding / NMD files
    buffers: list = field(default_factory=list)       # the run's large host arrays, released together with the engine


def window_totals(seqlens, fsize: int) -> tuple[int, float]:
    """(windows, bases they cover) of a run, from the per-window record lengths of its passes' window tables."""
    return sum(len(s) for s in seqlens), sum(float(np.minimum(np.asarray(s, np.int64), fsize).sum()) for s in seqlens)


# ---- steps both paths take ----------------------------------------------------------------------------------
def make_engine(plan: RunPlan):
    from .engine import JaegerHipEngine
    opt, t_eng = plan.options, time.time()
    _mark("engine_setup_begin")
    try:
        # the engine resolves the weights itself (weights.load_weights): the graph's variable bundle - what the reference
        # executes - first, then the .weights.h5, then the canonical .npz
        eng = JaegerHipEngine(plan.model_info, device_id=plan.local_rank, chunk=opt.get("chunk", 0),
                              precision="f32" if opt.get("exact_f32") else None,
                              trust_project=True if opt.get("trust_project") else None)
        if opt.get("stream_bytes"):                 # span budget of the host -> HBM ingest (default 32 MiB)
            eng.device.set_stream_bytes(int(opt["stream_bytes"]))
        return eng
    finally:
        LAST_RUN["engine_create_s"] = round(time.time() - t_eng, 3)
        _mark("engine_ready")


def log_setup(plan: RunPlan, engine) -> None:
    sp = engine.string_processor_config
    logger.info(f"input file: {plan.input_path.name}")
    logger.info(f"outpath: {plan.out_dir.resolve()}")
    logger.info(f"fragment size: {plan.fsize}  stride: {plan.stride}  batch: {plan.common['batch']}")
    logger.info(f"model: {plan.model_id}  arithmetic: {engine.model.precision}  device: MI355X #{plan.local_rank} "
                f"(rank {plan.rank}/{plan.world})")
    try:                                   # kernel placement (engines of other kinds have none)
        pl = engine.model.placement()
        if pl["small_fused"]:
            logger.info("kernels: fused small-window kernel (ids -> pooled sums in one launch)")
        elif engine.model.precision == "f16x3":
            logger.info(f"kernels: {pl['convs_f16x3']} of {pl['convs']} convolutions on the split-f16 kernels"
                        + (f", {pl['layout_conversions']} layout conversions" if pl["layout_conversions"] else ""))
            if pl["convs_f16x3"] < pl["convs"]:
                slow = [ln for ln in engine.model.describe().splitlines() if "exact-f32" in ln]
                logger.warning("convolutions left on the exact-f32 kernel (about 4x slower):\n  " + "\n  ".join(slow))
    except AttributeError:
        pass
    msg = _crop_length_warning(sp.get("crop_size_codons"), sp.get("crop_size_nt"), plan.fsize)
    if msg:
        logger.warning(msg)


def host_dust(plan: RunPlan, fa: "frag.FastaBatch") -> None:
    """``--dust-host``: soft-mask the bases this process holds (under torchrun: this rank's contigs) in place."""
    if plan.dust == "host":
        t0 = time.time()
        n_masked = frag.dust_mask(fa)
        whose = f" of this rank's {len(fa)} contigs" if plan.sharded else ""
        logger.info(f"DUST (window 64, threshold 20): {n_masked} of {fa.bases.size} bases{whose} soft-masked in "
                    f"{time.time() - t0:.2f} s")


def log_passes(plan: RunPlan) -> None:
    if len(plan.passes) > 1:
        logger.info(f"Two-pass prediction: long contigs (>= {plan.fsize} bp) then short contigs "
                    f"({plan.user_min_len}-{plan.fsize - 1} bp)")


# ---- one GPU ------------------------------------------------------------------------------------------------
# A worker thread owns the engine: it sets the model up while the FASTA is read (every core, native), then runs ONE fused
# call over all windows of the long pass (DUST on its uploaded spans, encoder, forward; the library streams the spans through
# pinned staging and publishes its progress).  Beside it the calling thread aggregates the contigs whose windows are final,
# a third thread scans for terminal repeats on a stream of its own and a fourth writes the rows of finished batches, so that
# what is left behind the forward is the last batch and the TSV (_predict_pipelined).  --no-pipeline runs the same steps one
# after the other (_predict_sequential).
def scan_repeats(plan: RunPlan, device, fa: "frag.FastaBatch"):
    t_term = time.time()
    _mark("repeat_scan_begin")
    from .termini import REPORT_MIN_COLUMNS, RepeatColumns, terminal_repeat_table
    # (alignments of at most 12 columns never reach the table: the scan may skip them - same repeat columns)
    table = terminal_repeat_table(device, fa, plan.fsize, report_min=REPORT_MIN_COLUMNS)
    _mark("repeat_table_done")
    rep = RepeatColumns(table, fa.names, fa.lengths)       # (the DataFrame form only where something asks for it)
    LAST_RUN["terminal_repeats_s"] = round(time.time() - t_term, 3)
    _mark("repeat_scan_done")
    logger.info(f"terminal repeats: {rep.n_found} of {len(rep)} contigs in {time.time() - t_term:.2f} s")
    return rep


class _SideThread(threading.Thread):
    """A daemon thread beside the forward: ``result`` or ``error`` of ``fn(*args)`` is for the calling thread to take."""

    def __init__(self, name: str, fn, *args):
        super().__init__(name=name, daemon=True)
        self.fn, self.args, self.result, self.error = fn, args, None, None

    def run(self) -> None:
        try:
            self.result = self.fn(*self.args)
        except BaseException as e:          # noqa: BLE001 - handed to the calling thread
            self.error = e


# The terminal-repeat scan of the pipelined run starts as soon as the bases are there - a thread and a stream of its own - so
# that most of it runs while the model is still being set up: beside the forward its workgroups only get the CUs in the gaps
# between the network's launches (the conv and small-window kernels take a CU's whole LDS), and the rows of finished batches
# cannot go to the table before the repeat columns exist.
def _scan_on_side_device(plan: RunPlan, fa: "frag.FastaBatch"):
    from .engine import HipDevice
    side = HipDevice(plan.local_rank)
    # the scan's short kernels go in front of the network's launches (stream priority): the repeat table is
    # there long before the forward ends, and finished batches' rows are written beside it, not behind it
    if hasattr(side, "set_stream_priority"):               # (duck-typed devices)
        side.set_stream_priority(True)
    try:
        return scan_repeats(plan, side, fa)
    finally:
        side.close()


# Rows of finished batches go to the table beside the forward, on a thread of their own (the calling thread aggregates;
# formatting a batch's rows is native code and numpy: both run without the interpreter lock).
def _flush_rows(agg: _Aggregator, writer: _LazyTableWriter, scan: _SideThread, stopping: threading.Event) -> None:
    while True:
        last = stopping.is_set()
        if scan.result is not None:         # (the pass after the stop signal waits for the pool's last batches)
            agg.flush(writer, scan.result, wait=last)
        if last:
            return
        time.sleep(0.002)


class _SingleGpuRun:
    """The steps the pipelined and the sequential sequence share, and what each leaves for the next."""

    def __init__(self, plan: RunPlan):
        self.plan = plan
        self.t_predict = self.t_setup = time.time()
        self.fa = self.table = self.starts = self.engine = self.out = self.writer = self.agg = None
        self.num, self.t_ingest, self.y_short = 0, 0.0, {}

    def ingest(self) -> None:
        """(under torchrun rank 0 indexes the file and every rank reads its own contigs instead)"""
        try:
            t0 = time.time()
            _mark("ingest_begin")
            self.fa = frag.load_fasta(str(self.plan.input_path))
            self.t_ingest = time.time() - t0
            _mark("ingest_done")
            self.num = validate_fasta_entries(self.fa, min_len=self.plan.min_len)
        except Exception as e:
            logger.error(e)
            sys.exit(1)

    def window_table(self) -> None:
        """Host DUST where asked for, then the long pass's windows."""
        plan, fa = self.plan, self.fa
        host_dust(plan, fa)
        log_passes(plan)
        self.table = frag.build_window_table(fa.lengths, plan.fsize, plan.stride, plan.common["dynamic_stride"],
                                             plan.common["dynamic_stride_threshold"], *plan.passes[0][:2])
        self.starts = fa.offsets[self.table.contig] + self.table.start
        _mark("window_table_done")
        LAST_RUN["ingest_and_table_s"] = round(time.time() - self.t_setup, 3)

    def take_engine(self, get_engine) -> None:
        """``get_engine()`` gives the engine or raises what its set-up raised; then the long pass's rows, aggregator, writer."""
        plan = self.plan
        try:
            self.engine = get_engine()
        except Exception as e:
            logger.debug(traceback.format_exc())
            logger.error(f"could not set up the model on GPU {plan.local_rank}: {e}")
            sys.exit(1)
        self.t_setup = time.time() - self.t_setup
        n_long, class_map = len(self.table), self.engine.class_map
        self.out = self.engine.model.host_outputs(n_long, plan.want)
        self.writer = _LazyTableWriter(class_map, plan.table_path, plan.phage_path, plan.rc, plan.pc)
        self.agg = _Aggregator(self.table, self.fa.names, self.out, dict(plan.pred_kw, class_map=class_map, term_repeats=None),
                               min_batch=n_long // 16, workers=2 if plan.piped else 1)

    def classify(self) -> float:
        """The one fused call over every window of the long pass; its seconds."""
        plan, fa, t0 = self.plan, self.fa, time.time()
        _mark("fused_call_begin")
        if len(self.table):
            self.engine.predict_windows(fa.bases, self.starts, self.table.length, plan.fsize, pre_cased=plan.dust == "host",
                                        want=plan.want, dust_records=fa.offsets if plan.dust == "device" else None, out=self.out)
        _mark("fused_call_done")
        return time.time() - t0

    def remaining_passes(self) -> None:
        """The long pass's last contigs, then the passes behind it (the short contigs), each as one more batch."""
        plan = self.plan
        self.agg.advance(len(self.table), final=True)
        for lo, hi, padded in plan.passes[1:]:
            y = predict_batch(self.engine, self.fa, plan.fsize, plan.stride, min_len=lo, max_len=hi, padded=padded, **plan.common)
            self.agg.add(y)
            self.y_short = _concat_predictions(self.y_short, y)

    def inference_failed(self, e: Exception) -> None:
        """(called while ``e`` is being handled)"""
        self.writer.abort()             # rows of finished batches were appended beside the forward: no truncated table stays
        logger.debug(traceback.format_exc())
        logger.error(f"an error {e} occured during inference on MI355X #{self.plan.local_rank}!")
        sys.exit(1)

    def result(self, term_repeats, t_forward: float) -> RunResult:
        plan, agg, n_long = self.plan, self.agg, len(self.table)
        t_predict = time.time() - self.t_predict
        n_windows, n_bp = window_totals([self.table.seqlen, self.y_short.get("meta_4", ())], plan.fsize)
        y_pred = None
        if plan.options.get("save_embedding") or plan.options.get("save_nmd"):   # the per-window vectors with their headers
            y_pred = _concat_predictions(agg.slice(0, n_long) if n_long else {}, self.y_short)
        logger.info(f"GPU worker: model set-up {self.t_setup:.2f} s (beside the FASTA ingest), {n_long} windows classified "
                    f"in {t_forward:.2f} s; {len(agg.parts)} aggregation batches, {agg.busy_s:.2f} s beside the forward")
        LAST_RUN.update(model_setup_and_ingest_s=round(self.t_setup, 3), ingest_s=round(self.t_ingest, 3),
                        forward_s=round(t_forward, 3), aggregation_batches=len(agg.parts),
                        aggregation_beside_forward_s=round(agg.busy_s, 3), windows=n_windows, pipelined=bool(plan.piped))
        return RunResult(class_map=self.engine.class_map, term_repeats=term_repeats, num=self.num, n_windows=n_windows,
                         n_bp=n_bp, t_ingest=self.t_ingest, t_predict=t_predict, engine=self.engine, agg=agg, writer=self.writer,
                         y_pred=y_pred, buffers=[self.fa, self.table, self.out, agg, self.starts, y_pred])


def _predict_sequential(plan: RunPlan) -> RunResult:
    """``--no-pipeline``: every step on the calling thread, one after the other."""
    run = _SingleGpuRun(plan)
    run.ingest()
    run.window_table()
    run.take_engine(lambda: make_engine(plan))
    try:
        log_setup(plan, run.engine)
        term_repeats = scan_repeats(plan, run.engine.device, run.fa)
        t_forward = run.classify()
        run.remaining_passes()
    except Exception as e:
        run.inference_failed(e)
    finally:
        run.agg.close()
    return run.result(term_repeats, t_forward)


def _predict_pipelined(plan: RunPlan) -> RunResult:
    from concurrent.futures import ThreadPoolExecutor
    pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="jaeger-gpu")
    run = _SingleGpuRun(plan)
    f_engine = pool.submit(make_engine, plan)
    run.ingest()
    scan = _SideThread("jaeger-termini", _scan_on_side_device, plan, run.fa)
    scan.start()
    run.window_table()
    run.take_engine(f_engine.result)
    agg, flusher, stop_rows = run.agg, None, threading.Event()
    try:
        f_pred = pool.submit(run.classify)
        log_setup(plan, run.engine)
        flusher = _SideThread("jaeger-rows", _flush_rows, agg, run.writer, scan, stop_rows)
        flusher.start()
        while not f_pred.done():
            agg.names_unique()
            agg.advance(run.engine.device.windows_done())
            time.sleep(0.004)
        t_forward = f_pred.result()
        agg.advance(len(run.table), final=True)     # the last contigs: needs no repeat column, runs while the scan finishes
        _mark("aggregated")
        scan.join()
        stop_rows.set()
        flusher.join()
        _mark("rows_beside_forward_done")
        if flusher.error is not None:
            raise flusher.error
        if scan.error is not None:
            raise scan.error
        run.remaining_passes()
    except Exception as e:
        run.inference_failed(e)
    finally:
        if flusher is not None:             # (an error path: the row thread must not outlive the writer it uses)
            stop_rows.set()
            flusher.join()
        agg.close()                         # (every batch handed to the pool has been aggregated)
        pool.shutdown(wait=True)
    return run.result(scan.result, t_forward)


# ---- the tail: tables, side outputs, release ----------------------------------------------------------------
def _write_tables_single(plan: RunPlan, res: RunResult):
    """What is left behind the forward: the last batch (and the short-contig pass).  (rows written, per-window data)"""
    try:
        _mark("last_flush_begin")
        res.agg.flush(res.writer, res.term_repeats)
        n_written = res.writer.close()
        _mark("tables_closed")
    except BaseException:
        res.writer.abort()
        raise
    LAST_RUN["merge_s"] = 0.0
    return n_written, res.agg.result_full()


def _write_tables_sharded(plan: RunPlan, res: RunResult):
    """Rank 0 after the gathers: one aggregation over every window, one table write.  (rows written, per-window data)"""
    t0 = time.time()
    from .postprocess import pred_to_dict, write_output
    data, data_full = pred_to_dict(res.y_pred, class_map=res.class_map, term_repeats=res.term_repeats, **plan.pred_kw)
    LAST_RUN["merge_s"] = round(time.time() - t0, 3)
    return write_output(data, labels=res.class_map.get("class"), indices=res.class_map.get("index"),
                        output_table_path=plan.table_path, output_phage_table_path=plan.phage_path,
                        reliability_cutoff=plan.rc, phage_score=plan.pc), data_full


def _prophage_regions_and_report(plan: RunPlan, res: RunResult, data_full: dict, frames: dict, pro_dir: Path) -> None:
    """``segment`` over the frames, then the att-site search and ``prophages_jaeger.tsv`` (commands/predict.py:378-437).
    Single and sharded runs alike: the process that holds the frames reads the flanks' contigs from the input file; the
    device is the run's engine where it is still open, else one opened for the call - and none when no contig has a region."""
    from .postprocess import header_strings
    from .prophage_report import prophage_report
    from .prophage_segment import segment
    opt = plan.options
    lc = opt.get("lc", 500_000)
    phage_cord = segment(frames, cutoff_length=lc, sensitivity=opt.get("sensitivity", 1.5), identifier="phage")
    if not any(len(cords) > 0 and len(scores) > 0 for cords, scores in phage_cord.values()):
        logger.info("no prophage regions found")
        return
    # contig of a frame -> record of the file: both hold the records of at least lc bases in file order
    headers, lengths = header_strings(data_full["headers"]), np.asarray(data_full["lengths"])
    kept = [c for c in range(len(headers)) if lengths[c] >= lc]
    index = frag.index_fasta(str(plan.input_path))
    in_file = np.nonzero(np.asarray(index.lengths) >= lc)[0]
    if len(in_file) != len(kept) or not np.array_equal(np.asarray(index.lengths)[in_file], lengths[kept]):
        raise ValueError("the contigs of the segmentation frames are not the file's records of at least --lc bases")
    with_regions = {}                                             # record number -> [ranges, scores]
    for c, rec in zip(kept, in_file.tolist()):
        cords, scores = phage_cord.get(f"{headers[c]}", [[], []])
        if len(cords) > 0 and len(scores) > 0:
            with_regions[rec] = [cords, scores]
    recs = sorted(with_regions)
    fa = frag.load_fasta_records(str(plan.input_path), index.rec_off, recs)      # the bytes as read, before DUST
    records = [(fa.names[k], fa.sequence(k).decode("latin-1")) for k in range(len(recs))]
    opened = []

    def align(bases, jobs):
        from . import attscan
        device = res.engine.device if res.engine is not None else None
        if device is None:
            from .engine import HipDevice
            device = HipDevice(plan.local_rank)
            opened.append(device)
        return attscan.align_flanks(device, bases, jobs)      # one call: the long entry point where a flank needs it

    try:
        prophage_report(fsize=plan.fsize, records=records, prophage_cordinates=[with_regions[r] for r in recs],
                        outdir=pro_dir, align=align, stride=opt.get("stride"))
    finally:
        for device in opened:
            device.close()


def _write_side_outputs(plan: RunPlan, res: RunResult, data_full: dict) -> None:
    """Window scores, prophage segmentation inputs, phage FASTA, embedding / NMD vectors - whichever were asked for."""
    from .postprocess import header_strings
    opt, out_dir, file_base = plan.options, plan.out_dir, plan.file_base
    if opt.get("window_scores"):
        np.savez(out_dir / f"{file_base}_window_scores.npz", headers=header_strings(data_full["headers"]),
                 lengths=data_full["lengths"], predictions=np.array(data_full["predictions"], dtype=object),
                 gc_skews=np.array(data_full["gc_skews"], dtype=object),
                 gcs=np.array(data_full["gcs"], dtype=object))
    if opt.get("prophage"):
        # --- prophages (commands/predict.py:353-442): the per-contig frames logits_to_df_v2 builds from the window
        # logits (written out as they always were), the change-point segmentation over them, the att-site search at
        # the regions' boundaries on the GPU and prophages_jaeger.tsv.  Gene-based boundary refinement and the plots
        # (pyrodigal-gv / pycirclize) are not part of this path.
        try:
            from .prophage_inputs import logits_to_df_v2
            frames = logits_to_df_v2(class_map=res.class_map, cmdline_kwargs=opt, headers=header_strings(data_full["headers"]),
                                     predictions=data_full["predictions"], lengths=data_full["lengths"],
                                     gc_skews=data_full["gc_skews"], gcs=data_full["gcs"])
            if frames:
                pro_dir = out_dir / f"{file_base}_prophages"
                pro_dir.mkdir(parents=True, exist_ok=True)
                keys = list(frames)
                np.savez(pro_dir / f"{file_base}_segmentation_inputs.npz",
                         contigs=np.array(keys, dtype=object), hosts=np.array([frames[k][1] for k in keys], dtype=object),
                         lengths=np.array([frames[k][2] for k in keys], np.int64),
                         columns=np.array(list(frames[keys[0]][0].columns), dtype=object),
                         tracks=np.array([frames[k][0].to_numpy(np.float64) for k in keys], dtype=object))
                logger.info(f"prophage segmentation inputs of {len(keys)} contigs (>= {opt.get('lc', 500000)} bp) written "
                            f"to {pro_dir}")
                logger.info("identifying prophages")
                _prophage_regions_and_report(plan, res, data_full, frames, pro_dir)
            else:
                logger.info("no prophage regions found")
        except Exception as e:
            logger.error(f"an error {e} occurred during the prophage prediction step")
            logger.debug(traceback.format_exc())
    if opt.get("getsequences"):
        # --- phage sequences as FASTA (commands/predict.py:444-456) ---
        from .postprocess import write_fasta_from_results
        out_fasta = out_dir / f"{file_base}_phages_jaeger.fasta"
        logger.info(f"generating fasta file {out_fasta}")
        n_seq = write_fasta_from_results(plan.input_path, plan.phage_path, out_fasta)
        logger.info(f"{n_seq} phage sequences written")
    y_pred = res.y_pred
    if y_pred is not None:
        headers = np.asarray(y_pred.get("meta_0", np.array([], dtype=object))).astype(str)
        if opt.get("save_embedding") and "embedding" in y_pred:
            np.savez(out_dir / f"{file_base}_embedding.npz", embedding=y_pred["embedding"], headers=headers)
        if opt.get("save_nmd") and "nmd" in y_pred:
            np.savez(out_dir / f"{file_base}_nmd.npz", embedding=y_pred["nmd"], headers=headers)   # legacy key name


def _release_behind(engine, buffers: list) -> None:
    # the engine's buffers (workspace, pinned staging) are released beside the caller: freeing them takes tens of
    # milliseconds - a tenth of a short run - and nothing the caller gets depends on it
    # ... nor on the large host buffers of the run (bases, window table, per-window outputs: unmapping half a gigabyte
    # takes another 20 ms): ``buffers`` is emptied on that thread too, which drops their last references once the caller
    # has let go of its own
    def release():
        try:
            engine.close()
        except Exception as e:          # noqa: BLE001 - nobody joins this thread for its result: say it in the run log
            logger.warning(f"releasing the engine failed: {type(e).__name__}: {e}")
        finally:
            buffers.clear()

    th_close = threading.Thread(target=release, name="jaeger-engine-close")
    _PENDING_RELEASE.append(th_close)   # the next run_core (and bench.py before it times anything) joins it
    th_close.start()


# ---- run_core ---------------------------------------------------------------------------------
def run_core(**kwargs) -> int:
    """Equivalent of ``commands/predict.py:run_core``; returns the number of table rows written."""
    wait_for_release()
    t_start = time.time()
    LAST_RUN.clear()
    LAST_RUN.update(timeline=[], t_start_epoch=t_start)
    plan = plan_run(kwargs)
    if plan.sharded:
        from . import sharded
        res = sharded.predict_sharded(plan)
        if res is None:                 # ranks other than 0 are done after the gather
            sharded._close_process_group()
            return 0
    else:
        res = (_predict_pipelined if plan.piped else _predict_sequential)(plan)
    if plan.dust == "device" and res.engine is not None:
        logger.info(f"DUST (window 64, threshold 20) on the GPU: {res.engine.dust_masked_total} bases soft-masked inside "
                    f"the fused calls")
    t_post = time.time()
    n_written, data_full = (_write_tables_sharded if plan.sharded else _write_tables_single)(plan, res)
    LAST_RUN["tsv_s"] = round(time.time() - t_post - LAST_RUN["merge_s"], 3)
    logger.info(f"processed {n_written}/{res.num} sequences")
    _write_side_outputs(plan, res, data_full)
    _mark("end")
    t_all = time.time() - t_start
    LAST_RUN.update(behind_forward_s=round(time.time() - t_post, 3), wall_s=round(t_all, 3))
    logger.info(f"wall time(s) : {t_all:.2f}  ({res.n_windows} windows; FASTA ingest {res.t_ingest:.2f} s, "
                f"encode+forward {res.t_predict:.2f} s = {res.n_bp / 1e6 / max(res.t_predict, 1e-9):.1f} Mbp/s, "
                f"aggregation+TSV behind the forward {time.time() - t_post:.2f} s; "
                f"end to end {res.n_bp / 1e6 / max(t_all, 1e-9):.1f} Mbp/s)")
    if res.engine is not None:
        _release_behind(res.engine, res.buffers)
    if plan.sharded:
        sharded._close_process_group()
    return n_written
