"""``run_core`` under ``torchrun`` (WORLD_SIZE > 1, or JAEGER_SHARDED=1): contig-sharded prediction, one gather of f32 rows.

Rank 0 indexes the FASTA and broadcasts (record byte offsets, lengths); every rank reads, soft-masks, scans and classifies
only the contigs LPT deals it; one padded gather of f32 rows (logits | reliability | G C A T counts [| embedding | nmd]) and
one of the int32 repeat table go to rank 0, which rebuilds the window metadata from its own window table and restores FASTA
order (long pass before short pass).  This module imports torch: ``predict.py`` imports it only on this path.
"""

from __future__ import annotations

import os
import sys
import time
import traceback
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist

from . import dist as jdist
from . import fragment as frag
from .predict import (SHARD_STATS, RunPlan, RunResult, _concat_predictions, host_dust, log_passes, log_setup, logger,
                      make_engine, predict_batch, window_totals)

# the column blocks of a gathered row, in this order (a model without an output has width 0 there)
ROW_COLUMNS = ("prediction", "reliability", "counts", "embedding", "nmd")


def _shard_records(lengths: np.ndarray, fsize: int, stride: int | None, world: int):
    """Whole contigs to ranks, balanced by window count (LPT); returns one index list per rank."""
    step = fsize if stride is None else stride
    w = np.where(lengths >= fsize, np.maximum(1, (lengths - fsize) // step + 1), 1)
    return jdist.lpt_partition(w, world)


def _close_process_group():
    """Destroy the process group if ``_init_process_group`` created it (a caller's own group is left alone)."""
    if SHARD_STATS.pop("own_process_group", False) and dist.is_initialized():
        dist.destroy_process_group()


def _coll_device(local_rank: int):
    return torch.device("cuda", local_rank) if dist.get_backend() == "nccl" else torch.device("cpu")


def _bcast(arr: np.ndarray | None, dtype, n: int, dev):
    """Broadcast a 1-D array from rank 0 (``arr`` is None elsewhere)."""
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype)).to(dev) if arr is not None else \
        torch.zeros(n, dtype=torch.from_numpy(np.zeros(0, dtype)).dtype, device=dev)
    dist.broadcast(t, src=0)
    return t.cpu().numpy()


def _place_rows(out: np.ndarray, part: np.ndarray, items: np.ndarray, rows_per_item: np.ndarray, first: np.ndarray):
    """``part`` holds the rows of ``items`` back to back (``rows_per_item[i]`` each); write them to their global
    positions ``first[i]...`` (vectorised :func:`jaeger_amd.dist.restore_order`)."""
    n = rows_per_item[items]
    total = int(n.sum())
    if total == 0:
        return
    local_first = np.cumsum(n) - n
    dest = np.repeat(first[items] - local_first, n) + np.arange(total, dtype=np.int64)
    out[dest] = part[:total]


def _init_process_group(plan: RunPlan):
    """Join (or, outside a caller's own group, create) the process group; the device its collectives' tensors live on."""
    rank, world, local_rank = plan.rank, plan.world, plan.local_rank
    if not dist.is_initialized():
        SHARD_STATS["own_process_group"] = True          # run_core destroys what it created
        if torch.cuda.is_available():
            torch.cuda.set_device(local_rank)
        # RCCL ("nccl") when GPUs are there; JAEGER_DIST_BACKEND=gloo lets several ranks share one GPU (tests)
        backend = os.environ.get("JAEGER_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ and world == 1:      # one rank outside torchrun (JAEGER_SHARDED=1)
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        try:
            if backend == "nccl":
                dist.init_process_group(backend, rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
            else:
                dist.init_process_group(backend, rank=rank, world_size=world)
        except Exception as e:              # no fallback to another backend: the error is the result
            logger.error(f"could not initialise the {backend} process group on rank {rank}/{world} "
                         f"(HSA_ENABLE_IPC_MODE_LEGACY={os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')}): {type(e).__name__}: {e}")
            raise
    return _coll_device(local_rank)


def _broadcast_index(plan: RunPlan, dev):
    """Rank 0 indexes the FASTA; every rank gets (rank 0's index - None elsewhere -, record byte offsets, lengths) from
    the three broadcasts, or exits 1 when rank 0 found nothing to classify."""
    ix, head = None, np.zeros(2, np.int64)
    if plan.rank == 0:
        try:
            ix = frag.index_fasta(str(plan.input_path))
            ok = int((ix.lengths >= plan.min_len).sum())
            logger.info(f"{ok}/{len(ix)} entries in {plan.input_path}")
            if ok == 0:
                raise Exception(f"all records in {plan.input_path} are < {plan.min_len}bp")
            head[:] = (0, len(ix))
        except Exception as e:
            logger.error(e)
            head[:] = (1, 0)
    head = _bcast(head if plan.rank == 0 else None, np.int64, 2, dev)
    if head[0] != 0:
        sys.exit(1)
    n_rec = int(head[1])
    rec_off = _bcast(ix.rec_off if plan.rank == 0 else None, np.int64, n_rec + 1, dev)
    lengths = _bcast(ix.lengths if plan.rank == 0 else None, np.int64, n_rec, dev)
    return ix, rec_off, lengths


def _classify_own(plan: RunPlan, rec_off: np.ndarray, lengths: np.ndarray, mine: np.ndarray, t_begin: float):
    """Read, soft-mask, classify (every pass) and scan the records ``mine`` of this rank.  Never raises: what the rank brings
    to the gathers - ``local``: its rows, ROW_COLUMNS side by side, None without windows - or ``ok`` False."""
    from .termini import terminal_repeat_table
    fsize, stride = plan.fsize, plan.stride
    work = SimpleNamespace(ok=True, engine=None, local=None, widths={}, rep_local=None, t_ingest=0.0, t_predict=0.0)
    try:
        fa = frag.load_fasta_records(str(plan.input_path), rec_off, mine)
        if not np.array_equal(fa.lengths, lengths[mine]):
            raise RuntimeError(f"{plan.input_path}: record lengths changed between the index pass and this rank's read")
        work.t_ingest = time.time() - t_begin
        SHARD_STATS.update(rank=plan.rank, local_bases=int(fa.bases.size), total_bases=int(lengths.sum()),
                           local_records=len(fa), total_records=len(lengths))
        host_dust(plan, fa)
        engine = work.engine = make_engine(plan)
        log_setup(plan, engine)
        t0 = time.time()
        log_passes(plan)
        parts = [predict_batch(engine, fa, fsize, stride, min_len=lo, max_len=hi, padded=padded, meta=False, **plan.common)
                 for lo, hi, padded in plan.passes]
        cols = [k for k in ROW_COLUMNS if any(k in p for p in parts)]
        mats = [np.concatenate([np.asarray(p[k], np.float32).reshape(len(p[k]), -1) for k in cols], axis=1)
                for p in parts if p]
        work.widths = {k: next(np.asarray(p[k]).reshape(len(p[k]), -1).shape[1] for p in parts if p) for k in cols}
        work.local = np.concatenate(mats, axis=0) if mats else None
        work.t_predict = time.time() - t0
        work.rep_local = terminal_repeat_table(engine.device, fa, fsize)
    except BaseException as e:               # every rank must reach the collectives behind this, or the others hang
        logger.debug(traceback.format_exc())
        logger.error(f"an error {e} occured during inference on MI355X #{plan.local_rank} (rank {plan.rank})!")
        work.ok = False
    return work


def _gather_and_merge(plan: RunPlan, dev, ix, lengths: np.ndarray, owned: list, work) -> RunResult | None:
    """The collectives behind the ranks' work - error all_reduce, width all_reduce, two ``gather_rows``, barrier - and on
    rank 0 (None elsewhere) the result: metadata from its own window tables, rows back in the reference's emission order."""
    from .termini import repeats_frame
    failed = torch.tensor([0 if work.ok else 1], dtype=torch.int32, device=dev)
    dist.all_reduce(failed, op=dist.ReduceOp.MAX)
    if int(failed.item()) != 0:
        if work.engine is not None:
            work.engine.close()
        sys.exit(1)
    # column layout is the same on every rank (same model); ranks without windows send zero rows
    local = work.local
    wtab = torch.zeros(8, dtype=torch.int64, device=dev)
    if local is not None:
        for j, k in enumerate(ROW_COLUMNS):
            wtab[j] = work.widths.get(k, 0)
    dist.all_reduce(wtab, op=dist.ReduceOp.MAX)
    wlist = [int(v) for v in wtab.tolist()[:len(ROW_COLUMNS)]]
    n_col = sum(wlist)
    if local is None:
        local = np.zeros((0, n_col), np.float32)
    got = jdist.gather_rows(torch.from_numpy(np.ascontiguousarray(local)).to(dev), dst=0)
    rep = jdist.gather_rows(torch.from_numpy(np.ascontiguousarray(work.rep_local.reshape(-1, 10))).to(dev), dst=0)
    class_map = work.engine.class_map
    work.engine.close()
    if plan.rank != 0:
        dist.barrier()
        return None
    n_rec, fsize, common = len(lengths), plan.fsize, plan.common
    tables = [frag.build_window_table(lengths, fsize, plan.stride, common["dynamic_stride"],
                                      common["dynamic_stride_threshold"], lo, hi) for lo, hi, _ in plan.passes]
    y_pred: dict = {}
    consumed = [0] * plan.world
    for t in tables:
        n_w = np.bincount(t.contig, minlength=n_rec).astype(np.int64)
        rows = np.zeros((len(t), n_col), np.float32)
        first = np.cumsum(n_w) - n_w
        for q, items in enumerate(owned):
            take = int(n_w[items].sum())
            part = got[q].cpu().numpy()[consumed[q]:consumed[q] + take]
            _place_rows(rows, part, items, n_w, first)
            consumed[q] += take
        out, c0 = {}, 0
        for k, w in zip(ROW_COLUMNS, wlist):
            if w:
                out[k] = rows[:, c0:c0 + w]
            c0 += w
        counts = np.rint(out.pop("counts")).astype(np.int32)
        out.update(frag.window_metadata(t, ix.names, counts))
        y_pred = _concat_predictions(y_pred, out) if len(t) else y_pred
    res = np.full((n_rec, 10), -1, np.int32)
    for q, items in enumerate(owned):
        res[items] = rep[q].cpu().numpy()
    term_repeats = repeats_frame(res, ix.names, lengths)
    logger.info(f"terminal repeats: {int(term_repeats['terminal_repeats'].notna().sum())} of {len(term_repeats)} contigs")
    dist.barrier()
    n_windows, n_bp = window_totals([t.seqlen for t in tables], fsize)
    return RunResult(class_map=class_map, term_repeats=term_repeats, num=n_rec, n_windows=n_windows, n_bp=n_bp,
                     t_ingest=work.t_ingest, t_predict=work.t_predict, y_pred=y_pred)


def predict_sharded(plan: RunPlan) -> RunResult | None:
    """The prediction stage of ``run_core`` on this rank; the result on rank 0, None on the others."""
    dev = _init_process_group(plan)
    t_begin = time.time()
    ix, rec_off, lengths = _broadcast_index(plan, dev)
    used = lengths >= plan.min_len                               # contigs that yield a window in either pass
    groups = [np.sort(g) for g in _shard_records(lengths, plan.fsize, plan.stride, plan.world)]
    owned = [g[used[g]] for g in groups]                         # per rank: its records, in FASTA order
    work = _classify_own(plan, rec_off, lengths, owned[plan.rank], t_begin)
    return _gather_and_merge(plan, dev, ix, lengths, owned, work)
