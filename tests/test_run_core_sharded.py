"""The torchrun path of ``run_core`` on CPU: world_size 2 over gloo with a stand-in engine (deterministic logits
computed from the window bases on the host - the GPU engine itself is covered by the -m gpu tests).  Contig
sharding (LPT), the object gather, the restoration of the reference's emission order (FASTA order, long pass before
short pass) and the TSV must equal a single-process run byte for byte.  Under torchrun rank 0 indexes the FASTA,
every rank reads / masks / classifies only its own contigs (asserted: no rank holds the whole base buffer), one
gather of f32 rows + one of the int32 repeat table; duplicate record names survive (order is by record index)."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import ROOT, make_model_dir
from run_core_standin import _run, _write_fasta


def _worker(rank, world, port, tmp, min_len):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _run(Path(tmp) / "sharded", Path(tmp) / "in.fasta", Path(tmp) / "m", min_len)
    import json

    import jaeger_amd.predict as P
    (Path(tmp) / f"shard_stats_{rank}.json").write_text(json.dumps(P.SHARD_STATS))
    dist.destroy_process_group()


@pytest.mark.parametrize("min_len", [None, 600])
def test_sharded_run_core_equals_single_process(tmp_path, min_len, monkeypatch):
    import torch.multiprocessing as mp
    _write_fasta(tmp_path / "in.fasta")
    make_model_dir(tmp_path / "m")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    import jaeger_amd.engine as E
    import jaeger_amd.termini as T
    keep = (E.JaegerHipEngine, E.HipDevice, T.scan_for_terminal_repeats, T.terminal_repeat_table)
    try:
        n_single = _run(tmp_path / "single", tmp_path / "in.fasta", tmp_path / "m", min_len)
        # the single-GPU host pipeline (worker thread owns the engine; the calling thread aggregates finished contigs in
        # batches beside the forward - here every two windows or more)
        import jaeger_amd.predict as P
        real_agg = P._Aggregator
        batches = []

        class SmallBatches(real_agg):
            def __init__(self, *a, **k):
                k["min_batch"] = 2
                super().__init__(*a, **k)
                batches.append(self)

        monkeypatch.setattr(P, "_Aggregator", SmallBatches)
        n_piped = _run(tmp_path / "piped", tmp_path / "in.fasta", tmp_path / "m", min_len, no_pipeline=False)
        monkeypatch.setattr(P, "_Aggregator", real_agg)
        assert len(batches) == 1 and len(batches[0].parts) >= 3        # aggregation really ran in several batches
        # --dust-host: the host pass over the FASTA image instead of DUST inside the fused calls (record tables of the
        # whole-buffer and of the compacted short-contig batches): same TSV
        n_host = _run(tmp_path / "hostdust", tmp_path / "in.fasta", tmp_path / "m", min_len, dust_host=True)
    finally:
        E.JaegerHipEngine, E.HipDevice, T.scan_for_terminal_repeats, T.terminal_repeat_table = keep
    assert n_piped == n_single == n_host
    assert (tmp_path / "hostdust" / "38341_1.4M" / "in.tsv").read_text() == \
        (tmp_path / "single" / "38341_1.4M" / "in.tsv").read_text()
    assert (tmp_path / "piped" / "38341_1.4M" / "in.tsv").read_text() == \
        (tmp_path / "single" / "38341_1.4M" / "in.tsv").read_text()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path), min_len), nprocs=2, join=True)
    single = (tmp_path / "single" / "38341_1.4M" / "in.tsv").read_text()
    sharded = (tmp_path / "sharded" / "38341_1.4M" / "in.tsv").read_text()
    assert n_single > 0 and single == sharded
    # -p: the segmentation-input frames of the contigs >= --lc, identical from one process and from two ranks
    seg = [np.load(tmp_path / d / "38341_1.4M" / "in_prophages" / "in_segmentation_inputs.npz", allow_pickle=True)
           for d in ("single", "sharded")]
    assert list(seg[0]["contigs"]) == list(seg[1]["contigs"]) == ["ctg_0", "ctg_10", "ctg_12", "ctg_14"]
    for a, b in zip(seg[0]["tracks"], seg[1]["tracks"]):
        np.testing.assert_array_equal(a, b)
    ids = [ln.split("\t")[0] for ln in single.splitlines()[1:]]
    long_first = [f"ctg_{i}" for i in (0, 3, 7, 10, 12, 14)]
    assert ids.count("ctg_dup") >= 2                                # both records that share a name are reported
    ids = [i for i in ids if i != "ctg_dup"]
    # per-rank ingest: each rank parsed only its own contigs, together they cover the used ones exactly once
    import json
    stats = [json.loads((tmp_path / f"shard_stats_{r}.json").read_text()) for r in range(2)]
    total = stats[0]["total_bases"]
    assert all(0 < st["local_bases"] < total for st in stats), stats
    assert sum(st["local_bases"] for st in stats) <= total and stats[0]["total_records"] == 15
    assert ids[:len(long_first)] == long_first                      # FASTA order, long pass first
    if min_len is not None:
        assert set(ids[len(long_first):]) <= {"ctg_1", "ctg_2", "ctg_4", "ctg_5", "ctg_8", "ctg_13"}
