"""``run_core`` as stages, on CPU with the stand-in engine of tests/run_core_standin.py: the sequential, the pipelined and the
``--dust-host`` run reproduce the TSVs and window scores recorded before ``run_core`` was split (tests/golden/
run_core_standin_*: tests/golden/make_golden.py run_core_standin), ``LAST_RUN`` keeps its keys, every timeline mark is there
and comes from the thread that issued it before, and a failing forward leaves no table and no thread behind."""
import threading

import numpy as np
import pytest

from conftest import GOLDEN, make_model_dir
from run_core_standin import _run, _StandInEngine, _write_fasta

LAST_RUN_KEYS = {"timeline", "t_start_epoch", "engine_create_s", "ingest_and_table_s", "terminal_repeats_s",
                 "model_setup_and_ingest_s", "ingest_s", "forward_s", "aggregation_batches", "aggregation_beside_forward_s",
                 "windows", "pipelined", "merge_s", "tsv_s", "behind_forward_s", "wall_s"}
SEQUENTIAL = ["ingest_begin", "ingest_done", "window_table_done", "engine_setup_begin", "engine_ready", "repeat_scan_begin",
              "repeat_table_done", "repeat_scan_done", "fused_call_begin", "fused_call_done", "last_flush_begin",
              "tables_closed", "end"]
CHAINS = {"calling thread": ["ingest_begin", "ingest_done", "window_table_done", "aggregated", "rows_beside_forward_done",
                             "last_flush_begin", "tables_closed", "end"],
          "worker": ["engine_setup_begin", "engine_ready", "fused_call_begin", "fused_call_done", "aggregated"],
          "scan": ["ingest_done", "repeat_scan_begin", "repeat_table_done", "repeat_scan_done", "rows_beside_forward_done"]}


@pytest.fixture
def standin(tmp_path):
    """The FASTA and the model directory; the real engine, side device and repeat scan are back afterwards."""
    import jaeger_amd.engine as E
    import jaeger_amd.predict as P
    import jaeger_amd.termini as T
    keep = (E.JaegerHipEngine, E.HipDevice, T.scan_for_terminal_repeats, T.terminal_repeat_table)
    _write_fasta(tmp_path / "in.fasta")
    make_model_dir(tmp_path / "m")
    yield tmp_path
    P.wait_for_release()
    E.JaegerHipEngine, E.HipDevice, T.scan_for_terminal_repeats, T.terminal_repeat_table = keep


def _check_outputs(out_dir, tag):
    got = out_dir / "38341_1.4M"
    assert (got / "in.tsv").read_bytes() == (GOLDEN / f"run_core_standin_{tag}.tsv").read_bytes()
    assert (got / "in_phages.tsv").read_bytes() == (GOLDEN / f"run_core_standin_{tag}_phages.tsv").read_bytes()
    ws, want = np.load(got / "in_window_scores.npz", allow_pickle=True), np.load(GOLDEN / f"run_core_standin_{tag}.npz")
    np.testing.assert_array_equal(ws["lengths"], want["lengths"])
    assert ws["lengths"].dtype == want["lengths"].dtype
    assert [len(p) for p in ws["predictions"]] == want["rows"].tolist()
    pred = np.concatenate([np.asarray(p) for p in ws["predictions"]], axis=0)
    assert pred.dtype == want["predictions"].dtype
    np.testing.assert_array_equal(pred, want["predictions"])


@pytest.mark.parametrize("min_len", [None, 600])
def test_every_sequence_reproduces_the_recorded_outputs(standin, min_len):
    import jaeger_amd.predict as P
    tag = "none" if min_len is None else str(min_len)
    runs = {"sequential": {}, "pipelined": dict(no_pipeline=False), "dust_host": dict(dust_host=True)}
    for name, kw in runs.items():
        n = _run(standin / name, standin / "in.fasta", standin / "m", min_len, window_scores=True, **kw)
        assert n == len((GOLDEN / f"run_core_standin_{tag}.tsv").read_text().splitlines()) - 1
        _check_outputs(standin / name, tag)
        assert set(P.LAST_RUN) == LAST_RUN_KEYS, name
        assert P.LAST_RUN["pipelined"] == (name == "pipelined")
        events = [e for e, _ in P.LAST_RUN["timeline"]]
        if name != "pipelined":
            assert events == SEQUENTIAL, name
            continue
        assert sorted(events) == sorted(SEQUENTIAL + ["aggregated", "rows_beside_forward_done"])
        # every chain's marks follow from one another (same thread, or a join / a future's result in between), so each is
        # appended after the one before it: the position in the list is their time order (the times are rounded)
        at = {e: i for i, e in enumerate(events)}
        for who, chain in CHAINS.items():
            assert [at[e] for e in chain] == sorted(at[e] for e in chain), (who, events)


@pytest.mark.parametrize("min_len", [None, 600])
@pytest.mark.parametrize("no_pipeline", [True, False])
def test_a_failing_forward_leaves_no_table_and_no_thread(standin, min_len, no_pipeline):
    class Failing(_StandInEngine):
        def predict_windows(self, *a, **k):
            raise RuntimeError("forward failed")

    with pytest.raises(SystemExit) as exc:
        _run(standin / "out", standin / "in.fasta", standin / "m", min_len, no_pipeline=no_pipeline, engine=Failing)
    assert exc.value.code == 1
    assert not (standin / "out" / "38341_1.4M" / "in.tsv").exists()
    left = [t.name for t in threading.enumerate() if t.name.startswith(("jaeger-rows", "jaeger-gpu", "jaeger-agg"))]
    assert not left, left
