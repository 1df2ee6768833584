"""``run_core`` on CPU: a stand-in engine (deterministic logits computed from the window bases on the host - the GPU engine
itself is covered by the -m gpu tests), a seeded 15-record FASTA and the ``run_core`` call the CPU tests share
(tests/test_run_core_sharded.py, tests/test_run_core_stages.py, tests/golden/make_golden.py)."""
from pathlib import Path

import numpy as np


class _StandInModel:
    precision = "stand-in"

    def __init__(self, n_classes):
        self.n_classes = n_classes

    def host_outputs(self, n_win, want=("prediction", "reliability"), counts=True):
        out = {"prediction": np.zeros((n_win, self.n_classes), np.float32), "reliability": np.zeros((n_win, 1), np.float32)}
        out = {k: v for k, v in out.items() if k in want}
        if counts:
            out["counts"] = np.zeros((n_win, 4), np.int32)
        return out


class _StandInDevice:
    """JG_STAT_WINDOWS_DONE of the stand-in: rows below the mark are final while predict_windows is still running."""
    done = 0

    def windows_done(self):
        return self.done


class _StandInEngine:
    """Same surface as JaegerHipEngine for run_core: class_map, string_processor_config, model.host_outputs,
    predict_windows(out=...), device.windows_done."""

    def __init__(self, path_dict=None, **kw):
        import yaml
        classes = yaml.safe_load(Path(path_dict["classes"]).read_text())["classes"]
        self.class_map = {"num_classes": len(classes), "class": [c["class"] for c in classes],
                          "index": [c["label"] for c in classes]}
        self.string_processor_config = {"crop_size_codons": None, "crop_size_nt": None}
        self.model = _StandInModel(len(classes))
        self.device = _StandInDevice()

    dust_masked_total = 0

    def predict_windows(self, bases, win_start, win_len, fsize, l_pad=None, pre_cased=False,
                        want=("prediction", "reliability"), dust_records=None, out=None):
        import time
        if dust_records is not None:
            # what jg_engine_set_dust does on the device: DUST on a COPY of the bases by their record table, then the
            # encoder respects the case (the host scan gives the same masks bit for bit: tests/test_gpu_dust.py)
            from jaeger_amd import fragment as frag
            off = np.asarray(dust_records, np.int64)
            assert off[0] >= 0 and off[-1] <= len(bases) and (np.diff(off) >= 0).all()
            tmp = frag.FastaBatch([""] * (len(off) - 1), np.array(bases, np.uint8, copy=True), off)
            self.dust_masked_total += frag.dust_mask(tmp, threads=1)
            bases, pre_cased = tmp.bases, True
        n = len(win_start)
        res = out if out is not None else self.model.host_outputs(n, want)
        pred, rel, counts = res["prediction"], res["reliability"], res["counts"]
        self.device.done = 0
        for i, (s, ln) in enumerate(zip(np.asarray(win_start).tolist(), np.asarray(win_len).tolist())):
            w = np.asarray(bases[s:s + ln])
            up = w & 0xDF if not pre_cased else w
            c = np.array([(up == ord(ch)).sum() for ch in "GCAT"], np.int32)          # meta_5..8 order: G C A T
            counts[i] = c
            h = np.cumsum(w.astype(np.int64) * (np.arange(ln) % 7 + 1))[-1] if ln else 0
            pred[i] = [((h >> (3 * k)) % 97) / 9.0 - 5.0 for k in range(pred.shape[1])]
            rel[i, 0] = ((h >> 5) % 31) / 5.0 - 3.0
            if out is not None and i % 3 == 2:           # progress in steps of three windows, slow enough to be polled
                self.device.done = i + 1
                time.sleep(0.01)
        self.device.done = n
        return res

    def close(self):
        pass


def _write_fasta(path, seed=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = [5200, 700, 1499, 3100, 650, 1203, 400, 1500, 999, 2999, 12000, 1800, 4700, 800, 6100]
    with open(path, "w") as fh:
        for i, n in enumerate(lens):
            seq = "".join(rng.choice(list("ACGT"), n))
            if i == 3:
                seq = seq[:500] + "AT" * 60 + seq[620:]          # a low-complexity stretch for DUST
            fh.write(f">{'ctg_dup' if i in (9, 11) else f'ctg_{i}'} len={n}\n")     # two records share a name
            for j in range(0, n, 60):
                fh.write(seq[j:j + 60] + "\n")
    return lens


def _run(out_dir, fasta, model_root, min_len, no_pipeline=True, dust_host=False, engine=_StandInEngine, **extra):
    """``run_core`` with the stand-ins in place of the engine, the side device and the repeat scan (the caller puts the
    real ones back); ``extra``: further ``run_core`` keywords."""
    import pandas as pd

    import jaeger_amd.engine as E
    import jaeger_amd.termini as T
    from jaeger_amd.predict import run_core
    E.JaegerHipEngine = engine
    E.HipDevice = lambda *a, **k: type("SideStream", (), {"close": lambda self: None})()
    T.scan_for_terminal_repeats = lambda device, fa, fsize: pd.DataFrame(
        {"contig_id": [n.strip().replace(",", "___") for n, ln in zip(fa.names, fa.lengths.tolist()) if ln >= fsize],
         "terminal_repeats": None, "repeat_length": np.nan})
    T.terminal_repeat_table = lambda device, fa, fsize, report_min=0: np.where(
        (fa.lengths >= fsize)[:, None], np.zeros((len(fa), 10), np.int32), np.int32(-1)).astype(np.int32)
    return run_core(input=str(fasta), output=str(out_dir), model_path=str(model_root), fsize=1500, stride=1500,
                    min_len=min_len, batch=2, dustmask=True, rc=0.1, pc=1, overwrite=True, verbose=1,
                    no_pipeline=no_pipeline, prophage=True, lc=4000, dust_host=dust_host, **extra)
