"""A forward does not depend on what earlier calls left in the model's workspace (cases: tests/poison_cases.py; the CPU tier,
tests/test_poison_census.py, holds every ``__global__`` kernel of the sources to a case here or to a reason).

Every other GPU module builds a fresh model in a fresh process, where a first ``hipMalloc`` hands back zero pages - the right
padding value - so a kernel that reads a halo row, a padded lane, a gap position or a partial row nobody wrote in the current
launch group passes there and is wrong in production from the second call of a handle on.  Here:

* per case, ONE handle: the forward with ``JG_OPT_POISON_WORKSPACE`` off, under 0x00, under 0xFF (NaN in f32 and f16, a valid
  mask byte), under 0x7B (1.3e36 / 61280 - finite, so it wins a maximum and survives a select a NaN would lose - and a valid
  mask byte), and off again: the five results are bit-identical on every output the model has, as one launch group and with a
  chunk that leaves a short last group; the target op's tap is bit-identical under off / 0x00 / 0xFF as well, which names the
  op when a case fails; where the source module can tell which kernel ran, that is asserted too;
* two ``predict_windows`` cases (whole buffer; streamed through 8 KiB spans with ragged windows and DUST records), ``counts``
  included;
* the range-guard programs: the second attempt of the fallback under every fill equals a handle set to exact f32 beforehand;
* call history, option off: six calls on one handle - two row lengths either side of a placement flip, 7 / 1 / 8 windows, chunk
  0 / 3, split-f16 -> exact f32 -> split-f16 - each bit-identical to the same call on a handle that made no other call: what the
  fills cannot see (host-side state a call leaves for the next, a buffer the option's list forgot).

No tolerance appears: forwards are bit-repeatable (test_gpu_parity.py::test_f16x3_repeatable), and the unpoisoned run is the one
the per-family modules hold to float64.  No test here provokes a fault: the fills go into scratch buffers only, never into
ids, indices, offsets or operands; every test runs under a watchdog, and a failed HIP call ends the session.
"""
import faulthandler
import time
import warnings

import numpy as np
import pytest

import poison_cases as pc

pytestmark = pytest.mark.gpu

_T0 = [None]
_RAN = {}
_NOT_FINITE = []


@pytest.fixture(autouse=True)
def _watchdog():
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def device():
    from jaeger_amd.engine import HipDevice
    d = HipDevice(0)
    _T0[0] = time.time()
    yield d
    print("\npoisoned-workspace cases run, per family: " + ", ".join(f"{k} {v}" for k, v in sorted(_RAN.items())))
    for row in _NOT_FINITE:
        print("  not finite with the option off (a NaN there hides a NaN fill): " + row)
    print("  (module wall time %.1f s)" % (time.time() - _T0[0]))
    d.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _guarded(name, fn):
    """A HIP call that failed (a fault, a lost device) ends the session: nothing more runs on the device.  A refusal of the
    library itself is a finding and fails this test alone."""
    from jaeger_amd import _lib as L
    try:
        fn()
    except L.JaegerHipError as exc:
        if f"failed ({L.JG_ERR_HIP})" in str(exc):
            pytest.exit(f"{name}: {exc}", returncode=3)
        raise


def _fill_name(byte):
    return "off" if byte is None else f"0x{byte:02X}"


def _same_bits(a: dict, b: dict, what: str):
    """Every output, bit for bit (a NaN differs from another NaN of other bits, and equals itself)."""
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape)
        if not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            bad = np.argwhere(x.view(np.uint32 if x.itemsize == 4 else np.uint8) != y.view(np.uint32 if x.itemsize == 4 else np.uint8))
            i = tuple(int(v) for v in bad[0])
            raise AssertionError(f"{what}: {k} differs at {len(bad)} of {x.size} elements, first at {i}: {x[i]!r} against {y[i]!r}")


def _run_fills(set_poison, forward, what, sequence=pc.SEQUENCE):
    """``forward()`` under every fill of the sequence; all results equal the first (the option off)."""
    first = None
    for step, byte in enumerate(sequence):
        set_poison(byte)
        got = forward()
        if first is None:
            first = got
            for k, v in got.items():      # (reported, not asserted: a planted logit may overflow a signal on purpose)
                if v.dtype.kind == "f" and not np.isfinite(v).all():
                    _NOT_FINITE.append(f"{what}: {k}")
        else:
            _same_bits(first, got, f"{what}: fill {_fill_name(byte)} (step {step}) against the option off")
    return first


def _run_case(device, n_cu, case):
    run = case.make(device, n_cu)
    model = run.model
    try:
        for label, ids in run.inputs:
            n = len(ids)
            chunks = [0] + ([run.short(n)] if 0 < run.short(n) < n else [])
            if run.id_chunk and run.id_chunk not in chunks:
                chunks.append(run.id_chunk)
            for chunk in chunks:
                what = f"{case.name} / {label} / chunk {chunk}"
                _run_fills(device.set_poison, lambda: model.forward(ids, chunk=chunk), what)
                at_identity = chunk == run.id_chunk
                if run.tap is not None:
                    first = None
                    for byte in pc.TAP_SEQUENCE:
                        device.set_poison(byte)
                        got = {"tap": model.tap(run.tap, ids, chunk=chunk)}
                        if first is None:
                            first = got
                            if at_identity and run.identity is not None:
                                run.identity(model, ids, None)
                        else:
                            _same_bits(first, got, f"{what}: op {run.tap}'s tap under {_fill_name(byte)} against the option off")
                elif at_identity and run.identity is not None:
                    device.set_poison(None)
                    run.identity(model, ids, lambda: model.forward(ids, chunk=chunk))
        _RAN[case.family] = _RAN.get(case.family, 0) + 1
    finally:
        device.set_poison(None)
        device.set_fuse_resblock(True)
        device.set_table_net_lds(False)
        model.close()


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_outputs_do_not_depend_on_the_workspace_fill(device, n_cu, name):
    _guarded(name, lambda: _run_case(device, n_cu, pc.BY_NAME[name]))


def test_the_option_takes_a_byte_or_minus_one(device):
    from jaeger_amd import _lib as L
    for bad in (-2, 256, 1 << 20):
        with pytest.raises(L.JaegerHipError):
            L.check(device.lib.jg_engine_set_option(device.handle, L.JG_OPT_POISON_WORKSPACE, bad), "jg_engine_set_option")
    for ok in (0, 255, 0x7B, -1):
        L.check(device.lib.jg_engine_set_option(device.handle, L.JG_OPT_POISON_WORKSPACE, ok), "jg_engine_set_option")


# ---- the range-guard programs: the fallback's second attempt under every fill -----------------------------------------------------
@pytest.mark.parametrize("name", pc.GUARD_CASES)
def test_range_guard_fallback_under_every_fill(device, name):
    """A fresh handle per fill: its first call trips the guard inside the call, and the second attempt - exact f32 on buffers the
    first attempt left full of Inf and NaN, filled again by the option - equals a handle set to exact f32 before its first call."""
    import resblock_cases as rc
    from jaeger_amd.engine import HipModel
    c = rc.BY_NAME[name.split("/", 1)[1]]

    def body():
        b = rc.build(c)
        device.set_fuse_resblock(True)
        exact = HipModel(device, b.prog)
        try:
            exact.set_precision("f32")
            want = exact.forward(b.ids)
            for k in want:
                assert np.isfinite(want[k]).all(), k
            for byte in pc.SEQUENCE[:4]:
                model = HipModel(device, b.prog)
                try:
                    assert model.precision == "f16x3"
                    device.set_poison(byte)
                    got = model.forward(b.ids)
                    assert model.precision == "f32", f"{name}: the range guard did not trip"
                    _same_bits(want, got, f"{name}: fallback under {_fill_name(byte)} against exact f32 from the start")
                    _same_bits(want, model.forward(b.ids, chunk=max(len(b.ids) - 1, 1)), f"{name}: the call after the fallback, {_fill_name(byte)}")
                finally:
                    device.set_poison(None)
                    model.close()
        finally:
            exact.close()
    _guarded(name, body)


# ---- predict_windows ----------------------------------------------------------------------------------------------------------------
def _brain_engine(scale_first_conv=None, precision=None):
    from conftest import load_model_cfg
    from jaeger_amd.engine import JaegerHipEngine
    from oracle import forward as ofwd
    cfg = load_model_cfg("brain")
    weights = ofwd.random_weights(cfg, seed=38341)
    if scale_first_conv is not None:
        weights["rep/0/kernel"] = weights["rep/0/kernel"] * np.float32(scale_first_conv)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision=precision)


def _brain_windows(n_win=7, fsize=1500, ragged=False, seed=31):
    """One record of ``n_win`` windows: random DNA with N runs and short tandem repeats (DUST masks them)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seq = acgt[rng.integers(0, 4, fsize * n_win)].copy()
    for _ in range(3 * n_win):
        unit = acgt[rng.integers(0, 4, int(rng.integers(1, 4)))]
        length, p = int(rng.integers(20, 160)), int(rng.integers(0, seq.size - 200))
        seq[p:p + length] = np.tile(unit, length // len(unit) + 1)[:length]
    seq[700:740] = ord("N")
    starts = (np.arange(n_win) * fsize).astype(np.int64)
    lens = np.full(n_win, fsize, np.int32)
    if ragged:
        lens[1::3] = rng.integers(fsize // 3, fsize, lens[1::3].size)
    return seq, starts, lens, fsize


@pytest.mark.parametrize("name", pc.PREDICT_CASES)
def test_predict_windows_does_not_depend_on_the_workspace_fill(name):
    streamed = name == "predict/streamed-dust"

    def body():
        eng = _brain_engine()
        try:
            assert eng.model.precision == "f16x3"
            seq, starts, lens, fsize = _brain_windows(ragged=streamed)
            records = np.array([0, seq.size], np.int64) if streamed else None
            if streamed:
                eng.device.set_stream_bytes(8192)
                eng.chunk = 2                       # (groups of whole passes of 2 windows; the call's last pass holds 1)
            else:
                eng.chunk = 3                       # (launch groups of 3, 3 and 1 windows)

            def forward():
                out = eng.predict_windows(seq, starts, lens, fsize, dust_records=records)
                assert (eng.device.stream_stats()["groups"] >= 3) == streamed, eng.device.stream_stats()
                return out
            first = _run_fills(eng.device.set_poison, forward, name)
            assert set(first) == set(pc.OUTPUTS) | {"counts"}
            assert not streamed or eng.dust_masked_total > 0
            assert eng.model.precision == "f16x3"
        finally:
            eng.device.set_poison(None)
            eng.close()
    _guarded(name, body)


# ---- call history on one handle, option off -----------------------------------------------------------------------------------------
#: (which of the family's two row lengths, windows, chunk, arithmetic)
SCHEDULE = ((0, 7, 0, "f16x3"), (1, 1, 0, "f16x3"), (0, 8, 3, "f32"), (1, 7, 3, "f16x3"), (0, 1, 0, "f16x3"), (1, 8, 0, "f16x3"))


def _history_program(family):
    """(program, the two row lengths either side of the family's placement flip)."""
    import op_cases as oc
    import placement_cases as plc
    from jaeger_amd.engine import dicodon_frame_length, frame_length  # noqa: F401
    if family == "legacy":
        from conftest import GOLDEN
        from jaeger_amd import legacy
        return legacy.compile_legacy(legacy.load_legacy_h5(GOLDEN / "legacy_data" / "models" / "default" / "WRes_1024.h5")), (500, 665)
    if family == "mixer_chain":
        import mixer_reference as mx
        cfg = mx.chain_cfg("masked_first")
        return pc.compile_cfg(cfg, mx.random_weights(cfg)), (frame_length(mx.FSIZE), 100)
    cfg, weights = plc.model_and_weights(family)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prog = pc.compile_cfg(cfg, weights)
    # the small-window family: 500 / 755 bp (one fused launch / layer by layer); window-packed tiling: 500 / 665 codons (row-tiled /
    # packed); the two-strand model: inside / beyond the table net's LDS bound
    lengths = {"baseline500": tuple(frame_length(f) for f in plc.MODELS["baseline500"]), "dvf500": plc.MODELS["dvf500"]}.get(family, (500, 665))
    return prog, lengths


def _history_ids(model, prog, l, n_win, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = model.strands if model.strands > 1 else 6
    vocab = 5 if model.strands > 1 else prog.vocab
    ids = rng.integers(1, vocab, (n_win, rows, l))
    ids[rng.random(ids.shape) < 0.02] = 0
    ids[n_win - 1, :, l - l // 3:] = 0                  # a ragged last window
    return ids.astype(np.uint16 if model.wide_ids else np.uint8)


@pytest.mark.parametrize("family", pc.HISTORY_FAMILIES)
def test_call_history_on_one_handle(device, family):
    from jaeger_amd.engine import HipModel

    def body():
        prog, lengths = _history_program(family)
        device.set_poison(None)
        device.set_fuse_resblock(True)
        model = HipModel(device, prog)
        try:
            both = model.precision == "f16x3"           # (a model without a split-f16 program runs the whole schedule in exact f32)
            seen = set()
            for call, (which, n_win, chunk, precision) in enumerate(SCHEDULE):
                precision = precision if both else "f32"
                l = lengths[which]
                ids = _history_ids(model, prog, l, n_win, seed=100 + call)
                model.set_precision(precision)
                got = model.forward(ids, chunk=chunk)
                assert model.precision == precision, (family, call, "the f16 range guard tripped")
                fresh = HipModel(device, prog)
                try:
                    fresh.set_precision(precision)
                    want = fresh.forward(ids, chunk=chunk)
                finally:
                    fresh.close()
                _same_bits(want, got, f"{family}: call {call} (rows of {l}, {n_win} windows, chunk {chunk}, {precision}) against a fresh handle")
                seen.add((which, precision))
            assert not both or seen == {(0, "f16x3"), (1, "f16x3"), (0, "f32")}
            if family == "baseline500":
                assert model.placement()["small_fused"]
        finally:
            model.close()
    _guarded(family, body)


def test_range_guard_fallback_equals_exact_f32_from_the_start():
    """The model of test_gpu_parity.py::test_f16_range_guard_falls_back_to_exact_f32: behind the fallback - whose second attempt
    runs on buffers the first left full of Inf and NaN - every output equals that of a handle in exact f32 from its first call."""
    def body():
        seq, starts, lens, fsize = _brain_windows(n_win=6, seed=9)
        eng = _brain_engine(scale_first_conv=3.0e5)
        try:
            assert eng.model.precision == "f16x3"
            got = eng.predict_windows(seq, starts, lens, fsize)
            assert eng.model.precision == "f32"
            again = eng.predict_windows(seq, starts, lens, fsize)
        finally:
            eng.close()
        eng = _brain_engine(scale_first_conv=3.0e5, precision="f32")
        try:
            want = eng.predict_windows(seq, starts, lens, fsize)
        finally:
            eng.close()
        assert np.isfinite(want["prediction"]).all()
        _same_bits(want, got, "the call that fell back against exact f32 from the start")
        _same_bits(want, again, "the call after the fallback against exact f32 from the start")
    _guarded("history/range-guard-fallback", body)
