"""The bidirectional LSTM on the GPU (the CPU tier is tests/test_bilstm_reference.py).

Models with ``masked_bilstm`` layers through ``HipModel.forward`` in both arithmetics of the conv stack, on seven kinds of
windows (full, ragged tail, nearly empty, an N run in the middle, rows that START with invalid positions, rows with no valid
position at all, rows with an invalid run every 24 positions):

* logits, embedding and NMD against the composed float64 reference (tests/bilstm_reference.py: oracle/forward.py's layers
  around the restated layer) at the project's gate of 1e-4; ``chunk=2`` bit for bit the same (the rows of one 16-row group
  then come from other windows);
* per op: the tensor every bilstm op writes (``jg_model_set_tap``) against the restatement applied to the op's own read-back
  input and mask, at EVERY position, inside the bound the numpy emulation of the kernel's arithmetic sets for that input
  (4 x its error, rounded up to a power of two); where the store carries no stage, masked positions hold bit for bit the
  forward half of the nearest valid position before them and the backward half of the nearest one behind (zeros if none);
* row lengths around the kernel's time block (``_lib.BILSTM_STEPS``) and window counts around its 16-row group through the
  id-tensor entry point; row isolation; the two directions; the refusals at model creation; the CLI.

No test here provokes a fault; every test runs under a watchdog that ends the process if a GPU call does not return.
"""
import copy
import faulthandler

import numpy as np
import pytest

import attention_reference as ar
import bilstm_reference as br
from conftest import GOLDEN, load_model_cfg, make_model_dir
from mixer_reference import producer
from test_gpu_hyena import check_vectors, mask_writer

pytestmark = pytest.mark.gpu

_TABLE = []


@pytest.fixture(autouse=True)
def _watchdog():
    faulthandler.dump_traceback_later(900, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nbilstm op against the restatement on its own input, every position (errors in units of the output's rms):")
    for row in _TABLE:
        print("  " + row)


def bilstm_ops(prog):
    from jaeger_amd import _lib as L
    return [i for i, op in enumerate(prog.ops) if op.kind == L.OP_BILSTM]


def layers_of(cfg, prog):
    """[(op index, weight prefix, the layer's parameters)] of every bilstm op, in program order."""
    out = [(f"rep/{i}", br.params_of(a)) for i, kind, a in br.mixer_layers(cfg) if kind == br.BILSTM]
    ops = bilstm_ops(prog)
    assert len(out) == len(ops)
    return [(i, prefix, p) for i, (prefix, p) in zip(ops, out)]


def check_op(eng, weights, i, prefix, params, ids, what):
    """The op's own output from its own read-back input and mask: every position inside the emulation's bound; masked ones
    bit for bit the carried values (where the store carries no stage).  Returns how many masked positions were held so."""
    from jaeger_amd import _lib as L
    prog = eng.program
    op = prog.ops[i]
    x = eng.model.tap(producer(prog, i), ids)
    mw = mask_writer(prog, i)
    mask = None if mw is None else eng.model.tap(mw, ids) != 0
    y = eng.model.tap(i, ids)
    bits = eng.model.tap_variant()
    assert bits & L.TAP_EXACT_F32 and not bits & (L.TAP_F16S | L.TAP_PHASE_SPLIT), (what, bits)
    w_, fr, l, c = x.shape
    u = params["units"]
    assert y.shape == (w_, fr, l, 2 * u) and (op.cin, op.k, op.cout, op.arg & 1) == (c, u, 2 * u, int(params["ignore_mask"]))
    rows = lambda a: None if a is None else a.reshape((w_ * fr, l) + a.shape[3:])
    lw = ar.sub_weights(weights, prefix)
    want = br.bilstm(rows(x), lw, rows(mask), params["ignore_mask"])
    emu = br.emulate(rows(x), lw, rows(mask), params["ignore_mask"])
    got = rows(y)
    seen = rows(mask) if (mask is not None and not params["ignore_mask"]) else None
    n_masked = 0 if seen is None else int((~seen).sum())
    held = 0
    if op.n_stages == 0 and seen is not None:
        assert np.array_equal(got, br.carried_expectation(got, seen)), f"{what} op {i}: masked positions do not hold the carried values"
        held = n_masked
    want = ar.apply_stages(want, prog, op)
    emu = ar.apply_stages(emu, prog, op, dtype=np.float32)
    b = ar.bounds_from(emu, want)
    e, r = ar.errors(got, want)
    _TABLE.append(f"{what:40s} op {i:2d} L {l:3d} ({n_masked:4d} masked): max {e:.3g} (emulation {b['emu_elem']:.3g}, bound {b['elem']:.3g}), "
                  f"rms {r:.3g} (emulation {b['emu_rms']:.3g}, bound {b['rms']:.3g})")
    print(_TABLE[-1])
    assert np.isfinite(got).all() and e <= b["elem"] and r <= b["rms"], _TABLE[-1]
    return held


@pytest.mark.parametrize("name", br.VARIANTS)
def test_model_outputs_and_bilstm_ops(name):
    """Both arithmetics of the conv stack: the program's own default (split-f16 where the convs have such a program) and
    exact f32.  16-channel convs have no split-f16 tile, and the fixture must have one."""
    from jaeger_amd.engine import JaegerHipEngine
    cfg = br.variant(name)
    weights = br.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0)
    try:
        precisions = [eng.model.precision] + (["f32"] if eng.model.precision != "f32" else [])
        if name in ("fixture", "u64", "stacked", "then_conv"):
            assert precisions == ["f16x3", "f32"], precisions
        assert not eng.model.placement()["small_fused"]
        ops = layers_of(cfg, eng.program)
        assert "bilstm" in eng.model.describe()
        held = 0
        refs = {kind: br.forward(cfg, weights, br.ids_of(kind, name)) for kind in br.KINDS}     # once, for both arithmetics
        for precision in precisions:
            eng.model.set_precision(precision)
            assert eng.model.precision == precision
            for kind in br.KINDS:
                what = f"{name} / {precision} / {kind}"
                ids = br.ids_of(kind, name)
                got = eng.model.forward(ids)
                errs = check_vectors(what, got, refs[kind])
                print(what, {k: f"{v:.2e}" for k, v in errs.items()})
                split = eng.model.forward(ids, chunk=2)               # launch groups of 2 + 2 + 1 windows: bit for bit the same
                for k in got:
                    np.testing.assert_array_equal(got[k], split[k], err_msg=f"{what} {k}: chunk 2")
                for i, prefix, params in ops:
                    held += check_op(eng, weights, i, prefix, params, ids, what)
        if name in ("stacked", "ln_tail"):
            assert held > 0, "no masked position reached an op without fused stages"
    finally:
        eng.close()


# ---- row lengths --------------------------------------------------------------------------------------------------------
def minimal_cfg(**over) -> dict:
    """embedding -> masked 3-tap conv ('same': the rows keep their length) -> batch norm -> gelu -> masked_bilstm -> batch norm
    -> average pool -> dense."""
    cfg = br.with_bilstm_config(load_model_cfg("bilstm500"), **over)
    layers = cfg["representation_learner"]["hidden_layers"]
    lstm = [l for l in layers if l["name"] == br.BILSTM][0]
    front = [{"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same")},
             {"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]
    cfg["representation_learner"]["hidden_layers"] = front + [lstm, {"name": "masked_batchnorm", "config": {}}]
    return cfg


def _cases():
    from jaeger_amd._lib import BILSTM_STEPS as S
    lengths = sorted({1, 2, S - 1, S, S + 1, 2 * S + 3, 166})
    return [(l, n) for l in lengths for n in (1, 3, 11)] + [(665, 1)]


def _ragged_ids(l, n_win=3):
    rng = np.random.Generator(np.random.PCG64(l))
    ids = rng.integers(1, 65, (n_win, 6, l)).astype(np.uint8)
    for f in range(6):
        ids[n_win - 1, f, max(l - 1 - 3 * f, 1):] = 0           # frame 0 keeps all but its last position (l = 1: all of it)
        if l > 30:
            ids[n_win - 1, f, 5 + f:5 + f + 9] = 0               # an invalid run inside
    return ids


@pytest.fixture(scope="module")
def length_model():
    from jaeger_amd.engine import JaegerHipEngine
    cfg = minimal_cfg()
    weights = br.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision="f32")
    yield cfg, weights, eng
    eng.close()


@pytest.mark.parametrize("l, n_win", _cases())
def test_row_lengths_and_row_counts(length_model, l, n_win):
    """Rows of ``l`` positions, the last window ragged: a single position, a ragged last time block, one block alone, a second
    and a third, the longest row the short-contig pass meets; 6 rows (under one 16-row group), 18 (a ragged second group)
    and 66."""
    from jaeger_amd import _lib as L
    cfg, weights, eng = length_model
    assert L.load().jg_bilstm_rows() == L.BILSTM_ROWS == 16 and L.load().jg_bilstm_steps() == L.BILSTM_STEPS
    ids = _ragged_ids(l, n_win=n_win)
    what = f"row length {l}, {n_win} windows"
    got = eng.model.forward(ids)
    errs = check_vectors(what, got, br.forward(cfg, weights, ids))
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    for i, prefix, params in layers_of(cfg, eng.program):
        check_op(eng, weights, i, prefix, params, ids, what)


def test_rows_do_not_see_their_neighbours():
    """The middle row shares its 16-row group - one block of the matrix cores, one LDS tile - with eleven others.  With
    values of 1e30 in every other row its output is bit for bit what it is without them."""
    from jaeger_amd._lib import BILSTM_STEPS as S
    from jaeger_amd.engine import JaegerHipEngine
    cfg = minimal_cfg()
    layers = cfg["representation_learner"]["hidden_layers"]
    cfg["representation_learner"]["hidden_layers"] = layers[:1] + layers[3:]     # conv -> bilstm: the huge values arrive as they are
    weights = br.random_weights(cfg)
    huge_id = 64
    weights_huge = dict(weights)
    weights_huge["embedding/embeddings"] = weights["embedding/embeddings"].copy()
    weights_huge["embedding/embeddings"][huge_id] = 1e30
    for l in (S, 2 * S + 5):
        rng = np.random.Generator(np.random.PCG64(l))
        ids = rng.integers(1, 64, (2, 6, l)).astype(np.uint8)           # (ids 1 .. 63: id 64 only where it is put)
        marked = ids.copy()
        mid = (0, 3)
        for w in range(2):
            for f in range(6):
                if (w, f) != mid:
                    marked[w, f, :] = huge_id
        outs = []
        for wts, tensor in ((weights, ids), (weights_huge, marked)):
            eng = JaegerHipEngine(model_cfg=cfg, weights=wts, device_id=0, precision="f32")
            try:
                op = bilstm_ops(eng.program)[-1]
                assert eng.program.ops[op].n_stages == 1
                outs.append(eng.model.tap(op, tensor)[mid[0], mid[1]])
                if wts is weights_huge:
                    x = eng.model.tap(producer(eng.program, op), tensor)
                    assert np.abs(x[0, 2, -1]).max() > 1e28 and np.abs(x[0, 4, 0]).max() > 1e28      # the neighbours do hold them
            finally:
                eng.close()
        assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
        np.testing.assert_array_equal(outs[0], outs[1], err_msg=f"L {l}: the middle row changed with its neighbours")


def test_the_two_directions_on_the_first_layer_model():
    """Changing the ids from t0 on - other codons, and invalid ones - leaves the forward half in front of t0 bit for bit;
    changing them in front of t0 leaves the backward half from t0 on bit for bit; the other half does change."""
    from jaeger_amd.engine import JaegerHipEngine
    cfg = br.variant("first")
    weights = br.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision="f32")
    try:
        op = bilstm_ops(eng.program)[0]
        u = eng.program.ops[op].k
        ids = br.ids_of("n_run", "first", n_win=3)
        l = ids.shape[2]
        base = eng.model.tap(op, ids)
        for t0 in (1, 15, 16, 17, 130):
            rng = np.random.Generator(np.random.PCG64(t0))
            behind = ids.copy()
            behind[:, :, t0:] = rng.integers(0, 65, (3, 6, l - t0))
            got = eng.model.tap(op, behind)
            np.testing.assert_array_equal(got[:, :, :t0, :u], base[:, :, :t0, :u], err_msg=f"forward half, t0 {t0}")
            assert np.abs(got[:, :, :t0, u:] - base[:, :, :t0, u:]).max() > 1e-3
            front = ids.copy()
            front[:, :, :t0] = rng.integers(0, 65, (3, 6, t0))
            got = eng.model.tap(op, front)
            np.testing.assert_array_equal(got[:, :, t0:, u:], base[:, :, t0:, u:], err_msg=f"backward half, t0 {t0}")
            assert np.abs(got[:, :, t0:, :u] - base[:, :, t0:, :u]).max() > 1e-3
    finally:
        eng.close()


def test_flops_per_window_counts_the_two_matrix_products_of_both_directions():
    from jaeger_amd.engine import JaegerHipEngine
    cfg = br.variant("first")
    eng = JaegerHipEngine(model_cfg=cfg, weights=br.random_weights(cfg), device_id=0)
    try:
        for l in (1, 166, 665):
            identity = 2.0 * 64 * 64 * 6 * l
            want = identity + 6 * l * 2 * (2.0 * 64 * 4 * 32 + 2.0 * 32 * 4 * 32)
            assert eng.model.flops_per_window(l) == want, (l, eng.model.flops_per_window(l), want)
    finally:
        eng.close()


def test_bad_ops_are_refused_at_model_creation():
    """The plan refuses them first; a program that reaches the library anyway is refused there, with the reason."""
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd.engine import HipDevice, HipModel
    from jaeger_amd.program import compile_plan
    cfg = br.variant("fixture")
    prog = compile_plan(P.build_plan(cfg), br.random_weights(cfg))
    i = bilstm_ops(prog)[0]
    dev = HipDevice(0)
    try:
        for field, value, word in (("k", 48, "48 units"), ("k", 128, "128 units"), ("cout", 32, "32 output channels"),
                                   ("cin", 24, "24 incoming channels"), ("cin", 144, "144 incoming channels"),
                                   ("out_buf", prog.ops[i].in_buf, "in place"), ("arg", 2, "bilstm flags 2"),
                                   ("arg", 1, "out_mask against arg"), ("out_mask", L.JG_BUF_NONE, "out_mask against arg"),
                                   ("w_off", len(prog.blob), "outside the weight blob")):
            bad = copy.copy(prog)
            bad.ops = list(prog.ops)
            op = L.JgOp.from_buffer_copy(prog.ops[i])
            setattr(op, field, value)
            bad.ops[i] = op
            with pytest.raises(L.JaegerHipError, match=word):
                HipModel(dev, bad)
    finally:
        dev.close()


def test_cli_predict_bilstm_model(tmp_path, monkeypatch):
    """``python -m jaeger_amd predict`` with a bilstm500 model directory (fixture yaml, classes file, .weights.npz) against
    the reference composition, as tests/test_gpu_hyena.py does it for the hyena model."""
    from click.testing import CliRunner

    import test_gpu_cli as tc
    from jaeger_amd.cli import main
    from jaeger_amd.fragment import read_fasta
    from jaeger_amd.weights import load_npz
    from oracle import forward as ofwd
    root = make_model_dir(tmp_path / "m", name="bilstm500")
    cfg = load_model_cfg("bilstm500")
    weights = load_npz(next((root / "model").glob("*.weights.npz")))
    assert set(weights) == set(br.weight_specs(cfg))
    fasta = GOLDEN / "test_contigs.fasta"
    r = CliRunner().invoke(main, ["predict", "-i", str(fasta), "-o", str(tmp_path / "out"), "--model_path", str(root),
                                  "--fsize", "500", "--stride", "500", "--no-dustmask"])
    assert r.exit_code == 0, r.output
    tsv = list((tmp_path / "out").rglob("test_contigs.tsv"))
    assert len(tsv) == 1, list((tmp_path / "out").rglob("*"))
    monkeypatch.setattr(ofwd, "forward", lambda c, w, ids, dtype=None: {
        k: v.astype(np.float32) for k, v in br.forward(c, w, ids).items()})
    records = [(n, s.decode()) for n, s in read_fasta(str(fasta))]
    exp, _, _ = tc._expected(tmp_path, records, cfg, weights, 500, 500, None, 96)
    tc._compare_tsv(tsv[0], exp)
