"""The multi-scale conv on the GPU (the CPU tier is tests/test_multiscale_reference.py).

Models with ``multi_scale_conv`` layers through ``HipModel.forward`` in both arithmetics of the conv stack, on eight kinds of
windows (``hyena_reference.window_ids``' six, rows with an invalid run every 24 positions, rows of valid islands of one and
two positions).  Five windows at fsize 500 are rows of 165 positions: tiles of 64 + 64 + 37.

* logits, embedding and NMD against the composed float64 reference (tests/multiscale_reference.py: oracle/forward.py's
  layers around the restated layer) at the project's gate of 1e-4; ``chunk=2`` bit for bit the same;
* per MSCONV op: the tensor it writes (``jg_model_set_tap``) against the restatement applied to the op's own read-back input
  and mask, at EVERY position, masked ones included, inside the bound the numpy emulation of the kernel's arithmetic sets
  for that input (4 x its error, rounded up to a power of two);
* per MSMASK op: the mask it writes equals the restated mask of its own read-back input mask at every position, exactly;
* row lengths around the kernel's 64-position tile and window counts through the id-tensor entry point; row isolation; the
  refusals at model creation; describe(); the CLI.

No test here provokes a fault; every test runs under a watchdog that ends the process if a GPU call does not return.
"""
import copy
import faulthandler

import numpy as np
import pytest

import attention_reference as ar
import multiscale_reference as mr
from conftest import GOLDEN, load_model_cfg, make_model_dir
from mixer_reference import mask_writer, producer
from test_gpu_hyena import check_vectors

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
    print("\nmulti-scale conv op against the restatement on its own input, every position (errors in units of the output's rms):")
    for row in _TABLE:
        print("  " + row)


def ops_of_kind(prog, kind):
    return [i for i, op in enumerate(prog.ops) if op.kind == kind]


def layers_of(cfg, prog):
    """[(op index, weight prefix, the layer's parameters)] of every multi-scale conv op, in program order."""
    from jaeger_amd import _lib as L
    out = [(f"rep/{i}", mr.params_of(a)) for i, kind, a in mr.mixer_layers(cfg) if kind == mr.MSCONV]
    ops = ops_of_kind(prog, L.OP_MSCONV)
    assert len(out) == len(ops)
    return [(i, prefix, p) for i, (prefix, p) in zip(ops, out)]


def check_op(eng, weights, i, prefix, params, ids, what):
    """The MSCONV op's own output from its own read-back input and mask, every position inside the emulation's bound; and
    the MSMASK op in front of it, exactly.  Returns how many positions the op's output mask leaves invalid."""
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
    cout = mr.out_channels(params)
    assert y.shape == (w_, fr, l, cout) and (op.cin, op.k, op.cout, op.arg) == (c, len(params["branches"]), cout, int(params["merge"] == "add"))
    rows = lambda a: None if a is None else a.reshape((w_ * fr, l) + a.shape[3:])
    lw = ar.sub_weights(weights, prefix)
    want, want_mask = mr.rows_op(rows(x), rows(mask), lw, params)
    emu = mr.emulate(rows(x), lw, params, rows(mask))
    n_invalid = 0
    if want_mask is None:
        assert op.out_mask == L.JG_BUF_NONE and (mask is None or not params["branches"][0]["use_masking"])
        assert i == 0 or prog.ops[i - 1].kind != L.OP_MSMASK
    else:
        mop = prog.ops[i - 1]
        assert mop.kind == L.OP_MSMASK and mop.out_mask == op.out_mask and mop.in_mask == op.in_mask and mop.w_off == op.w_off
        got_mask = rows(eng.model.tap(i - 1, ids) != 0)
        np.testing.assert_array_equal(got_mask, want_mask, err_msg=f"{what} op {i - 1}: the layer's output mask")
        n_invalid = int((~want_mask).sum())
    got = rows(y)
    want = ar.apply_stages(want, prog, op)
    emu = ar.apply_stages(emu, prog, op, dtype=np.float32)
    b = ar.bounds_from(emu, want)
    e, r = ar.errors(got, want)
    n_masked = 0 if mask is None else int((~mask).sum())
    _TABLE.append(f"{what:44s} op {i:2d} L {l:3d} ({n_masked:4d} masked in, {n_invalid:4d} out): max {e:.3g} (emulation {b['emu_elem']:.3g}, "
                  f"bound {b['elem']:.3g}), rms {r:.3g} (emulation {b['emu_rms']:.3g}, bound {b['rms']:.3g})")
    print(_TABLE[-1])
    assert np.isfinite(got).all() and e <= b["elem"] and r <= b["rms"], _TABLE[-1]
    return n_invalid


@pytest.mark.parametrize("name", mr.VARIANTS)
def test_model_outputs_and_multiscale_ops(name):
    """Both arithmetics of the conv stack: the program's own default (split-f16 where the convs have such a program) and
    exact f32."""
    from jaeger_amd.engine import JaegerHipEngine
    cfg = mr.variant(name)
    weights = mr.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0)
    try:
        precisions = [eng.model.precision] + (["f32"] if eng.model.precision != "f32" else [])
        if name in ("fixture", "then_conv", "wide"):
            assert precisions == ["f16x3", "f32"], precisions
        assert not eng.model.placement()["small_fused"]
        ops = layers_of(cfg, eng.program)
        assert "multi-scale conv" in eng.model.describe()
        invalid = 0
        refs = {kind: mr.forward(cfg, weights, mr.ids_of(kind)) for kind in mr.KINDS}     # once, for both arithmetics
        for precision in precisions:
            eng.model.set_precision(precision)
            assert eng.model.precision == precision
            for kind in mr.KINDS:
                what = f"{name} / {precision} / {kind}"
                ids = mr.ids_of(kind)
                got = eng.model.forward(ids)
                errs = check_vectors(what, got, refs[kind])
                print(what, {k: f"{v:.2e}" for k, v in errs.items()})
                split = eng.model.forward(ids, chunk=2)               # launch groups of 2 + 2 + 1 windows: bit for bit the same
                for k in got:
                    np.testing.assert_array_equal(got[k], split[k], err_msg=f"{what} {k}: chunk 2")
                for i, prefix, params in ops:
                    invalid += check_op(eng, weights, i, prefix, params, ids, what)
        if name not in ("behind_cross", "unmasked"):
            assert invalid > 0, "no position was invalid behind the layer"
    finally:
        eng.close()


# ---- row lengths --------------------------------------------------------------------------------------------------------
def minimal_cfg() -> dict:
    """embedding -> multi_scale_conv (the fixture's three branches) -> batch norm -> gelu -> masked average pool -> dense."""
    cfg = mr.variant("fixture")
    rep = cfg["representation_learner"]
    rep["hidden_layers"] = rep["hidden_layers"][:3]
    return cfg


def _ragged_ids(l, n_win):
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
    weights = mr.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision="f32")
    yield cfg, weights, eng
    eng.close()


@pytest.mark.parametrize("l, n_win", [(l, 3) for l in (1, 2, 63, 64, 65, 127, 128, 129, 166)] + [(65, 1), (65, 7)])
def test_row_lengths_and_window_counts(length_model, l, n_win):
    """Rows of ``l`` positions, the last window ragged: a single position, one under / at / over one and two tiles (the halo
    crosses the tile border, the last tile is ragged), the fixture's 166; 1 and 7 windows."""
    from jaeger_amd import _lib as L
    cfg, weights, eng = length_model
    assert L.load().jg_msconv_tile() == L.MSCONV_TILE == mr.TILE
    ids = _ragged_ids(l, n_win)
    what = f"row length {l}, {n_win} windows"
    got = eng.model.forward(ids)
    errs = check_vectors(what, got, mr.forward(cfg, weights, ids))
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    for i, prefix, params in layers_of(cfg, eng.program):
        check_op(eng, weights, i, prefix, params, ids, what)


def test_rows_do_not_see_their_neighbours():
    """The middle row's tiles are neighbours of other rows' tiles in the launch grid and in memory.  With values of 1e30 in
    every other row its output is bit for bit what it is without them."""
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import JaegerHipEngine
    cfg = minimal_cfg()
    weights = mr.random_weights(cfg)
    huge_id = 64
    weights_huge = dict(weights)
    weights_huge["embedding/embeddings"] = weights["embedding/embeddings"].copy()
    weights_huge["embedding/embeddings"][huge_id] = 1e30
    for l in (mr.TILE, 2 * mr.TILE + 5):
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
                op = ops_of_kind(eng.program, L.OP_MSCONV)[-1]
                outs.append(eng.model.tap(op, tensor)[mid[0], mid[1]])
                if wts is weights_huge:
                    x = eng.model.tap(producer(eng.program, op), tensor)
                    assert np.abs(x[0, 2, -1]).max() > 1e28 and np.abs(x[0, 4, 0]).max() > 1e28      # the neighbours do hold them
            finally:
                eng.close()
        assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
        np.testing.assert_array_equal(outs[0], outs[1], err_msg=f"L {l}: the middle row changed with its neighbours")


def test_bad_ops_are_refused_at_model_creation():
    """The plan refuses them first; a program that reaches the library anyway is refused there, with the reason: sizes, a
    corrupted descriptor, in-place slots."""
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd.engine import HipDevice, HipModel
    from jaeger_amd.program import compile_plan
    cfg = mr.variant("fixture")
    prog = compile_plan(P.build_plan(cfg), mr.random_weights(cfg))
    i = ops_of_kind(prog, L.OP_MSCONV)[0]
    im = ops_of_kind(prog, L.OP_MSMASK)[0]
    w0 = prog.ops[i].w_off
    dev = HipDevice(0)
    try:
        def refused(word, at=i, blob=None, **fields):
            bad = copy.copy(prog)
            bad.ops = list(prog.ops)
            op = L.JgOp.from_buffer_copy(prog.ops[at])
            for field, value in fields.items():
                setattr(op, field, value)
            bad.ops[at] = op
            if blob is not None:
                bad.blob = blob
            with pytest.raises(L.JaegerHipError, match=word):
                HipModel(dev, bad)

        def descriptor(branch, field, value):
            blob = prog.blob.copy()
            blob[w0 + branch * L.MSCONV_DESC_FIELDS + field:][:1].view(np.int32)[0] = value
            return blob

        refused("24 incoming channels", cin=24)
        refused("144 incoming channels", cin=144)
        refused("5 branches", k=5)
        refused("0 branches", k=0)
        refused("merge kind 2", arg=2)
        refused("40 output channels", cout=40)
        refused("in place", out_buf=prog.ops[i].in_buf)
        refused("outside the weight blob", w_off=len(prog.blob))
        refused("reads one mask slot and writes another", at=im, out_mask=prog.ops[im].in_mask)
        refused("12 filters", blob=descriptor(0, 0, 12))
        refused("kernel_size 16", blob=descriptor(1, 1, 16))
        refused(r"\(kernel_size - 1\) x dilation_rate = 66", blob=descriptor(2, 2, 33))
        refused("mask mode 3", blob=descriptor(0, 4, 3))
        refused("channel offset 8", blob=descriptor(1, 6, 8))
        refused("outside the blob", blob=descriptor(2, 7, len(prog.blob)))
        refused("outside the blob", blob=descriptor(0, 7, -4))
        refused("for 64 output channels", blob=descriptor(2, 0, 16))
    finally:
        dev.close()


def test_cli_predict_multiscale_model(tmp_path, monkeypatch):
    """``python -m jaeger_amd predict`` with a multiscale500 model directory (fixture yaml, classes file, .weights.npz) against
    the reference composition, as tests/test_gpu_bilstm.py does it for the bilstm model."""
    from click.testing import CliRunner

    import test_gpu_cli as tc
    from jaeger_amd.cli import main
    from jaeger_amd.fragment import read_fasta
    from jaeger_amd.weights import load_npz
    from oracle import forward as ofwd
    root = make_model_dir(tmp_path / "m", name="multiscale500")
    cfg = load_model_cfg("multiscale500")
    weights = load_npz(next((root / "model").glob("*.weights.npz")))
    assert set(weights) == set(mr.weight_specs(cfg))
    fasta = GOLDEN / "test_contigs.fasta"
    r = CliRunner().invoke(main, ["predict", "-i", str(fasta), "-o", str(tmp_path / "out"), "--model_path", str(root),
                                  "--fsize", "500", "--stride", "500", "--no-dustmask"])
    assert r.exit_code == 0, r.output
    tsv = list((tmp_path / "out").rglob("test_contigs.tsv"))
    assert len(tsv) == 1, list((tmp_path / "out").rglob("*"))
    monkeypatch.setattr(ofwd, "forward", lambda c, w, ids, dtype=None: {
        k: v.astype(np.float32) for k, v in mr.forward(c, w, ids).items()})
    records = [(n, s.decode()) for n, s in read_fasta(str(fasta))]
    exp, _, _ = tc._expected(tmp_path, records, cfg, weights, 500, 500, None, 96)
    tc._compare_tsv(tsv[0], exp)
