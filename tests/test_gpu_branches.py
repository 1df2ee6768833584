"""``parallel_branches`` of pooled branches and last pooling on the GPU (the CPU tier is tests/test_branches_reference.py).

Models through ``HipModel.forward`` in both arithmetics of the conv stack, on five kinds of windows at fsize 500 (three windows
of 165 codons a frame): ``full``; ``long_n`` - a run of N inside the row, so that ``count - 1`` is not the last valid index;
``tail_n`` - trailing padding; ``empty_row`` - one frame all invalid; ``empty_window`` - every frame invalid, so zeros.

* logits and embedding against the composed float64 reference (tests/branches_reference.py) at the project's gate of 1e-4;
  ``chunk=2`` bit for bit the same; no ``nmd`` output;
* per POOLVEC op: from the op's own read-back input tensor and mask (``jg_model_set_tap`` on their producers) the pooled
  vector in float64 and in a float32 emulation of the kernel's sum order, merged by the layer's rule, against the
  ``embedding`` the model returns.  A max pool under STORE selects one of its float32 inputs: bit equality with the float64
  reference.  A last pool under STORE adds the rows of up to six frames and divides once, so it selects only where one frame
  is valid: bit equality with the float32 evaluation of that sum in frame order (and with the rounded float64 reference
  wherever one frame is valid).  Average pools and the add / max / scaled merges: inside 4 x the emulation's own error;
* branches of one conv each at row lengths 1, 2, 63, 64, 65 and 165 and 1, 3 and 70 windows; window isolation; the refusals
  at model creation; describe(); the CLI.

No test here provokes a fault; every test runs under a watchdog that ends the process if a GPU call does not return.
"""
import copy
import faulthandler

import numpy as np
import pytest
import torch

import attention_reference as ar
import branches_reference as xr
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
    print("\npool-and-merge ops against the reference on their own inputs (errors in units of the vector's rms):")
    for row in _TABLE:
        print("  " + row)


def poolvecs(prog):
    from jaeger_amd import _lib as L
    return [i for i, op in enumerate(prog.ops) if op.kind == L.OP_POOLVEC]


def check_poolvecs(eng, ids, embedding, what):
    """Every POOLVEC op of the program from its own tapped input and mask; returns how many positions the pools saw masked."""
    from jaeger_amd import _lib as L
    prog = eng.program
    kinds = {L.POOL_MAX: "max", L.POOL_AVG: "average", L.POOL_LAST: "last"}
    ops = poolvecs(prog)
    assert ops
    want, emu, n_masked = [], [], 0
    for i in ops:
        op = prog.ops[i]
        x = eng.model.tap(producer(prog, i), ids)
        mw = mask_writer(prog, i)
        mask = None if mw is None else eng.model.tap(mw, ids) != 0
        assert x.shape[3] == op.cout and (mask is None or mask.shape == x.shape[:3])
        n_masked += 0 if mask is None else int((~mask).sum())
        kind = kinds[op.arg]
        tm = None if mask is None else torch.as_tensor(mask.astype(np.float64))
        want.append(xr.pool(torch.as_tensor(x.astype(np.float64)), tm, kind).numpy())
        emu.append(xr.emulate_pool(x, mask, kind))
        if op.k == L.POOLVEC_STORE and op.f0 == 1.0 and len({o for o in ops if prog.ops[o].vec_off == op.vec_off}) == 1:
            got = embedding[:, op.vec_off:op.vec_off + op.cout]               # nothing is merged into this range later
            if kind == "max":
                np.testing.assert_array_equal(got, want[-1].astype(np.float32), err_msg=f"{what} op {i}: max under STORE")
            if kind == "last":
                np.testing.assert_array_equal(got, emu[-1], err_msg=f"{what} op {i}: last under STORE")
                one = np.ones(len(x), bool) if mask is None else (mask.any(-1).sum(-1) <= 1)
                if mask is not None:
                    np.testing.assert_array_equal(got[one], want[-1].astype(np.float32)[one], err_msg=f"{what} op {i}: last selects")
    stores = [prog.ops[i].k == L.POOLVEC_STORE for i in ops]
    how = "concat" if all(stores) else "max" if prog.ops[ops[1]].k == L.POOLVEC_MAX else \
        "average" if np.float32(prog.ops[ops[-1]].f0) != 1.0 else "sum"
    assert how == "concat" or (stores[0] and not any(stores[1:]))
    ref = xr.merge([torch.as_tensor(v) for v in want], how).numpy()
    em = xr.emulate_merge(emu, how)
    assert embedding.shape == ref.shape, (what, embedding.shape, ref.shape)
    b = ar.bounds_from(em, ref)
    e, r = ar.errors(embedding, ref)
    _TABLE.append(f"{what:44s} {len(ops)} ops {how:7s} ({n_masked:5d} masked): max {e:.3g} (emulation {b['emu_elem']:.3g}, bound {b['elem']:.3g}), "
                  f"rms {r:.3g} (emulation {b['emu_rms']:.3g}, bound {b['rms']:.3g})")
    print(_TABLE[-1])
    assert np.isfinite(embedding).all() and e <= b["elem"] and r <= b["rms"], _TABLE[-1]
    return n_masked


@pytest.mark.parametrize("name", list(xr.VARIANTS))
def test_model_outputs_and_poolvec_ops(name):
    """Both arithmetics of the conv stack: the program's own default (split-f16 where the convs have such a program) and
    exact f32."""
    from jaeger_amd.engine import JaegerHipEngine
    cfg = xr.variant(name)
    weights = xr.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0)
    try:
        precisions = [eng.model.precision] + (["f32"] if eng.model.precision != "f32" else [])
        if name in ("fixture", "four_branches", "merge_average", "pool_last"):
            assert precisions == ["f16x3", "f32"], precisions
        assert not eng.model.placement()["small_fused"]
        assert "pool-and-merge" in eng.model.describe()
        refs = {kind: xr.forward(cfg, weights, xr.ids_of(kind)) for kind in xr.WINDOW_KINDS}     # once, for both arithmetics
        masked = 0
        for precision in precisions:
            eng.model.set_precision(precision)
            assert eng.model.precision == precision
            for kind in xr.WINDOW_KINDS:
                what = f"{name} / {precision} / {kind}"
                ids = xr.ids_of(kind)
                got = eng.model.forward(ids)
                assert set(got) == {"prediction", "embedding"}, (what, sorted(got))
                errs = check_vectors(what, got, refs[kind])
                print(what, {k: f"{v:.2e}" for k, v in errs.items()})
                split = eng.model.forward(ids, chunk=2)               # launch groups of 2 + 1 windows: bit for bit the same
                for k in got:
                    np.testing.assert_array_equal(got[k], split[k], err_msg=f"{what} {k}: chunk 2")
                masked += check_poolvecs(eng, ids, got["embedding"], what)
                if kind == "empty_window":
                    assert not got["embedding"][1].any(), f"{what}: the empty window does not pool to zeros"
        assert masked > 0, "no position was masked in front of a pool"
    finally:
        eng.close()


# ---- row lengths --------------------------------------------------------------------------------------------------------
def conv_branches_cfg() -> dict:
    """embedding -> 3-tap conv (same) -> three branches of ONE conv each (same padding, so rows of one position run): 3 taps ->
    max, 5 taps d2 -> last, 1 tap -> average; concat; dense."""
    conv = lambda k, d=1: {"name": "masked_conv1d", "config": dict(filters=32, kernel_size=k, padding="same", dilation_rate=d)}
    cfg = xr.branches_cfg([xr._branch([conv(3)], "max"), xr._branch([conv(5, 2)], "last"), xr._branch([conv(1)], "average")])
    rep = cfg["representation_learner"]
    rep["hidden_layers"] = [conv(3)] + rep["hidden_layers"][-1:]
    return cfg


def _ragged_ids(l, n_win):
    rng = np.random.Generator(np.random.PCG64(l))
    ids = rng.integers(1, 65, (n_win, 6, l)).astype(np.uint8)
    for f in range(6):
        ids[n_win - 1, f, max(l - 1 - 3 * f, 1):] = 0           # frame 0 keeps all but its last position (l = 1: all of it)
        if l > 30:
            ids[n_win - 1, f, 5 + f:5 + f + 19] = 0              # an invalid run inside that outlasts the convs
    if n_win > 2:
        ids[1, 4] = 0                                            # an empty frame
    return ids


@pytest.fixture(scope="module")
def length_model():
    from jaeger_amd.engine import JaegerHipEngine
    cfg = conv_branches_cfg()
    weights = xr.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision="f32")
    yield cfg, weights, eng
    eng.close()


@pytest.mark.parametrize("l, n_win", [(l, 3) for l in (1, 2, 63, 64, 65, 165)] + [(65, 1), (65, 70)])
def test_row_lengths_and_window_counts(length_model, l, n_win):
    """Rows of ``l`` positions: one and two (fewer than a wave's 64 lanes, fewer positions than position groups), one under /
    at / over the 64 lanes the count reduction strides by, the fixture's 165; 1, 3 and 70 windows."""
    cfg, weights, eng = length_model
    ids = _ragged_ids(l, n_win)
    what = f"row length {l}, {n_win} windows"
    got = eng.model.forward(ids)
    errs = check_vectors(what, got, xr.forward(cfg, weights, ids))
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    check_poolvecs(eng, ids, got["embedding"], what)


@pytest.mark.parametrize("name", ["pool_last", "merge_sum"])
def test_windows_do_not_see_their_neighbours(name):
    """Changing window 1 leaves windows 0 and 2 bit for bit as they were: the read-modify-write of a merge stays inside its
    window's row of the vector."""
    from jaeger_amd.engine import JaegerHipEngine
    cfg = xr.variant(name)
    eng = JaegerHipEngine(model_cfg=cfg, weights=xr.random_weights(cfg), device_id=0)
    try:
        ids = xr.ids_of("tail_n")
        other = ids.copy()
        other[1] = np.random.Generator(np.random.PCG64(1)).integers(1, 65, ids[1].shape)
        other[1, 3, 40:] = 0
        a, b = eng.model.forward(ids), eng.model.forward(other)
        for k in a:
            assert not np.array_equal(a[k][1], b[k][1]), k
            np.testing.assert_array_equal(a[k][[0, 2]], b[k][[0, 2]], err_msg=f"{name} {k}: windows 0 / 2 changed with window 1")
    finally:
        eng.close()


def test_bad_ops_are_refused_at_model_creation():
    """The plan refuses them first; a program that reaches the library anyway is refused there, with the reason."""
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd.engine import HipDevice, HipModel
    from jaeger_amd.program import compile_plan
    cfg = xr.variant("merge_sum")
    prog = compile_plan(P.build_plan(cfg), xr.random_weights(cfg))
    first, second = poolvecs(prog)[:2]
    dev = HipDevice(0)
    try:
        def refused(word, at=first, **fields):
            bad = copy.copy(prog)
            bad.ops = list(prog.ops)
            op = L.JgOp.from_buffer_copy(prog.ops[at])
            for field, value in fields.items():
                setattr(op, field, value)
            bad.ops[at] = op
            with pytest.raises(L.JaegerHipError, match=word):
                HipModel(dev, bad)

        refused("pool kind 2", arg=L.POOL_MAX_NOMASK)
        refused("pool kind 7", arg=7)
        refused("merge code 3", k=3)
        refused("merge code -1", at=second, k=-1)
        refused("beyond the vector slot's 1024 floats", vec_off=1024)
        refused("beyond the vector slot's 1024 floats", at=second, vec_off=1 << 30)
        refused("no earlier op of the program wrote", k=L.POOLVEC_ADD)
        refused("no earlier op of the program wrote", k=L.POOLVEC_MAX)
        refused("no earlier op of the program wrote", at=second, vec_off=32)
        refused("16 channels, activation slot . holds 32", cout=16)
        refused("multiple of 4", vec_off=2)
        refused("multiple of 4", cout=30)
        refused("reads an activation slot", in_buf=L.JG_BUF_NONE)
        HipModel(dev, prog).close()
    finally:
        dev.close()


def test_cli_predict_branches_model(tmp_path, monkeypatch):
    """``python -m jaeger_amd predict`` with a branches500 model directory (fixture yaml, classes file, .weights.npz) against
    the reference composition, as tests/test_gpu_multiscale.py does it for its model."""
    from click.testing import CliRunner

    import test_gpu_cli as tc
    from jaeger_amd.cli import main
    from jaeger_amd.fragment import read_fasta
    from jaeger_amd.weights import load_npz
    from oracle import forward as ofwd
    root = make_model_dir(tmp_path / "m", name="branches500")
    cfg = load_model_cfg("branches500")
    weights = load_npz(next((root / "model").glob("*.weights.npz")))
    assert set(weights) == set(xr.weight_specs(cfg))
    fasta = GOLDEN / "test_contigs.fasta"
    r = CliRunner().invoke(main, ["predict", "-i", str(fasta), "-o", str(tmp_path / "out"), "--model_path", str(root),
                                  "--fsize", "500", "--stride", "500", "--no-dustmask"])
    assert r.exit_code == 0, r.output
    tsv = list((tmp_path / "out").rglob("test_contigs.tsv"))
    assert len(tsv) == 1, list((tmp_path / "out").rglob("*"))
    monkeypatch.setattr(ofwd, "forward", lambda c, w, ids, dtype=None: {
        k: v.astype(np.float32) for k, v in xr.forward(c, w, ids).items()})
    records = [(n, s.decode()) for n, s in read_fasta(str(fasta))]
    exp, _, _ = tc._expected(tmp_path, records, cfg, weights, 500, 500, None, 96)
    tc._compare_tsv(tsv[0], exp)
