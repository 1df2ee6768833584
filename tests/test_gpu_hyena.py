"""Hyena on the GPU (the CPU tier is tests/test_hyena_reference.py).

Models with ``hyena_block`` layers through ``HipModel.forward`` in both arithmetics of the conv stack, on six kinds of
windows (full, ragged tail, nearly empty, an N run in the middle, rows that START with invalid positions, rows with no valid
position at all):

* logits, embedding and NMD against the composed float64 reference (tests/hyena_reference.py: oracle/forward.py's layers
  around the restated layer) at the project's gate of 1e-4;
* per op: the tensor every hyena op writes (``jg_model_set_tap``) against the restatement applied to the op's own read-back
  input and mask, at EVERY position, inside the bound the numpy emulation of the kernels' arithmetic sets for that input
  (4 x its error, rounded up to a power of two); exact zeros at masked positions;
* row lengths around the kernels' tile and chunk (``_lib.HYENA_TILE``, ``_lib.HYENA_CHUNK``) through the id-tensor entry
  point, calls of different lengths on one model with ``filter_normalize``;
* row isolation, causality, the refusal of a row longer than the filter table.

No test here provokes a fault; every test runs under a watchdog that ends the process if a GPU call does not return.
"""
import copy
import faulthandler

import numpy as np
import pytest

import attention_reference as ar
import hyena_reference as hr
from conftest import GOLDEN, load_model_cfg, make_model_dir
from mixer_reference import mask_writer, producer

pytestmark = pytest.mark.gpu

TOL = 1e-4
FSIZE = 500
_TABLE = []


@pytest.fixture(autouse=True)
def _watchdog():
    faulthandler.dump_traceback_later(900, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nhyena op against the restatement on its own input, every position (errors in units of the output's rms):")
    for row in _TABLE:
        print("  " + row)


# ---- models -----------------------------------------------------------------------------------------------------------
def variant(name: str) -> dict:
    if name == "first":
        return copy.deepcopy(load_model_cfg("hyenafirst500"))
    cfg = copy.deepcopy(load_model_cfg("hyena500"))
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    at = [i for i, l in enumerate(layers) if l["name"] == hr.HYENA][0]
    hy = layers[at]["config"]

    def width(c):
        for layer in layers:
            if "filters" in layer["config"]:
                layer["config"]["filters"] = c
        cfg["classifier"]["input_shape"] = c
        hy["dim"] = c

    if name == "fixture":
        pass
    elif name == "c16":
        width(16)
    elif name == "wide":                                  # 64 channels, three convolutions, the output projection
        width(64)
        hy.update(order=3, output_projection=True)
    elif name == "order1":
        hy["order"] = 1
    elif name == "normalize":
        hy["filter_normalize"] = True
    elif name == "sin":
        hy["filter_activation"] = "sin"
    elif name == "seq_len":
        hy["seq_len"] = 200
    elif name == "behind_cross":                          # no mask arrives: no multiply by one anywhere
        layers.insert(at, {"name": ar.ATTN, "config": dict(embed_dim=32, num_heads=4, feed_forward_dim=128)})
    elif name == "then_conv":                             # f32 rows -> the next conv's F16S in the split-f16 program
        layers += [{"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same")},
                   {"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]
    elif name == "ln_tail":
        layers[-1] = {"name": "masked_layernorm", "config": {}}
        layers.append({"name": "activation", "config": {"activation": "gelu"}})
    elif name == "two_layers":
        layers.insert(at + 1, {"name": hr.HYENA, "config": dict(dim=32, order=2, output_projection=True, filter_normalize=True)})
    elif name == "nmd_front":
        layers.insert(1, {"name": "nmd", "config": {}})
    elif name == "pool_max":
        rep["pooling"] = "max"
    else:
        raise ValueError(name)
    return cfg


VARIANTS = ("fixture", "first", "c16", "wide", "order1", "normalize", "sin", "seq_len", "behind_cross", "then_conv", "ln_tail",
            "two_layers", "nmd_front", "pool_max")
#: by how many positions the convs in front of the layer shorten an invalid run: the 7-tap conv by 6, the four 3-tap convs
#: of the two residual blocks by 2 each
GROW = 14


def ids_of(kind: str, name: str, n_win: int = 5):
    from oracle import encoder as oenc
    return hr.window_ids(oenc.frame_length(FSIZE), kind, n_win=n_win, seed=17, grow=0 if name == "first" else GROW)


def check_vectors(what, got, ref):
    """The project's gate: 1e-4 absolute on the logits; on the side outputs 1e-4 absolute where |ref| <= 8 and 1.25e-5
    relative above (tests/test_gpu_parity.py: check_side_output)."""
    errs = {}
    for k, r in ref.items():
        assert got[k].shape == r.shape, (what, k, got[k].shape, r.shape)
        g64, r64 = np.asarray(got[k], np.float64), np.asarray(r, np.float64)
        err = np.abs(g64 - r64)
        errs[k] = float(err.max())
        if k == "prediction":
            assert err.max() <= TOL, (what, k, float(err.max()))
        else:
            small = np.abs(r64) <= 8.0
            assert not small.any() or err[small].max() <= TOL, (what, k, float(err[small].max()))
            assert small.all() or (err[~small] / np.abs(r64[~small])).max() <= 1.25e-5, (what, k)
    return errs


def hyena_ops(prog):
    from jaeger_amd import _lib as L
    return [i for i, op in enumerate(prog.ops) if op.kind == L.OP_HYENA]


def layers_of(cfg, prog):
    """[(op index, weight prefix, the layer's parameters)] of every hyena op, in program order."""
    out = [(f"rep/{i}", hr.params_of(a)) for i, kind, a in hr.hyena_layers(cfg) if kind == hr.HYENA]
    ops = hyena_ops(prog)
    assert len(out) == len(ops)
    return [(i, prefix, p) for i, (prefix, p) in zip(ops, out)]


def check_op(eng, weights, i, prefix, params, ids, what):
    """The op's own output from its own read-back input and mask: every position inside the emulation's bound, masked ones
    exact zeros (where the store carries no stage)."""
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
    rows = lambda a: None if a is None else a.reshape((w_ * fr, l) + a.shape[3:])
    lw = ar.sub_weights(weights, prefix)
    assert op.stride == (params["seq_len"] or hr.TABLE_ROWS) and op.k == params["order"]
    want = hr.hyena_block(rows(x), lw, rows(mask), **params)
    emu = hr.emulate_block(rows(x), lw, rows(mask), **params)
    got = rows(y)
    n_masked = 0 if mask is None else int((~rows(mask)).sum())
    if op.n_stages == 0 and mask is not None:
        assert (got[~rows(mask)] == 0.0).all(), f"{what} op {i}: non-zero values at masked positions"
    want = ar.apply_stages(want, prog, op)
    emu = ar.apply_stages(emu, prog, op, dtype=np.float32)
    b = ar.bounds_from(emu, want)
    e, r = ar.errors(got, want)
    _TABLE.append(f"{what:40s} op {i:2d} L {l:3d} ({n_masked:4d} masked): max {e:.3g} (emulation {b['emu_elem']:.3g}, bound {b['elem']:.3g}), "
                  f"rms {r:.3g} (emulation {b['emu_rms']:.3g}, bound {b['rms']:.3g})")
    print(_TABLE[-1])
    assert np.isfinite(got).all() and e <= b["elem"] and r <= b["rms"], _TABLE[-1]
    return mask


@pytest.mark.parametrize("name", VARIANTS)
def test_model_outputs_and_hyena_ops(name):
    """Both arithmetics of the conv stack: the program's own default (split-f16 where the convs have such a program) and
    exact f32.  16-channel convs have no split-f16 tile, and the fixture must have one."""
    from jaeger_amd.engine import JaegerHipEngine
    cfg = variant(name)
    weights = hr.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0)
    try:
        precisions = [eng.model.precision] + (["f32"] if eng.model.precision != "f32" else [])
        if name in ("fixture", "wide", "then_conv", "two_layers"):
            assert precisions == ["f16x3", "f32"], precisions
        assert not eng.model.placement()["small_fused"]
        ops = layers_of(cfg, eng.program)
        assert "hyena" in eng.model.describe()
        seen_masked_first = 0
        refs = {kind: hr.forward(cfg, weights, ids_of(kind, name)) for kind in hr.KINDS}     # once, for both arithmetics
        for precision in precisions:
            eng.model.set_precision(precision)
            assert eng.model.precision == precision
            for kind in hr.KINDS:
                what = f"{name} / {precision} / {kind}"
                ids = ids_of(kind, name)
                got = eng.model.forward(ids)
                errs = check_vectors(what, got, refs[kind])
                print(what, {k: f"{v:.2e}" for k, v in errs.items()})
                split = eng.model.forward(ids, chunk=2)               # launch groups of 2 + 2 + 1 windows: bit for bit the same
                for k in got:
                    np.testing.assert_array_equal(got[k], split[k], err_msg=f"{what} {k}: chunk 2")
                for i, prefix, params in ops:
                    mask = check_op(eng, weights, i, prefix, params, ids, what)
                    if mask is not None and kind in ("n_run", "starts_invalid"):
                        m2 = mask.reshape(-1, mask.shape[2])
                        seen_masked_first += int((~m2 & (m2[:, ::-1].cumsum(axis=1)[:, ::-1] > 0)).sum())
        if name != "behind_cross":
            assert seen_masked_first > 0, "no masked position with valid ones behind it reached the op"
    finally:
        eng.close()


# ---- row lengths --------------------------------------------------------------------------------------------------------
def minimal_cfg(**over) -> dict:
    """embedding -> masked 3-tap conv ('same': the rows keep their length) -> batch norm -> gelu -> hyena_block -> batch norm
    -> average pool -> dense."""
    cfg = copy.deepcopy(load_model_cfg("hyena500"))
    layers = cfg["representation_learner"]["hidden_layers"]
    hy = copy.deepcopy([l for l in layers if l["name"] == hr.HYENA][0])
    hy["config"].update(over)
    front = [{"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same")},
             {"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]
    cfg["representation_learner"]["hidden_layers"] = front + [hy, {"name": "masked_batchnorm", "config": {}}]
    return cfg


def _lengths():
    from jaeger_amd._lib import HYENA_CHUNK as CH
    from jaeger_amd._lib import HYENA_TILE as T
    return sorted({1, 2, T - 1, T, T + 1, CH - 1, CH, CH + 1, 2 * CH + 3, 665})


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
    cfg = minimal_cfg(output_projection=True)
    weights = hr.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision="f32")
    yield cfg, weights, eng
    eng.close()


@pytest.mark.parametrize("l", _lengths())
def test_row_lengths(length_model, l):
    """Three windows of rows of ``l`` positions, the last one ragged: a single position, a ragged last tile, the diagonal
    chunk alone, a second and a third chunk, the longest row the short-contig pass meets."""
    from jaeger_amd import _lib as L
    cfg, weights, eng = length_model
    assert L.load().jg_hyena_tile() == L.HYENA_TILE and L.load().jg_hyena_chunk() == L.HYENA_CHUNK
    ids = _ragged_ids(l, n_win=1 if l > 300 else 3)
    what = f"row length {l}"
    got = eng.model.forward(ids)
    errs = check_vectors(what, got, hr.forward(cfg, weights, ids))
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    for i, prefix, params in layers_of(cfg, eng.program):
        check_op(eng, weights, i, prefix, params, ids, what)


def test_calls_of_different_lengths_on_one_normalising_model():
    """``filter_normalize`` is the one place where a value depends on the row length of the call: 166, then 40, then 166
    again - the first and third results are bit-identical, the second matches its own reference."""
    from jaeger_amd.engine import JaegerHipEngine
    cfg = minimal_cfg(filter_normalize=True)
    weights = hr.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision="f32")
    try:
        long_ids, short_ids = _ragged_ids(166), _ragged_ids(40)
        first = eng.model.forward(long_ids)
        second = eng.model.forward(short_ids)
        third = eng.model.forward(long_ids)
        for k in first:
            np.testing.assert_array_equal(first[k], third[k], err_msg=k)
        check_vectors("L 166", first, hr.forward(cfg, weights, long_ids))
        check_vectors("L 40 between two calls at 166", second, hr.forward(cfg, weights, short_ids))
        for i, prefix, params in layers_of(cfg, eng.program):
            check_op(eng, weights, i, prefix, params, short_ids, "normalize, L 40 behind L 166")
    finally:
        eng.close()


def test_rows_do_not_see_their_neighbours():
    """Row r's tail and row r + 1's head are adjacent in memory.  With values of 1e30 in every other row the middle row's
    output is bit for bit what it is without them (a convolution running on over the row's end would change it)."""
    from jaeger_amd._lib import HYENA_TILE as T
    from jaeger_amd.engine import JaegerHipEngine
    cfg = minimal_cfg()
    cfg["representation_learner"]["hidden_layers"] = cfg["representation_learner"]["hidden_layers"][:1] + \
        cfg["representation_learner"]["hidden_layers"][3:]                       # conv -> hyena: the huge values arrive as they are
    weights = hr.random_weights(cfg)
    huge_id = 64
    weights_huge = dict(weights)
    weights_huge["embedding/embeddings"] = weights["embedding/embeddings"].copy()
    weights_huge["embedding/embeddings"][huge_id] = 1e30
    for l in (T, T + 5):
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
                op = hyena_ops(eng.program)[-1]
                outs.append(eng.model.tap(op, tensor)[mid[0], mid[1]])
                if wts is weights_huge:
                    x = eng.model.tap(producer(eng.program, op), tensor)
                    assert np.abs(x[0, 2, -1]).max() > 1e28 and np.abs(x[0, 4, 0]).max() > 1e28      # the neighbours do hold them
            finally:
                eng.close()
        assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
        np.testing.assert_array_equal(outs[0], outs[1], err_msg=f"L {l}: the middle row changed with its neighbours")


def test_causality_on_the_first_layer_model():
    """hyenafirst500: changing the ids from position t0 on - other codons, and invalid ones - leaves the op's output in
    front of t0 bit for bit."""
    from jaeger_amd.engine import JaegerHipEngine
    cfg = variant("first")
    weights = hr.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision="f32")
    try:
        op = hyena_ops(eng.program)[0]
        ids = ids_of("n_run", "first", n_win=3)
        l = ids.shape[2]
        base = eng.model.tap(op, ids)
        for t0 in (1, 63, 64, 65, 130):
            rng = np.random.Generator(np.random.PCG64(t0))
            changed = ids.copy()
            changed[:, :, t0:] = rng.integers(0, 65, (3, 6, l - t0))
            got = eng.model.tap(op, changed)
            np.testing.assert_array_equal(got[:, :, :t0], base[:, :, :t0], err_msg=f"t0 {t0}")
            assert np.abs(got[:, :, t0:] - base[:, :, t0:]).max() > 1e-3
    finally:
        eng.close()


def test_a_row_longer_than_the_filter_table_is_refused_and_the_model_runs_on():
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import JaegerHipEngine
    cfg = minimal_cfg(seq_len=100)
    weights = hr.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision="f32")
    try:
        with pytest.raises(L.JaegerHipError, match=r"\(-3\).*hyena over rows of 166 positions, the layer's filter table holds 100"):
            eng.model.forward(_ragged_ids(166))
        ids = _ragged_ids(100)
        check_vectors("L 100 = seq_len, behind the refusal", eng.model.forward(ids), hr.forward(cfg, weights, ids))
    finally:
        eng.close()


def test_flops_per_window_counts_the_projections_and_the_convolutions():
    from jaeger_amd.engine import JaegerHipEngine
    cfg = variant("first")
    eng = JaegerHipEngine(model_cfg=cfg, weights=hr.random_weights(cfg), device_id=0)
    try:
        for l in (1, 166, 665):
            identity = 2.0 * 32 * 32 * 6 * l
            want = identity + 6 * (2.0 * 3 * 32 * 32 * l + 2.0 * 2 * 32 * (l * (l + 1) / 2))
            assert eng.model.flops_per_window(l) == want, (l, eng.model.flops_per_window(l), want)
    finally:
        eng.close()


def test_other_sizes_are_refused_at_model_creation():
    """The plan refuses them first; a program that reaches the library anyway is refused there, with the reason."""
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd.engine import HipDevice, HipModel
    from jaeger_amd.program import compile_plan
    cfg = variant("fixture")
    prog = compile_plan(P.build_plan(cfg), hr.random_weights(cfg))
    i = hyena_ops(prog)[0]
    dev = HipDevice(0)
    try:
        for field, value, word in (("k", 5, "order 5"), ("k", 0, "order 0"), ("arg", 4, "flags"), ("stride", 0, "0 rows"),
                                   ("stride", 1 << 24, "outside the weight blob"), ("out_buf", prog.ops[i].in_buf, "in place"),
                                   ("out_mask", L.JG_BUF_NONE, "keeps its mask")):
            bad = copy.copy(prog)
            bad.ops = list(prog.ops)
            op = L.JgOp.from_buffer_copy(prog.ops[i])
            setattr(op, field, value)
            bad.ops[i] = op
            with pytest.raises(L.JaegerHipError, match=word):
                HipModel(dev, bad)
    finally:
        dev.close()


def test_cli_predict_first_layer_model(tmp_path, monkeypatch):
    """``python -m jaeger_amd predict`` with a hyenafirst500 model directory (fixture yaml, classes file, .weights.npz)
    against the reference composition, as tests/test_gpu_localattn.py does it for the local-attention model."""
    from click.testing import CliRunner

    import test_gpu_cli as tc
    from jaeger_amd.cli import main
    from jaeger_amd.fragment import read_fasta
    from jaeger_amd.weights import load_npz
    from oracle import forward as ofwd
    root = make_model_dir(tmp_path / "m", name="hyenafirst500")
    cfg = load_model_cfg("hyenafirst500")
    weights = load_npz(next((root / "model").glob("*.weights.npz")))
    assert set(weights) == set(hr.weight_specs(cfg))
    fasta = GOLDEN / "test_contigs.fasta"
    r = CliRunner().invoke(main, ["predict", "-i", str(fasta), "-o", str(tmp_path / "out"), "--model_path", str(root),
                                  "--fsize", "500", "--stride", "500", "--no-dustmask"])
    assert r.exit_code == 0, r.output
    tsv = list((tmp_path / "out").rglob("test_contigs.tsv"))
    assert len(tsv) == 1, list((tmp_path / "out").rglob("*"))
    monkeypatch.setattr(ofwd, "forward", lambda c, w, ids, dtype=None: {
        k: v.astype(np.float32) for k, v in hr.forward(c, w, ids).items()})
    records = [(n, s.decode()) for n, s in read_fasta(str(fasta))]
    exp, _, _ = tc._expected(tmp_path, records, cfg, weights, 500, 500, None, 96)
    tc._compare_tsv(tsv[0], exp)
