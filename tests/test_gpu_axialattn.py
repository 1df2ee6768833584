"""Axial attention and the stand-alone transformer encoder on the GPU (the CPU tier is tests/test_axialattn_reference.py).

Models with ``axial_attention`` / ``transformer_encoder`` layers through ``HipModel.forward`` in both arithmetics of the
conv stack, on five kinds of windows (full, ragged, nearly empty, one invalid run longer than a key chunk, one window
whose forward frames hold no valid codon at all):

* logits, embedding and NMD against the composed float64 reference (tests/axial_attention_reference.py: oracle/forward.py's
  layers around the restated layers) at the project's gate of 1e-4;
* per op: the tensor every length-attention op writes (``jg_model_set_tap``) against the restatement applied to the op's
  own read-back input and mask, at EVERY position - masked queries included -, inside the bound the numpy emulation of the
  kernel's arithmetic sets for that input (4 x its error, rounded up to a power of two);
* geometry: row lengths around the kernel's query tile and key chunk (``jg_lengthattn_tile()``, ``jg_lengthattn_chunk()``),
  through the id-tensor entry point (``forward(ids)`` takes rows of any length; a 'same'-padded conv keeps them);
* key invisibility: 1e3 at the masked positions of the op's input leaves its output at every valid position bit for bit;
* row isolation: 1e3 at the ends of the neighbouring rows leaves a row's output bit for bit as it was;
* an in-place op is refused at model creation.

No test here provokes a fault; every test runs under a watchdog that ends the process if a GPU call does not return.
"""
import copy
import faulthandler

import numpy as np
import pytest

import attention_reference as ar
import axial_attention_reference as xr
from conftest import load_model_cfg
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
    print("\nlength-attention op against the restatement on its own input, every position (errors in units of the output's rms):")
    for row in _TABLE:
        print("  " + row)


# ---- models -----------------------------------------------------------------------------------------------------------
def variant(name: str) -> dict:
    cfg = copy.deepcopy(load_model_cfg("axial500"))
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    at = [i for i, l in enumerate(layers) if l["name"] == xr.AXIAL][0]
    att = layers[at]["config"]

    def width(c):
        for layer in layers:
            if "filters" in layer["config"]:
                layer["config"]["filters"] = c
        cfg["classifier"]["input_shape"] = c

    if name == "fixture":
        pass
    elif name == "wide":
        width(64)
        att.update(embed_dim=64, num_heads=8, feed_forward_dim=256)
    elif name == "two_blocks":
        att["num_blocks"] = 2
    elif name in ("masked_layernorm", "masked_dyt", "masked_batchnorm"):      # (the fixture's own norm_type is layernorm)
        att.update(norm_type=name, num_blocks=2, epsilon=1e-3)
    elif name == "key_dim4":
        att["num_heads"] = 8
    elif name == "key_dim32":
        att["num_heads"] = 1
    elif name == "behind_cross":                          # no mask arrives
        layers.insert(at, {"name": ar.ATTN, "config": dict(embed_dim=32, num_heads=4, feed_forward_dim=128)})
    elif name == "then_conv":                             # the mask survives; f32 rows -> the conv's F16S in the split-f16 program
        layers += [{"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same")},
                   {"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]
    elif name == "pool_max":
        rep["pooling"] = "max"
    elif name == "nmd_front":
        layers.insert(1, {"name": "nmd", "config": {}})
    elif name == "encoder_c16":                           # a stand-alone transformer_encoder, 16 channels wide
        width(16)
        layers[at] = {"name": xr.ENCODER, "config": dict(embed_dim=16, num_heads=2, feed_forward_dim=32, dropout_rate=0.1)}
    else:
        raise ValueError(name)
    return cfg


VARIANTS = ("fixture", "wide", "two_blocks", "masked_layernorm", "masked_dyt", "masked_batchnorm", "key_dim4", "key_dim32",
            "behind_cross", "then_conv", "pool_max", "nmd_front", "encoder_c16")
#: by how many positions the convs in front of the layer shorten an invalid run: the 7-tap conv by 6, the four 3-tap convs
#: of the two residual blocks by 2 each
GROW = 14


def ids_of(kind: str, n_win: int = 5):
    from jaeger_amd._lib import LENGTHATTN_CHUNK
    from oracle import encoder as oenc
    return xr.window_ids(oenc.frame_length(FSIZE), kind, n_win=n_win, seed=17, chunk=LENGTHATTN_CHUNK, grow=GROW)


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


def length_ops(prog):
    from jaeger_amd import _lib as L
    return [i for i, op in enumerate(prog.ops) if op.kind == L.OP_LENGTHATTN]


def encoders_of(cfg, prog):
    """[(op index, weight prefix of its encoder)] of every length-attention op, in program order."""
    out, ops = [], length_ops(prog)
    for i, kind, a in xr.attention_layers(cfg):
        if kind == xr.AXIAL:
            out += [f"rep/{i}/block{j}/length" for j in range(int(a.get("num_blocks", 1)))]
        elif kind == xr.ENCODER:
            out.append(f"rep/{i}")
    assert len(out) == len(ops)
    return list(zip(ops, out))


def check_op(model, weights, i, prefix, ids, what):
    """The op's own output from its own read-back input and mask, at every position, inside the emulation's bound."""
    from jaeger_amd import _lib as L
    prog = model.program
    op = prog.ops[i]
    x = model.tap(producer(prog, i), ids)
    mw = mask_writer(prog, i)
    mask = None if mw is None else model.tap(mw, ids) != 0
    y = model.tap(i, ids)
    bits = model.tap_variant()
    assert bits & L.TAP_EXACT_F32 and not bits & (L.TAP_F16S | L.TAP_PHASE_SPLIT), (what, bits)
    w_, fr, l, c = x.shape
    rows = lambda a: None if a is None else a.reshape((w_ * fr, l) + a.shape[3:])
    lw = ar.sub_weights(weights, prefix)
    want = ar.apply_stages(xr.transformer_encoder(rows(x), lw, op.k, rows(mask)), prog, op)
    emu = ar.apply_stages(xr.emulate_encoder(rows(x), lw, op.k, rows(mask)), prog, op, dtype=np.float32)
    got = rows(y)
    assert got.shape == want.shape and np.isfinite(got).all()
    b = xr.bounds_from(emu, want)
    e, r = xr.errors(got, want)
    n_masked = 0 if mask is None else int((~rows(mask)).sum())
    whole = 0 if mask is None else int((~rows(mask).any(axis=1)).sum())
    _TABLE.append(f"{what:40s} op {i:2d} L {l:3d} ({n_masked:4d} masked queries, {whole:2d} rows masked as a whole): max {e:.3g} "
                  f"(emulation {b['emu_elem']:.3g}, bound {b['elem']:.3g}), rms {r:.3g} (emulation {b['emu_rms']:.3g}, bound {b['rms']:.3g})")
    print(_TABLE[-1])
    assert e <= b["elem"] and r <= b["rms"], _TABLE[-1]
    return mask


#: both arithmetics of the conv stack - but for 16 channels: no split-f16 conv tile is that narrow (a model of such convs
#: alone has no split-f16 program), so that variant runs in exact f32 only
CASES = [(name, precision) for name in VARIANTS for precision in ("f16x3", "f32") if (name, precision) != ("encoder_c16", "f16x3")]


@pytest.mark.parametrize("name, precision", CASES)
def test_model_outputs_and_length_attention_ops(name, precision):
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import JaegerHipEngine
    cfg = variant(name)
    weights = xr.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision=precision)
    try:
        assert eng.model.precision == precision
        assert not eng.model.placement()["small_fused"]
        ops = encoders_of(cfg, eng.program)
        assert "length attention" in eng.model.describe()
        if precision == "f16x3":
            assert eng.model.placement()["convs_f16x3"] >= 1
        masked_queries = whole_rows = 0
        for kind in xr.KINDS:
            what = f"{name} / {precision} / {kind}"
            ids = ids_of(kind)
            ref = xr.forward(cfg, weights, ids)
            got = eng.model.forward(ids)
            errs = check_vectors(what, got, ref)
            print(what, {k: f"{v:.2e}" for k, v in errs.items()})
            split = eng.model.forward(ids, chunk=2)               # launch groups of 2 + 2 + 1 windows: bit for bit the same
            for k in got:
                np.testing.assert_array_equal(got[k], split[k], err_msg=f"{what} {k}: chunk 2")
            for i, prefix in ops:
                mask = check_op(eng.model, weights, i, prefix, ids, what)
                if mask is not None:
                    masked_queries += int((~mask).sum())
                    whole_rows += int((~mask.reshape(-1, mask.shape[-1]).any(axis=1)).sum())
        masked_op = eng.program.ops[ops[0][0]].in_mask != L.JG_BUF_NONE
        assert masked_op == (name != "behind_cross")
        if masked_op:
            assert masked_queries > 0 and whole_rows >= 3, "the windows left no masked query / no row masked as a whole"
        # the profile's keys are what they were: the op has no profiling class of its own
        eng.device.profile_enable(True)
        eng.model.forward(ids_of("full"))
        prof = eng.device.profile_read()
        eng.device.profile_enable(False)
        assert set(prof) == {"conv_ms", "conv_launches", "conv_flops", "mfma_f16x3", "mfma_f32", "table", "fused_small",
                             "frame_attn", "frame_attn_cvt"}
    finally:
        eng.close()


# ---- geometry -----------------------------------------------------------------------------------------------------------
def minimal_cfg(blocks: int = 2, activation: bool = True, kernel_size: int = 3, embedding: int | None = None) -> dict:
    """embedding -> masked conv ('same': the rows keep their length) [-> batch norm -> gelu] -> axial_attention -> batch norm
    -> average pool -> dense."""
    cfg = copy.deepcopy(load_model_cfg("axial500"))
    layers = cfg["representation_learner"]["hidden_layers"]
    att = copy.deepcopy([l for l in layers if l["name"] == xr.AXIAL][0])
    att["config"].update(num_blocks=blocks)
    front = [{"name": "masked_conv1d", "config": dict(filters=32, kernel_size=kernel_size, padding="same")}]
    if activation:
        front += [{"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]
    cfg["representation_learner"]["hidden_layers"] = front + [att, {"name": "masked_batchnorm", "config": {}}]
    if embedding is not None:
        cfg["embedding"]["embedding_size"] = embedding
    return cfg


def _geometry_lengths():
    from jaeger_amd._lib import LENGTHATTN_CHUNK as CH
    from jaeger_amd._lib import LENGTHATTN_TILE as T
    return sorted({1, 15, 16, 17, CH - 1, CH, CH + 1, 2 * CH + 1, T - 1, T, T + 1, T + CH + 3})


@pytest.mark.parametrize("l", _geometry_lengths())
def test_row_lengths_around_tile_and_chunk(l):
    """Three windows of rows of ``l`` positions, the last one ragged (right-padded rows, an invalid run inside, one row
    without a valid codon): a ragged last tile, a ragged last chunk, a ragged last softmax step, rows of one position."""
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import JaegerHipEngine
    assert L.load().jg_lengthattn_tile() == L.LENGTHATTN_TILE and L.load().jg_lengthattn_chunk() == L.LENGTHATTN_CHUNK
    cfg = minimal_cfg()
    weights = xr.random_weights(cfg)
    rng = np.random.Generator(np.random.PCG64(l))
    ids = rng.integers(1, 65, (3, 6, l)).astype(np.uint8)
    for f in range(5):
        ids[2, f, max(l - 1 - 3 * f, 1):] = 0                   # frame 0 keeps all but its last position (l = 1: all of it)
        if l > 30:
            ids[2, f, 5 + f:5 + f + 9] = 0
    ids[2, 5, :] = 0
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision="f32")
    try:
        what = f"geometry L {l}"
        got = eng.model.forward(ids)
        errs = check_vectors(what, got, xr.forward(cfg, weights, ids))
        print(what, {k: f"{v:.2e}" for k, v in errs.items()})
        for i, prefix in encoders_of(cfg, eng.program):
            check_op(eng.model, weights, i, prefix, ids, what)
    finally:
        eng.close()


# ---- key invisibility, row isolation -------------------------------------------------------------------------------------
def test_masked_keys_are_invisible_to_valid_queries():
    """The op's input holds 1e3 at every masked position - the one-tap conv in front is patched to read the embedding rows
    unmasked, and row 0 (the invalid codon's) holds 1e3 in the second model - and its output at every valid position is
    bit for bit what it is with ordinary values there: a masked key's score is selected away, not added to, and its v row
    is zeroed."""
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd.engine import HipDevice, HipModel
    from jaeger_amd.program import compile_plan
    cfg = minimal_cfg(blocks=1, activation=False, kernel_size=1, embedding=32)
    weights = xr.random_weights(cfg)
    loud = dict(weights)
    loud["embedding/embeddings"] = weights["embedding/embeddings"].copy()
    loud["embedding/embeddings"][0] = 1e3
    l = L.LENGTHATTN_TILE + L.LENGTHATTN_CHUNK + 3
    ids = xr.window_ids(l, "empty_fwd", n_win=3, seed=5)
    ids[0, :, 40:40 + L.LENGTHATTN_CHUNK + 6] = 0                # an invalid run longer than a chunk, valid codons behind it
    dev = HipDevice(0)
    try:
        outs = []
        for wts in (weights, loud):
            prog = compile_plan(P.build_plan(cfg), wts)
            conv = [i for i, op in enumerate(prog.ops) if op.kind == L.OP_CONV]
            assert len(conv) == 1 and prog.ops[conv[0]].k == 1 and prog.ops[conv[0]].in_mask == L.JG_BUF_IDS
            op = L.JgOp.from_buffer_copy(prog.ops[conv[0]])
            op.in_mask = L.JG_BUF_NONE                               # the conv reads the rows as they are: row 0 at invalid codons
            prog.ops[conv[0]] = op
            model = HipModel(dev, prog)
            try:
                model.set_precision("f32")
                at = length_ops(prog)[0]
                assert prog.ops[at].in_mask >= 0
                mask = model.tap(mask_writer(prog, at), ids) != 0
                x = model.tap(conv[0], ids)
                outs.append((model.tap(at, ids), x, mask))
            finally:
                model.close()
        (y0, x0, m0), (y1, x1, m1) = outs
        assert np.array_equal(m0, m1) and np.array_equal(m0, ids != 0) and (~m0).sum() > 100 and m0.sum() > 100
        assert np.array_equal(x0[m0], x1[m0])                        # the valid positions read the same input ...
        assert np.abs(x1[~m1]).max(axis=-1).min() > 1e2 and np.abs(x0).max() < 1e2      # ... every masked one a loud one
        assert np.isfinite(y0).all() and np.isfinite(y1).all()
        np.testing.assert_array_equal(y0[m0], y1[m0], err_msg="a valid query's output changed with the values at masked keys")
        assert np.abs(y0[~m0] - y1[~m0]).max() > 1e2                 # (the masked queries' own outputs carry their inputs on)
    finally:
        dev.close()


def test_rows_do_not_see_their_neighbours():
    """Row r's tail and row r + 1's head are adjacent in memory.  With 1e3 at both ends of every other row the middle
    row's output is bit for bit what it is without them."""
    from jaeger_amd._lib import LENGTHATTN_CHUNK as CH
    from jaeger_amd._lib import LENGTHATTN_TILE as T
    from jaeger_amd.engine import JaegerHipEngine
    cfg = minimal_cfg(blocks=1, activation=False, kernel_size=1, embedding=32)
    weights = xr.random_weights(cfg)
    huge_id = 64
    weights_huge = dict(weights)
    weights_huge["embedding/embeddings"] = weights["embedding/embeddings"].copy()
    weights_huge["embedding/embeddings"][huge_id] = 1e3
    for l in (CH - 3, T + 5):
        rng = np.random.Generator(np.random.PCG64(l))
        ids = rng.integers(1, 64, (2, 6, l)).astype(np.uint8)           # (ids 1 .. 63: id 64 only where it is put)
        marked = ids.copy()
        mid = (0, 3)
        for w in range(2):
            for f in range(6):
                if (w, f) != mid:
                    marked[w, f, :3] = huge_id
                    marked[w, f, -3:] = huge_id
        outs = []
        for wts, tensor in ((weights, ids), (weights_huge, marked)):
            eng = JaegerHipEngine(model_cfg=cfg, weights=wts, device_id=0, precision="f32")
            try:
                at = length_ops(eng.program)[0]
                outs.append(eng.model.tap(at, tensor)[mid[0], mid[1]])
                if wts is weights_huge:
                    x = eng.model.tap(producer(eng.program, at), tensor)
                    assert np.abs(x[0, 2, -1]).max() > 1e2 and np.abs(x[0, 4, 0]).max() > 1e2      # the neighbours do hold them
            finally:
                eng.close()
        assert np.isfinite(outs[0]).all()
        np.testing.assert_array_equal(outs[0], outs[1], err_msg=f"L {l}: the middle row changed with its neighbours' row ends")


def test_in_place_and_other_sizes_are_refused_at_model_creation():
    """The plan refuses them first; a program that reaches the library anyway is refused there, with the reason."""
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd.engine import HipDevice, HipModel
    from jaeger_amd.program import compile_plan
    cfg = variant("fixture")
    prog = compile_plan(P.build_plan(cfg), xr.random_weights(cfg))
    i = length_ops(prog)[0]
    dev = HipDevice(0)
    try:
        for field, value, word in (("out_buf", prog.ops[i].in_buf, "cannot run in place"), ("k", 3, "heads"),
                                   ("arg", 520, "feed-forward width"), ("arg", 0, "feed-forward width"),
                                   ("out_mask", prog.ops[i].in_mask + 1, "keeps its mask or drops it")):
            bad = copy.copy(prog)
            bad.ops = list(prog.ops)
            op = L.JgOp.from_buffer_copy(prog.ops[i])
            setattr(op, field, value)
            bad.ops[i] = op
            with pytest.raises(L.JaegerHipError, match=word):
                HipModel(dev, bad)
    finally:
        dev.close()
