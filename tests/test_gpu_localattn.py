"""Local attention on the GPU (the CPU tier is tests/test_localattn_reference.py).

Models with ``local_attention`` layers through ``HipModel.forward`` in both arithmetics of the conv stack, on five kinds
of windows (full, ragged, nearly empty, one invalid run longer than the band, one shorter):

* logits, embedding and NMD against the composed float64 reference (tests/local_attention_reference.py: oracle/forward.py's
  layers around the restated layer, which holds a LARGE value at dead positions where the op writes zeros - agreement
  shows that no valid output sees them) at the project's gate of 1e-4;
* per op: the tensor every local-attention op writes (``jg_model_set_tap``) against the restatement applied to the op's own
  read-back input and mask, at every live position, inside the bound the numpy emulation of the kernel's arithmetic sets
  for that input (4 x its error, rounded up to a power of two); exact zeros at dead positions;
* tile geometry: row lengths around the kernel's tile of T = ``_lib.LOCALATTN_TILE`` query positions and around the
  half-window, through the id-tensor entry point (``forward(ids)`` takes rows of any length, so the lengths are set
  directly and not through a window size: a 'same'-padded conv keeps them);
* row isolation: huge values at the ends of the neighbouring rows leave a row's output bit for bit as it was.

No test here provokes a fault; every test runs under a watchdog that ends the process if a GPU call does not return.
"""
import copy
import faulthandler

import numpy as np
import pytest

import attention_reference as ar
import local_attention_reference as lr
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
    print("\nlocal-attention op against the restatement on its own input, live positions (errors in units of the output's rms):")
    for row in _TABLE:
        print("  " + row)


# ---- models -----------------------------------------------------------------------------------------------------------
def variant(name: str) -> dict:
    cfg = copy.deepcopy(load_model_cfg("localattn500"))
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    att = [l for l in layers if l["name"] == lr.LOCAL][0]["config"]

    def width(c):
        for layer in layers:
            if "filters" in layer["config"]:
                layer["config"]["filters"] = c
        cfg["classifier"]["input_shape"] = c

    if name == "fixture":
        pass
    elif name == "c16":                                   # the reference's own instance is 16 channels wide
        width(16)
        att.update(embed_dim=16, num_heads=2, feed_forward_dim=32)
    elif name == "wide":                                  # 64 channels, 8 heads, 256 hidden, half-window 32: two halo blocks
        width(64)
        att.update(embed_dim=64, num_heads=8, feed_forward_dim=256, window_size=64)
    elif name == "window1":                               # every position attends itself alone: no halo
        att["window_size"] = 1
    elif name == "one_block":
        att["num_blocks"] = 1
    elif name == "behind_cross":                          # no mask arrives: the band alone
        layers.insert(6, {"name": ar.ATTN, "config": dict(embed_dim=32, num_heads=4, feed_forward_dim=128)})
    elif name == "then_conv":                             # f32 rows -> the next conv's F16S in the split-f16 program
        layers += [{"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same")},
                   {"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]
    elif name == "ln_tail":
        layers[-1] = {"name": "masked_layernorm", "config": {}}
        layers.append({"name": "activation", "config": {"activation": "gelu"}})
    elif name == "pool_max":
        rep["pooling"] = "max"
    elif name == "nmd_front":
        layers.insert(1, {"name": "nmd", "config": {}})
    else:
        raise ValueError(name)
    return cfg


VARIANTS = ("fixture", "c16", "wide", "window1", "one_block", "behind_cross", "then_conv", "ln_tail", "pool_max", "nmd_front")
#: by how many positions the convs in front of the layer shorten an invalid run: the 7-tap conv by 6, the four 3-tap convs
#: of the two residual blocks by 2 each
GROW = 14


def ids_of(kind: str, half: int, n_win: int = 5):
    from oracle import encoder as oenc
    return lr.window_ids(oenc.frame_length(FSIZE), kind, n_win=n_win, seed=17, half=half, grow=GROW)


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


def local_ops(prog):
    from jaeger_amd import _lib as L
    return [i for i, op in enumerate(prog.ops) if op.kind == L.OP_LOCALATTN]


def blocks_of(cfg, prog):
    """[(op index, weight prefix of its block)] of every local-attention op, in program order."""
    out, ops = [], local_ops(prog)
    for i, kind, a in lr.attention_layers(cfg):
        if kind == lr.LOCAL:
            out += [f"rep/{i}/block{j}" for j in range(int(a.get("num_blocks", 1)))]
    assert len(out) == len(ops)
    return list(zip(ops, out))


def check_op(eng, cfg, weights, i, prefix, ids, what):
    """The op's own output from its own read-back input and mask: live positions inside the emulation's bound, dead ones zero."""
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
    window = 2 * op.stride + 1                              # (window // 2 = the op's half-window)
    want, dead = lr.local_attention_block(rows(x), lw, op.k, window, rows(mask))
    emu = lr.emulate_block(rows(x), lw, op.k, window, rows(mask))
    want = ar.apply_stages(want, prog, op)
    emu = ar.apply_stages(emu, prog, op, dtype=np.float32)
    got = rows(y)
    assert (got[dead] == 0.0).all(), f"{what} op {i}: {int((got[dead] != 0).sum())} non-zero values at dead positions"
    b = lr.bounds_from(emu, want, dead)
    e, r = lr.live_errors(got, want, dead)
    n_masked_live = 0 if mask is None else int((~rows(mask) & ~dead).sum())
    _TABLE.append(f"{what:38s} op {i:2d} L {l:3d} ({int(dead.sum()):4d} dead, {n_masked_live:4d} masked but live): max {e:.3g} "
                  f"(emulation {b['emu_elem']:.3g}, bound {b['elem']:.3g}), rms {r:.3g} (emulation {b['emu_rms']:.3g}, bound {b['rms']:.3g})")
    print(_TABLE[-1])
    assert e <= b["elem"] and r <= b["rms"], _TABLE[-1]
    return dead, mask


#: both arithmetics of the conv stack - but for 16 channels: no split-f16 conv tile is that narrow (a model of such convs
#: alone has no split-f16 program, jg_model_set_precision says so), so that variant runs in exact f32 only
CASES = [(name, precision) for name in VARIANTS for precision in ("f16x3", "f32") if (name, precision) != ("c16", "f16x3")]


@pytest.mark.parametrize("name, precision", CASES)
def test_model_outputs_and_local_attention_ops(name, precision):
    from jaeger_amd.engine import JaegerHipEngine
    cfg = variant(name)
    weights = lr.random_weights(cfg)
    half = [int(a["window_size"]) // 2 for _, kind, a in lr.attention_layers(cfg) if kind == lr.LOCAL][0]
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision=precision)
    try:
        assert eng.model.precision == precision
        assert not eng.model.placement()["small_fused"]
        ops = blocks_of(cfg, eng.program)
        assert "local attention" in eng.model.describe()
        if precision == "f16x3":
            assert eng.model.placement()["convs_f16x3"] >= 1
        interior_dead = 0
        for kind in lr.KINDS:
            what = f"{name} / {precision} / {kind}"
            ids = ids_of(kind, half)
            ref = lr.forward(cfg, weights, ids)
            got = eng.model.forward(ids)
            errs = check_vectors(what, got, ref)
            print(what, {k: f"{v:.2e}" for k, v in errs.items()})
            split = eng.model.forward(ids, chunk=2)               # launch groups of 2 + 2 + 1 windows: bit for bit the same
            for k in got:
                np.testing.assert_array_equal(got[k], split[k], err_msg=f"{what} {k}: chunk 2")
            for i, prefix in ops:
                dead, mask = check_op(eng, cfg, weights, i, prefix, ids, what)
                if kind == "long_n" and mask is not None:                 # dead positions with valid codons behind them
                    m2 = mask.reshape(dead.shape)
                    interior_dead += int((dead & (m2[:, ::-1].cumsum(axis=1)[:, ::-1] > 0)).sum())
        if name in ("fixture", "c16", "one_block", "pool_max", "nmd_front", "then_conv", "ln_tail"):
            assert interior_dead > 0, "the long invalid run left no dead position with valid codons behind it"
        # one launch per block and launch group; the profile's existing keys are what they were
        ids = ids_of("full", half)
        for chunk, groups in ((0, 1), (2, 3)):
            eng.device.profile_enable(True)
            eng.model.forward(ids, chunk=chunk)
            prof = eng.device.profile_read()
            mine = eng.device.profile_read_local_attn()
            eng.device.profile_enable(False)
            assert set(prof) == {"conv_ms", "conv_launches", "conv_flops", "mfma_f16x3", "mfma_f32", "table", "fused_small",
                                 "frame_attn", "frame_attn_cvt"}
            assert mine["local_attn"]["launches"] == len(ops) * groups, (name, chunk, mine)
            assert mine["local_attn"]["flops"] > 0
    finally:
        eng.close()


# ---- tile geometry ------------------------------------------------------------------------------------------------------
def minimal_cfg(window: int, blocks: int = 2, activation: bool = True) -> dict:
    """embedding -> masked 3-tap conv ('same': the rows keep their length) [-> batch norm -> gelu] -> local_attention ->
    batch norm -> average pool -> dense."""
    cfg = copy.deepcopy(load_model_cfg("localattn500"))
    layers = cfg["representation_learner"]["hidden_layers"]
    att = copy.deepcopy([l for l in layers if l["name"] == lr.LOCAL][0])
    att["config"].update(window_size=window, num_blocks=blocks)
    front = [{"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same")}]
    if activation:
        front += [{"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]
    cfg["representation_learner"]["hidden_layers"] = front + [att, {"name": "masked_batchnorm", "config": {}}]
    return cfg


def _geometry_cases():
    from jaeger_amd._lib import LOCALATTN_TILE as T
    h = 8
    return [(1, h), (h, h), (h + 1, h), (T - 1, h), (T, h), (T + 1, h), (2 * T + 1, h), (T + 1, 32)]


@pytest.mark.parametrize("l, half", _geometry_cases())
def test_tile_geometry(l, half):
    """Three windows of rows of ``l`` positions, the last one ragged (right-padded rows, an invalid run inside): halos
    across tile borders, the row's two ends, a ragged last tile, rows shorter than the halo."""
    from jaeger_amd.engine import JaegerHipEngine
    cfg = minimal_cfg(2 * half)
    weights = lr.random_weights(cfg)
    rng = np.random.Generator(np.random.PCG64(l))
    ids = rng.integers(1, 65, (3, 6, l)).astype(np.uint8)
    for f in range(6):
        ids[2, f, max(l - 1 - 3 * f, 1):] = 0                   # frame 0 keeps all but its last position (l = 1: all of it)
        if l > 30:
            ids[2, f, 5 + f:5 + f + 2 * half + 3] = 0             # a dead stretch inside (the 3-tap conv shortens it by 2)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision="f32")
    try:
        what = f"geometry L {l} half {half}"
        got = eng.model.forward(ids)
        errs = check_vectors(what, got, lr.forward(cfg, weights, ids))
        print(what, {k: f"{v:.2e}" for k, v in errs.items()})
        for i, prefix in blocks_of(cfg, eng.program):
            check_op(eng, cfg, weights, i, prefix, ids, what)
    finally:
        eng.close()


def test_rows_do_not_see_their_neighbours():
    """Row r's tail and row r + 1's head are adjacent in memory.  With values of 1e30 at both ends of every other row the
    middle row's output is bit for bit what it is without them (a halo read over the row's end would turn it into
    inf / nan, a halo taken as keys would change it)."""
    from jaeger_amd._lib import LOCALATTN_TILE as T
    from jaeger_amd.engine import JaegerHipEngine
    cfg = minimal_cfg(16, blocks=2, activation=False)
    cfg["representation_learner"]["hidden_layers"][0]["config"]["use_bias"] = True
    weights = lr.random_weights(cfg)
    weights["embedding/embeddings"] = weights["embedding/embeddings"].copy()
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
                    marked[w, f, :3] = huge_id
                    marked[w, f, -3:] = huge_id
        outs = []
        for wts, tensor in ((weights, ids), (weights_huge, marked)):
            eng = JaegerHipEngine(model_cfg=cfg, weights=wts, device_id=0, precision="f32")
            try:
                last = local_ops(eng.program)[-1]
                outs.append(eng.model.tap(last, tensor)[mid[0], mid[1]])
                if wts is weights_huge:
                    x = eng.model.tap(producer(eng.program, local_ops(eng.program)[0]), tensor)
                    assert np.abs(x[0, 2, -1]).max() > 1e28 and np.abs(x[0, 4, 0]).max() > 1e28      # the neighbours do hold them
            finally:
                eng.close()
        assert np.isfinite(outs[0]).all()
        np.testing.assert_array_equal(outs[0], outs[1], err_msg=f"L {l}: the middle row changed with its neighbours' row ends")


def test_other_sizes_are_refused_at_model_creation():
    """The plan refuses them first; a program that reaches the library anyway is refused there, with the reason."""
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd.engine import HipDevice, HipModel
    from jaeger_amd.program import compile_plan
    cfg = variant("fixture")
    prog = compile_plan(P.build_plan(cfg), lr.random_weights(cfg))
    i = local_ops(prog)[0]
    dev = HipDevice(0)
    try:
        for field, value, word in (("k", 3, "heads"), ("arg", 520, "feed-forward width"), ("arg", 0, "feed-forward width"),
                                   ("stride", 33, "half-window"), ("out_buf", prog.ops[i].in_buf, "in place"),
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


def test_cli_predict_local_attention_model(tmp_path, monkeypatch):
    """``python -m jaeger_amd predict`` with a localattn500 model directory (fixture yaml, classes file, .weights.npz)
    against the reference composition, as tests/test_gpu_frameattn.py does it for the cross-frame model."""
    from click.testing import CliRunner

    import test_gpu_cli as tc
    from jaeger_amd.cli import main
    from jaeger_amd.fragment import read_fasta
    from jaeger_amd.weights import load_npz
    from oracle import forward as ofwd
    root = make_model_dir(tmp_path / "m", name="localattn500")
    cfg = load_model_cfg("localattn500")
    weights = load_npz(next((root / "model").glob("*.weights.npz")))
    assert set(weights) == set(lr.weight_specs(cfg))
    fasta = GOLDEN / "test_contigs.fasta"
    r = CliRunner().invoke(main, ["predict", "-i", str(fasta), "-o", str(tmp_path / "out"), "--model_path", str(root),
                                  "--fsize", "500", "--stride", "500", "--no-dustmask"])
    assert r.exit_code == 0, r.output
    tsv = list((tmp_path / "out").rglob("test_contigs.tsv"))
    assert len(tsv) == 1, list((tmp_path / "out").rglob("*"))
    monkeypatch.setattr(ofwd, "forward", lambda c, w, ids, dtype=None: {
        k: v.astype(np.float32) for k, v in lr.forward(c, w, ids).items()})
    records = [(n, s.decode()) for n, s in read_fasta(str(fasta))]
    exp, _, _ = tc._expected(tmp_path, records, cfg, weights, 500, 500, None, 96)
    tc._compare_tsv(tsv[0], exp)
