"""Frame attention on the GPU (the CPU tier is tests/test_frameattn_reference.py).

Models with ``cross_frame_attention`` layers through ``HipModel.forward`` and ``predict_windows`` in both arithmetics of
the conv stack, on full, ragged and nearly empty windows - behind the attention layer no mask exists, so what the network
holds at padded positions reaches the outputs and must be what the Keras graph holds there:

* logits, embedding and NMD against the composed float64 reference (tests/attention_reference.py: oracle/forward.py's
  layers around the restated attention layer) at the project's gate of 1e-4;
* per op: the tensor the attention op writes (``jg_model_set_tap``) against the restatement applied to the op's own
  read-back input.  The bound is not a constant: it is the error of the numpy emulation of the kernel's arithmetic on the
  same input, times 4, rounded up to a power of two (element error and RMS error, in units of the output's RMS) - the rule
  tests/test_frameattn_reference.py measures and holds every mutation 8x outside of;
* bit-identical outputs across launch-group sizes and between the id-tensor and the fused entry point;
* the variant bits of the tapped launch, and one launch per attention layer and launch group.

No test here provokes a fault; every test runs under a watchdog that ends the process if a GPU call does not return.
"""
import copy
import faulthandler

import numpy as np
import pytest

import attention_reference as ar
from conftest import GOLDEN, load_model_cfg, make_model_dir
from mixer_reference import producer

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
    print("\nattention op against the restatement on its own input (errors in units of the output's rms):")
    for row in _TABLE:
        print("  " + row)


# ---- models -----------------------------------------------------------------------------------------------------------
def variant(name: str) -> dict:
    cfg = copy.deepcopy(load_model_cfg("crossframe500"))
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    att = [l for l in layers if l["name"] == ar.ATTN][0]["config"]
    if name == "fixture":
        pass
    elif name == "wide":                                  # 64 channels, 8 heads, 256 hidden
        for layer in layers:
            if "filters" in layer["config"]:
                layer["config"]["filters"] = 64
        att.update(embed_dim=64, num_heads=8, feed_forward_dim=256)
        cfg["classifier"]["input_shape"] = 64
    elif name == "no_ffn":
        att["use_ffn"] = False
    elif name == "one_head":
        att["num_heads"] = 1
    elif name == "two_layers":
        layers.append({"name": ar.ATTN, "config": dict(embed_dim=32, num_heads=2, feed_forward_dim=64, dropout_rate=0.1)})
        layers.append({"name": "activation", "config": {"activation": "gelu"}})
    elif name == "then_conv":                             # f32 rows -> the next conv's F16S in the split-f16 program
        layers += [{"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same")},
                   {"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]
    elif name == "pool_max":
        rep["pooling"] = "max"
    elif name == "nmd_front":
        layers.insert(1, {"name": "nmd", "config": {}})
    else:
        raise ValueError(name)
    return cfg


VARIANTS = ("fixture", "wide", "no_ffn", "one_head", "two_layers", "then_conv", "pool_max", "nmd_front")
KINDS = ("full", "ragged", "few")


def windows(kind: str, n_win: int = 5, seed: int = 17):
    """DNA for ``n_win`` windows of up to FSIZE bases: ``full`` - whole windows; ``ragged`` - lengths between a third of a
    window and a whole one, with N runs; ``few`` - 24 .. 45 bases, a handful of valid codons per frame."""
    rng = np.random.Generator(np.random.PCG64(seed + KINDS.index(kind)))
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, FSIZE * n_win)].copy()
    starts = (np.arange(n_win) * FSIZE).astype(np.int64)
    if kind == "full":
        lens = np.full(n_win, FSIZE, np.int32)
    elif kind == "ragged":
        lens = rng.integers(FSIZE // 3, FSIZE + 1, n_win).astype(np.int32)
        lens[0] = FSIZE
        for w in range(1, n_win, 2):
            a = int(starts[w] + rng.integers(0, lens[w] - 12))
            seq[a:a + 7] = ord("N")
    else:
        lens = rng.integers(24, 46, n_win).astype(np.int32)
    return seq, starts, lens


def encode(seq, starts, lens):
    from oracle import encoder as oenc
    wins = [seq[s:s + n].tobytes() for s, n in zip(starts, lens)]
    return oenc.encode_windows(wins, FSIZE, pad_to=oenc.frame_length(FSIZE))


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


def attention_ops(prog):
    from jaeger_amd import _lib as L
    return [i for i, op in enumerate(prog.ops) if op.kind == L.OP_FRAMEATTN]


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("name", VARIANTS)
def test_model_outputs_and_attention_op(name, precision):
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import JaegerHipEngine
    cfg = variant(name)
    weights = ar.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision=precision)
    try:
        assert eng.model.precision == precision
        assert not eng.model.placement()["small_fused"]              # layer by layer: the fused whole-row kernels do not match
        prog = eng.program
        att = attention_ops(prog)
        n_layers = len(ar.attention_layers(cfg))
        assert len(att) == n_layers
        assert "frame attention" in eng.model.describe()
        if precision == "f16x3":
            # the op's producer stores f32 rows for it (the format pass gives a conv's output its first reader's layout), so
            # only a split-f16 conv BEHIND the op needs a conversion: the queued f32 -> F16S launch in front of that conv
            assert eng.model.placement()["convs_f16x3"] >= 1
            if name == "then_conv":
                assert eng.model.placement()["layout_conversions"] >= 1, eng.model.placement()
        for kind in KINDS:
            what = f"{name} / {precision} / {kind}"
            seq, starts, lens = windows(kind)
            ids = encode(seq, starts, lens)
            ref = ar.forward(cfg, weights, ids)
            got = eng.model.forward(ids)
            errs = check_vectors(what, got, ref)
            print(what, {k: f"{v:.2e}" for k, v in errs.items()})
            # launch groups of 2 + 2 + 1 windows, and the fused entry point: bit for bit the same
            split = eng.model.forward(ids, chunk=2)
            fused = eng.predict_windows(seq, starts, lens, FSIZE)
            eng.chunk = 2
            fused2 = eng.predict_windows(seq, starts, lens, FSIZE)
            eng.chunk = 0
            for k in got:
                np.testing.assert_array_equal(got[k], split[k], err_msg=f"{what} {k}: chunk 2")
                np.testing.assert_array_equal(got[k], fused[k], err_msg=f"{what} {k}: predict_windows")
                np.testing.assert_array_equal(got[k], fused2[k], err_msg=f"{what} {k}: predict_windows, chunk 2")
            # per op: the attention op's own output from its own read-back input
            for i in att:
                op = prog.ops[i]
                x = eng.model.tap(producer(prog, i), ids)
                y = eng.model.tap(i, ids)
                bits = eng.model.tap_variant()
                assert bits & L.TAP_EXACT_F32 and not bits & (L.TAP_F16S | L.TAP_PHASE_SPLIT), (what, bits)
                np.testing.assert_array_equal(y, eng.model.tap(i, ids, chunk=2), err_msg=f"{what} op {i}: chunk 2")
                lw = ar.sub_weights(weights, f"rep/{ar.attention_layers(cfg)[att.index(i)][0]}")
                use_ffn = op.arg > 0
                want = ar.apply_stages(ar.cross_frame_attention(x, lw, op.k, use_ffn), prog, op)
                emu = ar.apply_stages(ar.emulate(x, lw, op.k, use_ffn), prog, op, dtype=np.float32)
                b = ar.bounds_from(emu, want)
                e, r = ar.errors(y, want)
                _TABLE.append(f"{what:34s} op {i:2d}: max {e:.3g} (emulation {b['emu_elem']:.3g}, bound {b['elem']:.3g}), "
                              f"rms {r:.3g} (emulation {b['emu_rms']:.3g}, bound {b['rms']:.3g})")
                print(_TABLE[-1])
                assert e <= b["elem"] and r <= b["rms"], _TABLE[-1]
        # one launch per attention layer and launch group
        seq, starts, lens = windows("full")
        ids = encode(seq, starts, lens)
        for chunk, groups in ((0, 1), (2, 3)):
            eng.device.profile_enable(True)
            eng.model.forward(ids, chunk=chunk)
            prof = eng.device.profile_read()
            eng.device.profile_enable(False)
            assert prof["frame_attn"]["launches"] == n_layers * groups, (name, chunk, prof["frame_attn"])
    finally:
        eng.close()


def test_other_sizes_are_refused_at_model_creation():
    """The plan refuses them first; a program that reaches the library anyway is refused there, with the reason."""
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd.engine import HipDevice, HipModel
    from jaeger_amd.program import compile_plan
    cfg = variant("fixture")
    prog = compile_plan(P.build_plan(cfg), ar.random_weights(cfg))
    i = attention_ops(prog)[0]
    dev = HipDevice(0)
    try:
        for field, value, word in (("k", 3, "heads"), ("arg", 520, "feed-forward width")):
            bad = copy.copy(prog)
            bad.ops = list(prog.ops)
            op = L.JgOp.from_buffer_copy(prog.ops[i])
            setattr(op, field, value)
            bad.ops[i] = op
            with pytest.raises(L.JaegerHipError, match=word):
                HipModel(dev, bad)
    finally:
        dev.close()


def test_cli_predict_crossframe_model(tmp_path, monkeypatch):
    """``python -m jaeger_amd predict`` with a crossframe500 model directory (fixture yaml, classes file, .weights.npz)
    against the reference composition: same fragmenter, encoder and postprocess as tests/test_gpu_cli.py, the forward
    through tests/attention_reference.py."""
    from click.testing import CliRunner

    import test_gpu_cli as tc
    from jaeger_amd.cli import main
    from jaeger_amd.fragment import read_fasta
    from jaeger_amd.weights import load_npz
    from oracle import forward as ofwd
    root = make_model_dir(tmp_path / "m", name="crossframe500")
    cfg = load_model_cfg("crossframe500")
    weights = load_npz(next((root / "model").glob("*.weights.npz")))
    assert set(weights) == set(ar.weight_specs(cfg))
    fasta = GOLDEN / "test_contigs.fasta"
    r = CliRunner().invoke(main, ["predict", "-i", str(fasta), "-o", str(tmp_path / "out"), "--model_path", str(root),
                                  "--fsize", "500", "--stride", "500", "--no-dustmask"])
    assert r.exit_code == 0, r.output
    tsv = list((tmp_path / "out").rglob("test_contigs.tsv"))
    assert len(tsv) == 1, list((tmp_path / "out").rglob("*"))
    monkeypatch.setattr(ofwd, "forward", lambda c, w, ids, dtype=None: {
        k: v.astype(np.float32) for k, v in ar.forward(c, w, ids).items()})
    records = [(n, s.decode()) for n, s in read_fasta(str(fasta))]
    exp, _, _ = tc._expected(tmp_path, records, cfg, weights, 500, 500, None, 96)
    tc._compare_tsv(tsv[0], exp)
