"""Frame attention on the CPU tier (the GPU tier is tests/test_gpu_frameattn.py):

(a) the float64 restatement of ``CrossFrameAttention`` (tests/attention_reference.py) against torch's own multi-head
    attention and layer norm in float64;
(b) what the layer's structure implies: frames permute through it, positions do not see each other, ``use_ffn: false`` is
    the first half;
(c) ``tests/golden/crossframe500_project.yaml`` -> plan -> program: one frame-attention op, no mask behind it;
(d) the refusals;
(e) a numpy emulation of the kernel's arithmetic sets the per-op bound (a power of two at or above 4 x its own error against
    the restatement), and every mutation - the bugs such a kernel typically has - lies at least 8 x outside it.  The
    errors, the bounds and each mutation's ratio are printed (pytest -s).
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_reference as ar
from conftest import load_model_cfg

SIZES = {"32/4/128": (32, 4, 128, True), "64/8/256": (64, 8, 256, True), "32/4 no ffn": (32, 4, 0, False),
         "32/1/128": (32, 1, 128, True), "64/2/64": (64, 2, 64, True)}


def _layer(size, seed=3):
    c, h, f, ffn = SIZES[size]
    rng = np.random.Generator(np.random.PCG64(seed))
    return ar.random_layer_weights(ar.layer_specs(c, h, f, ffn), rng), c, h, ffn


def _inputs(c, seed=5, l=23):
    """(name, x (B, 6, L, C) f32): unit normal; activations as they come out of a GELU (one-sided, a few large); rows with
    a common offset far above their spread (the layer norm's cancellation); exact zeros at 'padded' positions."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.normal(0, 1, (3, 6, l, c))
    gelu = np.maximum(x, 0) * rng.choice([1.0, 1.0, 1.0, 8.0], x.shape)
    offset = 0.05 * x + rng.normal(0, 3, (3, 6, l, 1))
    padded = x.copy()
    padded[:, :, l // 2:] = 0.0
    padded[1, 2:, 3:] = 0.0
    return [(n, v.astype(np.float32)) for n, v in (("normal", x), ("gelu-like", gelu), ("offset rows", offset), ("zero rows", padded))]


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
def test_restatement_against_torch(size):
    w, c, h, ffn = _layer(size)
    d = c // h
    t = lambda name: torch.as_tensor(np.asarray(w[name], np.float64))
    for name, x in _inputs(c):
        x64 = torch.as_tensor(x.astype(np.float64))
        b, fr, l, _ = x64.shape
        tok = x64.permute(1, 0, 2, 3).reshape(fr, b * l, c)                               # (6 tokens, B L, C): sequence first
        xn = F.layer_norm(tok, (c,), t("attn_norm/gamma"), t("attn_norm/beta"), 1e-6)
        in_w = torch.cat([t(f"mha/{p}/kernel").reshape(c, h * d).T for p in ("query", "key", "value")])
        in_b = torch.cat([t(f"mha/{p}/bias").reshape(h * d) for p in ("query", "key", "value")])
        out, _ = F.multi_head_attention_forward(
            xn, xn, xn, c, h, in_w, in_b, None, None, False, 0.0, t("mha/attention_output/kernel").reshape(h * d, c).T,
            t("mha/attention_output/bias"), training=False, need_weights=False)
        y = tok + out
        if ffn:
            yn = F.layer_norm(y, (c,), t("ffn_norm/gamma"), t("ffn_norm/beta"), 1e-6)
            y = y + F.gelu(yn @ t("ffn_dense1/kernel") + t("ffn_dense1/bias"), approximate="tanh") @ t("ffn_dense2/kernel") \
                + t("ffn_dense2/bias")
        want = y.reshape(fr, b, l, c).permute(1, 0, 2, 3).numpy()
        got = ar.cross_frame_attention(x, w, h, ffn)
        elem, rms = ar.errors(got, want)
        print(f"{size:12s} {name:12s} restatement vs torch float64: max {elem:.2e}, rms {rms:.2e} (of the output's rms)")
        assert elem < 1e-12, (size, name, elem)


# ---- (b) ----------------------------------------------------------------------------------------------------------------
def test_structure():
    w, c, h, ffn = _layer("32/4/128")
    x = _inputs(c)[0][1]
    y = ar.cross_frame_attention(x, w, h)
    perm = np.array([3, 0, 5, 1, 4, 2])
    assert ar.errors(ar.cross_frame_attention(x[:, perm], w, h), y[:, perm])[0] < 1e-13          # frames permute through
    x2 = np.random.Generator(np.random.PCG64(9)).normal(0, 2, x.shape).astype(np.float32)
    x2[:, :, 7] = x[:, :, 7]
    assert np.array_equal(ar.cross_frame_attention(x2, w, h)[:, :, 7], y[:, :, 7])             # a position sees itself only
    first = ar.cross_frame_attention(x, w, h, first_half_only=True)
    w_noffn = {k: v for k, v in w.items() if not k.startswith("ffn")}
    assert np.array_equal(ar.cross_frame_attention(x, w_noffn, h, use_ffn=False), first)        # use_ffn: false = the first half
    assert ar.errors(first, y)[1] > 1e-2                                                         # (and the second half does something)


# ---- (c) ----------------------------------------------------------------------------------------------------------------
def test_fixture_compiles_to_one_attention_op_and_no_mask_behind_it():
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    cfg = load_model_cfg("crossframe500")
    plan = P.build_plan(cfg)
    att = [l for l in plan.rep if isinstance(l, P.FrameAttn)]
    assert len(att) == 1 and (att[0].channels, att[0].heads, att[0].key_dim, att[0].ff_dim, att[0].use_ffn) == (32, 4, 8, 128, True)
    assert {n: tuple(s) for n, s in P.weight_shapes(plan).items()} == {n: tuple(s) for n, s in ar.weight_specs(cfg).items()}
    w = ar.random_weights(cfg)
    prog = G.compile_plan(plan, w)
    kinds = [op.kind for op in prog.ops]
    assert kinds.count(L.OP_FRAMEATTN) == 1
    at = kinds.index(L.OP_FRAMEATTN)
    op = prog.ops[at]
    assert (op.cin, op.cout, op.k, op.arg, op.out_mask, op.in_buf != op.out_buf) == (32, 32, 4, 128, L.JG_BUF_NONE, True)
    assert abs(op.f0 - 1e-6) < 1e-12
    assert [prog.ops[at].stages[s].kind for s in range(op.n_stages)] == [L.ST_BN]      # the batch norm behind it rides the store
    for later in prog.ops[at + 1:]:
        assert later.kind != L.OP_MASK and later.in_mask == L.JG_BUF_NONE and later.out_mask == L.JG_BUF_NONE
    pool = [o for o in prog.ops if o.kind == L.OP_POOL][0]
    assert pool.arg == L.POOL_AVG and pool.in_mask == L.JG_BUF_NONE and pool.in_buf == op.out_buf
    assert any("FRAMEATTN" in row and "heads=4 ff=128" in row for row in prog.describe())
    # the packed weights are the fold the emulation restates, bit for bit
    fw = ar.fold(ar.sub_weights(w, att[0].name), 4, True)
    want = np.concatenate([fw[k].ravel() for k in ("wq", "wk", "wv", "bq", "bk", "bv", "wo", "bo", "w1", "b1", "w2", "b2")])
    assert np.array_equal(prog.blob[op.w_off:op.w_off + want.size], want)
    flops = P.frame_attn_flops_per_position(plan)
    assert flops == [("rep/6", 6 * (8 * 32 * 32 + 4 * 32 * 128), 4 * 36 * 32)]            # ~150 kFLOP per position


def test_layernorm_behind_attention_is_cut_into_its_own_op():
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    cfg = load_model_cfg("crossframe500")
    layers = cfg["representation_learner"]["hidden_layers"]
    layers[-1] = {"name": "masked_layernorm", "config": {}}
    layers.append({"name": "activation", "config": {"activation": "gelu"}})
    plan = P.build_plan(cfg)
    from jaeger_amd.weights import random_weights
    prog = G.compile_plan(plan, random_weights(plan))
    kinds = [op.kind for op in prog.ops]
    at = kinds.index(L.OP_FRAMEATTN)
    assert prog.ops[at].n_stages == 0 and kinds[at + 1] == L.OP_ELTWISE
    ln = prog.ops[at + 1]
    assert [ln.stages[s].kind for s in range(ln.n_stages)] == [L.ST_LN, L.ST_ACT] and ln.stages[0].arg == 0 and ln.out_mask == L.JG_BUF_NONE


def test_model_reference_uses_the_values_at_masked_positions():
    """The composed forward: what the network holds at padded positions reaches the output (the mask is gone behind the
    attention layer) - the same valid codons with other padding ids in front of ... cannot be told here, but the same
    window padded to another length gives another embedding, where a masked average would not."""
    cfg = load_model_cfg("crossframe500")
    w = ar.random_weights(cfg)
    ids = ar.window_ids(60, "ragged", n_win=3)
    a = ar.forward(cfg, w, ids)
    longer = np.concatenate([ids, np.zeros((3, 6, 9), np.uint8)], axis=2)
    b = ar.forward(cfg, w, longer)
    assert a["prediction"].shape == (3, 3) and a["embedding"].shape == (3, 32)
    assert np.abs(a["embedding"] - b["embedding"]).max() > 1e-3
    masked = copy.deepcopy(cfg)
    masked["representation_learner"]["hidden_layers"] = [l for l in masked["representation_learner"]["hidden_layers"]
                                                         if l["name"] != ar.ATTN]
    from oracle import forward as of
    wm = {k: v for k, v in w.items() if not k.startswith("rep/6/")}
    wm.update({k.replace("rep/7/", "rep/6/"): v for k, v in w.items() if k.startswith("rep/7/")})
    a0 = of.forward(masked, wm, ids, dtype=torch.float64)
    b0 = of.forward(masked, wm, longer, dtype=torch.float64)
    assert np.abs(a0["embedding"] - b0["embedding"]).max() < 1e-12           # (the masked model does not see the padding)


# ---- (d) ----------------------------------------------------------------------------------------------------------------
def _with_attention(**over):
    cfg = load_model_cfg("crossframe500")
    layer = [l for l in cfg["representation_learner"]["hidden_layers"] if l["name"] == ar.ATTN][0]
    layer["config"].update(over)
    return cfg


@pytest.mark.parametrize("over, word", [
    (dict(embed_dim=64), "embed_dim 64 != 32 incoming channels"),
    (dict(num_heads=3), "num_heads 3"),
    (dict(num_heads=16), "key_dim"),
    (dict(feed_forward_dim=512), "feed_forward_dim 512"),
    (dict(feed_forward_dim=100), "feed_forward_dim 100"),
])
def test_plan_refusals_name_the_limit(over, word):
    from jaeger_amd import plan as P
    with pytest.raises(P.UnsupportedLayer, match=word):
        P.build_plan(_with_attention(**over))


def test_plan_refuses_other_widths_frame_counts_heads_and_strand_branches():
    from jaeger_amd import plan as P
    cfg = load_model_cfg("crossframe500")
    for layer in cfg["representation_learner"]["hidden_layers"]:
        if "filters" in layer["config"]:
            layer["config"]["filters"] = 48
        if "embed_dim" in layer["config"]:
            layer["config"]["embed_dim"] = 48
    with pytest.raises(P.UnsupportedLayer, match="embed_dim 48 .*32 / 64"):
        P.build_plan(cfg)
    cfg = load_model_cfg("crossframe500")
    cfg["embedding"]["input_shape"] = [3, None]
    with pytest.raises(P.UnsupportedLayer, match="over 3 frames"):
        P.build_plan(cfg)
    cfg = load_model_cfg("crossframe500")
    cfg["classifier"]["hidden_layers"].insert(0, {"name": ar.ATTN, "config": dict(embed_dim=32, num_heads=4, feed_forward_dim=128)})
    with pytest.raises(P.UnsupportedLayer, match="head or on a strand branch"):
        P.build_plan(cfg)
    cfg = load_model_cfg("dvf500")
    cfg["representation_learner"]["branch"]["hidden_layers"].insert(
        1, {"name": ar.ATTN, "config": dict(embed_dim=32, num_heads=4, feed_forward_dim=128)})
    with pytest.raises(P.UnsupportedLayer):
        P.build_plan(cfg)
    for other in ("transformer_encoder", "axial_attention", "local_attention", "hyena_block", "masked_bilstm"):
        cfg = load_model_cfg("crossframe500")
        cfg["representation_learner"]["hidden_layers"][6] = {"name": other, "config": {}}
        with pytest.raises(P.UnsupportedLayer, match="outside the Conv1D"):
            P.build_plan(cfg)
    cfg = load_model_cfg("crossframe500")
    cfg["representation_learner"]["pooling"] = "gatedframe"
    with pytest.raises(P.UnsupportedLayer):
        P.build_plan(cfg)


def test_nmd_tap_behind_attention_is_refused():
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    from jaeger_amd.weights import random_weights
    cfg = load_model_cfg("crossframe500")
    cfg["representation_learner"]["hidden_layers"][7]["config"]["return_nmd"] = True
    plan = P.build_plan(cfg)
    with pytest.raises(P.UnsupportedLayer, match="nmd tap directly behind cross_frame_attention"):
        G.compile_plan(plan, random_weights(plan))


def test_h5_bundle_and_verify_model_refuse_loudly(tmp_path):
    from jaeger_amd import plan as P
    from jaeger_amd import weights as W
    from jaeger_amd.verify import verify_model
    plan = P.build_plan(load_model_cfg("crossframe500"))
    with pytest.raises(W.AttentionWeightsUnsupported, match=r"weights\.npz"):
        W.load_keras3_h5(tmp_path / "m.weights.h5", plan)
    with pytest.raises(W.AttentionWeightsUnsupported, match=r"weights\.npz"):
        W.load_savedmodel_bundle(tmp_path / "m_graph", plan)
    with pytest.raises(P.UnsupportedLayer, match=r"verify-model does not cover cross_frame_attention.*weights\.npz"):
        verify_model(tmp_path / "m_graph", plan)
    # the npz route: seeded weights round-trip under the canonical names
    w = W.random_weights(plan)
    assert set(w) == set(ar.weight_specs(load_model_cfg("crossframe500")))
    W.save_npz(tmp_path / "m.weights.npz", w)
    back = W.load_weights({"weights_npz": tmp_path / "m.weights.npz"}, plan)
    assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
    # a bundle beside the npz: the bundle loader's refusal falls through to the file, with a warning
    (tmp_path / "m_graph" / "variables").mkdir(parents=True)
    (tmp_path / "m_graph" / "variables" / "variables.index").write_bytes(b"")
    with pytest.warns(RuntimeWarning, match="cross_frame_attention"):
        back = W.load_weights({"graph": tmp_path / "m_graph", "weights_npz": tmp_path / "m.weights.npz"}, plan)
    assert set(back) == set(w)
    with pytest.raises(W.AttentionWeightsUnsupported):
        W.load_weights({"graph": tmp_path / "m_graph"}, plan)


def test_verify_model_command_refuses(tmp_path):
    from click.testing import CliRunner

    from jaeger_amd.cli import main
    from conftest import GOLDEN
    (tmp_path / "g").mkdir()
    res = CliRunner().invoke(main, ["verify-model", str(tmp_path / "g"), "--project", str(GOLDEN / "crossframe500_project.yaml")])
    assert res.exit_code != 0 and "cross_frame_attention" in res.output and "weights.npz" in res.output


# ---- (e) ----------------------------------------------------------------------------------------------------------------
#: a broken emulation would set a useless bound: its own error must stay where f32 arithmetic puts it.  The worst input
#: here is "offset rows" (row offset 3, spread 0.05: the layer norm's subtraction loses log2(60) ~ 6 bits, and 1 / std = 20
#: scales what is left): 2^-24 x 60 x 20 ~ 7e-5 of a unit-scale output; 2^-12 = 2.4e-4 is the next power of two with
#: room above that, and still below the weakest mutation (erf-GELU, 5e-4 element error on the well-conditioned inputs)
EMULATION_SANITY = 2.0 ** -12


def test_emulation_sets_the_bound_and_every_mutation_fails_it():
    weakest = (np.inf, "")
    worst_emu = (0.0, 0.0, "")
    for size in ("32/4/128", "64/8/256"):
        w, c, h, ffn = _layer(size)
        caught = {m: (0.0, "") for m in ar.MUTATIONS}
        for name, x in _inputs(c):
            ref = ar.cross_frame_attention(x, w, h, ffn)
            b = ar.bounds_from(ar.emulate(x, w, h, ffn), ref)
            worst_emu = max(worst_emu, (b["emu_elem"], b["emu_rms"], f"{size} / {name}"))
            print(f"{size:9s} {name:12s} emulation: max {b['emu_elem']:.3g} rms {b['emu_rms']:.3g} -> bound max 2^{int(np.log2(b['elem']))} "
                  f"= {b['elem']:.3g} (headroom {b['elem'] / b['emu_elem']:.1f}x), rms 2^{int(np.log2(b['rms']))} = {b['rms']:.3g} "
                  f"(headroom {b['rms'] / b['emu_rms']:.1f}x)")
            assert b["elem"] >= ar.HEADROOM * b["emu_elem"] and b["rms"] >= ar.HEADROOM * b["emu_rms"]
            assert b["emu_elem"] < EMULATION_SANITY, "the emulation itself is off"
            for m in ar.MUTATIONS:
                e, r = ar.errors(ar.cross_frame_attention(x, w, h, ffn, mutation=m), ref)
                caught[m] = max(caught[m], (max(e / b["elem"], r / b["rms"]), f"{size} / {name}: max {e:.3g}, rms {r:.3g}"))
        for m, (s, where) in sorted(caught.items(), key=lambda kv: kv[1][0]):
            print(f"{s:12.3g}x  {m}  <-  {where}")
            assert s >= ar.MUTATION_MARGIN, (size, m, s, where)
            weakest = min(weakest, (s, f"{m} ({size})"))
    print(f"worst emulation error: max {worst_emu[0]:.3g}, rms {worst_emu[1]:.3g} of the output's rms ({worst_emu[2]}); "
          f"smallest mutation: {weakest[0]:.3g}x its bound ({weakest[1]}; >= {ar.MUTATION_MARGIN:g} required)")


@pytest.mark.parametrize("size", ["32/4 no ffn", "32/1/128", "64/2/64"])
def test_emulation_on_the_other_sizes(size):
    w, c, h, ffn = _layer(size)
    for name, x in _inputs(c):
        b = ar.bounds_from(ar.emulate(x, w, h, ffn), ar.cross_frame_attention(x, w, h, ffn))
        print(f"{size:12s} {name:12s} emulation: max {b['emu_elem']:.3g} rms {b['emu_rms']:.3g}")
        assert b["emu_elem"] < EMULATION_SANITY
