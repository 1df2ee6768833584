"""Axial attention and the stand-alone transformer encoder on the CPU tier (the GPU tier is tests/test_gpu_axialattn.py):

(1) the float64 restatement of ``TransformerEncoder`` under Keras 3's implicit masks (tests/axial_attention_reference.py)
    against torch's own multi-head attention with ``key_padding_mask`` at every valid query, and against the closed form
    ``x + b_o`` followed by the feed-forward half at every masked query;
(2) the host-side fold, evaluated plainly, equals the restatement;
(3) a numpy emulation of the kernel's arithmetic (online softmax, 16 keys a step) sets the per-op bound (a power of two at
    or above 4 x its own error against the restatement, element and RMS error in units of the output's RMS);
(4) every mutation lies at least 8 x outside that bound on the input kinds named for it; where a mutation cannot show on
    a kind it is printed as invisible there (pytest -s);
(5) the fixture model (tests/golden/axial500_project.yaml) -> plan -> program, the refusals, the weight loaders;
(6) the new symbols and constants of the C-ABI.
"""
import copy
import ctypes
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_reference as ar
import axial_attention_reference as xr
from conftest import ROOT, load_model_cfg

#: channels / heads / feed-forward width
SIZES = {"16/2/32": (16, 2, 32), "32/4/128": (32, 4, 128), "64/8/256": (64, 8, 256), "32/8/64": (32, 8, 64), "32/1/16": (32, 1, 16)}
LENGTHS = (1, 5, 17, 70)


def _encoder(size, seed=3):
    c, h, f = SIZES[size]
    rng = np.random.Generator(np.random.PCG64(seed))
    return ar.random_layer_weights(xr.encoder_specs(c, h, f), rng), c, h


def _row_masks(l):
    """Five rows: all valid; right-padded from the middle on; an invalid run inside; one valid position alone; no valid
    position at all."""
    m = np.ones((5, l), bool)
    m[1, (l + 1) // 2:] = False
    m[2, l // 3:l // 3 + max(l // 4, 1)] = False
    m[3, :] = False
    m[3, l // 2] = True
    m[4, :] = False
    return m


# ---- (1) ----------------------------------------------------------------------------------------------------------------
#: the two float64 evaluations differ in the order of their sums alone, a few ulp of 2^-53 per term: the run shows 5.1e-15
#: of the output's rms at the valid queries and 2.7e-16 at the masked ones; asserted at the power of ten above
TORCH_TOL = 1e-14


def test_restatement_against_torch_and_the_closed_form_at_masked_queries():
    worst = worst_masked = 0.0
    seen_valid = seen_masked = 0
    for size in SIZES:
        w, c, h = _encoder(size)
        d = c // h
        t = lambda name: torch.as_tensor(np.asarray(w[name], np.float64))
        for l in LENGTHS:
            x = np.random.Generator(np.random.PCG64(l)).normal(0, 1, (5, l, c)).astype(np.float32)
            mask = _row_masks(l)
            got = xr.transformer_encoder(x, w, h, mask)
            # valid queries: torch's attention over the valid keys (rows without a valid key have no valid query: left out)
            rows = np.flatnonzero(mask.any(axis=1))
            tok = torch.as_tensor(x[rows].astype(np.float64)).permute(1, 0, 2)            # (L tokens, rows, C)
            xn = F.layer_norm(tok, (c,), t("attn_norm/gamma"), t("attn_norm/beta"), 1e-6)
            in_w = torch.cat([t(f"mha/{p}/kernel").reshape(c, h * d).T for p in ("query", "key", "value")])
            in_b = torch.cat([t(f"mha/{p}/bias").reshape(h * d) for p in ("query", "key", "value")])
            out, _ = F.multi_head_attention_forward(
                xn, xn, xn, c, h, in_w, in_b, None, None, False, 0.0, t("mha/attention_output/kernel").reshape(h * d, c).T,
                t("mha/attention_output/bias"), training=False, need_weights=False,
                key_padding_mask=torch.as_tensor(~mask[rows]))
            y = tok + out
            yn = F.layer_norm(y, (c,), t("ffn_norm/gamma"), t("ffn_norm/beta"), 1e-6)
            y = y + F.gelu(yn @ t("ffn_dense1/kernel") + t("ffn_dense1/bias"), approximate="tanh") @ t("ffn_dense2/kernel") + t("ffn_dense2/bias")
            want = y.permute(1, 0, 2).numpy()
            vq = mask[rows]
            e, _ = ar.errors(got[rows][vq], want[vq])
            worst = max(worst, e)
            seen_valid += int(vq.sum())
            # masked queries: x + b_o, then the feed-forward half
            x64 = x.astype(np.float64)
            tm = x64 + np.asarray(w["mha/attention_output/bias"], np.float64)
            g = lambda name: np.asarray(w[name], np.float64)
            hm = ar.gelu_tanh(ar.layer_norm(tm, g("ffn_norm/gamma"), g("ffn_norm/beta")) @ g("ffn_dense1/kernel") + g("ffn_dense1/bias"))
            closed = tm + hm @ g("ffn_dense2/kernel") + g("ffn_dense2/bias")
            if (~mask).any():
                em, _ = ar.errors(got[~mask], closed[~mask])
                worst_masked = max(worst_masked, em)
                seen_masked += int((~mask).sum())
            print(f"{size:10s} L {l:3d}: restatement vs torch float64 at {int(vq.sum()):3d} valid queries: max {e:.2e}; "
                  f"vs x + b_o -> feed-forward at {int((~mask).sum()):3d} masked queries: max {em if (~mask).any() else 0.0:.2e}")
    print(f"worst: valid queries {worst:.2e}, masked queries {worst_masked:.2e}")
    assert seen_valid > 0 and seen_masked > 0
    assert worst <= TORCH_TOL and worst_masked <= TORCH_TOL


def test_no_mask_means_every_position_and_masked_keys_are_invisible():
    w, c, h = _encoder("32/4/128")
    x = np.random.Generator(np.random.PCG64(1)).normal(0, 1, (2, 30, c)).astype(np.float32)
    y = xr.transformer_encoder(x, w, h, None)
    assert np.array_equal(y, xr.transformer_encoder(x, w, h, np.ones((2, 30), bool)))
    mask = np.ones((2, 30), bool)
    mask[:, 20:] = False
    x2 = x.copy()
    x2[:, 20:] = 1e3
    a, b = xr.transformer_encoder(x, w, h, mask), xr.transformer_encoder(x2, w, h, mask)
    assert np.array_equal(a[:, :20], b[:, :20]) and np.abs(a[:, 20:] - b[:, 20:]).max() > 1.0
    assert np.abs(a[:, :20] - y[:, :20]).max() > 1e-6                       # (and the masked keys did count without the mask)


# ---- (2) ----------------------------------------------------------------------------------------------------------------
#: as tests/test_localattn_reference.py: every folded weight is rounded to f32 once
FOLD_BOUND = 2.0 ** -20


@pytest.mark.parametrize("size", list(SIZES))
def test_fold_evaluated_plainly_is_the_restatement(size):
    w, c, h = _encoder(size)
    fw = xr.fold(w, h)
    for l in (17, 40):
        x = np.random.Generator(np.random.PCG64(l)).normal(0, 1, (5, l, c)).astype(np.float32)
        mask = _row_masks(l)
        e, r = ar.errors(xr.evaluate_fold(x, fw, h, mask), xr.transformer_encoder(x, w, h, mask))
        print(f"{size:10s} L {l}: folded operands vs restatement: max {e:.2e}, rms {r:.2e}")
        assert e <= FOLD_BOUND


# ---- (3) ----------------------------------------------------------------------------------------------------------------
EMULATION_SANITY = 2.0 ** -12          # as tests/test_localattn_reference.py: the emulation's own error stays where f32 puts it


@pytest.mark.parametrize("size", list(SIZES))
def test_emulation_sets_the_bound(size):
    w, c, h = _encoder(size)
    l = 70                                                             # five softmax steps, the last one ragged, two chunks
    for kind in ("ragged", "empty_fwd"):
        mask = xr.window_ids(l, kind, n_win=2)[1] != 0                      # (empty_fwd: window 1 holds the empty rows)
        for name, x in xr.value_inputs(c, 6, l):
            ref = xr.transformer_encoder(x, w, h, mask)
            emu = xr.emulate_encoder(x, w, h, mask)
            b = xr.bounds_from(emu, ref)
            print(f"{size:10s} {kind:9s} {name:12s} emulation: max {b['emu_elem']:.3g} rms {b['emu_rms']:.3g} -> bound max "
                  f"2^{int(np.log2(b['elem']))} = {b['elem']:.3g}, rms 2^{int(np.log2(b['rms']))} = {b['rms']:.3g}")
            assert b["elem"] >= ar.HEADROOM * b["emu_elem"] and b["rms"] >= ar.HEADROOM * b["emu_rms"]
            assert b["emu_elem"] < EMULATION_SANITY, "the emulation itself is off"
            assert np.isfinite(emu).all()
    # the step of the online softmax changes the rounding alone
    x = xr.value_inputs(c, 6, l)[0][1]
    a, b2 = xr.emulate_encoder(x, w, h, mask, step=16), xr.emulate_encoder(x, w, h, mask, step=l)
    assert ar.errors(a, b2.astype(np.float64))[0] < EMULATION_SANITY


# ---- (4) ----------------------------------------------------------------------------------------------------------------
def test_every_mutation_lies_outside_its_bound():
    c, h, f = SIZES["32/4/128"]
    blocks, l, eps = 2, 40, 1e-3              # (two blocks: block 1's rule; epsilon 1e-3: not the encoders' own 1e-6)
    w = xr.random_layer_weights(xr.layer_specs(c, h, f, blocks, "layernorm"), np.random.Generator(np.random.PCG64(3)))
    x = xr.value_inputs(c, 12, l)[0][1].reshape(2, 6, l, c)
    shown = {m: [] for m in xr.MUTATIONS}
    for kind in xr.KINDS:
        mask = xr.window_ids(l, kind, n_win=2, chunk=8) != 0
        ref = xr.axial_attention(x, w, h, blocks, "layernorm", eps, mask)
        b = xr.bounds_from(xr.emulate(x, w, h, blocks, "layernorm", eps, mask), ref)
        whole = int((~mask.any(axis=-1)).sum())
        print(f"{kind}: {int((~mask).sum())} masked positions, {whole} rows masked as a whole; emulation max {b['emu_elem']:.3g}; "
              f"bound max {b['elem']:.3g}, rms {b['rms']:.3g}")
        assert b["emu_elem"] < EMULATION_SANITY
        if kind == "empty_fwd":
            assert whole >= 3
        for m in xr.MUTATIONS:
            e, r = ar.errors(xr.axial_attention(x, w, h, blocks, "layernorm", eps, mask, mutation=m), ref)
            margin = max(e / b["elem"], r / b["rms"])
            required = kind in xr.VISIBLE_ON[m]
            print(f"    {margin:12.3g}x  {m:36s} {'' if required else ('invisible on this kind' if margin <= 1 else '(not required on this kind)')}")
            if required:
                assert margin >= ar.MUTATION_MARGIN, (m, kind, margin)
                shown[m].append(kind)
            elif kind == "full":
                assert margin == 0.0, (m, "a mask mutation changed an unmasked window")
    for m, kinds in shown.items():
        assert kinds, f"{m} is visible on no input kind"
    for need in ("key_mask_ignored", "query_mask_ignored", "masked_query_uniform", "mask_in_block1_as_well",
                 "post_norm_epsilon_in_inner_norms", "post_norm_masked_under_layernorm", "residual_taken_after_length_half",
                 "frame_half_before_length_half", "softmax_over_queries", "scale_sqrt_channels", "bias_dropped_at_masked_queries"):
        assert need in xr.MUTATIONS


@pytest.mark.parametrize("norm_type", xr.NORM_TYPES)
def test_post_norms_follow_the_mask_rule(norm_type):
    """masked_layernorm / masked_dyt see the incoming mask in every block (their output is zero at masked positions: the
    layer's output there is the block input alone); layernorm and masked_batchnorm see none."""
    c, h, f = SIZES["32/4/128"]
    w = xr.random_layer_weights(xr.layer_specs(c, h, f, 2, norm_type), np.random.Generator(np.random.PCG64(5)))
    x = xr.value_inputs(c, 6, 24)[0][1].reshape(1, 6, 24, c)
    mask = xr.window_ids(24, "ragged", n_win=1) != 0
    one = xr.axial_attention(x, w, h, 1, norm_type, 1e-6, mask)
    two = xr.axial_attention(x, w, h, 2, norm_type, 1e-6, mask)
    if norm_type in ("masked_layernorm", "masked_dyt"):
        assert np.array_equal(one[~mask], x.astype(np.float64)[~mask]) and np.array_equal(two[~mask], one[~mask])
    else:
        assert np.abs(one[~mask] - x[~mask]).min() > 0 and np.abs(two[~mask] - one[~mask]).max() > 1e-6
    with pytest.raises(ValueError, match="Unsupported norm_type"):
        xr.post_norm(x, {}, "batchnorm", 1e-6)


# ---- (5) ----------------------------------------------------------------------------------------------------------------
def _cfg(**over):
    cfg = copy.deepcopy(load_model_cfg("axial500"))
    layer = [l for l in cfg["representation_learner"]["hidden_layers"] if l["name"] == xr.AXIAL][0]
    layer["config"].update(over)
    return cfg


def _encoder_cfg(**over):
    cfg = _cfg()
    layers = cfg["representation_learner"]["hidden_layers"]
    at = [i for i, l in enumerate(layers) if l["name"] == xr.AXIAL][0]
    layers[at] = {"name": xr.ENCODER, "config": {**dict(embed_dim=32, num_heads=4, feed_forward_dim=128, dropout_rate=0.1), **over}}
    return cfg


def _compile(cfg):
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    from jaeger_amd.weights import random_weights
    plan = P.build_plan(cfg)
    return plan, G.compile_plan(plan, random_weights(plan))


def _kinds(prog):
    return [op.kind for op in prog.ops]


def test_fixture_is_the_reference_config_and_compiles_to_length_frame_norm_add():
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    cfg = load_model_cfg("axial500")
    att = [l for l in cfg["representation_learner"]["hidden_layers"] if l["name"] == xr.AXIAL]
    assert len(att) == 1 and att[0]["config"] == xr.FIXTURE
    plan = P.build_plan(cfg)                                              # (the parent commit refuses here)
    a = [l for l in plan.rep if isinstance(l, P.AxialAttn)]
    assert len(a) == 1 and (a[0].channels, a[0].heads, a[0].key_dim, a[0].ff_dim, a[0].blocks, a[0].norm_type, a[0].epsilon) == \
        (32, 4, 8, 128, 1, "layernorm", 1e-6)
    assert {n: tuple(s) for n, s in P.weight_shapes(plan).items()} == {n: tuple(s) for n, s in xr.weight_specs(cfg).items()}
    w = xr.random_weights(cfg)
    prog = G.compile_plan(plan, w)
    kinds = _kinds(prog)
    at = kinds.index(L.OP_LENGTHATTN)
    assert kinds.count(L.OP_LENGTHATTN) == 1 and kinds[at:at + 4] == [L.OP_LENGTHATTN, L.OP_FRAMEATTN, L.OP_ELTWISE, L.OP_POOL]
    ln, fa, el, pool = prog.ops[at:at + 4]
    assert (ln.cin, ln.cout, ln.k, ln.arg) == (32, 32, 4, 128) and abs(ln.f0 - 1e-6) < 1e-12 and ln.n_stages == 0
    assert ln.in_buf != ln.out_buf and ln.in_mask >= 0 and ln.out_mask == ln.in_mask
    assert fa.in_buf == ln.out_buf and fa.in_mask == fa.out_mask == L.JG_BUF_NONE and fa.arg == 128 and fa.n_stages == 0
    assert el.in_buf == el.out_buf == fa.out_buf and el.out_mask == ln.in_mask
    st = [el.stages[s] for s in range(el.n_stages)]
    assert [s.kind for s in st] == [L.ST_LN, L.ST_ADD, L.ST_BN]           # post norm, + block input, the norm behind the layer
    assert st[0].arg == 0 and abs(st[0].f0 - 1e-6) < 1e-12 and st[1].arg == ln.in_buf
    assert el.out_buf not in (ln.in_buf,)                                 # the block-input slot stays taken until the add
    assert pool.in_buf == el.out_buf and pool.in_mask == ln.in_mask       # the mask slot survives the layer
    assert any("LENGTHATTN" in row and "heads=4 ff=128" in row for row in prog.describe())
    # the packed weights are the fold the emulation restates, bit for bit
    want = xr.blob_of(xr.fold(ar.sub_weights(w, f"{a[0].name}/block0/length"), 4))
    assert np.array_equal(prog.blob[ln.w_off:ln.w_off + want.size], want)
    want = xr.blob_of(ar.fold(ar.sub_weights(w, f"{a[0].name}/block0/frame"), 4, True))
    assert np.array_equal(prog.blob[fa.w_off:fa.w_off + want.size], want)
    # existing models compile as before
    base = G.compile_plan(P.build_plan(load_model_cfg("crossframe500")), ar.random_weights(load_model_cfg("crossframe500")))
    assert L.OP_LENGTHATTN not in _kinds(base)


def test_block_one_is_unmasked_and_the_masked_post_norms_get_the_mask_in_every_block():
    from jaeger_amd import _lib as L
    for nt, lead, arg in (("layernorm", L.ST_LN, 0), ("masked_layernorm", L.ST_LN, 1), ("masked_dyt", L.ST_DYT, 1),
                          ("masked_batchnorm", L.ST_BN, 0)):
        _, prog = _compile(_cfg(num_blocks=2, norm_type=nt, epsilon=1e-3))
        ops = prog.ops
        at = [i for i, k in enumerate(_kinds(prog)) if k == L.OP_LENGTHATTN]
        assert len(at) == 2 and at[1] == at[0] + 3
        b0, b1 = ops[at[0]], ops[at[1]]
        assert b0.in_mask >= 0 and b0.out_mask == b0.in_mask
        assert b1.in_mask == L.JG_BUF_NONE and b1.out_mask == L.JG_BUF_NONE      # block 1's length half is unmasked
        assert abs(b0.f0 - 1e-6) < 1e-12 and abs(b1.f0 - 1e-6) < 1e-12              # the inner norms keep 1e-6
        for j, i in enumerate(at):
            el = ops[i + 2]
            assert el.kind == L.OP_ELTWISE and el.stages[0].kind == lead and el.stages[0].arg == arg, (nt, j)
            assert el.stages[1].kind == L.ST_ADD and el.stages[1].arg == ops[i].in_buf
            assert el.out_mask == b0.in_mask
            if lead == L.ST_LN:
                assert abs(el.stages[0].f0 - 1e-3) < 1e-9                      # the post norm's epsilon is the layer's
        assert b1.in_buf == ops[at[0] + 2].out_buf
        pool = [o for o in ops if o.kind == L.OP_POOL][0]
        assert pool.in_mask == b0.in_mask
    from jaeger_amd import plan as P
    alias = [l for l in P.build_plan(_cfg(norm_type="layer_normalization")).rep if isinstance(l, P.AxialAttn)]
    assert alias[0].norm_type == "layernorm"                                          # layers.py:2449


def test_stand_alone_encoder_takes_the_mask_and_drops_it():
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    cfg = _encoder_cfg()
    plan, prog = _compile(cfg)
    enc = [l for l in plan.rep if isinstance(l, P.LengthAttn)]
    assert len(enc) == 1 and (enc[0].channels, enc[0].heads, enc[0].ff_dim) == (32, 4, 128)
    assert {n: tuple(s) for n, s in P.weight_shapes(plan).items()} == {n: tuple(s) for n, s in xr.weight_specs(cfg).items()}
    assert f"{enc[0].name}/attn_norm/gamma" in P.weight_shapes(plan) and f"{enc[0].name}/ffn_dense2/bias" in P.weight_shapes(plan)
    op = [o for o in prog.ops if o.kind == L.OP_LENGTHATTN]
    assert len(op) == 1 and op[0].in_mask >= 0 and op[0].out_mask == L.JG_BUF_NONE
    assert [op[0].stages[s].kind for s in range(op[0].n_stages)] == [L.ST_BN]        # the norm behind it rides the store
    pool = [o for o in prog.ops if o.kind == L.OP_POOL][0]
    assert pool.in_mask == L.JG_BUF_NONE and pool.in_buf == op[0].out_buf
    _compile(_encoder_cfg(attention_axes=2))
    # behind cross_frame_attention no mask arrives
    cfg = _cfg()
    cfg["representation_learner"]["hidden_layers"].insert(6, {"name": ar.ATTN, "config": dict(embed_dim=32, num_heads=4, feed_forward_dim=128)})
    _, prog = _compile(cfg)
    op = [o for o in prog.ops if o.kind == L.OP_LENGTHATTN][0]
    assert op.in_mask == L.JG_BUF_NONE and op.out_mask == L.JG_BUF_NONE


@pytest.mark.parametrize("over, word", [
    (dict(embed_dim=64), "embed_dim 64 != 32 incoming channels"),
    (dict(num_heads=3), "num_heads 3"),
    (dict(num_heads=16), "key_dim"),
    (dict(feed_forward_dim=512), "feed_forward_dim 512"),
    (dict(feed_forward_dim=100), "feed_forward_dim 100"),
    (dict(feed_forward_dim=0), "feed_forward_dim 0"),
    (dict(num_blocks=0), "num_blocks 0"),
    (dict(norm_type="batchnorm"), "norm_type 'batchnorm'"),
])
def test_plan_refusals_name_the_limit(over, word):
    from jaeger_amd import plan as P
    with pytest.raises(P.UnsupportedLayer, match=word):
        P.build_plan(_cfg(**over))
    enc_over = {k: v for k, v in over.items() if k in ("embed_dim", "num_heads", "feed_forward_dim")}
    if enc_over:
        with pytest.raises(P.UnsupportedLayer, match=word):
            P.build_plan(_encoder_cfg(**enc_over))


def _width(cfg, c):
    for layer in cfg["representation_learner"]["hidden_layers"]:
        if "filters" in layer["config"]:
            layer["config"]["filters"] = c
    cfg["classifier"]["input_shape"] = c
    return cfg


def test_plan_refuses_other_widths_axes_heads_branches_frames_and_entries_the_constructor_refuses():
    from jaeger_amd import plan as P
    with pytest.raises(P.UnsupportedLayer, match="embed_dim 48 .*16 / 32 / 64"):
        P.build_plan(_width(_cfg(embed_dim=48), 48))
    with pytest.raises(P.UnsupportedLayer, match="axial_attention with embed_dim 16 .*32 / 64.*frame half"):
        P.build_plan(_width(_cfg(embed_dim=16, num_heads=2, feed_forward_dim=32), 16))
    P.build_plan(_width(_encoder_cfg(embed_dim=16, num_heads=2, feed_forward_dim=32), 16))       # the encoder alone runs at 16
    for axes in (1, 3, [1, 2]):
        with pytest.raises(P.UnsupportedLayer, match="attention_axes"):
            P.build_plan(_encoder_cfg(attention_axes=axes))
    for name, conf in ((xr.AXIAL, xr.FIXTURE), (xr.ENCODER, dict(embed_dim=32, num_heads=4, feed_forward_dim=128))):
        cfg = load_model_cfg("axial500")
        cfg["classifier"]["hidden_layers"].insert(0, {"name": name, "config": dict(conf)})
        with pytest.raises(P.UnsupportedLayer, match=f"{name}.*head or on a strand branch"):
            P.build_plan(cfg)
        cfg = load_model_cfg("dvf500")
        cfg["representation_learner"]["branch"]["hidden_layers"].insert(1, {"name": name, "config": dict(conf)})
        with pytest.raises(P.UnsupportedLayer):
            P.build_plan(cfg)
    cfg = _cfg()
    cfg["embedding"]["input_shape"] = [3, None]
    with pytest.raises(P.UnsupportedLayer, match="axial_attention over 3 frames"):
        P.build_plan(cfg)
    # what the reference's constructors refuse falls through to the generic refusal: a required argument missing, an
    # unknown keyword (the two entry shapes older tests pin: an empty config, one that carries window_size)
    for name, conf in ((xr.AXIAL, xr.FIXTURE), (xr.ENCODER, dict(embed_dim=32, num_heads=4, feed_forward_dim=128))):
        for bad in [{}] + [{k: v for k, v in conf.items() if k != gone} for gone in ("embed_dim", "num_heads", "feed_forward_dim")] + \
                [dict(conf, window_size=16), dict(conf, use_ffn=True)] + ([dict(conf, num_blocks=2)] if name == xr.ENCODER else [dict(conf, attention_axes=2)]):
            cfg = _cfg()
            cfg["representation_learner"]["hidden_layers"][6] = {"name": name, "config": bad}
            with pytest.raises(P.UnsupportedLayer, match="outside the Conv1D"):
                P.build_plan(cfg)
    for name in ("multi_scale_conv", "hyena_block", "masked_bilstm"):
        cfg = _cfg()
        cfg["representation_learner"]["hidden_layers"][6] = {"name": name, "config": dict(xr.FIXTURE)}
        with pytest.raises(P.UnsupportedLayer, match="outside the Conv1D"):
            P.build_plan(cfg)


def test_compiler_refusals_and_what_compiles_behind_the_layers():
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    conv = lambda **kw: {"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same", **kw)}
    res = lambda **kw: {"name": "residual_block", "config": dict(filters=32, kernel_size=3, **kw)}
    # the mask survives an axial layer: masked convs, residual blocks, masked norms, nmd taps behind a conv all compile
    for extra in ([conv()], [res()], [conv(), {"name": "nmd", "config": {}}], [{"name": "masked_layernorm", "config": {}}],
                  [{"name": "masked_dyt", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]):
        cfg = _cfg()
        cfg["representation_learner"]["hidden_layers"] += extra
        _, prog = _compile(cfg)
        if extra[0]["name"] == "masked_conv1d":
            c = [o for o in prog.ops if o.kind == L.OP_CONV][-1]
            assert c.in_mask >= 0
    for make, name in ((_cfg, "axial_attention"), (_encoder_cfg, "transformer_encoder")):
        cfg = make()
        cfg["representation_learner"]["hidden_layers"][7]["config"]["return_nmd"] = True
        with pytest.raises(P.UnsupportedLayer, match=f"nmd tap directly behind {name}"):
            _compile(cfg)
        cfg = make()
        cfg["representation_learner"]["hidden_layers"] = cfg["representation_learner"]["hidden_layers"][6:]
        cfg["embedding"]["embedding_size"] = 32
        with pytest.raises(P.UnsupportedLayer, match=f"{name} directly on the embedding"):
            _compile(cfg)
        # behind a masked local_attention whose dead positions are still live both are refused: they read masked positions
        cfg = make()
        cfg["representation_learner"]["hidden_layers"].insert(6, {"name": "local_attention", "config": dict(
            embed_dim=32, num_heads=4, feed_forward_dim=128, window_size=16)})
        with pytest.raises(P.UnsupportedLayer, match=name) as err:
            _compile(cfg)
        assert "local_attention" in str(err.value) and "reads masked positions unmasked" in str(err.value)
        # ... and with a masked conv between them (it reads valid positions only) they compile
        cfg["representation_learner"]["hidden_layers"].insert(7, conv())
        _compile(cfg)


def test_h5_bundle_and_verify_model_refuse_and_name_the_npz_route(tmp_path):
    from click.testing import CliRunner

    import yaml
    from jaeger_amd import plan as P
    from jaeger_amd import weights as W
    from jaeger_amd.cli import main
    from jaeger_amd.verify import verify_model
    for cfg, name in ((_cfg(num_blocks=2, norm_type="masked_batchnorm"), xr.AXIAL), (_encoder_cfg(), xr.ENCODER)):
        plan = P.build_plan(cfg)
        with pytest.raises(W.AttentionWeightsUnsupported, match=rf"{name}.*weights\.npz"):
            W.load_keras3_h5(tmp_path / "m.weights.h5", plan)
        with pytest.raises(W.AttentionWeightsUnsupported, match=rf"{name}.*weights\.npz"):
            W.load_savedmodel_bundle(tmp_path / "m_graph", plan)
        with pytest.raises(P.UnsupportedLayer, match=rf"verify-model does not cover {name}.*weights\.npz"):
            verify_model(tmp_path / "m_graph", plan)
        w = W.random_weights(plan)
        assert set(w) == set(xr.weight_specs(cfg)) and all(tuple(w[k].shape) == tuple(s) for k, s in xr.weight_specs(cfg).items())
        W.save_npz(tmp_path / f"{name}.weights.npz", w)
        back = W.load_weights({"weights_npz": tmp_path / f"{name}.weights.npz"}, plan)
        assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
        (tmp_path / f"g_{name}").mkdir()
        (tmp_path / f"{name}.yaml").write_text(yaml.safe_dump({"model": cfg}))
        res = CliRunner().invoke(main, ["verify-model", str(tmp_path / f"g_{name}"), "--project", str(tmp_path / f"{name}.yaml")])
        assert res.exit_code != 0 and name in res.output and "weights.npz" in res.output
    names = set(W.random_weights(P.build_plan(_cfg(norm_type="masked_batchnorm"))))
    assert {"rep/6/block0/length/attn_norm/gamma", "rep/6/block0/length/mha/query/kernel", "rep/6/block0/frame/ffn_dense1/kernel",
            "rep/6/block0/post_norm/moving_variance"} <= names


# ---- (6) ----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_constants():
    from jaeger_amd import _lib as L
    lib = L.load()
    header = (ROOT / "include" / "jaeger_hip.h").read_text()
    enum = lambda name: int(re.search(rf"\b{name}\s*=\s*(\d+)", header).group(1))
    assert enum("JG_OP_LENGTHATTN") == L.OP_LENGTHATTN == 15 == L.OP_LOCALATTN + 1
    assert enum("JG_PROF_CLASSES") == 8
    assert lib.jg_sizeof(0) == ctypes.sizeof(L.JgOp) and lib.jg_abi_version() == 1
    kernel_header = (ROOT / "jaeger_amd" / "csrc" / "jg_lengthattn.h").read_text()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", kernel_header).group(1))
    assert lib.jg_lengthattn_tile() == L.LENGTHATTN_TILE == define("JG_LENGTHATTN_TILE")
    assert lib.jg_lengthattn_chunk() == L.LENGTHATTN_CHUNK == define("JG_LENGTHATTN_CHUNK")
    assert define("JG_LENGTHATTN_STEP") == xr.STEP and L.LENGTHATTN_CHUNK % xr.STEP == 0 and L.LENGTHATTN_TILE % L.LENGTHATTN_CHUNK == 0
    from jaeger_amd import plan as P
    assert P.LENGTHATTN_CHANNELS == (16, 32, 64) and P.LENGTHATTN_MAX_FF == 256
