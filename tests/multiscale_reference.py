"""Reference side of the multi-scale conv checks (tests/test_multiscale_reference.py on the CPU, tests/test_gpu_multiscale.py
on the GPU).  Nothing here imports the product: the layer is restated from the reference's source, the model forward
composes it with the functions of ``oracle/forward.py`` as they are.

**The layer** - ``MultiScaleConv1D`` (nnlib/v2/layers.py:1433-1595); read, not executed (no TensorFlow / Keras here).  Input
``(B, F, L, C)`` with an implicit mask ``m (B, F, L)`` or none.  ``build`` makes one ``MaskedConv1D`` (:1137-1330) per entry
of ``branches``, with ``padding`` defaulting to "same", ``strides`` to 1 and ``use_bias`` to the layer's (:1502-1528); a
branch's ``use_masking`` defaults to MaskedConv1D's own True.  ``call`` runs every branch on the same input and mask,
concatenates the outputs along the channels (``merge="concat"``) or adds them (``tf.add_n``, ``merge="add"``), and the mask it
leaves is the AND of the branches' output masks - None where the first branch leaves none (:1531-1550).

The float64 restatement uses ``oracle.forward.masked_conv1d`` per branch as it is; tests/test_multiscale_reference.py holds
it against ``torch.nn.functional.conv1d`` with explicit TF-SAME padding.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch
import torch.nn.functional as F

import attention_reference as ar
import hyena_reference as hr
import local_attention_reference as lr
from attention_reference import f32
from oracle import forward as of

MSCONV = "multi_scale_conv"
TILE = 64                      # csrc/jg_msconv.h (the tests hold the library's exported constant against this)
KINDS = hr.KINDS + ("many_runs", "islands")

#: the mutations the issue lists
MUTATIONS = ("pad_left_ceil", "dilation_ignored", "input_not_masked", "mask_or_not_and", "mask_of_first_branch", "majority_floor",
             "branches_swapped", "act_after_add", "bias_after_act")
MASK_MUTATIONS = ("mask_or_not_and", "mask_of_first_branch", "majority_floor")
#: the model each mutation is shown on: one whose branches it can change at all
MODEL_OF = {"pad_left_ceil": "even_k", "dilation_ignored": "fixture", "input_not_masked": "fixture", "mask_or_not_and": "fixture",
            "mask_of_first_branch": "fixture", "majority_floor": "modes", "branches_swapped": "fixture", "act_after_add": "add",
            "bias_after_act": "add"}
_MASKED = ("ragged", "few", "n_run", "starts_invalid", "empty_row", "many_runs", "islands")
#: the window kinds on which a mutation shows in the logits of its model.  The arithmetic mutations show everywhere; an input
#: that is not multiplied by the mask needs masked positions next to valid ones.  The three mask mutations change which
#: positions the layers BEHIND the op count as valid.  OR for AND: wherever an invalid run ends, the 5-tap branch reaches one
#: position further than the 3-tap one.  The first branch's mask for the AND (fixture: 3 taps at dilation 1, the narrowest but
#: for the dilated branch): a position whose neighbour is valid while t - 3, t and t + 3 are not - islands alone.  The
#: majority threshold (modes: 5 taps, 3 against 2 valid ones, under a strict 2-tap branch that needs t and t + 1): the first
#: position of a two-position island between runs of two or more - islands alone
VISIBLE_ON = {"pad_left_ceil": KINDS, "dilation_ignored": KINDS, "input_not_masked": _MASKED, "mask_or_not_and": _MASKED,
              "mask_of_first_branch": ("islands",), "majority_floor": ("islands",), "branches_swapped": KINDS,
              "act_after_add": KINDS, "bias_after_act": KINDS}


# ---- the restatement ----------------------------------------------------------------------------------------------------
def branch_params(a: dict) -> list[dict]:
    """The branches of a YAML entry under the defaults of MultiScaleConv1D.build (:1502-1515) and MaskedConv1D (:1148-1165)."""
    out = []
    for b in a["branches"]:
        assert str(b.get("padding", "same")).lower() == "same" and b.get("strides", 1) == 1
        out.append(dict(filters=int(b["filters"]), kernel_size=int(b["kernel_size"]), dilation_rate=int(b.get("dilation_rate", 1)),
                        activation=b.get("activation"), use_bias=bool(b.get("use_bias", a.get("use_bias", True))),
                        use_masking=bool(b.get("use_masking", True)), mask_mode=b.get("mask_mode", "any")))
    return out


def params_of(a: dict) -> dict:
    return dict(merge=a.get("merge", "concat"), branches=branch_params(a))


def out_channels(p: dict) -> int:
    return sum(b["filters"] for b in p["branches"]) if p["merge"] == "concat" else p["branches"][0]["filters"]


def _mutated_branch(x, mask, w, p, mutation):
    """One MaskedConv1D with ``mutation`` built in: the formulas of ``oracle.forward.masked_conv1d``, written out."""
    k, d = p["kernel_size"], p["dilation_rate"]
    if mutation == "dilation_ignored":
        d = 1
    total = (k - 1) * d
    pl = total - total // 2 if mutation == "pad_left_ceil" else total // 2
    w_, fr, l, c = x.shape
    um = p["use_masking"] and mask is not None
    om = None
    if um:
        cnt = of.conv1d_nwc(F.pad(mask.reshape(-1, l, 1), (0, 0, pl, total - pl)), torch.ones((k, 1, 1), dtype=mask.dtype), 1, "VALID", d)
        if p["mask_mode"] == "any":
            om = cnt > 0
        elif p["mask_mode"] == "majority":
            om = cnt >= (k // 2 if mutation == "majority_floor" else (k + 1) // 2)
        else:
            om = cnt == float(k)
        om = om.squeeze(-1).reshape(w_, fr, l).to(x.dtype)
        if mutation != "input_not_masked":
            x = x * mask.unsqueeze(-1)
    y = of.conv1d_nwc(F.pad(x.reshape(-1, l, c), (0, 0, pl, total - pl)), w["kernel"], 1, "VALID", d)
    if mutation == "bias_after_act":
        y = of.activation(p["activation"], y)
    if p["use_bias"]:
        y = y + w["bias"]
    if mutation != "bias_after_act":
        y = of.activation(p["activation"], y)
    return y.reshape(w_, fr, l, -1), om


def multi_scale_conv(x, mask, lw: dict, p: dict, mutation: str | None = None, dtype=torch.float64):
    """(y (B, F, L, cout), mask (B, F, L) or None).  x (B, F, L, C) and mask (B, F, L) 0 / 1 or None, torch tensors of
    ``dtype``; lw: the layer's variables by leaf name (``branch<b>/kernel`` ...)."""
    outs, masks = [], []
    for b, bp in enumerate(p["branches"]):
        w = {k: torch.as_tensor(v).to(dtype) for k, v in ar.sub_weights(lw, f"branch{b}").items()}
        if mutation in ("pad_left_ceil", "dilation_ignored", "input_not_masked", "majority_floor", "bias_after_act"):
            y, om = _mutated_branch(x, mask, w, bp, mutation)
        else:
            y, om = of.masked_conv1d(x, mask, w, kernel_size=bp["kernel_size"], strides=1, padding="same", dilation_rate=bp["dilation_rate"],
                                     use_bias=bp["use_bias"], act=None if mutation == "act_after_add" else bp["activation"],
                                     use_masking=bp["use_masking"], mask_mode=bp["mask_mode"])
        outs.append(y)
        masks.append(om)
    if mutation == "branches_swapped" and len(outs) > 1:
        outs[0], outs[1] = outs[1], outs[0]
    if p["merge"] == "concat":
        y = torch.cat(outs, dim=-1)
    else:
        y = outs[0]
        for o in outs[1:]:
            y = y + o
        if mutation == "act_after_add":
            y = of.activation(p["branches"][0]["activation"], y)
    out_mask = None
    if masks[0] is not None:
        out_mask = masks[0]
        if mutation != "mask_of_first_branch":
            for m in masks[1:]:
                out_mask = torch.maximum(out_mask, m) if mutation == "mask_or_not_and" else out_mask * m
    return y, out_mask


def rows_op(x, mask, lw: dict, p: dict, mutation: str | None = None):
    """The layer on frame rows: x (R, L, C), mask (R, L) bool or None -> (float64 (R, L, cout), mask (R, L) bool or None)."""
    xt = torch.as_tensor(np.asarray(x, np.float64))[None]
    mt = None if mask is None else torch.as_tensor(np.asarray(mask, np.float64))[None]
    y, om = multi_scale_conv(xt, mt, lw, p, mutation)
    return y[0].numpy(), None if om is None else om[0].numpy() != 0


# ---- weights ------------------------------------------------------------------------------------------------------------
def mixer_layers(cfg: dict) -> list[tuple[int, str, dict]]:
    return [(i, str(layer.get("name", "")).lower(), dict(layer.get("config") or {}))
            for i, layer in enumerate(cfg["representation_learner"]["hidden_layers"])
            if str(layer.get("name", "")).lower() in (MSCONV, ar.ATTN, lr.LOCAL)]


def layer_specs(c: int, p: dict) -> dict[str, tuple]:
    out = {}
    for b, bp in enumerate(p["branches"]):
        out[f"branch{b}/kernel"] = (bp["kernel_size"], c, bp["filters"])
        if bp["use_bias"]:
            out[f"branch{b}/bias"] = (bp["filters"],)
    return out


def weight_specs(cfg: dict) -> dict[str, tuple]:
    """``oracle.forward.weight_specs`` with the multi-scale / attention layers' own variables, the channel count carried over a
    multi-scale layer."""
    specs: dict[str, tuple] = {}
    emb = cfg["embedding"]
    assert emb.get("use_embedding_layer", False)
    cin = int(emb["embedding_size"])
    specs["embedding/embeddings"] = (of.vocab_size(cfg), cin)
    layers = cfg["representation_learner"]["hidden_layers"]
    pad = {"name": "dropout", "config": {}}
    start = 0
    for cut, kind, a in mixer_layers(cfg) + [(len(layers), "", {})]:
        cin = of._block_specs("rep", [pad] * start + list(layers[start:cut]), cin, specs, [])
        if kind == MSCONV:
            p = params_of(a)
            for leaf, shp in layer_specs(cin, p).items():
                specs[f"rep/{cut}/{leaf}"] = shp
            cin = out_channels(p)
        elif kind in (ar.ATTN, lr.LOCAL):
            for leaf, shp in lr._specs_of(kind, a).items():
                specs[f"rep/{cut}/{leaf}"] = shp
        start = cut + 1
    of._block_specs("classifier", cfg["classifier"]["hidden_layers"], cin, specs)
    return specs


def random_weights(cfg: dict, seed: int = 38341) -> dict[str, np.ndarray]:
    """Seeded stand-in weights: ``oracle.forward.random_weights``' rules (He-uniform kernels over kernel_size x cin, biases
    ~ N(0, 0.1)) for the conv family and the branches, ``attention_reference``'s for an attention layer."""
    rng = np.random.Generator(np.random.PCG64(seed))
    specs = weight_specs(cfg)
    mixers = {f"rep/{i}": kind for i, kind, _ in mixer_layers(cfg)}
    out = {}
    for name, shp in sorted(specs.items()):
        leaf = name.rsplit("/", 1)[1]
        top = "/".join(name.split("/")[:2])
        if mixers.get(top) in (ar.ATTN, lr.LOCAL):
            continue
        if leaf == "kernel":
            lim = math.sqrt(6.0 / int(np.prod(shp[:-1])))
            v = rng.uniform(-lim, lim, shp)
        elif leaf == "embeddings":
            v = rng.normal(0.0, 1.0 / math.sqrt(shp[1]) * 4.0, shp)
        elif leaf in ("gamma", "moving_variance"):
            v = rng.uniform(0.5, 1.5, shp)
        else:
            v = rng.normal(0.0, 0.1, shp)
        out[name] = v.astype(f32)
    for top, kind in mixers.items():
        if kind in (ar.ATTN, lr.LOCAL):
            sub = {k[len(top) + 1:]: s for k, s in specs.items() if k.startswith(top + "/")}
            for leaf, v in ar.random_layer_weights(sub, rng).items():
                out[f"{top}/{leaf}"] = v
    return out


# ---- the model forward --------------------------------------------------------------------------------------------------
def forward(cfg: dict, weights: dict, ids: np.ndarray, dtype=torch.float64, layer_fn=None, mutation: str | None = None,
            dead_fill: float = lr.DEAD_FILL) -> dict[str, np.ndarray]:
    """``oracle.forward.forward`` for a model with multi-scale conv layers, composed as ``bilstm_reference.forward`` does it: the
    layers in front of one run through ``oracle.forward._run_block`` with the mask they have, the layer through
    :func:`multi_scale_conv` - ``layer_fn(x, mask, weights, params)`` in its place when given -, and the mask behind it is
    the one it returns.  Behind a ``cross_frame_attention`` no mask exists; a ``local_attention`` keeps the mask and its dead
    positions hold ``dead_fill``."""
    idt = torch.as_tensor(np.asarray(ids).astype(np.int64))
    emb_cfg = cfg["embedding"]
    assert emb_cfg.get("use_embedding_layer", False) and not emb_cfg.get("use_positional_embeddings", False)
    x = torch.as_tensor(weights["embedding/embeddings"]).to(dtype)[idt]
    mask = (idt != 0).to(dtype)
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    pad = {"name": "dropout", "config": {}}
    nmds = []
    start = 0
    for cut, kind, a in mixer_layers(cfg) + [(len(layers), "", {})]:
        last = cut == len(layers)
        seg = [pad] * start + list(layers[start:cut])
        x, n_ = of._run_block(x, mask, seg, "rep", weights, cfg, dtype, pooling=rep.get("pooling") if last else None)
        nmds += n_
        if last:
            break
        mask = lr._mask_behind(mask, seg, cfg, dtype)
        lw = ar.sub_weights(weights, f"rep/{cut}")
        if kind == ar.ATTN:
            y = ar.cross_frame_attention(x.detach().numpy(), lw, int(a["num_heads"]), bool(a.get("use_ffn", True)))
            x, mask = torch.as_tensor(y).to(dtype), None                 # the layer does not set supports_masking
        elif kind == lr.LOCAL:
            y, dead = lr.local_attention(x.detach().numpy(), lw, int(a["num_heads"]), int(a["window_size"]), int(a.get("num_blocks", 1)),
                                         None if mask is None else mask.numpy())
            y[dead] = dead_fill
            x = torch.as_tensor(y).to(dtype)
        else:
            p = params_of(a)
            x, mask = layer_fn(x, mask, lw, p) if layer_fn is not None else multi_scale_conv(x, mask, lw, p, mutation, dtype)
        start = cut + 1
    out = {"embedding": x}
    logits, _ = of._run_block(x, None, cfg["classifier"]["hidden_layers"], "classifier", weights, cfg, dtype)
    out["prediction"] = logits
    if nmds:
        out["nmd"] = nmds[0] if len(nmds) == 1 else torch.cat(nmds, dim=-1)
    return {k: v.detach().numpy() for k, v in out.items()}


# ---- emulation of the kernel's arithmetic (csrc/jg_msconv.hip), rounding where the kernel rounds ------------------------
def _act32(name, v):
    """jg_apply_act in float32."""
    name = None if name is None or str(name).lower() == "linear" else str(name).lower()
    if name is None:
        return v
    if name == "gelu":
        return ar._gelu32(v)
    if name == "relu":
        return np.maximum(v, f32(0.0))
    if name == "tanh":
        return np.tanh(v).astype(f32)
    if name == "sigmoid":
        with np.errstate(over="ignore"):
            return (f32(1.0) / (f32(1.0) + np.exp2((f32(-1.4426950) * v).astype(f32)))).astype(f32)
    raise ValueError(name)


def emulate(x, lw: dict, p: dict, mask=None) -> np.ndarray:
    """The kernel's arithmetic in numpy, f32 everywhere: a masked or out-of-row position is a zero row; per branch an
    accumulator starts from the bias (0 without one) and takes ONE k-ordered fma chain, tap-major and channel-minor; then
    the branch's activation; with add the sum in branch order.  x (R, L, C), mask (R, L) bool or None -> (R, L, cout)."""
    x = np.asarray(x, f32)
    rows, l, c = x.shape
    outs = []
    for b, bp in enumerate(p["branches"]):
        k, d, fl = bp["kernel_size"], bp["dilation_rate"], bp["filters"]
        xz = x if (mask is None or not bp["use_masking"]) else np.where(np.asarray(mask, bool)[..., None], x, f32(0.0))
        total = (k - 1) * d
        xp = np.pad(xz, ((0, 0), (total // 2, total - total // 2), (0, 0)))
        kern = np.asarray(lw[f"branch{b}/kernel"], f32)
        bias = np.asarray(lw[f"branch{b}/bias"], f32) if bp["use_bias"] else np.zeros(fl, f32)
        acc = np.broadcast_to(bias, (rows * l, fl)).astype(f32)
        for j in range(k):
            acc = ar._fma_chain(acc, xp[:, j * d:j * d + l].reshape(rows * l, c), kern[j])
        outs.append(_act32(bp["activation"], acc).reshape(rows, l, fl))
    if p["merge"] == "concat":
        return np.concatenate(outs, axis=-1)
    y = outs[0]
    for o in outs[1:]:
        y = (y + o).astype(f32)
    return y


# ---- the models of the two test tiers -----------------------------------------------------------------------------------
FSIZE = 500
VARIANTS = ("fixture", "reference_small", "add", "even_k", "modes", "wide", "one_branch", "behind_conv", "then_conv", "ln_tail",
            "behind_cross", "unmasked")


def fixture_cfg() -> dict:
    from pathlib import Path

    import yaml
    return yaml.safe_load((Path(__file__).resolve().parent / "golden" / "multiscale500_project.yaml").read_text())["model"]


def _conv(filters, k, **kw):
    return [{"name": "masked_conv1d", "config": dict(filters=filters, kernel_size=k, padding="same", **kw)},
            {"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]


def variant(name: str) -> dict:
    """The fixture - embedding 64 -> multi_scale_conv [16 k3 d1 | 16 k5 d1 | 32 k3 d3, concat] -> batch norm -> gelu ->
    local_attention 64 -> layer norm -> masked average -> dense 3 - and its siblings."""
    cfg = fixture_cfg()
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    ms = layers[0]["config"]
    local = layers[3]["config"]

    def local_width(c, heads, ff, window, blocks):
        local.update(embed_dim=c, num_heads=heads, feed_forward_dim=ff, window_size=window, num_blocks=blocks)
        cfg["classifier"]["input_shape"] = c

    if name == "fixture":
        pass
    elif name == "reference_small":                       # the reference's integration test: 8 k3 | 8 k5 -> local_attention 16
        ms["branches"] = [dict(filters=8, kernel_size=3, dilation_rate=1), dict(filters=8, kernel_size=5, dilation_rate=1)]
        local_width(16, 2, 32, 16, 1)
    elif name == "add":                                   # three 32-filter branches summed, other activations, one without bias
        ms["merge"] = "add"
        ms["branches"] = [dict(filters=32, kernel_size=3, activation="gelu"), dict(filters=32, kernel_size=5, activation="tanh", use_bias=False),
                          dict(filters=32, kernel_size=3, dilation_rate=2, activation="relu")]
        local_width(32, 4, 64, 32, 1)
    elif name == "even_k":
        ms["branches"] = [dict(filters=32, kernel_size=4, dilation_rate=1), dict(filters=32, kernel_size=2, dilation_rate=5)]
    elif name == "modes":
        ms["branches"] = [dict(filters=16, kernel_size=3, mask_mode="any"), dict(filters=16, kernel_size=5, mask_mode="majority"),
                          dict(filters=32, kernel_size=2, mask_mode="strict")]
    elif name == "wide":                                  # behind a 128-filter conv, four branches, 128 out
        rep["hidden_layers"] = _conv(128, 3) + layers[:3] + [{"name": "masked_conv1d", "config": dict(filters=64, kernel_size=1, padding="same")}] + layers[3:]
        ms["branches"] = [dict(filters=32, kernel_size=15), dict(filters=32, kernel_size=5, dilation_rate=16),
                          dict(filters=48, kernel_size=3, dilation_rate=2, activation="relu"), dict(filters=16, kernel_size=1)]
    elif name == "one_branch":
        ms["branches"] = [dict(filters=64, kernel_size=7, dilation_rate=2)]
    elif name == "behind_conv":                           # at 32 channels
        rep["hidden_layers"] = _conv(32, 5) + layers
    elif name == "then_conv":                             # f32 rows -> the next conv's F16S in the split-f16 program
        rep["hidden_layers"] = layers[:3] + _conv(64, 3) + layers[3:]
    elif name == "ln_tail":
        layers[1] = {"name": "masked_layernorm", "config": {}}
    elif name == "behind_cross":                          # no mask arrives
        rep["hidden_layers"] = _conv(64, 3) + [{"name": ar.ATTN, "config": dict(embed_dim=64, num_heads=4, feed_forward_dim=128)}] + layers[:3]
        rep["pooling"] = "average"
    elif name == "unmasked":                              # all branches use_masking: false, behind a conv: no mask leaves the layer
        rep["hidden_layers"] = _conv(64, 3) + layers[:3]
        for b in ms["branches"]:
            b["use_masking"] = False
        rep["pooling"] = "average"
    else:
        raise ValueError(name)
    return cfg


def ids_of(kind: str, n_win: int = 5) -> np.ndarray:
    """(n_win, 6, l) codon ids at FSIZE (l = 165: tiles of 64 + 64 + 37): ``hyena_reference.window_ids``' six kinds;
    ``many_runs``: an invalid run of three positions every 24, at a row-dependent offset; ``islands``: over the first two
    thirds of every row valid islands of one and two positions between invalid runs of two to six - where a branch that
    reaches one position sees no valid one and a branch that reaches three does, so that the AND of the branches' masks
    differs from every single branch's."""
    from oracle import encoder as oenc
    l = oenc.frame_length(FSIZE)
    if kind not in ("many_runs", "islands"):
        return hr.window_ids(l, kind, n_win=n_win, seed=17)
    ids = np.random.Generator(np.random.PCG64(23)).integers(1, 65, (n_win, 6, l))
    for w in range(n_win):
        for f in range(6):
            if kind == "many_runs":
                for a in range(5 + (2 * w + f) % 7, l - 3, 24):
                    ids[w, f, a:a + 3] = 0
            else:
                t, q = (w + 2 * f) % 5, w + f
                while t < 2 * l // 3:
                    run = 2 + q % 5
                    ids[w, f, t:t + run] = 0
                    t += run + 1 + q % 2
                    q += 1
    return ids.astype(np.uint8)


def with_branches(cfg: dict, branches: list, **over) -> dict:
    out = copy.deepcopy(cfg)
    for layer in out["representation_learner"]["hidden_layers"]:
        if str(layer.get("name", "")).lower() == MSCONV:
            layer["config"]["branches"] = copy.deepcopy(branches)
            layer["config"].update(over)
    return out
