"""Reference side of the row-mixer pair checks (tests/test_mixer_reference.py on the CPU, tests/test_gpu_mixer_pairs.py on the
GPU): ONE composed float64 forward for models that mix the seven row-mixer layers.  Nothing here restates a layer and
nothing here imports the product: every layer is the restatement its own reference module holds, and around them run
``oracle.forward._run_block`` and ``local_attention_reference._mask_behind`` exactly as the six modules' own ``forward``s run
them (tests/test_mixer_reference.py holds this forward bit for bit against each of the six).

What this module adds is the HAND-OVER between two mixers - which mask the next layer sees:

=========  ==========================================================================================
layer      mask behind it
=========  ==========================================================================================
cross      none (the layer does not set ``supports_masking``)
encoder    none (likewise)
local      kept; the layer's dead positions hold ``dead_fill`` (default ``lr.DEAD_FILL``)
axial      kept
hyena      kept
bilstm     kept, or none with ``ignore_mask``
msconv     the mask the layer returns (none if no branch masks or no mask arrives)
=========  ==========================================================================================

(:data:`MASK_BEHIND` is the same table for the tests.)  ``forward(..., handover=)`` breaks the hand-over between the first
mixer and the second on purpose: ``"stale"`` - the second mixer sees the mask the first one READ; ``"dropped"`` - it sees
none.  On the ``long_n`` windows the logits of the compiled pairs move by at least 5.7e-3 under ``stale`` (msconv -> bilstm)
and by at least 1.8e-2 under ``dropped`` (msconv -> bilstm); the project's gate is 1e-4 (measured by
tests/test_mixer_reference.py, which prints the table and asserts 8 x the gate).

The models: tests/golden/bilstm500_project.yaml (embedding 64 -> 7-tap conv 32 -> batch norm -> gelu -> two residual blocks
of 32 -> batch norm -> gelu -> masked_bilstm -> batch norm -> average pool -> dense 3) with the bilstm entry replaced by the
mixers.  The conv and the residual blocks in front shorten an invalid run by ``GROW`` positions, so every id generator is
called with that ``grow``: without it no invalid position reaches the mixers and every mask check is vacuous.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

import attention_reference as ar
import axial_attention_reference as xr
import bilstm_reference as br
import hyena_reference as hr
import local_attention_reference as lr
import multiscale_reference as mr
from attention_reference import f32
from oracle import forward as of

#: the seven layers, by the short names the tables use
KINDS = ("cross", "local", "encoder", "axial", "hyena", "bilstm", "msconv")
LAYER = {"cross": ar.ATTN, "local": lr.LOCAL, "encoder": xr.ENCODER, "axial": xr.AXIAL, "hyena": hr.HYENA, "bilstm": br.BILSTM,
         "msconv": mr.MSCONV}
SHORT = {v: k for k, v in LAYER.items()}
#: the mask behind each layer: "none", "kept" (the one it read) or "own" (the one it writes)
MASK_BEHIND = {"cross": "none", "encoder": "none", "local": "kept", "axial": "kept", "hyena": "kept", "bilstm": "kept", "msconv": "own"}
#: the ordered pairs the compiler refuses: these three layers read masked positions unmasked, and a local_attention leaves
#: zeros at its dead positions where the Keras graph holds values that depend on its version and precision
REFUSED = (("local", "cross"), ("local", "encoder"), ("local", "axial"))
HANDOVERS = ("stale", "dropped")

FSIZE = 500
GROW = br.GROW
WINDOW_KINDS = ("full", "long_n", "empty_row")
N_WIN = 3


# ---- the models ---------------------------------------------------------------------------------------------------------
def layer_entry(kind: str, cin: int, cout: int | None = None) -> dict:
    """The YAML entry of one mixer on ``cin`` channels: the attention layers with heads of 8 channels, a feed-forward half
    twice as wide, one block, a local window of 16; hyena of order 2; and the two width-changing kinds leaving ``cout``
    (default ``cin``) channels - a bilstm of ``cout / 2`` units, a multi-scale conv [cout / 2 k3 | cout / 2 k5 d2], concat."""
    cout = cin if cout is None else cout
    att = dict(embed_dim=cin, num_heads=cin // 8, feed_forward_dim=2 * cin)
    if kind in ("cross", "encoder"):
        config = att
    elif kind == "local":
        config = dict(att, window_size=16, num_blocks=1)
    elif kind == "axial":
        config = dict(att, num_blocks=1)
    elif kind == "hyena":
        config = dict(dim=cin, order=2)
    elif kind == "bilstm":
        config = dict(units=cout // 2)
    elif kind == "msconv":
        config = dict(branches=[dict(filters=cout // 2, kernel_size=3), dict(filters=cout // 2, kernel_size=5, dilation_rate=2)],
                      merge="concat")
    else:
        raise ValueError(kind)
    assert kind in ("bilstm", "msconv") or cout == cin, (kind, cin, cout)
    return {"name": LAYER[kind], "config": config}


def model_cfg(entries: list[dict], width: int, front: int = 32, tail: list[dict] | None = None) -> dict:
    """The bilstm fixture with its ``masked_bilstm`` entry replaced by ``entries``, convs of ``front`` channels in front, the
    layers behind them ``tail`` (default: the fixture's batch norm) and ``classifier.input_shape`` the final ``width``."""
    cfg = br.fixture_cfg()
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    at = [i for i, layer in enumerate(layers) if layer["name"] == br.BILSTM][0]
    for layer in layers[:at]:
        if "filters" in layer["config"]:
            layer["config"]["filters"] = front
    rep["hidden_layers"] = layers[:at] + copy.deepcopy(entries) + (layers[at + 1:] if tail is None else copy.deepcopy(tail))
    cfg["classifier"]["input_shape"] = width
    return cfg


def pair_cfg(a: str, b: str, width: int = 32) -> dict:
    """Layer ``a`` directly in front of layer ``b``, both at ``width`` channels."""
    return model_cfg([layer_entry(a, width), layer_entry(b, width)], width, front=width)


#: the wide hand-overs: a width-changing first layer 32 -> 64 in front of each of the six other kinds at 64 channels, and a
#: bilstm 32 -> 128 in front of a multi-scale conv 128 -> 32 (one slot then holds 128-wide and 32-wide rows in one forward)
WIDE = tuple((a, b) for a in ("bilstm", "msconv") for b in KINDS if b != a) + (("bilstm128", "msconv"),)


def wide_cfg(a: str, b: str) -> dict:
    if a == "bilstm128":
        assert b == "msconv"
        return model_cfg([layer_entry("bilstm", 32, 128), layer_entry("msconv", 128, 32)], 32)
    return model_cfg([layer_entry(a, 32, 64), layer_entry(b, 64)], 64)


CHAINS = {"masked_first": ("msconv", "local", "bilstm", "hyena", "axial", "encoder", "cross"),
          "unmasked_last": ("cross", "encoder", "axial", "hyena", "bilstm", "msconv", "local")}


def chain_cfg(name: str) -> dict:
    """``masked_first``: every layer that can take a mask takes one, batch norm -> gelu behind the last; ``unmasked_last``: no
    mask arrives behind the first layer, a layer norm behind the last."""
    tail = {"masked_first": [{"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}],
            "unmasked_last": [{"name": "masked_layernorm", "config": {}}]}[name]
    return model_cfg([layer_entry(k, 32) for k in CHAINS[name]], 32, tail=tail)


def ids_of(kind: str, n_win: int = N_WIN) -> np.ndarray:
    """(n_win, 6, 165) codon ids at FSIZE, every generator with ``grow=GROW``: ``full`` - no invalid id; ``long_n`` - in every
    other row an invalid run that stays longer than the local window behind the convs (dead positions with valid ones on
    both sides); ``empty_row`` - ragged windows, two rows without a valid id."""
    from oracle import encoder as oenc
    l = oenc.frame_length(FSIZE)
    if kind == "long_n":
        return lr.window_ids(l, "long_n", n_win=n_win, seed=17, half=8, grow=GROW)
    assert kind in ("full", "empty_row"), kind
    return hr.window_ids(l, kind, n_win=n_win, seed=17, grow=GROW)


# ---- weights ------------------------------------------------------------------------------------------------------------
def mixer_layers(cfg: dict) -> list[tuple[int, str, dict]]:
    return [(i, str(layer.get("name", "")).lower(), dict(layer.get("config") or {}))
            for i, layer in enumerate(cfg["representation_learner"]["hidden_layers"])
            if str(layer.get("name", "")).lower() in SHORT]


def _layer_specs(kind: str, a: dict, cin: int) -> tuple[dict[str, tuple], int]:
    """(the layer's variables by leaf name, the channels it leaves): each from the layer's own reference module."""
    if kind == ar.ATTN:
        return ar.layer_specs(int(a["embed_dim"]), int(a["num_heads"]), int(a.get("feed_forward_dim", 0)), bool(a.get("use_ffn", True))), cin
    if kind == lr.LOCAL:
        return lr._specs_of(kind, a), cin
    if kind in (xr.ENCODER, xr.AXIAL):
        return xr._specs_of(kind, a), cin
    if kind == hr.HYENA:
        return hr._specs_of(kind, a), cin
    if kind == br.BILSTM:
        return br.layer_specs(cin, int(a["units"])), 2 * int(a["units"])
    p = mr.params_of(a)
    return mr.layer_specs(cin, p), mr.out_channels(p)


def weight_specs(cfg: dict) -> dict[str, tuple]:
    """``oracle.forward.weight_specs`` with every mixer's own variables, the channel count carried over the two
    width-changing kinds."""
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
        if kind:
            own, cin = _layer_specs(kind, a, cin)
            for leaf, shp in own.items():
                specs[f"rep/{cut}/{leaf}"] = shp
        start = cut + 1
    of._block_specs("classifier", cfg["classifier"]["hidden_layers"], cin, specs)
    return specs


_OWN_WEIGHTS = {ar.ATTN: ar.random_layer_weights, lr.LOCAL: lr.random_layer_weights, xr.ENCODER: xr.random_layer_weights,
                xr.AXIAL: xr.random_layer_weights, hr.HYENA: hr.random_layer_weights}


def random_weights(cfg: dict, seed: int = 38341) -> dict[str, np.ndarray]:
    """Seeded stand-in weights for any mix.  The conv family, the bilstm and the multi-scale branches by the rules of
    ``bilstm_reference.random_weights`` (He-uniform kernels, a bilstm's glorot-like over one gate's block, its recurrent kernels
    at orthogonal scale, its forget-gate bias plus one); the attention layers and hyena by their own module's
    ``random_layer_weights`` (hyena's with its ``FILTER_GAIN``)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    specs = weight_specs(cfg)
    mixers = {f"rep/{i}": kind for i, kind, _ in mixer_layers(cfg)}
    out = {}
    for name, shp in sorted(specs.items()):
        leaf = name.rsplit("/", 1)[1]
        kind = mixers.get("/".join(name.split("/")[:2]))
        if kind in _OWN_WEIGHTS:
            continue
        if leaf == "recurrent_kernel":
            lim = math.sqrt(3.0 / shp[0])
            v = rng.uniform(-lim, lim, shp)
        elif leaf == "kernel" and kind == br.BILSTM:
            lim = math.sqrt(6.0 / (shp[0] + shp[1] // 4))
            v = rng.uniform(-lim, lim, shp)
        elif leaf == "kernel":
            lim = math.sqrt(6.0 / int(np.prod(shp[:-1])))
            v = rng.uniform(-lim, lim, shp)
        elif leaf == "embeddings":
            v = rng.normal(0.0, 1.0 / math.sqrt(shp[1]) * 4.0, shp)
        elif leaf in ("gamma", "moving_variance"):
            v = rng.uniform(0.5, 1.5, shp)
        else:
            v = rng.normal(0.0, 0.1, shp)
            if kind == br.BILSTM:                              # Keras' unit_forget_bias
                v[shp[0] // 4:shp[0] // 2] += 1.0
        out[name] = v.astype(f32)
    for top, kind in mixers.items():
        if kind in _OWN_WEIGHTS:
            sub = {k[len(top) + 1:]: s for k, s in specs.items() if k.startswith(top + "/")}
            for leaf, v in _OWN_WEIGHTS[kind](sub, rng).items():
                out[f"{top}/{leaf}"] = v
    return out


# ---- the model forward --------------------------------------------------------------------------------------------------
def forward(cfg: dict, weights: dict, ids: np.ndarray, dtype=torch.float64, dead_fill: float = lr.DEAD_FILL,
            handover: str | None = None, info: list | None = None) -> dict[str, np.ndarray]:
    """``oracle.forward.forward`` for a model with any of the seven mixers, composed as the six modules' own ``forward``s: the
    layers in front of a mixer run through ``oracle.forward._run_block`` with the mask they have, the mixer through its own
    module's restatement, and the mask behind it follows the table in the module's docstring.  ``handover``: one of
    HANDOVERS, applied between the first mixer and the second.  ``info``: a list that receives one dict per mixer - its
    short name, the masks it read and left (bool arrays or None) and, for a local layer, its dead positions."""
    assert handover is None or handover in HANDOVERS, handover
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
    n_mixers = 0
    for cut, kind, a in mixer_layers(cfg) + [(len(layers), "", {})]:
        last = cut == len(layers)
        seg = [pad] * start + list(layers[start:cut])
        x, n_ = of._run_block(x, mask, seg, "rep", weights, cfg, dtype, pooling=rep.get("pooling") if last else None)
        nmds += n_
        if last:
            break
        mask = lr._mask_behind(mask, seg, cfg, dtype)
        mask_in = mask
        lw = ar.sub_weights(weights, f"rep/{cut}")
        xn = x.detach().numpy()
        b_, fr, l, c = xn.shape
        mk = None if mask is None else mask.numpy() != 0
        rows = lambda t: None if t is None else t.reshape((b_ * fr, l) + t.shape[3:])
        dead = None
        if kind == ar.ATTN:
            y = ar.cross_frame_attention(xn, lw, int(a["num_heads"]), bool(a.get("use_ffn", True)))
            mask = None
        elif kind == lr.LOCAL:
            y, dead = lr.local_attention(xn, lw, int(a["num_heads"]), int(a["window_size"]), int(a.get("num_blocks", 1)),
                                         None if mask is None else mask.numpy())
            y[dead] = dead_fill
        elif kind == xr.ENCODER:
            y = xr.transformer_encoder(rows(xn), lw, int(a["num_heads"]), rows(mk)).reshape(b_, fr, l, c)
            mask = None
        elif kind == xr.AXIAL:
            y = xr.axial_attention(xn, lw, int(a["num_heads"]), int(a.get("num_blocks", 1)), xr.norm_type_of(a),
                                   float(a.get("epsilon", 1e-6)), mk)
        elif kind == hr.HYENA:
            y = hr.hyena_block(rows(xn), lw, rows(mk), **hr.params_of(a)).reshape(b_, fr, l, c)
        elif kind == br.BILSTM:
            p = br.params_of(a)
            y = np.asarray(br.bilstm(rows(xn), lw, rows(mk), p["ignore_mask"]), np.float64).reshape(b_, fr, l, 2 * p["units"])
            if p["ignore_mask"]:
                mask = None
        else:
            y, mask = mr.multi_scale_conv(x, mask, lw, mr.params_of(a), None, dtype)
        if info is not None:
            info.append(dict(kind=SHORT[kind], mask_in=mk, mask_out=None if mask is None else mask.numpy() != 0, dead=dead))
        if n_mixers == 0 and handover == "stale":
            mask = mask_in
        elif n_mixers == 0 and handover == "dropped":
            mask = None
        x = torch.as_tensor(y).to(dtype)
        start = cut + 1
        n_mixers += 1
    out = {"embedding": x}
    logits, _ = of._run_block(x, None, cfg["classifier"]["hidden_layers"], "classifier", weights, cfg, dtype)
    out["prediction"] = logits
    if nmds:
        out["nmd"] = nmds[0] if len(nmds) == 1 else torch.cat(nmds, dim=-1)
    return {k: v.detach().numpy() for k, v in out.items()}


# ---- who wrote what an op reads: by slot numbers alone ------------------------------------------------------------------
def producer(prog, i: int, slot: int | None = None) -> int:
    """The last op in front of op ``i`` that writes the activation slot it reads (``slot``: another slot op ``i`` reads, such
    as the one an add stage names), whatever its kind."""
    slot = prog.ops[i].in_buf if slot is None else slot
    assert slot >= 0, f"op {i}: reads no activation slot ({slot})"
    for j in range(i - 1, -1, -1):
        if prog.ops[j].out_buf == slot:
            return j
    raise AssertionError(f"op {i}: no producer of slot {slot}")


def mask_writer(prog, i: int):
    """The last op in front of op ``i`` that writes the mask slot it reads (None: it reads none).  A mask the embedding op
    wrote cannot be tapped: an assertion error."""
    from jaeger_amd import _lib as L
    slot = prog.ops[i].in_mask
    if slot == L.JG_BUF_NONE:
        return None
    assert slot >= 0, f"op {i}: reads the id tensor as its mask"
    for j in range(i - 1, -1, -1):
        o = prog.ops[j]
        # (the three kinds that WRITE a mask slot; every other op that names one in out_mask reads it)
        if o.out_mask == slot and o.kind in (L.OP_MASK, L.OP_MSMASK, L.OP_EMBED):
            assert o.kind != L.OP_EMBED, f"op {i}: mask slot {slot} comes from the embedding op"
            return j
    raise AssertionError(f"op {i}: no writer of mask slot {slot}")


def layer_ops(cfg: dict, prog) -> list[tuple[str, str, dict, list[int]]]:
    """[(short name, weight prefix, the YAML config, the indices of the layer's ops)] per mixer layer, in program order.  The
    op kinds a layer compiles to are stated HERE, not read off the compiler: cross - one frame-attention op; local - one
    local-attention op per block; encoder - one length-attention op; axial - per block a length-attention, a frame-attention
    and an element-wise op; hyena, bilstm - one op; msconv - a mask op (only where the layer masks) and the conv op."""
    from jaeger_amd import _lib as L
    mixer_kinds = (L.OP_FRAMEATTN, L.OP_LOCALATTN, L.OP_LENGTHATTN, L.OP_HYENA, L.OP_BILSTM, L.OP_MSCONV, L.OP_MSMASK)
    at = next(i for i, op in enumerate(prog.ops) if op.kind in mixer_kinds)
    out = []
    for idx, kind, a in mixer_layers(cfg):
        short = SHORT[kind]
        want = {"cross": [L.OP_FRAMEATTN], "local": [L.OP_LOCALATTN] * int(a.get("num_blocks", 1)), "encoder": [L.OP_LENGTHATTN],
                "axial": [L.OP_LENGTHATTN, L.OP_FRAMEATTN, L.OP_ELTWISE] * int(a.get("num_blocks", 1)), "hyena": [L.OP_HYENA],
                "bilstm": [L.OP_BILSTM], "msconv": [L.OP_MSCONV]}[short]
        while prog.ops[at].kind not in mixer_kinds:            # the layers between two mixers: none of them is a mixer op
            at += 1
        if short == "msconv" and prog.ops[at].kind == L.OP_MSMASK:
            want = [L.OP_MSMASK] + want
        got = [prog.ops[at + j].kind for j in range(len(want))]
        assert got == want, (short, idx, got, want)
        out.append((short, f"rep/{idx}", a, list(range(at, at + len(want)))))
        at += len(want)
    assert not any(op.kind in mixer_kinds for op in prog.ops[at:]), "mixer ops behind the last mixer layer"
    return out
