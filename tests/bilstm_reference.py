"""Reference side of the bilstm checks (tests/test_bilstm_reference.py on the CPU, tests/test_gpu_bilstm.py on the GPU).
Nothing here imports the product: the layer is restated from the reference's source and Keras 3's, the model forward
composes it with the functions of ``oracle/forward.py`` as they are.

**The layer** - ``MaskedBiLSTM`` (nnlib/v2/layers.py:1335-1430); read, not executed (no TensorFlow / Keras here).  Input
``(B, F, L, C)`` with an implicit mask ``m (B, F, L)`` or none: reshape to rows ``(B F, L, C)``;
``Bidirectional(LSTM(U, return_sequences=True, use_cudnn=False), merge_mode="concat")`` with ``mask = m`` unless
``ignore_mask``; reshape back to ``(B, F, L, 2U)``; ``compute_mask`` returns ``m``, or None with ``ignore_mask``.

Per direction, Keras 3 ``LSTMCell`` at its defaults: ``z = x_t @ kernel + h @ recurrent_kernel + bias``; the four U-wide
slices of z in order ``i = sigmoid, f = sigmoid, g = tanh, o = sigmoid``; ``c' = f c + i g``; ``h' = o tanh(c')``;
``h_0 = c_0 = 0``; the step's output is ``h'``.  Under a mask (``backend.rnn``, ``zero_output_for_mask=False``), at a step
whose position is invalid both states are carried unchanged and the output written is the previous step's output of that
direction - zeros while no valid step has come.  The backward direction walks ``t = L - 1 .. 0`` with the same rule and its
output sequence is flipped back before the concat.

The float64 restatement evaluates sigmoid and tanh in float64; what TensorFlow's float32 kernels add to that is not
measured anywhere (no TensorFlow) - DESIGN 3.9 says so.  tests/test_bilstm_reference.py holds the restatement against
``torch.nn.LSTM(bidirectional=True)`` in float64.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

import attention_reference as ar
import hyena_reference as hr
from attention_reference import f32
from oracle import forward as of

BILSTM = "masked_bilstm"
ROWS, STEPS = 16, 8            # csrc/jg_bilstm.h (the tests hold the library's exported constants against these)
DIRECTIONS = ("forward", "backward")
KINDS = hr.KINDS + ("many_runs",)      # hyena_reference.window_ids' six kinds, and rows with an invalid run every 24 positions

#: the mutations the issue lists
MUTATIONS = ("gates_ifog", "backward_not_flipped", "masked_step_zeroes_state", "masked_step_writes_zeros",
             "recurrent_kernel_transposed", "backward_from_row_end", "mask_ignored")
_MASKED = ("ragged", "few", "n_run", "starts_invalid", "empty_row", "many_runs")
#: the window kinds on which a mutation CAN show in the logits of a model whose readers behind the layer are masked (on the
#: others it changes nothing at all).  A zeroed state needs valid positions behind masked ones in the direction of the walk,
#: the row-end start trailing masked positions; a backward half that is not flipped back holds the same values in another
#: order along the row, which the fixture's per-channel norm and average pool cannot tell apart on rows without a masked
#: position.  ``masked_step_writes_zeros`` changes masked positions only: no masked reader sees it -
#: tests/test_bilstm_reference.py asserts that it changes no bit of the fixture's outputs and holds it on the
#: ``unmasked_tail`` sibling, whose last batch norm drops the mask (there it shows on every kind with masked positions)
VISIBLE_ON = {"gates_ifog": KINDS, "backward_not_flipped": _MASKED, "masked_step_zeroes_state": ("n_run", "many_runs"),
              "masked_step_writes_zeros": (), "recurrent_kernel_transposed": KINDS,
              "backward_from_row_end": ("ragged", "few", "empty_row"), "mask_ignored": _MASKED}


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


# ---- the restatement ----------------------------------------------------------------------------------------------------
def lstm_direction(x, kernel, recurrent, bias, mask=None, reverse: bool = False, mutation: str | None = None) -> np.ndarray:
    """float64 (R, L, U): one LSTM over the rows x (R, L, C), mask (R, L) bool or None; ``reverse``: the backward layer
    (``go_backwards`` and the flip back)."""
    x = np.asarray(x, np.float64)
    w, r, b = (np.asarray(a, np.float64) for a in (kernel, recurrent, bias))
    rows, l, _ = x.shape
    u = r.shape[0]
    if mutation == "recurrent_kernel_transposed":
        r = np.concatenate([r[:, g * u:(g + 1) * u].T for g in range(4)], axis=1)
    ok_all = np.ones((rows, l), bool) if (mask is None or mutation == "mask_ignored") else np.asarray(mask, bool).copy()
    if mutation == "backward_from_row_end" and reverse:
        # the walk starts at the row's last position: the masked positions behind the last valid one are steps like any other
        behind_last = ok_all[:, ::-1].cumsum(axis=1)[:, ::-1] == 0
        ok_all |= behind_last & ok_all.any(axis=1, keepdims=True)
    x = np.where(ok_all[..., None], x, 0.0)                    # (a masked position's values reach nothing)
    h, c, prev = np.zeros((rows, u)), np.zeros((rows, u)), np.zeros((rows, u))
    out = np.zeros((rows, l, u))
    for t in (range(l - 1, -1, -1) if reverse else range(l)):
        z = x[:, t] @ w + h @ r + b
        i_, f_ = sigmoid(z[:, :u]), sigmoid(z[:, u:2 * u])
        if mutation == "gates_ifog":
            o_, g_ = sigmoid(z[:, 2 * u:3 * u]), np.tanh(z[:, 3 * u:])
        else:
            g_, o_ = np.tanh(z[:, 2 * u:3 * u]), sigmoid(z[:, 3 * u:])
        cn = f_ * c + i_ * g_
        hn = o_ * np.tanh(cn)
        ok = ok_all[:, t, None]
        keep_c, keep_h = (0.0, 0.0) if mutation == "masked_step_zeroes_state" else (c, h)
        c, h = np.where(ok, cn, keep_c), np.where(ok, hn, keep_h)
        prev = np.where(ok, hn, 0.0 if mutation == "masked_step_writes_zeros" else prev)
        out[:, t] = prev
    if mutation == "backward_not_flipped" and reverse:
        out = out[:, ::-1]
    return out


def bilstm(x, w: dict, mask=None, ignore_mask: bool = False, mutation: str | None = None) -> np.ndarray:
    """float64 (R, L, 2U).  x (R, L, C) frame rows, mask (R, L) bool or None; w: the layer's variables by leaf name
    (``forward/kernel`` ...)."""
    m = None if ignore_mask else mask
    return np.concatenate([lstm_direction(x, w[f"{d}/kernel"], w[f"{d}/recurrent_kernel"], w[f"{d}/bias"], m, d == "backward", mutation)
                           for d in DIRECTIONS], axis=-1)


def carried_expectation(y, mask) -> np.ndarray:
    """What the layer holds at every position given its values ``y`` (R, L, 2U) at the valid ones: at a masked position the
    forward half of the nearest valid position before it and the backward half of the nearest valid one behind it, zeros
    where there is none.  Valid positions are returned as they are."""
    y = np.asarray(y)
    rows, l, c2 = y.shape
    u = c2 // 2
    out = y.copy()
    for r in range(rows):
        last = None
        for t in range(l):
            if mask[r, t]:
                last = t
            else:
                out[r, t, :u] = 0.0 if last is None else y[r, last, :u]
        last = None
        for t in range(l - 1, -1, -1):
            if mask[r, t]:
                last = t
            else:
                out[r, t, u:] = 0.0 if last is None else y[r, last, u:]
    return out


# ---- weights ------------------------------------------------------------------------------------------------------------
def params_of(a: dict) -> dict:
    """The constructor's defaults (:1354-1363) under the config of a YAML entry."""
    assert bool(a.get("return_sequences", True))
    return dict(units=int(a["units"]), ignore_mask=bool(a.get("ignore_mask", False)))


def mixer_layers(cfg: dict) -> list[tuple[int, str, dict]]:
    return [(i, str(layer.get("name", "")).lower(), dict(layer.get("config") or {}))
            for i, layer in enumerate(cfg["representation_learner"]["hidden_layers"])
            if str(layer.get("name", "")).lower() in (BILSTM, ar.ATTN)]


def layer_specs(c: int, units: int) -> dict[str, tuple]:
    return {f"{d}/{leaf}": shp for d in DIRECTIONS
            for leaf, shp in (("kernel", (c, 4 * units)), ("recurrent_kernel", (units, 4 * units)), ("bias", (4 * units,)))}


def weight_specs(cfg: dict) -> dict[str, tuple]:
    """``oracle.forward.weight_specs`` with the bilstm / attention layers' own variables, the channel count carried over a
    bilstm layer (it leaves 2 x units)."""
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
        if kind == BILSTM:
            for leaf, shp in layer_specs(cin, int(a["units"])).items():
                specs[f"rep/{cut}/{leaf}"] = shp
            cin = 2 * int(a["units"])
        elif kind == ar.ATTN:
            for leaf, shp in ar.layer_specs(int(a["embed_dim"]), int(a["num_heads"]), int(a.get("feed_forward_dim", 0)),
                                            bool(a.get("use_ffn", True))).items():
                specs[f"rep/{cut}/{leaf}"] = shp
        start = cut + 1
    of._block_specs("classifier", cfg["classifier"]["hidden_layers"], cin, specs)
    return specs


def random_weights(cfg: dict, seed: int = 38341) -> dict[str, np.ndarray]:
    """Seeded stand-in weights: ``oracle.forward.random_weights``' rules for the conv family and ``attention_reference``'s for
    an attention layer; for a bilstm glorot-like kernels over one gate's (C, U) block, recurrent kernels at orthogonal scale
    (entries of variance 1 / U) and biases ~ N(0, 0.1), the forget gate's plus one as Keras initialises it
    (``unit_forget_bias``: the state then remembers over tens of positions) - gains at which the recurrence neither dies nor saturates, so that
    the gates move (tests/test_bilstm_reference.py asserts it)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    specs = weight_specs(cfg)
    mixers = {f"rep/{i}": kind for i, kind, _ in mixer_layers(cfg)}
    out = {}
    for name, shp in sorted(specs.items()):
        leaf = name.rsplit("/", 1)[1]
        top = "/".join(name.split("/")[:2])
        if mixers.get(top) == ar.ATTN:
            continue
        if leaf == "recurrent_kernel":
            lim = math.sqrt(3.0 / shp[0])
            v = rng.uniform(-lim, lim, shp)
        elif leaf == "kernel" and mixers.get(top) == BILSTM:
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
            if mixers.get(top) == BILSTM:                      # Keras' unit_forget_bias: the forget gate's slice starts at one
                v[shp[0] // 4:shp[0] // 2] += 1.0
        out[name] = v.astype(f32)
    for top, kind in mixers.items():
        if kind == ar.ATTN:
            sub = {k[len(top) + 1:]: s for k, s in specs.items() if k.startswith(top + "/")}
            for leaf, v in ar.random_layer_weights(sub, rng).items():
                out[f"{top}/{leaf}"] = v
    return out


# ---- the model forward --------------------------------------------------------------------------------------------------
def forward(cfg: dict, weights: dict, ids: np.ndarray, dtype=torch.float64, layer_fn=None, mutation: str | None = None) -> dict[str, np.ndarray]:
    """``oracle.forward.forward`` for a model with bilstm layers, composed as ``hyena_reference.forward`` does it: the layers
    in front of one run through ``oracle.forward._run_block`` with the mask they have, the bilstm layer through
    :func:`bilstm` on the frame rows - ``layer_fn(rows, weights, mask, ignore_mask)`` in its place when given -, and the mask is
    KEPT behind it unless ``ignore_mask``; behind a ``cross_frame_attention`` no mask exists."""
    import local_attention_reference as lr
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
        xn = x.detach().numpy()
        if kind == ar.ATTN:
            y = ar.cross_frame_attention(xn, lw, int(a["num_heads"]), bool(a.get("use_ffn", True)))
            mask = None                                                  # the layer does not set supports_masking
        else:
            p = params_of(a)
            b_, fr, l, c = xn.shape
            mk = None if mask is None else mask.numpy().reshape(b_ * fr, l) != 0
            if layer_fn is not None:
                y = layer_fn(xn.reshape(b_ * fr, l, c), lw, mk, p["ignore_mask"])
            else:
                y = bilstm(xn.reshape(b_ * fr, l, c), lw, mk, p["ignore_mask"], mutation)
            y = np.asarray(y, np.float64).reshape(b_, fr, l, 2 * p["units"])
            if p["ignore_mask"]:
                mask = None
        x = torch.as_tensor(y).to(dtype)
        start = cut + 1
    out = {"embedding": x}
    logits, _ = of._run_block(x, None, cfg["classifier"]["hidden_layers"], "classifier", weights, cfg, dtype)
    out["prediction"] = logits
    if nmds:
        out["nmd"] = nmds[0] if len(nmds) == 1 else torch.cat(nmds, dim=-1)
    return {k: v.detach().numpy() for k, v in out.items()}


# ---- emulation of the kernel's arithmetic (csrc/jg_bilstm.hip), rounding where the kernel rounds ------------------------
def _sigmoid32(v):
    return (f32(1.0) / (f32(1.0) + np.exp2((f32(-1.4426950) * v).astype(f32)))).astype(f32)


def _tanh32(v):
    return (f32(2.0) * (f32(1.0) / (f32(1.0) + np.exp2((f32(-2.8853900) * v).astype(f32)))).astype(f32) - f32(1.0)).astype(f32)


def emulate(x, w: dict, mask=None, ignore_mask: bool = False) -> np.ndarray:
    """The kernel's arithmetic in numpy: f32 everywhere, one rounding where the kernel has one.  A step's gate sums are ONE
    k-ordered fma chain: from the bias over the C inputs (formed ahead of the recurrence, which changes no value), then
    over the U state values; sigmoid and tanh through exp2 and a reciprocal; ``c' = fma(f, c, round(i g))``; a masked step
    is dropped by a select.  x (R, L, C) -> (R, L, 2U)."""
    x = np.asarray(x, f32)
    rows, l, _ = x.shape
    ok_all = np.ones((rows, l), bool) if (mask is None or ignore_mask) else np.asarray(mask, bool)
    with np.errstate(over="ignore"):
        halves = []
        for d in DIRECTIONS:
            wk, rk, b = (np.asarray(w[f"{d}/{n}"], f32) for n in ("kernel", "recurrent_kernel", "bias"))
            u = rk.shape[0]
            xz = np.where(ok_all[..., None], x, f32(0.0))
            pre = ar._fma_chain(np.broadcast_to(b, (rows * l, 4 * u)).astype(f32), xz.reshape(rows * l, -1), wk).reshape(rows, l, 4 * u)
            h, c = np.zeros((rows, u), f32), np.zeros((rows, u), f32)
            out = np.zeros((rows, l, u), f32)
            for t in (range(l - 1, -1, -1) if d == "backward" else range(l)):
                z = ar._fma_chain(pre[:, t], h, rk)
                ig, fg, gg, og = _sigmoid32(z[:, :u]), _sigmoid32(z[:, u:2 * u]), _tanh32(z[:, 2 * u:3 * u]), _sigmoid32(z[:, 3 * u:])
                ig_gg = (ig * gg).astype(f32)
                cn = (fg.astype(np.float64) * c.astype(np.float64) + ig_gg.astype(np.float64)).astype(f32)
                hv = (og * _tanh32(cn)).astype(f32)
                ok = ok_all[:, t, None]
                c, h = np.where(ok, cn, c), np.where(ok, hv, h)
                out[:, t] = h
            halves.append(out)
    return np.concatenate(halves, axis=-1)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def with_bilstm_config(cfg: dict, **over) -> dict:
    out = copy.deepcopy(cfg)
    for layer in out["representation_learner"]["hidden_layers"]:
        if str(layer.get("name", "")).lower() == BILSTM:
            layer["config"].update(over)
    return out


# ---- the models of the two test tiers -----------------------------------------------------------------------------------
FSIZE = 500
#: by how many positions the convs in front of the layer shorten an invalid run: the 7-tap conv by 6, the four 3-tap convs
#: of the two residual blocks by 2 each
GROW = 14
VARIANTS = ("fixture", "u16", "u64", "first", "stacked", "ignore_mask", "behind_cross", "then_conv", "ln_tail", "nmd_front",
            "pool_max", "unmasked_tail")


def fixture_cfg() -> dict:
    from pathlib import Path

    import yaml
    return yaml.safe_load((Path(__file__).resolve().parent / "golden" / "bilstm500_project.yaml").read_text())["model"]


def variant(name: str) -> dict:
    """The fixture and its siblings.  ``unmasked_tail`` is the one model here in which something reads the layer's masked
    positions: its last batch norm drops the mask, and the average pool runs over every position."""
    cfg = fixture_cfg()
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    at = [i for i, l in enumerate(layers) if l["name"] == BILSTM][0]
    lstm = layers[at]["config"]

    def width(c, units):
        for layer in layers:
            if "filters" in layer["config"]:
                layer["config"]["filters"] = c
        lstm["units"] = units
        cfg["classifier"]["input_shape"] = 2 * units

    if name == "fixture":
        pass
    elif name == "u16":
        width(16, 16)
    elif name == "u64":
        width(64, 64)
    elif name == "first":                                 # directly behind the 64-wide embedding
        rep["hidden_layers"] = layers[at:]
    elif name == "stacked":                               # 32 -> units 64 -> 128 channels -> units 16 -> 32 channels
        lstm["units"] = 64
        layers.insert(at + 1, {"name": BILSTM, "config": dict(units=16)})
        cfg["classifier"]["input_shape"] = 32
    elif name == "ignore_mask":
        lstm["ignore_mask"] = True
    elif name == "behind_cross":                          # no mask arrives
        layers.insert(at, {"name": ar.ATTN, "config": dict(embed_dim=32, num_heads=4, feed_forward_dim=128)})
    elif name == "then_conv":                             # f32 rows -> the next conv's F16S in the split-f16 program
        layers += [{"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same")},
                   {"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]
        cfg["classifier"]["input_shape"] = 32
    elif name == "ln_tail":
        layers[-1] = {"name": "masked_layernorm", "config": {}}
        layers.append({"name": "activation", "config": {"activation": "gelu"}})
    elif name == "nmd_front":
        layers.insert(1, {"name": "nmd", "config": {}})
    elif name == "pool_max":
        rep["pooling"] = "max"
    elif name == "unmasked_tail":
        layers[-1] = {"name": "masked_batchnorm", "config": {"use_masking": False}}
    else:
        raise ValueError(name)
    return cfg


def ids_of(kind: str, name: str, n_win: int = 5) -> np.ndarray:
    """(n_win, 6, l) codon ids at FSIZE: ``hyena_reference.window_ids``' kinds, and ``many_runs`` - every row of every window
    holds an invalid run every 24 positions (three positions long where the layer sees it, at a row-dependent offset), so
    that a state which does not survive masked steps is lost six or seven times a row."""
    from oracle import encoder as oenc
    if kind == "many_runs":
        l = oenc.frame_length(FSIZE)
        grow = 0 if name == "first" else GROW
        ids = np.random.Generator(np.random.PCG64(23)).integers(1, 65, (n_win, 6, l))
        for w in range(n_win):
            for f in range(6):
                for a in range(5 + (2 * w + f) % 7, l - 3 - grow, 24):
                    ids[w, f, a:a + 3 + grow] = 0
        return ids.astype(np.uint8)
    return hr.window_ids(oenc.frame_length(FSIZE), kind, n_win=n_win, seed=17, grow=0 if name == "first" else GROW)
