"""Reference side of the hyena checks (tests/test_hyena_reference.py on the CPU, tests/test_gpu_hyena.py on the GPU).
Nothing here imports the product: the layer is restated from the reference's source, the model forward composes it with
the functions of ``oracle/forward.py`` as they are.

**The layer** - ``HyenaBlock`` (nnlib/v2/layers.py:3023-3153), ``HyenaOperator`` (:2937-3002), ``HyenaFilter`` (:2766-2915),
``causal_fft_convolve`` (:2724-2763); read, not executed (no TensorFlow here):

* block, input ``(B, 6, L, C)`` with mask ``m (B, 6, L)``: ``x = x * m``; ``r = x``; ``x = LayerNormalization(eps 1e-6)(x) * m``;
  reshape to rows ``(B * 6, L, C)``; ``y = HyenaOperator(x)``; with ``output_projection`` ``y = Dense(C)(y)`` (with a bias);
  ``out = (y + r) * m``.  Without a mask every ``* m`` is absent.  ``supports_masking``: the mask stays behind the layer.
* operator: ``p_k = x @ W_k`` (no bias), ``k = 0 .. order``; ``z = p_0``; ``z = p_(i+1) * causal_conv(z, h_i)`` for
  ``i < order``.
* ``causal_conv(z, h)[t, c] = sum over s <= t of h[t - s, c] z[s, c]`` - the reference takes the float32 FFT route at
  length ``2 L - 1``; the restatement is the direct float64 sum (tests/test_hyena_reference.py holds the two together).
* filter, for ``t < L``: ``h_i[t] = (exp(-|alpha_i| t) + bias_i) * FFN_i(PE[t])``; ``PE`` the interleaved sin / cos rows at
  ``pe_dim = 16`` whose arguments ``pos * div`` are float32 products; ``FFN_i`` = ``filter_layers`` Dense layers, the hidden
  ones ``filter_hidden`` wide with ``filter_activation`` ("sin" = tf.sin, else Keras' activation of that name: "gelu" is
  the tanh form, see tests/attention_reference.py), the last ``C`` wide and linear; with ``filter_normalize`` every channel
  divided by its L2 norm over the ``L`` positions of the call (divide_no_nan); with ``seq_len`` the ``PE`` rows are a stored
  weight of that many rows.

The float64 restatement evaluates ``PE``'s sine and cosine, the FFN, the window and the norm in float64; what TensorFlow's
float32 ``exp`` / ``sin`` / Dense layers add to that is not measured anywhere (no TensorFlow) - DESIGN 3.8 says so.
"""
from __future__ import annotations

import copy
import math
import re

import numpy as np
import torch

import attention_reference as ar
from attention_reference import f32, gelu_tanh, layer_norm
from oracle import forward as of

LN_EPS = 1e-6
HYENA = "hyena_block"
PE_DIM = 16
TABLE_ROWS = 8192          # rows of the filter table a program carries for a layer without seq_len
FILTER_GAIN = 2.0 ** -4    # of the stand-in weights: random_layer_weights
TILE = CHUNK = 64          # csrc/jg_hyena.h (the tests hold the library's exported constants against these)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def positional_rows(n: int) -> np.ndarray:
    """(n, 16) float64: [sin(a_0), cos(a_0), sin(a_1), ...] with a_j = pos * div_j formed in float32 (:2871-2880)."""
    pos = np.arange(n).astype(f32)[:, None]
    div = np.exp(np.arange(0, PE_DIM, 2).astype(f32) * f32(-(np.log(f32(10000.0)) / f32(PE_DIM)))).astype(f32)
    a = (pos * div).astype(f32).astype(np.float64)
    out = np.empty((n, PE_DIM))
    out[:, 0::2], out[:, 1::2] = np.sin(a), np.cos(a)
    return out


def activation(name, x):
    name = None if name is None else str(name).lower()
    if name in (None, "linear"):
        return x
    if name == "sin":
        return np.sin(x)
    if name == "gelu":
        return gelu_tanh(x)
    if name == "relu":
        return np.maximum(x, 0.0)
    if name == "tanh":
        return np.tanh(x)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if name in ("silu", "swish"):
        return x / (1.0 + np.exp(-x))
    raise ValueError(name)


def params_of(a: dict) -> dict:
    """The constructor's defaults (:3047-3059) under the config of a YAML entry."""
    return dict(order=int(a.get("order", 2)), filter_hidden=int(a.get("filter_hidden", 32)), filter_layers=int(a.get("filter_layers", 2)),
                filter_activation=a.get("filter_activation", "gelu"), filter_normalize=bool(a.get("filter_normalize", False)),
                output_projection=bool(a.get("output_projection", False)), seq_len=a.get("seq_len"))


def hyena_filter(w: dict, l: int, *, order=2, filter_layers=2, filter_activation="gelu", filter_normalize=False, seq_len=None,
                 mutation: str | None = None, norm_rows: int | None = None, **_) -> np.ndarray:
    """float64 (order, l, C): HyenaFilter.call(l).  w: the layer's variables by leaf name (``hyena/filter/...``).
    ``norm_rows``: what the mutation ``norm_over_table_rows`` takes the norm over."""
    g = lambda name: np.asarray(w[f"hyena/filter/{name}"], np.float64)
    if seq_len is not None:
        assert l <= seq_len, "the reference slices a stored encoding of seq_len rows: a longer call fails there"
        pe_all = g("pos_encoding") if "hyena/filter/pos_encoding" in w else positional_rows(int(seq_len))
    rows = l if not (filter_normalize and mutation == "norm_over_table_rows") else int(norm_rows)
    pe = pe_all[:rows] if seq_len is not None else positional_rows(rows)
    t = np.arange(rows, dtype=np.float64)[:, None]
    alphas = g("alphas") if mutation == "alpha_signed" else np.abs(g("alphas"))
    out = []
    for i in range(order):
        x = pe
        for j in range(filter_layers):
            x = x @ g(f"ffn_{i}/dense_{j}/kernel") + g(f"ffn_{i}/dense_{j}/bias")
            if j < filter_layers - 1:
                x = activation(filter_activation, x)
        window = np.exp(-alphas[i][None, :] * t)
        if mutation != "window_bias_dropped":
            window = window + g("biases")[i][None, :]
        h = window * x
        if filter_normalize:
            norm = np.sqrt((h * h).sum(axis=0, keepdims=True))
            h = np.where(norm > 0, h / np.where(norm > 0, norm, 1.0), 0.0)
        out.append(h[:l])
    return np.stack(out)


def causal_conv(z, h, mutation: str | None = None) -> np.ndarray:
    """float64 direct sum.  z (R, L, C), h (L, C) -> y[r, t, c] = sum over s <= t of h[t - s, c] z[r, s, c]."""
    z, h = np.asarray(z, np.float64), np.asarray(h, np.float64)
    r_, l, c = z.shape
    y = np.zeros_like(z)
    if mutation == "filter_by_absolute_position":
        return np.cumsum(h[None] * z, axis=1)
    if mutation == "conv_runs_on_from_previous_row":
        # the rows as one sequence, as they lie in memory: h here holds 2 L lags, row r sees row r - 1 at lags t + L - s
        assert h.shape[0] == 2 * l
        prev = np.concatenate([np.zeros((1, l, c)), z[:-1]])
        both = np.concatenate([prev, z], axis=1)
        return causal_conv(both, h)[:, l:]
    for lag in range(l):
        if mutation == "lag_off_by_one":                                   # h[t - s + 1] where h[t - s] belongs
            if lag + 1 < l:
                y[:, lag:] += h[lag + 1][None, None] * z[:, :l - lag]
            continue
        y[:, lag:] += h[lag][None, None] * z[:, :l - lag]
        if mutation == "non_causal_sum" and lag > 0:                       # ... and the later positions, by |t - s|
            y[:, :l - lag] += h[lag][None, None] * z[:, lag:]
    return y


def causal_conv_fft(z, h) -> np.ndarray:
    """The reference's route (:2751-2762) in float64: rfft / irfft at length 2 L - 1, truncated to L."""
    zt = torch.as_tensor(np.asarray(z, np.float64)).permute(0, 2, 1)      # (R, C, L)
    ht = torch.as_tensor(np.asarray(h, np.float64)).T                    # (C, L)
    l = zt.shape[-1]
    n = 2 * l - 1
    y = torch.fft.irfft(torch.fft.rfft(zt, n=n) * torch.fft.rfft(ht, n=n)[None], n=n)[..., :l]
    return y.permute(0, 2, 1).numpy()


def hyena_block(x, w: dict, mask=None, mutation: str | None = None, table_rows: int = TABLE_ROWS, **params) -> np.ndarray:
    """float64.  x (R, L, C) frame rows, mask (R, L) bool or None; w: the layer's variables by leaf name; params: params_of.
    ``mutation``: one of MUTATIONS."""
    p = {**params_of({}), **params}
    x = np.asarray(x, np.float64)
    g = lambda name: np.asarray(w[name], np.float64)
    r_, l, c = x.shape
    order = p["order"]
    m = None if mask is None else np.asarray(mask, bool)[..., None].astype(np.float64)
    xm = x * m if (m is not None and mutation != "entry_mask_dropped") else x
    residual = x if mutation in ("residual_unmasked", "residual_behind_exit_mask") else xm
    n = layer_norm(xm, g("norm/gamma"), g("norm/beta"))
    if m is not None and mutation != "mask_behind_norm_dropped":
        n = n * m
    proj = [n @ g(f"hyena/proj_{k}/kernel") for k in range(order + 1)]
    long_rows = mutation == "conv_runs_on_from_previous_row"
    hp = {**p, "filter_normalize": p["filter_normalize"] and not long_rows}
    hs = hyena_filter(w, 2 * l if long_rows else l, mutation=mutation, norm_rows=p["seq_len"] or table_rows, **{**hp, "seq_len": None if long_rows else p["seq_len"]})
    if long_rows and p["filter_normalize"]:                                # (the scale of the call at l positions)
        hl = hyena_filter(w, l, **{**p, "filter_normalize": False})
        norm = np.sqrt((hl * hl).sum(axis=1, keepdims=True))
        hs = np.where(norm > 0, hs / np.where(norm > 0, norm, 1.0), 0.0)
    z = proj[0]
    steps = order - 1 if mutation == "order_loop_one_short" else order
    for i in range(steps):
        gate = proj[order - i] if mutation == "gates_wrong_order" else proj[i + 1]
        z = gate * causal_conv(z, hs[i], mutation)
    if p["output_projection"]:
        z = z @ g("out_proj/kernel")
        if mutation != "out_proj_bias_dropped":
            z = z + g("out_proj/bias")
    if mutation == "residual_behind_exit_mask" and m is not None:          # y m + r, r the layer's own input
        return z * m + residual
    out = z + residual
    if m is not None and mutation != "exit_mask_dropped":
        out = out * m
    return out


#: the mutations the issue lists (the first thirteen), and two more that stand for the two of them that are algebraically
#: invisible: with the exit multiply in place, ``entry_mask_dropped`` and ``residual_unmasked`` change NOTHING (at a masked
#: position the output is 0 either way, at a valid one x m = x) - tests/test_hyena_reference.py asserts exactly that, bit for
#: bit - so the bugs they point at are caught in the forms that do show: the residual added behind the exit multiply, and the
#: exit multiply itself dropped.
MUTATIONS = ("non_causal_sum", "lag_off_by_one", "filter_by_absolute_position", "gates_wrong_order", "mask_behind_norm_dropped",
             "entry_mask_dropped", "residual_unmasked", "window_bias_dropped", "alpha_signed", "norm_over_table_rows",
             "out_proj_bias_dropped", "conv_runs_on_from_previous_row", "order_loop_one_short",
             "residual_behind_exit_mask", "exit_mask_dropped")
INVISIBLE = ("entry_mask_dropped", "residual_unmasked")

KINDS = ("full", "ragged", "few", "n_run", "starts_invalid", "empty_row")

#: the window kinds on which a mutation must show (8 x outside the bound).  ``mask_behind_norm_dropped`` needs masked
#: positions IN FRONT of valid ones (beta leaks forward only: the convolution is causal); the exit-mask mutations need
#: masked positions; the previous-row mutation needs valid codons at the end of a row's predecessor.
_MASKED_FIRST = ("n_run", "starts_invalid")
_MASKED = ("ragged", "few", "n_run", "starts_invalid", "empty_row")
VISIBLE_ON = {
    "non_causal_sum": KINDS, "lag_off_by_one": KINDS, "filter_by_absolute_position": KINDS, "gates_wrong_order": KINDS,
    "mask_behind_norm_dropped": _MASKED_FIRST, "entry_mask_dropped": (), "residual_unmasked": (),
    "window_bias_dropped": KINDS, "alpha_signed": KINDS, "norm_over_table_rows": KINDS, "out_proj_bias_dropped": KINDS,
    "conv_runs_on_from_previous_row": ("full", "n_run", "starts_invalid"), "order_loop_one_short": KINDS,
    "residual_behind_exit_mask": _MASKED, "exit_mask_dropped": _MASKED,
}


# ---- weights ------------------------------------------------------------------------------------------------------------
def hyena_layers(cfg: dict) -> list[tuple[int, str, dict]]:
    return [(i, str(layer.get("name", "")).lower(), dict(layer.get("config") or {}))
            for i, layer in enumerate(cfg["representation_learner"]["hidden_layers"])
            if str(layer.get("name", "")).lower() in (HYENA, ar.ATTN)]


def without_hyena(cfg: dict) -> dict:
    """The same model with every hyena / attention layer replaced by a dropout layer (see tests/attention_reference.py)."""
    out = copy.deepcopy(cfg)
    for i, _, _ in hyena_layers(cfg):
        out["representation_learner"]["hidden_layers"][i] = {"name": "dropout", "config": {"rate": 0.0}}
    return out


def layer_specs(c: int, *, order=2, filter_hidden=32, filter_layers=2, output_projection=False, **_) -> dict[str, tuple]:
    s = {"norm/gamma": (c,), "norm/beta": (c,), "hyena/filter/alphas": (order, c), "hyena/filter/biases": (order, c)}
    for k in range(order + 1):
        s[f"hyena/proj_{k}/kernel"] = (c, c)
    for o in range(order):
        cin = PE_DIM
        for j in range(filter_layers):
            units = c if j == filter_layers - 1 else filter_hidden
            s[f"hyena/filter/ffn_{o}/dense_{j}/kernel"] = (cin, units)
            s[f"hyena/filter/ffn_{o}/dense_{j}/bias"] = (units,)
            cin = units
    if output_projection:
        s.update({"out_proj/kernel": (c, c), "out_proj/bias": (c,)})
    return s


def _specs_of(kind: str, a: dict) -> dict[str, tuple]:
    if kind == HYENA:
        return layer_specs(int(a["dim"]), **params_of(a))
    return ar.layer_specs(int(a["embed_dim"]), int(a["num_heads"]), int(a.get("feed_forward_dim", 0)), bool(a.get("use_ffn", True)))


def weight_specs(cfg: dict) -> dict[str, tuple]:
    specs = dict(of.weight_specs(without_hyena(cfg)))
    for i, kind, a in hyena_layers(cfg):
        for leaf, shp in _specs_of(kind, a).items():
            specs[f"rep/{i}/{leaf}"] = shp
    return specs


def random_layer_weights(specs: dict[str, tuple], rng) -> dict[str, np.ndarray]:
    """``attention_reference.random_layer_weights``, and for the window: decay rates log-uniform in [1e-3, 1] as the
    reference initialises them (:2847-2849), a quarter of them NEGATIVE (the layer takes their absolute value), and
    biases ~ N(0, 0.1).

    The last Dense of every filter FFN (kernel and bias) is scaled by ``FILTER_GAIN``.  The positional rows change slowly
    with t, so a Glorot-scaled FFN gives filters of order one whose ``l`` lags add up coherently: every convolution
    multiplies the values by up to ``l`` (two of them: logits of 160 to 3500 at l = 166, where float32 resolves 1e-5 to
    2e-4 - this composition evaluated in float32 instead of float64 then misses the project's absolute gate of 1e-4 by
    itself, whatever runs it).  ``FILTER_GAIN`` = 2^-4, the power of two next to 1 / sqrt(166), keeps what the operator
    adds beside the residual at the residual's size, and the model outputs at the size the gate was made for."""
    out = ar.random_layer_weights(specs, rng)
    last = {}
    for name, shp in sorted(specs.items()):
        if name.endswith("/alphas"):
            out[name] = (10.0 ** rng.uniform(-3.0, 0.0, shp) * rng.choice([1.0, 1.0, 1.0, -1.0], shp)).astype(f32)
        m = re.match(r"(.*hyena/filter/ffn_\d+)/dense_(\d+)/", name)
        if m:
            last[m.group(1)] = max(last.get(m.group(1), 0), int(m.group(2)))
    for ffn, j in last.items():
        for leaf in ("kernel", "bias"):
            out[f"{ffn}/dense_{j}/{leaf}"] = (out[f"{ffn}/dense_{j}/{leaf}"] * f32(FILTER_GAIN)).astype(f32)
    return out


def random_weights(cfg: dict, seed: int = 38341) -> dict[str, np.ndarray]:
    w = dict(of.random_weights(without_hyena(cfg), seed))
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for i, kind, a in hyena_layers(cfg):
        gen = random_layer_weights if kind == HYENA else ar.random_layer_weights
        for leaf, v in gen(_specs_of(kind, a), rng).items():
            w[f"rep/{i}/{leaf}"] = v
    return w


# ---- the model forward --------------------------------------------------------------------------------------------------
def forward(cfg: dict, weights: dict, ids: np.ndarray, dtype=torch.float64) -> dict[str, np.ndarray]:
    """``oracle.forward.forward`` for a model with hyena layers, composed as ``local_attention_reference.forward`` does it:
    the layers in front of one run through ``oracle.forward._run_block`` with the mask they have, the hyena layer through
    :func:`hyena_block` on the frame rows, and the mask is KEPT behind it (supports_masking); behind a
    ``cross_frame_attention`` no mask exists."""
    import local_attention_reference as lr
    idt = torch.as_tensor(np.asarray(ids).astype(np.int64))
    emb_cfg = cfg["embedding"]
    assert emb_cfg.get("use_embedding_layer", False) and not emb_cfg.get("use_positional_embeddings", False)
    table = torch.as_tensor(weights["embedding/embeddings"]).to(dtype)
    x = table[idt]
    mask = (idt != 0).to(dtype)
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    pad = {"name": "dropout", "config": {}}
    nmds = []
    start = 0
    for cut, kind, a in hyena_layers(cfg) + [(len(layers), "", {})]:
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
            b_, fr, l, c = xn.shape
            mk = None if mask is None else mask.numpy().reshape(b_ * fr, l) != 0
            y = hyena_block(xn.reshape(b_ * fr, l, c), lw, mk, **params_of(a)).reshape(b_, fr, l, c)
        x = torch.as_tensor(y).to(dtype)
        start = cut + 1
    out = {"embedding": x}
    logits, _ = of._run_block(x, None, cfg["classifier"]["hidden_layers"], "classifier", weights, cfg, dtype)
    out["prediction"] = logits
    if nmds:
        out["nmd"] = nmds[0] if len(nmds) == 1 else torch.cat(nmds, dim=-1)
    return {k: v.detach().numpy() for k, v in out.items()}


# ---- inputs -------------------------------------------------------------------------------------------------------------
def window_ids(l: int, kind: str, n_win: int = 5, seed: int = 11, grow: int = 0) -> np.ndarray:
    """(n_win, 6, l) codon ids.  ``full`` / ``ragged`` / ``few`` (nearly empty): tests/attention_reference.py.  ``n_run``: a
    run of invalid codons in the middle of every row of the odd (window + frame) sums; ``starts_invalid``: those rows START
    with invalid codons; ``empty_row``: ragged windows in which two rows hold no valid codon at all.  ``grow``: by how many
    positions the convs in front of the layer shorten an invalid run - the runs are made that much longer."""
    if kind in ("full", "ragged", "few"):
        return ar.window_ids(l, kind, n_win, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 7))
    if kind == "empty_row":
        ids = ar.window_ids(l, "ragged", n_win, seed).copy()
        ids[0, 2] = 0
        ids[n_win - 1, 5] = 0
        return ids
    assert kind in ("n_run", "starts_invalid"), kind
    ids = rng.integers(1, 65, (n_win, 6, l))
    run = min(9 + grow, max(l - 2, 0))
    for w in range(n_win):
        for f in range(6):
            if (w + f) % 2 and run > 0:
                a = 0 if kind == "starts_invalid" else int(rng.integers(1, max(l - run, 2)))
                ids[w, f, a:a + run] = 0
    return ids.astype(np.uint8)


def value_inputs(c: int, rows: int, l: int, seed: int = 5):
    """``local_attention_reference.value_inputs``: unit normal; GELU-like; offset rows; exact zeros at half the positions."""
    import local_attention_reference as lr
    return lr.value_inputs(c, rows, l, seed)


def row_masks(rows: int, l: int, kind: str, seed: int = 3) -> np.ndarray | None:
    """(rows, l) bool validity of the op-level tests, in the shapes of KINDS (None for ``full``)."""
    if kind == "full":
        return None
    rng = np.random.Generator(np.random.PCG64(seed))
    m = np.ones((rows, l), bool)
    for r in range(rows):
        if kind == "ragged":
            m[r, int(rng.integers(l // 3, l + 1)):] = False
        elif kind == "few":
            m[r, int(rng.integers(min(3, l), min(12, l) + 1)):] = False
        elif kind == "n_run" and r % 2:
            a = int(rng.integers(1, max(l - 9, 2)))
            m[r, a:a + 9] = False
        elif kind == "starts_invalid" and r % 2:
            m[r, :min(9, l - 1)] = False
        elif kind == "empty_row":
            m[r, int(rng.integers(l // 3, l + 1)):] = False
            if r in (1, rows - 1):
                m[r] = False
    return m


# ---- emulation of the kernels' arithmetic (csrc/jg_hyena.hip), rounding where the kernels round ----------------------------
def fold(w: dict, *, order=2, output_projection=False, **_) -> dict[str, np.ndarray]:
    """The host-side fold, restated: gamma into the projections, ``beta @ W_k`` as their bias; float64, rounded once."""
    g = lambda name: np.asarray(w[name], np.float64)
    out = {"wp": np.stack([g("norm/gamma")[:, None] * g(f"hyena/proj_{k}/kernel") for k in range(order + 1)]).astype(f32),
           "bp": np.stack([g("norm/beta") @ g(f"hyena/proj_{k}/kernel") for k in range(order + 1)]).astype(f32)}
    if output_projection:
        out["wo"], out["bo"] = g("out_proj/kernel").astype(f32), g("out_proj/bias").astype(f32)
    return out


def filter_tables(w: dict, rows: int, **params) -> tuple[np.ndarray, np.ndarray]:
    """(h f32 (order, rows, C), ssq f32): the un-normalised filter rounded to float32, and the running sum of ITS squares
    (summed in float64, rounded once) - what the blob of an op carries."""
    p = {**params_of({}), **params}
    h = hyena_filter(w, rows, **{**p, "filter_normalize": False}).astype(f32)
    return h, np.cumsum(h.astype(np.float64) ** 2, axis=1).astype(f32)


def _conv32(z, h, chunk: int = CHUNK) -> np.ndarray:
    """The convolution kernel's sum: per chunk of ``chunk`` earlier positions an f32 fma chain from zero over ascending s
    (lags below zero multiply by a zero filter row), the chunk's sum added to the running sum."""
    r_, l, c = z.shape
    acc = np.zeros((r_, l, c), f32)
    t = np.arange(l)
    hz = np.concatenate([h[:l].astype(np.float64), np.zeros((1, c))])     # row l: the zero row of a negative lag
    for s0 in range(0, l, chunk):
        part = np.zeros((r_, l, c), np.float64)
        for s in range(s0, min(s0 + chunk, l)):
            lag = t - s
            hv = hz[np.where(lag >= 0, lag, l)]                           # (l, c)
            part = (part + hv[None] * z[:, s, None, :].astype(np.float64)).astype(f32).astype(np.float64)
        acc = (acc + part.astype(f32)).astype(f32)
    return acc


def emulate_block(x, w: dict, mask=None, table_rows: int = TABLE_ROWS, **params) -> np.ndarray:
    """The three kernels' arithmetic in numpy: f32 everywhere, one rounding where a kernel has one.  x (R, L, C)."""
    p = {**params_of({}), **params}
    x = np.asarray(x, f32)
    r_, l, c = x.shape
    order = p["order"]
    ok = np.ones((r_, l), bool) if mask is None else np.asarray(mask, bool)
    fw = fold(w, **p)
    h, ssq = filter_tables(w, l, **p)                                     # (rows beyond l are never read at this length)
    xm = np.where(ok[..., None], x, f32(0.0)).reshape(-1, c)
    n_tok = xm.shape[0]
    xn = ar._ln32(xm, LN_EPS)
    proj = []
    for k in range(order + 1):
        pk = ar._fma_chain(np.broadcast_to(fw["bp"][k], (n_tok, c)).astype(f32), xn, fw["wp"][k]).reshape(r_, l, c)
        proj.append(np.where(ok[..., None], pk, f32(0.0)))
    z = proj[0]
    for i in range(order):
        acc = _conv32(z, h[i])
        if p["filter_normalize"]:
            s2 = ssq[i, l - 1]
            with np.errstate(divide="ignore"):
                inv = np.where(s2 > 0, f32(1.0) / np.sqrt(s2, dtype=f32), f32(0.0)).astype(f32)
            acc = (acc * inv[None, None]).astype(f32)
        z = (proj[i + 1] * acc).astype(f32)
    y = z.reshape(-1, c)
    if p["output_projection"]:
        y = ar._fma_chain(np.broadcast_to(fw["bo"], (n_tok, c)).astype(f32), y, fw["wo"])
    out = (y.reshape(r_, l, c) + x).astype(f32)
    return np.where(ok[..., None], out, f32(0.0))
