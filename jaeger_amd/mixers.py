"""The row-mixer layer kinds: one class per kind that answers every question the Python compiler asks about it.

A row mixer runs on the rows of the (frames, length, channels) tensor of the representation learner as an op of its own -
the Python side of ``jg_mixer_kinds`` (csrc/jg_host.h).  Each class below is the plan node of its kind (a dataclass in
``ModelPlan.rep``) and carries ``yaml_name`` and ``accepts`` (the entry of a project YAML the reference's constructor would
take), ``parse`` (config, incoming channels and frames -> the layer, with the kind's refusals and its ``*_limit``),
``channels`` (what the layer leaves), ``weight_shapes`` (its Keras variables under their canonical names), ``pack`` (those
variables as the kernel reads them) and ``emit`` (its ops: the refusals against unmasked readers, what it does to the dead
positions a ``local_attention`` leaves, the mask behind it - around ``_Compiler._emit_mixer``, ``program.py``).

``MIXERS`` maps the YAML names to the classes; ``plan._block``, ``plan.weight_shapes``, ``_Compiler._walk`` and
``weights.py`` dispatch on it or on :class:`Mixer`.  ``Conv``, ``Norm`` and ``UnsupportedLayer`` live here because the
mixers are built from them; ``plan.py`` hands them on.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib as L

_ACT_CODE = {None: L.ACT_NONE, "linear": L.ACT_NONE, "gelu": L.ACT_GELU_TANH, "gelu_erf": L.ACT_GELU_ERF,
             "relu": L.ACT_RELU, "tanh": L.ACT_TANH, "sigmoid": L.ACT_SIGMOID}
_MASK_MODE = {"any": L.MASK_ANY, "majority": L.MASK_MAJORITY, "strict": L.MASK_STRICT}


class UnsupportedLayer(ValueError):
    """A layer / option of the project YAML that the MI355X engine does not implement."""


def act_code(name) -> int:
    key = name.lower() if isinstance(name, str) else name
    if key not in _ACT_CODE:
        raise UnsupportedLayer(f"activation {name!r} is not supported by the MI355X engine")
    return _ACT_CODE[key]


@dataclass
class Conv:
    name: str                      # weight prefix
    kernel_size: int
    cin: int
    filters: int
    strides: int = 1               # layers.py:1154
    padding: str = "valid"         # layers.py:1156 (MaskedConv1D default!)
    dilation_rate: int = 1         # layers.py:1157
    use_bias: bool = True          # layers.py:1159
    activation: str | None = None  # layers.py:1158
    use_masking: bool = True       # layers.py:1163
    mask_mode: str = "any"         # layers.py:1164


@dataclass
class Norm:
    name: str
    kind: str                      # masked_batchnorm | masked_dyt | masked_layernorm
    channels: int
    epsilon: float = 1e-5          # MaskedBatchNorm layers.py:804; LN 1e-3 layers.py:306
    use_masking: bool = True


class Mixer:
    """What the walks ask of every row-mixer kind; the refusals that read the same for every kind are written here."""
    yaml_name = ""
    tap_lookahead = False          # plan._block refuses an nmd tap directly behind the layer (its store carries no partial sums)
    on_embedding: str | None = None   # why _Compiler._rep refuses the layer as the first one, None: it may be
    required: tuple = ()           # the arguments of the reference's constructor that have no default
    keywords: set | None = None    # every keyword it takes (keras.layers.Layer.__init__ raises on another), None: not held to

    @classmethod
    def accepts(cls, cfg: dict) -> bool:
        """Whether the reference's constructor would take this config: the required arguments are there and no key is an
        unknown keyword.  An entry it would not take falls through to ``plan._block``'s generic refusal."""
        return all(k in cfg for k in cls.required) and (cls.keywords is None or not set(cfg) - cls.keywords)

    @classmethod
    def _need_frames(cls, p: str, frames) -> None:
        if frames is None:
            raise UnsupportedLayer(f"{p}: {cls.yaml_name} needs the (frames, length, channels) tensor of the "
                                   "representation learner: not supported in a head or on a strand branch")

    @staticmethod
    def _need_width(p: str, key: str, c: int, cin: int, cite: str) -> None:
        if c != cin:
            raise UnsupportedLayer(f"{p}: {key} {c} != {cin} incoming channels (the layer's residual adds them, {cite})")

    @classmethod
    def _need_fit(cls, p: str, why: str | None, note: str = "") -> None:
        if why is not None:
            raise UnsupportedLayer(f"{p}: {cls.yaml_name} with {why}{note}")


@dataclass(frozen=True)
class AttnKernel:
    """What one of the attention kernels covers, where they differ."""
    channels: tuple
    ff_optional: bool              # feed_forward_dim 0 (no feed-forward half) is allowed
    max_half: int | None           # the largest half-window, None: no window


ATTN_KEY_DIMS = (4, 8, 16, 32, 64)
ATTN_MAX_FF = 256
LOCALATTN_MAX_HALF = 32
LENGTHATTN_CHANNELS = (16, 32, 64)
LENGTHATTN_MAX_FF = ATTN_MAX_FF
FRAMEATTN = AttnKernel((32, 64), True, None)                             # csrc/jg_frameattn.hip
LOCALATTN = AttnKernel((16, 32, 64), False, LOCALATTN_MAX_HALF)          # csrc/jg_localattn.hip
LENGTHATTN = AttnKernel(LENGTHATTN_CHANNELS, False, None)               # csrc/jg_lengthattn.hip


def attn_limit(kernel: AttnKernel, channels: int, heads: int, ff_dim: int, half_window: int = 0) -> str | None:
    """Why the attention kernel cannot run this size, or None."""
    if channels not in kernel.channels:
        return f"embed_dim {channels} (the kernel covers {' / '.join(map(str, kernel.channels))} channels)"
    if heads < 1 or channels % heads or channels // heads not in ATTN_KEY_DIMS:
        return (f"num_heads {heads} at embed_dim {channels} (key_dim = embed_dim / num_heads must be one of "
                f"{', '.join(map(str, ATTN_KEY_DIMS))})")
    if (ff_dim or not kernel.ff_optional) and (ff_dim % 16 or not 16 <= ff_dim <= ATTN_MAX_FF):
        return f"feed_forward_dim {ff_dim} (a multiple of 16 up to {ATTN_MAX_FF})"
    if kernel.max_half is not None and not 0 <= half_window <= kernel.max_half:
        return (f"window_size {2 * half_window} or more (the kernel covers half-windows of 0 to {kernel.max_half} "
                f"positions, window_size up to {2 * kernel.max_half + 1})")
    return None


# the sub-layers of a LocalAttention block under the names CrossFrameAttention / TransformerEncoder give theirs
_LOCALATTN_LEAVES = {"attn_norm": "ln1", "ffn_norm": "ln2", "ffn_dense1": "ffn1", "ffn_dense2": "ffn2"}


def _attn_var(p: str, name: str, leaves: dict) -> str:
    head, rest = name.split("/", 1)
    return f"{p}/{leaves.get(head, head)}/{rest}"


def attn_weight_shapes(p: str, c: int, h: int, d: int, f: int, use_ffn: bool = True, leaves: dict = {}) -> dict[str, tuple]:
    """Keras variable shapes of one attention block under ``p``: LayerNormalization gamma / beta (C); MultiHeadAttention
    query / key / value EinsumDense kernels (C, H, D) with biases (H, D), attention_output kernel (H, D, C) with bias (C);
    the two Dense layers of the feed-forward half.  CrossFrameAttention and TransformerEncoder hold the same sub-layers
    under the same names (layers.py:2224-2245, :2321-2345); a LocalAttention block renames them (``leaves``)."""
    out = {"attn_norm/gamma": (c,), "attn_norm/beta": (c,)}
    for part in ("query", "key", "value"):
        out[f"mha/{part}/kernel"] = (c, h, d)
        out[f"mha/{part}/bias"] = (h, d)
    out["mha/attention_output/kernel"] = (h, d, c)
    out["mha/attention_output/bias"] = (c,)
    if use_ffn:
        out.update({"ffn_norm/gamma": (c,), "ffn_norm/beta": (c,), "ffn_dense1/kernel": (c, f), "ffn_dense1/bias": (f,),
                    "ffn_dense2/kernel": (f, c), "ffn_dense2/bias": (c,)})
    return {_attn_var(p, name, leaves): shp for name, shp in out.items()}


def pack_attn(p: str, c: int, h: int, d: int, use_ffn: bool, w: dict[str, np.ndarray], leaves: dict = {}) -> np.ndarray:
    """The weights of one attention block under ``p`` as the kernels read them (csrc/jg_frameattn.hip, jg_localattn.hip,
    jg_lengthattn.hip), folded in float64:

    * ``LN(x) @ W + b`` with ``LN(x) = n(x) * gamma + beta`` is ``n(x) @ (gamma[:, None] * W) + (beta @ W + b)``: the layer
      norms' gamma / beta go into the q / k / v kernels and into ffn_dense1, the kernel normalises only;
    * MultiHeadAttention multiplies the query by ``1 / sqrt(key_dim)`` behind its bias: into the query's kernel and bias.

    Layout: ``JgAttnWeights`` (csrc/jg_mixer_dev.h), the one view the three attention kernels read the blob through -
    wqkv | bqkv | wo | bo and, with a feed-forward half, w1 | b1 | w2 | b2."""
    f64 = lambda name: np.asarray(w[_attn_var(p, name, leaves)], np.float64)
    g1, be1 = f64("attn_norm/gamma"), f64("attn_norm/beta")
    parts_w, parts_b = [], []
    for part, scale in (("query", 1.0 / np.sqrt(float(d))), ("key", 1.0), ("value", 1.0)):
        kern = f64(f"mha/{part}/kernel").reshape(c, h * d)
        bias = f64(f"mha/{part}/bias").reshape(h * d)
        parts_w.append(g1[:, None] * kern * scale)
        parts_b.append((be1 @ kern + bias) * scale)
    out = [np.stack(parts_w), np.stack(parts_b), f64("mha/attention_output/kernel").reshape(h * d, c),
           f64("mha/attention_output/bias")]
    if use_ffn:
        g2, be2 = f64("ffn_norm/gamma"), f64("ffn_norm/beta")
        k1 = f64("ffn_dense1/kernel")
        out += [g2[:, None] * k1, be2 @ k1 + f64("ffn_dense1/bias"), f64("ffn_dense2/kernel"), f64("ffn_dense2/bias")]
    return np.concatenate([x.ravel() for x in out]).astype(np.float32)


@dataclass
class _Attn(Mixer):
    """What the four attention kinds share: the sizes of an attention block; its variables and its blob under ``name`` as
    CrossFrameAttention and TransformerEncoder hold them."""
    name: str
    channels: int
    heads: int
    key_dim: int
    ff_dim: int
    use_ffn = True                 # (CrossFrameAttention alone can do without its feed-forward half)
    # the two LayerNormalization layers of CrossFrameAttention (layers.py:2321-2323, :2335-2337), of a LocalAttention block
    # (:2556-2558, :2565-2567) and of a TransformerEncoder (:2224-2226, :2237-2239)
    LN_EPSILON = 1e-6

    def weight_shapes(self) -> dict[str, tuple]:
        return attn_weight_shapes(self.name, self.channels, self.heads, self.key_dim, self.ff_dim, self.use_ffn)

    def pack(self, w: dict[str, np.ndarray]) -> np.ndarray:
        return pack_attn(self.name, self.channels, self.heads, self.key_dim, self.use_ffn, w)


@dataclass
class FrameAttn(_Attn):
    """One CrossFrameAttention layer (layers.py:2283-2384): at every position the six frames are six tokens of
    ``channels``: pre-LN (eps 1e-6, :2321-2323) -> MultiHeadAttention(num_heads, key_dim = channels // num_heads,
    :2324-2330) over the frames -> residual (:2367); with ``use_ffn`` LN -> Dense(ff_dim, gelu) -> Dense(channels) ->
    residual (:2370-2376).  The layer does not set supports_masking: no mask leaves it."""
    use_ffn: bool = True           # layers.py:2310
    yaml_name = "cross_frame_attention"

    @classmethod
    def parse(cls, p: str, cfg: dict, cin: int, frames):
        # builder.py:1155: CrossFrameAttention(**config) (embed_dim, num_heads, feed_forward_dim, dropout_rate, use_ffn);
        # :1165-1166: previous_channels = embed_dim
        cls._need_frames(p, frames)
        if frames != 6:
            raise UnsupportedLayer(f"{p}: cross_frame_attention over {frames} frames (the kernel attends over the six "
                                   "reading frames of a translated window)")
        c, h = int(cfg["embed_dim"]), int(cfg["num_heads"])
        use_ffn = bool(cfg.get("use_ffn", True))
        f = int(cfg["feed_forward_dim"]) if use_ffn else 0
        cls._need_width(p, "embed_dim", c, cin, "layers.py:2367")
        cls._need_fit(p, attn_limit(FRAMEATTN, c, h, f))
        return cls(p, c, h, c // h, f, use_ffn)

    def op(self, c, in_buf: int, out_buf: int):
        return c._op(L.OP_FRAMEATTN, in_buf=in_buf, out_buf=out_buf, in_mask=L.JG_BUF_NONE, out_mask=L.JG_BUF_NONE,
                     k=self.heads, cin=self.channels, cout=self.channels, arg=self.ff_dim if self.use_ffn else 0,
                     f0=self.LN_EPSILON, w_off=c.blob.add(self.pack(c.w)))

    def emit(self, c, layers: list, i: int, buf: int, mask: int):
        c._refuse_unmasked_reader(f"{self.name}: cross_frame_attention (it attends over all six frames of a position)")
        # CrossFrameAttention does not set supports_masking (layers.py:2283-2384): the norm / activation / pool / conv
        # behind it see NO mask, and the values the network holds at masked positions flow on as they are
        return c._emit_mixer(layers, i, self.yaml_name, buf, mask, L.JG_BUF_NONE, [lambda src, dst: self.op(c, src, dst)])


@dataclass
class LocalAttn(_Attn):
    """One LocalAttention layer (layers.py:2520-2645): windowed self-attention along the length axis inside every frame
    row, ``blocks`` times: pre-LN (eps 1e-6, :2556-2558) -> MultiHeadAttention(num_heads, key_dim = channels //
    num_heads, :2559-2564) under the mask ``|q - k| <= half_window and mask[k]`` (:2579-2585, :2604-2609) -> residual
    (:2619); LN -> Dense(ff_dim, gelu) -> Dense(channels) -> residual (:2621-2623), always present.  The layer sets
    supports_masking and ``compute_mask`` returns the mask (:2550, :2627-2628): the mask stays behind it."""
    half_window: int               # window_size // 2 (:2581)
    blocks: int = 1                # num_blocks (:2538)
    yaml_name = "local_attention"
    on_embedding = "(the reference's stacks put a conv in front of it; the embedding's rows at invalid codons are not zeros)"
    required = ("embed_dim", "num_heads", "feed_forward_dim", "window_size")   # no defaults (layers.py:2531-2537)

    @classmethod
    def parse(cls, p: str, cfg: dict, cin: int, frames):
        # builder.py:290, :1155: LocalAttention(**config) (embed_dim, num_heads, feed_forward_dim, window_size,
        # dropout_rate, num_blocks); an entry without one of the four required arguments raises in the reference's
        # constructor (``accepts``)
        cls._need_frames(p, frames)
        c, h, f = int(cfg["embed_dim"]), int(cfg["num_heads"]), int(cfg["feed_forward_dim"])
        window, blocks = int(cfg["window_size"]), int(cfg.get("num_blocks", 1))
        if window < 1:
            raise UnsupportedLayer(f"{p}: local_attention window_size {window} (must be positive, layers.py:2542-2543)")
        if blocks < 1:
            raise UnsupportedLayer(f"{p}: local_attention num_blocks {blocks} (at least one block)")
        cls._need_width(p, "embed_dim", c, cin, "layers.py:2619")
        cls._need_fit(p, attn_limit(LOCALATTN, c, h, f, window // 2))
        return cls(p, c, h, c // h, f, window // 2, blocks)

    def weight_shapes(self) -> dict[str, tuple]:
        """Per block ``<name>/block<j>/`` the shapes of an attention block with its feed-forward half."""
        return {name: shp for j in range(self.blocks) for name, shp in attn_weight_shapes(
            f"{self.name}/block{j}", self.channels, self.heads, self.key_dim, self.ff_dim, True, _LOCALATTN_LEAVES).items()}

    def pack(self, w: dict[str, np.ndarray], block: int) -> np.ndarray:
        """The weights of block ``block`` as the kernel reads them (csrc/jg_localattn.hip): :func:`pack_attn`'s fold and
        layout - ln1 / ln2 gamma and beta into the q / k / v kernels and into ffn1, the query's scale into its kernel and bias."""
        return pack_attn(f"{self.name}/block{block}", self.channels, self.heads, self.key_dim, True, w, _LOCALATTN_LEAVES)

    def emit(self, c, layers: list, i: int, buf: int, mask: int):
        # LocalAttention keeps the mask (supports_masking, compute_mask returns it: layers.py:2550, :2627-2628)
        if mask != L.JG_BUF_NONE:
            c.dead_margin = self.half_window if c.dead_margin is None else min(c.dead_margin, self.half_window)
            c.dead_layer = f"{self.name} (local_attention)"
        # one op per block (a tile reads its neighbours' positions as its halo): two slots ping-pong
        return c._emit_mixer(layers, i, self.yaml_name, buf, mask, mask, [
            lambda src, dst, j=j: c._op(L.OP_LOCALATTN, in_buf=src, out_buf=dst, in_mask=mask, out_mask=mask, k=self.heads,
                                        cin=self.channels, cout=self.channels, arg=self.ff_dim, stride=self.half_window,
                                        f0=self.LN_EPSILON, w_off=c.blob.add(self.pack(c.w, j)))
            for j in range(self.blocks)])


AXIAL_NORM_TYPES = ("layernorm", "masked_layernorm", "masked_dyt", "masked_batchnorm")


def _length_sizes(cls, p: str, cfg: dict, cin: int, frames):
    """What transformer_encoder and axial_attention share (builder.py:1155: TransformerEncoder(**config) /
    AxialAttention(**config)): the sizes, held to the length-attention kernel."""
    cls._need_frames(p, frames)
    c, h, f = int(cfg["embed_dim"]), int(cfg["num_heads"]), int(cfg["feed_forward_dim"])
    cls._need_width(p, "embed_dim", c, cin, "layers.py:2256")
    cls._need_fit(p, attn_limit(LENGTHATTN, c, h, f))
    return c, h, f


@dataclass
class LengthAttn(_Attn):
    """One stand-alone TransformerEncoder layer (layers.py:2206-2280) with ``attention_axes = 2``: full self-attention
    along the length axis inside every frame row - pre-LN (eps 1e-6, :2224-2226) -> MultiHeadAttention(num_heads, key_dim
    = channels // num_heads, :2227-2233) under Keras 3's implicit query / value masks -> residual (:2256); LN ->
    Dense(ff_dim, gelu) -> Dense(channels) -> residual (:2259-2264).  The layer does not set supports_masking: no mask
    leaves it."""
    yaml_name = "transformer_encoder"
    on_embedding = "(the reference's stacks put a conv in front of it)"
    required = ("embed_dim", "num_heads", "feed_forward_dim")                    # no defaults (layers.py:2207-2212, :2420-2425)
    # the constructor's own arguments plus what keras.layers.Layer.__init__ takes: any other key is an unknown keyword there
    keywords = {"embed_dim", "num_heads", "feed_forward_dim", "dropout_rate", "attention_axes", "name", "dtype", "trainable"}

    @classmethod
    def parse(cls, p: str, cfg: dict, cin: int, frames):
        c, h, f = _length_sizes(cls, p, cfg, cin, frames)
        axes = cfg.get("attention_axes", 2)
        if axes != 2 and list(axes if isinstance(axes, (list, tuple)) else [axes]) != [2]:
            raise UnsupportedLayer(f"{p}: transformer_encoder attention_axes {axes!r} (the kernel attends along the "
                                   "length axis, attention_axes = 2)")
        return cls(p, c, h, c // h, f)

    def op(self, c, in_buf: int, out_buf: int, in_mask: int, out_mask: int):
        return c._op(L.OP_LENGTHATTN, in_buf=in_buf, out_buf=out_buf, in_mask=in_mask, out_mask=out_mask, k=self.heads,
                     cin=self.channels, cout=self.channels, arg=self.ff_dim, f0=self.LN_EPSILON,
                     w_off=c.blob.add(self.pack(c.w)))

    def emit(self, c, layers: list, i: int, buf: int, mask: int):
        c._refuse_unmasked_reader(f"{self.name}: transformer_encoder (a masked query's output is computed from "
                                  "its input value, and the layer drops the mask)")
        # TransformerEncoder sees the implicit mask of its input (Keras 3 fills MultiHeadAttention's query_mask /
        # value_mask from it) and does not set supports_masking: the norm / activation / pool / conv behind it see NO
        # mask
        return c._emit_mixer(layers, i, self.yaml_name, buf, mask, L.JG_BUF_NONE,
                             [lambda src, dst: self.op(c, src, dst, mask, L.JG_BUF_NONE)])


@dataclass
class AxialAttn(_Attn):
    """One AxialAttention layer (layers.py:2400-2517): per block a TransformerEncoder along the length (:2461-2470), a
    CrossFrameAttention with its feed-forward half (:2474-2483), the post norm and the residual add of the block's input
    (:2485-2501).  Only block 0's encoder sees the layer's incoming mask; ``masked_layernorm`` / ``masked_dyt`` post norms
    get it in every block (:2495-2496).  The layer sets supports_masking (:2442): the mask stays behind it."""
    blocks: int = 1                # num_blocks (:2426)
    norm_type: str = "layernorm"   # :2428 (layernorm | masked_layernorm | masked_dyt | masked_batchnorm)
    epsilon: float = 1e-6          # of the post norm only (:2427); the encoders' layer norms have 1e-6 hard-coded
    alpha_init: float = 0.5        # MaskedDYT's initial alpha (:2429): training only, the weights carry alpha
    yaml_name = "axial_attention"
    on_embedding = LengthAttn.on_embedding

    def post_norm(self, block: int) -> Norm:
        """The post norm of block ``block`` as a :class:`Norm` (``layernorm`` has masked_layernorm's variables)."""
        kind = "masked_layernorm" if self.norm_type == "layernorm" else self.norm_type
        return Norm(f"{self.name}/block{block}/post_norm", kind, self.channels, self.epsilon, True)

    def length(self, block: int) -> LengthAttn:
        return LengthAttn(f"{self.name}/block{block}/length", self.channels, self.heads, self.key_dim, self.ff_dim)

    def frame(self, block: int) -> FrameAttn:
        return FrameAttn(f"{self.name}/block{block}/frame", self.channels, self.heads, self.key_dim, self.ff_dim, True)

    required = LengthAttn.required
    keywords = {"embed_dim", "num_heads", "feed_forward_dim", "dropout_rate", "num_blocks", "epsilon", "norm_type",
                "alpha_init", "name", "dtype", "trainable"}                # as for TransformerEncoder

    @classmethod
    def parse(cls, p: str, cfg: dict, cin: int, frames):
        c, h, f = _length_sizes(cls, p, cfg, cin, frames)
        if frames != 6:
            raise UnsupportedLayer(f"{p}: axial_attention over {frames} frames (its frame half attends over the six "
                                   "reading frames of a translated window)")
        blocks = int(cfg.get("num_blocks", 1))
        if blocks < 1:
            raise UnsupportedLayer(f"{p}: axial_attention num_blocks {blocks} (at least one block)")
        nt = str(cfg.get("norm_type", "layernorm")).lower()
        nt = "layernorm" if nt == "layer_normalization" else nt          # layers.py:2449
        if nt not in AXIAL_NORM_TYPES:
            raise UnsupportedLayer(f"{p}: axial_attention norm_type {nt!r} (layers.py:2457 raises: one of "
                                   f"{', '.join(AXIAL_NORM_TYPES)})")
        cls._need_fit(p, attn_limit(FRAMEATTN, c, h, f), " (its frame half)")
        return cls(p, c, h, c // h, f, blocks, nt, float(cfg.get("epsilon", 1e-6)), float(cfg.get("alpha_init", 0.5)))

    def weight_shapes(self) -> dict[str, tuple]:
        out: dict[str, tuple] = {}
        for j in range(self.blocks):
            out.update(self.length(j).weight_shapes())
            out.update(self.frame(j).weight_shapes())
            out.update(norm_weight_shapes(self.post_norm(j)))
        return out

    def emit(self, c, layers: list, i: int, buf: int, mask: int):
        c._refuse_unmasked_reader(f"{self.name}: axial_attention (a masked query's output is computed from its "
                                  "input value, and its frame half attends over all six frames of a position)")
        # per block (layers.py:2485-2501): r = x; x = length(x) - under the layer's incoming mask in block 0 only:
        # from block 1 on x is the result of a tensor op inside call() and carries no implicit mask -; x = frame(x),
        # unmasked; x = norm(x) (masked_layernorm / masked_dyt: with the incoming mask, in every block) + r.  The layer
        # keeps the mask (supports_masking, :2442); the block-input slot stays taken until the add
        pending: list = []
        for j in range(self.blocks):
            t1 = c.bufs.take()
            lm = mask if j == 0 else L.JG_BUF_NONE
            c.ops.append(self.length(j).op(c, buf, t1, lm, lm))
            t2 = c.bufs.take()
            c.ops.append(self.frame(j).op(c, t1, t2))
            c.bufs.give(t1)
            masked_norm = self.norm_type in ("masked_layernorm", "masked_dyt") and mask != L.JG_BUF_NONE
            stages = [c._norm_stage(self.post_norm(j), masked_norm), c._stage(L.ST_ADD, arg=buf)]
            mask2 = mask
            if j == self.blocks - 1:
                i, mask2 = c._fuse_tail(layers, i + 1, stages, mask, self.channels, pending)
                if pending:
                    raise UnsupportedLayer(f"{self.name}: an nmd tap directly behind axial_attention is not supported "
                                           "(the element-wise op that closes the layer carries no partial sums)")
            c._emit_ln_tail(self.name, stages, mask, t2, self.channels)
            c.bufs.give(buf)
            buf = t2
        if mask2 != mask:
            c.masks.give(mask)
        return i, buf, mask2


def norm_weight_shapes(n: Norm) -> dict[str, tuple]:
    vars_ = {"masked_batchnorm": ("gamma", "beta", "moving_mean", "moving_variance"),
             "masked_dyt": ("alpha", "gamma", "beta"),
             "masked_layernorm": ("gamma", "beta")}[n.kind]
    return {f"{n.name}/{v}": (1,) if v == "alpha" else (n.channels,) for v in vars_}


#: what the hyena kernels (csrc/jg_hyena.hip) and the host's filter table cover
HYENA_CHANNELS = (16, 32, 64)
HYENA_MAX_ORDER = 4
HYENA_PE_DIM = 16                  # HyenaFilter's pe_dim default (:2797); HyenaOperator never passes another
HYENA_ACTIVATIONS = ("gelu", "sin", "relu", "tanh", "sigmoid", "silu", "swish", "linear")
HYENA_EPSILON = 1e-6           # the LayerNormalization of a HyenaBlock (layers.py:3075)
POSITION_ROWS = 8192        # rows of the position table a program carries: windows of up to 24 576 bases (a row = one frame's codons)


def hyena_limit(channels: int, order: int, filter_layers: int, activation) -> str | None:
    """Why the hyena kernels / the host's filter table cannot run this layer, or None."""
    if channels not in HYENA_CHANNELS:
        return f"dim {channels} (the kernels cover {' / '.join(map(str, HYENA_CHANNELS))} channels)"
    if not 1 <= order <= HYENA_MAX_ORDER:
        return f"order {order} (the kernels cover orders 1 to {HYENA_MAX_ORDER})"
    if filter_layers < 1:
        return f"filter_layers {filter_layers} (the filter network needs at least one Dense layer)"
    if activation is not None and str(activation).lower() not in HYENA_ACTIVATIONS:
        return (f"filter_activation {activation!r} (the host tables the filter with one of "
                f"{', '.join(HYENA_ACTIVATIONS)} or none)")
    return None


def hyena_position_rows(n_pos: int) -> np.ndarray:
    """HyenaFilter._make_positional_encoding (layers.py:2871-2880) for positions 0 .. n_pos - 1 at pe_dim 16: the ARGUMENTS
    ``pos * div`` as the reference forms them, float32 products of float32 factors (``div = exp(range(0, 16, 2) * -(log(10000)
    / 16))``), their sine and cosine in float64; row ``[sin_0, cos_0, sin_1, cos_1, ...]``."""
    f = np.float32
    pos = np.arange(n_pos, dtype=f)[:, None]
    div = np.exp(np.arange(0, HYENA_PE_DIM, 2, dtype=f) * f(-(np.log(f(10000.0)) / f(HYENA_PE_DIM)))).astype(f)
    arg = (pos * div[None, :]).astype(f).astype(np.float64)
    return np.stack([np.sin(arg), np.cos(arg)], axis=-1).reshape(n_pos, HYENA_PE_DIM)


def _hyena_activation(name, x: np.ndarray) -> np.ndarray:
    """HyenaFilter._hidden_activation (layers.py:2864-2869) in float64: "sin" is tf.sin, the others what Keras 3 resolves
    the name to ("gelu": the tanh form)."""
    if name is None or name == "linear":
        return x
    if name == "sin":
        return np.sin(x)
    if name == "gelu":
        return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))
    if name == "relu":
        return np.maximum(x, 0.0)
    if name == "tanh":
        return np.tanh(x)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if name in ("silu", "swish"):
        return x / (1.0 + np.exp(-x))
    raise UnsupportedLayer(f"hyena filter_activation {name!r} cannot be evaluated on the host")


def hyena_table_rows(a: "Hyena") -> int:
    """Rows of the layer's filter table: ``seq_len`` where the layer fixes it (the reference's stored positional encoding has
    that many rows, a longer call fails there), else the position rows a program carries."""
    return a.seq_len if a.seq_len is not None else POSITION_ROWS


def hyena_filter_tables(a: "Hyena", w: dict[str, np.ndarray], rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """HyenaFilter.call (layers.py:2882-2915) for every position the program may meet, once:
    ``h[i, t, :] = (exp(-|alpha_i| t) + bias_i) * FFN_i(PE[t])`` as float32 ``(order, rows, C)``, evaluated in float64 from the
    positional rows (the stored ``<name>/hyena/filter/pos_encoding`` of a layer with ``seq_len`` if the weights hold it, else recomputed) - and the
    running sum of its squares over ``t``, ``ssq[i, t, :] = sum over s <= t of h[i, s, :] ** 2`` (of the float32 table, summed
    in float64): with ``filter_normalize`` a call at ``l`` positions divides channel ``c`` of filter ``i`` by
    ``sqrt(ssq[i, l - 1, c])``, and by nothing where that is zero (divide_no_nan)."""
    rows = hyena_table_rows(a) if rows is None else rows
    # (without seq_len the reference stores one row and recomputes the encoding at every call, :2817, :2888-2891)
    stored = w.get(f"{a.name}/hyena/filter/pos_encoding") if a.seq_len is not None else None
    if stored is not None:
        stored = np.asarray(stored, np.float64)
        if stored.ndim != 2 or stored.shape[1] != HYENA_PE_DIM or stored.shape[0] < rows:
            raise ValueError(f"weight {a.name}/hyena/filter/pos_encoding: shape {stored.shape} != expected ({rows}, {HYENA_PE_DIM})")
        pe = stored[:rows]
    else:
        pe = hyena_position_rows(rows)
    f64 = lambda name: np.asarray(w[f"{a.name}/hyena/filter/{name}"], np.float64)
    alphas, biases = np.abs(f64("alphas")), f64("biases")
    t = np.arange(rows, dtype=np.float64)[:, None]
    h = np.empty((a.order, rows, a.channels), np.float32)
    for i in range(a.order):
        x = pe
        for j in range(a.filter_layers):
            x = x @ f64(f"ffn_{i}/dense_{j}/kernel") + f64(f"ffn_{i}/dense_{j}/bias")
            if j < a.filter_layers - 1:
                x = _hyena_activation(a.filter_activation, x)
        h[i] = ((np.exp(-alphas[i][None, :] * t) + biases[i][None, :]) * x).astype(np.float32)
    ssq = np.cumsum(h.astype(np.float64) ** 2, axis=1).astype(np.float32)
    return h, ssq


@dataclass
class Hyena(Mixer):
    """One HyenaBlock (layers.py:3023-3153) on the rows of the (frames, length, channels) tensor: ``x * m`` -> LayerNorm
    (eps 1e-6, :3075) ``* m`` -> HyenaOperator (:2937-3002: ``order + 1`` bias-free projections, ``order`` gated causal long
    convolutions whose filters come from HyenaFilter, :2766-2915) -> with ``output_projection`` Dense(channels) -> plus the
    masked input, ``* m`` (:3103-3133).  The layer sets supports_masking (:3072): the mask stays behind it, and masked
    positions are exact zeros."""
    name: str
    channels: int
    order: int = 2                 # :3051
    filter_hidden: int = 32        # :3052
    filter_layers: int = 2         # :3053
    filter_activation: str | None = "gelu"   # :3054
    filter_normalize: bool = False # :3057
    output_projection: bool = False   # :3056
    seq_len: int | None = None     # :3050: rows of the stored positional encoding; a longer call fails in the reference
    yaml_name = "hyena_block"
    tap_lookahead = True

    required = ("dim",)
    # the constructor's own arguments (:3047-3059) plus what keras.layers.Layer.__init__ takes; kernel_regularizer_w is the
    # builder's spelling of the regulariser's weight
    keywords = {"dim", "seq_len", "order", "filter_hidden", "filter_layers", "filter_activation", "dropout",
                "output_projection", "filter_normalize", "kernel_regularizer", "kernel_regularizer_w", "name", "dtype",
                "trainable"}

    @classmethod
    def parse(cls, p: str, cfg: dict, cin: int, frames):
        # builder.py:1155: HyenaBlock(**config); an entry without `dim` or with an unknown keyword raises in the reference's
        # constructor (``accepts``).  dropout and the regulariser matter in training only
        cls._need_frames(p, frames)
        c, order = int(cfg["dim"]), int(cfg.get("order", 2))
        cls._need_width(p, "dim", c, cin, "layers.py:3129")
        fl, act = int(cfg.get("filter_layers", 2)), cfg.get("filter_activation", "gelu")
        cls._need_fit(p, hyena_limit(c, order, fl, act))
        seq_len = cfg.get("seq_len")
        if seq_len is not None and int(seq_len) < 1:
            raise UnsupportedLayer(f"{p}: hyena_block seq_len {seq_len} (a positive number of positions, or none)")
        return cls(p, c, order, int(cfg.get("filter_hidden", 32)), fl,
                   None if act is None or str(act).lower() == "linear" else str(act).lower(),
                   bool(cfg.get("filter_normalize", False)), bool(cfg.get("output_projection", False)),
                   None if seq_len is None else int(seq_len))

    def weight_shapes(self) -> dict[str, tuple]:
        """Keras variable shapes of one HyenaBlock: the LayerNormalization's gamma / beta (C); the operator's ``order + 1``
        bias-free projections (C, C); per order the filter network's Dense layers (16 -> filter_hidden ... -> C, the last one
        alone with ``filter_layers`` 1) and the window's ``alphas`` / ``biases`` (order, C); the output projection if there is
        one.  ``<name>/hyena/filter/pos_encoding`` (seq_len, 16) is optional and not listed: when the weights hold it the
        filter table uses its rows (:func:`hyena_filter_tables`)."""
        c, n = self.channels, self.name
        out: dict[str, tuple] = {f"{n}/norm/gamma": (c,), f"{n}/norm/beta": (c,)}
        for k in range(self.order + 1):
            out[f"{n}/hyena/proj_{k}/kernel"] = (c, c)
        for o in range(self.order):
            cin = HYENA_PE_DIM
            for j in range(self.filter_layers):
                units = c if j == self.filter_layers - 1 else self.filter_hidden
                out[f"{n}/hyena/filter/ffn_{o}/dense_{j}/kernel"] = (cin, units)
                out[f"{n}/hyena/filter/ffn_{o}/dense_{j}/bias"] = (units,)
                cin = units
        out[f"{n}/hyena/filter/alphas"] = (self.order, c)
        out[f"{n}/hyena/filter/biases"] = (self.order, c)
        if self.output_projection:
            out[f"{n}/out_proj/kernel"] = (c, c)
            out[f"{n}/out_proj/bias"] = (c,)
        return out

    def check_weights(self, w: dict) -> None:
        # (optional: the stored positional encoding of a layer with seq_len is used when it is there)
        pe = f"{self.name}/hyena/filter/pos_encoding"
        if pe in w and self.seq_len is not None and tuple(w[pe].shape) != (self.seq_len, HYENA_PE_DIM):
            raise ValueError(f"weight {pe}: shape {tuple(w[pe].shape)} != expected ({self.seq_len}, {HYENA_PE_DIM}) "
                             "(HyenaFilter stores the rows of its seq_len only)")

    def pack(self, w: dict[str, np.ndarray]) -> np.ndarray:
        """The weights and tables of one HyenaBlock as the kernels read them (csrc/jg_hyena.hip), folded in float64:
        ``(n(x) * gamma + beta) @ W_k`` is ``n(x) @ (gamma[:, None] * W_k) + beta @ W_k`` - the kernel normalises only, and
        zeroes the projections of a masked position.  Layout: wp [order + 1][C][C] | bp [order + 1][C] | with
        output_projection wo [C][C] | bo [C] | h [order][rows][C] | with filter_normalize ssq [order][rows][C]."""
        f64 = lambda name: np.asarray(w[f"{self.name}/{name}"], np.float64)
        gamma, beta = f64("norm/gamma"), f64("norm/beta")
        kernels = [f64(f"hyena/proj_{k}/kernel") for k in range(self.order + 1)]
        out = [np.stack([gamma[:, None] * k for k in kernels]), np.stack([beta @ k for k in kernels])]
        if self.output_projection:
            out += [f64("out_proj/kernel"), f64("out_proj/bias")]
        h, ssq = hyena_filter_tables(self, w)
        out.append(h)
        if self.filter_normalize:
            out.append(ssq)
        return np.concatenate([np.asarray(x, np.float32).ravel() for x in out])

    def emit(self, c, layers: list, i: int, buf: int, mask: int):
        # HyenaBlock multiplies by the mask on entry, behind its layer norm and on exit (layers.py:3109-3132): it
        # reads valid positions only and writes Keras' exact values everywhere - zeros at masked positions.  So it
        # may stand behind a local_attention with live dead positions, and its output holds none.  It keeps the mask
        # (supports_masking, :3072)
        if mask == L.JG_BUF_NONE:
            c._refuse_unmasked_reader(f"{self.name}: hyena_block without a mask")
        c.dead_margin = None
        flags = (L.HYENA_OUT_PROJ if self.output_projection else 0) | (L.HYENA_NORMALIZE if self.filter_normalize else 0)
        return c._emit_mixer(layers, i, self.yaml_name, buf, mask, mask, [
            lambda src, dst: c._op(L.OP_HYENA, in_buf=src, out_buf=dst, in_mask=mask, out_mask=mask, k=self.order,
                                   cin=self.channels, cout=self.channels, stride=hyena_table_rows(self), f0=HYENA_EPSILON,
                                   arg=flags, w_off=c.blob.add(self.pack(c.w)))])


#: what the kernel (csrc/jg_bilstm.hip) covers
BILSTM_UNITS = (16, 32, 64)
BILSTM_MAX_CHANNELS = 128


def bilstm_limit(channels: int, units: int) -> str | None:
    """Why the bilstm kernel cannot run this layer, or None."""
    if units not in BILSTM_UNITS:
        return f"units {units} (the kernel covers {' / '.join(map(str, BILSTM_UNITS))} units)"
    if channels % 16 or not 16 <= channels <= BILSTM_MAX_CHANNELS:
        return f"{channels} incoming channels (a multiple of 16 up to {BILSTM_MAX_CHANNELS})"
    return None


@dataclass
class BiLstm(Mixer):
    """One MaskedBiLSTM (layers.py:1335-1430) on the rows of the (frames, length, channels) tensor: Keras 3
    ``Bidirectional(LSTM(units, return_sequences=True), merge_mode="concat")`` under the incoming mask - a masked step keeps
    both states and repeats the direction's previous output (zeros while no valid step has come) - or, with ``ignore_mask``,
    under none.  ``compute_mask`` returns the mask, or None with ``ignore_mask`` (:1405-1410)."""
    name: str
    cin: int
    units: int
    ignore_mask: bool = False      # :1361
    yaml_name = "masked_bilstm"
    tap_lookahead = True

    @property
    def channels(self) -> int:
        """What the layer leaves: the two directions side by side."""
        return 2 * self.units

    required = ("units",)
    # the constructor's own arguments (:1354-1363) plus what keras.layers.Layer.__init__ takes
    keywords = {"units", "dropout", "recurrent_dropout", "return_sequences", "use_cudnn", "ignore_mask", "name", "dtype",
                "trainable"}

    @classmethod
    def parse(cls, p: str, cfg: dict, cin: int, frames):
        # builder.py:282, :1155: MaskedBiLSTM(**config); an entry without `units` or with an unknown keyword raises in the
        # reference's constructor (``accepts``).  dropout / recurrent_dropout matter in training only, use_cudnn changes
        # no formula
        cls._need_frames(p, frames)
        if not bool(cfg.get("return_sequences", True)):
            raise UnsupportedLayer(f"{p}: masked_bilstm with return_sequences: false (the tensor loses its length axis, "
                                   "and no layer behind it here takes a (frames, channels) tensor)")
        units = int(cfg["units"])
        cls._need_fit(p, bilstm_limit(cin, units))
        return cls(p, cin, units, bool(cfg.get("ignore_mask", False)))

    def weight_shapes(self) -> dict[str, tuple]:
        """Keras variable shapes of one MaskedBiLSTM: per direction (``layer.bilstm.forward_layer.cell`` /
        ``backward_layer.cell``) the LSTMCell's kernel (C, 4U), recurrent_kernel (U, 4U) and bias (4U), the 4U columns in the
        gate order i, f, g, o."""
        out: dict[str, tuple] = {}
        for d in ("forward", "backward"):
            out[f"{self.name}/{d}/kernel"] = (self.cin, 4 * self.units)
            out[f"{self.name}/{d}/recurrent_kernel"] = (self.units, 4 * self.units)
            out[f"{self.name}/{d}/bias"] = (4 * self.units,)
        return out

    def pack(self, w: dict[str, np.ndarray]) -> np.ndarray:
        """The weights of one MaskedBiLSTM as the kernel reads them (csrc/jg_bilstm.hip): per direction (forward, backward)
        W [C][4U] | R [U][4U] | b [4U], the 4U columns permuted so that the four gates of one unit stand next to each other and
        the units of one wave together - column ``64 w + 4 n + g`` holds Keras' column ``g U + 16 w + n`` (gate g of i, f, g, o;
        unit 16 w + n).  Nothing is folded: the values pass through float64 and are rounded back unchanged."""
        u = self.units
        perm = np.arange(4 * u).reshape(4, u).T.ravel()                    # new column 4 unit + g <- old column g U + unit
        out = []
        for d in ("forward", "backward"):
            f64 = lambda name: np.asarray(w[f"{self.name}/{d}/{name}"], np.float64)
            out += [f64("kernel")[:, perm], f64("recurrent_kernel")[:, perm], f64("bias")[perm]]
        return np.concatenate([x.ravel() for x in out]).astype(np.float32)

    def emit(self, c, layers: list, i: int, buf: int, mask: int):
        # MaskedBiLSTM hands its mask to the two LSTMs (layers.py:1392-1397): a masked step keeps the states and
        # repeats the previous output, so x at a masked position reaches no output and every output is defined and
        # finite - the layer may stand behind a local_attention with live dead positions, and its output holds none.
        # With ignore_mask (or no mask) it reads every position, and drops the mask (:1405-1410)
        if self.ignore_mask or mask == L.JG_BUF_NONE:
            c._refuse_unmasked_reader(f"{self.name}: masked_bilstm with ignore_mask" if self.ignore_mask
                                      else f"{self.name}: masked_bilstm without a mask")
        else:
            c.dead_margin = None
        out_mask = L.JG_BUF_NONE if self.ignore_mask else mask
        return c._emit_mixer(layers, i, self.yaml_name, buf, mask, out_mask, [
            lambda src, dst: c._op(L.OP_BILSTM, in_buf=src, out_buf=dst, in_mask=mask, out_mask=out_mask, k=self.units,
                                   cin=self.cin, cout=self.channels, arg=L.BILSTM_IGNORE_MASK if self.ignore_mask else 0,
                                   w_off=c.blob.add(self.pack(c.w)))])


#: what the kernel (csrc/jg_msconv.hip) covers
MSCONV_MAX_BRANCHES = 4
MSCONV_MAX_CHANNELS = 128
MSCONV_MAX_KERNEL = 15
MSCONV_MAX_SPAN = 64
# MaskedConv1D's arguments (:1150-1168) a branch entry may carry
_MSCONV_BRANCH_KEYS = {"filters", "kernel_size", "strides", "padding", "dilation_rate", "activation", "use_bias",
                       "kernel_initializer", "bias_initializer", "kernel_regularizer", "axis",
                       "use_masking", "mask_mode", "name", "dtype", "trainable"}


def msconv_limit(cin: int, merge: str, branches: list) -> str | None:
    """Why the multi-scale conv kernel cannot run this layer, or None."""
    if cin % 16 or not 16 <= cin <= MSCONV_MAX_CHANNELS:
        return f"{cin} incoming channels (a multiple of 16 up to {MSCONV_MAX_CHANNELS})"
    if not 1 <= len(branches) <= MSCONV_MAX_BRANCHES:
        return f"{len(branches)} branches (the kernel covers 1 to {MSCONV_MAX_BRANCHES})"
    for b, c in enumerate(branches):
        if c.filters % 8 or not 8 <= c.filters <= MSCONV_MAX_CHANNELS:
            return f"branch {b}: filters {c.filters} (a multiple of 8 up to {MSCONV_MAX_CHANNELS})"
        if not 1 <= c.kernel_size <= MSCONV_MAX_KERNEL:
            return f"branch {b}: kernel_size {c.kernel_size} (the kernel covers 1 to {MSCONV_MAX_KERNEL})"
        if c.dilation_rate < 1 or (c.kernel_size - 1) * c.dilation_rate > MSCONV_MAX_SPAN:
            return (f"branch {b}: (kernel_size - 1) x dilation_rate = {(c.kernel_size - 1) * c.dilation_rate} "
                    f"(dilation_rate at least 1, the product up to {MSCONV_MAX_SPAN})")
    cout = sum(c.filters for c in branches) if merge == "concat" else branches[0].filters
    if cout % 16 or not 16 <= cout <= MSCONV_MAX_CHANNELS:
        return f"{cout} output channels (a multiple of 16 up to {MSCONV_MAX_CHANNELS})"
    return None


@dataclass
class MultiScaleConv(Mixer):
    """One MultiScaleConv1D (layers.py:1433-1595): ``len(branches)`` MaskedConv1Ds over the same rows of the (frames, length,
    channels) tensor, every one with padding "same" and strides 1 (:1504-1505, :1517-1526) and its own kernel_size,
    dilation_rate, activation, use_bias and mask_mode; their outputs concatenated along the channels (``merge`` "concat") or
    summed in branch order (``merge`` "add", tf.add_n; :1539-1542).  The mask behind the layer is the AND of the branches'
    output masks (:1544-1548), none where the branches do not mask or no mask arrives."""
    name: str
    cin: int
    merge: str                     # "concat" | "add" (:1448)
    branches: list                 # list[Conv], named <name>/branch<b>
    yaml_name = "multi_scale_conv"
    tap_lookahead = True

    @property
    def channels(self) -> int:
        """What the layer leaves: the branches side by side, or their common width."""
        return sum(b.filters for b in self.branches) if self.merge == "concat" else self.branches[0].filters

    @property
    def use_masking(self) -> bool:
        return self.branches[0].use_masking

    required = ("branches",)
    # the constructor's own arguments (:1445-1453); the last three matter in training only
    keywords = {"branches", "merge", "use_bias", "kernel_initializer", "kernel_regularizer", "kernel_regularizer_w"}

    @classmethod
    def parse(cls, p: str, cfg: dict, cin: int, frames):
        # builder.py:277-304, :1155: MultiScaleConv1D(**config); an entry without `branches` or with a key that is none of
        # the constructor's arguments raises there (``accepts``).  The initialiser and the regulariser matter in training
        # only
        branches, merge = cfg["branches"], cfg.get("merge", "concat")
        if not isinstance(branches, list) or len(branches) == 0 or not all(isinstance(b, dict) for b in branches):
            raise ValueError(f"{p}: branches must be a non-empty list of dicts")                      # :1456-1459
        if merge not in ("concat", "add"):
            raise ValueError(f"{p}: merge must be 'concat' or 'add', got {merge!r}")                 # :1460-1461
        if merge == "add" and len({b.get("filters") for b in branches}) != 1:
            raise ValueError(f"{p}: All branches must have the same filters when merge='add'")        # :1495-1500
        convs = []
        for b, bcfg in enumerate(branches):
            pad, strides = bcfg.get("padding", "same"), bcfg.get("strides", 1)                       # :1504-1505
            if str(pad).lower() != "same":
                raise ValueError(f"{p}: Branch {b}: padding must be 'same' to keep sequence length aligned across "
                                 f"branches, got {pad!r}")                                            # :1517-1521
            if strides != 1:
                raise ValueError(f"{p}: Branch {b}: strides must be 1 to keep sequence length aligned across "
                                 f"branches, got {strides!r}")                                        # :1522-1526
            mode = bcfg.get("mask_mode", "any")
            if mode not in ("any", "majority", "strict"):
                raise ValueError(f"{p}: Branch {b}: Invalid mask_mode: {mode!r} (use 'any', 'majority' or 'strict')")   # :1170-1173
            if set(bcfg) - _MSCONV_BRANCH_KEYS:
                raise UnsupportedLayer(f"{p}: branch {b}: {sorted(set(bcfg) - _MSCONV_BRANCH_KEYS)} are no arguments of "
                                       "MaskedConv1D (layers.py:1148-1165)")
            if bcfg.get("axis", -1) != -1:
                raise UnsupportedLayer(f"{p}: branch {b}: axis {bcfg['axis']!r} (the kernel convolves along the length axis "
                                       "with the channels last, axis = -1)")
            # use_bias defaults to the layer's (:1515); use_masking to MaskedConv1D's own True (:1161): builder.py:1019-1020
            # injects the model-level use_masking for masked_conv1d / masked_batchnorm / residual_block entries only
            convs.append(Conv(f"{p}/branch{b}", int(bcfg["kernel_size"]), cin, int(bcfg["filters"]), 1, "same",
                              int(bcfg.get("dilation_rate", 1)), bool(bcfg.get("use_bias", cfg.get("use_bias", True))),
                              bcfg.get("activation"), bool(bcfg.get("use_masking", True)), mode))
        cls._need_frames(p, frames)
        if len({c.use_masking for c in convs}) != 1:
            raise UnsupportedLayer(f"{p}: multi_scale_conv whose branches disagree on use_masking (the reference ANDs a "
                                   "branch's mask with None there, layers.py:1544-1548)")
        cls._need_fit(p, msconv_limit(cin, merge, convs))
        # builder.py:1161-1166 does not update previous_channels behind this layer (the entry has no top-level `filters`),
        # so a residual_block that follows is constructed with a stale `shape` (:1075-1087).  That argument reaches
        # ResidualBlockStack.__init__ as `in_shape` and is never read (layers.py:2658-2692, :2716-2721): the blocks build
        # from the tensor they are called on.  The graph is the same, so such a block is accepted
        return cls(p, cin, merge, convs)

    def weight_shapes(self) -> dict[str, tuple]:
        """Keras variable shapes of one MultiScaleConv1D: per branch (``layer._convs[b]``, a MaskedConv1D) the kernel
        (kernel_size, cin, filters) and, with use_bias, the bias (filters)."""
        out: dict[str, tuple] = {}
        for c in self.branches:
            out[f"{c.name}/kernel"] = (c.kernel_size, c.cin, c.filters)
            if c.use_bias:
                out[f"{c.name}/bias"] = (c.filters,)
        return out

    def pack(self, w: dict[str, np.ndarray]) -> np.ndarray:
        """The blob of one MultiScaleConv1D as the two ops read it (csrc/jg_msconv.h): a descriptor of ``MSCONV_MAX_BRANCHES`` x
        ``MSCONV_DESC_FIELDS`` int32 values stored as float32 BIT PATTERNS - per branch filters, taps, dilation, activation code,
        mask mode, has-bias, channel offset in the output (0 for every branch under "add"), weight offset in floats from the
        blob's start; unused branches zeros - then per branch the kernel ``[taps][cin][fpad]`` and the bias ``[fpad]``, fpad =
        filters rounded up to 16, the padding columns and an absent bias zeros.  Nothing is folded."""
        n = L.MSCONV_MAX_BRANCHES * L.MSCONV_DESC_FIELDS
        desc = np.zeros((L.MSCONV_MAX_BRANCHES, L.MSCONV_DESC_FIELDS), np.int32)
        parts, at, ch = [], n, 0
        for b, c in enumerate(self.branches):
            fpad = (c.filters + 15) // 16 * 16
            kern = np.zeros((c.kernel_size, c.cin, fpad), np.float32)
            kern[:, :, :c.filters] = np.asarray(w[f"{c.name}/kernel"], np.float32)
            bias = np.zeros(fpad, np.float32)
            if c.use_bias:
                bias[:c.filters] = np.asarray(w[f"{c.name}/bias"], np.float32)
            desc[b] = (c.filters, c.kernel_size, c.dilation_rate, act_code(c.activation), _MASK_MODE[c.mask_mode], int(c.use_bias),
                       ch if self.merge == "concat" else 0, at)
            parts += [kern.ravel(), bias]
            at += kern.size + fpad
            ch += c.filters
        return np.concatenate([desc.ravel().view(np.float32)] + parts)

    def emit(self, c, layers: list, i: int, buf: int, mask: int):
        # Every branch is a MaskedConv1D (layers.py:1217-1280): it multiplies its input by the mask and convolves, so
        # the layer reads valid positions only and writes defined values everywhere - it may stand behind a
        # local_attention with live dead positions, and its output holds none (as behind a masked conv).  With
        # use_masking false in all branches (or no mask) it reads every position, and no mask leaves it
        masked = self.use_masking and mask != L.JG_BUF_NONE
        if masked:
            c.dead_margin = None
        else:
            c._refuse_unmasked_reader(f"{self.name}: multi_scale_conv whose branches do not mask" if mask != L.JG_BUF_NONE
                                      else f"{self.name}: multi_scale_conv without a mask")
        fields = dict(k=len(self.branches), cin=self.cin, cout=self.channels,
                      arg=L.MSCONV_ADD if self.merge == "add" else L.MSCONV_CONCAT, w_off=c.blob.add(self.pack(c.w)))
        in_mask, out_mask = (mask, c.masks.take()) if masked else (L.JG_BUF_NONE, L.JG_BUF_NONE)
        if masked:      # the layer's output-mask rule, in front of the op whose output it describes
            c.ops.append(c._op(L.OP_MSMASK, in_mask=in_mask, out_mask=out_mask, **fields))
        return c._emit_mixer(layers, i, self.yaml_name, buf, mask, out_mask, [
            lambda src, dst: c._op(L.OP_MSCONV, in_buf=src, out_buf=dst, in_mask=in_mask, out_mask=out_mask, **fields)])


def unpack_msconv_descriptor(blob: np.ndarray, n_branches: int) -> list[dict]:
    """The descriptor at the head of a :meth:`MultiScaleConv.pack` blob, back as one dict per branch."""
    fields = ("filters", "taps", "dilation", "activation", "mask_mode", "has_bias", "channel_offset", "weight_offset")
    n = L.MSCONV_MAX_BRANCHES * L.MSCONV_DESC_FIELDS
    desc = np.ascontiguousarray(blob[:n], np.float32).view(np.int32).reshape(L.MSCONV_MAX_BRANCHES, L.MSCONV_DESC_FIELDS)
    return [dict(zip(fields, map(int, desc[b]))) for b in range(n_branches)]


#: YAML name -> class, in the order ``weights.attention_kinds`` names them
MIXERS = {cls.yaml_name: cls for cls in (FrameAttn, LocalAttn, LengthAttn, AxialAttn, Hyena, BiLstm, MultiScaleConv)}
