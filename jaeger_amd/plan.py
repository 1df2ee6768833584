"""``*_project.yaml`` -> explicit layer plan.

The reference turns the ``model:`` section of a project YAML into a Keras graph
in ``nnlib/builder.py`` (``build_fragment_classifier`` :442-838,
``_build_embedding`` :844-894, ``_build_block`` :982-1193, ``_get_pooler``
:1697-1714).  This module resolves the same section into a flat, fully
defaulted plan (every default below cites the constructor it comes from) that
``program.py`` compiles for the MI355X engine.  Layers outside the conv family
(gated pooling ...) raise :class:`UnsupportedLayer`; the attention layers, ``hyena_block``, ``masked_bilstm``,
``multi_scale_conv`` and ``parallel_branches`` are plan nodes of their own.

Canonical weight names (shared with the loaders in ``weights.py``):
``embedding/embeddings``; ``rep/<i>/{kernel,bias,gamma,beta,moving_mean,
moving_variance,alpha}`` for the i-th ``hidden_layers`` entry;
``rep/<i>/block<j>/{conv1,conv2,conv3,bn1,bn2,bn3}/<var>`` inside a
``residual_block``; ``rep/<i>/{forward,backward}/{kernel,recurrent_kernel,bias}`` for a ``masked_bilstm``;
``rep/<i>/branch<b>/{kernel,bias}`` for the b-th branch of a ``multi_scale_conv``;
``rep/<i>/branch<b>/<j>/...`` for the j-th ``hidden_layers`` entry of the b-th branch of a ``parallel_branches``, by the same
rules as ``rep/<j>/...``;
``classifier/<i>/...`` and ``reliability/<i>/...`` for the heads.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Any

from . import maps

_ACT_ALIASES = ("relu", "gelu", "sigmoid", "softmax", "tanh")
_NORMS = ("masked_batchnorm", "masked_dyt", "masked_layernorm")
_DEFAULT_SIGNALS = ["max_prob", "entropy", "energy", "margin", "nmd_norm"]


class UnsupportedLayer(ValueError):
    """A layer / option of the project YAML that the MI355X engine does not implement."""


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


@dataclass
class Act:
    kind: str


@dataclass
class Nmd:
    name: str
    channels: int
    epsilon: float = 1e-5          # nmd.py:19


@dataclass
class ResBlock:
    """One ResidualBlock (layers.py:1774-1915)."""
    name: str
    conv1: Conv
    bn1: Norm
    conv2: Conv
    bn2: Norm
    conv3: Conv | None
    bn3: Norm | None
    activation: str = "gelu"       # layers.py:1781
    use_masking: bool = True
    nmd: "Nmd | None" = None       # return_nmd (last block of a stack): bn2's NMD side output (layers.py:1896-1899)


@dataclass
class Dense:
    name: str
    cin: int
    units: int
    use_bias: bool = True
    activation: str | None = None


@dataclass
class FrameAttn:
    """One CrossFrameAttention layer (layers.py:2283-2384): at every position the six frames are six tokens of
    ``channels``: pre-LN (eps 1e-6, :2321-2323) -> MultiHeadAttention(num_heads, key_dim = channels // num_heads,
    :2324-2330) over the frames -> residual (:2367); with ``use_ffn`` LN -> Dense(ff_dim, gelu) -> Dense(channels) ->
    residual (:2370-2376).  The layer does not set supports_masking: no mask leaves it."""
    name: str
    channels: int
    heads: int
    key_dim: int
    ff_dim: int
    use_ffn: bool = True           # layers.py:2310


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


@dataclass
class LocalAttn:
    """One LocalAttention layer (layers.py:2520-2645): windowed self-attention along the length axis inside every frame
    row, ``blocks`` times: pre-LN (eps 1e-6, :2556-2558) -> MultiHeadAttention(num_heads, key_dim = channels //
    num_heads, :2559-2564) under the mask ``|q - k| <= half_window and mask[k]`` (:2579-2585, :2604-2609) -> residual
    (:2619); LN -> Dense(ff_dim, gelu) -> Dense(channels) -> residual (:2621-2623), always present.  The layer sets
    supports_masking and ``compute_mask`` returns the mask (:2550, :2627-2628): the mask stays behind it."""
    name: str
    channels: int
    heads: int
    key_dim: int
    ff_dim: int
    half_window: int               # window_size // 2 (:2581)
    blocks: int = 1                # num_blocks (:2538)


_LOCALATTN_REQUIRED = ("embed_dim", "num_heads", "feed_forward_dim", "window_size")   # no defaults (layers.py:2531-2537)


@dataclass
class LengthAttn:
    """One stand-alone TransformerEncoder layer (layers.py:2206-2280) with ``attention_axes = 2``: full self-attention
    along the length axis inside every frame row - pre-LN (eps 1e-6, :2224-2226) -> MultiHeadAttention(num_heads, key_dim
    = channels // num_heads, :2227-2233) under Keras 3's implicit query / value masks -> residual (:2256); LN ->
    Dense(ff_dim, gelu) -> Dense(channels) -> residual (:2259-2264).  The layer does not set supports_masking: no mask
    leaves it."""
    name: str
    channels: int
    heads: int
    key_dim: int
    ff_dim: int


@dataclass
class AxialAttn:
    """One AxialAttention layer (layers.py:2400-2517): per block a TransformerEncoder along the length (:2461-2470), a
    CrossFrameAttention with its feed-forward half (:2474-2483), the post norm and the residual add of the block's input
    (:2485-2501).  Only block 0's encoder sees the layer's incoming mask; ``masked_layernorm`` / ``masked_dyt`` post norms
    get it in every block (:2495-2496).  The layer sets supports_masking (:2442): the mask stays behind it."""
    name: str
    channels: int
    heads: int
    key_dim: int
    ff_dim: int
    blocks: int = 1                # num_blocks (:2426)
    norm_type: str = "layernorm"   # :2428 (layernorm | masked_layernorm | masked_dyt | masked_batchnorm)
    epsilon: float = 1e-6          # of the post norm only (:2427); the encoders' layer norms have 1e-6 hard-coded
    alpha_init: float = 0.5        # MaskedDYT's initial alpha (:2429): training only, the weights carry alpha

    def post_norm(self, block: int) -> Norm:
        """The post norm of block ``block`` as a :class:`Norm` (``layernorm`` has masked_layernorm's variables)."""
        kind = "masked_layernorm" if self.norm_type == "layernorm" else self.norm_type
        return Norm(f"{self.name}/block{block}/post_norm", kind, self.channels, self.epsilon, True)

    def length(self, block: int) -> LengthAttn:
        return LengthAttn(f"{self.name}/block{block}/length", self.channels, self.heads, self.key_dim, self.ff_dim)

    def frame(self, block: int) -> FrameAttn:
        return FrameAttn(f"{self.name}/block{block}/frame", self.channels, self.heads, self.key_dim, self.ff_dim, True)


_ATTN_REQUIRED = ("embed_dim", "num_heads", "feed_forward_dim")                    # no defaults (layers.py:2207-2212, :2420-2425)
# the constructors' own arguments plus what keras.layers.Layer.__init__ takes: any other key is an unknown keyword there
_AXIAL_KEYS = {"embed_dim", "num_heads", "feed_forward_dim", "dropout_rate", "num_blocks", "epsilon", "norm_type",
               "alpha_init", "name", "dtype", "trainable"}
_ENCODER_KEYS = {"embed_dim", "num_heads", "feed_forward_dim", "dropout_rate", "attention_axes", "name", "dtype", "trainable"}
AXIAL_NORM_TYPES = ("layernorm", "masked_layernorm", "masked_dyt", "masked_batchnorm")


@dataclass
class Hyena:
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


#: what the hyena kernels (csrc/jg_hyena.hip) and the host's filter table (program.py) cover
HYENA_CHANNELS = (16, 32, 64)
HYENA_MAX_ORDER = 4
HYENA_PE_DIM = 16                  # HyenaFilter's pe_dim default (:2797); HyenaOperator never passes another
HYENA_ACTIVATIONS = ("gelu", "sin", "relu", "tanh", "sigmoid", "silu", "swish", "linear")
# the constructor's own arguments (:3047-3059) plus what keras.layers.Layer.__init__ takes; kernel_regularizer_w is the
# builder's spelling of the regulariser's weight
_HYENA_KEYS = {"dim", "seq_len", "order", "filter_hidden", "filter_layers", "filter_activation", "dropout",
               "output_projection", "filter_normalize", "kernel_regularizer", "kernel_regularizer_w", "name", "dtype",
               "trainable"}


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


@dataclass
class BiLstm:
    """One MaskedBiLSTM (layers.py:1335-1430) on the rows of the (frames, length, channels) tensor: Keras 3
    ``Bidirectional(LSTM(units, return_sequences=True), merge_mode="concat")`` under the incoming mask - a masked step keeps
    both states and repeats the direction's previous output (zeros while no valid step has come) - or, with ``ignore_mask``,
    under none.  ``compute_mask`` returns the mask, or None with ``ignore_mask`` (:1405-1410)."""
    name: str
    cin: int
    units: int
    ignore_mask: bool = False      # :1361

    @property
    def channels(self) -> int:
        """What the layer leaves: the two directions side by side."""
        return 2 * self.units


#: what the kernel (csrc/jg_bilstm.hip) covers
BILSTM_UNITS = (16, 32, 64)
BILSTM_MAX_CHANNELS = 128
# the constructor's own arguments (:1354-1363) plus what keras.layers.Layer.__init__ takes
_BILSTM_KEYS = {"units", "dropout", "recurrent_dropout", "return_sequences", "use_cudnn", "ignore_mask", "name", "dtype",
                "trainable"}


def bilstm_limit(channels: int, units: int) -> str | None:
    """Why the bilstm kernel cannot run this layer, or None."""
    if units not in BILSTM_UNITS:
        return f"units {units} (the kernel covers {' / '.join(map(str, BILSTM_UNITS))} units)"
    if channels % 16 or not 16 <= channels <= BILSTM_MAX_CHANNELS:
        return f"{channels} incoming channels (a multiple of 16 up to {BILSTM_MAX_CHANNELS})"
    return None


@dataclass
class MultiScaleConv:
    """One MultiScaleConv1D (layers.py:1433-1595): ``len(branches)`` MaskedConv1Ds over the same rows of the (frames, length,
    channels) tensor, every one with padding "same" and strides 1 (:1504-1505, :1517-1526) and its own kernel_size,
    dilation_rate, activation, use_bias and mask_mode; their outputs concatenated along the channels (``merge`` "concat") or
    summed in branch order (``merge`` "add", tf.add_n; :1539-1542).  The mask behind the layer is the AND of the branches'
    output masks (:1544-1548), none where the branches do not mask or no mask arrives."""
    name: str
    cin: int
    merge: str                     # "concat" | "add" (:1448)
    branches: list                 # list[Conv], named <name>/branch<b>

    @property
    def channels(self) -> int:
        """What the layer leaves: the branches side by side, or their common width."""
        return sum(b.filters for b in self.branches) if self.merge == "concat" else self.branches[0].filters

    @property
    def use_masking(self) -> bool:
        return self.branches[0].use_masking


#: what the kernel (csrc/jg_msconv.hip) covers
MSCONV_MAX_BRANCHES = 4
MSCONV_MAX_CHANNELS = 128
MSCONV_MAX_KERNEL = 15
MSCONV_MAX_SPAN = 64
# the constructor's own arguments (:1445-1453); the last three matter in training only
_MSCONV_KEYS = {"branches", "merge", "use_bias", "kernel_initializer", "kernel_regularizer", "kernel_regularizer_w"}
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
class Branch:
    """One entry of ``parallel_branches.branches``: a block of its own on the layer's input (builder.py:1116-1122)."""
    layers: list                   # the compiled ``hidden_layers``, named <name>/branch<b>/<j>
    pooling: str                   # "max" | "average" | "last"
    channels: int                  # what the branch's pooled vector holds


@dataclass
class ParallelBranches:
    """One ``parallel_branches`` entry (builder.py:1109-1153): every branch a recursive ``_build_block`` on the same tensor
    under the same mask, with ``nmd_merge=None`` and a tuple result cut to its first element - NMD taps inside a branch are
    built and dropped -; the branch outputs merged in branch order: ``concat`` along the channels, ``sum`` (Add: a running
    sum), ``average`` (Average: that sum divided by the number of branches), ``max`` (Maximum: a running maximum).  Here every
    branch pools, so the layer leaves a (B, C) vector: it closes the representation learner, whose own pooling is null."""
    name: str
    merge: str                     # "concat" | "sum" | "average" | "max"
    branches: list                 # list[Branch]

    @property
    def channels(self) -> int:
        """The merged width: the branches side by side, or their common width."""
        return sum(b.channels for b in self.branches) if self.merge == "concat" else self.branches[0].channels


#: what the pool-and-merge op (csrc/jg_poolvec.hip) covers
BRANCHES_MAX = 4
BRANCHES_MAX_WIDTH = 1024          # floats of the merged vector: the pool kernels' limit, inside what the dense kernels read
BRANCH_MERGES = ("concat", "sum", "average", "max")
_POOLINGS = {"max": "max", "masked_max": "max", "average": "average", "masked_average": "average", "last": "last",
             "masked_last": "last"}                                          # builder.py:1703-1712
_BRANCHES_KEYS = {"merge", "branches"}                                       # what builder.py:1110-1111 reads
_BRANCH_KEYS = {"hidden_layers", "pooling"}                                  # what _build_block reads (:1007, :1169)


class _DropTaps:
    """``_block``'s ``nmd_dims`` where the reference builds NMD taps and drops them (inside a ``parallel_branches`` branch,
    and in front of one that closes the block: builder.py:1124-1125, :1169-1193): ``nmd`` layers vanish, ``return_nmd`` norms
    and blocks compute what they compute without the side output."""


DROP_TAPS = _DropTaps()


def _constructor_accepts(cfg: dict, keys: set) -> bool:
    """Whether the reference's constructor would take this config: the three required arguments are there and no key is
    an unknown keyword (keras.layers.Layer.__init__ raises on one)."""
    return all(k in cfg for k in _ATTN_REQUIRED) and not set(cfg) - keys


@dataclass
class ModelPlan:
    vocab: int
    embedding_dim: int
    rep: list[Any]
    pooling: str | None            # "max" | "average" | "last"; None: the last rep layer is a parallel_branches of pooled branches
    rep_channels: int
    classifier: list[Any]
    n_classes: int
    nmd_dims: list[int] = field(default_factory=list)
    reliability: list[Any] | None = None
    reliability_mode: str = "nmd"
    reliability_signals: list[str] = field(default_factory=list)
    use_masking: bool = True
    string_processor: dict = field(default_factory=dict)
    class_label_map: list[dict] = field(default_factory=list)
    # "embedding" = Embedding(vocab, E, mask_zero) on ids; "onehot_dense" = one-hot input -> Masking(0) -> bias-free
    # Dense(E); "onehot" = the one-hot rows themselves (embedding_size 0) (builder.py:844-880).  The one-hot forms
    # are the same gather with table row 0 = zeros (the all-zero one-hot row of an invalid codon, masked by Masking)
    embedding_kind: str = "embedding"
    # input_type "nucleotide" (builder.py:881-882): a (2, L, 4) one-hot input whose two strands run through ONE
    # shared-weight branch each - representation learner and classifier head - and are merged behind the head
    # (builder.py:488-494, :563-590, :1195-1266).  strands > 1 marks such a plan; merge = the classifier's merge method
    strands: int = 1
    merge: str = "average"
    # NMDMerge (nnlib/v2/nmd.py:93-170) over two or more NMD vectors: None / "concat" = the vectors side by side; "sum" /
    # "mean" / "max" / "weighted" = every vector through its own bias-free Dense(nmd_merge_dim) first
    # (rep/nmd_merge/proj_<i>/kernel; "weighted": + rep/nmd_merge/layer_weights, softmax-ed), then combined
    nmd_merge_mode: str = "concat"
    nmd_merge_dim: int = 0
    nmd_merge_act: str | None = None        # projection_kwargs.activation of the projections (round 6), None = linear
    # use_positional_embeddings (builder.py:886-892): SinusoidalPositionEmbedding(max_wavelength) rows (layers.py:2149-2195)
    # added to the embedded input; None = none
    positional_wavelength: float | None = None

    @property
    def nmd_raw_dim(self) -> int:
        """Width of the NMD vectors side by side (what the taps write)."""
        return sum(self.nmd_dims)

    @property
    def nmd_dim(self) -> int:
        """Width of the model's ``nmd`` output (what the reliability head reads)."""
        return self.nmd_merge_dim if self.nmd_merge_mode != "concat" else sum(self.nmd_dims)


def _norm(name: str, kind: str, channels: int, cfg: dict, use_masking: bool) -> Norm:
    if cfg.get("return_nmd") and kind != "masked_batchnorm":
        # MaskedDYT / MaskedLayerNormalization raise on return_nmd=True (layers.py:307-311, 398-402)
        raise UnsupportedLayer(f"{name}: return_nmd=True is only defined for masked_batchnorm")
    eps = {"masked_batchnorm": 1e-5, "masked_layernorm": 1e-3, "masked_dyt": 0.0}[kind]
    return Norm(name, kind, channels, float(cfg.get("epsilon", eps)), use_masking)


def _block(layers: list[dict], prefix: str, cin: int, use_masking_default: bool,
           nmd_dims: list[int] | None, frames: int | None = None):
    """builder.py:982-1158: walk one ``hidden_layers`` list.  ``frames``: the frame axis of the tensor the list runs on
    (the representation learner of a translated model), None where there is none (heads, strand branches)."""
    out: list[Any] = []
    drop = nmd_dims is DROP_TAPS
    for i, layer in enumerate(layers):
        name = str(layer.get("name", "")).lower()
        cfg = dict(layer.get("config", {}) or {})
        p = f"{prefix}/{i}"
        if out and isinstance(out[-1], ParallelBranches) and name != "dropout":
            raise UnsupportedLayer(f"{p}: layer {name!r} behind a parallel_branches of pooled branches (the merged (B, C) vector "
                                   "goes to the heads: only dropout may follow)")
        if name == "conv1d":
            # tf.keras.layers.Conv1D (builder.py:280): strides 1, padding "valid", dilation 1, bias, no activation, and no
            # mask handling of its own - an incoming Keras mask is dropped
            out.append(Conv(p, int(cfg["kernel_size"]), cin, int(cfg["filters"]), int(cfg.get("strides", 1)),
                            str(cfg.get("padding", "valid")).lower(), int(cfg.get("dilation_rate", 1)),
                            bool(cfg.get("use_bias", True)), cfg.get("activation"), False, "any"))
            if out[-1].padding not in ("valid", "same"):
                raise UnsupportedLayer(f"{p}: conv1d padding {out[-1].padding!r}")
            cin = int(cfg["filters"])
        elif name == "masked_conv1d":
            um = bool(cfg.get("use_masking", use_masking_default))   # builder.py:1019-1020
            mode = cfg.get("mask_mode", "any")
            if mode not in ("any", "majority", "strict"):
                raise ValueError(f"{p}: invalid mask_mode {mode!r}")
            out.append(Conv(p, int(cfg["kernel_size"]), cin, int(cfg["filters"]),
                            int(cfg.get("strides", 1)), str(cfg.get("padding", "valid")).lower(),
                            int(cfg.get("dilation_rate", 1)), bool(cfg.get("use_bias", True)),
                            cfg.get("activation"), um, mode))
            cin = int(cfg["filters"])
        elif name in _NORMS:
            um = bool(cfg.get("use_masking", use_masking_default)) if name == "masked_batchnorm" else True
            norm = _norm(p, name, cin, cfg, um)
            if cfg.get("return_nmd") and not drop:
                # MaskedBatchNorm(return_nmd=True) also returns the masked per-example channel mean of its INPUT
                # minus its own moving_mean (layers.py:943-954): an NMD tap in front of the norm that shares the
                # norm's moving_mean and epsilon
                if nmd_dims is None:
                    raise UnsupportedLayer(f"{p}: return_nmd norm outside the representation learner")
                out.append(Nmd(p, cin, norm.epsilon))
                nmd_dims.append(cin)
            out.append(norm)
        elif name == "nmd":
            if drop:
                continue                                        # built on the side and dropped: the tensor passes unchanged
            if nmd_dims is None:
                raise UnsupportedLayer(f"{p}: nmd layer outside the representation learner")
            out.append(Nmd(p, cin, float(cfg.get("epsilon", 1e-5))))
            nmd_dims.append(cin)
        elif name == "activation" or name in _ACT_ALIASES:
            kind = name if name in _ACT_ALIASES else cfg.get("activation")   # builder.py:1022-1023
            out.append(Act(str(kind).lower()))
        elif name == "residual_block":
            um = bool(cfg.get("use_masking", use_masking_default))
            filters = int(cfg["filters"])
            k = int(cfg.get("kernel_size", 3))                 # layers.py:1788
            stride = int(cfg.get("strides", 1))
            pad = str(cfg.get("padding", "same")).lower()      # layers.py:1790
            dil = int(cfg.get("dilation_rate", 1))
            bias = bool(cfg.get("use_bias", True))
            nt = str(cfg.get("norm_type", "masked_batchnorm")).lower()
            if nt not in _NORMS:
                raise UnsupportedLayer(f"{p}: norm_type {nt!r}")
            act = cfg.get("activation", "gelu")
            for j in range(int(cfg.get("block_size", 1))):
                bp = f"{p}/block{j}"
                # use_1x1conv only reaches the first block (layers.py:2677-2679)
                bypass = (bool(cfg.get("use_1x1conv", False)) and j == 0) or stride > 1
                c1 = Conv(f"{bp}/conv1", k, cin, filters, stride, pad, dil, bias, None, um, "any")
                c2 = Conv(f"{bp}/conv2", k, filters, filters, 1, pad, dil, bias, None, um, "any")
                c3 = b3 = None
                if bypass:
                    c3 = Conv(f"{bp}/conv3", 1, cin, filters, stride, pad, dil, bias, None, um, "any")
                    b3 = _norm(f"{bp}/bn3", nt, filters, {}, um)
                blk = ResBlock(bp, c1, _norm(f"{bp}/bn1", nt, filters, {}, um), c2,
                               _norm(f"{bp}/bn2", nt, filters, {}, um), c3, b3, act, um)
                if cfg.get("return_nmd") and j == int(cfg.get("block_size", 1)) - 1:   # layers.py:2682-2686
                    if nt != "masked_batchnorm":
                        raise ValueError(f"{p}: return_nmd=True is only supported with norm_type='masked_batchnorm'")
                    if nmd_dims is None:
                        raise UnsupportedLayer(f"{p}: return_nmd block outside the representation learner")
                    if not drop:
                        blk.nmd = Nmd(f"{bp}/bn2", filters, blk.bn2.epsilon)
                        nmd_dims.append(filters)
                out.append(blk)
                cin = filters
        elif name == "dense":
            out.append(Dense(p, cin, int(cfg["units"]), bool(cfg.get("use_bias", True)),
                             cfg.get("activation")))
            cin = int(cfg["units"])
        elif name == "dropout":
            continue                                            # identity at inference
        elif name == "cross_frame_attention":
            # builder.py:1155: CrossFrameAttention(**config) (embed_dim, num_heads, feed_forward_dim, dropout_rate, use_ffn);
            # :1165-1166: previous_channels = embed_dim
            if frames is None:
                raise UnsupportedLayer(f"{p}: cross_frame_attention needs the (frames, length, channels) tensor of the "
                                       "representation learner: not supported in a head or on a strand branch")
            if frames != 6:
                raise UnsupportedLayer(f"{p}: cross_frame_attention over {frames} frames (the kernel attends over the six "
                                       "reading frames of a translated window)")
            c, h = int(cfg["embed_dim"]), int(cfg["num_heads"])
            use_ffn = bool(cfg.get("use_ffn", True))
            f = int(cfg["feed_forward_dim"]) if use_ffn else 0
            if c != cin:
                raise UnsupportedLayer(f"{p}: embed_dim {c} != {cin} incoming channels (the layer's residual adds them, "
                                       "layers.py:2367)")
            why = attn_limit(FRAMEATTN, c, h, f)
            if why is not None:
                raise UnsupportedLayer(f"{p}: cross_frame_attention with {why}")
            out.append(FrameAttn(p, c, h, c // h, f, use_ffn))
        elif name == "local_attention" and all(k in cfg for k in _LOCALATTN_REQUIRED):
            # builder.py:290, :1155: LocalAttention(**config) (embed_dim, num_heads, feed_forward_dim, window_size,
            # dropout_rate, num_blocks); an entry without one of the four required arguments raises in the reference's
            # constructor and falls through to the generic refusal below
            if frames is None:
                raise UnsupportedLayer(f"{p}: local_attention needs the (frames, length, channels) tensor of the "
                                       "representation learner: not supported in a head or on a strand branch")
            c, h, f = int(cfg["embed_dim"]), int(cfg["num_heads"]), int(cfg["feed_forward_dim"])
            window, blocks = int(cfg["window_size"]), int(cfg.get("num_blocks", 1))
            if window < 1:
                raise UnsupportedLayer(f"{p}: local_attention window_size {window} (must be positive, layers.py:2542-2543)")
            if blocks < 1:
                raise UnsupportedLayer(f"{p}: local_attention num_blocks {blocks} (at least one block)")
            if c != cin:
                raise UnsupportedLayer(f"{p}: embed_dim {c} != {cin} incoming channels (the layer's residual adds them, "
                                       "layers.py:2619)")
            why = attn_limit(LOCALATTN, c, h, f, window // 2)
            if why is not None:
                raise UnsupportedLayer(f"{p}: local_attention with {why}")
            out.append(LocalAttn(p, c, h, c // h, f, window // 2, blocks))
        elif (name == "transformer_encoder" and _constructor_accepts(cfg, _ENCODER_KEYS)) or \
                (name == "axial_attention" and _constructor_accepts(cfg, _AXIAL_KEYS)):
            # builder.py:1155: TransformerEncoder(**config) / AxialAttention(**config); an entry the constructor would not
            # take (a required argument missing, an unknown keyword) falls through to the generic refusal below
            if frames is None:
                raise UnsupportedLayer(f"{p}: {name} needs the (frames, length, channels) tensor of the "
                                       "representation learner: not supported in a head or on a strand branch")
            c, h, f = int(cfg["embed_dim"]), int(cfg["num_heads"]), int(cfg["feed_forward_dim"])
            if c != cin:
                raise UnsupportedLayer(f"{p}: embed_dim {c} != {cin} incoming channels (the layer's residual adds them, "
                                       "layers.py:2256)")
            why = attn_limit(LENGTHATTN, c, h, f)
            if why is not None:
                raise UnsupportedLayer(f"{p}: {name} with {why}")
            if name == "transformer_encoder":
                axes = cfg.get("attention_axes", 2)
                if axes != 2 and list(axes if isinstance(axes, (list, tuple)) else [axes]) != [2]:
                    raise UnsupportedLayer(f"{p}: transformer_encoder attention_axes {axes!r} (the kernel attends along the "
                                           "length axis, attention_axes = 2)")
                out.append(LengthAttn(p, c, h, c // h, f))
            else:
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
                why = attn_limit(FRAMEATTN, c, h, f)
                if why is not None:
                    raise UnsupportedLayer(f"{p}: axial_attention with {why} (its frame half)")
                out.append(AxialAttn(p, c, h, c // h, f, blocks, nt, float(cfg.get("epsilon", 1e-6)),
                                     float(cfg.get("alpha_init", 0.5))))
        elif name == "hyena_block" and "dim" in cfg and not set(cfg) - _HYENA_KEYS:
            # builder.py:1155: HyenaBlock(**config); an entry without `dim` or with an unknown keyword raises in the reference's
            # constructor and falls through to the generic refusal below.  dropout and the regulariser matter in training only
            if frames is None:
                raise UnsupportedLayer(f"{p}: hyena_block needs the (frames, length, channels) tensor of the "
                                       "representation learner: not supported in a head or on a strand branch")
            c, order = int(cfg["dim"]), int(cfg.get("order", 2))
            if c != cin:
                raise UnsupportedLayer(f"{p}: dim {c} != {cin} incoming channels (the layer's residual adds them, "
                                       "layers.py:3129)")
            fl, act = int(cfg.get("filter_layers", 2)), cfg.get("filter_activation", "gelu")
            why = hyena_limit(c, order, fl, act)
            if why is not None:
                raise UnsupportedLayer(f"{p}: hyena_block with {why}")
            seq_len = cfg.get("seq_len")
            if seq_len is not None and int(seq_len) < 1:
                raise UnsupportedLayer(f"{p}: hyena_block seq_len {seq_len} (a positive number of positions, or none)")
            nxt = layers[i + 1] if i + 1 < len(layers) else {}
            if not drop and (str(nxt.get("name", "")).lower() == "nmd" or (nxt.get("config") or {}).get("return_nmd")):
                raise UnsupportedLayer(f"{p}: an nmd tap directly behind hyena_block is not supported "
                                       "(the op's store carries no partial sums)")
            out.append(Hyena(p, c, order, int(cfg.get("filter_hidden", 32)), fl,
                             None if act is None or str(act).lower() == "linear" else str(act).lower(),
                             bool(cfg.get("filter_normalize", False)), bool(cfg.get("output_projection", False)),
                             None if seq_len is None else int(seq_len)))
        elif name == "masked_bilstm" and "units" in cfg and not set(cfg) - _BILSTM_KEYS:
            # builder.py:282, :1155: MaskedBiLSTM(**config); an entry without `units` or with an unknown keyword raises in the
            # reference's constructor and falls through to the generic refusal below.  dropout / recurrent_dropout matter in
            # training only, use_cudnn changes no formula
            if frames is None:
                raise UnsupportedLayer(f"{p}: masked_bilstm needs the (frames, length, channels) tensor of the "
                                       "representation learner: not supported in a head or on a strand branch")
            if not bool(cfg.get("return_sequences", True)):
                raise UnsupportedLayer(f"{p}: masked_bilstm with return_sequences: false (the tensor loses its length axis, "
                                       "and no layer behind it here takes a (frames, channels) tensor)")
            units = int(cfg["units"])
            why = bilstm_limit(cin, units)
            if why is not None:
                raise UnsupportedLayer(f"{p}: masked_bilstm with {why}")
            nxt = layers[i + 1] if i + 1 < len(layers) else {}
            if not drop and (str(nxt.get("name", "")).lower() == "nmd" or (nxt.get("config") or {}).get("return_nmd")):
                raise UnsupportedLayer(f"{p}: an nmd tap directly behind masked_bilstm is not supported "
                                       "(the op's store carries no partial sums)")
            out.append(BiLstm(p, cin, units, bool(cfg.get("ignore_mask", False))))
            cin = 2 * units
        elif name == "multi_scale_conv" and "branches" in cfg and not set(cfg) - _MSCONV_KEYS:
            # builder.py:277-304, :1155: MultiScaleConv1D(**config); an entry without `branches` or with a key that is none of
            # the constructor's arguments raises there and falls through to the generic refusal below.  The initialiser and
            # the regulariser matter in training only
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
            if frames is None:
                raise UnsupportedLayer(f"{p}: multi_scale_conv needs the (frames, length, channels) tensor of the "
                                       "representation learner: not supported in a head or on a strand branch")
            if len({c.use_masking for c in convs}) != 1:
                raise UnsupportedLayer(f"{p}: multi_scale_conv whose branches disagree on use_masking (the reference ANDs a "
                                       "branch's mask with None there, layers.py:1544-1548)")
            why = msconv_limit(cin, merge, convs)
            if why is not None:
                raise UnsupportedLayer(f"{p}: multi_scale_conv with {why}")
            nxt = layers[i + 1] if i + 1 < len(layers) else {}
            if not drop and (str(nxt.get("name", "")).lower() == "nmd" or (nxt.get("config") or {}).get("return_nmd")):
                raise UnsupportedLayer(f"{p}: an nmd tap directly behind multi_scale_conv is not supported "
                                       "(the op's store carries no partial sums)")
            # builder.py:1161-1166 does not update previous_channels behind this layer (the entry has no top-level `filters`),
            # so a residual_block that follows is constructed with a stale `shape` (:1075-1087).  That argument reaches
            # ResidualBlockStack.__init__ as `in_shape` and is never read (layers.py:2658-2692, :2716-2721): the blocks build
            # from the tensor they are called on.  The graph is the same, so such a block is accepted
            out.append(MultiScaleConv(p, cin, merge, convs))
            cin = out[-1].channels
        elif name == "parallel_branches":
            out.append(_parallel_branches(p, cfg, cin, use_masking_default, nmd_dims, frames))
            cin = out[-1].channels
        else:
            raise UnsupportedLayer(
                f"{p}: layer {name!r} is outside the Conv1D -> norm -> pool -> dense family "
                "the MI355X engine implements")
    return out, cin


def _parallel_branches(p: str, cfg: dict, cin: int, use_masking_default: bool, nmd_dims, frames: int | None) -> ParallelBranches:
    """builder.py:1109-1153.  The reference's two ValueErrors keep their wording; what Keras' merge layers refuse is a
    ValueError too; what this engine does not run is an UnsupportedLayer with the reason."""
    merge = str(cfg.get("merge", "concat")).lower()
    branch_cfgs = cfg.get("branches", [])
    if not branch_cfgs:
        raise ValueError("parallel_branches requires at least one branch")                               # :1112-1113
    if merge not in BRANCH_MERGES:
        raise ValueError(f"Unknown parallel_branches merge method: {merge}")                             # :1143-1145
    if nmd_dims is None or frames is None:
        raise UnsupportedLayer(f"{p}: parallel_branches needs the (frames, length, channels) tensor of the representation "
                               "learner: not supported in a head or on a strand branch")
    if set(cfg) - _BRANCHES_KEYS:
        raise UnsupportedLayer(f"{p}: parallel_branches keys {sorted(set(cfg) - _BRANCHES_KEYS)} (the builder reads "
                               f"{' / '.join(sorted(_BRANCHES_KEYS))})")
    if not isinstance(branch_cfgs, list) or not all(isinstance(b, dict) for b in branch_cfgs):
        raise UnsupportedLayer(f"{p}: parallel_branches branches must be a list of blocks (hidden_layers, pooling)")
    if len(branch_cfgs) > BRANCHES_MAX:
        raise UnsupportedLayer(f"{p}: parallel_branches with {len(branch_cfgs)} branches (up to {BRANCHES_MAX})")
    pooled = [b.get("pooling") is not None for b in branch_cfgs]
    if any(pooled) and not all(pooled):
        raise UnsupportedLayer(f"{p}: parallel_branches that mixes pooled and unpooled branches (a (B, C) vector cannot be "
                               "merged with a (B, frames, L, C) tensor)")
    branches = []
    for b, bcfg in enumerate(branch_cfgs):
        bp = f"{p}/branch{b}"
        if set(bcfg) - _BRANCH_KEYS:
            raise UnsupportedLayer(f"{bp}: branch keys {sorted(set(bcfg) - _BRANCH_KEYS)} (a branch is a block of "
                                   f"{' / '.join(sorted(_BRANCH_KEYS))})")
        if bcfg.get("pooling") is None:
            raise UnsupportedLayer(f"{bp}: a branch without pooling is not supported (the mask of the merged tensor is decided "
                                   "by Keras' merge layers, whose rule could not be pinned here)")
        raw = str(bcfg["pooling"]).lower()
        if "gated" in raw:
            raise UnsupportedLayer(f"{bp}: pooling {raw!r} in a branch is not supported (its gate output has no place in a merge)")
        if raw not in _POOLINGS:
            raise UnsupportedLayer(f"{bp}: pooling {raw!r} is not supported (max / average / last)")
        hidden = bcfg.get("hidden_layers", []) or []
        if any(str(l.get("name", "")).lower() == "parallel_branches" for l in hidden):
            raise UnsupportedLayer(f"{bp}: a nested parallel_branches is not supported")
        layers, width = _block(hidden, bp, cin, use_masking_default, DROP_TAPS, frames=frames)
        if width % 4:
            raise UnsupportedLayer(f"{bp}: a branch of {width} channels (a multiple of 4: a lane of the pool kernel owns four)")
        branches.append(Branch(layers, _POOLINGS[raw], width))
    if merge != "concat" and len({b.channels for b in branches}) != 1:
        # keras.layers.Add / Average / Maximum: "Inputs have incompatible shapes"
        raise ValueError(f"{p}: parallel_branches merge {merge!r} over branches of unequal width "
                         f"{[b.channels for b in branches]} (Inputs have incompatible shapes)")
    node = ParallelBranches(p, merge, branches)
    if node.channels > BRANCHES_MAX_WIDTH:
        raise UnsupportedLayer(f"{p}: parallel_branches leaves {node.channels} channels (up to {BRANCHES_MAX_WIDTH}: the width of "
                               "the vector slot the pool kernels fill and the dense kernels read)")
    return node


def resolve_string_processor(model_cfg: dict) -> dict:
    """``InferModel._load_string_processor_config`` (nnlib/inference.py:423-483)."""
    cfg = dict(model_cfg.get("embedding", {}) or {})
    cfg.update(model_cfg.get("string_processor", {}) or {})
    cfg["input_type"] = cfg.get("type", "translated")          # inference.py:443-444
    if cfg.get("codon") is not None and cfg.get("codon_id") is not None:
        codon_name, id_name = cfg["codon"], cfg["codon_id"]
        cfg["codon"] = maps.NAMED_MAPS.get(codon_name)
        cfg["codon_id"] = maps.NAMED_MAPS.get(id_name)
        if cfg["codon"] is None or cfg["codon_id"] is None:
            raise UnsupportedLayer(f"codon map {codon_name!r}/{id_name!r} is not supported")
        cfg["codon_depth"] = max(cfg["codon_id"]) + 1
        cfg["vocab_size"] = len(cfg["codon_id"]) + 1
        cfg["ngram_width"] = int(math.log(len(cfg["codon"]), 4))
        shape = (model_cfg.get("embedding", {}) or {}).get("input_shape")
        if cfg.get("seq_onehot") is None and shape is not None:
            cfg["seq_onehot"] = len(shape) == 3 and shape[-1] is not None and shape[-1] > 1
        cfg["seq_onehot"] = cfg.get("seq_onehot", False)
        if cfg["seq_onehot"] is False:
            cfg["codon_depth"] = 1
    if "crop_size" in cfg:
        size = cfg["crop_size"]
        units = cfg.setdefault("crop_units", "nucleotide" if cfg["input_type"] == "nucleotide" else "codon")
        if cfg["input_type"] == "nucleotide":
            cfg["crop_size_nt"] = int(size)
        elif units == "codon":                                  # seqops/crop.py:70-89
            cfg["crop_size_codons"], cfg["crop_size_nt"] = int(size), 3 * int(size) + 5
        else:
            cfg["crop_size_codons"], cfg["crop_size_nt"] = (int(size) - 5) // 3, int(size)
    return cfg


def build_plan(model_cfg: dict) -> ModelPlan:
    """Resolve the ``model:`` section of a project YAML into a :class:`ModelPlan`."""
    sp = resolve_string_processor(model_cfg)
    emb = model_cfg.get("embedding")
    if emb is None:
        raise ValueError("Missing 'embedding' section in config")   # builder.py:476
    graph_input = str(emb.get("input_type", "translated")).lower()      # what the builder builds (builder.py:846,854-884)
    branched = ["branch" in (model_cfg.get(section) or {}) for section in ("representation_learner", "classifier")]
    if graph_input == "nucleotide" or any(branched):
        return _build_strand_plan(model_cfg, sp, graph_input, branched)
    use_emb = bool(emb.get("use_embedding_layer", False))
    if use_emb == bool(sp.get("seq_onehot")):
        # Embedding needs ids, the Dense / pass-through branch needs one-hot rows (builder.py:856-880)
        raise UnsupportedLayer("use_embedding_layer and seq_onehot must be opposite (ids -> Embedding, one-hot -> Dense)")
    positional = None
    if emb.get("use_positional_embeddings", False):
        # builder.py:886-892: x = Add()([x, SinusoidalPositionEmbedding(max_wavelength=positional_embedding_length)(x)])
        positional = emb.get("positional_embedding_length")
        if not positional or float(positional) <= 0:
            raise ValueError("use_positional_embeddings needs embedding.positional_embedding_length (the max_wavelength)")
        positional = float(positional)
    if sp["input_type"] != "translated":
        raise UnsupportedLayer(f"input_type {sp['input_type']!r} on a graph built for translated input")
    if sp.get("ngram_width", 3) not in (3, 6):
        raise UnsupportedLayer(f"n-gram width {sp.get('ngram_width')} (codons: 3, dicodons: 6)")
    if sp.get("ngram_width", 3) == 6:
        # codon: DICODON (nnlib/inference.py:430-451 -> ngram_width 6, commands/predict.py:224, seqops/encode.py:272-284): ids
        # of 4 096 codon pairs, 16-bit on the device; an Embedding lookup runs as an op of its own in front of the first conv
        if sp["codon_id"] != maps.DICODON_ID or sp["codon"] != maps.DICODONS:
            raise UnsupportedLayer("6-gram encodings other than DICODON / DICODON_ID")
    if "projection" in model_cfg:
        pass  # training-only head, not part of the serving graph outputs
    use_masking = bool(model_cfg.get("use_masking", True))          # builder.py:259
    e = int(emb.get("embedding_size", 4))
    kind = "embedding"
    if not use_emb:
        depth = max(sp["codon_id"]) + 1                        # one_hot depth (seqops/encode.py:297-302)
        kind = "onehot_dense" if e > 0 else "onehot"
        e = e if e > 0 else depth
        sp["vocab_size"] = depth + 1                           # ids on the device: 0 = invalid / padding, id + 1 else
    nmd_dims: list[int] = []
    rep_cfg = model_cfg["representation_learner"]
    frames = int((emb.get("input_shape") or [None])[0] or emb.get("frames", 6))   # the graph input is input_shape (builder.py:846)
    hidden = rep_cfg.get("hidden_layers", [])
    # a parallel_branches of pooled branches closes the block with `pooling: null`, and _build_block then returns the tensor
    # alone (builder.py:1169-1193): the taps in front of the branches are dropped too, the model has no nmd output
    closes = any(str(l.get("name", "")).lower() == "parallel_branches" for l in hidden)
    rep, rep_c = _block(hidden, "rep", e, use_masking, DROP_TAPS if closes else nmd_dims, frames=frames)
    if rep and isinstance(rep[-1], ParallelBranches):
        if rep_cfg.get("pooling") is not None:
            raise ValueError(f"representation_learner.pooling {rep_cfg.get('pooling')!r} behind a parallel_branches of pooled "
                             "branches: the poolers take a (B, frames, L, C) tensor, the merge leaves (B, C) - pooling must be null")
        pooling = None
    else:
        pooling = str(rep_cfg.get("pooling", "")).lower()
        if pooling not in _POOLINGS:
            raise UnsupportedLayer(f"pooling {pooling!r} is not supported (max / average / last)")
        pooling = _POOLINGS[pooling]
    cls, n_cls = _block(model_cfg["classifier"].get("hidden_layers", []), "classifier", rep_c,
                        use_masking, None)
    plan = ModelPlan(vocab=sp["vocab_size"], embedding_dim=e, rep=rep, pooling=pooling,
                     rep_channels=rep_c, classifier=cls, n_classes=n_cls, nmd_dims=nmd_dims,
                     use_masking=use_masking, string_processor=sp,
                     class_label_map=list(model_cfg.get("class_label_map", []) or []), embedding_kind=kind,
                     positional_wavelength=positional)
    rel = model_cfg.get("reliability_model")
    if rel is not None and nmd_dims:
        merge = rel.get("merge") or {}
        if len(nmd_dims) > 1 and merge:                        # builder.py:1176-1180: NMDMerge(**merge) over the list
            mmode = merge.get("mode", "concat")
            if mmode not in ("concat", "sum", "mean", "max", "weighted"):
                raise ValueError(f"Unsupported NMD merge mode: {mmode}")          # nmd.py:110-111
            if merge.get("axis", -1) != -1:
                raise UnsupportedLayer("NMDMerge: only axis = -1 is supported")
            if mmode != "concat":
                target = merge.get("target_dim")
                if target is None:
                    if len(set(nmd_dims)) != 1:
                        raise ValueError(f"target_dim is required for merge mode '{mmode}' when NMD channel "
                                         f"dimensions differ.")                 # nmd.py:128-132
                    target = nmd_dims[0]
                pk = {k: v for k, v in (merge.get("projection_kwargs") or {}).items()
                      if not k.startswith("kernel_")}          # (initialisers / regularisers / constraints: training only)
                # Dense(target_dim, use_bias=False, name=..., **projection_kwargs) (nmd.py:133-141): `use_bias` or `units` here
                # would be a duplicate keyword in the reference; what is left that changes the graph is `activation`
                if set(pk) - {"activation"}:
                    raise UnsupportedLayer(f"NMDMerge projection_kwargs {sorted(set(pk) - {'activation'})} are not supported "
                                           f"(bias-free projections, optionally with an activation)")
                act = pk.get("activation")
                if act is not None and str(act).lower() not in (set(_ACT_ALIASES) | {"linear"}):
                    raise UnsupportedLayer(f"NMDMerge projection activation {act!r}")
                plan.nmd_merge_act = None if act is None or str(act).lower() == "linear" else str(act).lower()
                plan.nmd_merge_mode, plan.nmd_merge_dim = mmode, int(target)
        mode = rel.get("mode", "nmd")
        if mode not in ("nmd", "nmd_plus_signals"):
            raise ValueError(f"Unsupported reliability_model.mode: {mode!r}")   # builder.py:628-632
        sig = list(rel.get("signals", _DEFAULT_SIGNALS)) if mode == "nmd_plus_signals" else []
        rin = plan.nmd_dim + len(sig)
        expected = rel.get("input_shape")
        if expected is not None and expected != rin:
            raise ValueError(f"reliability_model.input_shape ({expected}) does not match computed "
                             f"reliability input dimension ({rin})")              # builder.py:662-667
        plan.reliability, _ = _block(rel.get("hidden_layers", []), "reliability", rin, use_masking, None)
        plan.reliability_mode = mode
        plan.reliability_signals = sig
    elif rel is not None:
        raise ValueError("reliability_model is configured but the representation learner "
                         "produced no NMD tensor")                                # builder.py:636-641
    return plan


def _build_strand_plan(model_cfg: dict, sp: dict, graph_input: str, branched: list[bool]) -> ModelPlan:
    """The branched nucleotide model (``train_config/nn_config_500bp_dvf.yaml``): ``embedding.input_type: nucleotide``
    makes the input the (2, L, 4) one-hot strands themselves (builder.py:881-882; ``Masking`` passes the values through
    and the first plain Keras layer drops its mask); ``representation_learner.branch`` is ONE ``_build_block`` model applied
    to each strand (:1195-1266, :488-494), ``classifier.branch`` one head applied to each strand's vector with a closing
    ``merge`` layer (:563-590); outputs ``prediction`` (merged) and ``embedding`` (Average of the strand vectors,
    :776-791); no reliability head.  Compiled as rows of ONE frame: a strand is a program row, ``strands`` rows make a
    window (program.py: ``OP_STRANDS``)."""
    emb = model_cfg["embedding"]
    if graph_input != "nucleotide" or not all(branched):
        raise UnsupportedLayer("a branched representation learner / classifier is supported for the two-strand "
                               "nucleotide model only (embedding.input_type: nucleotide, both sections branched)")
    if emb.get("use_embedding_layer", False) or emb.get("use_positional_embeddings", False):
        raise UnsupportedLayer("nucleotide input takes the one-hot strands as they are (no embedding layer)")
    strands = int((emb.get("input_shape") or [2])[0] or 2)
    if strands != 2:
        raise UnsupportedLayer(f"nucleotide input has two strands (input_shape[0] = {strands})")
    if model_cfg.get("reliability_model") is not None:
        raise UnsupportedLayer("reliability head on a branched model (the reference's combined model has none, builder.py:776-791)")
    if sp["input_type"] != "nucleotide":
        # nnlib/inference.py:443-444 reads embedding.type: without it the reference's engine hands the TRANSLATED tensor
        # to this nucleotide graph and exits; the graph decides here
        sp["input_type_note"] = ("embedding.type is not 'nucleotide': the reference's InferModel would feed "
                                 f"x[{sp['input_type']!r}] to this nucleotide graph (nnlib/inference.py:443-444)")
        sp["input_type"] = "nucleotide"
        if "crop_size" in sp:
            sp["crop_units"] = "nucleotide"
            sp["crop_size_nt"] = int(sp["crop_size"])
            sp.pop("crop_size_codons", None)
    sp["vocab_size"] = 5                                          # device ids: 0 = all-zero one-hot row, 1..4 = A, G, C, T
    rep_cfg = model_cfg["representation_learner"]["branch"]
    plain = {"conv1d", "dense", "dropout", "activation", "merge", *_ACT_ALIASES}   # stock Keras layers (builder.py:280-302)
    for section in ("representation_learner", "classifier"):
        for layer in model_cfg[section]["branch"].get("hidden_layers", []):
            if str(layer.get("name", "")).lower() not in plain:
                raise UnsupportedLayer(f"{section}.branch: layer {layer.get('name')!r} (a strand carries no mask and no "
                                       "frame axis: conv1d / activation / dense / dropout only)")
    rep, rep_c = _block(rep_cfg.get("hidden_layers", []), "rep", 4, False, None)
    if not rep or not isinstance(rep[0], Conv):
        raise UnsupportedLayer("the strand branch must start with a conv1d layer")
    pooling = {"max1d": "max1d", "average1d": "average1d"}.get(str(rep_cfg.get("pooling", "")).lower())
    if pooling is None:
        raise UnsupportedLayer(f"strand branch pooling {rep_cfg.get('pooling')!r} (max1d / average1d: builder.py:1706-1707)")
    hidden = list(model_cfg["classifier"]["branch"].get("hidden_layers", []))
    if not hidden or str(hidden[-1].get("name", "")).lower() != "merge":
        raise ValueError("Branched classifier must end with a 'merge' layer")           # builder.py:565-568
    merge = str((hidden[-1].get("config") or {}).get("method", "average")).lower()    # builder.py:569-570
    if merge not in ("average", "sum", "max", "concat"):
        raise ValueError(f"Unknown merge method: {merge}")                               # builder.py:1266
    cls, n_cls = _block(hidden[:-1], "classifier", rep_c, False, None)
    return ModelPlan(vocab=5, embedding_dim=4, rep=rep, pooling=pooling, rep_channels=rep_c, classifier=cls,
                     n_classes=n_cls, use_masking=False, string_processor=sp,
                     class_label_map=list(model_cfg.get("class_label_map", []) or []), embedding_kind="onehot",
                     strands=strands, merge=merge)


def flat_layers(seq):
    """The layers of ``seq`` with every ``parallel_branches`` replaced by its branches' layers, in branch order."""
    for layer in seq:
        if isinstance(layer, ParallelBranches):
            for b in layer.branches:
                yield from flat_layers(b.layers)
        else:
            yield layer


def weight_shapes(plan: ModelPlan) -> dict[str, tuple]:
    """Canonical variable names -> shapes."""
    out: dict[str, tuple] = {}
    if plan.embedding_kind == "embedding":
        out["embedding/embeddings"] = (plan.vocab, plan.embedding_dim)
    elif plan.embedding_kind == "onehot_dense":
        out["embedding/kernel"] = (plan.vocab - 1, plan.embedding_dim)      # Dense(E, use_bias=False) on one-hot rows

    def norm(n: Norm):
        vars_ = {"masked_batchnorm": ("gamma", "beta", "moving_mean", "moving_variance"),
                 "masked_dyt": ("alpha", "gamma", "beta"),
                 "masked_layernorm": ("gamma", "beta")}[n.kind]
        for v in vars_:
            out[f"{n.name}/{v}"] = (1,) if v == "alpha" else (n.channels,)

    def conv(c: Conv):
        out[f"{c.name}/kernel"] = (c.kernel_size, c.cin, c.filters)
        if c.use_bias:
            out[f"{c.name}/bias"] = (c.filters,)

    for seq in (plan.rep, plan.classifier, plan.reliability or []):
        for layer in flat_layers(seq):
            if isinstance(layer, Conv):
                conv(layer)
            elif isinstance(layer, Norm):
                norm(layer)
            elif isinstance(layer, Nmd):
                out[f"{layer.name}/moving_mean"] = (layer.channels,)
            elif isinstance(layer, ResBlock):
                for c in (layer.conv1, layer.conv2, layer.conv3):
                    if c is not None:
                        conv(c)
                for n in (layer.bn1, layer.bn2, layer.bn3):
                    if n is not None:
                        norm(n)
            elif isinstance(layer, Dense):
                out[f"{layer.name}/kernel"] = (layer.cin, layer.units)
                if layer.use_bias:
                    out[f"{layer.name}/bias"] = (layer.units,)
            elif isinstance(layer, FrameAttn):
                out.update(frame_attn_weight_shapes(layer))
            elif isinstance(layer, LocalAttn):
                out.update(local_attn_weight_shapes(layer))
            elif isinstance(layer, LengthAttn):
                out.update(length_attn_weight_shapes(layer))
            elif isinstance(layer, Hyena):
                out.update(hyena_weight_shapes(layer))
            elif isinstance(layer, BiLstm):
                out.update(bilstm_weight_shapes(layer))
            elif isinstance(layer, MultiScaleConv):
                out.update(msconv_weight_shapes(layer))
            elif isinstance(layer, AxialAttn):
                for j in range(layer.blocks):
                    out.update(length_attn_weight_shapes(layer.length(j)))
                    out.update(frame_attn_weight_shapes(layer.frame(j)))
                    norm(layer.post_norm(j))
        if seq is plan.rep and plan.nmd_merge_mode != "concat":                 # NMDMerge is built behind the rep block's layers
            for i, d in enumerate(plan.nmd_dims):
                out[f"rep/nmd_merge/proj_{i}/kernel"] = (d, plan.nmd_merge_dim)
            if plan.nmd_merge_mode == "weighted":
                out["rep/nmd_merge/layer_weights"] = (len(plan.nmd_dims),)
    return out


def frame_attn_weight_shapes(a: FrameAttn) -> dict[str, tuple]:
    """Keras variable shapes of one CrossFrameAttention layer: LayerNormalization gamma / beta (C); MultiHeadAttention
    query / key / value EinsumDense kernels (C, H, D) with biases (H, D), attention_output kernel (H, D, C) with bias (C);
    the two Dense layers of the feed-forward half."""
    c, h, d, f = a.channels, a.heads, a.key_dim, a.ff_dim
    out = {f"{a.name}/attn_norm/gamma": (c,), f"{a.name}/attn_norm/beta": (c,)}
    for part in ("query", "key", "value"):
        out[f"{a.name}/mha/{part}/kernel"] = (c, h, d)
        out[f"{a.name}/mha/{part}/bias"] = (h, d)
    out[f"{a.name}/mha/attention_output/kernel"] = (h, d, c)
    out[f"{a.name}/mha/attention_output/bias"] = (c,)
    if a.use_ffn:
        out.update({f"{a.name}/ffn_norm/gamma": (c,), f"{a.name}/ffn_norm/beta": (c,),
                    f"{a.name}/ffn_dense1/kernel": (c, f), f"{a.name}/ffn_dense1/bias": (f,),
                    f"{a.name}/ffn_dense2/kernel": (f, c), f"{a.name}/ffn_dense2/bias": (c,)})
    return out


def local_attn_weight_shapes(a: LocalAttn) -> dict[str, tuple]:
    """Keras variable shapes of one LocalAttention layer, per block ``<name>/block<j>/``: the two LayerNormalization
    layers' gamma / beta (C); MultiHeadAttention query / key / value EinsumDense kernels (C, H, D) with biases (H, D),
    attention_output kernel (H, D, C) with bias (C); the two Dense layers of the feed-forward half."""
    c, h, d, f = a.channels, a.heads, a.key_dim, a.ff_dim
    out: dict[str, tuple] = {}
    for j in range(a.blocks):
        b = f"{a.name}/block{j}"
        out.update({f"{b}/ln1/gamma": (c,), f"{b}/ln1/beta": (c,)})
        for part in ("query", "key", "value"):
            out[f"{b}/mha/{part}/kernel"] = (c, h, d)
            out[f"{b}/mha/{part}/bias"] = (h, d)
        out[f"{b}/mha/attention_output/kernel"] = (h, d, c)
        out[f"{b}/mha/attention_output/bias"] = (c,)
        out.update({f"{b}/ln2/gamma": (c,), f"{b}/ln2/beta": (c,), f"{b}/ffn1/kernel": (c, f), f"{b}/ffn1/bias": (f,),
                    f"{b}/ffn2/kernel": (f, c), f"{b}/ffn2/bias": (c,)})
    return out


def length_attn_weight_shapes(a: LengthAttn) -> dict[str, tuple]:
    """Keras variable shapes of one TransformerEncoder: the leaf names and shapes of a CrossFrameAttention layer with its
    feed-forward half (the two classes hold the same sub-layers under the same names, layers.py:2224-2245, :2321-2345)."""
    return frame_attn_weight_shapes(FrameAttn(a.name, a.channels, a.heads, a.key_dim, a.ff_dim, True))


def hyena_weight_shapes(a: Hyena) -> dict[str, tuple]:
    """Keras variable shapes of one HyenaBlock: the LayerNormalization's gamma / beta (C); the operator's ``order + 1``
    bias-free projections (C, C); per order the filter network's Dense layers (16 -> filter_hidden ... -> C, the last one
    alone with ``filter_layers`` 1) and the window's ``alphas`` / ``biases`` (order, C); the output projection if there is
    one.  ``<name>/hyena/filter/pos_encoding`` (seq_len, 16) is optional and not listed: when the weights hold it the
    filter table uses its rows (program.py: hyena_filter_tables)."""
    c, n = a.channels, a.name
    out: dict[str, tuple] = {f"{n}/norm/gamma": (c,), f"{n}/norm/beta": (c,)}
    for k in range(a.order + 1):
        out[f"{n}/hyena/proj_{k}/kernel"] = (c, c)
    for o in range(a.order):
        cin = HYENA_PE_DIM
        for j in range(a.filter_layers):
            units = c if j == a.filter_layers - 1 else a.filter_hidden
            out[f"{n}/hyena/filter/ffn_{o}/dense_{j}/kernel"] = (cin, units)
            out[f"{n}/hyena/filter/ffn_{o}/dense_{j}/bias"] = (units,)
            cin = units
    out[f"{n}/hyena/filter/alphas"] = (a.order, c)
    out[f"{n}/hyena/filter/biases"] = (a.order, c)
    if a.output_projection:
        out[f"{n}/out_proj/kernel"] = (c, c)
        out[f"{n}/out_proj/bias"] = (c,)
    return out


def bilstm_weight_shapes(a: BiLstm) -> dict[str, tuple]:
    """Keras variable shapes of one MaskedBiLSTM: per direction (``layer.bilstm.forward_layer.cell`` /
    ``backward_layer.cell``) the LSTMCell's kernel (C, 4U), recurrent_kernel (U, 4U) and bias (4U), the 4U columns in the
    gate order i, f, g, o."""
    out: dict[str, tuple] = {}
    for d in ("forward", "backward"):
        out[f"{a.name}/{d}/kernel"] = (a.cin, 4 * a.units)
        out[f"{a.name}/{d}/recurrent_kernel"] = (a.units, 4 * a.units)
        out[f"{a.name}/{d}/bias"] = (4 * a.units,)
    return out


def msconv_weight_shapes(a: MultiScaleConv) -> dict[str, tuple]:
    """Keras variable shapes of one MultiScaleConv1D: per branch (``layer._convs[b]``, a MaskedConv1D) the kernel
    (kernel_size, cin, filters) and, with use_bias, the bias (filters)."""
    out: dict[str, tuple] = {}
    for c in a.branches:
        out[f"{c.name}/kernel"] = (c.kernel_size, c.cin, c.filters)
        if c.use_bias:
            out[f"{c.name}/bias"] = (c.filters,)
    return out


def frame_attn_flops_per_position(plan: ModelPlan) -> list[tuple[str, int, int]]:
    """(name, FLOPs of the dense products, FLOPs of the score / softmax / context core) of every frame-attention layer,
    per POSITION (six tokens): q/k/v and output projections 4 x 2 C^2, feed-forward 2 x 2 C F, per token; scores and
    context 2 x 2 x 6 x 6 x C per position."""
    rows = []
    for layer in flat_layers(plan.rep):
        if isinstance(layer, FrameAttn):
            c, f = layer.channels, layer.ff_dim
            rows.append((layer.name, 6 * (8 * c * c + 4 * c * f), 4 * 36 * c))
    return rows


def conv_flops_per_position(plan: ModelPlan) -> list[tuple[str, int, int, int, str, int]]:
    """(name, k, cin, cout, padding, stride) of every conv, in execution order."""
    rows = []
    for layer in flat_layers(plan.rep):
        if isinstance(layer, Conv):
            rows.append((layer.name, layer.kernel_size, layer.cin, layer.filters, layer.padding, layer.strides))
        elif isinstance(layer, ResBlock):
            for c in (layer.conv1, layer.conv2, layer.conv3):
                if c is not None:
                    rows.append((c.name, c.kernel_size, c.cin, c.filters, c.padding, c.strides))
    return rows
