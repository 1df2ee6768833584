"""``*_project.yaml`` -> explicit layer plan.

The reference turns the ``model:`` section of a project YAML into a Keras graph
in ``nnlib/builder.py`` (``build_fragment_classifier`` :442-838,
``_build_embedding`` :844-894, ``_build_block`` :982-1193, ``_get_pooler``
:1697-1714).  This module resolves the same section into a flat, fully
defaulted plan (every default below cites the constructor it comes from) that
``program.py`` compiles for the MI355X engine.  Layers outside the conv family
(gated pooling ...) raise :class:`UnsupportedLayer`; the row-mixer kinds are plan nodes of their own, one class per kind
in ``mixers.py`` (``MIXERS``: YAML name -> class), and so is ``parallel_branches``.

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
from .mixers import *  # noqa: F401,F403 - the mixer classes, Conv, Norm, UnsupportedLayer and the kernels' limits: part of this module's interface

_ACT_ALIASES = ("relu", "gelu", "sigmoid", "softmax", "tanh")
_NORMS = ("masked_batchnorm", "masked_dyt", "masked_layernorm")
_DEFAULT_SIGNALS = ["max_prob", "entropy", "energy", "margin", "nmd_norm"]


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
        elif name in MIXERS and MIXERS[name].accepts(cfg):
            # a row mixer (mixers.py); an entry the reference's constructor would not take falls through to the generic
            # refusal below
            out.append(MIXERS[name].parse(p, cfg, cin, frames))
            nxt = layers[i + 1] if i + 1 < len(layers) else {}
            if MIXERS[name].tap_lookahead and not drop and \
                    (str(nxt.get("name", "")).lower() == "nmd" or (nxt.get("config") or {}).get("return_nmd")):
                raise UnsupportedLayer(f"{p}: an nmd tap directly behind {name} is not supported "
                                       "(the op's store carries no partial sums)")
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
    _check_kernel_widths(plan)
    return plan


#: what the conv, element-wise and LayerNorm kernels (csrc/jg_kernels.hip) cover: a lane owns a channel quad, a lane of the
#: LayerNorm kernel's wave two of them
CHANNEL_QUAD = 4
LAYERNORM_MAX_CHANNELS = 512


def _check_kernel_widths(plan: ModelPlan) -> None:
    """The channel limits of the kernels the representation learner of a translated model runs on (``jg_model_create``
    refuses the same programs): last, so that every refusal above keeps its wording."""
    def conv(c: Conv) -> None:
        if c.cin % CHANNEL_QUAD or c.filters % CHANNEL_QUAD:
            raise UnsupportedLayer(f"{c.name}: a conv of {c.cin} -> {c.filters} channels (both must be multiples of "
                                   f"{CHANNEL_QUAD}: a lane of the conv kernels owns a channel quad)")

    def norm(n: Norm) -> None:
        if n.channels % CHANNEL_QUAD:
            raise UnsupportedLayer(f"{n.name}: {n.kind} over {n.channels} channels (a multiple of {CHANNEL_QUAD}: a lane of "
                                   "the element-wise kernels owns a channel quad)")
        if n.kind == "masked_layernorm" and n.channels > LAYERNORM_MAX_CHANNELS:
            raise UnsupportedLayer(f"{n.name}: masked_layernorm over {n.channels} channels (up to {LAYERNORM_MAX_CHANNELS}: "
                                   "a lane of the kernel's wave holds two channel quads)")

    for layer in flat_layers(plan.rep):
        if isinstance(layer, Conv):
            conv(layer)
        elif isinstance(layer, Norm):
            norm(layer)
        elif isinstance(layer, ResBlock):
            for c in (layer.conv1, layer.conv2, layer.conv3):
                if c is not None:
                    conv(c)
            for n in (layer.bn1, layer.bn2, layer.bn3):
                if n is not None:
                    norm(n)


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

    def conv(c: Conv):
        out[f"{c.name}/kernel"] = (c.kernel_size, c.cin, c.filters)
        if c.use_bias:
            out[f"{c.name}/bias"] = (c.filters,)

    for seq in (plan.rep, plan.classifier, plan.reliability or []):
        for layer in flat_layers(seq):
            if isinstance(layer, Conv):
                conv(layer)
            elif isinstance(layer, Norm):
                out.update(norm_weight_shapes(layer))
            elif isinstance(layer, Nmd):
                out[f"{layer.name}/moving_mean"] = (layer.channels,)
            elif isinstance(layer, ResBlock):
                for c in (layer.conv1, layer.conv2, layer.conv3):
                    if c is not None:
                        conv(c)
                for n in (layer.bn1, layer.bn2, layer.bn3):
                    if n is not None:
                        out.update(norm_weight_shapes(n))
            elif isinstance(layer, Dense):
                out[f"{layer.name}/kernel"] = (layer.cin, layer.units)
                if layer.use_bias:
                    out[f"{layer.name}/bias"] = (layer.units,)
            elif isinstance(layer, Mixer):
                out.update(layer.weight_shapes())
        if seq is plan.rep and plan.nmd_merge_mode != "concat":                 # NMDMerge is built behind the rep block's layers
            for i, d in enumerate(plan.nmd_dims):
                out[f"rep/nmd_merge/proj_{i}/kernel"] = (d, plan.nmd_merge_dim)
            if plan.nmd_merge_mode == "weighted":
                out["rep/nmd_merge/layer_weights"] = (len(plan.nmd_dims),)
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
