"""Layer plan -> op program + weight blob for ``libjaeger_hip.so``.

Fuses what the reference runs as separate Keras layers (``nnlib/builder.py:982-1193``
``_build_block``; ``nnlib/v2/layers.py:1882-1915`` ``ResidualBlock.call``) into
conv launches with epilogue stages:

* ``masked_conv1d -> [nmd] -> norm -> activation``            one conv op
* ``ResidualBlock``: ``conv1 -> bn1 -> act`` one conv op; ``conv2 -> bn2 -> (+ shortcut)
  -> act [-> nmd -> norm -> activation that follow the stack]`` one conv op;
  optional ``conv3 -> bn3`` bypass one conv op
* each conv with masking gets one tiny mask op (``layers.py:1226-1255``).
* ``cross_frame_attention -> norm -> activation``             one frame-attention op (``layers.py:2283-2384``); no mask
  leaves it
* ``local_attention -> norm -> activation``                   one local-attention op per block (``layers.py:2520-2645``),
  out of place, the mask kept; the norm / activation ride the last block's store
* ``transformer_encoder -> norm -> activation``               one length-attention op (``layers.py:2206-2280``), out of
  place, under the incoming mask; no mask leaves it
* ``axial_attention -> norm -> activation``                   per block a length-attention op (masked in block 0 only), a
  frame-attention op and an element-wise op with the post norm and the add of the block's input
  (``layers.py:2400-2517``); the mask kept; the norm / activation ride the last block's element-wise op
* ``hyena_block -> norm -> activation``                       one hyena op (``layers.py:2724-3153``), out of place, the mask
  kept; its implicit filters are tabled on the host once (:func:`hyena_filter_tables`) and travel in the weight blob
* ``masked_bilstm -> norm -> activation``                     one bilstm op (``layers.py:1335-1430``), out of place, rows of
  ``2 * units`` channels; the mask kept, or dropped with ``ignore_mask``
* ``multi_scale_conv -> norm -> activation``                  one mask op (the AND of the branches' output masks) and one
  multi-scale conv op (``layers.py:1433-1595``), out of place: every branch's conv, bias and activation and the concat / add
* ``parallel_branches`` of pooled branches                    per branch its layers by the same walk, on the trunk's tensor and
  mask, and one pool-and-merge op (``builder.py:1109-1153``): max / average / last pool of the branch's tensor, stored at
  the branch's offset (concat) or added / maximised into the vector (sum / average / max; average scales on its last branch)
* ``pooling: last``                                           one pool-and-merge op (``layers.py:541-578``)

The row mixers' ops: ``emit`` of the kind's class in ``mixers.py``.  Pure host logic (numpy + ctypes structs): unit-tested on CPU.
"""

from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

from . import _lib as L
from .mixers import (_MASK_MODE, POSITION_ROWS, Mixer, act_code,  # noqa: F401 - the last three: importable from here
                     hyena_filter_tables, hyena_table_rows, unpack_msconv_descriptor)
from .plan import Act, Conv, Dense, ModelPlan, Nmd, Norm, ParallelBranches, ResBlock, UnsupportedLayer, flat_layers, weight_shapes

_SIGNAL_CODE = {"max_prob": 1, "entropy": 2, "energy": 3, "margin": 4, "nmd_norm": 5}


class _Blob:
    """Flat f32 weight blob; every tensor starts on a 16-byte boundary."""

    def __init__(self):
        self.parts: list[np.ndarray] = []
        self.size = 0

    def add(self, arr) -> int:
        a = np.ascontiguousarray(arr, dtype=np.float32).ravel()
        off = self.size
        pad = (-a.size) % 4
        self.parts.append(a)
        if pad:
            self.parts.append(np.zeros(pad, np.float32))
        self.size += a.size + pad
        return off

    def finish(self) -> np.ndarray:
        return np.concatenate(self.parts) if self.parts else np.zeros(4, np.float32)


class _Slots:
    def __init__(self, n: int, what: str):
        self.free = list(range(n))
        self.what = what
        self.held: set[int] = set()          # slots that stay taken whoever gives them back (a trunk's, while its branches run)

    def take(self) -> int:
        if not self.free:
            raise UnsupportedLayer(f"program needs more than {L.JG_MAX_BUFS} {self.what} buffers")
        return self.free.pop(0)

    def give(self, s: int) -> None:
        if s is not None and s >= 0 and s not in self.free and s not in self.held:
            self.free.append(s)
            self.free.sort()


def pack_conv_kernel(kernel: np.ndarray) -> np.ndarray:
    """(k, cin, cout) -> (k, cin_pad, cout_pad) zero padded (cin to even, cout to x32)."""
    k, cin, cout = kernel.shape
    cin_pad, cout_pad = (cin + 1) & ~1, (cout + 31) // 32 * 32
    out = np.zeros((k, cin_pad, cout_pad), np.float32)
    out[:, :cin, :cout] = kernel
    return out


#: op kind -> what ``Program.describe`` adds behind the fields every op has
_DESCRIBE = {
    L.OP_FRAMEATTN: lambda op: f" heads={op.k} ff={op.arg}",
    L.OP_LOCALATTN: lambda op: f" heads={op.k} ff={op.arg} half_window={op.stride}",
    L.OP_HYENA: lambda op: f" order={op.k} flags={op.arg} table_rows={op.stride}",
    L.OP_BILSTM: lambda op: f" units={op.k} ignore_mask={op.arg & L.BILSTM_IGNORE_MASK}",
    L.OP_MSCONV: lambda op: f" branches={op.k} merge={'add' if op.arg == L.MSCONV_ADD else 'concat'}",
    L.OP_POOLVEC: lambda op: (f" pool={('max', 'average', '?', 'last')[op.arg & 3]} merge={('store', 'add', 'max')[op.k % 3]} "
                              f"vec={op.out_vec}[{op.vec_off}:{op.vec_off + op.cout}] scale={op.f0:g}"),
}
_DESCRIBE.update({L.OP_LENGTHATTN: _DESCRIBE[L.OP_FRAMEATTN], L.OP_MSMASK: _DESCRIBE[L.OP_MSCONV]})


@dataclass
class Program:
    ops: list            # list[L.JgOp]
    blob: np.ndarray     # float32
    vocab: int
    n_classes: int
    has_reliability: bool
    nmd_dim: int
    embedding_dim: int
    strands: int = 1     # > 1: ids (W, strands, L), one frame per program row (OP_STRANDS closes the program)

    def op_array(self):
        arr = (L.JgOp * len(self.ops))()
        for i, op in enumerate(self.ops):
            arr[i] = op
        return arr

    def describe(self) -> list[str]:
        kinds = {v: k for k, v in vars(L).items() if k.startswith("OP_")}
        stk = {v: k[3:] for k, v in vars(L).items() if k.startswith("ST_")}
        rows = []
        for op in self.ops:
            st = "+".join(stk[op.stages[s].kind] for s in range(op.n_stages))
            rows.append(f"{kinds[op.kind][3:]:9s} in={op.in_buf} out={op.out_buf} m={op.in_mask}->{op.out_mask} "
                        f"k={op.k} c={op.cin}->{op.cout} s={op.stride} d={op.dilation} [{st}]"
                        + _DESCRIBE.get(op.kind, lambda op: "")(op))
        return rows


class _Compiler:
    def __init__(self, plan: ModelPlan, weights: dict[str, np.ndarray]):
        self.plan, self.w = plan, weights
        for layer in flat_layers(plan.rep):     # (a kind's optional variables; weight_shapes covers the others)
            getattr(layer, "check_weights", lambda w: None)(weights)
        missing = [n for n in weight_shapes(plan) if n not in weights]
        if missing:
            raise KeyError(f"weights missing for: {missing[:6]}{'...' if len(missing) > 6 else ''}")
        for n, shp in weight_shapes(plan).items():
            if tuple(weights[n].shape) != tuple(shp):
                raise ValueError(f"weight {n}: shape {tuple(weights[n].shape)} != expected {shp}")
        self.blob = _Blob()
        self.ops: list = []
        self.bufs = _Slots(L.JG_MAX_BUFS, "activation")
        self.masks = _Slots(L.JG_MAX_BUFS, "mask")
        self.parts = _Slots(L.JG_MAX_BUFS, "nmd partial")
        self.nmd_off = 0
        # the taps write the model's nmd output itself - or, under an NMDMerge that projects (sum / mean / max / weighted),
        # a scratch vector the merge reads (the two last vector slots: the heads use the ones from VEC_SCRATCH0 up)
        self.nmd_vec = L.VEC_NMD if plan.nmd_merge_mode == "concat" else L.JG_MAX_VECS - 1
        # dead positions behind a masked local_attention (queries without a valid key in their band: the op writes zeros
        # where Keras' value depends on its version and precision).  They are masked, and stay harmless as long as every
        # later reader masks: None = the tensor holds none; else how many positions a later output mask may still grow
        # before it would validate one (a dead position lies more than half_window away from every valid one)
        self.dead_margin: int | None = None
        self.dead_layer = ""

    # ---- helpers -----------------------------------------------------------
    def _op(self, kind, **kw):
        op = L.JgOp()
        op.kind = kind
        for f in ("in_buf", "out_buf", "in_mask", "out_mask", "in_vec", "out_vec"):
            setattr(op, f, -1)
        op.w_off = op.b_off = -1
        op.stride = op.dilation = 1
        for k, v in kw.items():
            setattr(op, k, v)
        return op

    @staticmethod
    def _stage(kind, arg=0, p0=-1, p1=-1, p2=-1, p3=-1, f0=0.0):
        st = L.JgStage()
        st.kind, st.arg, st.p0, st.p1, st.p2, st.p3, st.f0 = kind, arg, p0, p1, p2, p3, f0
        return st

    def _norm_stage(self, n: Norm, has_mask: bool):
        w = self.w
        if n.kind == "masked_batchnorm":
            var = w[f"{n.name}/moving_variance"].astype(np.float32)
            inv_std = (np.float32(1.0) / np.sqrt(var + np.float32(n.epsilon))).astype(np.float32)
            return self._stage(L.ST_BN, p0=self.blob.add(w[f"{n.name}/moving_mean"]), p1=self.blob.add(inv_std),
                               p2=self.blob.add(w[f"{n.name}/gamma"]), p3=self.blob.add(w[f"{n.name}/beta"]))
        if n.kind == "masked_dyt":
            return self._stage(L.ST_DYT, arg=1 if has_mask else 0, f0=float(w[f"{n.name}/alpha"].ravel()[0]),
                               p2=self.blob.add(w[f"{n.name}/gamma"]), p3=self.blob.add(w[f"{n.name}/beta"]))
        if n.kind == "masked_layernorm":
            # a reduction over the channel axis: cannot live in a conv epilogue; _emit_conv cuts the stage list here
            return self._stage(L.ST_LN, arg=1 if has_mask else 0, f0=float(n.epsilon),
                               p2=self.blob.add(w[f"{n.name}/gamma"]), p3=self.blob.add(w[f"{n.name}/beta"]))
        raise UnsupportedLayer(f"{n.name}: {n.kind} is not supported by the MI355X engine yet")

    def _emit_conv(self, c: Conv, in_buf: int, in_mask: int, stages: list, out_mask: int, out_buf: int):
        # MaskedLayerNormalization needs a whole channel row: the conv keeps the stages in front of it and an
        # element-wise op (LayerNorm kernel) runs the norm and everything behind it, in place on the conv's output
        tail = []
        for j, st in enumerate(stages):
            if st.kind == L.ST_LN:
                stages, tail = stages[:j], stages[j:]
                break
        self._emit_conv_op(c, in_buf, in_mask, stages, out_mask, out_buf)
        self._emit_ln_tail(c.name, tail, out_mask, out_buf, c.filters)

    def _emit_ln_tail(self, name: str, tail: list, out_mask: int, out_buf: int, channels: int):
        while tail:                                   # one op per LayerNorm (each leads its own op)
            nxt = next((j for j, st in enumerate(tail) if st.kind == L.ST_LN and j > 0), len(tail))
            if nxt > L.JG_MAX_STAGES:
                raise UnsupportedLayer(f"{name}: more than {L.JG_MAX_STAGES} stages behind a layer norm")
            op = self._op(L.OP_ELTWISE, in_buf=out_buf, out_buf=out_buf, out_mask=out_mask, cout=channels)
            op.n_stages = nxt
            for j, st in enumerate(tail[:nxt]):
                op.stages[j] = st
            self.ops.append(op)
            tail = tail[nxt:]

    def _emit_conv_op(self, c: Conv, in_buf: int, in_mask: int, stages: list, out_mask: int, out_buf: int):
        if len(stages) > L.JG_MAX_STAGES:
            raise UnsupportedLayer(f"{c.name}: more than {L.JG_MAX_STAGES} fused epilogue stages")
        op = self._op(L.OP_CONV, in_buf=in_buf, out_buf=out_buf,
                      in_mask=in_mask if c.use_masking else L.JG_BUF_NONE, out_mask=out_mask,
                      k=c.kernel_size, cin=c.cin, cout=c.filters, stride=c.strides, dilation=c.dilation_rate,
                      padding=L.PAD_SAME if c.padding == "same" else L.PAD_VALID,
                      mask_mode=_MASK_MODE[c.mask_mode],
                      w_off=self.blob.add(pack_conv_kernel(self.w[f"{c.name}/kernel"])))
        if in_buf == L.JG_BUF_IDS:
            op.b_off = self.emb_off
        op.n_stages = len(stages)
        for i, st in enumerate(stages):
            op.stages[i] = st
        self.ops.append(op)

    def _conv_mask(self, c: Conv, in_mask: int) -> int:
        """Emit the mask op of a conv; returns the output mask slot (or NONE)."""
        if not c.use_masking or in_mask == L.JG_BUF_NONE:
            return L.JG_BUF_NONE
        if c.padding not in ("same", "valid"):
            raise ValueError(f"{c.name}: Invalid padding type {c.padding!r}")
        out = self.masks.take()
        self.ops.append(self._op(L.OP_MASK, in_mask=in_mask, out_mask=out, k=c.kernel_size, stride=c.strides,
                                 dilation=c.dilation_rate, mask_mode=_MASK_MODE[c.mask_mode],
                                 padding=L.PAD_SAME if c.padding == "same" else L.PAD_VALID))
        return out

    def _base_stages(self, c: Conv) -> list:
        st = []
        if c.use_bias:
            st.append(self._stage(L.ST_BIAS, p0=self.blob.add(self.w[f"{c.name}/bias"])))
        if c.activation is not None:
            st.append(self._stage(L.ST_ACT, arg=act_code(c.activation)))
        return st

    def _fuse_tail(self, layers: list, i: int, stages: list, mask: int, channels: int, pending_nmd: list):
        """Greedily fuse following nmd / norm / activation layers as epilogue stages."""
        while i < len(layers) and len(stages) < L.JG_MAX_STAGES:
            nxt = layers[i]
            if isinstance(nxt, Nmd):
                slot = self.parts.take()
                stages.append(self._stage(L.ST_NMD, arg=slot))
                pending_nmd.append((nxt, slot, mask))
            elif isinstance(nxt, Norm) and nxt.kind in ("masked_batchnorm", "masked_dyt", "masked_layernorm"):
                stages.append(self._norm_stage(nxt, mask != L.JG_BUF_NONE))
                if nxt.kind == "masked_batchnorm" and not nxt.use_masking:
                    self._refuse_unmasked_reader(f"{nxt.name}: masked_batchnorm with use_masking: false (it drops the mask "
                                                 "for every layer behind it)")
                    mask = L.JG_BUF_NONE          # supports_masking False drops the mask (layers.py:816)
            elif isinstance(nxt, Act):
                stages.append(self._stage(L.ST_ACT, arg=act_code(nxt.kind)))
            else:
                break
            i += 1
        return i, mask

    def _refuse_unmasked_reader(self, what: str) -> None:
        if self.dead_margin is not None:
            raise UnsupportedLayer(f"{what} behind {self.dead_layer}: it reads masked positions unmasked, and local_attention "
                                   "leaves zeros at positions whose band holds no valid key, where the Keras graph holds "
                                   "values that depend on its version and precision")

    def _emit_mixer(self, layers: list, i: int, what: str, buf: int, mask: int, out_mask: int, build_ops: list):
        """A row-mixer layer (frame / local / length attention, hyena, bilstm, multi-scale conv) at ``layers[i]``: its ops - ``build_ops``, one
        ``(in_buf, out_buf) -> op`` per op, each into a fresh slot, never in place - with the bias / batch norm / unmasked
        DyT / activation layers that follow fused into the LAST op's store; a LayerNorm or a masked DyT is cut off into an
        element-wise op behind it.  ``out_mask``: the mask the layers behind see (the incoming one, or none where the layer
        drops it).  Returns (index of the next layer, the output slot, the mask behind the fused tail)."""
        layer = layers[i]
        stages, pending = [], []
        i, mask2 = self._fuse_tail(layers, i + 1, stages, out_mask, layer.channels, pending)
        if pending:
            raise UnsupportedLayer(f"{layer.name}: an nmd tap directly behind {what} is not supported "
                                   "(the op's store carries no partial sums)")
        cut = next((j for j, st in enumerate(stages) if st.kind == L.ST_LN or (st.kind == L.ST_DYT and st.arg == 1)), len(stages))
        stages, tail = stages[:cut], stages[cut:]
        for build in build_ops:
            out = self.bufs.take()
            op = build(buf, out)
            if build is build_ops[-1]:
                op.n_stages = len(stages)
                for q, st in enumerate(stages):
                    op.stages[q] = st
            self.ops.append(op)
            self.bufs.give(buf)
            buf = out
        self._emit_ln_tail(layer.name, tail, out_mask, buf, layer.channels)
        if out_mask != mask:
            self.masks.give(mask)
        return i, buf, mask2

    def _flush_nmd(self, pending: list, buf: int):
        for nmd, slot, mask in pending:
            self.ops.append(self._op(L.OP_NMD_FINAL, in_buf=buf, in_mask=mask, cout=nmd.channels, arg=slot,
                                     out_vec=self.nmd_vec, vec_off=self.nmd_off, f0=nmd.epsilon,
                                     b_off=self.blob.add(self.w[f"{nmd.name}/moving_mean"])))
            self.nmd_off += nmd.channels
            self.parts.give(slot)
        pending.clear()

    # ---- representation learner ----------------------------------------------
    def _rep(self):
        plan = self.plan
        layers = plan.rep
        if plan.embedding_kind == "embedding":
            table = self.w["embedding/embeddings"]
        else:       # one-hot input: row 0 (invalid codon = all-zero one-hot row) is zero, row id + 1 the Dense row / unit row
            rows = self.w["embedding/kernel"] if plan.embedding_kind == "onehot_dense" else \
                np.eye(plan.vocab - 1, dtype=np.float32)
            table = np.concatenate([np.zeros((1, rows.shape[1]), np.float32), np.asarray(rows, np.float32)])
        self.emb_off = self.blob.add(table)
        buf, mask = L.JG_BUF_IDS, L.JG_BUF_IDS      # Embedding(mask_zero=True), builder.py:858-867
        if plan.vocab > 256 or plan.positional_wavelength is not None:
            # codon pairs (codon: DICODON, 4 097 ids): 16-bit ids do not fit the convs' one-byte gather - the lookup runs as
            # an op of its own that writes the rows and the mask (id != 0); everything behind it reads those.  The same op
            # adds the rows of SinusoidalPositionEmbedding (use_positional_embeddings): a table of POSITION_ROWS positions
            # computed here once - the sum depends on the position, so it cannot live in the convs' id -> row gather
            buf, mask = self.bufs.take(), self.masks.take()
            pos = {}
            if plan.positional_wavelength is not None:
                if plan.embedding_dim % 4:
                    raise UnsupportedLayer("positional embeddings need an embedding width that is a multiple of 4")
                pe = sinusoidal_position_rows(POSITION_ROWS, plan.embedding_dim, plan.positional_wavelength)
                pos = dict(w_off=self.blob.add(pe), k=POSITION_ROWS)
            self.ops.append(self._op(L.OP_EMBED, out_buf=buf, out_mask=mask, cout=plan.embedding_dim, b_off=self.emb_off, **pos))
        i = 0
        if layers and getattr(layers[0], "on_embedding", None):
            raise UnsupportedLayer(f"{layers[0].name}: {layers[0].yaml_name} directly on the embedding is not supported "
                                   f"{layers[0].on_embedding}")
        if not layers or not isinstance(layers[0], Conv):
            # A norm / activation / nmd / residual block - or the pool itself - directly on the Embedding output (the
            # reference's own Embedding -> MaskedBatchNorm -> masked max pool case, tests/unit/test_masked_pooling.py:
            # 186-209): the table rows pass through a one-tap identity conv that does NOT multiply by the mask, so that
            # masked positions keep Embedding row 0 exactly as in the Keras graph, and the Embedding's mask (ids != 0)
            # becomes a mask slot of its own; the layers that follow fuse into that conv's epilogue.
            e = plan.embedding_dim
            ident = Conv("embedding/identity", 1, e, e, 1, "same", 1, False, None, False, "any")
            self.w = dict(self.w)
            self.w["embedding/identity/kernel"] = np.eye(e, dtype=np.float32)[None]
            om = self._conv_mask(replace(ident, use_masking=True), mask)
            stages, pending = [], []
            i, om2 = self._fuse_tail(layers, 0, stages, om, e, pending)
            out = self.bufs.take()
            self._emit_conv(ident, buf, L.JG_BUF_NONE, stages, om, out)
            self._flush_nmd(pending, out)
            buf, mask = out, om2
        buf, mask = self._walk(layers, i, buf, mask, plan.embedding_dim)
        if buf == L.JG_BUF_IDS:
            raise UnsupportedLayer("the representation learner has no conv layer")
        if plan.pooling is None:                 # a parallel_branches of pooled branches wrote the embedding vector itself
            if buf is not None:
                raise UnsupportedLayer("pooling: null needs a parallel_branches of pooled branches as the last layer")
            return
        if buf is None:
            raise ValueError("a pooling behind a parallel_branches of pooled branches (the merge leaves a vector)")
        if plan.pooling == "last":
            self._pool_vec(buf, mask, "last", plan.rep_channels, 0, L.POOLVEC_STORE, 1.0, "pooling: last")
            return
        # max1d / average1d: the stock Keras Global*Pooling1D of a strand branch (builder.py:1706-1707) - no mask, no sentinel
        kind = L.POOL_MAX if plan.pooling in ("max", "max1d") else L.POOL_AVG      # (without a mask: plain max / mean)
        if plan.pooling in ("max1d", "average1d"):
            mask = L.JG_BUF_NONE
        self.ops.append(self._op(L.OP_POOL, in_buf=buf, in_mask=mask, out_vec=L.VEC_EMBEDDING, vec_off=0,
                                 cout=plan.rep_channels, arg=kind))

    def _pool_vec(self, buf: int, mask: int, pooling: str, channels: int, vec_off: int, merge: int, scale: float, what: str):
        """One pool-and-merge op: ``pooling`` of ``buf`` under ``mask`` into the embedding vector at ``vec_off``."""
        if pooling == "last":
            self._refuse_unmasked_reader(f"{what} (MaskedLastPooling reads position count - 1 of a row whatever its mask says)")
        kind = {"max": L.POOL_MAX, "average": L.POOL_AVG, "last": L.POOL_LAST}[pooling]
        self.ops.append(self._op(L.OP_POOLVEC, in_buf=buf, in_mask=mask, out_vec=L.VEC_EMBEDDING, vec_off=vec_off, cout=channels,
                                 arg=kind, k=merge, f0=scale))

    def _branches(self, layer: ParallelBranches, buf: int, mask: int, channels: int):
        """The branches of a ``parallel_branches`` on the trunk's tensor ``buf`` under ``mask``: the trunk's two slots stay
        taken while the branches run, every branch starts from the trunk's dead-position state, and its pooled vector meets
        the embedding vector by the layer's merge - in branch order, which fixes the float32 sum."""
        if buf == L.JG_BUF_IDS:
            raise UnsupportedLayer(f"{layer.name}: parallel_branches directly on the embedding is not supported")
        dead = (self.dead_margin, self.dead_layer)
        held = [(slots, s) for slots, s in ((self.bufs, buf), (self.masks, mask)) if s >= 0 and s not in slots.held]
        for slots, s in held:
            slots.held.add(s)
        n, off = len(layer.branches), 0
        for b, branch in enumerate(layer.branches):
            self.dead_margin, self.dead_layer = dead
            bbuf, bmask = self._walk(branch.layers, 0, buf, mask, channels)
            if bbuf is None:
                raise UnsupportedLayer(f"{layer.name}: a nested parallel_branches is not supported")
            if layer.merge == "concat":
                merge, scale = L.POOLVEC_STORE, 1.0
            else:
                merge = L.POOLVEC_STORE if b == 0 else L.POOLVEC_MAX if layer.merge == "max" else L.POOLVEC_ADD
                scale = 1.0 / n if layer.merge == "average" and b == n - 1 else 1.0
            self._pool_vec(bbuf, bmask, branch.pooling, branch.channels, off, merge, scale,
                           f"{layer.name}/branch{b}: pooling: last")
            off += branch.channels if layer.merge == "concat" else 0
            self.bufs.give(bbuf)                 # (the trunk's own slots are held: a branch without layers gives nothing back)
            self.masks.give(bmask)
        self.dead_margin, self.dead_layer = dead
        for slots, s in held:
            slots.held.discard(s)
            slots.give(s)

    # ---- the layer walk: one handler per layer type, (layers, i, buf, mask, cin) -> (next i, slot, mask slot, channels) --
    def _conv(self, layers: list, i: int, buf: int, mask: int, cin: int):
        layer, pending = layers[i], []
        if not layer.use_masking or mask == L.JG_BUF_NONE:
            self._refuse_unmasked_reader(f"{layer.name}: a conv without masking")
        self.dead_margin = None           # a masked conv reads valid positions only: its output holds no dead value
        om = self._conv_mask(layer, mask)
        stages = self._base_stages(layer)
        i, om2 = self._fuse_tail(layers, i + 1, stages, om, layer.filters, pending)
        out = self.bufs.take()
        self._emit_conv(layer, buf, mask, stages, om, out)
        self._flush_nmd(pending, out)
        self.bufs.give(buf)
        if mask != om:
            self.masks.give(mask)
        return i, out, om2, layer.filters

    def _resblock(self, layers: list, i: int, buf: int, mask: int, cin: int):
        blk, pending = layers[i], []
        if not blk.use_masking or mask == L.JG_BUF_NONE:
            self._refuse_unmasked_reader(f"{blk.name}: a residual block without masking")
        if self.dead_margin is not None and blk.conv3 is None:
            # the shortcut adds the block's input as it is (layers.py:1907-1913) while the two convs grow the mask
            span = (blk.conv1.kernel_size - 1) * blk.conv1.dilation_rate
            grow = 2 * (span - span // 2)
            if grow > self.dead_margin:
                self._refuse_unmasked_reader(f"{blk.name}: a residual block whose output mask grows by {grow} positions "
                                             f"(its shortcut carries the input's masked positions; room {self.dead_margin})")
            self.dead_margin -= grow
        elif blk.conv3 is not None:
            self.dead_margin = None       # every path into the output is a masked conv
        in_mask = mask if blk.use_masking else L.JG_BUF_NONE
        m1 = self._conv_mask(blk.conv1, in_mask)
        b1 = self.bufs.take()
        st1 = self._base_stages(blk.conv1) + [self._norm_stage(blk.bn1, m1 != L.JG_BUF_NONE),
                                              self._stage(L.ST_ACT, arg=act_code(blk.activation))]
        self._emit_conv(blk.conv1, buf, in_mask, st1, m1, b1)
        shortcut = buf
        b3 = None
        if blk.conv3 is not None:
            m3 = self._conv_mask(blk.conv3, in_mask)
            b3 = self.bufs.take()
            st3 = self._base_stages(blk.conv3) + [self._norm_stage(blk.bn3, m3 != L.JG_BUF_NONE)]
            self._emit_conv(blk.conv3, buf, in_mask, st3, m3, b3)
            self.masks.give(m3)
            shortcut = b3
        if shortcut == L.JG_BUF_IDS:
            raise UnsupportedLayer(f"{blk.name}: a residual block cannot be the first layer")
        m2 = self._conv_mask(blk.conv2, m1)
        b2 = self.bufs.take()
        st2 = self._base_stages(blk.conv2)
        if blk.nmd is not None:             # bn2(return_nmd=True): tap on bn2's input, conv2's mask
            slot = self.parts.take()
            st2.append(self._stage(L.ST_NMD, arg=slot))
            pending.append((blk.nmd, slot, m2))
        st2 += [self._norm_stage(blk.bn2, m2 != L.JG_BUF_NONE), self._stage(L.ST_ADD, arg=shortcut),
                self._stage(L.ST_ACT, arg=act_code(blk.activation))]
        i, m2b = self._fuse_tail(layers, i + 1, st2, m2, blk.conv2.filters, pending)
        self._emit_conv(blk.conv2, b1, m1, st2, m2, b2)
        self._flush_nmd(pending, b2)
        for s in (buf, b1, b3):
            self.bufs.give(s)
        for s in (mask, m1):
            if s != m2:
                self.masks.give(s)
        return i, b2, m2b, blk.conv2.filters

    def _eltwise(self, layers: list, i: int, buf: int, mask: int, cin: int):
        """A norm / activation that no conv in front of it could take: an element-wise op, in place."""
        layer, pending = layers[i], []
        if buf == L.JG_BUF_IDS:
            raise UnsupportedLayer("a norm / activation directly on the embedding is not supported")
        if buf in self.bufs.held:
            raise UnsupportedLayer(f"{getattr(layer, 'name', layer.__class__.__name__)}: a norm / activation as the first layer of "
                                   "a branch is not supported (it runs in place, on the tensor the other branches read)")
        stages: list = []
        i, mask2 = self._fuse_tail(layers, i, stages, mask, 0, pending)
        if pending:
            raise UnsupportedLayer("an nmd layer must directly follow a conv or residual block")
        if not stages:
            raise UnsupportedLayer(f"{getattr(layer, 'name', layer)}: unsupported standalone layer")
        # a LayerNorm must lead its op (the LayerNorm kernel): cut the list in front of every LN stage
        cuts = [0] + [j for j, st in enumerate(stages) if st.kind == L.ST_LN and j > 0] + [len(stages)]
        for a_, b_ in zip(cuts[:-1], cuts[1:]):
            op = self._op(L.OP_ELTWISE, in_buf=buf, out_buf=buf, out_mask=mask, cout=cin)
            op.n_stages = b_ - a_
            for j, st in enumerate(stages[a_:b_]):
                op.stages[j] = st
            self.ops.append(op)
        return i, buf, mask2, cin

    _HANDLERS = {Conv: _conv, ResBlock: _resblock, Norm: _eltwise, Act: _eltwise}

    def _walk(self, layers: list, i: int, buf: int, mask: int, cin: int):
        """The layer walk from ``layers[i]`` on: the tensor in slot ``buf`` (``cin`` channels) under mask slot ``mask`` through
        the layers; returns the output slot and the mask slot behind them - or (None, None) behind a ``parallel_branches``,
        which leaves the embedding vector.  The trunk and every branch of a ``parallel_branches`` go through this."""
        while i < len(layers):
            layer = layers[i]
            if isinstance(layer, Mixer):
                (i, buf, mask), cin = layer.emit(self, layers, i, buf, mask), layer.channels
            elif type(layer) in self._HANDLERS:
                i, buf, mask, cin = self._HANDLERS[type(layer)](self, layers, i, buf, mask, cin)
            elif isinstance(layer, ParallelBranches):
                if i + 1 != len(layers):
                    raise UnsupportedLayer(f"{layer.name}: a layer behind a parallel_branches of pooled branches")
                self._branches(layer, buf, mask, cin)
                return None, None
            elif isinstance(layer, Nmd):
                raise UnsupportedLayer("an nmd layer must directly follow a conv or residual block")
            else:
                raise UnsupportedLayer(f"layer {layer!r} is not supported in the representation learner")
        return buf, mask

    # ---- heads -----------------------------------------------------------------
    def _head(self, layers: list, in_vec: int, out_vec: int, scratch0: int) -> None:
        dense_idx = [j for j, l in enumerate(layers) if isinstance(l, Dense)]
        if not dense_idx:
            raise UnsupportedLayer("a head needs at least one dense layer")
        cur, scratch = in_vec, scratch0
        j = 0
        while j < len(layers):
            layer = layers[j]
            if not isinstance(layer, Dense):
                raise UnsupportedLayer(f"head layer {layer!r} must follow a dense layer")
            act = layer.activation
            if j + 1 < len(layers) and isinstance(layers[j + 1], Act):
                if act is not None:
                    raise UnsupportedLayer("dense activation followed by another activation")
                act = layers[j + 1].kind
                j += 1
            last = not any(isinstance(l, Dense) for l in layers[j + 1:])
            dst = out_vec if last else scratch
            if not last:
                scratch += 1
                if scratch >= L.JG_MAX_VECS:
                    raise UnsupportedLayer("head too deep for the vector slots")
            b_off = self.blob.add(self.w[f"{layer.name}/bias"]) if layer.use_bias else -1
            self.ops.append(self._op(L.OP_DENSE, in_vec=cur, out_vec=dst, vec_off=0, cin=layer.cin,
                                     cout=layer.units, arg=act_code(act),
                                     w_off=self.blob.add(self.w[f"{layer.name}/kernel"]), b_off=b_off))
            cur = dst
            j += 1

    def _nmd_merge(self) -> None:
        """NMDMerge(mode != "concat") (nnlib/v2/nmd.py:141-155) behind the representation learner.  Every tap's vector goes
        through its own bias-free projection and the results are added (sum), averaged (mean), weighted by
        softmax(layer_weights) (weighted) - all three ONE dense layer over the vectors side by side, its kernel the
        projections stacked and scaled - or maximised element by element (max: the projections as one block-diagonal
        dense layer, then JG_OP_VECMAX over the blocks)."""
        plan = self.plan
        n, t = len(plan.nmd_dims), plan.nmd_merge_dim
        proj = [np.asarray(self.w[f"rep/nmd_merge/proj_{i}/kernel"], np.float32) for i in range(n)]
        raw = plan.nmd_raw_dim
        act = getattr(plan, "nmd_merge_act", None)
        if plan.nmd_merge_mode == "max" or act is not None:
            # the projections as ONE block-diagonal dense layer (with the projections' activation, projection_kwargs: round 6)
            kernel = np.zeros((raw, n * t), np.float32)
            at = 0
            for i, (d, p) in enumerate(zip(plan.nmd_dims, proj)):
                kernel[at:at + d, i * t:(i + 1) * t] = p
                at += d
            blocks = L.JG_MAX_VECS - 2
            self.ops.append(self._op(L.OP_DENSE, in_vec=self.nmd_vec, out_vec=blocks, vec_off=0, cin=raw, cout=n * t,
                                     arg=act_code(act), w_off=self.blob.add(kernel), b_off=-1))
            if plan.nmd_merge_mode == "max":
                self.ops.append(self._op(L.OP_VECMAX, in_vec=blocks, out_vec=L.VEC_NMD, vec_off=0, k=n, cout=t))
                return
        if plan.nmd_merge_mode == "weighted":
            lw = np.asarray(self.w["rep/nmd_merge/layer_weights"], np.float32)
            e = np.exp(lw - lw.max())
            scale = (e / e.sum()).astype(np.float32)            # tf.nn.softmax(layer_weights), nmd.py:153-155
        else:
            scale = np.full(n, 1.0 if plan.nmd_merge_mode == "sum" else 1.0 / n, np.float32)
        if act is not None:
            # sum / mean / weighted of ACTIVATED projections: a second, linear dense layer over the blocks whose kernel is the
            # scaled identity matrices stacked (every product with a zero is exact: the sum is the weighted sum of the blocks)
            kernel = np.concatenate([np.eye(t, dtype=np.float32) * s for s in scale], axis=0).astype(np.float32)
            self.ops.append(self._op(L.OP_DENSE, in_vec=L.JG_MAX_VECS - 2, out_vec=L.VEC_NMD, vec_off=0, cin=n * t, cout=t,
                                     arg=act_code(None), w_off=self.blob.add(kernel), b_off=-1))
            return
        kernel = np.concatenate([p * s for p, s in zip(proj, scale)], axis=0).astype(np.float32)
        self.ops.append(self._op(L.OP_DENSE, in_vec=self.nmd_vec, out_vec=L.VEC_NMD, vec_off=0, cin=raw, cout=t,
                                 arg=act_code(None), w_off=self.blob.add(kernel), b_off=-1))

    def compile(self) -> Program:
        plan = self.plan
        self._rep()
        if plan.nmd_merge_mode != "concat":
            self._nmd_merge()
        self._head(plan.classifier, L.VEC_EMBEDDING, L.VEC_PREDICTION, L.VEC_SCRATCH0)
        if plan.reliability is not None:
            if plan.reliability_signals:
                order = 0
                for idx, s in enumerate(plan.reliability_signals):
                    if s not in _SIGNAL_CODE:
                        raise ValueError(f"Unsupported signal(s): {s!r}")       # layers.py:1626-1630
                    order |= _SIGNAL_CODE[s] << (4 * idx)
                self.ops.append(self._op(L.OP_OODSIG, in_vec=L.VEC_PREDICTION, k=L.VEC_NMD, cin=plan.n_classes,
                                         cout=len(plan.reliability_signals), out_vec=L.VEC_NMD,
                                         vec_off=plan.nmd_dim, arg=order, f0=1e-10, stride=plan.nmd_dim))
            self._head(plan.reliability, L.VEC_NMD, L.VEC_RELIABILITY, L.VEC_SCRATCH0 + 4)
        if plan.strands > 1:
            # the heads above ran per strand (shared weights); the window's outputs are the strands' merged
            # (tf.keras.layers.Average / Add / Maximum, builder.py:1251-1262; embedding: Average, :779-780)
            self.ops.append(self._op(L.OP_STRANDS, k=plan.strands,
                                     arg={"average": L.MERGE_AVERAGE, "sum": L.MERGE_SUM, "max": L.MERGE_MAX,
                                          "concat": L.MERGE_CONCAT}[plan.merge]))
        return Program(self.ops, self.blob.finish(), plan.vocab, plan.n_classes,
                       plan.reliability is not None, plan.nmd_dim, plan.rep_channels, plan.strands)


def sinusoidal_position_rows(n_pos: int, hidden: int, max_wavelength: float) -> np.ndarray:
    """SinusoidalPositionEmbedding.call (nnlib/v2/layers.py:2155-2195) for positions 0 .. n_pos - 1, in float32 like the
    layer's compute dtype: timescale_i = (1 / max_wavelength) ** (2 floor(i / 2) / hidden), row[p, i] = sin(p timescale_i) for
    even i, cos(p timescale_i) for odd i."""
    f = np.float32
    positions = np.arange(n_pos, dtype=f)
    dims = np.arange(hidden, dtype=f)
    even = np.floor(dims / f(2)) * f(2)
    timescales = np.power(f(1.0) / f(max_wavelength), even / f(hidden)).astype(f)
    angles = (positions[:, None] * timescales[None, :]).astype(f)
    sin_mask = (np.arange(hidden) % 2 == 0).astype(f)
    return (np.sin(angles) * sin_mask + np.cos(angles) * (f(1.0) - sin_mask)).astype(f)


def compile_plan(plan: ModelPlan, weights: dict[str, np.ndarray]) -> Program:
    return _Compiler(plan, weights).compile()
