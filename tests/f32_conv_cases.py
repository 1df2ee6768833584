"""The cases of the exact-f32 conv and layer-norm checks (tests/test_f32_conv_reference.py on the CPU,
tests/test_gpu_f32_conv.py on the GPU): every tile shape, width, row length and channel pass of ``conv_f32_kernel`` and every
quad slot of ``layernorm_kernel`` (``jaeger_amd/csrc/jg_kernels.hip``), one op at a time.

The launcher's choices, restated (the CPU module pins them to the source text of ``jg_launch_conv``, ``jg_conv_tile_m``,
``conv_f32_cchunk`` and ``conv_f32_lds``):

* ``tile_of(cout)`` - the column block ``BN`` of the instantiation and ``gridDim.y``: ``cout_pad`` (``cout`` rounded to 32) a
  multiple of 128 runs ``<2,2,1,2>`` (BN 128), of 64 ``<2,2,1,1>`` (BN 64), else ``<2,1,1,1>`` (BN 32);
* ``passes_of(k, stride, dil, cin)`` - the widths of the channel passes: all of ``cin_pad`` (``cin`` rounded to 8) when the
  ``63 stride + (k - 1) dil + 1`` input rows of a 64-position tile fit 160 KB at a pitch of ``cin_pad + 4`` floats, else the
  largest multiple of 8 that fits, and the rest;
* ``tiles_m(l_out)`` - 64-position tiles per row (``jg_conv_tile_m`` returns 64 whatever it is given).

A conv case is the smallest program that puts ONE conv (the target) in front of the check: a first-layer conv from the ids that
makes its input of ``cin`` channels (a second one the shortcut where the epilogue adds one), the MASK op of the target's
geometry, the target, an NMD finish per tap, an average pool and a 2-class dense layer - op lists written with
``conv_instance_cases._Writer`` (biases away from zero, batch norms far from the identity).  In the first-layer form the target
reads the ids itself.  A layer-norm case puts an ELTWISE op whose first stage is LN behind a first-layer conv of ``c`` channels.
Inputs are ``op_cases.edge_ids`` (rows shorter than 8 positions: ``small_ids``).

Each axis is swept on the base case (32 -> 32 channels, k 5, ``same``, 165 positions); axes are combined only where ``_cases``
says so.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np

from conv_instance_cases import _Writer

ACT_GELU_TANH, ACT_GELU_ERF, ACT_RELU = 1, 2, 3
MASK_ANY, MASK_MAJORITY, MASK_STRICT = 0, 1, 2
VOCAB = 65
TILE_M = 64
LDS_BYTES = 160 * 1024
LN_EPS = 1e-3


# ---- the launcher, restated ------------------------------------------------------------------------------------------------
def tile_of(cout: int) -> tuple:
    """(BN, gridDim.y) of jg_launch_conv's instantiation for ``cout`` output channels."""
    cout_pad = -(-cout // 32) * 32
    bn = 128 if cout_pad % 128 == 0 else 64 if cout_pad % 64 == 0 else 32
    return bn, -(-cout // bn)


def instantiation(cout: int) -> str:
    return {128: "<2,2,1,2>", 64: "<2,2,1,1>", 32: "<2,1,1,1>"}[tile_of(cout)[0]]


def rows_in(k: int, stride: int, dil: int) -> int:
    return (TILE_M - 1) * stride + (k - 1) * dil + 1


def cchunk(k: int, cin_pad: int, stride: int, dil: int) -> int:
    """conv_f32_cchunk at 64-position tiles: input channels staged per pass (0: not even 8 fit)."""
    fit = LDS_BYTES // (rows_in(k, stride, dil) * 4) - 4
    if fit >= cin_pad:
        return cin_pad
    return 0 if fit < 8 else fit // 8 * 8


def passes_of(k: int, stride: int, dil: int, cin: int) -> list:
    cin_pad = -(-cin // 8) * 8
    ch = cchunk(k, cin_pad, stride, dil)
    assert ch >= 8, (k, stride, dil, cin)
    return [min(ch, cin_pad - c0) for c0 in range(0, cin_pad, ch)]


def lds_bytes(bn: int, k: int, cch: int, stride: int, dil: int) -> int:
    """conv_f32_lds at 64-position tiles: the staged rows of a pass or the accumulator exchange, whichever is larger."""
    a, c = rows_in(k, stride, dil) * (cch + 4) * 4, TILE_M * (bn + 4) * 4
    return (max(a, c) + 15) & ~15


def tiles_m(l_out: int) -> int:
    return -(-l_out // TILE_M)


def l_out_of(l: int, k: int, stride: int, dil: int, padding: str) -> int:
    if padding == "same":
        return -(-l // stride)
    span = dil * (k - 1) + 1
    return (l - span) // stride + 1 if l >= span else 0


def cell(cin: int, cout: int, k: int, stride: int, dil: int, l_out: int) -> tuple:
    """What the census counts: (BN, gridDim.y, partial last column block, cin % 8, passes, partial last pass, tiles per row -
    1, 2 or 3 and more)."""
    bn, gy = tile_of(cout)
    ps = passes_of(k, stride, dil, cin)
    return bn, min(gy, 5), cout % bn != 0, cin % 8, min(len(ps), 2), len(ps) > 1 and ps[-1] != ps[0], min(tiles_m(l_out), 3)


# ---- cases -------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    cin: int = 32
    cout: int = 32
    k: int = 5
    l: int = 165
    stride: int = 1
    dil: int = 1
    padding: str = "same"
    ep: str = "bn_act"             # bias | bn_act | dyt | add_act | nmd1 | nmd2
    first: bool = False            # the target reads the ids (cin = the embedding width)
    mask_from_ids: bool = True     # first-layer form: zero the rows of id 0
    out_mask: bool = True
    mask_mode: int = MASK_ANY
    n_win: int = 4
    chunk: int = 0

    @property
    def l_out(self) -> int:
        return l_out_of(self.l, self.k, self.stride, self.dil, self.padding)

    @property
    def cell(self) -> tuple:
        return cell(self.cin, self.cout, self.k, self.stride, self.dil, self.l_out)

    @property
    def n_taps(self) -> int:
        return {"nmd1": 1, "nmd2": 2}.get(self.ep, 0)


COUTS = {32: (4, 28, 32, 72, 96, 160), 64: (36, 64, 164, 192), 128: (100, 128, 228, 256, 384)}
CINS = (4, 8, 12, 20, 36, 128, 260)
ROW_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 165)
#: the rows of the pass table: (cin, k, dilation, stride, cout) - cout so that every BN and both partial column blocks meet passes
PASS_ROWS = ((256, 7, 8, 2, 28), (512, 5, 4, 1, 64), (256, 9, 12, 1, 128), (128, 15, 18, 1, 36), (260, 9, 12, 1, 100))


def one_pass_dilation(cin: int, k: int, dil: int, stride: int) -> int:
    """The largest dilation at or below ``dil`` at which the conv takes exactly one pass."""
    while len(passes_of(k, stride, dil, cin)) > 1:
        dil -= 1
        assert dil >= 1
    return dil


def _cases() -> list:
    out = []

    def add(name, **kw):
        out.append(Case(name, **kw))

    for bn, couts in COUTS.items():
        for cout in couts:
            assert tile_of(cout)[0] == bn, cout
            add(f"cout{cout}-bn{bn}", cout=cout)
    for cin in CINS:
        add(f"cin{cin}", cin=cin)
    for bn, cout in ((32, 28), (64, 36), (128, 100)):              # (a partial column block at every row length)
        for l in ROW_LENGTHS:
            add(f"l{l}-bn{bn}", l=l, cout=cout, ep="nmd2")
    for k in (1, 2, 3, 4, 7, 9, 15):
        add(f"k{k}", k=k)
    for dil in (2, 3, 8):
        add(f"dil{dil}", dil=dil)
    add("k4-dil3", k=4, dil=3)                                      # (an even k whose uneven padding is three positions apart)
    for stride in (2, 3):
        add(f"stride{stride}", stride=stride)
        add(f"stride{stride}-k4", stride=stride, k=4)
    add("valid", padding="valid")
    add("valid-dil3", padding="valid", dil=3)
    add("valid-k4-stride2", padding="valid", k=4, stride=2)
    add("valid-one-position", padding="valid", dil=3, l=13)
    add("valid-one-position-k15", padding="valid", k=15, l=15, cout=36)
    for emb in (4, 8, 16, 64):
        for from_ids in (True, False):
            for k in (3, 7):
                add(f"first-e{emb}-k{k}-{'idmask' if from_ids else 'nomask'}", first=True, cin=emb, k=k, mask_from_ids=from_ids,
                    cout=(32, 64, 128, 36)[((emb // 4).bit_length() + (k == 7)) % 4])
    for cin, k, dil, stride, cout in PASS_ROWS:
        # 65 output positions: one whole tile and a tail tile of one position
        l = 65 * stride
        assert len(passes_of(k, stride, dil, cin)) == 2
        add(f"pass2-cin{cin}-k{k}-d{dil}-s{stride}", cin=cin, k=k, dil=dil, stride=stride, cout=cout, l=l, ep="nmd1")
        d1 = one_pass_dilation(cin, k, dil, stride)
        assert len(passes_of(k, stride, d1 + 1, cin)) == 2
        add(f"pass1-cin{cin}-k{k}-d{d1}-s{stride}", cin=cin, k=k, dil=d1, stride=stride, cout=cout, l=l, ep="nmd1")
    for ep in ("bias", "dyt", "add_act", "nmd1", "nmd2"):
        add(f"ep-{ep}", ep=ep)
    add("ep-bn_act-nomask", out_mask=False)
    add("ep-nmd2-nomask", ep="nmd2", out_mask=False)
    add("ep-add_act-c100", ep="add_act", cout=100)
    add("mask-majority", mask_mode=MASK_MAJORITY, k=7, dil=2)
    add("mask-strict", mask_mode=MASK_STRICT, k=3)
    add("mask-any-k9", mask_mode=MASK_ANY, k=9, ep="nmd1")
    for bn, cout in ((32, 72), (64, 164), (128, 228)):
        add(f"chunk2-bn{bn}", cout=cout, n_win=5, chunk=2, ep="nmd1")
    cin, k, dil, stride, _ = PASS_ROWS[0]
    add("chunk2-pass2", cin=cin, k=k, dil=dil, stride=stride, cout=32, l=65 * stride, n_win=5, chunk=2, ep="nmd1")
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


@dataclass
class LnCase:
    name: str
    c: int
    l: int
    kind: str = "ln"               # ln | ln_add_act | ln_nmd | bn_act | dyt   (the last two: a plain ELTWISE op)
    mask: bool = True              # the op names an output mask
    use_masking: bool = True       # the LN stage's own mask multiply (its arg)
    n_win: int = 4

    @property
    def is_ln(self) -> bool:
        return self.kind.startswith("ln")


LN_WIDTHS = (4, 36, 252, 256, 260, 384, 512)
LN_ROWS = (1, 3, 4, 5, 165)


def _ln_cases() -> list:
    out = []
    j = 0
    for c in LN_WIDTHS:
        for l in LN_ROWS:
            # the forms rotate over the cross of widths and rows; the NMD tap sits on the three-tile rows of every width
            kind = "ln_nmd" if l == 165 else ("ln", "ln_add_act")[j % 2]
            mask, um = ((True, True), (True, False), (False, True), (False, False))[(j // 2) % 4] if l != 165 else (True, True)
            out.append(LnCase(f"ln-c{c}-l{l}-{kind}-{'mask' if mask else 'nomask'}-{'um' if um else 'noum'}", c, l, kind, mask, um))
            j += 1
    for c in (260, 512):
        out.append(LnCase(f"ln-c{c}-l165-ln_add_act-mask-noum", c, 165, "ln_add_act", True, False))
        out.append(LnCase(f"ln-c{c}-l165-ln_nmd-nomask-um", c, 165, "ln_nmd", False, True))
    for c in (4, 260, 512):
        for kind in ("bn_act", "dyt"):
            out.append(LnCase(f"elt-c{c}-{kind}", c, 165, kind))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


LN_CASES = _ln_cases()
LN_BY_NAME = {c.name: c for c in LN_CASES}


# ---- inputs and programs -----------------------------------------------------------------------------------------------------
def small_ids(l: int, n_win: int) -> np.ndarray:
    """Rows shorter than 8 positions: random valid ids, a ragged last window, one empty frame."""
    rng = np.random.Generator(np.random.PCG64(l))
    ids = rng.integers(1, VOCAB, (n_win, 6, l)).astype(np.uint8)
    for f in range(6):
        ids[n_win - 1, f, max(l - 1 - f % 3, 1 if f else 0):] = 0    # (frame 0 of the last window: empty)
    if n_win > 2:
        ids[1, 4] = 0
    return ids


def ids_of(l: int, n_win: int) -> np.ndarray:
    import op_cases as oc
    return small_ids(l, n_win) if l < 8 else oc.edge_ids(l, n_win=n_win, vocab=VOCAB)


@dataclass
class Built:
    prog: object
    target: int                     # op index of the conv / element-wise op under test
    mask_op: int | None             # the MASK op the target writes under (None: no output mask)
    feeders: list
    finals: list                    # NMD_FINAL op indices in stage order
    ids: np.ndarray = field(default=None, repr=False)


EMB = 8


def build(c: Case) -> Built:
    from jaeger_amd import _lib as L
    w = _Writer(zlib.crc32(("f32:" + c.name).encode()))
    emb_w = c.cin if c.first else EMB
    emb_off = w.blob.add(w.rng.standard_normal((VOCAB, emb_w)).astype(np.float32))
    pad = L.PAD_SAME if c.padding == "same" else L.PAD_VALID
    slots = []

    def nmd():
        slots.append(len(slots))
        return w.stage(L.ST_NMD, arg=slots[-1])

    def stages():
        act = w.stage(L.ST_ACT, arg=ACT_GELU_TANH)
        st = [w.bias(c.cout)]
        if c.ep == "bn_act":
            st += [w.bn(c.cout), act]
        elif c.ep == "dyt":
            st += [w.dyt(c.cout, masked=c.out_mask), act]
        elif c.ep == "add_act":
            st += [w.bn(c.cout), w.stage(L.ST_ADD, arg=1), act]
        elif c.ep == "nmd1":
            st += [nmd(), w.bn(c.cout), act]
        elif c.ep == "nmd2":
            st += [nmd(), w.bn(c.cout), act, nmd()]
        else:
            assert c.ep == "bias", c.ep
        return st

    feeders, mask_op = [], None
    om = 1 if c.out_mask else L.JG_BUF_NONE
    if c.first:
        assert c.ep != "add_act"
        if c.out_mask:
            mask_op = w.op(L.OP_MASK, in_mask=L.JG_BUF_IDS, out_mask=1, k=c.k, stride=c.stride, dilation=c.dil, padding=pad,
                           mask_mode=c.mask_mode)
        target = w.op(L.OP_CONV, in_buf=L.JG_BUF_IDS, out_buf=2, in_mask=L.JG_BUF_IDS if c.mask_from_ids else L.JG_BUF_NONE,
                      out_mask=om, k=c.k, cin=c.cin, cout=c.cout, stride=c.stride, dilation=c.dil, padding=pad,
                      w_off=w.kernel(c.k, c.cin, c.cout, 2.0), b_off=emb_off, stages=stages())
    else:
        w.op(L.OP_MASK, in_mask=L.JG_BUF_IDS, out_mask=0, k=3, padding=L.PAD_SAME)
        feeders.append(w.op(L.OP_CONV, in_buf=L.JG_BUF_IDS, out_buf=0, in_mask=L.JG_BUF_IDS, out_mask=0, k=3, cin=EMB, cout=c.cin,
                            padding=L.PAD_SAME, w_off=w.kernel(3, EMB, c.cin, 2.0), b_off=emb_off,
                            stages=[w.bias(c.cin), w.stage(L.ST_ACT, arg=ACT_GELU_TANH)]))
        if c.ep == "add_act":
            assert c.stride == 1 and c.padding == "same"
            feeders.append(w.op(L.OP_CONV, in_buf=L.JG_BUF_IDS, out_buf=1, in_mask=L.JG_BUF_IDS, out_mask=0, k=3, cin=EMB,
                                cout=c.cout, padding=L.PAD_SAME, w_off=w.kernel(3, EMB, c.cout, 2.0), b_off=emb_off,
                                stages=[w.bias(c.cout)]))
        if c.out_mask:
            mask_op = w.op(L.OP_MASK, in_mask=0, out_mask=1, k=c.k, stride=c.stride, dilation=c.dil, padding=pad,
                           mask_mode=c.mask_mode)
        target = w.op(L.OP_CONV, in_buf=0, out_buf=2, in_mask=0, out_mask=om, k=c.k, cin=c.cin, cout=c.cout, stride=c.stride,
                      dilation=c.dil, padding=pad, w_off=w.kernel(c.k, c.cin, c.cout, 1.6), stages=stages())
    finals = [w.op(L.OP_NMD_FINAL, in_buf=2, in_mask=om, cout=c.cout, arg=slot, b_off=w.normal(c.cout, 0.3), f0=1e-7,
                   out_vec=L.VEC_NMD, vec_off=q * c.cout) for q, slot in enumerate(slots)]
    return _finish(w, c.cout, om, target, mask_op, feeders, finals, ids_of(c.l, c.n_win))


def _finish(w, width, om, target, mask_op, feeders, finals, ids) -> Built:
    from jaeger_amd import _lib as L
    from jaeger_amd.program import Program
    w.op(L.OP_POOL, in_buf=2, in_mask=om, cout=width, arg=L.POOL_AVG, out_vec=L.VEC_EMBEDDING)
    w.op(L.OP_DENSE, in_vec=L.VEC_EMBEDDING, out_vec=L.VEC_PREDICTION, cin=width, cout=2,
         w_off=w.blob.add((w.rng.standard_normal((width, 2)) * 0.1).astype(np.float32)), b_off=w.normal(2, 0.1))
    prog = Program(w.ops, w.blob.finish(), VOCAB, 2, False, len(finals) * width, width)
    return Built(prog, target, mask_op, feeders, finals, ids)


def build_ln(c: LnCase) -> Built:
    from jaeger_amd import _lib as L
    w = _Writer(zlib.crc32(("f32:" + c.name).encode()))
    emb_off = w.blob.add(w.rng.standard_normal((VOCAB, EMB)).astype(np.float32))
    mask_op = w.op(L.OP_MASK, in_mask=L.JG_BUF_IDS, out_mask=0, k=3, padding=L.PAD_SAME)
    feeders = [w.op(L.OP_CONV, in_buf=L.JG_BUF_IDS, out_buf=0, in_mask=L.JG_BUF_IDS, out_mask=0, k=3, cin=EMB, cout=c.c,
                    padding=L.PAD_SAME, w_off=w.kernel(3, EMB, c.c, 2.0), b_off=emb_off,
                    stages=[w.bias(c.c), w.stage(L.ST_ACT, arg=ACT_GELU_TANH)])]
    if c.kind == "ln_add_act":
        feeders.append(w.op(L.OP_CONV, in_buf=L.JG_BUF_IDS, out_buf=1, in_mask=L.JG_BUF_IDS, out_mask=0, k=3, cin=EMB, cout=c.c,
                            padding=L.PAD_SAME, w_off=w.kernel(3, EMB, c.c, 2.0), b_off=emb_off, stages=[w.bias(c.c)]))
    om = 0 if c.mask else L.JG_BUF_NONE
    ln = w.stage(L.ST_LN, arg=1 if c.use_masking else 0, f0=LN_EPS, p2=w.vec(c.c, 0.5, 1.6, signs=True), p3=w.normal(c.c, 0.4))
    act = w.stage(L.ST_ACT, arg=ACT_GELU_TANH)
    slots = []
    if c.kind == "ln":
        st = [ln]
    elif c.kind == "ln_add_act":
        st = [ln, w.stage(L.ST_ADD, arg=1), act]
    elif c.kind == "ln_nmd":
        slots.append(0)
        st = [ln, w.stage(L.ST_NMD, arg=0), act]
    elif c.kind == "bn_act":
        st = [w.bn(c.c), act]
    else:
        assert c.kind == "dyt", c.kind
        st = [w.dyt(c.c, masked=True), act]
    target = w.op(L.OP_ELTWISE, in_buf=0, out_buf=2, out_mask=om, cout=c.c, stages=st)
    finals = [w.op(L.OP_NMD_FINAL, in_buf=2, in_mask=om, cout=c.c, arg=slot, b_off=w.normal(c.c, 0.3), f0=1e-7,
                   out_vec=L.VEC_NMD, vec_off=q * c.c) for q, slot in enumerate(slots)]
    return _finish(w, c.c, om, target, mask_op if c.mask else None, feeders, finals, ids_of(c.l, c.n_win))
