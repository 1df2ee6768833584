"""The census of the split-f16 conv template's instantiations (tests/test_conv_instance_reference.py on the CPU,
tests/test_gpu_conv_instances.py on the GPU): one case per instance compiled into the shipped library.

An instance is ``Instance(part, k, ep, flat, cw, tanh)`` - the translation unit and the template arguments of
``conv_f16x3_kernel<K, EP, LUT, FLAT, CW, TANH>`` (``k`` 0: the first-layer table variant).  ``compiled_instances()`` restates
the switch tables at the bottom of ``jaeger_amd/csrc/jg_conv_f16_impl.h``; the CPU module parses that file and fails when the
two differ, so adding or removing an instantiation without touching this census fails a test.

A case is the smallest program that puts ONE conv (the target) on its instance: two first-layer convs that feed it from the
ids (its input of 64 channels, and the shortcut tensor when the pattern adds one), the target with the stage list of its
pattern, an NMD finish per tap, a reader that decides the store form, a pool and a dense layer.  The programs are written as
op lists (``jaeger_amd.program.Program``), not through a model config: a layer list cannot yield most stage lists.  The
target's pattern comes from its stage list by the matcher of ``jg_prepare.hip`` ("match the stage list against the compiled
pattern"); which tiling it takes from ``conv_f16_tiling`` (``jg_run.hip``), restated here as ``window_packed``.

Store forms: ``f16s`` - a split-f16 conv reads the target (the form of the residual stacks); ``f32`` - only an average pool
reads it; ``free`` - only the masked max pool reads it, nothing is stored and the check goes through ``embedding``;
``psplit`` - only stride-2 convs read it (a five-tap and a 1x1 one): stored phase-split, the two readers are checked as well.

Unreachable instances.  The epilogue builder of ``jg_prepare.hip`` folds every BIAS / BN stage into the pending affine and
flushes it only in front of a stage of another kind, so two affine entries are never adjacent: ``NORM1_AFF`` cannot follow the
leading affine without an NMD tap between them.  Every ``NORM1_AFF | ACT1`` instance (one per table: 18) is therefore dead;
the nearest program - BIAS, BN, ACT - runs on the ``ACT1`` instance of the same part, which ``UNREACHABLE`` names and the GPU
module shows.  A width between the tile widths on the 64-wide tile (48 channels) is refused by the placement ("conv width is
not 32, 64, 80..128 or a multiple of 128 channels"), so the narrow tiles see 64 and 32 channels only.
"""
from __future__ import annotations

import zlib
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

# JG_EP_* (jg_common.h), restated
N1, AFF1, DYT1, ADD, A1, N2, AFF2, DYT2, A2 = (1 << q for q in range(9))
RT = 0xFFFE
ACT_GELU_TANH, ACT_GELU_ERF, ACT_RELU = 1, 2, 3
ACT_NAME = {ACT_GELU_TANH: "tanh", ACT_GELU_ERF: "erf", ACT_RELU: "relu"}

#: the row tables (JG_ROW_CASES: k = 5 in part 1, k = 7 and 9 in part 2)
ROW = (0, N1, A1, AFF1 | A1, DYT1 | A1, ADD | A1, DYT1 | ADD | A1, ADD | A1 | N2 | AFF2 | A2,
       DYT1 | ADD | A1 | N2 | DYT2 | A2, N1 | AFF1 | A1, N1 | DYT1 | A1, ADD | A1 | AFF2 | A2, DYT1 | ADD | A1 | DYT2 | A2,
       A1 | AFF2, A1 | AFF2 | A2, N1 | AFF1 | ADD | A1, N1 | AFF1 | ADD | A1 | AFF2 | A2, ADD | A1 | N2, DYT1 | ADD | A1 | N2,
       DYT1, RT)
#: the window-packed table (part 3)
FLAT = (A1, AFF1 | A1, DYT1 | A1, ADD | A1, DYT1 | ADD | A1, ADD | A1 | N2 | AFF2 | A2, DYT1 | ADD | A1 | N2 | DYT2 | A2,
        A1 | AFF2, A1 | AFF2 | A2, ADD | A1 | AFF2 | A2, DYT1 | ADD | A1 | DYT2 | A2, ADD | A1 | N2, DYT1 | ADD | A1 | N2, RT)
#: the first-layer table variant (part 4; CW 128 and 129 each)
LUT = (0, N1, A1, AFF1 | A1, DYT1 | A1, N1 | AFF1 | A1, N1 | DYT1 | A1, A1 | AFF2, RT)
#: the run-time-geometry tables (parts 5 - 7: k = 5, both tilings; parts 8 - 13: k = 7 / 9, row-tiled)
GEOM = (0, A1, AFF1 | A1, ADD | A1, ADD | A1 | AFF2 | A2, N1 | AFF1 | A1, N1 | AFF1 | ADD | A1, ADD | A1 | N2 | AFF2 | A2,
        DYT1 | A1, DYT1 | ADD | A1, N1, ADD | A1 | N2, DYT1, DYT1 | ADD | A1 | N2, RT)
#: patterns with a tanh-GELU build beside the general one (k = 5, 128 channels, both tilings) / in the table variant (CW 128)
HOT = (A1, ADD | A1, ADD | A1 | N2 | AFF2 | A2)
HOT_LUT = N1 | AFF1 | A1

Instance = namedtuple("Instance", "part k ep flat cw tanh")
GEOM_PARTS = {5: (5, 64), 6: (5, 32), 7: (5, 129), 8: (7, 64), 9: (7, 32), 10: (7, 129), 11: (9, 64), 12: (9, 32), 13: (9, 129)}
PART_NAME = {1: "k5", 2: "k79", 3: "flat", 4: "lut", 5: "n64", 6: "n32", 7: "g128", 8: "k7n64", 9: "k7n32", 10: "k7g",
             11: "k9n64", 12: "k9n32", 13: "k9g"}


def ep_name(ep: int) -> str:
    if ep == RT:
        return "RUNTIME"
    names = ("NMD1", "AFF1", "DYT1", "ADD", "ACT1", "NMD2", "AFF2", "DYT2", "ACT2")
    return "+".join(n for q, n in enumerate(names) if ep >> q & 1) or "0"


def compiled_instances() -> set:
    """Every instantiation of the shipped library (experiment builds - PIPE, jg_conv_pc.hip, JG_EXPERIMENT / JG_STAMP - left out)."""
    s = set()
    for ep in ROW:
        s.add(Instance(1, 5, ep, False, 128, False))
        s.add(Instance(2, 7, ep, False, 128, False))
        s.add(Instance(2, 9, ep, False, 128, False))
    for ep in FLAT:
        s.add(Instance(3, 5, ep, True, 128, False))
    for ep in HOT:
        s.add(Instance(1, 5, ep, False, 128, True))
        s.add(Instance(3, 5, ep, True, 128, True))
    for ep in LUT:
        s.add(Instance(4, 0, ep, False, 128, False))
        s.add(Instance(4, 0, ep, False, 129, False))
    s.add(Instance(4, 0, HOT_LUT, False, 128, True))
    for part, (k, cw) in GEOM_PARTS.items():
        for ep in GEOM:
            s.add(Instance(part, k, ep, False, cw, False))
            if k == 5:
                s.add(Instance(part, k, ep, True, cw, False))
    return s


def instances_per_part() -> dict:
    n = {}
    for i in compiled_instances():
        n[i.part] = n.get(i.part, 0) + 1
    return dict(sorted(n.items()))


#: instance -> (the source rule that excludes it, the instance its nearest accepted program runs on)
UNREACHABLE = {
    i: ("jg_prepare.hip, epilogue builder: BIAS / BN fold into the pending affine, flushed only in front of a stage of another "
        "kind - NORM1_AFF needs an NMD tap behind the leading affine", i._replace(ep=A1))
    for i in compiled_instances() if i.ep == AFF1 | A1
}


# ---- the dispatch, restated ------------------------------------------------------------------------------------------------
def dispatch(*, lut: bool, k: int, cw: int, cout: int, ostride: int, tap_lo: int, tap_hi: int, psplit: bool, flat: bool, ep: int,
             act: int):
    """jg_launch_conv_f16 and the per-part switches: launch arguments -> Instance (None: no compiled instance)."""
    tanh = act == ACT_GELU_TANH
    if lut:
        if ep not in LUT:
            return None
        if cout != 128:
            return Instance(4, 0, ep, False, 129, False)
        return Instance(4, 0, ep, False, 128, ep == HOT_LUT and tanh)
    if k not in (5, 7, 9):
        return None
    if cw != 128:
        if cw not in (64, 32) or (k != 5 and flat) or ep not in GEOM:
            return None
        part = {(5, 64): 5, (5, 32): 6, (7, 64): 8, (7, 32): 9, (9, 64): 11, (9, 32): 12}[(k, cw)]
        return Instance(part, k, ep, flat, cw, False)
    if cout != 128 or ostride != 1 or tap_lo != 0 or tap_hi != k - 1 or psplit:
        if (k != 5 and flat) or ep not in GEOM:
            return None
        return Instance({5: 7, 7: 10, 9: 13}[k], k, ep, flat, 129, False)
    hot = k == 5 and ep in HOT and tanh
    if flat:
        if k != 5 or ep not in FLAT:
            return None
        return Instance(3, 5, ep, True, 128, hot)
    if ep not in ROW:
        return None
    return Instance(1 if k == 5 else 2, k, ep, False, 128, hot)


def window_packed(*, k: int, dil: int, cout: int, stride: int, l: int, nw: int, ep: int, strip_rows: bool, as_k5: bool,
                  psplit: bool, first: bool) -> bool:
    """conv_f16_tiling (jg_run.hip) for a SAME conv over six frames of ``l`` positions in a launch group of ``nw`` windows:
    window-packed when that takes at most 95 % of the row tiling's 256-position tiles."""
    if first or stride != 1:
        return False
    kk, kd = (5, (1 if k == 1 else dil)) if as_k5 else (k, dil)
    if kk != 5:
        return False
    if cout == 128 and not as_k5 and not psplit:
        if ep not in FLAT:
            return False
    elif ep not in GEOM:
        return False
    halo = (kk - 1) * kd
    pad_left = ((k - 1) * dil) // 2 + (max(1, (5 - k) // 2) * kd if as_k5 else 0)
    gap = max(pad_left, halo - pad_left)
    unit = 128 if strip_rows else 32
    wp = -(-6 * (l + gap) // unit) * unit
    flat_tiles = -(-nw * wp // 256)
    row_tiles = nw * 6 * -(-l // 256)
    return nw * wp < (1 << 24) and flat_tiles * 100 <= row_tiles * 95


# ---- cases -------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    want: Instance | None          # None: the placement must leave the conv on the exact-f32 kernel
    bits: int                      # the stage list is written from these JG_EP_* bits (BIAS first)
    k: int
    cout: int
    l: int
    act: int = ACT_GELU_TANH
    stride: int = 1
    dil: int = 1
    first: bool = False            # the target reads the ids (the table variant)
    store: str = "f16s"
    ep_rt: int | None = None       # want.ep == RT: the stage bits the kernel gets at run time
    n_win: int = 4
    chunk: int = 0
    mixed: bool = False            # the launch groups take different tilings
    proves: Instance | None = None  # the unreachable instance this case is the nearest accepted program of

    @property
    def ep(self) -> int:
        """What the matcher makes of ``bits``: NORM1_AFF without a tap in front folds into the leading affine."""
        return self.bits & ~AFF1 if (self.bits & AFF1 and not self.bits & N1) else self.bits


CIN = 64          # the target's input channels (32 would make a 32-channel case the fused small-window family)
ROW_L = (251, 507)        # one tile holding the row end / a tile edge inside the row
FLAT_L = (100, 300)       # six frames in 2.5 tiles / a row with a second tile


def _geometry(part: int, j: int, ep: int) -> dict:
    """The conv geometry of pattern number j of a part: lengths, dilations, widths, tap counts and strides alternate, so that
    every part sees its forms (256 channels as two launches, 96 on the 128-wide tile, 3-tap and 1x1 convs riding the five-tap
    kernel; stride 2 on every run-time-geometry part, narrow tiles included, with the two patterns that carry neither a
    shortcut nor a tap - the placement refuses those on a strided conv) across its patterns."""
    plain = not ep & (ADD | N1 | N2) and ep != RT          # (a strided conv takes no shortcut and no tap)
    if part in (1, 2):
        return {"cout": 128, "l": ROW_L[j % 4 == 3], "dil": (1, 3, 2)[j % 3]}
    if part == 3:
        return {"cout": 128, "l": FLAT_L[j % 4 == 3], "dil": (1, 3)[j % 2]}
    if part == 4:
        return {"l": ROW_L[j % 4 == 3]}
    k, cw = GEOM_PARTS[part]
    g = {"l": ROW_L[j % 4 == 3], "dil": (1, 2)[j % 2]}
    if cw != 129:
        g["cout"] = cw
        if j in (1, 12) and plain:                 # ACT1, DYT1: stride 2 on the narrow tiles too (row tiling only)
            g.update(stride=2, dil=1)
        elif k == 5 and j % 5 == 2:
            g["k"] = 3
    else:
        if j in (1, 12) and plain:                 # ACT1, DYT1
            g.update(cout=128, stride=2, dil=1)
        elif j in (4, 5, 9) and k == 5:
            g.update(cout=128, k=3)
        elif j in (0, 8, 10) and not ep & ADD:     # 0, DYT1 + ACT1, NMD1 (the tap's partial rows of two launches)
            g["cout"] = 256
        else:
            g["cout"] = 96
    return g


RT_BITS = {"row": N1 | A1, "geom": A1 | AFF2 | A2, "lut": DYT1, "two": N1 | AFF1 | ADD | A1 | N2, "two_lut": N1 | AFF1 | A1 | N2}


def _cases() -> list:
    out = []

    def add(want, bits, k, cout, l, **kw):
        flat = "flat" if (want is not None and want.flat) else "row"
        tag = kw.pop("tag", "")
        part = PART_NAME[want.part] if want is not None else "f32"
        act = kw.get("act", ACT_GELU_TANH)
        name = f"{part}-k{k}-{flat}-{ep_name(bits)}-{ACT_NAME[act]}-c{cout}-l{l}" + ("-s2" if kw.get("stride", 1) == 2 else "") + \
            (f"-{tag}" if tag else "")
        out.append(Case(name, want, bits, k, cout, l, **kw))

    for inst in sorted(compiled_instances()):
        if inst in UNREACHABLE or inst.ep == RT:
            continue
        table = {1: ROW, 2: ROW, 3: FLAT, 4: LUT}.get(inst.part, GEOM)
        j = table.index(inst.ep)
        g = _geometry(inst.part, j, inst.ep)
        general_beside_hot = (inst.part in (1, 3) and inst.k == 5 and inst.ep in HOT and not inst.tanh) or \
                             (inst.part == 4 and inst.cw == 128 and inst.ep == HOT_LUT and not inst.tanh)
        acts = (ACT_GELU_ERF, ACT_RELU) if general_beside_hot else (ACT_GELU_TANH,)
        for act in acts:
            if inst.part == 4:
                cout = 128 if inst.cw == 128 else (96, 64, 32)[j % 3]
                add(inst, inst.ep, (5, 7, 3)[j % 3], cout, g["l"], act=act, first=True, store=("f16s", "f32")[j % 2])
                continue
            l = g["l"] if not inst.flat else FLAT_L[j % 4 == 3]
            add(inst, inst.ep, g.get("k", inst.k), g["cout"], l, act=act, stride=g.get("stride", 1) if not inst.flat else 1,
                dil=g.get("dil", 1), store="f32" if general_beside_hot and act == ACT_RELU else "f16s")
            if inst.flat and g.get("stride", 1) == 2 and inst.cw == 129:   # (stride 2 has no window-packed tiling: 96 channels here)
                out[-1].cout = 96
                out[-1].name = out[-1].name.replace("-c128-", "-c96-")
    # the run-time pattern on every part and tiling: a canonical list without an instantiation, and two taps in one conv
    for inst in sorted(i for i in compiled_instances() if i.ep == RT):
        kind = "lut" if inst.part == 4 else "row" if inst.part in (1, 2, 3) else "geom"
        for which in (kind, "two_lut" if inst.part == 4 else "two"):
            bits = RT_BITS[which]
            cout = {128: 128, 129: 96, 64: 64, 32: 32}[inst.cw]
            l = FLAT_L[0] if inst.flat else ROW_L[0]
            add(inst, bits, inst.k or 5, cout, l, first=inst.part == 4, ep_rt=bits, tag="rt2" if which.startswith("two") else "rt1",
                store="f32" if which.startswith("two") else "f16s")
    # erf and ReLU on every part (the general builds beside the hot ones have theirs above)
    for part in range(1, 14):
        for act in (ACT_GELU_ERF, ACT_RELU):
            if part == 4:
                add(Instance(4, 0, A1, False, 129, False), A1, 5, 64, ROW_L[0], act=act, first=True, tag="act")
                continue
            k, cw = GEOM_PARTS.get(part, (5 if part != 2 else 7, 128))
            bits = ADD | A1 | AFF2 | A2 if part not in (1, 3) else A1 | AFF2 | A2
            inst = Instance(part, k, bits, part == 3, cw, False)
            add(inst, bits, k, {128: 128, 129: 96}.get(cw, cw), FLAT_L[0] if part == 3 else ROW_L[0], act=act, tag="act")
    # the store-free form (the masked max pool fused into the epilogue) on every part: the table variant included
    for part in range(1, 14):
        if part == 4:
            add(Instance(4, 0, N1 | AFF1 | A1, False, 128, True), N1 | AFF1 | A1, 7, 128, ROW_L[0], first=True, store="free", tag="free")
            continue
        k, cw = GEOM_PARTS.get(part, (5 if part != 2 else 9, 128))
        bits = ADD | A1 | N2 | AFF2 | A2
        inst = Instance(part, k, bits, part == 3, cw, part in (1, 3))
        add(inst, bits, k, {128: 128, 129: 96}.get(cw, cw), FLAT_L[1] if part == 3 else ROW_L[1], store="free", tag="free", dil=3)
    # phase-split store (the writer lands on the general tile whatever its width) and both phase-split read forms
    add(Instance(7, 5, A1, False, 129, False), A1, 5, 128, ROW_L[0], store="psplit", tag="psplit")
    add(Instance(7, 5, A1, False, 129, False), A1, 5, 128, 250, store="psplit", tag="psplit-even")
    add(Instance(5, 5, ADD | A1, True, 64, False), ADD | A1, 5, 64, FLAT_L[0], store="psplit", tag="psplit")
    # a DyT pattern with another activation than the tanh-GELU: the matcher refuses it, the conv stays on exact f32
    add(None, DYT1 | A1, 5, 128, ROW_L[0], act=ACT_GELU_ERF, tag="refused")
    add(None, DYT1 | ADD | A1 | DYT2 | A2, 5, 128, FLAT_L[0], act=ACT_RELU, tag="refused")
    # the nearest accepted program of every unreachable instance: BIAS, BN, ACT folds to ACT1
    for inst, (_, lands) in sorted(UNREACHABLE.items()):
        g = _geometry(inst.part, 1, A1) if inst.part != 4 else {}
        if inst.part == 4:
            add(lands, AFF1 | A1, 5, 128 if inst.cw == 128 else 96, ROW_L[0], act=ACT_GELU_ERF, first=True, tag="folds", proves=inst)
            continue
        cout = {128: 128, 129: 96}.get(inst.cw, inst.cw)
        act = ACT_GELU_ERF if inst.part in (1, 3) else ACT_GELU_TANH        # (tanh would land on the hot build of ACT1)
        add(lands, AFF1 | A1, inst.k, cout, FLAT_L[0] if inst.flat else ROW_L[0], act=act, tag="folds", proves=inst)
    # one forward whose launch groups take different tilings: 230 codons, groups of 2, 2 and 1 windows - 2 windows pack
    # into 11 tiles against 12 (91.7 %: window-packed), the last one into 6 against 6 (row-tiled)
    add(Instance(3, 5, ADD | A1, True, 128, True), ADD | A1, 5, 128, 230, n_win=5, chunk=2, mixed=True, tag="mixed")
    names = [c.name for c in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def as_k5(c: Case) -> bool:
    return not c.first and 1 <= c.k <= 4


def expected_instance(c: Case, nw: int | None = None):
    """The instance the restated placement and dispatch give the case's target in a launch group of ``nw`` windows."""
    if c.want is None:
        return None
    ep = c.ep
    table_ok = ep in (LUT if c.first else ROW)
    narrow_geo = not c.first and (c.cout != 128 or c.stride != 1 or as_k5(c))
    if c.act == ACT_GELU_TANH and (not table_ok or (narrow_geo and ep not in GEOM) or (ep & N1 and ep & N2)):
        ep = RT
    strip_rows = bool(c.bits & (N1 | N2)) or c.store == "free"
    psplit = c.store == "psplit"
    flat = window_packed(k=c.k, dil=c.dil, cout=c.cout, stride=c.stride, l=c.l, nw=nw or c.n_win, ep=ep, strip_rows=strip_rows,
                         as_k5=as_k5(c), psplit=psplit, first=c.first)
    cw = c.cout if (c.cout in (32, 64) and not c.first) else 128
    k5 = as_k5(c)
    lo = max(1, (5 - c.k) // 2) if k5 else 0
    return dispatch(lut=c.first, k=5 if k5 else c.k, cw=cw, cout=c.cout, ostride=c.stride, tap_lo=lo,
                    tap_hi=lo + c.k - 1 if k5 else c.k - 1, psplit=psplit, flat=flat, ep=ep, act=c.act)


# ---- programs ----------------------------------------------------------------------------------------------------------------
@dataclass
class Built:
    prog: object
    target: int                     # op index of the conv under test
    feeders: list                   # op indices of the first-layer convs
    readers: list                   # stride-2 readers of a phase-split store (checked like the target)
    finals: list                    # [(NMD_FINAL op index, partial slot)] in stage order
    pool: int
    ids: np.ndarray = field(default=None, repr=False)


class _Writer:
    def __init__(self, seed: int):
        from jaeger_amd.program import _Blob
        self.blob = _Blob()
        self.ops = []
        self.rng = np.random.Generator(np.random.PCG64(seed))

    def op(self, kind, **kw):
        from jaeger_amd import _lib as L
        op = L.JgOp()
        op.kind = kind
        for f in ("in_buf", "out_buf", "in_mask", "out_mask", "in_vec", "out_vec"):
            setattr(op, f, -1)
        op.w_off = op.b_off = -1
        op.stride = op.dilation = 1
        stages = kw.pop("stages", [])
        for key, v in kw.items():
            setattr(op, key, v)
        op.n_stages = len(stages)
        for q, st in enumerate(stages):
            op.stages[q] = st
        self.ops.append(op)
        return len(self.ops) - 1

    @staticmethod
    def stage(kind, arg=0, p0=-1, p1=-1, p2=-1, p3=-1, f0=0.0):
        from jaeger_amd import _lib as L
        st = L.JgStage()
        st.kind, st.arg, st.p0, st.p1, st.p2, st.p3, st.f0 = kind, arg, p0, p1, p2, p3, f0
        return st

    def vec(self, c, lo, hi, signs=False):
        v = self.rng.uniform(lo, hi, c)
        if signs:
            v = v * self.rng.choice((-1.0, 1.0), c)
        return self.blob.add(v.astype(np.float32))

    def normal(self, c, sd):
        return self.blob.add((self.rng.standard_normal(c) * sd).astype(np.float32))

    def kernel(self, k, cin, cout, gain=1.0):
        from jaeger_amd.program import pack_conv_kernel
        a = gain * np.sqrt(3.0 / (k * cin))
        return self.blob.add(pack_conv_kernel(self.rng.uniform(-a, a, (k, cin, cout)).astype(np.float32)))

    def bias(self, c):
        # (away from zero: where a window is all padding the output is the bias alone, and an F16S element of magnitude
        # 1e-4 sits on the format's 2^-25 storage rounding, which no bound in M can cover with a margin)
        from jaeger_amd import _lib as L
        return self.stage(L.ST_BIAS, p0=self.vec(c, 0.1, 0.4, signs=True))

    # Stand-in weights that keep every stage visible: a batch norm far from the identity (scale 0.5 .. 1.6 of either sign, mean
    # and shift of a few tenths), DyT gains that differ from channel to channel
    def bn(self, c):
        from jaeger_amd import _lib as L
        return self.stage(L.ST_BN, p0=self.normal(c, 0.4), p1=self.vec(c, 0.7, 1.4), p2=self.vec(c, 0.6, 1.5, signs=True),
                          p3=self.normal(c, 0.4))

    def dyt(self, c, masked=True):
        from jaeger_amd import _lib as L
        return self.stage(L.ST_DYT, arg=1 if masked else 0, f0=0.8, p2=self.vec(c, 0.5, 1.6, signs=True), p3=self.normal(c, 0.4))


VOCAB, EMB = 65, 8


def build(c: Case) -> Built:
    """The program of a case (see the module docstring) and its ids."""
    import op_cases as oc
    from jaeger_amd import _lib as L
    from jaeger_amd.program import Program
    w = _Writer(zlib.crc32(c.name.encode()))
    emb_off = w.blob.add(w.rng.standard_normal((VOCAB, EMB)).astype(np.float32))
    same = L.PAD_SAME
    act = lambda: w.stage(L.ST_ACT, arg=c.act)                                  # noqa: E731
    nmd_slots = []

    def target_stages(cout, add_slot):
        st = [w.bias(cout)]
        b = c.bits
        if b & N1:
            nmd_slots.append(len(nmd_slots))
            st.append(w.stage(L.ST_NMD, arg=nmd_slots[-1]))
        if b & AFF1:
            st.append(w.bn(cout))
        if b & DYT1:
            st.append(w.dyt(cout))
        if b & ADD:
            st.append(w.stage(L.ST_ADD, arg=add_slot))
        if b & A1:
            st.append(act())
        if b & N2:
            nmd_slots.append(len(nmd_slots))
            st.append(w.stage(L.ST_NMD, arg=nmd_slots[-1]))
        if b & AFF2:
            st.append(w.bn(cout))
        if b & DYT2:
            st.append(w.dyt(cout))
        if b & A2:
            st.append(act())
        assert len(st) <= L.JG_MAX_STAGES
        return st

    feeders, readers = [], []
    if c.first:
        assert not c.bits & ADD and c.stride == 1
        w.op(L.OP_MASK, in_mask=L.JG_BUF_IDS, out_mask=1, k=c.k, dilation=c.dil, padding=same)
        target = w.op(L.OP_CONV, in_buf=L.JG_BUF_IDS, out_buf=2, in_mask=L.JG_BUF_IDS, out_mask=1, k=c.k, cin=EMB, cout=c.cout,
                      dilation=c.dil, padding=same, w_off=w.kernel(c.k, EMB, c.cout, 2.0), b_off=emb_off,
                      stages=target_stages(c.cout, -1))
    else:
        w.op(L.OP_MASK, in_mask=L.JG_BUF_IDS, out_mask=0, k=3, padding=same)
        feeders.append(w.op(L.OP_CONV, in_buf=L.JG_BUF_IDS, out_buf=0, in_mask=L.JG_BUF_IDS, out_mask=0, k=3, cin=EMB, cout=CIN,
                            padding=same, w_off=w.kernel(3, EMB, CIN, 2.0), b_off=emb_off,
                            stages=[w.bias(CIN), w.stage(L.ST_ACT, arg=ACT_GELU_TANH)]))
        if c.bits & ADD:
            assert c.cout <= 128 and c.stride == 1
            feeders.append(w.op(L.OP_CONV, in_buf=L.JG_BUF_IDS, out_buf=1, in_mask=L.JG_BUF_IDS, out_mask=0, k=3, cin=EMB,
                                cout=c.cout, padding=same, w_off=w.kernel(3, EMB, c.cout, 2.0), b_off=emb_off,
                                stages=[w.bias(c.cout)]))
        w.op(L.OP_MASK, in_mask=0, out_mask=1, k=c.k, stride=c.stride, dilation=c.dil, padding=same)
        target = w.op(L.OP_CONV, in_buf=0, out_buf=2, in_mask=0, out_mask=1, k=c.k, cin=CIN, cout=c.cout, stride=c.stride,
                      dilation=c.dil, padding=same, w_off=w.kernel(c.k, CIN, c.cout, 1.6), stages=target_stages(c.cout, 1))
    finals = []
    for q, slot in enumerate(nmd_slots):
        finals.append((w.op(L.OP_NMD_FINAL, in_buf=2, in_mask=1, cout=c.cout, arg=slot, b_off=w.normal(c.cout, 0.3), f0=1e-7,
                            out_vec=L.VEC_NMD, vec_off=q * c.cout), slot))
    pool_buf, pool_mask, pool_c, pool_kind = 2, 1, c.cout, L.POOL_AVG
    if c.store == "free":
        pool_kind = L.POOL_MAX
    elif c.store == "f16s":
        w.op(L.OP_MASK, in_mask=1, out_mask=2, k=5, padding=same)
        w.op(L.OP_CONV, in_buf=2, out_buf=3, in_mask=1, out_mask=2, k=5, cin=c.cout, cout=64, padding=same,
             w_off=w.kernel(5, c.cout, 64), stages=[w.bias(64)])
        pool_buf, pool_mask, pool_c = 3, 2, 64
    elif c.store == "psplit":
        w.op(L.OP_MASK, in_mask=1, out_mask=2, k=5, stride=2, padding=same)
        readers.append(w.op(L.OP_CONV, in_buf=2, out_buf=3, in_mask=1, out_mask=2, k=5, cin=c.cout, cout=64, stride=2, padding=same,
                            w_off=w.kernel(5, c.cout, 64), stages=[w.bias(64), w.stage(L.ST_ACT, arg=ACT_GELU_TANH)]))
        w.op(L.OP_MASK, in_mask=1, out_mask=3, k=1, stride=2, padding=same)
        readers.append(w.op(L.OP_CONV, in_buf=2, out_buf=4, in_mask=1, out_mask=3, k=1, cin=c.cout, cout=64, stride=2, padding=same,
                            w_off=w.kernel(1, c.cout, 64), stages=[w.bias(64)]))
        pool_buf, pool_mask, pool_c = 3, 2, 64
    else:
        assert c.store == "f32", c.store
    pool = w.op(L.OP_POOL, in_buf=pool_buf, in_mask=pool_mask, cout=pool_c, arg=pool_kind, out_vec=L.VEC_EMBEDDING)
    w.op(L.OP_DENSE, in_vec=L.VEC_EMBEDDING, out_vec=L.VEC_PREDICTION, cin=pool_c, cout=2,
         w_off=w.blob.add((w.rng.standard_normal((pool_c, 2)) * 0.1).astype(np.float32)), b_off=w.normal(2, 0.1))
    prog = Program(w.ops, w.blob.finish(), VOCAB, 2, False, len(finals) * c.cout, pool_c)
    return Built(prog, target, feeders, readers, finals, pool, oc.edge_ids(c.l, n_win=c.n_win, vocab=VOCAB))
