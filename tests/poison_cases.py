"""Cases of tests/test_gpu_poison.py and the kernel census of tests/test_poison_census.py.

What is tested.  A model's workspace (activation, mask, partial-row and vector slots, the conversion / hyena / pool / merge
scratch) is allocated once, grows only and is shared by every call on the handle.  A kernel that reads a halo row, a padded
lane, a gap position of a window-packed tiling or a partial row that no kernel of the SAME launch group wrote computes from
what an earlier call left there - zero pages in a fresh process, which is the right padding value, so no per-op check against
a reference can see it.  ``JG_OPT_POISON_WORKSPACE`` (include/jaeger_hip.h) fills that workspace in front of every launch
group; a forward whose outputs do not depend on memory it does not own gives the same bits under every fill.

A case is ONE model handle and the id tensors it is run on.  The cases are those of the per-family case modules - they are
already the smallest programs that put one kernel at one edge - taken through those modules' own builders:

=================  ==============================================================================================================
family             source
=================  ==============================================================================================================
``conv``           every case of conv_instance_cases (each compiled split-f16 instance; the instance is asserted by identity)
``f32conv``        every case of f32_conv_cases (conv and layer norm / element-wise), exact f32
``resblock``       every case of resblock_cases: fused, refused (layer by layer) and the range-guard programs
``small``          fused_cases.SMALL_VARIANTS x small_input_sets (``small_net_kernel``)
``tab``            fused_cases.TAB_VARIANTS x both forms (``tab_mfma_kernel``, ``tab_conv_pool_kernel``) x their row sets
``head``           head_cases: the dense families (one launch group: tiled / narrow / plain; groups of 5, 5, 3: plain), the
                   odd-width pools and NMD finishes, vecmax, the OOD signals, the strand merge
``mixer``          the VARIANTS of the six row-mixer GPU modules and of the pool-and-merge module on their window kinds, and
                   their row-length lists around tile and chunk edges on the modules' minimal models
``tower``          the legacy tower at 665 codons (MAXPOOL1D on F16S and on f32 tensors, FRAMESUM), baseline500_dicodon_pos
                   (EMBED), brain_ln (a mixed program: layout conversions, the slot / scratch swap)
=================  ==============================================================================================================

Every case runs as one launch group and with a chunk that leaves a short last group (the previous group's windows then sit
behind this group's rows).  No case is larger than its source's.  Where the source module can tell which kernel ran
(``placement()``, ``tap_instance``, ``tap_variant``, one launch of a profiling class), the case's ``identity`` asserts it.
"""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable

import numpy as np

import conv_instance_cases as cc
import f32_conv_cases as fc32
import fused_cases as fu
import head_cases as hc
import op_cases as oc
import resblock_cases as rc

#: the fills, in the order every case goes through them (None: the option off)
OFF = None
SEQUENCE = (OFF, 0x00, 0xFF, 0x7B, OFF)
#: the fills under which the target op's tap is compared as well
TAP_SEQUENCE = (OFF, 0x00, 0xFF)
OUTPUTS = ("prediction", "reliability", "embedding", "nmd")


@dataclass
class Run:
    """One model handle, ready to run: ``inputs`` [(label, ids)], the chunk of the short-last-group pass (a function of the
    window count), the op whose tap names a failing op (None: nothing is stored, or the outputs are the op's), the chunk the
    identity is asserted at and the identity check itself (called behind the first, unpoisoned, tapped forward - or behind a
    plain forward when there is no tap - with (model, ids, forward))."""
    model: object
    inputs: list
    short: Callable[[int], int] = lambda n: max(n - 1, 1)
    tap: int | None = None
    id_chunk: int = 0
    identity: Callable | None = None


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    kernels: tuple = field(compare=False)          # the __global__ kernels the case is there to launch (the census)
    make: Callable = field(compare=False, repr=False)   # (device, n_cu) -> Run


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def _model(device, prog, precision=None):
    from jaeger_amd.engine import HipModel
    model = HipModel(device, prog)
    if precision is not None:
        model.set_precision(precision)
    return model


def _one_launch(device, cls_name):
    """identity: the forward is exactly one launch of the profiling class (one launch group)."""
    def check(model, ids, forward):
        device.profile_enable(True)
        try:
            before = device.profile_read()[cls_name]["launches"]
            forward()
            after = device.profile_read()[cls_name]["launches"]
        finally:
            device.profile_enable(False)
        assert after - before == 1, (cls_name, before, after)
    return check


def compile_cfg(cfg, weights):
    from jaeger_amd.plan import build_plan
    from jaeger_amd.program import compile_plan
    return compile_plan(build_plan(cfg), weights)


# ---- conv: every compiled split-f16 instance -------------------------------------------------------------------------------------
def _as_instance(d):
    return None if d is None else cc.Instance(d["part"], d["k"], d["ep"], d["flat"], d["cw"], d["tanh"])


def _conv_case(c) -> Case:
    def make(device, n_cu):
        from jaeger_amd import _lib as L
        device.set_fuse_resblock(False)
        b = cc.build(c)
        model = _model(device, b.prog)
        assert model.precision == "f16x3", model.describe()

        def identity(m, ids, forward):
            variant = m.tap_variant()
            inst = m.tap_instance(op=b.target) if c.store == "free" else m.tap_instance()
            if c.want is None:
                assert inst is None and variant & L.TAP_EXACT_F32, (inst, variant)
                return
            assert _as_instance(inst) == c.want, (inst, c.want)
            assert inst["mixed"] == c.mixed, inst
            if c.store != "free":
                assert bool(variant & L.TAP_WINDOW_PACKED) == c.want.flat and not variant & L.TAP_EXACT_F32, variant
                assert bool(variant & L.TAP_PHASE_SPLIT) == (c.store == "psplit"), variant

        # (a store-free conv cannot be tapped: the mask op in front of it is, and the conv's instance is recorded all the same)
        tap = b.target - 1 if c.store == "free" else b.target
        short = (lambda n: c.chunk) if c.chunk else (lambda n: max(n - 1, 1))
        return Run(model, [("ids", b.ids)], short, tap, c.chunk, identity)
    ks = ["mask_kernel", "dense_narrow_kernel" if (64 if c.store in ("f16s", "psplit") else c.cout) >= 64 else "dense_kernel"]
    ks.append("conv_f16x3_kernel" if c.want is not None else "conv_f32_kernel")
    if c.bits & (cc.N1 | cc.N2):
        ks.append("nmd_final_kernel")
    ks.append("pool_final_kernel" if c.store == "free" else "pool_kernel")
    return Case("conv/" + c.name, "conv", tuple(ks), make)


# ---- f32conv: the exact-f32 conv, the layer norm and the element-wise kernel ---------------------------------------------------------
def _f32_case(c, ln: bool) -> Case:
    def make(device, n_cu):
        from jaeger_amd import _lib as L
        device.set_fuse_resblock(False)
        b = fc32.build_ln(c) if ln else fc32.build(c)
        model = _model(device, b.prog, "f32")

        def identity(m, ids, forward):
            assert m.precision == "f32"
            if not ln:
                assert m.tap_variant() & L.TAP_EXACT_F32, m.tap_variant()

        chunk = getattr(c, "chunk", 0)
        short = (lambda n: chunk) if chunk else (lambda n: max(n - 1, 1))
        return Run(model, [("ids", b.ids)], short, b.target, chunk, identity)
    ks = ["conv_f32_kernel", "mask_kernel", "pool_kernel"]
    if ln:
        ks.append("layernorm_kernel" if c.is_ln else "eltwise_kernel")
    if (c.kind == "ln_nmd") if ln else c.n_taps:
        ks.append("nmd_final_kernel")
    return Case(("f32ln/" if ln else "f32conv/") + c.name, "f32conv", tuple(ks), make)


# ---- resblock: the fused residual-block kernels ----------------------------------------------------------------------------------------
def _resblock_case(c) -> Case:
    def make(device, n_cu):
        from jaeger_amd import _lib as L
        device.set_fuse_resblock(True)
        n_win = rc.launch_windows(c, n_cu) if c.launch is not None else None
        b = rc.build(c, n_win)
        model = _model(device, b.prog)
        assert model.precision == "f16x3", model.describe()
        bits = L.TAP_FUSED_RESBLOCK | L.TAP_F16S | L.TAP_PHASE_SPLIT | L.TAP_EXACT_F32

        def identity(m, ids, forward):
            got = m.tap_variant() & bits
            if c.fused:
                assert got == L.TAP_FUSED_RESBLOCK | L.TAP_F16S | (L.TAP_PHASE_SPLIT if c.store == "psplit" else 0), (c.name, hex(got))
            else:
                assert not got & L.TAP_FUSED_RESBLOCK and "fused residual block" not in m.describe(), (c.name, hex(got))

        short = (lambda n: c.chunk) if c.chunk else (lambda n: max(n - 1, 1))
        return Run(model, [("ids", b.ids)], short, b.conv2, c.chunk, identity)
    k = ("resblock64_kernel" if c.c == 64 else "resblock32_kernel") if c.fused else "conv_f16x3_kernel"
    return Case("resblock/" + c.name, "resblock", (k, "conv_f16x3_kernel", "mask_kernel", "pool_kernel"), make)


# ---- small / tab: the fused whole-row kernels --------------------------------------------------------------------------------------------
def _small_case(name: str) -> Case:
    def make(device, n_cu):
        _, _, prog = fu.compile_small(name)
        net = fu.SmallNet(prog)
        model = _model(device, prog, "f16x3")
        assert model.placement()["small_fused"], model.describe()
        return Run(model, list(fu.small_input_sets(net, n_cu=n_cu).items()), identity=_one_launch(device, "fused_small"))
    return Case("small/" + name, "small", ("small_net_kernel", "small_pool_final_kernel"), make)


def _tab_case(name: str, lds: bool) -> Case:
    def make(device, n_cu):
        _, _, prog = fu.compile_tab(name)
        model = _model(device, prog)
        device.set_table_net_lds(lds)
        assert "table-net" in model.describe(), model.describe()
        sets = {f"rows l={l}": fu.strand_ids(14, l) for l in (400, 131, 37)}
        sets["multi-row set l=200"] = fu.strand_multirow_ids(200, n_cu)
        if not lds and name == "dvf500":
            sets["rows l=1200"] = fu.strand_ids(8, 1200)          # (asked for the matrix cores: only the LDS form fits the row)
        return Run(model, list(sets.items()), identity=_one_launch(device, "table"))
    ks = ("tab_conv_pool_kernel",) if lds else ("tab_mfma_kernel", "tab_conv_pool_kernel")
    return Case(f"tab/{name}-{'lds' if lds else 'mfma'}", "tab", ks + ("strand_merge_kernel",), make)


# ---- head: the vector head's kernels -----------------------------------------------------------------------------------------------------
def _head_short(n):
    return hc.CHUNK                       # 13 windows in groups of 5, 5 and 3 (no tile of 8: wide layers take the plain kernel)


@functools.lru_cache(maxsize=None)
def _dense_family(name, bias):
    return hc.dense_family(name, bias)


@functools.lru_cache(maxsize=None)
def _vecmax_family(name):
    return hc.vecmax_family(name)


@functools.lru_cache(maxsize=None)
def _strand_family():
    return hc.strand_family()


def _head_ids():
    return oc.edge_ids(hc.CODONS, n_win=hc.ROWS)


def _dense_kernels(name):
    width, layers = hc.DENSE_FAMILIES[name]
    cin, ks = width, set()
    for units, _ in layers:
        ks.add({"tiled": "dense_tiled_kernel", "narrow": "dense_narrow_kernel", "plain": "dense_kernel"}[hc.dense_kernel(hc.ROWS, cin, units)])
        ks.add({"narrow": "dense_narrow_kernel"}.get(hc.dense_kernel(hc.CHUNK, cin, units), "dense_kernel"))
        cin = units
    return tuple(sorted(ks))


def _dense_case(name: str, bias: bool) -> Case:
    def make(device, n_cu):
        from oracle import ops
        fam = _dense_family(name, bias)
        prog = fam.progs[max(fam.progs)]                      # the whole head: every layer of the family in one program

        def identity(m, ids, forward):                       # (the launch rule, restated: the family holds the shapes it is there for)
            for i in hc.head_chain(prog, ops.VEC_PREDICTION):
                op = prog.ops[i]
                kernel = hc.dense_kernel(hc.ROWS, op.cin, op.cout)
                assert hc.DENSE_WANT.get((op.cin, op.cout), kernel) == kernel, (op.cin, op.cout, kernel)
                assert (op.b_off >= 0) == bias
        return Run(_model(device, prog, "f32"), [("ids", _head_ids())], _head_short, identity=identity)
    return Case(f"head/dense-{name}-{'bias' if bias else 'nobias'}", "head", _dense_kernels(name) + ("pool_kernel",), make)


def _pool_case(width: int, pooling: str, masked: bool) -> Case:
    def make(device, n_cu):
        prog = hc.Family({"pool": hc.pool_cfg(width, pooling, masked)}).progs["pool"]
        inputs = [(f"l={l}", oc.edge_ids(l, n_win=hc.ROWS)) for l in (hc.CODONS, 3)]
        return Run(_model(device, prog, "f32"), inputs, _head_short)
    return Case(f"head/pool-w{width}-{pooling}-{'masked' if masked else 'unmasked'}", "head", ("pool_kernel", "nmd_final_kernel"), make)


def _vecmax_case(name: str, which: str) -> Case:
    def make(device, n_cu):
        return Run(_model(device, _vecmax_family(name).progs[which], "f32"), [("ids", _head_ids())], _head_short)
    return Case(f"head/vecmax-{name.replace(' ', '_')}-{which}", "head", ("vecmax_kernel", "nmd_final_kernel") if which == "max" else ("nmd_final_kernel",), make)


def _ood_case(name: str) -> Case:
    def make(device, n_cu):
        fam, ids, _ = hc.ood_family(name)
        return Run(_model(device, fam.progs["ood"], "f32"), [("ids", ids)], _head_short)
    return Case("head/ood-" + name.replace(" ", "_"), "head", ("oodsig_kernel",), make)


STRAND_PROGS = ("concat", "average", "sum", "max", "prefix", "identity")


def _strand_case(which: str, n_win: int) -> Case:
    def make(device, n_cu):
        prog = _strand_family().progs[which]
        return Run(_model(device, prog, "f32"), [("ids", fu.strand_ids(n_win, hc.STRAND_BASES))])
    return Case(f"head/strands-{which}-{n_win}win", "head", ("strand_merge_kernel", "dense_tiled_kernel", "dense_kernel"), make)


# ---- mixer: the row mixers and the pool-and-merge op ------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Mixer:
    key: str
    module: str                  # the GPU test module: its VARIANTS / variant() / ids / minimal model / row lengths
    reference: str               # the module whose random_weights the GPU module uses
    kernels: tuple
    describe: str                # what describe() says of the op


MIXERS = (
    Mixer("frameattn", "test_gpu_frameattn", "attention_reference", ("frameattn_kernel",), "frame attention"),
    Mixer("localattn", "test_gpu_localattn", "local_attention_reference", ("localattn_kernel",), "local attention"),
    Mixer("axialattn", "test_gpu_axialattn", "axial_attention_reference", ("lengthattn_kernel", "frameattn_kernel"), "length attention"),
    Mixer("hyena", "test_gpu_hyena", "hyena_reference", ("hyena_proj_kernel", "hyena_conv_kernel", "hyena_out_kernel"), "hyena"),
    Mixer("bilstm", "test_gpu_bilstm", "bilstm_reference", ("bilstm_kernel",), "bilstm"),
    Mixer("msconv", "test_gpu_multiscale", "multiscale_reference", ("msconv_kernel", "msmask_kernel"), "multi-scale conv"),
    Mixer("poolvec", "test_gpu_branches", "branches_reference", ("poolvec_sweep_kernel", "poolvec_last_kernel"), "pool-and-merge"),
)


def _mod(name):
    import importlib
    return importlib.import_module(name)


def mixer_variants(mx: Mixer) -> tuple:
    t, r = _mod(mx.module), _mod(mx.reference)
    return tuple(getattr(t, "VARIANTS", None) or r.VARIANTS)


def _mixer_variant_cfg(mx: Mixer, name: str):
    t, r = _mod(mx.module), _mod(mx.reference)
    return (getattr(t, "variant", None) or r.variant)(name)


def _mixer_inputs(mx: Mixer, name: str, cfg) -> list:
    """The window kinds of the mixer's own GPU module, through that module's id generators."""
    t, r = _mod(mx.module), _mod(mx.reference)
    if mx.key == "frameattn":
        return [(kind, t.encode(*t.windows(kind))) for kind in t.KINDS]
    if mx.key == "localattn":
        half = [int(a["window_size"]) // 2 for _, kind, a in r.attention_layers(cfg) if kind == r.LOCAL][0]
        return [(kind, t.ids_of(kind, half)) for kind in r.KINDS]
    if mx.key == "axialattn":
        return [(kind, t.ids_of(kind)) for kind in r.KINDS]
    if mx.key == "hyena":
        return [(kind, t.ids_of(kind, name)) for kind in r.KINDS]
    if mx.key == "bilstm":
        return [(kind, r.ids_of(kind, name)) for kind in r.KINDS]
    if mx.key == "msconv":
        return [(kind, r.ids_of(kind)) for kind in r.KINDS]
    return [(kind, r.ids_of(kind)) for kind in r.WINDOW_KINDS]


def _mixer_case(mx: Mixer, name: str, precision: str) -> Case:
    """``precision``: "own" - the program's default arithmetic (split-f16 where its convs have such a program) - or "f32"."""
    def make(device, n_cu):
        from jaeger_amd import _lib as L
        device.set_fuse_resblock(True)
        cfg = _mixer_variant_cfg(mx, name)
        prog = compile_cfg(cfg, _mod(mx.reference).random_weights(cfg))
        model = _model(device, prog, None if precision == "own" else "f32")
        assert mx.describe in model.describe() and not model.placement()["small_fused"], model.describe()
        kinds = {"frameattn": (L.OP_FRAMEATTN,), "localattn": (L.OP_LOCALATTN,), "axialattn": (L.OP_LENGTHATTN,), "hyena": (L.OP_HYENA,),
                 "bilstm": (L.OP_BILSTM,), "msconv": (L.OP_MSCONV,), "poolvec": ()}[mx.key]
        ops = [i for i, op in enumerate(prog.ops) if op.kind in kinds]

        def identity(m, ids, forward):                       # a row mixer: one arithmetic, one layout
            bits = m.tap_variant()
            assert bits & L.TAP_EXACT_F32 and not bits & (L.TAP_F16S | L.TAP_PHASE_SPLIT), bits
        return Run(model, _mixer_inputs(mx, name, cfg), lambda n: 2, ops[-1] if ops else None, 0, identity if ops else None)
    return Case(f"mixer/{mx.key}-{name}-{precision}", "mixer", mx.kernels, make)


def mixer_lengths(mx: Mixer) -> list:
    """[(row length, windows)] of the mixer module's row-length list (around its tile and chunk edges)."""
    from jaeger_amd import _lib as L
    t = _mod(mx.module)
    if mx.key == "localattn":
        return [(l, 3) for l, half in t._geometry_cases() if half == 8]
    if mx.key == "axialattn":
        return [(l, 3) for l in t._geometry_lengths()]
    if mx.key == "hyena":
        return [(l, 1 if l > 300 else 3) for l in t._lengths()]
    if mx.key == "bilstm":
        return list(t._cases())
    if mx.key == "msconv":
        return [(l, 3) for l in (1, 2, L.MSCONV_TILE - 1, L.MSCONV_TILE, L.MSCONV_TILE + 1, 2 * L.MSCONV_TILE - 1, 2 * L.MSCONV_TILE,
                                 2 * L.MSCONV_TILE + 1, 166)] + [(65, 1), (65, 7)]
    if mx.key == "poolvec":
        return [(l, 3) for l in (1, 2, 63, 64, 65, 165)] + [(65, 1), (65, 70)]
    return []                                                   # (frame attention mixes across the frames: no row-length list)


def _mixer_length_case(mx: Mixer) -> Case:
    """The mixer module's minimal model (exact f32, as there) on ONE handle over its whole row-length list, shortest row last but
    one: the calls follow each other on buffers sized by the longest."""
    def make(device, n_cu):
        t, r = _mod(mx.module), _mod(mx.reference)
        cfg = {"localattn": lambda: t.minimal_cfg(16), "hyena": lambda: t.minimal_cfg(output_projection=True),
               "poolvec": lambda: t.conv_branches_cfg()}.get(mx.key, lambda: t.minimal_cfg())()
        model = _model(device, compile_cfg(cfg, r.random_weights(cfg)), "f32")
        ragged = t._ragged_ids if hasattr(t, "_ragged_ids") else _mod("test_gpu_hyena")._ragged_ids
        lengths = sorted(mixer_lengths(mx), key=lambda ln: (-ln[0] * ln[1]))        # the largest call first: it sizes the buffers
        return Run(model, [(f"l={l} n={n}", ragged(l, n)) for l, n in lengths], lambda n: 2 if n > 2 else 1)
    return Case(f"mixer/{mx.key}-row-lengths", "mixer", mx.kernels, make)


# ---- tower: the ordinary kernels no case above reaches ---------------------------------------------------------------------------------
def _legacy_case(precision: str) -> Case:
    def make(device, n_cu):
        from conftest import GOLDEN
        from jaeger_amd import _lib as L
        from jaeger_amd import legacy
        device.set_fuse_resblock(True)
        prog = legacy.compile_legacy(legacy.load_legacy_h5(GOLDEN / "legacy_data" / "models" / "default" / "WRes_1024.h5"))
        model = _model(device, prog, precision)
        pools = [i for i, op in enumerate(prog.ops) if op.kind == L.OP_MAXPOOL1D]
        assert pools and any(op.kind == L.OP_FRAMESUM for op in prog.ops)

        def identity(m, ids, forward):                       # the max pool runs on F16S tensors in split-f16, on f32 ones in exact f32
            assert m.precision == precision and bool(m.tap_variant() & L.TAP_F16S) == (precision == "f16x3"), m.tap_variant()
        return Run(model, [("l=665", oc.edge_ids(665, n_win=6, vocab=prog.vocab))], tap=pools[-1], identity=identity)
    ks = ("maxpool1d_f16s_kernel" if precision == "f16x3" else "maxpool1d_kernel", "framesum_kernel", "eltwise_kernel")
    return Case(f"tower/legacy-665-{precision}", "tower", ks, make)


def _dicodon_case(precision: str) -> Case:
    def make(device, n_cu):
        from jaeger_amd import _lib as L
        device.set_fuse_resblock(True)
        _, _, prog = oc.compile_model("baseline500_dicodon_pos")
        assert prog.ops[0].kind == L.OP_EMBED
        model = _model(device, prog, precision)
        return Run(model, [("l=300", oc.edge_ids(300, n_win=12, vocab=prog.vocab))], tap=0)
    return Case(f"tower/baseline500_dicodon_pos-{precision}", "tower", ("embed_pos_kernel",), make)


def _mixed_case() -> Case:
    def make(device, n_cu):
        device.set_fuse_resblock(True)
        _, _, prog = oc.compile_model("brain_ln")
        model = _model(device, prog)

        def identity(m, ids, forward):
            pl = m.placement()
            assert m.precision == "f16x3" and pl["layout_conversions"] >= 1 and 0 < pl["convs_f16x3"], pl
        return Run(model, [("l=500", oc.edge_ids(500, n_win=5))], identity=identity)
    return Case("tower/brain_ln-layout-conversions", "tower", ("f32_to_f16s_kernel", "f16s_to_f32_kernel", "layernorm_kernel"), make)


# ---- the list ----------------------------------------------------------------------------------------------------------------------------
def _cases() -> list:
    out = [_conv_case(c) for c in cc.CASES]
    out += [_f32_case(c, False) for c in fc32.CASES] + [_f32_case(c, True) for c in fc32.LN_CASES]
    out += [_resblock_case(c) for c in rc.CASES if not c.guard]
    out += [_small_case(n) for n in fu.SMALL_VARIANTS]
    out += [_tab_case(n, lds) for n in fu.TAB_VARIANTS for lds in (False, True)]
    out += [_dense_case(n, bias) for n in hc.DENSE_FAMILIES for bias in (True, False)]
    out += [_pool_case(w, p, m) for w in hc.POOL_WIDTHS for p in ("average", "max") for m in (True, False)]
    out += [_vecmax_case(n, which) for n in hc.VECMAX_CASES for which in ("max", "concat")]
    out += [_ood_case(n) for n in hc.OOD_CASES]
    out += [_strand_case(which, n) for which in STRAND_PROGS for n in hc.STRAND_WINDOWS]
    for mx in MIXERS:
        out += [_mixer_case(mx, name, precision) for name in mixer_variants(mx) for precision in ("own", "f32")]
        if mx.key != "frameattn":
            out.append(_mixer_length_case(mx))
    out += [_legacy_case(p) for p in ("f16x3", "f32")] + [_dicodon_case(p) for p in ("f16x3", "f32")] + [_mixed_case()]
    names = [c.name for c in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
#: the range-guard programs of resblock_cases: a first call that falls back inside the call (tests/test_gpu_poison.py runs it
#: under every fill on a handle of its own, against a handle set to exact f32 before its first call)
GUARD_CASES = ["resblock-guard/" + c.name for c in rc.GUARD]
#: the predict_windows cases (the brain model at 1500 bp, seven windows) and the call histories; named here for the census
PREDICT_CASES = ["predict/whole-buffer", "predict/streamed-dust"]
HISTORY_FAMILIES = ("brain", "pyramid", "baseline500", "dvf500", "legacy", "mixer_chain")
HISTORY_CASES = ["history/" + f for f in HISTORY_FAMILIES] + ["history/range-guard-fallback"]
ALL_NAMES = [c.name for c in CASES] + GUARD_CASES + PREDICT_CASES + HISTORY_CASES


def families() -> dict:
    n = {}
    for c in CASES:
        n[c.family] = n.get(c.family, 0) + 1
    return n


# ---- the kernel census -------------------------------------------------------------------------------------------------------------------
CSRC = Path(__file__).resolve().parents[1] / "jaeger_amd" / "csrc"


def source_kernels() -> dict:
    """name -> file of every ``__global__`` function of jaeger_amd/csrc/*.hip and *.h (comments stripped)."""
    found = {}
    for path in sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.h"))):
        text = re.sub(r"//[^\n]*", "", path.read_text())
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        for m in re.finditer(r"__global__\b[^;{}]*?\bvoid\s+(\w+)\s*\(", text, flags=re.S):
            found.setdefault(m.group(1), path.name)
    return found


def _launching(kernel: str) -> list:
    return [c.name for c in CASES if kernel in c.kernels]


_NOT_MODEL = "reads the caller's base buffer and job tables and per-call stream-ordered buffers it fills itself: no model workspace"
#: kernel -> the names of the cases that launch it (a list), or one sentence on why it reads no grow-only workspace (a string)
KERNELS = {
    # the forward's kernels
    "conv_f16x3_kernel": _launching("conv_f16x3_kernel"),
    "conv_f32_kernel": _launching("conv_f32_kernel"),
    "mask_kernel": _launching("mask_kernel"),
    "eltwise_kernel": _launching("eltwise_kernel"),
    "layernorm_kernel": _launching("layernorm_kernel"),
    "pool_kernel": _launching("pool_kernel"),
    "pool_final_kernel": _launching("pool_final_kernel"),
    "nmd_final_kernel": _launching("nmd_final_kernel"),
    "dense_kernel": _launching("dense_kernel"),
    "dense_narrow_kernel": _launching("dense_narrow_kernel"),
    "dense_tiled_kernel": _launching("dense_tiled_kernel"),
    "oodsig_kernel": _launching("oodsig_kernel"),
    "vecmax_kernel": _launching("vecmax_kernel"),
    "strand_merge_kernel": _launching("strand_merge_kernel"),
    "maxpool1d_kernel": _launching("maxpool1d_kernel"),
    "maxpool1d_f16s_kernel": _launching("maxpool1d_f16s_kernel"),
    "framesum_kernel": _launching("framesum_kernel"),
    "embed_pos_kernel": _launching("embed_pos_kernel"),
    "f32_to_f16s_kernel": _launching("f32_to_f16s_kernel"),
    "f16s_to_f32_kernel": _launching("f16s_to_f32_kernel"),
    "resblock32_kernel": _launching("resblock32_kernel"),
    "resblock64_kernel": _launching("resblock64_kernel"),
    "small_net_kernel": _launching("small_net_kernel"),
    "small_pool_final_kernel": _launching("small_pool_final_kernel"),
    "tab_mfma_kernel": _launching("tab_mfma_kernel"),
    "tab_conv_pool_kernel": _launching("tab_conv_pool_kernel"),
    "frameattn_kernel": _launching("frameattn_kernel"),
    "localattn_kernel": _launching("localattn_kernel"),
    "lengthattn_kernel": _launching("lengthattn_kernel"),
    "hyena_proj_kernel": _launching("hyena_proj_kernel"),
    "hyena_conv_kernel": _launching("hyena_conv_kernel"),
    "hyena_out_kernel": _launching("hyena_out_kernel"),
    "bilstm_kernel": _launching("bilstm_kernel"),
    "msconv_kernel": _launching("msconv_kernel"),
    "msmask_kernel": _launching("msmask_kernel"),
    "poolvec_sweep_kernel": _launching("poolvec_sweep_kernel"),
    "poolvec_last_kernel": _launching("poolvec_last_kernel"),
    # launched by jg_predict_windows in front of the forward, on input buffers
    "encode_kernel": list(PREDICT_CASES),
    "dust_kernel": ["predict/streamed-dust"],
    # not part of a model's forward
    "embed_kernel": "No launcher of the library calls jg_launch_embed: the EMBED op runs on embed_pos_kernel.",
    "conv_pc_kernel": "Compiled into the experiment library only (JG_OPT_CONV_PC is refused by the shipped one), so no shipped forward launches it.",
    "box_mfma_kernel": "The calibration loop of jg_box_calibrate: register operands and a stamp buffer of its own, no model.",
    "align_kernel": "Pairwise alignment of att sites: " + _NOT_MODEL + ".",
    "termini_kernel": "Terminal-repeat scan: " + _NOT_MODEL + ".",
    "termini_fast_kernel": "Terminal-repeat scan, packed pass: " + _NOT_MODEL + ".",
    "termini_finish_kernel": "Terminal-repeat scan, end cells of the packed pass: " + _NOT_MODEL + ".",
    "termini_single_kernel": "Terminal-repeat scan, one alignment a workgroup: " + _NOT_MODEL + ".",
    "termini_seed_kernel": "Terminal-repeat scan, the 13-mer probe: " + _NOT_MODEL + ".",
}
