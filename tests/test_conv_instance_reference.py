"""CPU tier of the split-f16 conv instance census (tests/conv_instance_cases.py; the GPU tier is
tests/test_gpu_conv_instances.py).

(a) What was compiled.  The host stubs of ``conv_f16x3_kernel<K, EP, LUT, FLAT, CW, TANH, PIPE>`` in the symbol table of the
    built library are exactly the census.  The four pattern lists of jg_common.h, from which the switches of
    jg_conv_f16_impl.h and the has_*_pattern predicates of jg_conv_f16.hip are generated, equal the census's, order included,
    and no second list survives in csrc.  Pinned as text: which predicate guards what (jg_prepare.hip, jg_run.hip), the
    ordered part selection of jg_launch_conv_f16 and the experiment guard of the pipelined build; the census's Python
    restatement of the dispatch maps onto the compiled set and reaches all of it.
(b) Every case compiles: jg_model_create's checks aside (GPU tier), oracle/ops.py evaluates every op of its program, the
    restated placement gives the target the instance the case is there for, and the split-f16 emulation of the target stays
    4x inside the bounds of op_cases.check on the case's own inputs.
(c) Every stage of every case is observable on the case's weights and inputs: the float64 reference with one epilogue stage
    dropped, with a DyT's gamma / beta swapped between two channels, or with an NMD tap read on the other side of a
    neighbouring stage leaves the bounds by at least 8x - so a dispatch to the wrong pattern cannot pass the GPU check.
"""
import copy
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import conv_instance_cases as cc
import op_cases as oc

CSRC = Path(__file__).resolve().parents[1] / "jaeger_amd" / "csrc"
READELF = "/opt/rocm/llvm/bin/llvm-readelf"      # ships with the compiler that built the library
EMU_MARGIN = 4.0
MUT_MARGIN = 8.0


def _norm(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return " ".join(text.replace("\\\n", " ").split())


@pytest.fixture(scope="module")
def ep_values():
    text = (CSRC / "jg_common.h").read_text()
    vals = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (JG_EP_\w+) (0x[0-9a-f]+)u", text)}
    assert vals["JG_EP_NMD1"] == cc.N1 and vals["JG_EP_NORM1_AFF"] == cc.AFF1 and vals["JG_EP_NORM1_DYT"] == cc.DYT1
    assert vals["JG_EP_ADD"] == cc.ADD and vals["JG_EP_ACT1"] == cc.A1 and vals["JG_EP_NMD2"] == cc.N2
    assert vals["JG_EP_NORM2_AFF"] == cc.AFF2 and vals["JG_EP_NORM2_DYT"] == cc.DYT2 and vals["JG_EP_ACT2"] == cc.A2
    assert vals["JG_EP_RUNTIME"] == cc.RT
    return vals


def _ep(expr: str, vals: dict) -> int:
    """A pattern expression of the sources (``JG_EP_ADD | JG_EP_ACT1``, ``0u``) as a number."""
    expr = expr.strip().strip("()").strip()
    if expr in ("0u", "0"):
        return 0
    v = 0
    for name in expr.split("|"):
        v |= vals[name.strip()]
    return v


def _part_of(k: int, lut: bool, flat: bool, cw: int) -> int:
    """The translation unit of an instantiation: the table variant is part 4, otherwise K, FLAT and CW decide."""
    if lut:
        return 4
    if cw == 128:
        return 3 if flat else {5: 1, 7: 2, 9: 2}[k]
    return {key: part for part, key in cc.GEOM_PARTS.items()}[(k, cw)]


@pytest.fixture(scope="module")
def compiled():
    """The instance set of the built library: the host stubs of the kernel template in its symbol table."""
    from jaeger_amd import _lib
    out = subprocess.run([READELF, "-s", "-W", "--demangle", str(_lib.lib_path())], check=True, capture_output=True, text=True).stdout
    stubs = re.findall(r"__device_stub__conv_f16x3_kernel<(\d+), (\d+)u, (true|false), (true|false), (\d+), (true|false), (true|false)>"
                       r"\(ConvHArgs\)", out)
    assert stubs, "no conv_f16x3_kernel stub in the symbol table of " + str(_lib.lib_path())
    assert len(set(stubs)) == len(stubs)
    assert all(pipe == "false" for *_, pipe in stubs), "a pipelined (JG_EXPERIMENT) instance in the shipped library"
    inst = set()
    for k, ep, lut, flat, cw, tanh, _ in stubs:
        k, ep, cw, lut, flat, tanh = int(k), int(ep), int(cw), lut == "true", flat == "true", tanh == "true"
        assert (k == 0) == lut, (k, lut)
        inst.add(cc.Instance(_part_of(k, lut, flat, cw), k, ep, flat, cw, tanh))
    assert len(inst) == len(stubs)
    return inst


@pytest.fixture(scope="module")
def lists(ep_values):
    """name -> [(X or H, pattern)] of the JG_CONV_PATTERNS_* lists of jg_common.h, in order."""
    text = re.sub(r"/\*.*?\*/", " ", (CSRC / "jg_common.h").read_text(), flags=re.S).replace("\\\n", " ")
    found = {}
    for name, args in (("ROW", "X, H"), ("FLAT", "X, H"), ("LUT", "X, H"), ("GEOM", "X")):
        body = re.search(rf"^#define JG_CONV_PATTERNS_{name}\({args}\)(.*)$", text, re.M).group(1)
        found[name] = [(kind, _ep(expr, ep_values)) for kind, expr in re.findall(r"\b([XH])\(([^()]*)\)", body)]
        assert re.sub(r"\b[XH]\([^()]*\)", "", body).strip() == "", name
    assert len(re.findall(r"^#define JG_CONV_PATTERNS_", text, re.M)) == 4
    return found


def test_every_translation_unit_is_one_part():
    mk = (CSRC / "Makefile").read_text()
    units = re.search(r"^CONV\s*:=\s*(.*)$", mk, re.M).group(1).split()
    parts = sorted(int(re.search(r"#define JG_CONV_PART (\d+)", (CSRC / u).read_text()).group(1)) for u in units)
    assert parts == list(range(1, 14)), parts
    assert "jg_conv_inst.hip" not in mk and not (CSRC / "jg_conv_inst.hip").exists()
    assert "jg_conv_pc.hip" in re.search(r"^EXP_ONLY\s*:=\s*(.*)$", mk, re.M).group(1).split()


def test_census_names_exactly_the_compiled_instances(compiled):
    assert compiled == cc.compiled_instances(), (sorted(compiled - cc.compiled_instances()), sorted(cc.compiled_instances() - compiled))
    assert cc.instances_per_part() == {1: 24, 2: 42, 3: 17, 4: 19, 5: 30, 6: 30, 7: 30, 8: 15, 9: 15, 10: 15, 11: 15, 12: 15, 13: 15}
    assert len(compiled) == 282
    covered = {c.want for c in cc.CASES if c.want is not None}
    assert covered | set(cc.UNREACHABLE) == compiled and not covered & set(cc.UNREACHABLE), \
        (sorted(compiled - covered - set(cc.UNREACHABLE)), sorted(covered - compiled))
    assert len(cc.UNREACHABLE) == 18
    for dead, (rule, lands) in cc.UNREACHABLE.items():
        assert "jg_prepare.hip" in rule and lands in compiled and lands not in cc.UNREACHABLE
        assert any(c.proves == dead and c.want == lands for c in cc.CASES), dead


def test_host_pattern_lists_equal_the_tables_they_guard(lists):
    for name, table in (("ROW", cc.ROW), ("FLAT", cc.FLAT), ("LUT", cc.LUT), ("GEOM", cc.GEOM)):
        assert [ep for _, ep in lists[name]] == list(table), name
    assert [ep for kind, ep in lists["ROW"] if kind == "H"] == list(cc.HOT)
    assert [ep for kind, ep in lists["FLAT"] if kind == "H"] == list(cc.HOT)
    assert [ep for kind, ep in lists["LUT"] if kind == "H"] == [cc.HOT_LUT]
    assert all(kind == "X" for kind, _ in lists["GEOM"])
    # no second list: the predicates expand the lists, nothing in csrc holds an array of patterns
    for src in sorted(CSRC.glob("*.h*")):
        text = _norm(src.read_text())
        assert not re.search(r"\b(?:unsigned|uint32_t)\s+\w+\s*\[\w*\]\s*=\s*\{[^}]*JG_EP_", text) and "PatternSet" not in text, src.name
    text = _norm((CSRC / "jg_conv_f16.hip").read_text())
    assert ("bool jg_conv_f16_has_pattern(unsigned ep, bool first_layer) { if (first_layer) { JG_CONV_PATTERNS_LUT(JG_IS, JG_IS) "
            "return false; } JG_CONV_PATTERNS_ROW(JG_IS, JG_IS) return false; }") in text
    assert "bool jg_conv_f16_has_flat_pattern(unsigned ep) { JG_CONV_PATTERNS_FLAT(JG_IS, JG_IS) return false; }" in text
    assert "bool jg_conv_f16_has_narrow_pattern(unsigned ep) { JG_CONV_PATTERNS_GEOM(JG_IS) return false; }" in text
    assert "#define JG_IS(p) if (ep == (p)) return true;" in text
    # which predicate guards what: the matcher and the tiling rule
    prep = _norm((CSRC / "jg_prepare.hip").read_text())
    assert "if (conv_ok && !jg_conv_f16_has_pattern(hp.ep, op.in_buf == JG_BUF_IDS)) {" in prep
    assert ("if (conv_ok && op.in_buf != JG_BUF_IDS && (op.cout != 128 || op.stride != 1 || hp.as_k5) && "
            "!jg_conv_f16_has_narrow_pattern(hp.ep))") in prep
    run = _norm((CSRC / "jg_run.hip").read_text())
    assert ("((op.cout == 128 && !hp.as_k5 && hp.ps_read == 0 && !hp.ps_store) ? jg_conv_f16_has_flat_pattern(hp.ep) : "
            "jg_conv_f16_has_narrow_pattern(hp.ep)) && (int64_t)nw * wp < (1 << 24) && flat_tiles * 100 <= row_tiles * 95") in run


def test_part_selection_of_the_launcher_and_its_restatements(compiled):
    text = _norm((CSRC / "jg_conv_f16.hip").read_text())
    body = text[text.index("int jg_launch_conv_f16("):]
    pieces = ["if (a.lut != nullptr) {", "return jg_conv_f16_part_lut(e, a, s, inst); }",
              "if (a.cw != HN) { if (a.k == 5) return a.cw == 64 ? jg_conv_f16_part_n64(e, a, s, inst) : jg_conv_f16_part_n32(e, a, s, inst);",
              "if (a.k == 7) return a.cw == 64 ? jg_conv_f16_part_x8(e, a, s, inst) : jg_conv_f16_part_x9(e, a, s, inst);",
              "return a.cw == 64 ? jg_conv_f16_part_x11(e, a, s, inst) : jg_conv_f16_part_x12(e, a, s, inst); }",
              "if (a.cout != HN || a.ostride != 1 || a.tap_lo != 0 || a.tap_hi != a.k - 1 || a.psplit) {",
              "if (a.k == 5) return jg_conv_f16_part_g128(e, a, s, inst);",
              "return a.k == 7 ? jg_conv_f16_part_x10(e, a, s, inst) : jg_conv_f16_part_x13(e, a, s, inst); }",
              "if (a.flat) {", "return jg_conv_f16_part_flat(e, a, s, inst); }",
              "if (a.k == 5) return jg_conv_f16_part_k5(e, a, s, inst); return jg_conv_f16_part_k79(e, a, s, inst);"]
    at = 0
    for p in pieces:
        assert p in body[at:], p
        at = body.index(p, at) + len(p)
    assert "constexpr int HM = 256, HN = 128," in text
    # the pipelined build is JG_EXPERIMENT only (the compiled fixture has checked that no stub of the library has PIPE set)
    impl = _norm((CSRC / "jg_conv_f16_impl.h").read_text())
    assert ("#ifdef JG_EXPERIMENT if (e->conv_pc == 2 && a.dil == 3 && a.cc_in % 2 == 0 && a.dbg == 0) return "
            "launch_ke<5, EP, FLAT, 128, true, true>(e, a, s, inst); #endif") in impl
    # the Python restatement maps onto the compiled set and reaches all of it
    image = set()
    for lut in (False, True):
        for k in (5, 7, 9):
            for cw, cout in ((128, 128), (128, 96), (64, 64), (32, 32)):
                for flat in (False, True):
                    for ep in set(cc.ROW) | set(cc.GEOM):
                        for act in (cc.ACT_GELU_TANH, cc.ACT_GELU_ERF):
                            got = cc.dispatch(lut=lut, k=k, cw=cw, cout=cout, ostride=1, tap_lo=0, tap_hi=k - 1, psplit=False,
                                              flat=flat, ep=ep, act=act)
                            if got is not None:
                                image.add(got)
    assert image == compiled, sorted(image ^ compiled)


def test_activation_kinds_and_forms_of_the_census():
    by_inst = {}
    for c in cc.CASES:
        by_inst.setdefault(c.want, []).append(c)
    for inst in cc.compiled_instances() - set(cc.UNREACHABLE):
        cases = by_inst[inst]
        beside_hot = not inst.tanh and ((inst.part in (1, 3) and inst.k == 5 and inst.ep in cc.HOT) or
                                        (inst.part == 4 and inst.cw == 128 and inst.ep == cc.HOT_LUT))
        acts = {c.act for c in cases}
        if beside_hot:                       # (the tanh-GELU goes to the hot build beside it)
            assert {cc.ACT_GELU_ERF, cc.ACT_RELU} <= acts and cc.ACT_GELU_TANH not in acts, inst
        else:
            assert cc.ACT_GELU_TANH in acts, inst
    for part in range(1, 14):
        mine = [c for c in cc.CASES if c.want is not None and c.want.part == part]
        assert {cc.ACT_GELU_ERF, cc.ACT_RELU} <= {c.act for c in mine if c.bits & cc.A1}, part
        assert any(c.store == "free" for c in mine), part
        rt = [c for c in mine if c.want.ep == cc.RT]
        assert any(c.ep_rt & cc.N1 and c.ep_rt & cc.N2 for c in rt) and any(not (c.ep_rt & cc.N1 and c.ep_rt & cc.N2) for c in rt), part
    assert sum(c.want is None for c in cc.CASES) == 2 and sum(c.mixed for c in cc.CASES) == 1
    assert {c.cout for c in cc.CASES if c.want is not None and c.want.cw == 129 and c.want.part != 4} >= {96, 128, 256}
    for part in cc.GEOM_PARTS:              # stride 2 on every part that takes it (the run-time-geometry tiles), by identity
        assert any(c.stride == 2 and c.want is not None and c.want.part == part for c in cc.CASES), part
    assert all(c.want.part in cc.GEOM_PARTS and not c.want.flat for c in cc.CASES if c.stride == 2)
    assert sum(c.store == "psplit" for c in cc.CASES) == 3
    assert all(4 <= c.n_win <= 6 for c in cc.CASES)


# ---- per-case checks ---------------------------------------------------------------------------------------------------------
def _worst(got, ref, M, gamma=oc.GAMMA):
    """op_cases.check's element criterion alone - max err / bound - without its table of offenders (a sort per call)."""
    return float((np.abs(got - ref) / (gamma * M + oc.REL * np.abs(ref) + oc.FLOOR)).max())


def _copy_op(op):
    return type(op).from_buffer_copy(bytes(op))


def _without(op, q):
    new = _copy_op(op)
    for s in range(q, op.n_stages - 1):
        new.stages[s] = op.stages[s + 1]
    new.n_stages = op.n_stages - 1
    return new


def _swapped(op, q):
    new = _copy_op(op)
    new.stages[q], new.stages[q + 1] = op.stages[q + 1], op.stages[q]
    return new


def _nmd_vectors(prog, built, state, taps, taps_m):
    from oracle import ops
    st = ops.State(state.ids, mask=dict(state.mask))
    st.part.update(taps)
    st.part_M.update(taps_m)
    res = [ops.run_op(prog, i, st) for i, _ in built.finals]
    return np.concatenate([r.out for r in res], axis=1), np.concatenate([r.M for r in res], axis=1)


def nmd_bounds(n_pos: int) -> tuple:
    """(gamma, RMS bound) of an NMD vector: the mean of n_pos tap values, each within op_cases.GAMMA x its magnitude of the
    float64 value (the conv's own bound), summed in f32 in any order (n 2^-24; RMS (sqrt n + 1) 2^-24, head_cases.gamma_sum)."""
    return oc.GAMMA + n_pos * 2.0 ** -24, oc.RMS_BOUND + (n_pos ** 0.5 + 1.0) * 2.0 ** -24


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_case_compiles_emulates_and_shows_every_stage(name):
    from oracle import ops
    c = cc.BY_NAME[name]
    # the restated placement and dispatch: the case selects its instance (and its tiling) by its own geometry
    if c.mixed:
        other = c.want._replace(part=1, flat=False)
        assert [cc.expected_instance(c, nw) for nw in (2, 2, 1)] == [c.want, c.want, other]
    else:
        assert cc.expected_instance(c) == c.want, (cc.expected_instance(c), c.want)
    b = cc.build(c)
    prog, op = b.prog, b.prog.ops[b.target]
    # every op evaluates (oracle/ops.py), one pass; the target's linear part once, its stage list and the mutations on it
    state = ops.State(ops.program_rows(prog, b.ids))
    for i in range(len(prog.ops)):
        if i == b.target:
            before = ops.State(state.ids, dict(state.act), dict(state.mask), dict(state.part), dict(state.vec))
            x = ops.conv_input(prog, op, state)
            wgt = ops.conv_weights(prog, op)
            lo, pl = ops.conv_geometry(x.shape[-2], op.k, op.stride, op.dilation, op.padding)
            y = ops.shifted_sum(x, wgt, op.stride, op.dilation, pl, lo)
            M0 = ops.shifted_sum(np.abs(x), np.abs(wgt), op.stride, op.dilation, pl, lo)
            base, base_m, (taps, taps_m) = ops._stages(prog, op, y, M0, state)
            ref = ops.OpOut(base, base_m, taps=taps, taps_M=taps_m)
            ops.apply(prog, i, state, ref)
        else:
            ops.apply(prog, i, state, ops.run_op(prog, i, state))
    assert set(state.vec) >= {ops.VEC_EMBEDDING, ops.VEC_PREDICTION} | ({ops.VEC_NMD} if b.finals else set())
    assert prog.ops[b.target - 1].kind == ops.OP_MASK and prog.ops[b.target - 1].out_mask == op.out_mask
    state = before                                                # (what the target read: the mask it writes under included)
    assert op.out_mask in state.mask
    emu = oc.emulate_conv(prog, b.target, state)
    res = oc.check(emu, ref.out, ref.M, f16s=True)
    assert res.worst * EMU_MARGIN <= 1.0 and res.rms * EMU_MARGIN <= oc.RMS_BOUND, res.report(f"{name} emulation")
    n_pos = base.shape[1] * base.shape[2]
    if b.finals:
        nmd_ref, nmd_m = _nmd_vectors(prog, b, state, taps, taps_m)
    kinds = [op.stages[q].kind for q in range(op.n_stages)]
    assert kinds[0] == ops.ST_BIAS
    for q in range(1, op.n_stages):
        if kinds[q] in (ops.ST_BN, ops.ST_DYT, ops.ST_ADD, ops.ST_ACT):
            mut, _, _ = ops._stages(prog, _without(op, q), y, M0, state)
            worst = _worst(mut, ref.out, ref.M)
            assert worst >= MUT_MARGIN, f"{name}: dropping stage {q} (kind {kinds[q]}) moves no element {MUT_MARGIN}x out: {worst:.3g}"
        if kinds[q] == ops.ST_DYT:
            p2 = copy.copy(prog)
            p2.blob = prog.blob.copy()
            g, be = op.stages[q].p2, op.stages[q].p3
            for off in (g, be):
                p2.blob[[off + 3, off + 4]] = prog.blob[[off + 4, off + 3]]
            mut, _, _ = ops._stages(p2, op, y, M0, state)
            worst = _worst(mut, ref.out, ref.M)
            assert worst >= MUT_MARGIN, f"{name}: DyT gamma / beta swapped between channels 3 and 4 moves nothing: {worst:.3g}"
        if kinds[q] == ops.ST_NMD:
            gamma, _ = nmd_bounds(n_pos)
            for other in (q - 1, q):                              # the tap read in front of the stage before it / behind the next
                if other + 1 >= op.n_stages:
                    continue
                _, _, (t2, tm2) = ops._stages(prog, _swapped(op, other), y, M0, state)
                got, _ = _nmd_vectors(prog, b, state, t2, tm2)
                worst = _worst(got, nmd_ref, nmd_m, gamma)
                assert worst >= MUT_MARGIN, f"{name}: NMD tap of stage {q} moved across stage {other if other < q else q + 1}: {worst:.3g}"
