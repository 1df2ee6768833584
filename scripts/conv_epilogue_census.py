#!/usr/bin/env python3
"""Static instruction census of the k = 5 split-f16 conv kernels (jg_conv_f16_k5.hip).

Compiles the translation unit to gfx950 assembly with the Makefile's FLAGS in a temporary
directory (device code only, about a minute, no GPU) and prints, per kernel symbol:

  * MFMAs;
  * vector + memory instructions (v_* other than MFMAs, ds_*, global_*, scratch_*, buffer_*,
    flat_*) before / inside / behind the MFMA region, the part behind it split into the
    epilogue arithmetic, the pool branch, the store section and the pass tail;
  * v_readlane / v_writelane per region (spilled SGPRs live in VGPR lanes: every use of one
    is a lane read in the vector pipe);
  * SGPR / VGPR spill counts and scratch bytes from the code object metadata.

How the text is cut (the cuts are at labels and branches of the assembly, so they move with
the compiler's block layout; the numbers are static counts of the text, not executed counts):

  MFMA region    first label block that holds an MFMA .. last label block that holds one
  steady body    the blocks of the deepest loop that holds MFMAs, by the compiler's own loop
                 comments: the chunk loop.  What is left of the region is its entry and the
                 peeled copy for the tile's last chunk.
  store section  first .. last label block behind the region that holds a global_store_dwordx4
  pool branch    behind the region and outside the store section: first .. last label block that
                 holds the pool's -inf literal (the branch's mask loads in front of it stay with
                 the epilogue)
  epilogue       from the end of the region to whichever of the two starts first, and what lies
                 between them
  tail           behind both (accumulator reset, next pass's tiles and bytes)

  python scripts/conv_epilogue_census.py            # all kernels of the translation unit
  python scripts/conv_epilogue_census.py --hot      # the three tanh-GELU instantiations only
  python scripts/conv_epilogue_census.py --asm F.s  # census of an existing assembly file
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "jaeger_amd" / "csrc"
UNIT = "jg_conv_f16_k5.hip"
# the residual stacks' hot patterns: <K = 5, EP, LUT = 0, FLAT = 0, CW = 128, TANH = 1, PIPE = 0>
HOT_EPS = (16, 24, 376)

REGIONS = ("before", "mfma_steady", "mfma_rest", "epilogue", "pool", "store", "tail")
_VMEM = ("ds_", "global_", "scratch_", "buffer_", "flat_")
_KERNEL = re.compile(r"conv_f16x3_kernelILi(\d+)ELj(\d+)ELb([01])ELb([01])ELi(\d+)ELb([01])ELb([01])EEEv")


def find_hipcc() -> str | None:
    cand = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    if os.path.isfile(cand) and os.access(cand, os.X_OK):
        return cand
    return shutil.which("hipcc")


def makefile_flags(arch: str = "gfx950") -> list[str]:
    """FLAGS of jaeger_amd/csrc/Makefile, its make variables expanded."""
    text = (CSRC / "Makefile").read_text()
    m = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M)
    if m is None:
        raise RuntimeError("no FLAGS line in the Makefile")
    flags = m.group(1).replace("$(ARCH)", arch).replace("$(ROOT)", str(ROOT))
    if "$(" in flags:
        raise RuntimeError(f"unexpanded make variable in FLAGS: {flags}")
    return flags.split()


def compile_asm(out_dir: str, hipcc: str | None = None, extra: list[str] | None = None) -> Path:
    hipcc = hipcc or find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    out = Path(out_dir) / (Path(UNIT).stem + ".s")
    cmd = [hipcc, *makefile_flags(), *(extra or []), "--cuda-device-only", "-S", "-o", str(out), UNIT]
    subprocess.run(cmd, check=True, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return out


def short_name(sym: str) -> str:
    m = _KERNEL.search(sym)
    if m is None:
        return sym
    k, ep, lut, flat, cw, tanh, pipe = m.groups()
    return f"conv_f16x3_kernel<{k}, {ep}, {lut}, {flat}, {cw}, {tanh}, {pipe}>"


def _mnemonic(line: str) -> str | None:
    s = line.strip()
    if not s or s[0] in ".;" or s.endswith(":"):
        return None
    return s.split()[0]


def _metadata(text: str) -> dict[str, dict[str, int]]:
    out: dict[str, dict[str, int]] = {}
    start = text.find(".amdgpu_metadata")
    if start < 0:
        return out
    cur: dict[str, int] = {}
    keys = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
            "agpr_count")
    # one YAML list item per kernel: its scalar fields come in alphabetical order, `.name` among them
    for line in text[start:].splitlines():
        s = line.strip()
        if s.startswith("- .agpr_count") or s.startswith("- .args"):
            cur = {}
        m = re.match(r"-?\s*\.(\w+):\s+(\S+)$", s)
        if m is None:
            continue
        key, val = m.groups()
        if key in keys:
            cur[key] = int(val)
        elif key == "name":
            out[val] = cur
    return out


def _innermost_mfma_loop(lines: list[str], mfma: list[int]) -> set[int]:
    """Line numbers of the blocks of the deepest loop that holds MFMAs.  Block membership comes from the
    comments the compiler writes behind block labels (`in Loop: Header=BBf_h Depth=d`, `This Inner Loop
    Header: Depth=d`), so out-of-line blocks of the loop count and blocks merely laid out between do not."""
    owner: list[tuple[str, int] | None] = []
    cur: tuple[str, int] | None = None
    for idx, l in enumerate(lines):
        m = re.match(r"(?:\.L(BB\d+_\d+):|; %bb\.\d+:)\s*(;.*)?$", l)
        if m:
            com = m.group(2) or ""
            nxt = lines[idx + 1] if idx + 1 < len(lines) else ""
            hdr = re.search(r"Loop Header: Depth=(\d+)", com) or (
                re.search(r"Loop Header: Depth=(\d+)", nxt) if nxt.lstrip().startswith(";") and "Parent Loop" in com else None)
            inl = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", com)
            if hdr and m.group(1):
                cur = (m.group(1), int(hdr.group(1)))
            elif inl:
                cur = (inl.group(1), int(inl.group(2)))
            else:
                cur = None
        owner.append(cur)
    loops = {owner[q] for q in mfma if owner[q] is not None}
    if not loops:
        return set()
    deepest = max(loops, key=lambda t: t[1])
    return {idx for idx, o in enumerate(owner) if o == deepest}


def census_kernel(lines: list[str]) -> dict[str, dict[str, int]]:
    """lines: the kernel's text from its symbol label to its .Lfunc_end."""
    n = len(lines)
    mn = [_mnemonic(l) for l in lines]
    label_at = {}
    for idx, l in enumerate(lines):
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if m:
            label_at[m.group(1)] = idx
    starts = sorted(label_at.values())

    def block_of(idx: int) -> tuple[int, int]:      # [start, end) of the label block that holds line idx
        lo, hi = 0, n
        for s in starts:
            if s <= idx:
                lo = s
            else:
                hi = s
                break
        return lo, hi

    mfma = [idx for idx, m in enumerate(mn) if m and m.startswith("v_mfma")]
    steady_lines: set[int] = set()
    if mfma:
        r0 = block_of(mfma[0])[0]
        r1 = block_of(mfma[-1])[1]
        # the chunk loop: the deepest loop (by the compiler's loop comments) whose blocks hold MFMAs
        steady_lines = _innermost_mfma_loop(lines, mfma)
    else:
        r0 = r1 = n
    stores = [idx for idx in range(r1, n) if mn[idx] and mn[idx].startswith("global_store_dwordx4")]
    if stores:
        s0 = block_of(stores[0])[0]
        s1 = block_of(stores[-1])[1]
    else:
        s0 = s1 = n
    # the pool branch: label blocks behind the region (outside the store section) from the first to the last one that
    # holds the pool's -inf literal; it may sit before or behind the store section
    pool_blocks = [block_of(idx) for idx in range(r1, n)
                   if "0xff800000" in lines[idx] and mn[idx] and not (s0 <= idx < s1)]
    if pool_blocks:
        p0, p1 = pool_blocks[0][0], pool_blocks[-1][1]
        if p0 < s0 < p1:        # (never seen: the store section inside the pool branch)
            p1 = s0
    else:
        p0 = p1 = s0
    in_pool = lambda idx: p0 <= idx < p1
    in_store = lambda idx: s0 <= idx < s1
    last = max(s1, p1) if (stores or pool_blocks) else n
    first = min(x for x in (s0 if stores else n, p0 if pool_blocks else n, n))
    spans = {
        "before": [(0, r0)],
        "mfma_steady": [],             # (the loop's blocks: steady_lines)
        "mfma_rest": [(r0, r1)],       # (minus steady_lines)
        "epilogue": [(r1, first)] + ([(min(s1, p1), max(s0, p0))] if stores and pool_blocks else []),
        "pool": [(p0, p1)],
        "store": [(s0, s1)],
        "tail": [(last, n)],
    }
    out: dict[str, dict[str, int]] = {}
    for name, sp in spans.items():
        c = {"mfma": 0, "vec_mem": 0, "readlane": 0, "writelane": 0, "store_x4": 0, "addr64": 0, "scratch": 0}
        if name == "mfma_steady":
            todo = sorted(steady_lines)
        else:
            todo = [idx for lo, hi in sp for idx in range(lo, hi) if name != "mfma_rest" or idx not in steady_lines]
        for idx in todo:
            m = mn[idx]
            if m is None:
                continue
            if m.startswith("v_mfma"):
                c["mfma"] += 1
            elif m.startswith("v_") or m.startswith(_VMEM):
                c["vec_mem"] += 1
                if m.startswith("v_readlane"):
                    c["readlane"] += 1
                elif m.startswith("v_writelane"):
                    c["writelane"] += 1
                elif m.startswith("global_store_dwordx4"):
                    c["store_x4"] += 1
                elif m.startswith(("v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32")):
                    c["addr64"] += 1
                elif m.startswith("scratch_"):
                    c["scratch"] += 1
        out[name] = c
    return out


def census(asm_text: str) -> dict[str, dict]:
    """kernel short name -> {"regions": {...}, "meta": {...}}, in the order of the text."""
    lines = asm_text.splitlines()
    meta = _metadata(asm_text)
    out: dict[str, dict] = {}
    idx = 0
    while idx < len(lines):
        m = re.match(r"(_Z\w*conv_f16x3_kernel\w*):", lines[idx])
        if m is None:
            idx += 1
            continue
        sym = m.group(1)
        end = idx + 1
        while end < len(lines) and not lines[end].startswith(".Lfunc_end"):
            end += 1
        out[short_name(sym)] = {"regions": census_kernel(lines[idx + 1:end]), "meta": meta.get(sym, {})}
        idx = end
    return out


def format_report(res: dict[str, dict], only_hot: bool = False) -> str:
    rows = []
    for name, r in res.items():
        if only_hot and name not in hot_names():
            continue
        reg, meta = r["regions"], r["meta"]
        rows.append(f"kernel {name}")
        rows.append("  mfma %d  sgpr_spill %d  vgpr_spill %d  scratch_bytes %d  vgprs %d  agprs %d" % (
            sum(c["mfma"] for c in reg.values()), meta.get("sgpr_spill_count", -1), meta.get("vgpr_spill_count", -1),
            meta.get("private_segment_fixed_size", -1), meta.get("vgpr_count", -1), meta.get("agpr_count", -1)))
        for name_r in REGIONS:
            c = reg[name_r]
            rows.append("  %-12s mfma %4d  vec_mem %5d  readlane %4d  writelane %4d  store_x4 %3d  addr64 %3d  scratch %3d" % (
                name_r, c["mfma"], c["vec_mem"], c["readlane"], c["writelane"], c["store_x4"], c["addr64"], c["scratch"]))
        lanes_rest = sum(reg[q]["readlane"] + reg[q]["writelane"] for q in REGIONS if q not in ("before", "mfma_steady"))
        st = reg["store"]
        rows.append("  lane_rw_outside_steady_body %d  store_instr_per_store %.2f" % (
            lanes_rest, st["vec_mem"] / st["store_x4"] if st["store_x4"] else 0.0))
    return "\n".join(rows) + "\n"


def parse_report(text: str) -> dict[str, dict]:
    """Inverse of format_report (reads a committed census file back)."""
    out: dict[str, dict] = {}
    cur = None
    for line in text.splitlines():
        t = line.split()
        if not t:
            continue
        if t[0] == "kernel":
            cur = {"regions": {}, "meta": {}}
            out[line[len("kernel "):].strip()] = cur
        elif cur is None:
            continue
        elif t[0] in REGIONS:
            cur["regions"][t[0]] = {t[q]: int(t[q + 1]) for q in range(1, len(t), 2)}
        elif t[0] == "mfma":
            kv = {t[q]: int(t[q + 1]) for q in range(0, len(t), 2)}
            cur["meta"] = {"sgpr_spill_count": kv["sgpr_spill"], "vgpr_spill_count": kv["vgpr_spill"],
                           "private_segment_fixed_size": kv["scratch_bytes"], "vgpr_count": kv["vgprs"],
                           "agpr_count": kv["agprs"]}
    return out


def hot_names() -> list[str]:
    return [f"conv_f16x3_kernel<5, {ep}, 0, 0, 128, 1, 0>" for ep in HOT_EPS]


def lane_rw_outside_steady(reg: dict[str, dict[str, int]]) -> int:
    return sum(reg[q]["readlane"] + reg[q]["writelane"] for q in REGIONS if q not in ("before", "mfma_steady"))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--asm", help="take this assembly file instead of compiling")
    ap.add_argument("--hot", action="store_true", help="only the three hot tanh-GELU instantiations")
    ap.add_argument("--keep", help="also copy the assembly to this path")
    args = ap.parse_args()
    if args.asm:
        text = Path(args.asm).read_text()
    else:
        with tempfile.TemporaryDirectory(prefix="jg_census_") as tmp:
            path = compile_asm(tmp)
            text = path.read_text()
            if args.keep:
                shutil.copy(path, args.keep)
    sys.stdout.write(format_report(census(text), only_hot=args.hot))
    return 0


if __name__ == "__main__":
    sys.exit(main())
