#!/usr/bin/env python3
"""Is the device code of the split-f16 conv kernels the same text as at another commit?

Exports jaeger_amd/csrc and include of <git-ref> into a temporary directory, compiles the
thirteen CONV units of the Makefile, jg_resblock.hip and jg_resblock64.hip of both trees to
gfx950 assembly (the Makefile's FLAGS, device code only, no GPU; about a minute per unit and
job), replaces the one symbol that differs between two compiles of the same source
(__hip_cuid_<hex>) by a fixed token and compares the texts.  Per unit: the two SHA-256
digests and `identical` or `different`; for a differing unit the kernels whose text differs,
with the register / spill / scratch metadata of both sides.  Exit status 1 on any difference.

  python scripts/conv_isa_diff.py --ref HEAD~1
  python scripts/conv_isa_diff.py --ref HEAD~1 --units jg_conv_f16_k5.hip --flags=-DJG_EXPERIMENT
  python scripts/conv_isa_diff.py --ref HEAD~1 --keep DIR      # leaves DIR/ref/*.s and DIR/new/*.s
  python scripts/conv_isa_diff.py --ref-asm DIR/ref            # compare against kept assembly
"""
from __future__ import annotations

import argparse
import hashlib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conv_epilogue_census import ROOT, _metadata, find_hipcc, makefile_flags  # noqa: E402

MAX_JOBS = 16
_CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
_META_KEYS = ("sgpr_count", "vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count",
              "private_segment_fixed_size")


def default_units() -> list[str]:
    text = (ROOT / "jaeger_amd" / "csrc" / "Makefile").read_text()
    m = re.search(r"^CONV\s*:=\s*(.*)$", text, re.M)
    if m is None:
        raise RuntimeError("no CONV line in the Makefile")
    return m.group(1).split() + ["jg_resblock.hip", "jg_resblock64.hip"]


def export_ref(ref: str, dest: Path) -> None:
    tar = subprocess.run(["git", "archive", ref, "jaeger_amd/csrc", "include"], cwd=ROOT, check=True,
                         stdout=subprocess.PIPE).stdout
    with tarfile.open(fileobj=io.BytesIO(tar)) as tf:
        tf.extractall(dest)


def compile_unit(hipcc: str, tree: Path, unit: str, out: Path, extra: list[str]) -> None:
    flags = [f.replace(str(ROOT), str(tree)) for f in makefile_flags()]
    cmd = [hipcc, *flags, *extra, "--cuda-device-only", "-S", "-o", str(out), unit]
    r = subprocess.run(cmd, cwd=tree / "jaeger_amd" / "csrc", stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    if r.returncode != 0:
        raise RuntimeError(f"{unit} in {tree}:\n{r.stderr.decode(errors='replace')}")


def normalised(path: Path) -> str:
    return _CUID.sub("__hip_cuid_X", path.read_text())


def functions(text: str) -> dict[str, str]:
    """symbol -> text from its label to its .Lfunc_end."""
    out: dict[str, str] = {}
    lines = text.splitlines()
    idx = 0
    while idx < len(lines):
        m = re.match(r"([A-Za-z_]\w*):", lines[idx])
        if m is None:
            idx += 1
            continue
        end = idx + 1
        while end < len(lines) and not lines[end].startswith(".Lfunc_end"):
            end += 1
        out[m.group(1)] = "\n".join(lines[idx:end])
        idx = end
    return out


def report_unit(unit: str, ref_text: str, new_text: str) -> tuple[bool, str]:
    d_ref = hashlib.sha256(ref_text.encode()).hexdigest()
    d_new = hashlib.sha256(new_text.encode()).hexdigest()
    same = ref_text == new_text
    rows = [f"{unit}  ref {d_ref}  new {d_new}  {'identical' if same else 'different'}"]
    if not same:
        f_ref, f_new = functions(ref_text), functions(new_text)
        m_ref, m_new = _metadata(ref_text), _metadata(new_text)
        for sym in sorted(set(f_ref) | set(f_new)):
            if f_ref.get(sym) == f_new.get(sym):
                continue
            rows.append(f"  {sym}" + ("" if sym in f_ref and sym in f_new else "  (one side only)"))
            for side, meta, fn in (("ref", m_ref, f_ref), ("new", m_new, f_new)):
                vals = "  ".join(f"{k} {meta.get(sym, {}).get(k, -1)}" for k in _META_KEYS)
                rows.append(f"    {side}  lines {fn.get(sym, '').count(chr(10)) + 1 if sym in fn else 0}  {vals}")
        if len(rows) == 1:
            rows.append("  (no kernel's text differs: the difference is outside the function bodies)")
    return same, "\n".join(rows)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ref", help="git ref whose device code is the reference")
    ap.add_argument("--ref-asm", help="directory of reference assembly kept by an earlier run (instead of --ref)")
    ap.add_argument("--units", nargs="+", help="translation units (default: the CONV units and the two resblock units)")
    ap.add_argument("--flags", action="append", default=[], help="extra compiler flag for both sides (repeatable)")
    ap.add_argument("--keep", help="leave the assembly of both sides under this directory (ref/, new/)")
    ap.add_argument("--jobs", type=int, default=min(MAX_JOBS, os.cpu_count() or 1))
    args = ap.parse_args()
    if (args.ref is None) == (args.ref_asm is None):
        ap.error("give one of --ref and --ref-asm")
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    units = args.units or default_units()
    with tempfile.TemporaryDirectory(prefix="jg_isa_diff_") as tmp:
        work = Path(args.keep) if args.keep else Path(tmp)
        new_dir = work / "new"
        ref_dir = Path(args.ref_asm) if args.ref_asm else work / "ref"
        new_dir.mkdir(parents=True, exist_ok=True)
        jobs = [(ROOT, u, new_dir / (Path(u).stem + ".s")) for u in units]
        if args.ref:
            ref_dir.mkdir(parents=True, exist_ok=True)
            ref_tree = Path(tmp) / "tree"
            export_ref(args.ref, ref_tree)
            jobs += [(ref_tree, u, ref_dir / (Path(u).stem + ".s")) for u in units]
        with ThreadPoolExecutor(max_workers=max(1, min(args.jobs, MAX_JOBS))) as pool:
            for f in [pool.submit(compile_unit, hipcc, tree, u, out, args.flags) for tree, u, out in jobs]:
                f.result()
        all_same = True
        for u in units:
            name = Path(u).stem + ".s"
            same, text = report_unit(u, normalised(ref_dir / name), normalised(new_dir / name))
            all_same = all_same and same
            print(text)
    print("all identical" if all_same else "DIFFERENT")
    return 0 if all_same else 1


if __name__ == "__main__":
    sys.exit(main())
