#!/usr/bin/env python3
"""Record tests/golden/placement_census.json (tests/test_gpu_placement_census.py) - against the library of the PARENT commit:

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/jaeger_amd/csrc
    JAEGER_HIP_LIB=/tmp/parent/jaeger_amd/libjaeger_hip.so python scripts/record_placement_census.py

The code under test never records it; a change that moves a placement on purpose re-records from its own parent plus the
one intended difference, reviewed as a diff of the JSON.  Needs a GPU (the profiling classes are read after a forward)."""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "placement_census.json"))
    args = ap.parse_args()
    if "JAEGER_HIP_LIB" not in os.environ:
        print("record_placement_census: JAEGER_HIP_LIB is not set - this would record the code under test", file=sys.stderr)
        return 2
    import placement_cases as pc
    out = {name: pc.census(name) for name in sorted(pc.MODELS)}
    Path(args.out).write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(f"{args.out}: {len(out)} models, {sum(len(v['runs']) for v in out.values())} runs")
    return 0


if __name__ == "__main__":
    sys.exit(main())
