#!/usr/bin/env python3
"""Record tests/golden/operand_digests.json (tests/test_gpu_operand_digest.py) - against a library of the PARENT commit:

    JAEGER_HIP_LIB=/tmp/parent/jaeger_amd/libjaeger_hip.so python scripts/record_operand_digests.py

The code under test never records it.  A change that moves operand bytes on purpose re-records from its own parent plus
the one intended difference, and says in its message which models' digests moved and why.  (The parent of the commit
that introduced the digest had none: it was recorded from that parent with the same hash added behind each of its
host-to-device copies.)  Needs a GPU: the operands are built and hashed while the model is created on the device."""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def digest_of(name: str, probe=None) -> str:
    """The model's operand digest as 16 hex digits; ``probe(engine)`` runs before the engine is closed."""
    import placement_cases as pc
    eng = pc.make_engine(name)
    try:
        if probe is not None:
            probe(eng)
        return f"{eng.model.operand_digest():016x}"
    finally:
        eng.close()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "operand_digests.json"))
    args = ap.parse_args()
    if "JAEGER_HIP_LIB" not in os.environ:
        print("record_operand_digests: JAEGER_HIP_LIB is not set - this would record the code under test", file=sys.stderr)
        return 2
    from test_gpu_operand_digest import MODELS
    out = {name: digest_of(name) for name in MODELS}
    Path(args.out).write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(f"{args.out}: {len(out)} models")
    return 0


if __name__ == "__main__":
    sys.exit(main())
