"""The bytes the kernels read, pinned: for every model of the placement census (placement_cases.py) and the variants below,
the digest of every operand buffer model creation uploads (``HipModel.operand_digest()``: conv weight and embedding planes,
epilogue tables, first-layer tables, phase-split weights, fused-block fragments, exact-f32 weights, the table net's and
the small-window network's operands) equals golden/operand_digests.json.

The golden file is recorded by scripts/record_operand_digests.py from a library built at the commit BEFORE a change to
the operand preparation (jg_prepare.hip), never from the code under test.  No forward runs: a case is model creation
only.  A packing or folding mistake otherwise shows, if at all, as a parity failure far downstream; which kernel reads the
operands is the placement census's business, not this test's."""
import json

import placement_cases as pc
import pytest
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

#: models beside the census's, for the upload sites none of those reaches (op_cases.model_cfg variants)
EXTRA_MODELS = ()
MODELS = sorted(pc.MODELS) + list(EXTRA_MODELS)


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "operand_digests.json").read_text())


def test_golden_covers_the_cases(golden):
    assert sorted(golden) == sorted(MODELS)


@pytest.mark.parametrize("name", MODELS)
def test_operand_digest(golden, name):
    eng = pc.make_engine(name)
    try:
        got = f"{eng.model.operand_digest():016x}"
    finally:
        eng.close()
    assert got == golden[name]
