"""Static census of the three hot k = 5 split-f16 conv instantiations (scripts/conv_epilogue_census.py).

CPU suite: compiles jg_conv_f16_k5.hip to gfx950 assembly once (about a minute) and holds the kernel text to
bounds that are set against the parent of the change that introduced them - its census is committed as
profiles/conv_k5_census_parent.txt (the same tool, run on that commit):

  * no scratch and no spilled VGPR;
  * no lane read / write (a spilled SGPR being restored / saved) in the steady chunk body of the main loop;
  * lane reads + writes in the rest of the MFMA region and behind it at most half the parent's;
  * the store section at most 2.5 vector + memory instructions per global_store_dwordx4
    (a store and one offset add each, plus slack; the parent spent 4.2 - 5.5);
  * the MFMA region (vector + memory instructions beside its MFMAs) not larger than the parent's.

Figures of the tree as committed (profiles/conv_k5_census_after.txt; parent in brackets) for the patterns
plain / shortcut / stack end: lane reads + writes outside the steady body 48 / 60 / 75 (255 / 218 / 206),
store section 1.22 / 1.16 / 1.19 instructions per store (5.45 / 4.56 / 4.16), MFMA region 499 / 503 / 507
(528 / 525 / 535), SGPR spills 48 / 58 / 63 (109 / 109 / 112), scratch 0 / 0 / 0 B (0 / 0 / 28).  The values
are printed before they are asserted (pytest -s).
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _load_tool():
    spec = importlib.util.spec_from_file_location("conv_epilogue_census", ROOT / "scripts" / "conv_epilogue_census.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


tool = _load_tool()

pytestmark = pytest.mark.skipif(tool.find_hipcc() is None, reason="hipcc not found")


@pytest.fixture(scope="module")
def after(tmp_path_factory):
    path = tool.compile_asm(str(tmp_path_factory.mktemp("census")))
    return tool.census(path.read_text())


@pytest.fixture(scope="module")
def parent():
    return tool.parse_report((ROOT / "profiles" / "conv_k5_census_parent.txt").read_text())


def _mfma_region(reg):
    return reg["mfma_steady"]["vec_mem"] + reg["mfma_rest"]["vec_mem"]


def test_parent_census_is_the_recorded_one(parent):
    # the committed parent file holds the three hot instantiations with the figures the bounds below start from
    for name in tool.hot_names():
        assert name in parent, name
        reg = parent[name]["regions"]
        assert sum(c["mfma"] for c in reg.values()) == 240
        assert reg["store"]["store_x4"] == 64
        assert tool.lane_rw_outside_steady(reg) >= 200


@pytest.mark.parametrize("ep", tool.HOT_EPS)
def test_hot_instantiation(after, parent, ep):
    name = f"conv_f16x3_kernel<5, {ep}, 0, 0, 128, 1, 0>"
    assert name in after, f"{name} is not in the translation unit"
    reg, meta = after[name]["regions"], after[name]["meta"]
    preg = parent[name]["regions"]
    lanes, planes = tool.lane_rw_outside_steady(reg), tool.lane_rw_outside_steady(preg)
    st = reg["store"]
    per_store = st["vec_mem"] / max(st["store_x4"], 1)
    print(f"{name}: scratch {meta['private_segment_fixed_size']} B, vgpr spills {meta['vgpr_spill_count']}, "
          f"sgpr spills {meta['sgpr_spill_count']} (parent {parent[name]['meta']['sgpr_spill_count']}); "
          f"steady body lane r/w {reg['mfma_steady']['readlane']}/{reg['mfma_steady']['writelane']}; "
          f"lane r+w outside it {lanes} (parent {planes}, bound {planes // 2}); "
          f"store section {st['vec_mem']} / {st['store_x4']} stores = {per_store:.2f} (bound 2.5); "
          f"MFMA region {_mfma_region(reg)} (parent {_mfma_region(preg)})")
    assert sum(c["mfma"] for c in reg.values()) == 240
    assert reg["mfma_steady"]["mfma"] == 120
    assert meta["private_segment_fixed_size"] == 0
    assert meta["vgpr_spill_count"] == 0
    assert reg["mfma_steady"]["readlane"] == 0 and reg["mfma_steady"]["writelane"] == 0
    assert 2 * lanes <= planes
    assert st["store_x4"] == 64
    assert per_store <= 2.5
    assert _mfma_region(reg) <= _mfma_region(preg)
