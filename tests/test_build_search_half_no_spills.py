"""Build-time guard for the scan over a half gallery (vtc_amd/csrc/search.hip, half_scan_kernel / half_scan_grouped_kernel): the body of
the fp32 scan with a row loader that widens 8 bytes to a float4, so what tests/test_build_search_no_spills.py says about a spilled
register holds.  Every instantiation -- the half plan's four tile shapes x masked x grouped, sixteen -- must compile without scratch and
without spills, and the fp32 kernels keep their counts: eight scans, eight grouped scans, two grouped merges."""
import os
import shutil

import pytest

from test_build_search_no_spills import _metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

HALF_TILES = ((1, 4), (2, 4), (4, 2), (8, 1))            # search_plan's tile shapes, the fp32 scan's: queries x gallery rows of a step


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_every_half_scan_instantiation_compiles_without_scratch(tmp_path):
    meta = _metadata(os.path.join(ROOT, "vtc_amd", "csrc", "search.hip"), tmp_path)
    for name in ("half_scan_kernel", "half_scan_grouped_kernel"):
        scans = [k for k in meta if name in k]
        assert len(scans) == 2 * len(HALF_TILES), scans
        for nq, nr in HALF_TILES:
            for masked in (0, 1):
                hits = [k for k in scans if f"{name}ILi{nq}ELi{nr}ELb{masked}EEE" in k]
                assert len(hits) == 1, (nq, nr, masked, scans)
                assert meta[hits[0]]["spill"] == 0 and meta[hits[0]]["scratch"] == 0, (hits[0], meta[hits[0]])
    assert len([k for k in meta if "half_scan" in k]) == 16
    # the fp32 kernels are counted by these substrings elsewhere: the new names must not move them
    assert len([k for k in meta if "search_scan_kernel" in k]) == 8
    assert len([k for k in meta if "search_grouped_scan_kernel" in k]) == 8
    assert len([k for k in meta if "merge_grouped_kernel" in k]) == 2
