"""Build-time guard for the grouped query-time scan (vtc_amd/csrc/search.hip, search_grouped_scan_kernel): it keeps one more register
per query of its tile (the entry's group) next to what tests/test_build_search_no_spills.py describes.  Its eight instantiations, the
four tile shapes with and without the row mask, must compile without scratch and without spills, beside the eight ungrouped ones."""
import os
import shutil

import pytest

from test_build_search_no_spills import _metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_every_grouped_scan_instantiation_compiles_without_scratch(tmp_path):
    meta = _metadata(os.path.join(ROOT, "vtc_amd", "csrc", "search.hip"), tmp_path)
    scans = [k for k in meta if "search_grouped_scan_kernel" in k]
    assert len(scans) == 8, scans
    for nq, nr in ((1, 4), (2, 4), (4, 2), (8, 1)):           # search_plan's tile shapes: queries x gallery rows of a step
        for masked in (0, 1):
            hits = [k for k in scans if f"search_grouped_scan_kernelILi{nq}ELi{nr}ELb{masked}EEE" in k]
            assert len(hits) == 1, (nq, nr, masked, scans)
            assert meta[hits[0]]["spill"] == 0 and meta[hits[0]]["scratch"] == 0, (hits[0], meta[hits[0]])
    merges = [k for k in meta if "merge_grouped_kernel" in k]
    assert len(merges) == 2 and all(meta[k]["spill"] == 0 and meta[k]["scratch"] == 0 for k in merges), merges
