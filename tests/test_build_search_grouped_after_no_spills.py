"""Build-time guard for the paged grouped search (vtc_amd/csrc/search.hip): videos_page_scan_kernel is the grouped scan with the cursor,
the excluded group and the ban word's load on its insertion path, videos_page_mark_kernel the scan's walk with the cursors and no lists;
what tests/test_build_search_no_spills.py says about a spilled register holds for both.  Every instantiation -- the four tile shapes x
masked x {float, _Float16}, sixteen of each -- must compile without scratch and without spills, and the kernels that are counted by
substring elsewhere keep their counts."""
import os
import shutil

import pytest

from test_build_search_no_spills import _metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

TILES = ((1, 4), (2, 4), (4, 2), (8, 1))                  # search_plan's tile shapes: queries x gallery rows of a step
GALLERY = {"f": "float", "DF16_": "_Float16"}              # the mangled element types


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_every_page_instantiation_compiles_without_scratch(tmp_path):
    meta = _metadata(os.path.join(ROOT, "vtc_amd", "csrc", "search.hip"), tmp_path)
    for name in ("videos_page_scan_kernel", "videos_page_mark_kernel"):
        kernels = [k for k in meta if name in k]
        assert len(kernels) == 2 * 2 * len(TILES), kernels
        for nq, nr in TILES:
            for masked in (0, 1):
                for g in GALLERY:
                    hits = [k for k in kernels if f"{name}I{g}Li{nq}ELi{nr}ELb{masked}EEE" in k]
                    assert len(hits) == 1, (name, nq, nr, masked, g, kernels)
                    assert meta[hits[0]]["spill"] == 0 and meta[hits[0]]["scratch"] == 0, (hits[0], meta[hits[0]])
    # the existing kernels are counted by these substrings elsewhere: the new names must not move them
    assert len([k for k in meta if "search_scan_kernel" in k]) == 8
    assert len([k for k in meta if "search_grouped_scan_kernel" in k]) == 8
    assert len([k for k in meta if "half_scan" in k]) == 16
    assert len([k for k in meta if "merge_grouped_kernel" in k]) == 2
    assert len([k for k in meta if "after_scan_kernel" in k]) == 16
    assert len([k for k in meta if "excluding_scan_kernel" in k]) == 16 and len([k for k in meta if "excluding_grouped_scan_kernel" in k]) == 16
    assert len([k for k in meta if "videos_page_" in k]) == 32
