"""Build-time guard for the range search (vtc_amd/csrc/range.hip): the count pass keeps the NQ x NR fp64 accumulators of a step, the
queries' radii and their hit words in registers inside a loop that is bound by HBM (one query) or by its fp64 arithmetic (more), as the
scan of tests/test_build_search_no_spills.py does -- a spilled register there is a scratch access per row.  Every instantiation must
compile without scratch and without spills: the count pass's four tile shapes x masked x {float, _Float16} = 16, the fill pass's two
(float, _Float16) and the prefix kernel, 19 kernels in all."""
import os
import shutil

import pytest

from test_build_search_no_spills import _metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

TILES = ((1, 4), (2, 4), (4, 2), (8, 1))                  # tile_plan's shapes: queries x gallery rows of a step
GALLERY = {"f": "float", "DF16_": "_Float16"}              # the mangled element types


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_every_range_instantiation_compiles_without_scratch(tmp_path):
    meta = _metadata(os.path.join(ROOT, "vtc_amd", "csrc", "range.hip"), tmp_path)
    counts = [k for k in meta if "range_count_kernel" in k]
    assert len(counts) == 2 * 2 * len(TILES), counts
    for nq, nr in TILES:
        for masked in (0, 1):
            for g in GALLERY:
                hits = [k for k in counts if f"range_count_kernelILi{nq}ELi{nr}ELb{masked}E{g}E" in k]
                assert len(hits) == 1, (nq, nr, masked, g, counts)
    fills = [k for k in meta if "range_fill_kernel" in k]
    assert len(fills) == 2 and all(any(f"range_fill_kernelI{g}E" in k for k in fills) for g in GALLERY), fills
    assert len([k for k in meta if "range_prefix_kernel" in k]) == 1
    assert len(meta) == 19, sorted(meta)
    for k, m in meta.items():
        assert m["spill"] == 0 and m["scratch"] == 0, (k, m)
