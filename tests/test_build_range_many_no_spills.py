"""Build-time guard for the many-query count pass of the range search (vtc_amd/csrc/range_many.hip).  The pass keeps two sets of up to
sixteen MFMA operand fragments, the accumulators, the fp64 radius and the word it builds in registers inside the loop that streams the
gallery; a spilled one is a scratch access per tile.  The file must define exactly the kernels below, each once -- the pass's eight
instantiations, the query prologue it shares with search_many.hip and the prefix launch it shares with range.hip -- and every one must
compile without scratch and without spilled registers.  Only the metadata is read."""
import os

import pytest

from test_build_search_no_spills import HIPCC, ROOT, _metadata

STEPS = (2, 4, 8, 16)          # MFMA steps of 32 columns an item of the pass: the largest that divides the row
KERNELS = {
    "16many_prep_kernelE": "the query prologue",
    **{f"22range_many_pass_kernelILb{masked}ELi{nks}EEEv": ("the pass", "masked" if masked else "every row live", nks)
       for masked in (0, 1) for nks in STEPS},
    "19range_prefix_kernelE": "lims and the chunk bases",
}


@pytest.fixture(scope="module")
def range_many_meta(tmp_path_factory):
    return _metadata(os.path.join(ROOT, "vtc_amd", "csrc", "range_many.hip"), tmp_path_factory.mktemp("range_many_asm"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_range_many_defines_exactly_its_kernels_without_scratch(range_many_meta):
    assert len(range_many_meta) == len(KERNELS) == 10, sorted(range_many_meta)
    taken = set()
    for start, what in KERNELS.items():
        hits = [k for k in range_many_meta if k.startswith("_ZN12_GLOBAL__N_1" + start)]
        assert len(hits) == 1, (what, start, hits)
        taken.add(hits[0])
        assert range_many_meta[hits[0]]["spill"] == 0 and range_many_meta[hits[0]]["scratch"] == 0, (what, hits[0], range_many_meta[hits[0]])
    assert taken == set(range_many_meta), sorted(set(range_many_meta) - taken)
