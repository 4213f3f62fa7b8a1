"""Build-time guard for the many-query search of a half gallery (vtc_amd/csrc/search_many.hip).  The candidate pass keeps sixteen sorted
lists, two sets of sixteen MFMA operand fragments and the accumulators in registers; a spilled one is a scratch access in the loop that
streams the gallery.  The file must define exactly the kernels below, each once, and every one without scratch and without spills."""
import os

import pytest

from test_build_search_no_spills import HIPCC, ROOT, _metadata

STEPS = (2, 4, 8, 16)          # MFMA steps of 32 columns an item of the pass: the largest that divides the row
KERNELS = {
    "16many_prep_kernelE": "the query prologue",
    **{f"16many_pass_kernelILb{masked}ELi{nks}EEEv": ("the candidate pass", "masked" if masked else "every row live", nks)
       for masked in (0, 1) for nks in STEPS},
    "18many_finish_kernelE": "merge, fp64 re-rank, certification",
    "20many_fallback_kernelE": "the exact scan of a flagged query",
}


@pytest.fixture(scope="module")
def many_meta(tmp_path_factory):
    return _metadata(os.path.join(ROOT, "vtc_amd", "csrc", "search_many.hip"), tmp_path_factory.mktemp("search_many_asm"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_search_many_defines_exactly_its_kernels_without_scratch(many_meta):
    assert len(many_meta) == len(KERNELS) == 11, sorted(many_meta)
    taken = set()
    for start, what in KERNELS.items():
        hits = [k for k in many_meta if k.startswith("_ZN12_GLOBAL__N_1" + start)]
        assert len(hits) == 1, (what, start, hits)
        taken.add(hits[0])
        assert many_meta[hits[0]]["spill"] == 0 and many_meta[hits[0]]["scratch"] == 0, (what, hits[0], many_meta[hits[0]])
    assert taken == set(many_meta), sorted(set(many_meta) - taken)
