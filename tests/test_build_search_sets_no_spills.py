"""Build-time guard for the set queries (vtc_amd/csrc/search_sets.hip): the file must define exactly the SET instantiations of the one
scan kernel -- scan_kernel<SetOf<G>, ...>: plain, grouped, the excluded row (the cursor scan's flags, its cursor never loaded) and the
excluded group, each with and without a mask, for float and _Float16 galleries, in the four tile shapes -- and the three merges its
driver launches, each once, and every one must compile without scratch and without spills: a set scan keeps ONE list per tile in
registers next to the NQ x NR fp64 accumulators of a step, and a spilled register there is a scratch access in its innermost loop."""
import os

import pytest

import test_build_search_no_spills as B

SET_MODES = {                                              # (GROUPED, AFTER, EXCL)
    "plain": (0, 0, 0),
    "grouped": (1, 0, 0),
    "excluded row": (0, 1, 1),
    "grouped + excluded group": (1, 0, 1),
}


def expected_kernels():
    want = {}
    for g, g_name in B.GALLERY.items():
        for nq, nr in B.TILES:
            for masked in (0, 1):
                for mode, (grouped, after, excl) in SET_MODES.items():
                    want[f"11scan_kernelINS_5SetOfI{g}EELi{nq}ELi{nr}ELb{masked}ELb{grouped}ELb{after}ELb{excl}EEEv"] = ("set scan", g_name, nq, nr, masked, mode)
    want["12merge_kernelINS_9ScanListsELb0EEEv"] = ("merge", "one tile a set, ungrouped")
    want["12merge_kernelINS_9ScanListsELb1EEEv"] = ("merge", "grouped")
    want["12merge_kernelINS_12ScanRowListsELb1EEEv"] = ("merge", "several tiles a set, ungrouped: a row once")
    return want


@pytest.fixture(scope="module")
def sets_meta(tmp_path_factory):
    return B._metadata(os.path.join(B.ROOT, "vtc_amd", "csrc", "search_sets.hip"), tmp_path_factory.mktemp("search_sets_asm"))


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc not available")
def test_search_sets_defines_exactly_the_set_scans_without_scratch(sets_meta):
    want = expected_kernels()
    assert len(want) == 64 + 3
    assert len(sets_meta) == len(want), sorted(sets_meta)
    taken = set()
    for start, what in want.items():
        hits = [k for k in sets_meta if k.startswith("_ZN12_GLOBAL__N_1" + start)]
        assert len(hits) == 1, (what, start, hits)
        taken.add(hits[0])
        assert sets_meta[hits[0]]["spill"] == 0 and sets_meta[hits[0]]["scratch"] == 0, (what, hits[0], sets_meta[hits[0]])
    assert taken == set(sets_meta), sorted(set(sets_meta) - taken)
