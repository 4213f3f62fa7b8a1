"""Build-time guard for the 8-bit gallery storage (vtc_amd/csrc/search_q8.hip, search_sets_q8.hip, range_q8.hip): each unit must define
exactly its table of q8 instantiations -- the kernels of search.hip / search_sets.hip / range.hip with vtcsweep::q8_t as the gallery's
element type, whose row loader adds a scale register a row and four multiplies a piece to the scan's innermost loop -- each once, and
every one must compile without scratch and without spills.  The test only reads the register metadata of the compiled units."""
import os

import pytest

import test_build_search_no_spills as B
from test_build_search_sets_no_spills import SET_MODES

Q8 = "N8vtcsweep4q8_tE"                                    # the mangled element type
CSRC = os.path.join(B.ROOT, "vtc_amd", "csrc")
pytestmark = pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc not available")


def _check(meta, want):
    assert len(meta) == len(want), sorted(meta)
    taken = set()
    for start, what in want.items():
        hits = [k for k in meta if k.startswith("_ZN12_GLOBAL__N_1" + start)]
        assert len(hits) == 1, (what, start, hits)
        taken.add(hits[0])
        assert meta[hits[0]]["spill"] == 0 and meta[hits[0]]["scratch"] == 0, (what, hits[0], meta[hits[0]])
    assert taken == set(meta), sorted(set(meta) - taken)


def test_search_q8_defines_exactly_the_q8_scans_without_scratch(tmp_path):
    want = {}
    for nq, nr in B.TILES:
        for masked in (0, 1):
            for mode, (grouped, after, excl) in B.MODES.items():
                want[f"11scan_kernelI{Q8}Li{nq}ELi{nr}ELb{masked}ELb{grouped}ELb{after}ELb{excl}EEEv"] = ("scan", nq, nr, masked, mode)
            want[f"11mark_kernelI{Q8}Li{nq}ELi{nr}ELb{masked}EEEv"] = ("mark", nq, nr, masked)
    want[f"19pair_dists64_kernelI{Q8}EEv"] = ("pair_dists64",)
    for grouped in (0, 1):
        want[f"12merge_kernelINS_9ScanListsELb{grouped}EEEv"] = ("merge", grouped)
    want["23quantize_rows_q8_kernelE"] = ("quantiser",)
    assert len(want) == 48 + 8 + 1 + 2 + 1
    _check(B._metadata(os.path.join(CSRC, "search_q8.hip"), tmp_path), want)


def test_search_sets_q8_defines_exactly_the_q8_set_scans_without_scratch(tmp_path):
    want = {}
    for nq, nr in B.TILES:
        for masked in (0, 1):
            for mode, (grouped, after, excl) in SET_MODES.items():
                want[f"11scan_kernelINS_5SetOfI{Q8}EELi{nq}ELi{nr}ELb{masked}ELb{grouped}ELb{after}ELb{excl}EEEv"] = ("set scan", nq, nr, masked, mode)
    want["12merge_kernelINS_9ScanListsELb0EEEv"] = ("merge", "one tile a set, ungrouped")
    want["12merge_kernelINS_9ScanListsELb1EEEv"] = ("merge", "grouped")
    want["12merge_kernelINS_12ScanRowListsELb1EEEv"] = ("merge", "several tiles a set, ungrouped: a row once")
    assert len(want) == 32 + 3
    _check(B._metadata(os.path.join(CSRC, "search_sets_q8.hip"), tmp_path), want)


def test_range_q8_defines_exactly_the_q8_range_passes_without_scratch(tmp_path):
    want = {}
    for nq, nr in B.TILES:
        for masked in (0, 1):
            want[f"18range_count_kernelILi{nq}ELi{nr}ELb{masked}E{Q8}EEv"] = ("count", nq, nr, masked)
    want[f"17range_fill_kernelI{Q8}EEv"] = ("fill",)
    want["19range_prefix_kernelE"] = ("prefix",)
    assert len(want) == 8 + 1 + 1
    _check(B._metadata(os.path.join(CSRC, "range_q8.hip"), tmp_path), want)
