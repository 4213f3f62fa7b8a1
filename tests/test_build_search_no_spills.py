"""Build-time guard for the query-time search (vtc_amd/csrc/search.hip).  scan_kernel keeps one sorted list per query of its tile in
registers, an entry per lane (the grouped lists one more register per query, the entry's group), next to the NQ x NR fp64 accumulators
of a step -- a spilled register there is a scratch access in the innermost loop of a kernel that is bound by HBM (one query) or by its
fp64 arithmetic (more); mark_kernel walks the gallery the same way.  The file must define exactly the kernels of the flag table below,
each once, and every one must compile without scratch and without spills."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

TILES = ((1, 4), (2, 4), (4, 2), (8, 1))                  # tile_plan's shapes: queries x gallery rows of a step
GALLERY = {"f": "float", "DF16_": "_Float16"}              # the mangled element types
MODES = {                                                  # (GROUPED, AFTER, EXCL): the six scans launch_scan_of chooses among
    "plain": (0, 0, 0),
    "grouped": (1, 0, 0),
    "cursor": (0, 1, 0),
    "cursor + excluded row": (0, 1, 1),
    "grouped + excluded group": (1, 0, 1),
    "page": (1, 1, 1),
}


def _metadata(src, tmp_path):
    out = tmp_path / (os.path.basename(src) + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), src],
                   check=True, capture_output=True, timeout=900)
    text = out.read_text()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n){0,14}?\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n){0,14}?\s+\.vgpr_count:\s+(\d+)\n"
                         r"\s+\.vgpr_spill_count:\s+(\d+)", text):
        meta[m.group(1)] = dict(scratch=int(m.group(2)), vgpr=int(m.group(3)), spill=int(m.group(4)))
    return meta


def expected_kernels():
    """What search.hip instantiates: the start of each kernel's mangled name, up to its parameter list, -> what it is."""
    want = {}
    for g, g_name in GALLERY.items():
        for nq, nr in TILES:
            for masked in (0, 1):
                for mode, (grouped, after, excl) in MODES.items():
                    want[f"11scan_kernelI{g}Li{nq}ELi{nr}ELb{masked}ELb{grouped}ELb{after}ELb{excl}EEEv"] = ("scan", g_name, nq, nr, masked, mode)
                want[f"11mark_kernelI{g}Li{nq}ELi{nr}ELb{masked}EEEv"] = ("mark", g_name, nq, nr, masked)
        want[f"19pair_dists64_kernelI{g}EEv"] = ("pair_dists64", g_name)
    for src in ("9ScanLists", "9PartLists"):
        for grouped in (0, 1):
            want[f"12merge_kernelINS_{src}ELb{grouped}EEEv"] = ("merge", src[1:], grouped)
    want["20row_mask_pack_kernelE"] = ("row_mask_pack",)
    return want


@pytest.fixture(scope="module")
def search_meta(tmp_path_factory):
    return _metadata(os.path.join(ROOT, "vtc_amd", "csrc", "search.hip"), tmp_path_factory.mktemp("search_asm"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_search_defines_exactly_the_flag_table_without_scratch(search_meta):
    want = expected_kernels()
    assert len(want) == 96 + 16 + 2 + 4 + 1
    assert len(search_meta) == len(want), sorted(search_meta)
    taken = set()
    for start, what in want.items():
        hits = [k for k in search_meta if k.startswith("_ZN12_GLOBAL__N_1" + start)]
        assert len(hits) == 1, (what, start, hits)
        taken.add(hits[0])
        assert search_meta[hits[0]]["spill"] == 0 and search_meta[hits[0]]["scratch"] == 0, (what, hits[0], search_meta[hits[0]])
    assert taken == set(search_meta), sorted(set(search_meta) - taken)
