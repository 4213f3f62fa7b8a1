"""Build-time guard for the query-time scan (vtc_amd/csrc/search.hip): search_scan_kernel keeps one sorted list per query of its tile in
registers, an entry per lane, next to the NQ x NR fp64 accumulators of a step -- a spilled register there is a scratch access in the
innermost loop of a kernel that is bound by HBM (one query) or by its fp64 arithmetic (more).  Every instantiation, the four tile shapes
with and without the row mask, must compile without scratch and without spills."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


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


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_every_scan_instantiation_compiles_without_scratch(tmp_path):
    meta = _metadata(os.path.join(ROOT, "vtc_amd", "csrc", "search.hip"), tmp_path)
    scans = [k for k in meta if "search_scan_kernel" in k]
    assert len(scans) == 8, scans
    for nq, nr in ((1, 4), (2, 4), (4, 2), (8, 1)):           # search_plan's tile shapes: queries x gallery rows of a step
        for masked in (0, 1):
            hits = [k for k in scans if f"search_scan_kernelILi{nq}ELi{nr}ELb{masked}EEE" in k]
            assert len(hits) == 1, (nq, nr, masked, scans)
            assert meta[hits[0]]["spill"] == 0 and meta[hits[0]]["scratch"] == 0, (hits[0], meta[hits[0]])
