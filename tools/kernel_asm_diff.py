#!/usr/bin/env python3
"""Which kernels differ between two device-assembly files of the same source (a refactor's proof that it left the kernels alone):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o old.s vtc_amd/csrc/sweep.hip     # on each commit
    tools/kernel_asm_diff.py old.s new.s

Compared per kernel, instruction for instruction, after dropping `;` comments and the function number inside local labels
(.LBB12_7 -> .LBB_7), which shifts when a kernel is added or removed.  Kernels are the `.amdhsa_kernel` symbols, matched by their
demangled name without the parameter list (c++filt), so a kernel that lost an argument shows as changed, not as removed + added.
Exit status 1 when a kernel was added."""
import re
import subprocess
import sys


def kernels(path):
    out, name = {}, None
    for line in open(path):
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
        m = re.match(r"(\w+):$", line)
        if m and not line.startswith(".L"):
            name = m.group(1)
            out[name] = []
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name and line:
            out[name].append(line)
    names = re.findall(r"^\s*\.amdhsa_kernel (\w+)$", open(path).read(), re.M)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {p.rsplit("(", 1)[0]: out[k] for k, p in zip(names, plain)}


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
removed, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
changed = sorted(k for k in set(old) & set(new) if old[k] != new[k])
print(f"{len(old)} -> {len(new)} kernels\nremoved: {removed}\nadded:   {added}\nchanged: {changed}")
sys.exit(1 if added else 0)
