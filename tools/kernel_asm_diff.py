#!/usr/bin/env python3
"""Which kernels differ between two builds' device assembly (a refactor's proof that it left the kernels alone).  Either side may be several
files, for a source that was split or merged between the two commits:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o NAME.s vtc_amd/csrc/NAME.hip     # per source, on each commit
    tools/kernel_asm_diff.py old.s new.s
    tools/kernel_asm_diff.py old.s -- new1.s new2.s ...
    tools/kernel_asm_diff.py old1.s old2.s -- new1.s new2.s

Compared per kernel, instruction for instruction, after dropping `;` comments and the function number inside local labels
(.LBB12_7 -> .LBB_7), which shifts when a kernel is added, removed or moved.  Kernels are the `.amdhsa_kernel` symbols, matched by their
demangled name without the parameter list (c++filt), so a kernel that lost an argument shows as changed, not as removed + added.
Exit status 1 when a kernel was added, 2 when one side defines a kernel twice (each kernel belongs to exactly one source)."""
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


def side(paths, label):
    out, twice = {}, []
    for path in paths:
        for name, body in kernels(path).items():
            if name in out:
                twice.append(name)
            out[name] = body
    if twice:
        print(f"{label} side defines twice: {sorted(twice)}")
    return out, bool(twice)


args = sys.argv[1:]
if "--" in args:
    cut = args.index("--")
    old_paths, new_paths = args[:cut], args[cut + 1:]
else:
    old_paths, new_paths = args[:1], args[1:]
if not old_paths or not new_paths:
    sys.exit(__doc__)
(old, old_twice), (new, new_twice) = side(old_paths, "old"), side(new_paths, "new")
removed, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
changed = sorted(k for k in set(old) & set(new) if old[k] != new[k])
print(f"{len(old)} -> {len(new)} kernels\nremoved: {removed}\nadded:   {added}\nchanged: {changed}")
sys.exit(2 if old_twice or new_twice else 1 if added else 0)
