#!/usr/bin/env python3
"""Are the kernels of two builds the same machine code?  (CPU only; next to isa_kernel_info.py)

    make -C topsy_amd/csrc EXTRA=--save-temps        # in both trees: leaves <unit>-hip-amdgcn-amd-amdhsa-gfx950.s beside the sources
    tools/isa_diff.py <dir A> <dir B>

Reads every *-hip-amdgcn-amd-amdhsa-gfx950.s of both directories and compares, per kernel symbol, whichever unit holds it:
the instruction stream from the symbol's label to its .Lfunc_end (comments and assembler directives dropped, the function
number in the .LBB<n>_ labels renumbered to 0), and the resource fields of its .amdhsa_kernel descriptor.  Exit status 1,
with the names, when the two sets of kernels differ or a kernel differs in either respect."""
import glob
import hashlib
import os
import re
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(directory):
    """{kernel symbol: {(hash of its instruction stream, lines, descriptor fields)}} over every device assembly file of `directory`"""
    out = {}
    files = sorted(glob.glob(os.path.join(directory, "*-hip-amdgcn-amd-amdhsa-gfx950.s")))
    if not files:
        sys.exit(f"isa_diff: no *-hip-amdgcn-amd-amdhsa-gfx950.s in {directory}")
    for path in files:
        text = open(path).read()
        desc = {}
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
            desc[m.group(1)] = tuple(" ".join(re.findall(r"\.amdhsa_%s\s+(\S+)" % f, m.group(2))) for f in FIELDS)
        for name in desc:
            m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.S | re.M)
            if not m:
                sys.exit(f"isa_diff: {name} has a descriptor but no body in {path}")
            lines = []
            for line in m.group(0).split("\n")[1:-1]:
                line = line.split(";")[0].strip()
                if not line or (line.startswith(".") and not line.endswith(":")):      # (directives go, labels stay)
                    continue
                lines.append(re.sub(r"\.LBB\d+_", ".LBB0_", line))
            body = (hashlib.sha256("\n".join(lines).encode()).hexdigest(), len(lines), desc[name])
            out.setdefault(name, set()).add(body)      # (a library template is emitted by every unit that uses it: all its bodies)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(a) - set(b)):
        print(f"only in {sys.argv[1]}: {name}"); bad += 1
    for name in sorted(set(b) - set(a)):
        print(f"only in {sys.argv[2]}: {name}"); bad += 1
    for name in sorted(set(a) & set(b)):
        if {h for h, _, _ in a[name]} != {h for h, _, _ in b[name]}:
            print(f"instructions differ ({sorted(n for _, n, _ in a[name])} / {sorted(n for _, n, _ in b[name])} lines): {name}"); bad += 1
        if {d for _, _, d in a[name]} != {d for _, _, d in b[name]}:
            print(f"descriptor differs ({[dict(zip(FIELDS, d)) for _, _, d in a[name]]} / {[dict(zip(FIELDS, d)) for _, _, d in b[name]]}): {name}"); bad += 1
    print(f"{len(a)} / {len(b)} kernels, {len(set(a) & set(b))} in both, {bad} differences")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
