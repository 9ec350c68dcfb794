#!/usr/bin/env python
"""Are two gfx950 device listings of one .hip file the same code?

    hipcc --offload-arch=gfx950 <the flags of _build.py> --cuda-device-only -S csrc/kernels/X.hip -o X.s
    python tools/device_listing_cmp.py OLD/X.s NEW/X.s

A host-side change that instantiates the same kernels in another order moves whole functions in the listing and
renumbers their local labels (``.LBB<n>_<k>``, ``.Lfunc_end<n>``: n is the function's ordinal in the file), which a
plain ``diff`` reports as a change in every function.  This compares the listings as multisets of sections and
metadata entries with that ordinal, the file / ident lines and the per-compilation ``__hip_cuid_`` symbol taken
out.  Exit status 0: the same functions, instruction for instruction, and the same kernel descriptors.
"""
import re
import sys

SKIP = re.compile(r"\.file|\.ident|__hip_cuid_")
ORDINAL = re.compile(r"(LBB|BB|Lfunc_begin|Lfunc_end)\d+")  # labels, and the comments that name them
PAD = re.compile(r" +;")  # comments are padded to a column, so a shorter label moves them
STARTS = ("\t.section", "\t.text", "  - .agpr_count", "  - .args", "amdhsa.")


def chunks(path):
    out, cur = [], []
    with open(path) as f:
        for line in f:
            if SKIP.search(line):
                continue
            if line.startswith(STARTS):
                out.append("".join(cur))
                cur = []
            cur.append(PAD.sub(" ;", ORDINAL.sub(r"\1", line)))
    out.append("".join(cur))
    return sorted(out)


def main():
    a, b = chunks(sys.argv[1]), chunks(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    print(f"{len(a)} / {len(b)} sections and metadata entries, {len(only_a)} / {len(only_b)} without a twin")
    for name, rest in (("old", only_a), ("new", only_b)):
        for c in rest[:5]:
            print(f"only in the {name} listing: {c.splitlines()[0][:160]}")
    return 0 if a == b else 1


if __name__ == "__main__":
    sys.exit(main())
