#!/usr/bin/env python3
"""Compare the gfx950 kernels of two `make asm` outputs (langsplatv2_amd/_build/asm).

    python tools/kernel_diff.py DIR_A DIR_B

For every kernel symbol (whichever .s file of the directory holds it) the
instruction text and the .amdhsa_* descriptor block must be equal.  Local
labels carry the function's index within its translation unit (.LBB12_3), so
the index is dropped before comparing, as are `;` comments.  Prints the symbols
on one side only, the symbols that differ and the number that match; exits 0
only if both sets are equal, no symbol is defined twice and every kernel matches.
"""
import glob
import os
import re
import sys

_LABEL = re.compile(r"\.L([A-Za-z_]+)\d+_")


def kernels(asm_dir):
    """{symbol: (instruction lines, descriptor lines)} over DIR/*.s, and the symbols defined more than once."""
    out, twice = {}, []
    for path in sorted(glob.glob(os.path.join(asm_dir, "*.s"))):
        lines = [_LABEL.sub(r".L\1_", ln.split(";")[0].rstrip()) for ln in open(path)]
        start = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":") and not ln.startswith(("\t", " ", "."))}
        for i, ln in enumerate(lines):
            if not ln.startswith("\t.amdhsa_kernel "):
                continue
            sym = ln.split()[1]
            end = lines.index("\t.end_amdhsa_kernel", i)
            if sym in out:
                twice.append(sym)
            out[sym] = ([x for x in lines[start[sym]:i] if x.strip()], lines[i:end])
    return out, twice


def compare(dir_a, dir_b):
    """(only in a, only in b, differing, matching, defined twice): sorted symbol lists."""
    (a, ta), (b, tb) = kernels(dir_a), kernels(dir_b)
    both = sorted(set(a) & set(b))
    differ = [s for s in both if a[s] != b[s]]
    return sorted(set(a) - set(b)), sorted(set(b) - set(a)), differ, [s for s in both if a[s] == b[s]], sorted(ta + tb)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    only_a, only_b, differ, same, twice = compare(sys.argv[1], sys.argv[2])
    for title, syms in (("only in " + sys.argv[1], only_a), ("only in " + sys.argv[2], only_b),
                        ("differ", differ), ("defined twice", twice)):
        for s in syms:
            print(f"{title}: {s}")
    print(f"kernel_diff: {len(same)} match, {len(differ)} differ, {len(only_a)} only in A, {len(only_b)} only in B, "
          f"{len(twice)} defined twice")
    sys.exit(1 if only_a or only_b or differ or twice else 0)


if __name__ == "__main__":
    main()
