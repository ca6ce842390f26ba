"""Instruction mix of one loop of a kernel in a hipcc -S listing, counted by basic-block membership (no GPU needed).

  python scripts/isa_loop_blocks.py d14.s ilq_lq_kernelIdLi14ELi3ELi2ELi1ELi2E BB62_865

scripts/isa_loops.py counts the instructions between a loop's label and its last backward branch.  The compiler lays some
blocks of a loop out after that branch (cold sides of divergent regions) and moves them back in when the code around them
changes, so two builds of the same loop can differ by a dozen instructions there that no wave executes differently.  This
script counts every block the listing annotates as `in Loop: Header=<HEADER>` (inner loops: `Parent Loop <HEADER>`),
wherever it lies.  HEADER is the `Header=` name in the listing's block comments: the loop header's label without `.L`."""
import re
import sys

from isa_loops import classify


def main():
    path, pat, header = sys.argv[1], sys.argv[2], sys.argv[3]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and pat in l and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    inside = False
    mix = {}
    for i in range(start, end + 1):
        s = lines[i].strip()
        m = re.match(r"^(\.LBB[0-9_]+):(.*)$", s) or re.match(r"^; (%bb\.[0-9]+):(.*)$", s)
        if m:
            rest = m.group(2) + " "
            inside = ("Header=%s " % header in rest or "Parent Loop %s " % header in rest or
                      ("Loop Header" in rest and m.group(1) == ".L" + header))
            continue
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        if inside:
            c = classify(s.split()[0])
            mix[c] = mix.get(c, 0) + 1
    print("loop %s by block membership: %d instrs %s" % (header, sum(mix.values()), dict(sorted(mix.items()))))


if __name__ == "__main__":
    main()
