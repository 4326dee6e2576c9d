#!/usr/bin/env python3
"""kernel_text.py: one line per kernel of `make asm`'s listings, to tell whether a change moved a kernel's code.

  tools/kernel_text.py ctstraffic_amd/build/*-gfx950.s > after.txt
  tools/kernel_text.py --compare before.txt after.txt

A line is: symbol, digest and line count of the kernel's normalised instruction text, then from its .amdhsa_
block group_segment_fixed_size (LDS bytes), private_segment_fixed_size (scratch bytes), next_free_vgpr and
next_free_sgpr. The text runs from the symbol's label to its .Lfunc_end; comments go, .LBB<n>_ labels lose the
function number n (it counts the functions before this one in the file), and the .p2align, .section, .type and
.size lines are dropped. Lines are sorted by symbol, so the listing does not depend on which file holds a kernel.
--compare prints the symbols whose lines differ or that only one listing has, and exits 1 if there are any.
"""
import hashlib
import re
import sys

FIELDS = ("group_segment_fixed_size", "private_segment_fixed_size", "next_free_vgpr", "next_free_sgpr")
DROPPED = (".p2align", ".section", ".type", ".size")


def normalise(lines):
    out = []
    for line in lines:
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";", 1)[0]).strip()
        if line and not line.startswith(DROPPED):
            out.append(line)
    return out


def kernels(path):
    """{symbol: listing line} of one assembly file."""
    lines = open(path).read().splitlines()
    labels = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"([A-Za-z_][\w$.]*):", l))}
    found = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        sym = m.group(1)
        meta = {}
        for d in lines[i + 1:]:
            if d.strip() == ".end_amdhsa_kernel":
                break
            f = d.split()
            if len(f) == 2 and f[0].startswith(".amdhsa_") and f[0][8:] in FIELDS:
                meta[f[0][8:]] = f[1]
        start = labels[sym]
        end = next(k for k in range(start, len(lines)) if lines[k].startswith(".Lfunc_end"))
        text = normalise(lines[start + 1:end])
        digest = hashlib.sha256("\n".join(text).encode()).hexdigest()[:16]
        found[sym] = " ".join([sym, digest, str(len(text))] + [meta[f] for f in FIELDS])
    return found


def read_listing(path):
    return {l.split()[0]: l.strip() for l in open(path) if l.strip() and not l.startswith("#")}


def main(argv):
    if len(argv) == 4 and argv[1] == "--compare":
        a, b = read_listing(argv[2]), read_listing(argv[3])
        differ = [s for s in sorted(set(a) | set(b)) if a.get(s) != b.get(s)]
        for s in differ:
            print("<", a.get(s, s + " (absent)"))
            print(">", b.get(s, s + " (absent)"))
        print(f"{len(a)} and {len(b)} kernels, {len(differ)} differ")
        return 1 if differ else 0
    if len(argv) < 2 or argv[1].startswith("-"):
        print(__doc__, file=sys.stderr)
        return 2
    found = {}
    for path in argv[1:]:
        found.update(kernels(path))
    print("# symbol digest lines " + " ".join(FIELDS))
    for s in sorted(found):
        print(found[s])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
