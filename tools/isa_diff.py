#!/usr/bin/env python3
"""Compare two device assembly listings kernel by kernel (hipcc ... --cuda-device-only -S).

    tools/isa_diff.py PARENT.s CHANGE.s [CHANGE2.s ...] [--only SUBSTRING]

The kernels of the first file are looked up in the others (a change may have spread them over several files).  Per kernel one line:
registers, scratch and LDS as parent -> change, whether the whole .amdhsa_* descriptor block is equal, the instruction count, the
number of lines that differ, and how many of those differ only in the order of their source operands (same mnemonic, same
destination, same operands: the reader checks that the mnemonics listed at the end are commutative).  Comments are stripped and the
per-function numbers of .LBB<n>_ / .Lfunc_end<n> labels normalised.  Exit status 1 if a descriptor or any other line differs.
"""
import difflib
import re
import subprocess
import sys


def kernels(path):
    """symbol -> (descriptor lines, body lines)"""
    text = open(path).read().split("\n")
    desc, body, cur, sym = {}, {}, None, None
    for raw in text:
        line = re.sub(r"\s+", " ", raw.split(";")[0]).strip()
        if not line:
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
        m = re.match(r"\.amdhsa_kernel (\S+)$", line)
        if m:
            cur = desc.setdefault(m.group(1), [])
        elif line == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None:
            cur.append(line)
        m = re.match(r"\.type (\S+),@function$", line)
        if m:
            sym = m.group(1)
            body[sym] = []
        elif sym is not None:
            if line.startswith(".Lfunc_end"):
                sym = None
            elif line != sym + ":":
                body[sym].append(line)
    return {s: (desc[s], body[s]) for s in desc}


def field(desc, name):
    for line in desc:
        if line.startswith(".amdhsa_" + name + " "):
            return line.split(" ", 1)[1]
    return "?"


def swapped(a, b):
    """the same instruction with its source operands in another order?"""
    ma, _, oa = a.partition(" ")
    mb, _, ob = b.partition(" ")
    oa, ob = [o.strip() for o in oa.split(",")], [o.strip() for o in ob.split(",")]
    return ma == mb and len(oa) > 2 and oa[0] == ob[0] and sorted(oa[1:]) == sorted(ob[1:])


def main():
    args = sys.argv[1:]
    only = None
    if "--only" in args:
        k = args.index("--only")
        only = args[k + 1]
        del args[k:k + 2]
    parent = kernels(args[0])
    change = {}
    for p in args[1:]:
        change.update(kernels(p))
    names = subprocess.run(["c++filt"] + list(parent), capture_output=True, text=True).stdout.split("\n")
    bad, mnemonics = 0, set()
    print("kernel | vgpr | sgpr | scratch | lds | descriptor | instructions | differing lines | of those, operands swapped")
    for sym, name in sorted(zip(parent, names), key=lambda t: t[1]):
        if only and only not in name:
            continue
        name = re.sub(r"^void clvr::|\(.*$", "", name)
        if sym not in change:
            print(f"{name} | MISSING")
            bad += 1
            continue
        (pd, pb), (cd, cb) = parent[sym], change[sym]
        differ = swaps = 0
        for op, i1, i2, j1, j2 in difflib.SequenceMatcher(None, pb, cb, autojunk=False).get_opcodes():
            if op == "equal":
                continue
            differ += max(i2 - i1, j2 - j1)
            if op == "replace" and i2 - i1 == j2 - j1:
                for a, b in zip(pb[i1:i2], cb[j1:j2]):
                    if swapped(a, b):
                        swaps += 1
                        mnemonics.add(a.split(" ")[0])
        cols = [f"{field(pd, f)} -> {field(cd, f)}" for f in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")]
        insts = sum(1 for line in cb if not line.startswith(".") and not line.endswith(":"))
        print(f"{name} | " + " | ".join(cols) + f" | {'equal' if pd == cd else 'DIFFERS'} | {insts} | {differ} | {swaps}")
        bad += pd != cd or differ != swaps
    print(f"{bad} kernels differ beyond swapped source operands; mnemonics of the swapped lines: {' '.join(sorted(mnemonics)) or 'none'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
