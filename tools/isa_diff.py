#!/usr/bin/env python3
"""Did a refactor change the machine code?  Compares, kernel by kernel, two assembly listings (hipcc -S --cuda-device-only):
the whole instruction stream with comments, directives and label numbers stripped, and the kernel descriptor's register,
LDS and scratch figures.  A kernel of the old listing is looked up in the new one under its own name after the --map
substitutions (regular expressions over the mangled name).  It complements spills.py, which looks inside one listing.

usage: isa_diff.py old.s new.s [--map REGEX=REPLACEMENT ...] [--show N] [--allow-new]
exit status 1 when a kernel differs or is missing on either side (with --allow-new: differs, or is missing in the new one)."""
import argparse, re, sys

FIGURES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    """{name: (instruction lines, {figure: value})} of the listing's kernels (the functions with an .amdhsa_kernel block)."""
    body, desc, fn = {}, {}, None
    for line in open(path):
        m = re.match(r"^(\w+):", line)
        if m and not line.startswith(".L"):
            fn = m.group(1)
            body[fn] = []
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\w+)", line)
        if m:
            fn, cur = None, desc.setdefault(m.group(1), {})
            continue
        m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", line)
        if m and m.group(1) in FIGURES:
            cur[m.group(1)] = m.group(2)
            continue
        text = line.split(";")[0].strip()
        if fn is None or not text or text.startswith("."):
            if text.startswith(".Lfunc_end"):
                fn = None
            continue
        body[fn].append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return {k: (body.get(k, []), d) for k, d in desc.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old"), ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPLACEMENT")
    ap.add_argument("--show", type=int, default=3, help="differing lines printed per kernel")
    ap.add_argument("--allow-new", action="store_true",
                    help="a kernel that only the new listing has is listed, not a failure (a feature adds instantiations)")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    same, seen, failed = 0, set(), False
    for name, (oi, od) in sorted(old.items()):
        to = name
        for rule in args.map:
            pat, rep = rule.split("=", 1)
            to = re.sub(pat, rep, to)
        if to not in new:
            print(f"MISSING {name} -> {to}")
            failed = True
            continue
        seen.add(to)
        ni, nd = new[to]
        if oi == ni and od == nd:
            same += 1
            continue
        failed = True
        print(f"DIFFERS {name} -> {to}: {len(oi)} / {len(ni)} instructions")
        print("   " + ", ".join(f"{f} {od.get(f)} / {nd.get(f)}" for f in FIGURES))
        shown = 0
        for n, (x, y) in enumerate(zip(oi, ni)):
            if x != y and shown < args.show:
                print(f"   [{n}] {x}   |   {y}")
                shown += 1
    for name in sorted(set(new) - seen):
        print(f"NEW {name}")
        failed = failed or not args.allow_new
    print(f"{same} of {len(old)} kernels identical")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
