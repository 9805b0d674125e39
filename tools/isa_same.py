"""Pair the kernels of two sets of device assembly files (`make asm-<unit>`) and compare their text.

  tools/isa_same.py OLD.s [OLD2.s ...] -- NEW.s [NEW2.s ...] [--table FILE]

FILE pairs renamed kernels, one `OLD_SYMBOL NEW_SYMBOL` per line, `OLD_SYMBOL -` for a kernel dropped on
purpose (profiles/match_split/renames.txt is the table of the match.hip split).

For every kernel of the old files (a `.amdhsa_kernel` block names one) the function text from its label to
its `.Lfunc_end` marker is compared with the same symbol's text in the new files: the body and, apart, the
`.amdhsa_*` descriptor block (registers, LDS, scratch, ...).  Assembler comments and the section switches
around the descriptor (`.section`, `.text`: a template instance has a comdat group, a plain function has
none) are stripped, the per-file
numbering of local labels (.LBB<n>_, .Ltmp<n>, .LJTI<n>_, .Lfunc_end<n>) is normalised, and a renamed kernel's
old symbol is read as its new one.  Prints one line per old kernel, `SAME <unit> <symbol>` or
`DIFF ...` / `MISSING ...`, then a summary; exit status 1 unless every kernel that was not dropped on
purpose is SAME.  It only pairs and compares text: it knows nothing about instructions."""
import os
import re
import sys


def kernels(path):
    """-> {symbol: (body lines, descriptor lines)}"""
    lines = open(path).read().split("\n")
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        body, desc, in_desc = [], [], False
        for ln in lines[start:end]:
            ln = ln.split(";")[0].rstrip()
            if not ln.strip() or ln.split()[0] in (".section", ".text"):   # section switches: a template's
                continue                                                   # instance sits in a comdat group
            if ln.strip().startswith(".amdhsa_kernel "):
                in_desc = True
            (desc if in_desc else body).append(ln.strip())
            if ln.strip() == ".end_amdhsa_kernel":
                in_desc = False
        out[name] = (body, desc)
    return out


def normalise(lines, rename):
    text = "\n".join(lines)
    for old, new in rename.items():
        text = text.replace(old, new)
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.LJTI\d+_", ".LJTI_", text)
    text = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", text)
    order = {}
    return re.sub(r"\.Ltmp(\d+)", lambda m: ".Ltmp_%d" % order.setdefault(m.group(1), len(order)), text)


def main(argv):
    split = argv.index("--")
    old_files = argv[:split]
    rest = argv[split + 1:]
    new_files = [a for a in rest if a.endswith(".s")]
    rename, dropped = {}, set()
    if "--table" in rest:
        for ln in open(rest[rest.index("--table") + 1]):
            if ln.strip() and not ln.startswith("#"):
                o, n = ln.split()
                if n == "-":
                    dropped.add(o)
                else:
                    rename[o] = n
    old = {}
    for f in old_files:
        old.update(kernels(f))
    new = {}
    for f in new_files:
        unit = os.path.splitext(os.path.basename(f))[0]
        for name, k in kernels(f).items():
            new[name] = (unit, k)
    bad = 0
    for name in sorted(old):
        if name in dropped:
            print("DROPPED", "-", name)
            bad += name in new
            continue
        target = rename.get(name, name)
        if target not in new:
            print("MISSING", "-", name)
            bad += 1
            continue
        unit, (nbody, ndesc) = new[target]
        obody, odesc = old[name]
        parts = [p for p, a, b in (("body", obody, nbody), ("descriptor", odesc, ndesc))
                 if normalise(a, rename) != normalise(b, {})]
        note = "" if target == name else "  (was " + name + ")"
        if parts:
            print("DIFF", unit, target, "+".join(parts) + note)
            bad += 1
        else:
            print("SAME", unit, target + note)
    extra = sorted(set(new) - {rename.get(n, n) for n in old})
    for name in extra:
        print("NEW", new[name][0], name)
    print("# %d old kernels, %d dropped, %d new-only, %d not the same" % (len(old), len(dropped), len(extra), bad + len(extra)))
    return 1 if bad or extra else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
