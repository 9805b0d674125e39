#!/usr/bin/env python3
"""Instruction order of a kernel's MFMA loop, read from the assembly `make asm-<name>` writes.

  tools/isa_loop_mix.py 3d_reconstruction_amd/csrc/match_fp6.s match_fp6_kernelILi256Es

The loop is the innermost backward branch whose body holds the most MFMAs (the block loop of the match
kernels).  Printed: the body's opcodes as run lengths in program order, and
  - the longest run of MFMAs,
  - the longest run of vector instructions that are not MFMAs (scalar instructions and waits neither
    count nor break a run), with and without the stretch between the loop's first and last MFMA
    (the block seam: barrier, DMA issue, first reads),
  - the smallest number of instructions between an MFMA and the first reader of its destination, and
    the s_nop count between such a pair,
then the kernel's register, scratch and LDS figures.  CPU only.
"""
import re
import sys


def kernel_text(lines, needle):
    names = [m.group(1) for l in lines if (m := re.match(r"^(\w+):\s*;\s*@", l)) and needle in m.group(1)]
    if not names:
        sys.exit(f"no kernel matching {needle!r}")
    name = names[0]
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return name, lines[start + 1:end]


def parse(body):
    """-> [(label | None, opcode, operands)]"""
    out = []
    for l in body:
        l = l.split(";")[0].rstrip()
        if not l:
            continue
        if re.match(r"^\.?\w+:$", l.strip()):
            out.append((l.strip()[:-1], None, None))
            continue
        if not l.startswith("\t") or l.strip().startswith("."):
            continue
        parts = l.strip().split(None, 1)
        out.append((None, parts[0], parts[1] if len(parts) > 1 else ""))
    return out


def regs(operand):
    """registers an operand names: v12 -> {12}, v[4:7] -> {4..7}; others -> {}"""
    operand = operand.strip()
    if m := re.match(r"^v\[(\d+):(\d+)\]$", operand):
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    if m := re.match(r"^v(\d+)$", operand):
        return {int(m.group(1))}
    return set()


def split_ops(s):
    return [o for o in re.split(r",\s*(?![^\[]*\])", s) if o]


def find_loop(ins):
    labels = {lab: i for i, (lab, op, _) in enumerate(ins) if lab}
    best = None
    for i, (lab, op, args) in enumerate(ins):
        if op and op.startswith("s_cbranch") or op == "s_branch":
            tgt = args.strip()
            if tgt in labels and labels[tgt] < i:
                n = sum(1 for _, o, _ in ins[labels[tgt]:i] if o and o.startswith("v_mfma"))
                span = i - labels[tgt]
                if n and (best is None or n > best[0] or (n == best[0] and span < best[1])):
                    best = (n, span, labels[tgt], i)
    if best is None:
        sys.exit("no loop with MFMAs")
    return [x for x in ins[best[2]:best[3] + 1] if x[1]]


def is_vector(op):
    return op.startswith(("v_", "ds_", "global_", "buffer_", "flat_"))


def report(path, needle):
    lines = open(path).read().splitlines()
    name, body = kernel_text(lines, needle)
    loop = find_loop(parse(body))
    ops = [op for _, op, _ in loop]
    short = [("v_mfma" if o.startswith("v_mfma") else o) for o in ops]
    print(f"kernel {name}")
    print(f"loop body: {len(ops)} instructions, {short.count('v_mfma')} MFMAs, "
          f"{sum(1 for o in short if o.startswith('v_') and o != 'v_mfma')} other VALU, "
          f"{sum(1 for o in short if o.startswith('ds_'))} LDS, {short.count('s_nop')} s_nop, "
          f"{short.count('s_waitcnt')} s_waitcnt")
    runs = []
    for o in short:
        if runs and runs[-1][0] == o:
            runs[-1][1] += 1
        else:
            runs.append([o, 1])
    text = ", ".join(f"{o} x{n}" for o, n in runs)
    print("sequence: " + text)

    mf = [i for i, o in enumerate(short) if o == "v_mfma"]
    longest_mfma = max(n for o, n in runs if o == "v_mfma")

    def longest_vec(seq, valu_only=False):
        best = cur = 0
        for o in seq:
            if o == "v_mfma":
                cur = 0
            elif o.startswith("v_") if valu_only else is_vector(o):
                cur += 1
                best = max(best, cur)
        return best
    inner = short[mf[0]:mf[-1] + 1]
    print(f"longest run of MFMAs: {longest_mfma}")
    print(f"longest run of non-MFMA vector instructions: {longest_vec(inner)} between the loop's first and last MFMA "
          f"({longest_vec(inner, True)} counting VALU only, the LDS reads of a k-step apart), "
          f"{longest_vec(short + short)} with the block seam")
    # distance from an MFMA to the first reader of its destination (the loop wraps once)
    two = loop + loop
    dist, nops_between = None, 0
    for i in mf:
        dst = regs(split_ops(loop[i][2])[0])
        for j in range(i + 1, i + len(loop)):
            _, op, args = two[j]
            o = split_ops(args)
            srcs = o[1:] if (is_vector(op) and not op.startswith(("ds_write", "global_store"))) else o
            if any(regs(x) & dst for x in srcs):
                d = j - i - 1
                if dist is None or d < dist:
                    dist = d
                if not op.startswith("v_mfma"):
                    nops_between += sum(1 for _, q, _ in two[i + 1:j] if q == "s_nop") if d <= 4 else 0
                break
            if is_vector(op) and o and regs(o[0]) & dst:
                break   # overwritten unread
    print(f"smallest distance MFMA -> first reader of its destination: {dist} instructions; "
          f"s_nop between an MFMA and a reader within 4 instructions: {nops_between}")
    meta = "\n".join(lines)
    for key in ("num_vgpr", "num_agpr", "private_seg_size"):
        if m := re.search(rf"\.set {re.escape(name)}\.{key}, (\S+)", meta):
            print(f"{key}: {m.group(1)}")
    if m := re.search(rf"\.amdhsa_kernel {re.escape(name)}\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        for key in ("amdhsa_group_segment_fixed_size", "amdhsa_next_free_vgpr", "amdhsa_accum_offset"):
            if k := re.search(rf"\.{key} (\S+)", m.group(1)):
                print(f"{key}: {k.group(1)}")
    if m := re.search(rf"; Occupancy: (\d+)", "\n".join(body) + meta[meta.find(name + ":"):][:400000]):
        print(f"occupancy (waves per SIMD): {m.group(1)}")


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    report(sys.argv[1], sys.argv[2])
