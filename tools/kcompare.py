#!/usr/bin/env python3
"""Parent against change, per kernel, from two hipcc -S device assembly files of one source file: VGPRs, SGPRs,
scratch bytes (the .amdhsa_ metadata, as tools/kregs.py) and the instruction count of the kernel's text.

usage: python tools/kcompare.py parent.s change.s [pairs.txt]

A kernel of the change whose template arguments end in one or more `false` beyond the parent's (flags added with
that default) is compared with the parent's kernel; one whose added arguments hold a `true` is a new variant and is
listed against the parent's kernel of the other arguments (its twin).  A renamed kernel is paired by pairs.txt: lines of
"parent-name change-name" (mangled); such pairs are listed with both figures whether or not they differ.
"""
import re
import sys


def parse(path):
    """{mangled name: (vgpr, sgpr, scratch bytes, instructions)}"""
    regs, counts = {}, {}
    cur = label = None
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = m.group(1)
            regs[cur] = {}
            continue
        if cur:
            for key in ("private_segment_fixed_size", "next_free_vgpr", "next_free_sgpr"):
                m = re.match(rf"\s*\.amdhsa_{key}\s+(\d+)", line)
                if m:
                    regs[cur][key] = int(m.group(1))
            if re.match(r"\s*\.end_amdhsa_kernel", line):
                cur = None
            continue
        m = re.match(r"^(_Z\w+):", line)
        if m:
            label = m.group(1)
            counts[label] = 0
        elif re.match(r"^\.Lfunc_end", line):
            label = None
        elif label and re.match(r"^\s+[a-z][a-z0-9_]+\s", line) and not line.strip().startswith("."):
            counts[label] += 1
    return {k: (v.get("next_free_vgpr"), v.get("next_free_sgpr"), v.get("private_segment_fixed_size"), counts.get(k))
            for k, v in regs.items()}


def waves(vgpr):
    """waves per SIMD the VGPR count allows (512 per lane, allocated in eights)"""
    return min(8, 512 // ((vgpr + 7) // 8 * 8))


def twin(name, parent, told):
    """(the parent's name of this kernel, whether it is a new variant)"""
    if name in told:
        return told[name], False
    if name in parent:
        return name, False
    m = re.search(r"I((?:Lb[01]E)+)E", name)
    if m:
        args = m.group(1)
        for cut in range(4, len(args), 4):  # one flag added, or several
            base = name.replace(args, args[:-cut])
            if base in parent:
                return base, "Lb1E" in args[-cut:]
    return None, True


def main(a_path, b_path, pairs_path=None):
    a, b = parse(a_path), parse(b_path)
    told = dict(reversed(line.split()) for line in open(pairs_path) if line.strip()) if pairs_path else {}
    short = lambda k: re.sub(r"_ZN5hippt12_GLOBAL__N_1\d+", "", k)
    same, diff, new, paired = 0, [], [], []
    for k in sorted(b):
        p, variant = twin(k, a, told)
        if k in told:
            paired.append(f"  {short(p)} {a[p]} -> {short(k)} {b[k]}")
        if p is None:
            new.append(f"  {short(k)}: new {b[k]}")
        elif variant:
            note = "  [scratch above its twin]" if b[k][2] > a[p][2] else ""
            note += "  [an occupancy step below its twin]" if waves(b[k][0]) < waves(a[p][0]) else ""
            new.append(f"  {short(p)}: twin {a[p]} -> new variant {b[k]}{note}")
        elif a[p] == b[k]:
            same += 1
        else:
            diff.append(f"  {short(p)}: {a[p]} -> {b[k]}")
    print(f"{len(a)} kernels of the parent, {same} with identical figures, {len(diff)} that differ; {len(new)} new variants")
    print("\n".join(diff + (["new variants:"] + new if new else []) + (["told pairs:"] + paired if paired else [])))


if __name__ == "__main__":
    main(*sys.argv[1:4])
