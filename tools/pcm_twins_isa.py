#!/usr/bin/env python3
"""Per-kernel comparison of two device-assembly listings of the same .hip file (hipcc ... --cuda-device-only -S):

    pcm_twins_isa.py OLD.s NEW.s [OLD2.s NEW2.s ...] [--diffs DIR]

Kernels are matched by slot name: a template instantiation `k_ola_compact<short, true>(...)` is the kernel that used to be
`k_ola_compact_s16_planar` (tools/rocprof_summary.py: slot_name, the mapping the trace summaries use).  Per kernel: the
resource fields of the code object's metadata and kernel descriptor (registers, spills, scratch, static LDS, everything that
decides occupancy) and the instruction stream with symbol names, labels and comments removed.  Prints one table line per kernel;
--diffs DIR keeps a unified diff for every kernel whose instructions differ.  Exit status 1 if a resource field differs."""
import difflib
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rocprof_summary import slot_name  # noqa: E402


def demangle(names):
    out = subprocess.run(["c++filt"] + list(names), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    return dict(zip(names, out))


META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size",
        ".uses_dynamic_stack")
# .amdhsa_ lines that carry nothing but the kernel's name are not among the descriptor fields (they have no value)


def parse(path):
    """-> {slot name: (symbol, {field: value}, [instruction lines])}"""
    text = open(path).read()
    lines = text.split("\n")
    syms = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    names = demangle(syms)
    kernels = {}
    for sym in syms:
        start = lines.index(next(l for l in lines if l.startswith(sym + ":")))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(("\t.section\t.rodata", ".Lfunc_end")))
        body = []
        for l in lines[start + 1:end]:
            l = l.split(";")[0].rstrip()
            if not l.strip() or re.match(r"^\.LBB\d+_\d+:", l) or l.strip().startswith((".p2align", ".cfi", "; ")):
                continue
            l = re.sub(r"\.LBB\d+_\d+", ".LBB", l)      # branch targets: the label numbering carries the function's index
            l = l.replace(sym, "KERNEL")
            l = re.sub(r"\b_Z\w+", "SYM", l)            # function-local statics (LDS arrays) carry the kernel's mangled name
            l = re.sub(r"\bk_\w+\.\w+", "SYM", l)
            body.append(l.strip())
        fields = {}
        k = lines.index("\t.amdhsa_kernel " + sym)
        while not lines[k].strip().startswith(".end_amdhsa_kernel"):
            m = re.match(r"\s*(\.amdhsa_\w+)\s+(\S+)", lines[k])
            if m and m.group(1) != ".amdhsa_kernel":
                fields[m.group(1)] = m.group(2)
            k += 1
        kernels[slot_name(names[sym])] = [names[sym], fields, body]
    # the metadata note: one YAML map per kernel
    for blk in re.split(r"\n  - \.agpr_count:", text[text.index("amdhsa.kernels:"):])[1:]:
        blk = "  - .agpr_count:" + blk
        sym = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
        f = kernels[slot_name(names[sym])][1]
        for key in META:
            m = re.search(r"^\s+(?:- )?" + re.escape(key) + r":\s+(\S+)", blk, re.M)
            if m:
                f[key] = m.group(1)
    return kernels


def main():
    args = sys.argv[1:]
    diffs = None
    if "--diffs" in args:
        i = args.index("--diffs")
        diffs = args[i + 1]
        del args[i:i + 2]
        os.makedirs(diffs, exist_ok=True)
    bad = 0
    print("%-28s %-34s %5s %5s %6s %8s %6s %8s  %s" % ("old name", "new name", "vgpr", "sgpr", "vspill", "scratch", "lds", "kernarg",
                                                     "resources / instructions (old -> new count)"))
    for old_path, new_path in zip(args[0::2], args[1::2]):
        old, new = parse(old_path), parse(new_path)
        for k in old:
            if k not in new:
                print("%-28s MISSING in %s" % (k, new_path))
                bad = 1
                continue
            (oname, of, ob), (nname, nf, nb) = old[k], new[k]
            res = sorted(f for f in set(of) | set(nf) if of.get(f) != nf.get(f))
            hard = [f for f in res if f not in (".kernarg_segment_size",)]
            if ob == nb:
                verdict = "identical (%d)" % len(ob)
            else:
                same_set = sorted(ob) == sorted(nb)
                same_ops = sorted(l.split()[0] for l in ob) == sorted(l.split()[0] for l in nb)
                d = list(difflib.unified_diff(ob, nb, "old/" + k, "new/" + k, lineterm="", n=2))
                changed = sum(1 for l in d if l[:1] in "+-" and l[:3] not in ("+++", "---"))
                verdict = "%s: %d -> %d, %d diff lines" % ("reordered, same instructions" if same_set else "same opcodes, registers / order differ" if same_ops else "DIFFERENT", len(ob), len(nb), changed)
                if diffs:
                    open(os.path.join(diffs, k + ".diff"), "w").write("\n".join(d) + "\n")
            rtxt = "same" if not res else ", ".join("%s %s -> %s" % (f, of.get(f), nf.get(f)) for f in res)
            if hard:
                bad = 1
            print("%-28s %-34s %5s %5s %6s %8s %6s %8s  %s / %s" % (
                re.sub(r"^void ", "", oname.split("(")[0]), re.sub(r"^void ", "", nname.split("(")[0]), nf.get(".vgpr_count"), nf.get(".sgpr_count"), nf.get(".vgpr_spill_count"),
                nf.get(".private_segment_fixed_size"), nf.get(".group_segment_fixed_size"), nf.get(".kernarg_segment_size"), rtxt, verdict))
        for k in new:
            if k not in old:  # a kernel the old listing does not have: its own figures
                nname, nf, nb = new[k]
                print("%-28s %-34s %5s %5s %6s %8s %6s %8s  NEW in %s (%d)" % (
                    "-", k, nf.get(".vgpr_count"), nf.get(".sgpr_count"), nf.get(".vgpr_spill_count"),
                    nf.get(".private_segment_fixed_size"), nf.get(".group_segment_fixed_size"), nf.get(".kernarg_segment_size"),
                    os.path.basename(new_path), len(nb)))
    return bad


if __name__ == "__main__":
    sys.exit(main())
