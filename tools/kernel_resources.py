#!/usr/bin/env python
"""The compiler's resource report of the PCM-emitting kernels (everything that calls report_clipped), as one table.

    python tools/kernel_resources.py [--tree DIR] [--label TEXT] [--reports FILE ...] [--files NAME ...] [--match REGEX]

Compiles kernels_synth.hip and kernels.hip of DIR (default: this checkout) for gfx950 with the flags of nvorbis_amd/build.py plus
-Rpass-analysis=kernel-resource-usage, and prints per kernel: VGPRs, AGPRs, SGPRs, scratch bytes per lane, the occupancy the
compiler states (waves per SIMD), spilled SGPRs and VGPRs and static LDS bytes.  Needs hipcc, no GPU.  Two runs -- one on an export of the parent commit, one on
the checkout -- put side by side are profiles/segment_clipped_resources.txt.  --reports: the compiler's saved remarks (its
standard error) instead of compiling again.  --files / --match: other files of csrc/ and the kernels to list from them, e.g.
--files kernels_resample.hip --match k_resample_rows (profiles/resample_rows_resources.txt).
"""
import argparse
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("kernels_synth.hip", "kernels.hip")
# the kernels that end in report_clipped: the emitting synthesis families and the overlap-add kernels
EMITTING = re.compile(r"^(k_synth_emit|k_synth8_emit|k_synth_group[24]|k_ola_compact|k_ola_emit|k_ola_emit_seq|k_copy_buffer)")
FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"), ("LDS Size [bytes/block]", "lds"))


def demangle(names):
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-cxxfilt"] if os.path.exists("/opt/rocm/llvm/bin/llvm-cxxfilt") else ["c++filt"],
                         input="\n".join(names), capture_output=True, text=True)
    return out.stdout.splitlines() if out.returncode == 0 else names


def short(name):
    """k_ola_compact<float, 0>(NvhDevSetup, ...) -> k_ola_compact<float, 0>"""
    m = re.match(r"^(?:void )?([\w:]+(?:<[^()]*>)?)\(", name)
    return m.group(1) if m else name


def report(tree, reports=None, files=FILES, match=EMITTING):
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]
    rows = {}
    for f in reports or files:
        if reports:
            text = open(f).read()
        else:
          with tempfile.TemporaryDirectory() as tmp:
              cmd = ["hipcc"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c",
                                         os.path.join(tree, "nvorbis_amd", "csrc", f), "-o", os.path.join(tmp, "x.o")]
              text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        cur = None
        for line in text.splitlines():
            m = re.search(r"remark: .*Function Name: (\S+)", line)
            if m:
                cur = rows.setdefault(m.group(1), {})
                continue
            for label, key in FIELDS:
                m = re.search(r"remark: .*\s%s: (\d+)" % re.escape(label), line)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
    names = list(rows)
    nice = [short(n) for n in demangle(names)]
    return [(nn, rows[n]) for n, nn in zip(names, nice) if match.match(nn)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--reports", nargs="*")
    ap.add_argument("--files", nargs="*", default=list(FILES))
    ap.add_argument("--match", default=None)
    a = ap.parse_args()
    rows = report(os.path.abspath(a.tree), a.reports, a.files, re.compile(a.match) if a.match else EMITTING)
    print("# %s" % (a.label or a.tree))
    print("%-32s %5s %5s %5s %8s %4s %7s %7s %6s" % ("kernel", "VGPR", "AGPR", "SGPR", "scratch", "occ", "s-spill", "v-spill", "LDS"))
    for name, r in rows:
        print("%-32s %5d %5d %5d %8d %4d %7d %7d %6d" % (name, r.get("vgpr", -1), r.get("agpr", -1), r.get("sgpr", -1),
                                                         r.get("scratch", -1), r.get("occ", -1), r.get("sspill", -1),
                                                         r.get("vspill", -1), r.get("lds", -1)))


if __name__ == "__main__":
    main()
