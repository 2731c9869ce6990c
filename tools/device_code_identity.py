#!/usr/bin/env python3
"""Prove that a source-only change left the gfx950 device code untouched (no GPU needed).

    tools/device_code_identity.py <base-revision> [-o report.txt]

Compiles every csrc/kg_*.hip of <base-revision> (taken with git archive) and of the work
tree to device assembly with csrc/Makefile's own HIPFLAGS plus --cuda-device-only -S, and
compares the texts file by file.  Two normalisations only: lines with __hip_cuid_ (a hash
of the translation unit) are dropped, and acq_correlate_kernel's former mangled template
arguments <P, 1, true, STAMPS> are rewritten to <P, STAMPS>.  The .amdhsa_ blocks and the
metadata notes are part of the text, so register counts, LDS and scratch sizes and
kernel-argument offsets are covered.  Exit status 1 if any file differs."""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("flydog_sdr_gps_amd", "csrc")
OLD_ARGS = re.compile(r"(acq_correlate_kernelILi(?:4|16)E)Li1ELb1E(Lb[01]EE)")


def hipcc_and_flags(tree):
    """HIPCC and HIPFLAGS as that tree's Makefile expands them (the hidden-option probe included)."""
    return subprocess.check_output(
        ["make", "-s", "-C", os.path.join(tree, CSRC), "-f", "Makefile", "-f", "-", "ARCH=gfx950", "_flags"],
        input="_flags:\n\t@echo $(HIPCC) $(HIPFLAGS)\n", text=True).split()


def device_text(tree, src, out):
    r = subprocess.run([*hipcc_and_flags(tree), "--cuda-device-only", "-S", src, "-o", out],
                       cwd=os.path.join(tree, CSRC), stderr=subprocess.PIPE, text=True)
    # hipcc itself passes --hip-link, which -S leaves unused: not worth a line per file
    sys.stderr.write("".join(l for l in r.stderr.splitlines(True) if "'--hip-link'" not in l))
    r.check_returncode()
    with open(out) as f:
        return [OLD_ARGS.sub(r"\1\2", l) for l in f if "__hip_cuid_" not in l]


def count_kernels(text):
    return sum(l.lstrip().startswith(".amdhsa_kernel ") for l in text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("base")
    ap.add_argument("files", nargs="*", help="kg_*.hip names to compare (default: all)")
    ap.add_argument("-o", "--output")
    args = ap.parse_args()
    base = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", args.base], text=True).strip()
    names = args.files or sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, CSRC, "kg_*.hip")))
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "base")
        os.mkdir(old)
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", args.base, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", old], stdin=tar.stdout)
        jobs = [(t, n, os.path.join(tmp, "%s_%s.s" % (tag, n))) for n in names for tag, t in (("a", old), ("b", ROOT))]
        with concurrent.futures.ThreadPoolExecutor(8) as pool:
            texts = list(pool.map(lambda j: device_text(*j), jobs))
        hipcc, *flags = hipcc_and_flags(ROOT)
        version = [l for l in subprocess.check_output([hipcc, "--version"], text=True).splitlines() if "version" in l]
    lines = ["device code of the work tree against %s" % base, *version, "flags: " + " ".join(flags), ""]
    differ = 0
    for i, n in enumerate(names):
        a, b = texts[2 * i], texts[2 * i + 1]
        kernels = count_kernels(b)
        first = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        same = a == b
        differ += not same
        lines.append("%-16s %3d kernels  %6d lines  %s" % (
            n, kernels, len(b), "identical" if same else "DIFFERS from line %d (of %d)" % (first + 1, len(a))))
    lines.append("")
    lines.append("%d files, %d kernels: %s" % (
        len(names), sum(count_kernels(t) for t in texts[1::2]),
        "all identical" if not differ else "%d DIFFER" % differ))
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if args.output:
        with open(args.output, "w") as f:
            f.write(report)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
