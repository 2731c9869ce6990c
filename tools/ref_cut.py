"""What the tools/make_ref_*_golden.py share: reading a file of the reference tree ($REFERENCE, default /root/reference), cutting line
ranges of it into a temporary directory after checking each range's first and last line, checking a table of pinned statements, and
the main() of the extension makers whose golden is one record per script.  These tools run only where the reference tree is present;
the cuts live in the caller's temporary directory alone, and only data is kept.  Compile commands stay with each maker.

One tuple order: a cut is (file, name, first line, last line, text of the first, text of the last[, a line of ours ahead of the cut]),
a pin is (file, line, text)."""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = os.environ.get("REFERENCE", "/root/reference")
REF = os.path.join(ROOT, "oracle", "_ref")
_text = {}


def read(rel):
    if rel not in _text:
        _text[rel] = open(os.path.join(R, rel), encoding="latin-1").read().split("\n")
    return _text[rel]


def squeezed(t):
    return " ".join(t.split())


def cut(tmp, cuts, whole=False):
    """writes tmp/<name>.inc per cut; its first and last line hold the two texts -- as the whole stripped line where `whole`"""
    for rel, name, a, b, t1, t2, *ahead in cuts:
        lines = read(rel)
        first, last = lines[a - 1], lines[b - 1]
        ok = (first.strip() == t1 and last.strip() == t2) if whole else (t1 in first and t2 in last)
        assert ok, ("cut moved", rel, name, a, b, first, last)
        open(os.path.join(tmp, name + ".inc"), "w", encoding="latin-1").write("".join(l + "\n" for l in ahead if l) + "\n".join(lines[a - 1:b]) + "\n")


def pin(pins, white_space_aside=False):
    """every pinned text is part of its line -- with every run of white space as one blank where `white_space_aside`"""
    for rel, ln, t in pins:
        line = read(rel)[ln - 1]
        assert (squeezed(t) in squeezed(line)) if white_space_aside else (t in line), ("statement moved", rel, ln, t, line)


def cut_macros(cuts):
    """-D<name>="<name>.inc" per cut, for the harnesses that include their cuts by macro"""
    return ['-D%s="%s.inc"' % (c[1], c[1]) for c in cuts]


def script_by_digest(C, lines):
    return "script_sha", np.frombuffer(C.digest("\n".join(lines).encode()), np.uint8)


def script_by_text(C, lines):
    return "script", np.array(lines)


def script_golden_main(C, build, golden, script_entry, report, check=True):
    """tests/golden/<golden>: the pool's digest, the script names and, per script of C.scripts() run through build(tmp)'s harness,
    the script itself as script_entry keeps it (by digest or by text) and C.golden_of(); report(name, got, out, k) prints the
    maker's line about the script whose entries lie under the prefix k.  The golden's test states the file's conditions
    (golden_conditions): checked before the file is kept."""
    out = {}
    samples = C.pool()
    out["pool_sha"] = np.frombuffer(C.digest(samples.tobytes()), np.uint8)
    sc = C.scripts()
    out["script_names"] = np.array(sorted(sc))
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name in sorted(sc):
            got = C.run_script_exe(exe, sc[name], samples, tmp)
            k = "s_%s_" % name
            key, v = script_entry(C, sc[name])
            out[k + key] = v
            for key, v in C.golden_of(got).items():
                out[k + key] = v
            report(name, got, out, k)
        path = os.path.join(tmp, golden)
        np.savez_compressed(path, **out)
        if check:
            test = __import__("tests.test_%s_cpu" % golden.split("_")[0], fromlist=["golden_conditions"])
            test.golden_conditions(np.load(path), os.path.getsize(path))
        final = os.path.join(C.GOLD, golden)
        shutil.copyfile(path, final)
    print("wrote %s, %d bytes" % (final, os.path.getsize(final)))
