"""What the helper modules of the script-driven tests share (cw_common, fax_common, lorc_common, iqd_common, fftext_common; nbw_common,
nrs_common and spec_common for the first two): the digest the goldens keep instead of pools and outputs, the build of a host driver
tools/<name>.cpp (a csrc header compiled for the host with the reference's flags), the run of a command / block script through one,
and the cut of a script into the steps of a device run.  Pools, scripts, parsers and recorders stay with each decoder."""
import hashlib
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest(b):
    return hashlib.sha256(bytes(b)).digest()[:16]


def digest_u8(b):
    """the same as the uint8 vector an .npz keeps"""
    return np.frombuffer(digest(b), np.uint8)


def build_driver(tmpdir, name):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host driver"
    exe = os.path.join(str(tmpdir), name)
    subprocess.run([gxx, "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", name + ".cpp")], check=True)
    return exe


def run_script(exe, flags, lines, pool, dtype, tmpdir, expect=0):
    """exe flags... script pool out, with the pool written as `dtype` -> what the driver wrote (None where a refusal is expected)"""
    P = lambda f: os.path.join(str(tmpdir), f)
    open(P("s.txt"), "w").write("\n".join(lines) + "\n")
    np.ascontiguousarray(pool, dtype).tofile(P("pool.bin"))
    r = subprocess.run([exe] + flags + [P("s.txt"), P("pool.bin"), P("out.bin")])
    assert r.returncode == expect, (r.returncode, expect)
    return open(P("out.bin"), "rb").read() if expect == 0 else None


def script_steps(lines, cuts):
    """a script as a list of steps: ("cmd", line) or ("push", [pool offsets], [block numbers]) -- consecutive B lines, cut where `cuts`
    (a callable: blocks wanted next) says"""
    steps, seen, want = [], 0, None
    for l in lines:
        if l[0] == "B":
            off = int(l.split()[1])
            last = steps[-1] if steps else None
            if last and last[0] == "push" and len(last[1]) < want:
                last[1].append(off)
                last[2].append(seen)
            else:
                want = int(cuts())
                steps.append(("push", [off], [seen]))
            seen += 1
        else:
            steps.append(("cmd", l))
    return steps
