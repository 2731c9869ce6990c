#!/usr/bin/env python3
"""Record tests/golden/rxbank_fingerprint.npz: the whole-step fingerprint of the receiver bank (tests/rxbank_fingerprint.py) from the
library that KIWIGPU_LIBRARY names -- the build of the commit the fixture is to pin, made in a worktree of it:

    git worktree add /tmp/base <revision> && make -C /tmp/base/flydog_sdr_gps_amd/csrc ARCH=gfx950
    KIWIGPU_LIBRARY=/tmp/base/flydog_sdr_gps_amd/libkiwigpu.so python tools/make_rxbank_fingerprint_golden.py [-o file.npz]

Needs a GPU.  The scenario runs twice: the integers must agree; a buffer whose digest differs between the two runs is left out of the
fixture and named on stdout (s16, adpcm and wf_pkts may not be: that is an error).  The scenario's own preconditions are asserted."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import rxbank_fingerprint as fp                               # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "tests", "golden", "rxbank_fingerprint.npz"))
    args = ap.parse_args()
    from flydog_sdr_gps_amd._lib import library_path
    print("library: %s" % library_path())
    a, b = fp.run(), fp.run()
    fp.check_preconditions(a)
    keep = []
    for k in sorted(a):
        same = np.array_equal(a[k], b[k])
        if k.startswith("digest_"):
            name = k[len("digest_"):]
            if same:
                keep.append(name)
            else:
                assert name not in fp.MUST_HOLD, "%s differs between two runs of one library" % name
                print("left out: %s differs between two runs on steps %s" % (name, np.flatnonzero(a[k] != b[k]).tolist()))
        else:
            assert same, "%s differs between two runs of one library" % k
    out = {k: v for k, v in a.items() if not k.startswith("digest_") or k[len("digest_"):] in keep}
    out["buffers"] = np.array(keep)
    np.savez_compressed(args.output, **out)
    info = a["info"]
    print("recorded %d steps, buffers %s, nmoves on steps %s, table_bytes %d .. %d -> %s" % (
        fp.STEPS, keep, np.flatnonzero(info[:, fp.INFO_FIELDS.index("nmoves")]).tolist(),
        info[:, fp.INFO_FIELDS.index("table_bytes")].min(), info[:, fp.INFO_FIELDS.index("table_bytes")].max(), args.output))
    return 0


if __name__ == "__main__":
    sys.exit(main())
